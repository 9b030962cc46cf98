"""GPU: the attention-pooling kernels of csrc/mil_pool.hip (pool_partial_kernel, pool_merge_kernel, pool_backward_kernel) held
to float64 at every chunk / merge edge, stage by stage: rrt_attn_pool_f32, rrt_pool_predict_f32 and rrt_attn_pool_backward_f32
called directly on the case lists of tests/mil_pool_cases.py (tests/test_mil_pool_cases_cpu.py proves on the CPU what the lists
cover), then the consumers at a bag above 32 768 tokens.

Every call writes into NaN-filled outputs with canary elements behind them, from a workspace of exactly the queried size, dirtied
with 0xFF, with canary bytes behind it.  Bounds (none of them new, mil_pool_cases.forward_errors / backward_errors):
  * forward: tests/test_clam_gpu.py::_check_fwd (pooled 2e-5, attn and raw scores 2e-5 * max(1, largest reference entry)), logits
    2e-5 * max(1, max |pooled_ref|) as tests/test_hip_parity.py::test_pool_predict, |sum attn - 1| < 1e-5; masked entries exactly
    0, tied and flat entries bit-equal;
  * backward: tests/test_clam_gpu.py::_grad_tol.
Beside every kernel error the table holds the error of the fp32 chunked CPU evaluation (mil_pool_ref.emulate32) on the same
inputs; RRT_MIL_POOL_ERRORS_OUT=<file> writes the table to that file (profiles/mil_pool_errors.txt is one such run)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mil_pool_cases as K
import mil_pool_ref as R
from rrt_mil_amd import _lib, synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda:0"
CANARY, CANARY_BYTE, TAIL = -777.25, 0xA5, 64
TABLE = []                      # (stage, case id, quantity, kernel error, emulation error, bound)


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    path = os.environ.get("RRT_MIL_POOL_ERRORS_OUT")
    if path and TABLE:
        with open(path, "w") as fh:
            fh.write("# csrc/mil_pool.hip against float64: max abs error of the kernel and of the fp32 chunked CPU evaluation\n")
            fh.write("# (tests/mil_pool_ref.py::emulate32) on the same inputs, and the bound (tests/test_mil_pool_matrix.py)\n")
            fh.write(f"# {'stage':9s} {'case':42s} {'quantity':8s} {'kernel':>10s} {'emulate32':>10s} {'bound':>10s}\n")
            for row in TABLE:
                fh.write("  {:9s} {:42s} {:8s} {:10.3e} {:10.3e} {:10.3e}\n".format(*row))


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """a device error is sticky: nothing more is started on a device that reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # pragma: no cover
        pytest.exit(f"device error, stopping the module: {e}", returncode=3)


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


def _guarded(n):
    """a NaN-filled [n] output at the front of a buffer whose last TAIL elements hold CANARY"""
    buf = torch.full((n + TAIL,), float("nan"), device=DEV)
    buf[n:] = CANARY
    return buf


def _intact(buf, n):
    return bool((buf[n:] == CANARY).all())


def _workspace(need):
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[need:] = CANARY_BYTE
    return ws


def _ws_intact(ws, need):
    return bool((ws[need:] == CANARY_BYTE).all())


def attn_pool(y, ha, hb, cw, cb):
    """rrt_attn_pool_f32 on device tensors -> (pooled [dim], attn [N], a_raw [N]) after every canary was checked"""
    lib = _lib.load()
    (N, dim), hid = y.shape, ha.shape[1]
    need = C.c_size_t()
    _lib.check(lib.rrt_attn_pool_workspace_size(N, dim, hid, C.byref(need)), "rrt_attn_pool_workspace_size")
    ws = _workspace(need.value)
    pooled, attn, raw = _guarded(dim), _guarded(N), _guarded(N)
    _lib.check(lib.rrt_attn_pool_f32(_p(y), _p(ha), _p(hb), _p(cw), _p(cb), _p(pooled), _p(attn), _p(raw), N, dim, hid, _p(ws),
                                     need.value, _st()), "rrt_attn_pool_f32")
    torch.cuda.synchronize()
    assert _ws_intact(ws, need.value), "workspace overrun"
    assert _intact(pooled, dim) and _intact(attn, N) and _intact(raw, N), "output overrun"
    return pooled[:dim], attn[:N], raw[:N]


def pool_predict(c, d):
    """rrt_pool_predict_f32 for PredCase c on the device dict d -> {logits, pooled or None, attn / s or None}"""
    lib = _lib.load()
    need = C.c_size_t()
    _lib.check(lib.rrt_pool_workspace_size(c.N, c.dim, c.hid, int(c.gated), C.byref(need)), "rrt_pool_workspace_size")
    ws = _workspace(need.value)
    pooled, attn, logits = _guarded(c.dim), _guarded(c.N), _guarded(c.ncls)
    rc = lib.rrt_pool_predict_f32(_p(d["y"]), _p(d["a_w"]), _p(d["a_b"]), _p(d["b_w"]), _p(d["b_b"]), _p(d["c_w"]), _p(d["c_b"]),
                                  _p(d["pred_w"]), _p(d["pred_b"]), _p(pooled) if c.want_pooled else None, _p(logits),
                                  _p(attn) if c.want_attn else None, c.no_norm, c.N, c.dim, c.hid, K.ACT_CODE[c.act], c.ncls, 0,
                                  _p(ws), need.value, _st())
    _lib.check(rc, "rrt_pool_predict_f32")
    torch.cuda.synchronize()
    assert _ws_intact(ws, need.value), "workspace overrun"
    assert _intact(pooled, c.dim) and _intact(attn, c.N) and _intact(logits, c.ncls), "output overrun"
    if not c.want_pooled:
        assert bool(torch.isnan(pooled[:c.dim]).all())
    if not c.want_attn:
        assert bool(torch.isnan(attn[:c.N]).all())
    row = attn[:c.N].cpu().numpy() if c.want_attn else None
    return {"logits": logits[:c.ncls].cpu().numpy(), "pooled": pooled[:c.dim].cpu().numpy() if c.want_pooled else None,
            "attn": None if c.no_norm else row, "s": row if c.no_norm else None}


def attn_pool_backward(c, inp):
    """rrt_attn_pool_backward_f32 for BwdCase c -> {dy, dhid_a, dhid_b, dcw, dcb} as numpy"""
    lib = _lib.load()
    N, dim, hid = c.N, c.dim, c.hid
    t = {k: dev(inp[k]) for k in ("y", "hid_a", "hid_b", "c_w", "attn", "pooled", "d_pooled", "d_attn", "d_raw", "c_ext")}
    need = C.c_size_t()
    _lib.check(lib.rrt_attn_pool_workspace_size(N, dim, hid, C.byref(need)), "rrt_attn_pool_workspace_size")
    ws = _workspace(need.value)
    dy, dha = _guarded(N * dim), _guarded(N * hid)
    dhb = _guarded(N * hid) if c.gated else None
    dwcb = _guarded(hid + 4)                                   # [hidden + 4]: d c_w, d c_b at [hidden]
    _lib.check(lib.rrt_attn_pool_backward_f32(_p(t["y"]), _p(t["hid_a"]), _p(t["hid_b"]), _p(t["c_w"]), _p(t["attn"]), _p(t["pooled"]),
                                              _p(t["d_pooled"]), _p(t["d_attn"]), _p(t["d_raw"]), _p(t["c_ext"]), _p(dy), _p(dha),
                                              _p(dhb), _p(dwcb), N, dim, hid, _p(ws), need.value, _st()), "rrt_attn_pool_backward_f32")
    torch.cuda.synchronize()
    assert _ws_intact(ws, need.value), "workspace overrun"
    assert _intact(dy, N * dim) and _intact(dha, N * hid) and _intact(dwcb, hid + 4) and (dhb is None or _intact(dhb, N * hid))
    out = {"dy": dy[:N * dim].reshape(N, dim), "dhid_a": dha[:N * hid].reshape(N, hid), "dcw": dwcb[:hid], "dcb": dwcb[hid:hid + 1]}
    if c.gated:
        out["dhid_b"] = dhb[:N * hid].reshape(N, hid)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _judge(stage, cid, errs, emu):
    """print and record kernel and emulation errors side by side, then hold the kernel to the bounds"""
    fails = []
    for name, (err, tol, *_) in errs.items():
        e_emu = emu[name][0] if name in emu else float("nan")
        print(f"{stage} {cid} {name}: kernel {err:.3e} emulate32 {e_emu:.3e} bound {tol:.3e}")
        TABLE.append((stage, cid, name, err, e_emu, tol))
        if not err <= tol:
            fails.append(f"{stage} {cid} {name}: {err:.3e} > {tol:.3e} (emulate32 {e_emu:.3e})")
    assert not fails, "\n".join(fails)


def _forward_case(c, inputs, meta, y_dev=None, stage="forward"):
    y, ha, hb, cw, cb = inputs
    ref = R.ref64(y, ha, hb, cw, cb)
    emu = K.forward_errors(R.emulate32(y, ha, hb, cw, cb), ref)
    pooled, attn, raw = attn_pool(dev(y) if y_dev is None else y_dev, dev(ha), dev(hb), dev(cw), dev(cb))
    got = {"pooled": pooled.cpu().numpy(), "attn": attn.cpu().numpy(), "s": raw.cpu().numpy()}
    assert np.isfinite(got["pooled"]).all() and np.isfinite(got["attn"]).all()
    if c.kind == "masked":
        assert float(np.abs(got["attn"][meta["masked"]]).max()) == 0.0, "masked entries must be exact zeros"
    if c.kind == "tie":
        a, b = meta["pair"]
        assert got["s"][a] == got["s"][b] and got["attn"][a] == got["attn"][b], "tied scores differ in their bits"
    if c.kind == "flat":
        assert (got["attn"] == got["attn"][0]).all() and (got["s"] == got["s"][0]).all(), "flat entries differ in their bits"
    _judge(stage, K.fwd_id(c), K.forward_errors(got, ref), emu)
    return pooled, attn, raw


@pytest.mark.parametrize("c", K.FWD_CASES, ids=K.fwd_id)
def test_forward_stage(c):
    y, ha, hb, cw, cb, meta = K.forward_inputs(c)
    _forward_case(c, (y, ha, hb, cw, cb), meta)


@pytest.mark.parametrize("N", K.LDS_NS)
def test_large_lds_merge(N):
    """the merge launch on both sides of its 64 KB LDS threshold and at the 1e6-token limit: every kind on one y; the same
    inputs twice give the same bits, and a small bag in between (default LDS) is not disturbed by the raised attribute"""
    cases = [c for c in K.LDS_CASES if c.N == N]
    assert (K.merge_lds(N, K.LDS_DIM) > K.LDS_DEFAULT) == (N > K.LDS_EDGE)
    small = K.FwdCase(100, 64, 12, True, True, "mild", None)
    y_dev = dev(K.forward_inputs(cases[0])[0])
    for c in cases:
        y, ha, hb, cw, cb, meta = K.forward_inputs(c)
        first = _forward_case(c, (y, ha, hb, cw, cb), meta, y_dev=y_dev, stage="large-lds")
        sy, sha, shb, scw, scb, smeta = K.forward_inputs(small)
        _forward_case(small, (sy, sha, shb, scw, scb), smeta, stage="after-lds")
        again = attn_pool(y_dev, dev(ha), dev(hb), dev(cw), dev(cb))
        for a, b, name in zip(first, again, ("pooled", "attn", "a_raw")):
            assert torch.equal(a, b), f"{K.fwd_id(c)} {name}: two runs differ in their bits"


@pytest.mark.parametrize("c", K.PRED_CASES, ids=K.pred_id)
def test_predictor_stage(c):
    d = K.predict_inputs(c)
    h64 = K.hidden_rows(d["y"], d["a_w"], d["a_b"], d["b_w"], d["b_b"], c.act, torch.float64)
    h32 = K.hidden_rows(d["y"], d["a_w"], d["a_b"], d["b_w"], d["b_b"], c.act, torch.float32)
    ref = R.ref64(d["y"], h64[0], h64[1], d["c_w"], d["c_b"], d["pred_w"], d["pred_b"])
    emu = R.emulate32(d["y"], h32[0], h32[1], d["c_w"], d["c_b"], d["pred_w"], d["pred_b"])
    got = pool_predict(c, {k: dev(v) for k, v in d.items()})
    assert np.isfinite(got["logits"]).all()
    _judge("predict", K.pred_id(c), K.forward_errors(got, ref), K.forward_errors(emu, ref))


@pytest.mark.parametrize("c", K.BWD_CASES, ids=K.bwd_id)
def test_backward_stage(c):
    inp = K.backward_inputs(c)
    emu = K.backward_errors(R.emulate32_backward(*(inp[k] for k in ("y", "hid_a", "hid_b", "c_w", "attn", "pooled", "d_pooled",
                                                                   "d_attn", "d_raw", "c_ext"))), inp)
    got = attn_pool_backward(c, inp)
    errs = K.backward_errors(got, inp)
    for name, (_err, _tol, scale) in errs.items():
        assert (scale <= 1e-9 * inp["natural"]) == K.floor_expected(c, name), (name, scale)
    _judge("backward", K.bwd_id(c), errs, emu)


# ------------------------------------------------------------------ the consumers at a bag above 32 768 tokens
BIG_N = 32801


def test_rrtmil_one_call_against_composite_at_large_n():
    """RRTMIL(input_dim=64), eval: the one-call path (rrt_mil_forward_f32: these kernels behind the encoder) against the
    composite path (the reference's op sequence in torch around the HIP encoder), as the last block of
    tests/test_hip_parity.py::test_rrtmil_variants_match_reference, at its 1e-4"""
    from rrt_mil_amd import RRTMIL
    st = synth.mil_state(input_dim=64, n_classes=2)
    mil = RRTMIL(input_dim=64).eval()
    mil.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    mil = mil.to(DEV)
    feats = dev(synth.bag(BIG_N, 64, tag="milpool/rrtmil", nonneg=True)).unsqueeze(0)
    with torch.no_grad():
        logits, attn = mil(feats, return_attn=True)
        x2 = mil.dp(mil.patch_to_emb(feats))
        y2 = mil.online_encoder(x2)
        p2, a2 = mil.pool_fn(y2, return_attn=True)
        l2 = mil.predictor(p2)
    torch.cuda.synchronize()
    assert logits.shape == (1, 2) and attn.shape == (1, BIG_N)
    err = float((l2.double() - logits.double()).abs().max())
    err_a = float((a2.double() - attn.double()).abs().max())
    print(f"RRTMIL N={BIG_N}: composite vs one-call logits {err:.3e} attention {err_a:.3e}")
    assert bool(torch.isfinite(logits).all()) and err <= 1e-4
    assert err_a <= 1e-6 and abs(float(attn.double().sum()) - 1.0) < 1e-5          # (1e-6: that test's attention bound)


def test_abmil_forward_bag_at_large_n():
    """ABMIL without an encoder through forward_bag (rrt_bagmil_forward_f32) against the same module in float64 torch, under
    tests/test_bagmil_gpu.py::test_whole_head's rule: max(2e-5, 8 x the fp32 restatement's error), relative to max(1, max |ref|)"""
    import bagmil_cases as BC
    import bagmil_ref as BR
    from rrt_mil_amd import ABMIL
    m = BC.construct({"attmil": ABMIL}, "attmil", rrt=None, bias=False)
    state = BC.head_state(m.state_dict(), "attmil")
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    m = m.to(DEV).eval()
    x = BC.bag("attmil", False, BIG_N)
    kw = dict(enc_cfg=BC.ENC_CFG, act=BC.ACT["attmil"], gate_act=BC.ACT["attmil"])
    r64, r32 = BR.head("attmil", x, state, dtype=torch.float64, **kw), BR.head("attmil", x, state, dtype=torch.float32, **kw)
    with torch.no_grad():
        out = m.forward_bag(torch.from_numpy(x).to(DEV), return_attn=True, return_features=True)
    torch.cuda.synchronize()
    for mine, theirs in (("logits", "logits"), ("attn", "attn"), ("features", "pooled")):
        got, ref = out[mine].detach().cpu(), torch.as_tensor(r64[theirs]).detach()
        assert tuple(got.shape) == tuple(ref.shape) and bool(torch.isfinite(got).all()), mine
        e32 = BR.rel_err(torch.as_tensor(r32[theirs]).detach(), ref)
        err, bound = BR.rel_err(got, ref), max(2e-5, 8.0 * e32)
        print(f"ABMIL N={BIG_N} {mine}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
        assert err <= bound, (mine, err, bound)


@pytest.mark.parametrize("no_norm", [False, True])
@pytest.mark.parametrize("N", [33, 32769])
def test_attn_pool_module_path(N, no_norm):
    """mil._AttnPool through RRTMIL._pool with a loss that reads both pooled and the returned attention (so c_ext is computed in
    Python), against float64 autograd of the same module, with the criterion of
    tests/test_hip_parity.py::test_attn_pool_forward_backward"""
    from rrt_mil_amd.mil import RRTMIL
    torch.manual_seed(7)
    mil = RRTMIL(input_dim=64, n_classes=2, da_act="tanh", da_gated=True, da_bias=True, dropout=0.0).to(DEV).train()
    ref = copy.deepcopy(mil.pool_fn).double()
    x = torch.from_numpy(synth.normal(f"milpool/x{N}", (1, N, 512))).to(DEV).requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    r1 = torch.from_numpy(synth.normal("milpool/r1", (1, 512))).to(DEV)
    r2 = torch.from_numpy(synth.normal(f"milpool/r2{N}", (1, N))).to(DEV)
    pooled, a = mil._pool(x, no_norm)
    p64, a64 = ref(x64, return_attn=True, no_norm=no_norm)
    assert pooled.shape == p64.shape and a.shape == a64.shape
    assert float((pooled.double() - p64).abs().max()) <= 2e-5
    assert float((a.double() - a64).abs().max()) <= 2e-5 * max(1.0, float(a64.abs().max()))
    ((pooled * r1).sum() + (a * r2).sum()).backward()
    ((p64 * r1.double()).sum() + (a64 * r2.double()).sum()).backward()
    torch.cuda.synchronize()

    def close(g, g64, what):
        scale = float(g64.abs().max()) + 1e-30
        err = float((g.double() - g64).abs().max())
        print(f"_AttnPool N={N} no_norm={no_norm} {what}: err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-4 * scale + 2e-6, (what, err, scale)
    close(x.grad, x64.grad, "dx")
    for (name, p), (_, p64_) in zip(mil.pool_fn.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (p64_.grad is None), name
        if p.grad is not None:
            close(p.grad, p64_.grad, name)


def test_layer_path_keeps_torch_ops_outside_the_lds_limits():
    """mil.lib_attn_pool declines (None: the caller keeps the torch ops) exactly the shapes rrt_attn_pool_workspace_size refuses
    for their LDS, and takes the neighbouring ones"""
    from rrt_mil_amd.mil import lib_attn_pool
    need = C.c_size_t()
    for dim, hid in ((32, 4084), (32, 4088), (512, 4096), (512, 128)):
        x, ha = torch.zeros(1, 4, dim, device=DEV), torch.zeros(1, 4, hid, device=DEV)
        lin = torch.nn.Linear(hid, 1).to(DEV)
        rc = _lib.load().rrt_attn_pool_workspace_size(4, dim, hid, C.byref(need))
        assert (rc == 0) == (K.backward_lds(dim, hid) <= K.LDS_DEFAULT)
        with torch.no_grad():
            out = lib_attn_pool(x, ha, None, lin)
        torch.cuda.synchronize()
        assert (out is not None) == (rc == 0), (dim, hid, rc)
