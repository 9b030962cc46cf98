"""GPU (-m gpu): the batched Nystrom-attention kernels of csrc/nystrom.hip, one stage at a time and as a whole, and the two
Nystrom ablations of RRTEncoder (attn='ntrans', region_attn='ntrans') and RRTMIL around them, against the float64 restatement
tests/ntrans_ref.py (pinned to the reference's own float64 run by tests/test_ntrans_cpu.py) -- never against another kernel,
except where the claim IS bit-identity: with b = 1 every batched entry gives the bits of its single-sequence counterpart.

Bound per quantity, the project's stage rule: err <= max(2e-5, 8 x e32) relative to max(1, max |float64 reference|), e32 = the
error of the same restatement evaluated in plain fp32 on the CPU on the same inputs -- measured here, never read off a kernel.
A stage's inputs are the fp32 roundings of the float64 run's tensors.  The harness is tests/test_transmil_gpu.py's: NaN-filled
outputs with canary rows behind them, workspaces of exactly the queried size with canary bytes behind them, every call twice
with the same bits.  The case lists are module data of tests/ntrans_cases.py; importing this module needs no device.
With RRT_NTRANS_ERRORS_OUT=<file> the module writes its error table (kept as profiles/ntrans_errors.txt)."""
import ctypes as C
import functools
import os

import pytest
import torch

import ntrans_cases as NC
import ntrans_ref as NR
from conftest import load_golden
from rrt_mil_amd import _lib
from test_transmil_gpu import Out, Ws, dev, error_table, size_of, stream, twice
import test_transmil_gpu as T1

pytestmark = pytest.mark.gpu

TOL = 2e-5
E32_FACTOR = 8.0
RECORDS = []
H = NC.HEADS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_NTRANS_ERRORS_OUT")
    if out and RECORDS:
        with open(out, "w") as fh:
            fh.write(error_table(RECORDS))


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """a device error is sticky: nothing more is started on a device that reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is run on it: {e}", returncode=3)


def judge(grp, case, what, got, ref64, ref32, fails, e32_floor=0.0):
    e32 = max(NR.rel_err(ref32, ref64), e32_floor)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (case, what, got.shape, ref64.shape)
    err = NR.rel_err(got, ref64) if bool(torch.isfinite(got).all()) else float("inf")
    bound = max(TOL, E32_FACTOR * e32)
    RECORDS.append((grp, what, e32, err))
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


@functools.lru_cache(maxsize=8)
def reference(name):
    """the restatement on the case's inputs in float64 and in fp32 (CPU); computed once per case, never modified"""
    b, n, peaked = NC.ATTN_CASES[name]
    state, x = NC.batch_inputs(b, n, peaked)
    return state, x, NR.nystrom_batched(x, state, H, dtype=torch.float64), NR.nystrom_batched(x, state, H, dtype=torch.float32)


# ------------------------------------------------------------------ the batched stage launchers
def run_landmarks(qkv, b):
    lib, npad = _lib.load(), qkv.shape[-2]
    ql, kl = twice(lambda a, c: lib.rrt_nystrom_landmarks_batched_f32(qkv.data_ptr(), a.ptr(), c.ptr(), b, npad, H, stream()),
                   lambda: (Out(b, H, 256, 64), Out(b, H, 256, 64)), "rrt_nystrom_landmarks_batched_f32")
    return ql.t, kl.t


def run_landmark_sim(ql, kl, b):
    lib = _lib.load()
    (a2,) = twice(lambda a: lib.rrt_nystrom_landmark_sim_batched_f32(ql.data_ptr(), kl.data_ptr(), a.ptr(), b, H, stream()),
                  lambda: (Out(b, H, 256, 256),), "rrt_nystrom_landmark_sim_batched_f32")
    return a2.t


def run_landmark_attn(qkv, ql, b):
    lib, npad = _lib.load(), qkv.shape[-2]
    need = size_of(lib.rrt_nystrom_landmark_attn_batched_workspace_size, b, npad, H)
    av, _ = twice(lambda a, w: lib.rrt_nystrom_landmark_attn_batched_f32(qkv.data_ptr(), ql.data_ptr(), a.ptr(), b, npad, H,
                                                                         w.ptr(), w.n, stream()),
                  lambda: (Out(b, H, 256, 64), Ws(need)), "rrt_nystrom_landmark_attn_batched_f32")
    return av.t


def run_pinv(a2, b, iters=NC.PINV_ITERATIONS, heads=H):
    lib = _lib.load()
    need = size_of(lib.rrt_nystrom_pinv_batched_workspace_size, b, heads)
    z, _ = twice(lambda a, w: lib.rrt_nystrom_pinv_batched_f32(a2.data_ptr(), a.ptr(), b, heads, iters, w.ptr(), w.n, stream()),
                 lambda: (Out(b, heads, 256, 256), Ws(need)), "rrt_nystrom_pinv_batched_f32")
    return z.t


def run_zav(z, av, b):
    lib = _lib.load()
    (wz,) = twice(lambda a: lib.rrt_nystrom_zav_batched_f32(z.data_ptr(), av.data_ptr(), a.ptr(), b, H, stream()),
                  lambda: (Out(b, H, 256, 64),), "rrt_nystrom_zav_batched_f32")
    return wz.t


def run_output(qkv, kl, wz, conv_w, b):
    lib, npad = _lib.load(), qkv.shape[-2]
    ks = conv_w.shape[1] if conv_w is not None else 0
    (o,) = twice(lambda a: lib.rrt_nystrom_output_batched_f32(qkv.data_ptr(), kl.data_ptr(), wz.data_ptr(),
                                                              conv_w.data_ptr() if conv_w is not None else None, a.ptr(), b,
                                                              npad, H, ks, stream()),
                 lambda: (Out(b, npad, H * 64),), "rrt_nystrom_output_batched_f32")
    return o.t


def nys_desc_weights(state, dim=NC.DIM, heads=H):
    d, w = _lib.NystromDesc(), _lib.NystromWeights()
    d.dim, d.heads, d.dim_head, d.num_landmarks, d.pinv_iterations = dim, heads, 64, 256, NC.PINV_ITERATIONS
    d.residual, d.residual_conv_kernel = 1, 33
    keep = [dev(torch.from_numpy(state[k])) for k in NR.NYS_KEYS]
    w.qkv_w, w.out_w, w.out_b, w.conv_w = (t.data_ptr() for t in keep)
    return d, w, keep


def run_attention_batched(x, state):
    lib = _lib.load()
    d, w, _keep = nys_desc_weights(state)
    xd = dev(torch.from_numpy(x))
    b, n, dim = x.shape
    need = size_of(lib.rrt_nystrom_batched_workspace_size, C.byref(d), b, n)
    y, _ = twice(lambda a, s: lib.rrt_nystrom_attention_batched_f32(C.byref(d), C.byref(w), xd.data_ptr(), a.ptr(), b, n, s.ptr(),
                                                                    s.n, stream()),
                 lambda: (Out(b, n, dim), Ws(need)), "rrt_nystrom_attention_batched_f32")
    return y.t


# ------------------------------------------------------------------ batched stages, each on its own
@pytest.mark.parametrize("name", list(NC.STAGE_CASES))
def test_batched_stages(name):
    b, n, _peaked = NC.STAGE_CASES[name]
    state, _x, r64, _r32 = reference(name)
    fails, grp = [], f"stages {name}"
    i32 = {k: r64[k].float() for k in ("qkv", "ql", "kl", "a2", "av", "z", "wz")}
    i64 = {k: v.double() for k, v in i32.items()}
    g = {k: dev(v) for k, v in i32.items()}
    conv32 = torch.from_numpy(state["res_conv.weight"]).reshape(H, -1)
    ql, kl = run_landmarks(g["qkv"], b)
    for what, got, a, c in zip(("ql", "kl"), (ql, kl), NR.st_landmarks(i64["qkv"], H), NR.st_landmarks(i32["qkv"], H)):
        judge(grp, name, what, got, a, c, fails)
    judge(grp, name, "a2", run_landmark_sim(g["ql"], g["kl"], b), NR.st_landmark_sim(i64["ql"], i64["kl"]),
          NR.st_landmark_sim(i32["ql"], i32["kl"]), fails)
    judge(grp, name, "a3.v", run_landmark_attn(g["qkv"], g["ql"], b), NR.st_landmark_attn(i64["qkv"], i64["ql"], H),
          NR.st_landmark_attn(i32["qkv"], i32["ql"], H), fails)
    judge(grp, name, "z", run_pinv(g["a2"], b), NR.pinv_iter(i64["a2"], NC.PINV_ITERATIONS),
          NR.pinv_iter(i32["a2"], NC.PINV_ITERATIONS), fails)
    judge(grp, name, "z.(a3.v)", run_zav(g["z"], g["av"], b), NR.st_zav(i64["z"], i64["av"]), NR.st_zav(i32["z"], i32["av"]), fails)
    for conv in (conv32, None):
        judge(grp, name, "o" if conv is not None else "o no conv",
              run_output(g["qkv"], g["kl"], g["wz"], dev(conv) if conv is not None else None, b),
              NR.st_output(i64["qkv"], i64["kl"], i64["wz"], H, conv.double() if conv is not None else None),
              NR.st_output(i32["qkv"], i32["kl"], i32["wz"], H, conv), fails)
    assert not fails, "\n".join(fails)


def test_pinv_scale_folds_more_matrices_than_the_loop_takes():
    """b * heads = 40 > 16 matrices: the records go through the reduction pass; the ONE peaked matrix sits where a fold that
    drops the tail of a strided pass, or takes a per-item maximum, would miss it"""
    b, i = 20, torch.arange(256)
    s = torch.zeros(b, 2, 256, 256, dtype=torch.float64)
    s[:, :, i, i] = 6.0
    s[17, 1, i, i] = 4.0
    s[17, 1, :, 7] += 4.0                                # matrix 35 of 40: column sum of tens
    a32 = s.softmax(-1).float()
    fails = []
    z = run_pinv(dev(a32), b, iters=1)
    ref = NR.pinv_iter(a32.double(), 1)
    judge("pinv 40 matrices", "one peaked matrix", "z it1", z, ref, NR.pinv_iter(a32, 1), fails)
    assert NR.rel_err(NR.pinv_iter_per_item(a32.double(), 1), ref) > 100 * TOL
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ the whole batched attention
@pytest.mark.parametrize("name", list(NC.ATTN_CASES))
def test_batched_attention(name):
    b, n, _peaked = NC.ATTN_CASES[name]
    state, x, r64, r32 = reference(name)
    fails, grp = [], f"attention {name}"
    y = run_attention_batched(x, state)
    judge(grp, name, "y", y, r64["y"], r32["y"], fails)
    gold = load_golden("ntrans_attn")
    gy = torch.from_numpy(gold[name + "/y"])
    judge(grp, name, "y golden", y[:, [0, n - 1]], gy, gy, fails, e32_floor=float(gold[name + "/e32"]))
    assert not fails, "\n".join(fails)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("n", NC.BIT_IDENTITY_LENGTHS)
def test_b1_gives_the_bits_of_the_single_sequence_entries(n):
    state, x = NC.batch_inputs(1, n, False)
    r64 = NR.nystrom_batched(x, state, H, dtype=torch.float64)
    g = {k: dev(r64[k].float()) for k in ("qkv", "ql", "kl", "a2", "av", "z", "wz")}
    s = {k: v[0] for k, v in g.items()}
    conv = dev(torch.from_numpy(state["res_conv.weight"]).reshape(H, -1))
    for a, c in zip(run_landmarks(g["qkv"], 1), T1.run_landmarks(s["qkv"], H)):
        assert same_bits(a[0], c)
    assert same_bits(run_landmark_sim(g["ql"], g["kl"], 1)[0], T1.run_landmark_sim(s["ql"], s["kl"], H))
    assert same_bits(run_landmark_attn(g["qkv"], g["ql"], 1)[0], T1.run_landmark_attn(s["qkv"], s["ql"], H))
    assert same_bits(run_pinv(g["a2"], 1)[0], T1.run_pinv(s["a2"], H, NC.PINV_ITERATIONS))
    assert same_bits(run_zav(g["z"], g["av"], 1)[0], T1.run_zav(s["z"], s["av"], H))
    assert same_bits(run_output(g["qkv"], g["kl"], g["wz"], conv, 1)[0], T1.run_output(s["qkv"], s["kl"], s["wz"], conv, H))
    assert same_bits(run_attention_batched(x, state)[0], T1.run_attention(x[0], state, NC.DIM, H))


def test_nystrom_module_takes_a_batch():
    from rrt_mil_amd import NystromAttention
    name = "b3_n144_peaked"
    state, x, _r64, _r32 = reference(name)
    mod = NystromAttention(NC.DIM, heads=H)
    mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    mod = mod.cuda().eval()
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        y = mod.forward_batch(xd)
        assert y.shape == xd.shape and same_bits(y, run_attention_batched(x, state))
        assert same_bits(mod.forward_batch(xd[:1]), run_attention_batched(x[:1], state)) and same_bits(mod(xd[:1]), mod.forward_batch(xd[:1]))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert same_bits(mod.forward_batch(xd), y)
        with pytest.raises(ValueError, match="b = 1"):
            mod.attention_row(xd)
        with pytest.raises(ValueError, match="forward_batch"):
            mod(xd)                                                                  # forward itself keeps one sequence
    with pytest.raises(NotImplementedError, match="b = 1"):
        mod.forward_batch(xd)                                                        # a graph is wanted


# ------------------------------------------------------------------ the encoder
def make_encoder(name):
    from rrt_mil_amd import RRTEncoder
    cfg, state, x = NC.encoder_inputs(name)
    enc = RRTEncoder(**cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return enc.cuda().eval(), cfg, state, x


@pytest.mark.parametrize("name", list(NC.ENCODER_CASES))
def test_encoder(name):
    enc, cfg, state, x = make_encoder(name)
    lib, (N, D) = _lib.load(), x.shape
    r64, r32 = (NR.encoder(x, state, cfg, dtype=dt) for dt in (torch.float64, torch.float32))
    xd = dev(torch.from_numpy(x))
    nd, w = enc._nystrom_desc(), enc._weights()
    assert nd.mode == (_lib.NYSTROM_BAG if NC.is_bag(cfg) else _lib.NYSTROM_REGIONS)
    need = size_of(lib.rrt_encoder_nystrom_workspace_size, C.byref(enc._desc), C.byref(nd), N)
    y, _ = twice(lambda a, s: lib.rrt_encoder_nystrom_forward_f32(C.byref(enc._desc), C.byref(nd), C.byref(w), xd.data_ptr(), a.ptr(),
                                                                  N, s.ptr(), s.n, stream()),
                 lambda: (Out(N, D), Ws(need)), "rrt_encoder_nystrom_forward_f32")
    fails, grp = [], "encoder " + ("bag" if NC.is_bag(cfg) else "regions")
    judge(grp, name, "y", y.t, r64, r32, fails)
    gold = load_golden("ntrans_encoder")
    gy = torch.from_numpy(gold[name + "/y"])
    judge(grp, name, "y golden", y.t[NC.golden_rows(N)], gy, gy, fails, e32_floor=float(gold[name + "/e32"]))
    with torch.no_grad():
        assert same_bits(enc(xd), y.t) and same_bits(enc(xd[None])[0], y.t)          # the module: the same one call
    assert not fails, "\n".join(fails)


def test_encoder_surface():
    enc, _cfg, _state, x = make_encoder("reg_n200_rn2")
    xd = dev(torch.from_numpy(x))
    x2 = dev(torch.from_numpy(NC.encoder_inputs("bag_n300")[2]))
    with torch.no_grad():
        y = enc(xd)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert same_bits(enc(xd), y)                                             # exact fp32 under autocast as well
        assert same_bits(enc.forward_bag(xd), y)
        outs = enc.forward_bags([xd, x2[None], xd])
        assert same_bits(outs[0], y) and same_bits(outs[2], y) and same_bits(outs[1][0], enc(x2)) and outs[1].dim() == 3
        enc._ws.fill_(0xFF)
        assert same_bits(enc(xd), y)                                                 # nothing is read before it is written
        with pytest.raises(NotImplementedError, match="one bag per call"):
            enc(torch.stack([xd, xd]))
        with pytest.raises(NotImplementedError, match="eval"):
            enc.train()(xd)
    enc.eval()
    with pytest.raises(NotImplementedError, match="no_grad"):
        enc(xd)                                                                      # a graph is wanted
    with pytest.raises(NotImplementedError, match="no backward"):
        enc.forward_bag_train(xd)


# ------------------------------------------------------------------ RRTMIL around it
@pytest.mark.parametrize("name", list(NC.MIL_CASES))
def test_rrtmil(name):
    from rrt_mil_amd import RRTMIL
    cfg, state, x = NC.mil_inputs(name)
    model = RRTMIL(input_dim=NC.MIL_INPUT_DIM, **cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    model = model.cuda().eval()
    xd = dev(torch.from_numpy(x))
    with torch.no_grad():
        logits = model(xd[None])
        assert logits.shape == (1, 2) and same_bits(logits, model(xd[None]))
        for call in (lambda: model.forward_bag(xd), lambda: model.forward_bags([xd, xd])):
            with pytest.raises(NotImplementedError, match="ntrans"):
                call()
    r64, r32 = (NR.rrtmil(x, state, cfg, dtype=dt) for dt in (torch.float64, torch.float32))
    fails = []
    judge("RRTMIL", name, "logits", logits[0], r64, r32, fails)
    gold = load_golden("ntrans_encoder")
    gl = torch.from_numpy(gold[name + "/logits"])
    judge("RRTMIL", name, "logits golden", logits[0], gl, gl, fails, e32_floor=float(gold[name + "/e32"]))
    assert not fails, "\n".join(fails)
