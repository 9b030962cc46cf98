"""GPU (-m gpu): the attention-map kernels of csrc/nystrom_row.hip -- the stage entry rrt_nystrom_attn_row_f32, the whole call
rrt_nystrom_attention_row_f32 and TransMIL's ``return_attn`` around rrt_transmil_forward_attn_f32 -- against the float64
restatement tests/transmil_attn_ref.py (pinned to the reference's own ``return_attn=True`` run by
tests/test_transmil_attn_cpu.py), never against another kernel.

Bound per quantity, the project's stage rule: err <= max(2e-5, 8 x e32), e32 = the error of the same restatement evaluated in
plain fp32 on the CPU on the same inputs -- measured here, never read off a kernel.  Both errors are relative to the float64
tensor's LARGEST |entry|, not to max(1, .): the entries of a row are about 1 / n at gain 1, and a bound relative to 1 would pass
anything.  The stage entry's inputs are the fp32 roundings of the float64 run's tensors (lse3 included), and its references are
computed from exactly those.  The golden cases are held to the reference's recorded rows with the reference's own recorded
fp32 error in the bound.

Every output is NaN-filled with canary rows behind it, workspaces have exactly the queried size with canary bytes behind them,
every call runs twice and must give the same bits.  With RRT_TRANSMIL_ATTN_ERRORS_OUT=<file> the module writes its error table
(kept as profiles/transmil_attn_errors.txt).  Importing this module needs no device."""
import ctypes as C
import functools
import os

import pytest
import torch

import nystrom_ref as R
import transmil_attn_cases as AC
import transmil_attn_ref as AR
import transmil_cases as TC
from conftest import load_golden
from rrt_mil_amd import _lib
from test_transmil_gpu import Out, Ws, dev, error_table, make_model, run_attention, size_of, stream, twice

pytestmark = pytest.mark.gpu

TOL = 2e-5
E32_FACTOR = 8.0
RECORDS = []                      # (group, quantity, e32, kernel error), both relative to the largest |entry|


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_TRANSMIL_ATTN_ERRORS_OUT")
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


def judge(grp, case, what, got, ref64, ref32, fails, e32_floor=0.0, scale=None):
    """one quantity against float64, both errors relative to max |ref64| (or to `scale`): bound max(TOL, 8 x e32)"""
    e32 = max(AR.rel_err_max(ref32, ref64, scale), e32_floor)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (case, what, got.shape, ref64.shape)
    err = AR.rel_err_max(got, ref64, scale) if bool(torch.isfinite(got).all()) else float("inf")
    bound = max(TOL, E32_FACTOR * e32)
    RECORDS.append((grp, what, e32, err))
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


@functools.lru_cache(maxsize=2)
def reference(dim, heads, n, gain):
    """the restatement on the case's inputs in float64 and in fp32 (CPU); computed once per case, never modified"""
    state, x = TC.attn_inputs(dim, heads, n, gain)
    return state, x, R.nystrom(x, state, heads, dtype=torch.float64), R.nystrom(x, state, heads, dtype=torch.float32)


def run_stage(g, row_padded, heads):
    """rrt_nystrom_attn_row_f32 on fp32 device tensors -> (r [h, 256], attn [h, np])"""
    lib, npad = _lib.load(), g["qkv"].shape[0]
    r, a = twice(lambda r, a: lib.rrt_nystrom_attn_row_f32(g["qkv"].data_ptr(), g["ql"].data_ptr(), g["kl"].data_ptr(),
                                                           g["z"].data_ptr(), g["lse3"].data_ptr(), r.ptr(), a.ptr(), row_padded,
                                                           npad, heads, stream()),
                 lambda: (Out(heads, 256), Out(heads, npad)), "rrt_nystrom_attn_row_f32")
    return r.t, a.t


def row_call(x, state, dim, heads, fill=0xA5):
    """(call, outs, size) of rrt_nystrom_attention_row_f32 for `twice`; the caller binds the row"""
    lib = _lib.load()
    d, w = _lib.NystromDesc(), _lib.NystromWeights()
    d.dim, d.heads, d.dim_head, d.num_landmarks, d.pinv_iterations, d.residual, d.residual_conv_kernel = dim, heads, 64, 256, 6, 1, 33
    ts = [dev(torch.from_numpy(state[k])) for k in ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias", "res_conv.weight")]
    w.qkv_w, w.out_w, w.out_b, w.conv_w = (t.data_ptr() for t in ts)
    xd, n = dev(torch.from_numpy(x)), x.shape[0]
    need = size_of(lib.rrt_nystrom_attention_row_workspace_size, C.byref(d), n)

    def call(row):
        return lambda y, a, s: lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), xd.data_ptr(), y.ptr(), row, a.ptr(), n,
                                                                 s.ptr(), s.n, stream())

    return call, (lambda: (Out(n, dim), Out(heads, n), Ws(need, fill))), (ts, xd)


# ------------------------------------------------------------------ the stage entry and the whole call
@pytest.mark.parametrize("dim,heads,n,gain", AC.ATTN_CASES, ids=lambda v: str(v))
def test_stage_and_whole_call(dim, heads, n, gain):
    state, x, r64, r32 = reference(dim, heads, n, gain)
    case, grp = f"d{dim} h{heads} n{n} g{gain:g}", f"d{dim} h{heads} gain {gain:g}"
    if gain > 1:
        assert TC.PEAK_RANGE[0] <= r64["peak"] <= TC.PEAK_RANGE[1], (case, r64["peak"])
    fails, pad = [], TC.pad_of(n)
    # the stage's inputs: the float64 run's tensors rounded to fp32; its references: the stage function on exactly those
    i32 = {k: r64[k].float() for k in ("qkv", "ql", "kl", "z")}
    i32["lse3"] = AR.lse3_of(r64["qkv"], r64["ql"], heads).float()
    i64 = {k: v.double() for k, v in i32.items()}
    g = {k: dev(v) for k, v in i32.items()}
    y_plain = run_attention(x, state, dim, heads)
    call, outs, _keep = row_call(x, state, dim, heads)
    for row in AC.rows_of(n):
        tag = f"{case} row {row}"
        r, a = run_stage(g, pad + row, heads)
        ref_r, ref_a = AR.st_attn_row(*(i64[k] for k in ("qkv", "ql", "kl", "z", "lse3")), pad + row, heads)
        f32_r, f32_a = AR.st_attn_row(*(i32[k] for k in ("qkv", "ql", "kl", "z", "lse3")), pad + row, heads)
        judge(grp, tag, "stage r", r, ref_r, f32_r, fails)
        judge(grp, tag, "stage attn", a, ref_a, f32_a, fails)
        # over all np columns the row sums to sum_i r_i (each softmax row of ql k^T sums to 1), relative to sum_i |r_i|
        # (the kernel's row sum against the kernel's own sum of r; e32: the gap the fp32 restatement leaves between its two)
        rd, scale = r.double().cpu(), float(ref_r.abs().sum(-1).max())
        gap32 = f32_a.double().sum(-1) - f32_r.double().sum(-1)
        judge(grp, tag, "stage sum", a.double().cpu().sum(-1), rd.sum(-1), rd.sum(-1) + gap32, fails, scale=scale)
        # the whole call: y with the bits of rrt_nystrom_attention_f32, the n real columns of the row
        y, aw, _ = twice(call(row), outs, "rrt_nystrom_attention_row_f32")
        assert torch.equal(y.t.view(torch.int32), y_plain.view(torch.int32)), f"{tag}: y differs from rrt_nystrom_attention_f32"
        judge(grp, tag, "attn", aw.t, AR.attn_row(r64, heads, row, n)["attn"], AR.attn_row(r32, heads, row, n)["attn"], fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dim,heads,n,gain", AC.GOLDEN_CASES, ids=lambda v: str(v))
def test_whole_call_against_the_reference_rows(dim, heads, n, gain):
    gold, key = load_golden("transmil_attn_row"), AC.golden_key(dim, heads, n, gain)
    state, x = TC.attn_inputs(dim, heads, n, gain)
    call, outs, _keep = row_call(x, state, dim, heads)
    _y, a, _ = twice(call(0), outs, "rrt_nystrom_attention_row_f32")
    ref, fails = torch.from_numpy(gold[key + "/attn"]), []
    judge("reference rows", key, "attn golden", a.t[:, 1:], ref, ref, fails, e32_floor=float(gold[key + "/e32"]))
    assert not fails, "\n".join(fails)


def test_a_dirtied_workspace_changes_nothing():
    state, x = TC.attn_inputs(128, 2, 513, 6.0)
    res = []
    for fill in (0xA5, 0xFF):                            # 0xFF: NaN patterns everywhere in the workspace
        call, outs, _keep = row_call(x, state, 128, 2, fill)
        y, a, _ = twice(call(256), outs, "rrt_nystrom_attention_row_f32")
        res.append((y.t, a.t))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))


# ------------------------------------------------------------------ the module and the model
def test_attention_row_module():
    from rrt_mil_amd import NystromAttention
    n = 513
    state, x, r64, r32 = reference(128, 2, n, 1.0)
    mod = NystromAttention(128, heads=2)
    mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    mod = mod.cuda().eval()
    xd = torch.from_numpy(x).cuda()[None]
    fails = []
    with torch.no_grad():
        y = mod(xd)
        for row in AC.rows_of(n):
            y2, a = mod.attention_row(xd, row=row)
            y3, a3 = mod.attention_row(xd, row=row)
            assert y2.shape == (1, n, 128) and a.shape == (1, 2, n)
            assert torch.equal(y2, y) and torch.equal(y3, y) and torch.equal(a, a3)
            judge("NystromAttention module", f"d128 h2 n513 row {row}", "attn", a[0], AR.attn_row(r64, 2, row, n)["attn"],
                  AR.attn_row(r32, 2, row, n)["attn"], fails)
        assert torch.equal(mod.attention_row(xd)[1], mod.attention_row(xd, row=0)[1])
        for bad in (-1, n):
            with pytest.raises(ValueError, match="row"):
                mod.attention_row(xd, row=bad)
        with pytest.raises(ValueError):
            mod.attention_row(torch.cat([xd, xd]))
        with pytest.raises(NotImplementedError, match="return_attn"):     # the existing refusals stay
            mod(xd, return_attn=True)
        with pytest.raises(NotImplementedError, match="mask"):
            mod(xd, mask=torch.ones(1, n, dtype=torch.bool, device="cuda"))
    for enabled in (False, True):                                          # the map is an inference output either way
        mod.enable_training(enabled)
        with pytest.raises(NotImplementedError, match="no_grad"):
            mod.attention_row(xd)                                          # parameters require grad and grad mode is on
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("input_dim,act,N", AC.MODEL_CASES, ids=lambda v: str(v))
def test_transmil_attention_maps(input_dim, act, N):
    model, state, x = make_model(input_dim, act, N)
    r64, r32 = (AR.transmil_attn(x, state, act, dtype=dt) for dt in (torch.float64, torch.float32))
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        plain, feat_plain = model.forward_bag(xd, return_features=True)
        logits, attn = model.forward_bag(xd, return_attn=True)
        logits2, feat2, attn2 = model.forward_bag(xd, return_features=True, return_attn=True)
    assert attn.shape == (2, 8, N) and attn.dtype == torch.float32
    assert torch.equal(logits, plain) and torch.equal(logits2, plain) and torch.equal(feat2, feat_plain)
    assert torch.equal(attn, attn2), "two runs differ in their bits"
    case, fails = f"TransMIL({input_dim}, {act}) N{N}", []
    for layer in range(2):
        judge("TransMIL", case, f"attn layer {layer + 1}", attn[layer], r64["attn"][layer], r32["attn"][layer], fails)
    assert not fails, "\n".join(fails)


def test_transmil_return_attn_api():
    """model(x, return_attn=True) == forward_bag == forward_bags, bit for bit; a dirtied workspace changes nothing; what must
    raise, raises, with or without enable_training()"""
    from rrt_mil_amd import TransMIL
    model, _state, x = make_model(64, "gelu", 250)
    xd = torch.from_numpy(x).cuda()
    x2 = torch.from_numpy(TC.model_inputs(64, 10)[1]).cuda()
    with torch.no_grad():
        plain = model.forward_bag(xd)
        la, a = model.forward_bag(xd, return_attn=True)
        assert torch.equal(la, plain) and a.shape == (2, 8, 250)
        for got in (model(xd, return_attn=True), model(xd[None], return_attn=True)):
            assert torch.equal(got[0], la) and torch.equal(got[1], a)
        b = model.forward_bags([xd, x2[None], xd], return_attn=True)
        lb, ab = model.forward_bag(x2, return_attn=True)
        assert ab.shape == (2, 8, 10)
        assert all(torch.equal(b[i][0], la) and torch.equal(b[i][1], a) for i in (0, 2))
        assert torch.equal(b[1][0], lb) and torch.equal(b[1][1], ab)
        assert torch.equal(model.forward_bags([x2])[0], lb)                # without the request: logits only, as before
        model._ws.fill_(0xFF)                                               # NaN patterns everywhere in the workspace
        la2, a2 = model.forward_bag(xd, return_attn=True)
        assert torch.equal(la2, la) and torch.equal(a2, a)
        assert torch.equal(model.forward_bag(xd), plain)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert torch.equal(model.forward_bag(xd, return_attn=True)[1], a)     # exact fp32 under autocast as well
        with pytest.raises(ValueError):
            model(torch.stack([xd, xd]), return_attn=True)
    for enabled in (False, True):
        model.enable_training(enabled)
        with pytest.raises(NotImplementedError, match="no_grad"):
            model(xd, return_attn=True)                                     # needs a graph: the map is an inference output
        with pytest.raises(NotImplementedError, match="no_grad"):
            model.forward_bags([xd], return_attn=True)
    model.enable_training(False)
    drop = TransMIL(64, 2, True, "gelu").cuda().train()                     # stochastic: train() with dropout
    for enabled in (False, True):
        drop.enable_training(enabled)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="no_grad"):
            drop(xd, return_attn=True)
