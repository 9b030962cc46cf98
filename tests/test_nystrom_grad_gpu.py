"""GPU (-m gpu): the backward of Nystrom attention (csrc/nystrom_bwd.hip), one stage at a time and as a whole, the
``enable_training()`` path of NystromAttention and of TransMIL -- against float64 autograd of the restatement
tests/nystrom_ref.py (pinned to the reference's own float64 gradients by tests/test_nystrom_grad_cpu.py), never against
another kernel.

Error of a gradient: max |got - ref64| / max |ref64|, relative to the gradient's own largest entry (every judged quantity must
have max |ref64| > 1e-4).  Bound: max(2e-5, 8 x e32), e32 = the fp32 CPU autograd of the same function on the same inputs
against the float64 one -- measured here, never read off a kernel.  A stage's inputs are the fp32 roundings of the float64
run's tensors; the stages that add are checked on a seeded prefill of the gradient's own size.  The pinv backward is judged
together with the softmax backward of a2 (d_ql, d_kl): d_a2 itself is not a testable quantity, which row attains the largest
row sum is a matter of rounding.

Every output is NaN-filled with canary rows behind it, workspaces and stashes have exactly the queried size with canary bytes
behind them, every call runs twice and must give the same bits.  The case lists are module data of
tests/nystrom_grad_cases.py; importing this module needs no device.  With RRT_NYSTROM_GRAD_ERRORS_OUT=<file> the module writes
its error table (kept as profiles/nystrom_grad_errors.txt)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nystrom_grad_cases as GC
import nystrom_ref as R
import transmil_cases as TC
from conftest import load_golden
from rrt_mil_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad")]

TOL = 2e-5
E32_FACTOR = 8.0
MIN_REF = 1e-4
CANARY = 1234.5
RECORDS = []                      # (group, quantity, e32, kernel error), both relative


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_NYSTROM_GRAD_ERRORS_OUT")
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


def error_table(records):
    rows = {}
    for grp, what, e32, err in records:
        n, w32, werr, wr = rows.get((grp, what), (0, 0.0, 0.0, 0.0))
        rows[(grp, what)] = (n + 1, max(w32, e32), max(werr, err), max(wr, err / e32 if e32 else 0.0))
    lines = [f"{'case group':34s} {'quantity':22s} {'cases':>5s} {'worst e32':>10s} {'worst err':>10s} {'worst err/e32':>13s}"]
    for (grp, what), (n, w32, werr, wr) in sorted(rows.items()):
        lines.append(f"{grp:34s} {what:22s} {n:5d} {w32:10.2e} {werr:10.2e} {wr:13.2f}")
    return "\n".join(lines) + "\n"


def judge(grp, case, what, got, ref64, ref32, fails, e32_floor=0.0):
    """one gradient against float64, relative to its own largest entry: bound max(TOL, 8 x e32)"""
    ref64, ref32 = ref64.detach().double(), ref32.detach().double()
    big = float(ref64.abs().max())
    assert big > MIN_REF, (case, what, big)
    e32 = max(float((ref32 - ref64).abs().max()) / big, e32_floor)
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref64.shape), (case, what, got.shape, ref64.shape)
    err = float((got - ref64).abs().max()) / big if bool(torch.isfinite(got).all()) else float("inf")
    bound = max(TOL, E32_FACTOR * e32)
    RECORDS.append((grp, what, e32, err))
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e} max|ref| {big:.2e}")
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


def dev(t):
    return torch.as_tensor(t).detach().to(torch.float32).contiguous().cuda()


class Out:
    """an output of `shape` with 8 canary rows behind it: NaN-filled, or holding `prefill` (the stages that add)"""

    def __init__(self, *shape, prefill=None):
        row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        self.buf = torch.full((shape[0] + 8, row), float("nan"), dtype=torch.float32, device="cuda")
        self.buf[shape[0]:] = CANARY
        self.shape = shape
        if prefill is not None:
            self.t.copy_(prefill)

    @property
    def t(self):
        return self.buf[:self.shape[0]].view(self.shape)

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.shape[0]:] == CANARY).all()), f"{what}: wrote behind its output"


class Ws:
    """a workspace or stash of exactly `nbytes` bytes, dirtied, with 256 canary bytes behind it"""

    def __init__(self, nbytes, fill=0xA5):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 256,), fill, dtype=torch.uint8, device="cuda")
        self.buf[self.n:] = 0x5C

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.n:] == 0x5C).all()), f"{what}: wrote behind its workspace"


def stream():
    return torch.cuda.current_stream().cuda_stream


def twice(call, outs, what):
    """run `call` twice into fresh outputs built by `outs(run)` (the second run's workspaces are dirtied with another
    pattern); same bits; returns the first run's outputs"""
    res = []
    for run in range(2):
        o = outs(run)
        _lib.check(call(*o), what)
        torch.cuda.synchronize()
        for x in o:
            x.check(what)
        res.append(o)
    for a, b in zip(*res):
        if isinstance(a, Out):
            assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)), f"{what}: two runs differ in their bits"
    return res[0]


FILLS = (0xA5, 0xFF)


def size_of(fn, *args):
    need = C.c_size_t()
    _lib.check(fn(*args, C.byref(need)), fn.__name__)
    return need.value


# ------------------------------------------------------------------ references: autograd of the restatement, float64 and fp32
def grads_of(fn, inputs, cot, dtype):
    """d (sum fn(*inputs) . cot) / d inputs in `dtype` (None inputs pass through and get no gradient)"""
    xs = [None if t is None else t.detach().to(dtype).requires_grad_(True) for t in inputs]
    out = fn(*xs)
    outs, cots = (out, cot) if isinstance(out, tuple) else ((out,), (cot,))
    sum((o * c.to(dtype)).sum() for o, c in zip(outs, cots)).backward()
    return [None if x is None else x.grad for x in xs]


def both(fn, inputs, cot):
    return grads_of(fn, inputs, cot, torch.float64), grads_of(fn, inputs, cot, torch.float32)


@functools.lru_cache(maxsize=2)
def forward64(dim, heads, n, gain):
    """the float64 run's stage tensors rounded to fp32 (the stages' inputs); computed once per case"""
    state, x = TC.attn_inputs(dim, heads, n, gain)
    with torch.no_grad():
        r64 = R.nystrom(x, state, heads, dtype=torch.float64)
    return state, x, {k: r64[k].float() for k in ("qkv", "ql", "kl", "a2", "av", "z", "wz")}


def cot(case, name, shape):
    return torch.from_numpy(GC.cotangent(f"{name}/{case}", shape))


def prefill_like(case, name, ref64):
    """a seeded prefill of the gradient's own size"""
    return (cot(case, "prefill_" + name, ref64.shape) * float(ref64.abs().max())).float()


# ------------------------------------------------------------------ the stage launchers
def run_output_backward(qkv, kl, wz, conv_w, d_o, heads):
    lib, npad = _lib.load(), qkv.shape[0]
    ks = conv_w.shape[1] if conv_w is not None else 0
    need = size_of(lib.rrt_nystrom_output_backward_workspace_size, npad, heads)
    outs = twice(lambda a, b, c, d, w: lib.rrt_nystrom_output_backward_f32(
        qkv.data_ptr(), kl.data_ptr(), wz.data_ptr(), conv_w.data_ptr() if conv_w is not None else None, d_o.data_ptr(),
        a.ptr(), b.ptr(), c.ptr(), d.ptr() if conv_w is not None else None, npad, heads, ks, w.ptr(), w.n, stream()),
        lambda run: (Out(npad, 3 * heads * 64), Out(heads, 256, 64), Out(heads, 256, 64), Out(heads, max(ks, 1)),
                     Ws(need, FILLS[run])), "rrt_nystrom_output_backward_f32")
    return [o.t for o in outs[:4]]


def run_zav_backward(z, av, d_wz, heads):
    lib = _lib.load()
    d_z, d_av = twice(lambda a, b: lib.rrt_nystrom_zav_backward_f32(z.data_ptr(), av.data_ptr(), d_wz.data_ptr(), a.ptr(), b.ptr(),
                                                                    heads, stream()),
                      lambda run: (Out(heads, 256, 256), Out(heads, 256, 64)), "rrt_nystrom_zav_backward_f32")
    return d_z.t, d_av.t


def run_landmark_attn_backward(qkv, ql, d_av, prefill, heads):
    lib, npad = _lib.load(), qkv.shape[0]
    need = size_of(lib.rrt_nystrom_landmark_attn_backward_workspace_size, npad, heads)
    d_qkv, d_ql, _ = twice(lambda a, b, w: lib.rrt_nystrom_landmark_attn_backward_f32(
        qkv.data_ptr(), ql.data_ptr(), d_av.data_ptr(), a.ptr(), b.ptr(), npad, heads, w.ptr(), w.n, stream()),
        lambda run: (Out(npad, 3 * heads * 64, prefill=prefill), Out(heads, 256, 64), Ws(need, FILLS[run])),
        "rrt_nystrom_landmark_attn_backward_f32")
    return d_qkv.t, d_ql.t


def run_pinv_sim_backward(ql, kl, d_z, heads, iters):
    lib = _lib.load()
    need = size_of(lib.rrt_nystrom_pinv_sim_backward_workspace_size, heads, iters)
    d_ql, d_kl, _ = twice(lambda a, b, w: lib.rrt_nystrom_pinv_sim_backward_f32(
        ql.data_ptr(), kl.data_ptr(), d_z.data_ptr(), a.ptr(), b.ptr(), heads, iters, w.ptr(), w.n, stream()),
        lambda run: (Out(heads, 256, 64), Out(heads, 256, 64), Ws(need, FILLS[run])), "rrt_nystrom_pinv_sim_backward_f32")
    return d_ql.t, d_kl.t


def run_landmarks_backward(d_ql, d_kl, prefill, npad, heads):
    lib = _lib.load()
    (d_qkv,) = twice(lambda a: lib.rrt_nystrom_landmarks_backward_f32(d_ql.data_ptr(), d_kl.data_ptr(), a.ptr(), npad, heads,
                                                                      stream()),
                     lambda run: (Out(npad, 3 * heads * 64, prefill=prefill),), "rrt_nystrom_landmarks_backward_f32")
    return d_qkv.t


def nystrom_desc(dim, heads, iters=6, residual=True):
    d = _lib.NystromDesc()
    d.dim, d.heads, d.dim_head, d.num_landmarks, d.pinv_iterations = dim, heads, 64, 256, iters
    d.residual, d.residual_conv_kernel = int(residual), 33
    return d


PARAMS = ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias", "res_conv.weight")


def run_attention_train(x, state, dy, dim, heads, iters=6, residual=True):
    """forward_train + backward through the C ABI -> {y, dx, the four parameter gradients}; y is held to the bits of
    rrt_nystrom_attention_f32, the gradients to the bits of a second run with another pattern in stash and workspace"""
    lib, n = _lib.load(), x.shape[0]
    d, w = nystrom_desc(dim, heads, iters, residual), _lib.NystromWeights()
    ts = [dev(state[k]) if (residual or k != "res_conv.weight") else None for k in PARAMS]
    w.qkv_w, w.out_w, w.out_b, w.conv_w = (t.data_ptr() if t is not None else None for t in ts)
    xd, dyd = dev(x), dev(dy)
    sb, wb = C.c_size_t(), C.c_size_t()
    _lib.check(lib.rrt_nystrom_train_sizes(C.byref(d), n, C.byref(sb), C.byref(wb)), "rrt_nystrom_train_sizes")
    fw = size_of(lib.rrt_nystrom_workspace_size, C.byref(d), n)
    y0, ws0 = Out(n, dim), Ws(fw)
    _lib.check(lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), xd.data_ptr(), y0.ptr(), n, ws0.ptr(), ws0.n, stream()),
               "rrt_nystrom_attention_f32")
    runs = []
    for run in range(2):
        stash, ws, y, dx = Ws(sb.value, FILLS[run]), Ws(wb.value, FILLS[run]), Out(n, dim), Out(n, dim)
        gs = [Out(*t.shape) if t is not None else None for t in ts]
        g = _lib.NystromGrads()
        g.qkv_w, g.out_w, g.out_b, g.conv_w = (o.ptr() if o is not None else None for o in gs)
        _lib.check(lib.rrt_nystrom_attention_forward_train_f32(C.byref(d), C.byref(w), xd.data_ptr(), y.ptr(), n, stash.ptr(),
                                                               stash.n, stream()), "rrt_nystrom_attention_forward_train_f32")
        _lib.check(lib.rrt_nystrom_attention_backward_f32(C.byref(d), C.byref(w), xd.data_ptr(), dyd.data_ptr(), stash.ptr(),
                                                          stash.n, C.byref(g), dx.ptr(), n, ws.ptr(), ws.n, stream()),
                   "rrt_nystrom_attention_backward_f32")
        torch.cuda.synchronize()
        for o in (stash, ws, y, dx, y0, ws0, *[o for o in gs if o is not None]):
            o.check("rrt_nystrom_attention_{forward_train,backward}_f32")
        assert torch.equal(y.t.view(torch.int32), y0.t.view(torch.int32)), "forward_train's y differs from the inference call's"
        runs.append({"y": y.t, "dx": dx.t, **{k: o.t for k, o in zip(PARAMS, gs) if o is not None}})
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), f"{k}: two runs differ in their bits"
    # without dx: the parameter gradients keep their bits
    stash, ws, y = Ws(sb.value), Ws(wb.value), Out(n, dim)
    gs = [Out(*t.shape) if t is not None else None for t in ts]
    g = _lib.NystromGrads()
    g.qkv_w, g.out_w, g.out_b, g.conv_w = (o.ptr() if o is not None else None for o in gs)
    _lib.check(lib.rrt_nystrom_attention_forward_train_f32(C.byref(d), C.byref(w), xd.data_ptr(), y.ptr(), n, stash.ptr(),
                                                           stash.n, stream()), "rrt_nystrom_attention_forward_train_f32")
    _lib.check(lib.rrt_nystrom_attention_backward_f32(C.byref(d), C.byref(w), xd.data_ptr(), dyd.data_ptr(), stash.ptr(),
                                                      stash.n, C.byref(g), None, n, ws.ptr(), ws.n, stream()),
               "rrt_nystrom_attention_backward_f32")
    torch.cuda.synchronize()
    for k, o in zip(PARAMS, gs):
        if o is not None:
            assert torch.equal(o.t.view(torch.int32), runs[0][k].view(torch.int32)), f"{k}: differs without dx"
    return runs[0]


def attention_reference(x, state, dy, heads, iters, residual, dtype):
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).to(dtype).requires_grad_(True)
    (R.nystrom(xd, p, heads, iters=iters, residual=residual, dtype=dtype)["y"] * dy.to(dtype)).sum().backward()
    out = {k: p[k].grad for k in PARAMS if p[k].grad is not None}
    out["dx"] = xd.grad
    return out


def judge_attention(grp, case, got, x, state, dy, heads, iters, residual, fails):
    r64, r32 = (attention_reference(x, state, dy, heads, iters, residual, dt) for dt in (torch.float64, torch.float32))
    assert set(r64) == set(got) - {"y"}, (set(r64), set(got))
    for k in r64:
        judge(grp, case, "attn " + k, got[k].reshape(r64[k].shape), r64[k], r32[k], fails)


# ------------------------------------------------------------------ stage and whole-attention cases
@pytest.mark.parametrize("dim,heads,n,gain", GC.STAGE_CASES, ids=lambda v: str(v))
def test_backward_stages_and_attention(dim, heads, n, gain):
    state, x, i32 = forward64(dim, heads, n, gain)
    case, grp = f"d{dim} h{heads} n{n} g{gain:g}", f"d{dim} h{heads} gain {gain:g}"
    key = GC.case_key(dim, heads, n, gain)
    g = {k: dev(v) for k, v in i32.items()}
    npad, hd = i32["qkv"].shape[0], heads * 64
    conv32 = torch.from_numpy(state["res_conv.weight"]).reshape(heads, -1)
    fails = []

    # output
    d_o = cot(key, "d_o", (npad, hd))
    for conv in (conv32, None):
        tag = "" if conv is not None else " no conv"
        r64, r32 = both(lambda q, k_, w_, c: R.st_output(q, k_, w_, heads, c), (i32["qkv"], i32["kl"], i32["wz"], conv), d_o)
        d_qkv, d_kl, d_wz, d_conv = run_output_backward(g["qkv"], g["kl"], g["wz"], dev(conv) if conv is not None else None,
                                                        dev(d_o), heads)
        if conv is None:
            assert not bool(d_qkv[:, 2 * hd:].any()), "no conv: the v third must be zero"
        assert not bool(d_qkv[:, hd:2 * hd].any()), "the k third must be zeroed"
        judge(grp, case, "output d_qkv" + tag, d_qkv, r64[0], r32[0], fails)
        judge(grp, case, "output d_kl" + tag, d_kl, r64[1], r32[1], fails)
        judge(grp, case, "output d_wz" + tag, d_wz, r64[2], r32[2], fails)
        if conv is not None:
            judge(grp, case, "output d_conv_w", d_conv, r64[3], r32[3], fails)

    # zav
    d_wz = cot(key, "d_wz", (heads, 256, 64))
    r64, r32 = both(R.st_zav, (i32["z"], i32["av"]), d_wz)
    for name, got, a, b in zip(("zav d_z", "zav d_av"), run_zav_backward(g["z"], g["av"], dev(d_wz), heads), r64, r32):
        judge(grp, case, name, got, a, b, fails)

    # landmark attention over the keys: d_ql written, dk / dv added onto a prefill, the q third untouched
    d_av = cot(key, "d_av", (heads, 256, 64))
    r64, r32 = both(lambda q, l_: R.st_landmark_attn(q, l_, heads), (i32["qkv"], i32["ql"]), d_av)
    assert not bool(r64[0][:, :hd].any())
    pre = prefill_like(key, "lattn", r64[0])
    d_qkv, d_ql = run_landmark_attn_backward(g["qkv"], g["ql"], dev(d_av), pre, heads)
    assert torch.equal(d_qkv[:, :hd].cpu(), pre[:, :hd]), "landmark_attn_backward touched the q third"
    judge(grp, case, "lattn d_qkv (k, v)", d_qkv, pre.double() + r64[0], (pre + r32[0]), fails)
    judge(grp, case, "lattn d_ql", d_ql, r64[1], r32[1], fails)

    # pinv through the landmark softmax
    for iters in GC.PINV_ITERATIONS:
        d_z = cot(key, f"d_z{iters}", (heads, 256, 256))
        r64, r32 = both(lambda a, b: R.pinv_iter(R.st_landmark_sim(a, b), iters), (i32["ql"], i32["kl"]), d_z)
        d_ql, d_kl = run_pinv_sim_backward(g["ql"], g["kl"], dev(d_z), heads, iters)
        judge(grp, case, f"pinv_sim d_ql it{iters}", d_ql, r64[0], r32[0], fails)
        judge(grp, case, f"pinv_sim d_kl it{iters}", d_kl, r64[1], r32[1], fails)

    # landmarks: the 1 / l shares added onto a prefill
    d_l = (cot(key, "d_ql", (heads, 256, 64)), cot(key, "d_kl", (heads, 256, 64)))
    r64, r32 = both(lambda q: R.st_landmarks(q, heads), (i32["qkv"],), d_l)
    pre = prefill_like(key, "landmarks", r64[0])
    d_qkv = run_landmarks_backward(dev(d_l[0]), dev(d_l[1]), pre, npad, heads)
    assert torch.equal(d_qkv[:, 2 * hd:].cpu(), pre[:, 2 * hd:]), "landmarks_backward touched the v third"
    judge(grp, case, "landmarks d_qkv (q, k)", d_qkv, pre.double() + r64[0], pre + r32[0], fails)

    # the whole attention
    dy = cot(key, "dy", (n, dim))
    got = run_attention_train(x, state, dy, dim, heads)
    judge_attention(grp, case, got, x, state, dy, heads, 6, True, fails)
    if (dim, heads, n, gain) in GC.GOLDEN_ATTN_CASES:
        gold = load_golden("transmil_grad")
        for k in (*PARAMS, "dx"):
            ref = torch.from_numpy(gold[f"attn/{key}/{k}"])
            g2 = got[k].cpu()
            rows = torch.stack([g2[0], g2[-1]]) if k == "dx" else GC.golden_rows(g2)
            judge(grp, case, f"attn {k} golden", rows, ref, ref, fails, e32_floor=float(gold[f"attn/{key}/e32/{k}"]))
    assert not fails, "\n".join(fails)


def test_pinv_den_gradient_with_tied_columns():
    """Two heads; in head 1 three key landmarks are the same row and draw every query: their column sums are equal bit for bit
    and the largest over BOTH heads, so the gradient through den is shared among them (torch's rule for a tied maximum) and
    reaches head 0 through the one scalar.  A backward that drops that gradient, or takes den per head, is far outside."""
    ql = torch.from_numpy(GC.cotangent("ties/ql", (2, 256, 64))).float()
    kl = torch.from_numpy(GC.cotangent("ties/kl", (2, 256, 64))).float() * 0.5
    u = torch.full((64,), 0.25)
    ql[1] += u
    kl[1, 9] = kl[1, 77] = kl[1, 200] = 2.0 * u
    a2 = R.st_landmark_sim(ql, kl)
    cs = a2.sum(-2)
    assert int((cs == cs.max()).sum()) == 3 and bool((cs[1, [9, 77, 200]] == cs.max()).all())
    fails = []
    for iters in GC.PINV_ITERATIONS:
        d_z = cot("ties", f"d_z{iters}", (2, 256, 256))
        r64, r32 = both(lambda a, b: R.pinv_iter(R.st_landmark_sim(a, b), iters), (ql, kl), d_z)
        d_ql, d_kl = run_pinv_sim_backward(dev(ql), dev(kl), dev(d_z), 2, iters)
        judge("pinv tied columns", "three tied columns", f"pinv_sim d_ql it{iters}", d_ql, r64[0], r32[0], fails)
        judge("pinv tied columns", "three tied columns", f"pinv_sim d_kl it{iters}", d_kl, r64[1], r32[1], fails)
        if iters == 1:                                       # the case does tell a per-head den apart
            per_head = torch.cat([grads_of(lambda a, b: R.pinv_iter(R.st_landmark_sim(a, b), iters),
                                           (ql[h:h + 1], kl[h:h + 1]), d_z[h:h + 1], torch.float64)[1] for h in range(2)])
            assert float((per_head - r64[1]).abs().max()) / float(r64[1].abs().max()) > 100 * TOL
    assert not fails, "\n".join(fails)


def test_attention_backward_without_residual_and_other_iterations():
    state, x = TC.attn_inputs(128, 2, 257, 1.0)
    fails = []
    for iters, residual in ((1, True), (6, False)):
        dy = cot("options", f"dy{iters}", x.shape)
        got = run_attention_train(x, state, dy, 128, 2, iters=iters, residual=residual)
        assert ("res_conv.weight" in got) == residual
        judge_attention("attention options", f"iters {iters} residual {residual}", got, x, state, dy, 2, iters, residual, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ the module
def make_attention(dim, heads, n, gain, dropout=0.):
    from rrt_mil_amd import NystromAttention
    state, x = TC.attn_inputs(dim, heads, n, gain)
    mod = NystromAttention(dim, heads=heads, dropout=dropout)
    mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return mod.cuda(), state, x


def test_nystrom_module_trains():
    mod, state, x = make_attention(128, 2, 513, 1.0)
    mod.eval()
    xd = torch.from_numpy(x).cuda()[None].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="no_grad"):
        mod(xd)                                              # off by default: the refusal is unchanged
    with torch.no_grad():
        y_eval = mod(xd)
    assert mod.enable_training() is mod
    dy = cot("module", "dy", x.shape)
    y = mod(xd)
    assert y.shape == (1, 513, 128) and y.requires_grad and torch.equal(y.detach(), y_eval)
    (y[0] * dy.cuda()).sum().backward()
    got = {k: p.grad for k, p in mod.named_parameters()}
    assert set(got) == set(PARAMS) and all(v is not None for v in got.values()) and xd.grad is not None
    got["dx"] = xd.grad[0]
    fails = []
    judge_attention("NystromAttention module", "d128 h2 n513", got, x, state, dy, 2, 6, True, fails)
    assert not fails, "\n".join(fails)
    with torch.no_grad():
        assert torch.equal(mod(xd), y_eval)                  # no graph needed: the one-call path
    for bad in (dict(mask=torch.ones(1, 513, dtype=torch.bool, device="cuda")), dict(return_attn=True)):
        with pytest.raises(NotImplementedError):
            mod(xd, **bad)
    # under autocast: fp32 all the same
    mod.zero_grad()
    x2 = xd.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y2 = mod(x2)
        assert y2.dtype == torch.float32 and torch.equal(y2.detach(), y_eval)
        (y2[0] * dy.cuda()).sum().backward()
    assert torch.equal(x2.grad, xd.grad)
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, got[k]), k


def test_nystrom_module_dropout_is_torchs():
    mod, _state, x = make_attention(128, 2, 257, 1.0, dropout=0.1)
    xd = torch.from_numpy(x).cuda()[None]
    with torch.no_grad():
        y_eval = mod.eval()(xd)
        with pytest.raises(NotImplementedError, match="eval"):
            mod.train()(xd)
    mod.enable_training().train()
    torch.manual_seed(7)
    y = mod(xd)
    torch.manual_seed(7)
    want = F.dropout(y_eval, 0.1, True)
    assert y.requires_grad and torch.equal(y.detach(), want) and not torch.equal(want, y_eval)
    y.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in mod.parameters())


# ------------------------------------------------------------------ the model
def make_model(input_dim, act, N, dropout=False):
    from rrt_mil_amd import TransMIL
    state, x = TC.model_inputs(input_dim, N)
    model = TransMIL(input_dim, 2, dropout, act)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return model.cuda().eval(), state, x


def model_reference(x, state, act, dtype):
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).to(dtype).requires_grad_(True)
    F.cross_entropy(R.transmil(xd, p, act, dtype=dtype)["logits"][None], torch.tensor([GC.LABEL])).backward()
    return {**{k: v.grad for k, v in p.items()}, "dx": xd.grad}


def model_backward(model, x):
    model.zero_grad(set_to_none=True)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    logits = model(xd)
    F.cross_entropy(logits, torch.tensor([GC.LABEL], device="cuda")).backward()
    return logits.detach(), {**{k: p.grad.clone() for k, p in model.named_parameters()}, "dx": xd.grad.clone()}


@pytest.mark.parametrize("input_dim,act,N", GC.MODEL_CASES, ids=lambda v: str(v))
def test_transmil_model_gradients(input_dim, act, N):
    model, state, x = make_model(input_dim, act, N)
    with torch.no_grad():
        one_call = model(torch.from_numpy(x).cuda())
    model.enable_training()
    logits, got = model_backward(model, x)
    logits2, again = model_backward(model, x)
    assert len(got) == 26 and logits.shape == (1, 2) and torch.equal(logits, logits2)
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{k}: two backward passes differ in their bits"
    with torch.no_grad():
        assert torch.equal(model(torch.from_numpy(x).cuda()), one_call)      # no graph: the one-call path's bits
    r64, r32 = (model_reference(x, state, act, dt) for dt in (torch.float64, torch.float32))
    case, fails = f"TransMIL({input_dim}, {act}) N{N}", []
    judge("TransMIL", case, "logits", logits[0], r64_logits(x, state, act), r64_logits(x, state, act, torch.float32), fails)
    for k in r64:
        judge("TransMIL", case, k, got[k].reshape(r64[k].shape), r64[k], r32[k], fails)
    if (input_dim, act, N) in GC.GOLDEN_MODEL_CASES:
        gold, key = load_golden("transmil_grad"), "model/" + GC.model_key(input_dim, act, N)
        for k in r64:
            ref = torch.from_numpy(gold[f"{key}/{k}"])
            g2 = got[k].cpu()
            rows = torch.stack([g2[0], g2[-1]]) if k == "dx" else GC.golden_rows(g2)
            judge("TransMIL", case, k + " golden", rows, ref, ref, fails, e32_floor=float(gold[f"{key}/e32/{k}"]))
    assert not fails, "\n".join(fails)


def r64_logits(x, state, act, dtype=torch.float64):
    with torch.no_grad():
        return R.transmil(x, state, act, dtype=dtype)["logits"]


def test_transmil_training_api():
    model, _state, x = make_model(64, "gelu", 37, dropout=True)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        a = model(xd)
    # off (the default): the refusals are unchanged
    with pytest.raises(NotImplementedError, match="no_grad"):
        model(xd)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="eval"):
        model.train()(xd)
    model.eval().enable_training()
    with torch.no_grad():
        assert torch.equal(model(xd), a) and torch.equal(model.forward_bag(xd), a)
        assert torch.equal(model.forward_bags([xd, xd[None]])[1], a)
    logits, feat = model.forward_bag(xd, return_features=True)
    assert logits.requires_grad and feat.shape == (1 + 49, 512) and R.rel_err(logits.detach(), a) < 1e-5
    with pytest.raises(ValueError):
        model(torch.stack([xd, xd]))
    # one optimiser step in train() (dropout in _fc1 and in both attentions) runs and changes every parameter
    model.train()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    torch.manual_seed(3)
    loss = F.cross_entropy(model(xd), torch.tensor([GC.LABEL], device="cuda"))
    loss.backward()
    assert bool(torch.isfinite(loss))
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), k
    opt.step()
    for k, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[k]), f"{k} did not change"
    model.enable_training(False)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="eval"):
        model(xd)
