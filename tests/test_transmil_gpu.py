"""GPU (-m gpu): the Nystrom-attention kernels of csrc/nystrom.hip, one stage at a time and as a whole, and the TransMIL model
around them, against the float64 restatement tests/nystrom_ref.py (pinned to the reference's own float64 run by
tests/test_transmil_cpu.py) -- never against another kernel.

Bound per quantity, the project's stage rule: err <= max(2e-5, 8 x e32) relative to max(1, max |float64 reference|), e32 = the
error of the same restatement evaluated in plain fp32 on the CPU on the same inputs -- measured here, never read off a kernel.
A stage's inputs are the fp32 roundings of the float64 run's tensors, and its float64 / fp32 references are computed from
exactly those inputs.  The whole-attention and whole-model cases are also held to the reference's golden rows / logits, with
the reference's own recorded e32 in the bound.

Every output is NaN-filled with canary rows behind it, workspaces have exactly the queried size with canary bytes behind them,
every call runs twice and must give the same bits.  The case lists are module data of tests/transmil_cases.py
(tests/test_transmil_cpu.py checks on the CPU that they cover what is claimed); importing this module needs no device.
With RRT_NYSTROM_STAGE_ERRORS_OUT=<file> the module writes its error table (kept as profiles/nystrom_stage_errors.txt)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import nystrom_ref as R
import transmil_cases as TC
from conftest import load_golden
from rrt_mil_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 2e-5
E32_FACTOR = 8.0
CANARY = 1234.5
RECORDS = []                      # (group, quantity, e32, kernel error), both relative


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_NYSTROM_STAGE_ERRORS_OUT")
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
    lines = [f"{'case group':34s} {'quantity':14s} {'cases':>5s} {'worst e32':>10s} {'worst err':>10s} {'worst err/e32':>13s}"]
    for (grp, what), (n, w32, werr, wr) in sorted(rows.items()):
        lines.append(f"{grp:34s} {what:14s} {n:5d} {w32:10.2e} {werr:10.2e} {wr:13.2f}")
    return "\n".join(lines) + "\n"


def judge(grp, case, what, got, ref64, ref32, fails, e32_floor=0.0):
    """one quantity against float64: bound max(TOL, 8 x e32); e32_floor: the reference's own recorded e32 (golden cases)"""
    e32 = max(R.rel_err(ref32, ref64), e32_floor)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (case, what, got.shape, ref64.shape)
    err = R.rel_err(got, ref64) if bool(torch.isfinite(got).all()) else float("inf")
    bound = max(TOL, E32_FACTOR * e32)
    RECORDS.append((grp, what, e32, err))
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


def dev(t):
    return t.detach().to(torch.float32).contiguous().cuda()


class Out:
    """an output of `shape`, NaN-filled, with 8 canary rows behind it"""

    def __init__(self, *shape):
        row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        self.buf = torch.full((shape[0] + 8, row), float("nan"), dtype=torch.float32, device="cuda")
        self.buf[shape[0]:] = CANARY
        self.shape = shape

    @property
    def t(self):
        return self.buf[:self.shape[0]].view(self.shape)

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.shape[0]:] == CANARY).all()), f"{what}: wrote behind its output"


class Ws:
    """a workspace of exactly `nbytes` bytes, dirtied, with 256 canary bytes behind it"""

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
    """run `call` twice into fresh outputs built by `outs()`; same bits; returns the first run's outputs"""
    res = []
    for _ in range(2):
        o = outs()
        _lib.check(call(*o), what)
        torch.cuda.synchronize()
        for x in o:
            x.check(what)
        res.append(o)
    for a, b in zip(*res):
        if isinstance(a, Out):
            assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)), f"{what}: two runs differ in their bits"
    return res[0]


def size_of(fn, *args):
    need = C.c_size_t()
    _lib.check(fn(*args, C.byref(need)), fn.__name__)
    return need.value


@functools.lru_cache(maxsize=4)
def reference(dim, heads, n, gain):
    """the restatement on the case's inputs in float64 and in fp32 (CPU); computed once per case"""
    state, x = TC.attn_inputs(dim, heads, n, gain)
    return state, x, R.nystrom(x, state, heads, dtype=torch.float64), R.nystrom(x, state, heads, dtype=torch.float32)


# ------------------------------------------------------------------ the stage launchers (fp32 device tensors in, Out objects out)
def run_landmarks(qkv, heads):
    lib, npad = _lib.load(), qkv.shape[0]
    ql, kl = twice(lambda a, b: lib.rrt_nystrom_landmarks_f32(qkv.data_ptr(), a.ptr(), b.ptr(), npad, heads, stream()),
                   lambda: (Out(heads, 256, 64), Out(heads, 256, 64)), "rrt_nystrom_landmarks_f32")
    return ql.t, kl.t


def run_landmark_sim(ql, kl, heads):
    lib = _lib.load()
    (a2,) = twice(lambda a: lib.rrt_nystrom_landmark_sim_f32(ql.data_ptr(), kl.data_ptr(), a.ptr(), heads, stream()),
                  lambda: (Out(heads, 256, 256),), "rrt_nystrom_landmark_sim_f32")
    return a2.t


def run_landmark_attn(qkv, ql, heads):
    lib, npad = _lib.load(), qkv.shape[0]
    need = size_of(lib.rrt_nystrom_landmark_attn_workspace_size, npad, heads)
    av, _ = twice(lambda a, w: lib.rrt_nystrom_landmark_attn_f32(qkv.data_ptr(), ql.data_ptr(), a.ptr(), npad, heads, w.ptr(),
                                                                 w.n, stream()),
                  lambda: (Out(heads, 256, 64), Ws(need)), "rrt_nystrom_landmark_attn_f32")
    return av.t


def run_pinv(a2, heads, iters):
    lib = _lib.load()
    need = size_of(lib.rrt_nystrom_pinv_workspace_size, heads)
    z, _ = twice(lambda a, w: lib.rrt_nystrom_pinv_f32(a2.data_ptr(), a.ptr(), heads, iters, w.ptr(), w.n, stream()),
                 lambda: (Out(heads, 256, 256), Ws(need)), "rrt_nystrom_pinv_f32")
    return z.t


def run_zav(z, av, heads):
    lib = _lib.load()
    (wz,) = twice(lambda a: lib.rrt_nystrom_zav_f32(z.data_ptr(), av.data_ptr(), a.ptr(), heads, stream()),
                  lambda: (Out(heads, 256, 64),), "rrt_nystrom_zav_f32")
    return wz.t


def run_output(qkv, kl, wz, conv_w, heads):
    lib, npad = _lib.load(), qkv.shape[0]
    ks = conv_w.shape[1] if conv_w is not None else 0
    (o,) = twice(lambda a: lib.rrt_nystrom_output_f32(qkv.data_ptr(), kl.data_ptr(), wz.data_ptr(),
                                                      conv_w.data_ptr() if conv_w is not None else None, a.ptr(), npad, heads,
                                                      ks, stream()),
                 lambda: (Out(npad, heads * 64),), "rrt_nystrom_output_f32")
    return o.t


def run_attention(x, state, dim, heads, iters=6, residual=True):
    lib = _lib.load()
    d, w = _lib.NystromDesc(), _lib.NystromWeights()
    d.dim, d.heads, d.dim_head, d.num_landmarks, d.pinv_iterations = dim, heads, 64, 256, iters
    d.residual, d.residual_conv_kernel = int(residual), 33
    ts = [dev(torch.from_numpy(state[k])) for k in ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias")]
    conv = dev(torch.from_numpy(state["res_conv.weight"])) if residual else None
    w.qkv_w, w.out_w, w.out_b = (t.data_ptr() for t in ts)
    w.conv_w = conv.data_ptr() if conv is not None else None
    xd, n = dev(torch.from_numpy(x)), x.shape[0]
    need = size_of(lib.rrt_nystrom_workspace_size, C.byref(d), n)
    y, _ = twice(lambda a, s: lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), xd.data_ptr(), a.ptr(), n, s.ptr(), s.n,
                                                            stream()),
                 lambda: (Out(n, dim), Ws(need)), "rrt_nystrom_attention_f32")
    return y.t


# ------------------------------------------------------------------ stage and attention cases
@pytest.mark.parametrize("dim,heads,n,gain", TC.ATTN_CASES, ids=lambda v: str(v))
def test_stages_and_attention(dim, heads, n, gain):
    state, x, r64, r32 = reference(dim, heads, n, gain)
    case, grp = f"d{dim} h{heads} n{n} g{gain:g}", f"d{dim} h{heads} gain {gain:g}"
    if gain > 1:
        assert TC.PEAK_RANGE[0] <= r64["peak"] <= TC.PEAK_RANGE[1], (case, r64["peak"])
    fails = []
    # a stage's inputs: the float64 run's tensors rounded to fp32; its references: the stage function on exactly those
    i32 = {k: r64[k].float() for k in ("qkv", "ql", "kl", "a2", "av", "z", "wz")}
    i64 = {k: v.double() for k, v in i32.items()}
    g = {k: dev(v) for k, v in i32.items()}
    conv32 = torch.from_numpy(state["res_conv.weight"]).reshape(heads, -1)

    ql, kl = run_landmarks(g["qkv"], heads)
    for name, got, a, b in zip(("ql", "kl"), (ql, kl), R.st_landmarks(i64["qkv"], heads), R.st_landmarks(i32["qkv"], heads)):
        judge(grp, case, name, got, a, b, fails)
    judge(grp, case, "a2", run_landmark_sim(g["ql"], g["kl"], heads), R.st_landmark_sim(i64["ql"], i64["kl"]),
          R.st_landmark_sim(i32["ql"], i32["kl"]), fails)
    judge(grp, case, "a3.v", run_landmark_attn(g["qkv"], g["ql"], heads), R.st_landmark_attn(i64["qkv"], i64["ql"], heads),
          R.st_landmark_attn(i32["qkv"], i32["ql"], heads), fails)
    for iters in TC.PINV_ITERATIONS:
        judge(grp, case, f"z it{iters}", run_pinv(g["a2"], heads, iters), R.pinv_iter(i64["a2"], iters),
              R.pinv_iter(i32["a2"], iters), fails)
    judge(grp, case, "z.(a3.v)", run_zav(g["z"], g["av"], heads), R.st_zav(i64["z"], i64["av"]), R.st_zav(i32["z"], i32["av"]),
          fails)
    for conv in (conv32, None):                       # residual = 1 and residual = 0 (no stencil)
        judge(grp, case, "o" if conv is not None else "o no conv",
              run_output(g["qkv"], g["kl"], g["wz"], dev(conv) if conv is not None else None, heads),
              R.st_output(i64["qkv"], i64["kl"], i64["wz"], heads, conv.double() if conv is not None else None),
              R.st_output(i32["qkv"], i32["kl"], i32["wz"], heads, conv), fails)
    # the whole attention, against the restatement and against the reference's golden rows
    y = run_attention(x, state, dim, heads)
    judge(grp, case, "y", y, r64["y"], r32["y"], fails)
    gold = load_golden("transmil_attn")
    key = f"d{dim}_h{heads}_n{n}_g{int(gain)}"
    rows = torch.stack([y[0], y[-1]])
    gy = torch.from_numpy(gold[key + "/y"])
    judge(grp, case, "y golden", rows, gy, gy, fails, e32_floor=float(gold[key + "/e32"]))
    assert not fails, "\n".join(fails)


def test_pinv_scale_is_global_over_heads():
    """two heads with very different column sums: the initial scale is ONE scalar over both (a per-head scale gives another
    z after one iteration, by far more than the bound)"""
    i = torch.arange(256)
    s = torch.zeros(2, 256, 256, dtype=torch.float64)
    s[0, i, i] = 6.0                                    # head 0: near the identity, column sums ~ 1
    s[1, i, i] = 4.0
    s[1, :, 7] += 4.0                                   # head 1: every row also looks at column 7, column sum of tens
    a32 = s.softmax(-1).float()
    fails = []
    for iters in TC.PINV_ITERATIONS:
        z = run_pinv(dev(a32), 2, iters)
        ref = R.pinv_iter(a32.double(), iters)
        judge("pinv two heads", "column sums 1 vs tens", f"z it{iters}", z, ref, R.pinv_iter(a32, iters), fails)
        if iters == 1:                                   # (six iterations have all but converged from either start)
            per_head = torch.cat([R.pinv_iter(a32[h:h + 1].double(), iters) for h in range(2)])
            assert R.rel_err(per_head, ref) > 100 * TOL  # the case does tell the two apart
    assert not fails, "\n".join(fails)


def test_attention_without_residual_and_other_iterations():
    state, x = TC.attn_inputs(128, 2, 257, 1.0)
    fails = []
    for iters, residual in ((1, True), (6, False)):
        y = run_attention(x, state, 128, 2, iters=iters, residual=residual)
        a, b = (R.nystrom(x, state, 2, iters=iters, residual=residual, dtype=dt)["y"] for dt in (torch.float64, torch.float32))
        judge("attention options", f"iters {iters} residual {residual}", "y", y, a, b, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ the module and the model
def make_model(input_dim, act, N):
    from rrt_mil_amd import TransMIL
    state, x = TC.model_inputs(input_dim, N)
    model = TransMIL(input_dim, 2, False, act)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return model.cuda().eval(), state, x


@pytest.mark.parametrize("input_dim,act,N", TC.MODEL_CASES, ids=lambda v: str(v))
def test_transmil_model(input_dim, act, N):
    model, state, x = make_model(input_dim, act, N)
    r64, r32 = (R.transmil(x, state, act, dtype=dt) for dt in (torch.float64, torch.float32))
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        logits, feat = model.forward_bag(xd, return_features=True)
        logits2, feat2 = model.forward_bag(xd, return_features=True)
    assert torch.equal(logits, logits2) and torch.equal(feat, feat2), "two runs differ in their bits"
    case, fails = f"TransMIL({input_dim}, {act}) N{N}", []
    judge("TransMIL", case, "logits", logits[0], r64["logits"], r32["logits"], fails)
    judge("TransMIL", case, "feat", feat, r64["feat"], r32["feat"], fails)
    gold = load_golden("transmil_model")
    key = f"i{input_dim}_{act}_n{N}"
    gl, gf = torch.from_numpy(gold[key + "/logits"]), torch.from_numpy(gold[key + "/feat"])
    judge("TransMIL", case, "logits golden", logits[0], gl, gl, fails, e32_floor=float(gold[key + "/e32_logits"]))
    judge("TransMIL", case, "feat golden", torch.stack([feat[0], feat[1], feat[-1]]), gf, gf, fails,
          e32_floor=float(gold[key + "/e32_feat"]))
    assert not fails, "\n".join(fails)


def test_transmil_api():
    """forward_bag == model(x) == forward_bags, bit for bit; a dirtied workspace changes nothing; what must raise, raises"""
    model, _state, x = make_model(64, "gelu", 250)
    xd = torch.from_numpy(x).cuda()
    x2 = torch.from_numpy(TC.model_inputs(64, 37)[1]).cuda()
    with torch.no_grad():
        a = model.forward_bag(xd)
        assert a.shape == (1, 2)
        assert torch.equal(a, model(xd)) and torch.equal(a, model(xd[None]))
        b = model.forward_bags([xd, x2[None], xd])
        assert torch.equal(b[0], a) and torch.equal(b[2], a) and torch.equal(b[1], model.forward_bag(x2))
        model._ws.fill_(0xFF)                            # NaN patterns everywhere in the workspace
        assert torch.equal(model.forward_bag(xd), a)
        with pytest.raises(ValueError):
            model(torch.stack([xd, xd]))
    with pytest.raises(NotImplementedError, match="no_grad"):
        model(xd)                                        # parameters require grad and grad mode is on: needs a graph
    with torch.no_grad(), pytest.raises(NotImplementedError, match="eval"):
        model.train()(xd)
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(model.forward_bag(xd), a)     # exact fp32 under autocast as well


def test_nystrom_module():
    from rrt_mil_amd import NystromAttention
    state, x = TC.attn_inputs(128, 2, 513, 1.0)
    mod = NystromAttention(128, heads=2)
    mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    mod = mod.cuda().eval()
    xd = torch.from_numpy(x).cuda()[None]
    with torch.no_grad():
        y = mod(xd)
        assert y.shape == (1, 513, 128) and torch.equal(y, mod(xd))
        assert torch.equal(y[0], run_attention(x, state, 128, 2))
        with pytest.raises(NotImplementedError):
            mod(xd, mask=torch.ones(1, 513, dtype=torch.bool, device="cuda"))
        with pytest.raises(NotImplementedError):
            mod(xd, return_attn=True)
        with pytest.raises(ValueError):
            mod(torch.cat([xd, xd]))
    fails = []
    a, b = (R.nystrom(x, state, 2, dtype=dt)["y"] for dt in (torch.float64, torch.float32))
    judge("NystromAttention module", "d128 h2 n513", "y", y[0], a, b, fails)
    assert not fails, "\n".join(fails)


def test_ppeg_side_entry():
    """rrt_ppeg_side_f32 at sides below and above 7 (no lift to 7 x 7, nothing wrapped), row 0 passing through"""
    import torch.nn.functional as F
    from rrt_mil_amd import synth
    lib, Cc, fails = _lib.load(), 96, []
    ws = [torch.from_numpy(synth.uniform(f"ppeg_side/w{k}", (Cc, 1, k, k), -1.0 / k, 1.0 / k)) for k in (7, 5, 3)]
    bs = [torch.from_numpy(synth.uniform(f"ppeg_side/b{k}", (Cc,), -0.1, 0.1)) for k in (7, 5, 3)]
    dw, db = [dev(t) for t in ws], [dev(t) for t in bs]
    wp = (C.c_void_p * 3)(*[t.data_ptr() for t in dw])
    bp = (C.c_void_p * 3)(*[t.data_ptr() for t in db])
    for side in (1, 2, 4, 6, 7, 9, 17):
        x = torch.from_numpy(synth.normal(f"ppeg_side/x{side}", (1 + side * side, Cc)))
        xd = dev(x)
        (y,) = twice(lambda a: lib.rrt_ppeg_side_f32(xd.data_ptr(), wp, bp, a.ptr(), side, Cc, stream()),
                     lambda: (Out(1 + side * side, Cc),), "rrt_ppeg_side_f32")
        refs = []
        for dt in (torch.float64, torch.float32):
            img = x[1:].to(dt).t().reshape(1, Cc, side, side)
            pe = img
            for w, b, k in zip(ws, bs, (7, 5, 3)):
                pe = pe + F.conv2d(img, w.to(dt), b.to(dt), padding=k // 2, groups=Cc)
            refs.append(torch.cat([x[:1].to(dt), pe.reshape(Cc, side * side).t()]))
        judge("PPEG with a stated side", f"side {side}", "y", y.t, refs[0], refs[1], fails)
        assert torch.equal(y.t[0].cpu(), x[0])
    assert not fails, "\n".join(fails)
