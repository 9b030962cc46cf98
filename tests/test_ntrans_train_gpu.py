"""GPU (-m gpu): training the Nystrom ablations of RRTEncoder -- the BATCHED backward of Nystrom attention (csrc/nystrom_bwd.hip
with b items per launch), one stage at a time and as a whole, ``NystromAttention.enable_training().forward_batch``, and the
opt-in layer path of ``RRTEncoder(attn='ntrans' | region_attn='ntrans')`` and of RRTMIL around it -- against float64 autograd
of the restatement tests/ntrans_ref.py (pinned to the reference's own float64 gradients by tests/test_ntrans_train_cpu.py),
never against another kernel, except where the claim IS bit-identity: with b = 1 every batched entry gives the bits of its
single-sequence counterpart, and forward_train's y those of the inference call.

Bounds.  Stages, the whole attention and the module: the project's gradient rule (tests/test_nystrom_grad_gpu.py::judge) --
each gradient relative to its own largest entry, <= max(2e-5, 8 x e32), e32 = the fp32 CPU autograd of the same function on
the same inputs against the float64 one, measured here.  The encoder and RRTMIL: every gradient within 1e-3 of its own largest
entry (the rule of tests/test_hip_parity.py's G15 cases).  The layer path's glue (LayerNorm, partition, FFN, PEG / PPEG) is
torch, so the forward with a graph is not the one-call path's bits: it is held to the forward tests' bound,
max(2e-5, 8 x e32) relative to max(1, max |float64|).

The harness is tests/test_nystrom_grad_gpu.py's: NaN-filled outputs with canary rows behind them, workspaces and stashes of
exactly the queried size (pre-filled with 0xA5, then 0xFF) with canary bytes behind them, every call twice with the same bits.
With RRT_NTRANS_GRAD_ERRORS_OUT=<file> the module writes its error table (kept as profiles/ntrans_grad_errors.txt)."""
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import ntrans_cases as NC
import ntrans_ref as NR
import nystrom_grad_cases as GC
import test_nystrom_grad_gpu as G
from rrt_mil_amd import _lib
from test_nystrom_grad_gpu import FILLS, Out, Ws, both, dev, grads_of, size_of, stream, twice

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad")]

H = NC.HEADS
ENC_TOL = 1e-3
RECORDS = []
PARAMS = NR.NYS_KEYS
STAGE_KEYS = ("qkv", "ql", "kl", "a2", "av", "z", "wz")
# name -> (b, n, peaked): the forward's stage cases, many short items, and b * heads = 80 > 64 per-matrix partials of d den
CASES = dict(NC.STAGE_CASES, b16_n16=(16, 16, False), b40_n16=(40, 16, False))
ENCODER_CASES = ("bag_n300", "bag_n700_l3_ffn_sc", "reg_n200_rn2", "reg_n1300_rn2_sc", "reg_n500_rsize9", "reg_n300_fallback",
                 "bag_n300_ppeg_first", "reg_n200_l3_peg_mid")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_NTRANS_GRAD_ERRORS_OUT")
    if out and RECORDS:
        with open(out, "w") as fh:
            fh.write(G.error_table(RECORDS))


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """a device error is sticky: nothing more is started on a device that reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is run on it: {e}", returncode=3)


def judge(grp, case, what, got, ref64, ref32, fails):
    """tests/test_nystrom_grad_gpu.py::judge, recorded in this module's table"""
    mine = []
    G.judge(grp, case, what, got, ref64, ref32, mine)
    RECORDS.append(G.RECORDS.pop())
    fails.extend(mine)


def judge_1e3(grp, case, what, got, ref64, ref32, fails):
    """the encoder's rule: within 1e-3 of the gradient's own largest entry"""
    ref64 = ref64.detach().double()
    big = float(ref64.abs().max())
    got = got.detach().cpu().double().reshape(ref64.shape)
    if big == 0:                                             # (a gradient that is exactly zero must come out exactly zero)
        assert not bool(got.any()), (case, what)
        return
    err = float((got - ref64).abs().max()) / big if bool(torch.isfinite(got).all()) else float("inf")
    e32 = float((ref32.detach().double() - ref64).abs().max()) / big
    RECORDS.append((grp, what, e32, err))
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {ENC_TOL:.0e} max|ref| {big:.2e}")
    if not err <= ENC_TOL:
        fails.append(f"{case} {what}: {err:.3e} > {ENC_TOL:.0e} (e32 {e32:.2e})")


def judge_forward(grp, case, what, got, ref64, ref32, fails):
    """the forward tests' rule (tests/test_ntrans_gpu.py::judge)"""
    e32 = NR.rel_err(ref32, ref64)
    err = NR.rel_err(got.detach().cpu(), ref64)
    bound = max(G.TOL, G.E32_FACTOR * e32)
    RECORDS.append((grp, what, e32, err))
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def cot(case, name, shape):
    return torch.from_numpy(GC.cotangent(f"ntrans/{name}/{case}", tuple(shape)))


@functools.lru_cache(maxsize=2)
def forward64(name):
    """the float64 run's stage tensors rounded to fp32 (the stages' inputs); computed once per case, never modified"""
    b, n, peaked = CASES[name]
    state, x = NC.batch_inputs(b, n, peaked)
    with torch.no_grad():
        r64 = NR.nystrom_batched(x, state, H, dtype=torch.float64)
    return state, x, {k: r64[k].float() for k in STAGE_KEYS}


# ------------------------------------------------------------------ the batched stage launchers
def run_output_backward(qkv, kl, wz, conv_w, d_o, b):
    lib, npad = _lib.load(), qkv.shape[-2]
    ks = conv_w.shape[1] if conv_w is not None else 0
    need = size_of(lib.rrt_nystrom_output_batched_backward_workspace_size, b, npad, H)
    outs = twice(lambda a, c, e, d, w: lib.rrt_nystrom_output_batched_backward_f32(
        qkv.data_ptr(), kl.data_ptr(), wz.data_ptr(), conv_w.data_ptr() if conv_w is not None else None, d_o.data_ptr(),
        a.ptr(), c.ptr(), e.ptr(), d.ptr() if conv_w is not None else None, b, npad, H, ks, w.ptr(), w.n, stream()),
        lambda run: (Out(b, npad, 3 * H * 64), Out(b, H, 256, 64), Out(b, H, 256, 64), Out(H, max(ks, 1)), Ws(need, FILLS[run])),
        "rrt_nystrom_output_batched_backward_f32")
    return [o.t for o in outs[:4]]


def run_zav_backward(z, av, d_wz, b):
    lib = _lib.load()
    d_z, d_av = twice(lambda a, c: lib.rrt_nystrom_zav_batched_backward_f32(z.data_ptr(), av.data_ptr(), d_wz.data_ptr(), a.ptr(),
                                                                            c.ptr(), b, H, stream()),
                      lambda run: (Out(b, H, 256, 256), Out(b, H, 256, 64)), "rrt_nystrom_zav_batched_backward_f32")
    return d_z.t, d_av.t


def run_landmark_attn_backward(qkv, ql, d_av, prefill, b):
    lib, npad = _lib.load(), qkv.shape[-2]
    need = size_of(lib.rrt_nystrom_landmark_attn_batched_backward_workspace_size, b, npad, H)
    d_qkv, d_ql, _ = twice(lambda a, c, w: lib.rrt_nystrom_landmark_attn_batched_backward_f32(
        qkv.data_ptr(), ql.data_ptr(), d_av.data_ptr(), a.ptr(), c.ptr(), b, npad, H, w.ptr(), w.n, stream()),
        lambda run: (Out(b, npad, 3 * H * 64, prefill=prefill), Out(b, H, 256, 64), Ws(need, FILLS[run])),
        "rrt_nystrom_landmark_attn_batched_backward_f32")
    return d_qkv.t, d_ql.t


def run_pinv_sim_backward(ql, kl, d_z, b, iters, heads=H):
    lib = _lib.load()
    need = size_of(lib.rrt_nystrom_pinv_sim_batched_backward_workspace_size, b, heads, iters)
    d_ql, d_kl, _ = twice(lambda a, c, w: lib.rrt_nystrom_pinv_sim_batched_backward_f32(
        ql.data_ptr(), kl.data_ptr(), d_z.data_ptr(), a.ptr(), c.ptr(), b, heads, iters, w.ptr(), w.n, stream()),
        lambda run: (Out(b, heads, 256, 64), Out(b, heads, 256, 64), Ws(need, FILLS[run])),
        "rrt_nystrom_pinv_sim_batched_backward_f32")
    return d_ql.t, d_kl.t


def run_landmarks_backward(d_ql, d_kl, prefill, b, npad):
    lib = _lib.load()
    (d_qkv,) = twice(lambda a: lib.rrt_nystrom_landmarks_batched_backward_f32(d_ql.data_ptr(), d_kl.data_ptr(), a.ptr(), b, npad, H,
                                                                              stream()),
                     lambda run: (Out(b, npad, 3 * H * 64, prefill=prefill),), "rrt_nystrom_landmarks_batched_backward_f32")
    return d_qkv.t


def run_attention_train(x, state, dy, iters=6, residual=True):
    """batched forward_train + backward through the C ABI -> {y, dx, the parameter gradients}: y is held to the bits of
    rrt_nystrom_attention_batched_f32, everything to the bits of a second run with another pattern in stash and workspace"""
    lib, (b, n, dim) = _lib.load(), x.shape
    d, w = G.nystrom_desc(dim, H, iters, residual), _lib.NystromWeights()
    ts = [dev(state[k]) if (residual or k != "res_conv.weight") else None for k in PARAMS]
    w.qkv_w, w.out_w, w.out_b, w.conv_w = (t.data_ptr() if t is not None else None for t in ts)
    xd, dyd = dev(x), dev(dy)
    sb, wb = C.c_size_t(), C.c_size_t()
    _lib.check(lib.rrt_nystrom_batched_train_sizes(C.byref(d), b, n, C.byref(sb), C.byref(wb)), "rrt_nystrom_batched_train_sizes")
    y0, ws0 = Out(b, n, dim), Ws(size_of(lib.rrt_nystrom_batched_workspace_size, C.byref(d), b, n))
    _lib.check(lib.rrt_nystrom_attention_batched_f32(C.byref(d), C.byref(w), xd.data_ptr(), y0.ptr(), b, n, ws0.ptr(), ws0.n,
                                                     stream()), "rrt_nystrom_attention_batched_f32")
    runs = []
    for run in range(2):
        stash, ws, y, dx = Ws(sb.value, FILLS[run]), Ws(wb.value, FILLS[run]), Out(b, n, dim), Out(b, n, dim)
        gs = [Out(*t.shape) if t is not None else None for t in ts]
        g = _lib.NystromGrads()
        g.qkv_w, g.out_w, g.out_b, g.conv_w = (o.ptr() if o is not None else None for o in gs)
        _lib.check(lib.rrt_nystrom_attention_batched_forward_train_f32(C.byref(d), C.byref(w), xd.data_ptr(), y.ptr(), b, n,
                                                                       stash.ptr(), stash.n, stream()),
                   "rrt_nystrom_attention_batched_forward_train_f32")
        _lib.check(lib.rrt_nystrom_attention_batched_backward_f32(C.byref(d), C.byref(w), xd.data_ptr(), dyd.data_ptr(), stash.ptr(),
                                                                  stash.n, C.byref(g), dx.ptr(), b, n, ws.ptr(), ws.n, stream()),
                   "rrt_nystrom_attention_batched_backward_f32")
        torch.cuda.synchronize()
        for o in (stash, ws, y, dx, y0, ws0, *[o for o in gs if o is not None]):
            o.check("rrt_nystrom_attention_batched_{forward_train,backward}_f32")
        assert same_bits(y.t, y0.t), "forward_train's y differs from the inference call's"
        runs.append({"y": y.t, "dx": dx.t, **{k: o.t for k, o in zip(PARAMS, gs) if o is not None}})
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), f"{k}: two runs differ in their bits"
    return runs[0]


def attention_reference(x, state, dy, iters, residual, dtype):
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).to(dtype).requires_grad_(True)
    (NR.nystrom_batched(xd, p, H, iters=iters, residual=residual, dtype=dtype)["y"] * dy.to(dtype)).sum().backward()
    out = {k: p[k].grad for k in PARAMS if p[k].grad is not None}
    out["dx"] = xd.grad
    return out


def judge_attention(grp, case, got, x, state, dy, iters, residual, fails):
    r64, r32 = (attention_reference(x, state, dy, iters, residual, dt) for dt in (torch.float64, torch.float32))
    assert set(r64) == set(got) - {"y"}, (set(r64), set(got))
    for k in r64:
        judge(grp, case, "attn " + k, got[k].reshape(r64[k].shape), r64[k], r32[k], fails)


# ------------------------------------------------------------------ b = 1: the bits of the single-sequence entries
@pytest.mark.parametrize("n", NC.BIT_IDENTITY_LENGTHS)
def test_b1_gives_the_bits_of_the_single_sequence_entries(n):
    lib = _lib.load()
    state, x = NC.batch_inputs(1, n, False)
    with torch.no_grad():
        r64 = NR.nystrom_batched(x, state, H, dtype=torch.float64)
    g = {k: dev(r64[k].float()) for k in STAGE_KEYS}
    s = {k: v[0] for k, v in g.items()}
    npad, hd, key = g["qkv"].shape[1], H * 64, f"b1_n{n}"
    conv = dev(torch.from_numpy(state["res_conv.weight"]).reshape(H, -1))
    d_o = dev(cot(key, "d_o", (1, npad, hd)))
    for c in (conv, None):
        for a, e in zip(run_output_backward(g["qkv"], g["kl"], g["wz"], c, d_o, 1)[:4 if c is not None else 3],
                        G.run_output_backward(s["qkv"], s["kl"], s["wz"], c, d_o[0], H)):
            assert same_bits(a.reshape(e.shape), e), "output_backward"
    d_wz = dev(cot(key, "d_wz", (1, H, 256, 64)))
    for a, e in zip(run_zav_backward(g["z"], g["av"], d_wz, 1), G.run_zav_backward(s["z"], s["av"], d_wz[0], H)):
        assert same_bits(a[0], e), "zav_backward"
    d_av, pre = dev(cot(key, "d_av", (1, H, 256, 64))), cot(key, "prefill", (1, npad, 3 * hd)).float()
    for a, e in zip(run_landmark_attn_backward(g["qkv"], g["ql"], d_av, pre, 1),
                    G.run_landmark_attn_backward(s["qkv"], s["ql"], d_av[0], pre[0], H)):
        assert same_bits(a[0], e), "landmark_attn_backward"
    for iters in GC.PINV_ITERATIONS:
        d_z = dev(cot(key, f"d_z{iters}", (1, H, 256, 256)))
        for a, e in zip(run_pinv_sim_backward(g["ql"], g["kl"], d_z, 1, iters),
                        G.run_pinv_sim_backward(s["ql"], s["kl"], d_z[0], H, iters)):
            assert same_bits(a[0], e), "pinv_sim_backward"
    d_l = dev(cot(key, "d_ql", (1, H, 256, 64))), dev(cot(key, "d_kl", (1, H, 256, 64)))
    assert same_bits(run_landmarks_backward(d_l[0], d_l[1], pre, 1, npad)[0],
                     G.run_landmarks_backward(d_l[0][0], d_l[1][0], pre[0], npad, H)), "landmarks_backward"
    dy = cot(key, "dy", x.shape)
    got, one = run_attention_train(x, state, dy), G.run_attention_train(x[0], state, dy[0], NC.DIM, H)
    for k in one:
        assert same_bits(got[k].reshape(one[k].shape), one[k]), f"attention {k}"
    sizes = [C.c_size_t() for _ in range(4)]
    d = G.nystrom_desc(NC.DIM, H)
    _lib.check(lib.rrt_nystrom_batched_train_sizes(C.byref(d), 1, n, C.byref(sizes[0]), C.byref(sizes[1])), "sizes")
    _lib.check(lib.rrt_nystrom_train_sizes(C.byref(d), n, C.byref(sizes[2]), C.byref(sizes[3])), "sizes")
    assert (sizes[0].value, sizes[1].value) == (sizes[2].value, sizes[3].value)


# ------------------------------------------------------------------ stages and the whole attention against float64
@pytest.mark.parametrize("name", list(CASES))
def test_batched_backward_stages_and_attention(name):
    b, n, _peaked = CASES[name]
    state, x, i32 = forward64(name)
    g = {k: dev(v) for k, v in i32.items()}
    npad, hd, grp, fails = i32["qkv"].shape[1], H * 64, f"batched {name}", []
    conv32 = torch.from_numpy(state["res_conv.weight"]).reshape(H, -1)

    # output: the stencil's adjoint along each item's own sequence, d_conv_w summed over the items
    d_o = cot(name, "d_o", (b, npad, hd))
    for conv in (conv32, None):
        tag = "" if conv is not None else " no conv"
        r64, r32 = both(lambda q, k_, w_, c: NR.st_output(q, k_, w_, H, c), (i32["qkv"], i32["kl"], i32["wz"], conv), d_o)
        d_qkv, d_kl, d_wz, d_conv = run_output_backward(g["qkv"], g["kl"], g["wz"], dev(conv) if conv is not None else None,
                                                        dev(d_o), b)
        if conv is None:
            assert not bool(d_qkv[..., 2 * hd:].any()), "no conv: the v third must be zero"
        assert not bool(d_qkv[..., hd:2 * hd].any()), "the k third must be zeroed"
        judge(grp, name, "output d_qkv" + tag, d_qkv, r64[0], r32[0], fails)
        judge(grp, name, "output d_kl" + tag, d_kl, r64[1], r32[1], fails)
        judge(grp, name, "output d_wz" + tag, d_wz, r64[2], r32[2], fails)
        if conv is not None:
            judge(grp, name, "output d_conv_w", d_conv, r64[3], r32[3], fails)

    # zav
    d_wz = cot(name, "d_wz", (b, H, 256, 64))
    r64, r32 = both(NR.st_zav, (i32["z"], i32["av"]), d_wz)
    for what, got, a, c in zip(("zav d_z", "zav d_av"), run_zav_backward(g["z"], g["av"], dev(d_wz), b), r64, r32):
        judge(grp, name, what, got, a, c, fails)

    # landmark attention over the keys: d_ql written, dk / dv added onto a prefill, the q third untouched
    d_av = cot(name, "d_av", (b, H, 256, 64))
    r64, r32 = both(lambda q, l_: NR.st_landmark_attn(q, l_, H), (i32["qkv"], i32["ql"]), d_av)
    pre = G.prefill_like(name, "ntrans_lattn", r64[0])
    d_qkv, d_ql = run_landmark_attn_backward(g["qkv"], g["ql"], dev(d_av), pre, b)
    assert torch.equal(d_qkv[..., :hd].cpu(), pre[..., :hd]), "landmark_attn_backward touched the q third"
    judge(grp, name, "lattn d_qkv (k, v)", d_qkv, pre.double() + r64[0], pre + r32[0], fails)
    judge(grp, name, "lattn d_ql", d_ql, r64[1], r32[1], fails)

    # pinv through the landmark softmax: ONE den over all b * heads matrices
    for iters in GC.PINV_ITERATIONS:
        d_z = cot(name, f"d_z{iters}", (b, H, 256, 256))
        r64, r32 = both(lambda a, c: NR.pinv_iter(NR.st_landmark_sim(a, c), iters), (i32["ql"], i32["kl"]), d_z)
        d_ql, d_kl = run_pinv_sim_backward(g["ql"], g["kl"], dev(d_z), b, iters)
        judge(grp, name, f"pinv_sim d_ql it{iters}", d_ql, r64[0], r32[0], fails)
        judge(grp, name, f"pinv_sim d_kl it{iters}", d_kl, r64[1], r32[1], fails)

    # landmarks: the 1 / l shares added onto a prefill
    d_l = (cot(name, "d_ql", (b, H, 256, 64)), cot(name, "d_kl", (b, H, 256, 64)))
    r64, r32 = both(lambda q: NR.st_landmarks(q, H), (i32["qkv"],), d_l)
    pre = G.prefill_like(name, "ntrans_landmarks", r64[0])
    d_qkv = run_landmarks_backward(dev(d_l[0]), dev(d_l[1]), pre, b, npad)
    assert torch.equal(d_qkv[..., 2 * hd:].cpu(), pre[..., 2 * hd:]), "landmarks_backward touched the v third"
    judge(grp, name, "landmarks d_qkv (q, k)", d_qkv, pre.double() + r64[0], pre + r32[0], fails)

    # the whole attention
    dy = cot(name, "dy", x.shape)
    judge_attention(grp, name, run_attention_train(x, state, dy), x, state, dy, 6, True, fails)
    assert not fails, "\n".join(fails)


def test_batched_attention_backward_without_residual_and_other_iterations():
    name = "b3_n300"
    b, n, peaked = CASES[name]
    state, x = NC.batch_inputs(b, n, peaked)
    fails = []
    for iters, residual in ((1, True), (6, False)):
        dy = cot(name, f"dy_options{iters}", x.shape)
        got = run_attention_train(x, state, dy, iters=iters, residual=residual)
        assert ("res_conv.weight" in got) == residual
        judge_attention("batched attention options", f"{name} iters {iters} residual {residual}", got, x, state, dy, iters,
                        residual, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ ties across items
def test_pinv_den_gradient_with_columns_tied_across_items():
    """ql, kl [3, 2, 256, 64].  Item 0 is test_pinv_den_gradient_with_tied_columns' construction (head 1: key landmarks 9, 77
    and 200 are one row and draw every query), item 1 is generic, item 2 is a copy of item 0: six column sums attain the maximum
    bit for bit, in two items, so d den is shared among columns of BOTH.  A backward with a denominator per item is far outside."""
    ql = torch.from_numpy(GC.cotangent("ties/ql", (2, 256, 64))).float()
    kl = torch.from_numpy(GC.cotangent("ties/kl", (2, 256, 64))).float() * 0.5
    u = torch.full((64,), 0.25)
    ql[1] += u
    kl[1, 9] = kl[1, 77] = kl[1, 200] = 2.0 * u
    ql1 = torch.from_numpy(GC.cotangent("ntrans/ties/ql1", (2, 256, 64))).float()
    kl1 = torch.from_numpy(GC.cotangent("ntrans/ties/kl1", (2, 256, 64))).float() * 0.5
    ql, kl = torch.stack([ql, ql1, ql]), torch.stack([kl, kl1, kl])
    for dt in (torch.float32, torch.float64):
        cs = NR.st_landmark_sim(ql.to(dt), kl.to(dt)).sum(-2)
        assert int((cs == cs.max()).sum()) == 6 and bool((cs[[0, 2]][:, 1][:, [9, 77, 200]] == cs.max()).all())
    fn = lambda iters: (lambda a, c: NR.pinv_iter(NR.st_landmark_sim(a, c), iters))      # noqa: E731
    fails = []
    for iters in GC.PINV_ITERATIONS:
        d_z = cot("ties", f"d_z{iters}", (3, 2, 256, 256))
        r64, r32 = both(fn(iters), (ql, kl), d_z)
        d_ql, d_kl = run_pinv_sim_backward(dev(ql), dev(kl), dev(d_z), 3, iters)
        judge("pinv ties across items", "six tied columns", f"pinv_sim d_ql it{iters}", d_ql, r64[0], r32[0], fails)
        judge("pinv ties across items", "six tied columns", f"pinv_sim d_kl it{iters}", d_kl, r64[1], r32[1], fails)
        per_item = grads_of(lambda a, c: NR.pinv_iter_per_item(NR.st_landmark_sim(a, c), iters), (ql, kl), d_z, torch.float64)
        for got, ref in zip(per_item, r64):                  # the case does tell a per-item den apart
            assert float((got - ref).abs().max()) / float(ref.abs().max()) > 100 * G.TOL
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ the module
def make_attention(name, dropout=0.):
    from rrt_mil_amd import NystromAttention
    b, n, peaked = CASES[name]
    state, x = NC.batch_inputs(b, n, peaked)
    mod = NystromAttention(NC.DIM, heads=H, dropout=dropout)
    mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return mod.cuda(), state, x


def test_nystrom_module_trains_on_a_batch():
    mod, state, x = make_attention("b3_n300")
    mod.eval()
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="b = 1"):
        mod.forward_batch(xd)                                # off by default: the refusal is unchanged
    with torch.no_grad():
        y_eval = mod.forward_batch(xd)
    assert mod.enable_training() is mod
    dy = cot("module", "dy", x.shape)
    y = mod.forward_batch(xd)
    assert y.shape == x.shape and y.requires_grad and same_bits(y.detach(), y_eval)
    (y * dy.cuda()).sum().backward()
    got = {k: p.grad for k, p in mod.named_parameters()}
    assert set(got) == set(PARAMS) and all(v is not None for v in got.values()) and xd.grad is not None
    got["dx"] = xd.grad
    fails = []
    judge_attention("NystromAttention.forward_batch", "b3_n300", got, x, state, dy, 6, True, fails)
    assert not fails, "\n".join(fails)
    with torch.no_grad():
        assert same_bits(mod.forward_batch(xd), y_eval)      # no graph needed: the one-call path
    with pytest.raises(ValueError, match="forward_batch"):
        mod(xd)                                              # forward keeps b = 1
    # eval() with grad is deterministic, and fp32 under autocast
    first = {k: v.clone() for k, v in got.items()}
    mod.zero_grad()
    x2 = xd.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y2 = mod.forward_batch(x2)
        assert y2.dtype == torch.float32 and same_bits(y2.detach(), y_eval)
        (y2 * dy.cuda()).sum().backward()
    assert same_bits(x2.grad, first["dx"])
    for k, p in mod.named_parameters():
        assert same_bits(p.grad, first[k]), k
    # a parameter modified between forward and backward
    y3 = mod.forward_batch(x2)
    with torch.no_grad():
        mod.to_out[0].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified"):
        y3.sum().backward()


def test_nystrom_module_batch_dropout_is_torchs():
    mod, _state, x = make_attention("b3_n144", dropout=0.1)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        y_eval = mod.eval().forward_batch(xd)
        with pytest.raises(NotImplementedError, match="b = 1"):
            mod.train().forward_batch(xd)
    mod.enable_training().train()
    torch.manual_seed(7)
    y = mod.forward_batch(xd)
    torch.manual_seed(7)
    want = F.dropout(y_eval, 0.1, True)
    assert y.requires_grad and torch.equal(y.detach(), want) and not torch.equal(want, y_eval)
    y.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in mod.parameters())


# ------------------------------------------------------------------ the encoder, both modes
def make_encoder(name, **kw):
    from rrt_mil_amd import RRTEncoder
    cfg, state, x = NC.encoder_inputs(name)
    enc = RRTEncoder(**dict(cfg, **kw))
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return enc.cuda().eval(), cfg, state, x


def encoder_reference(x, state, cfg, dy, dtype):
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = NR.encoder(xd, p, cfg, dtype=dtype)
    (y * dy.to(dtype)).sum().backward()
    return y.detach(), {**{k: v.grad for k, v in p.items()}, "dx": xd.grad}


def encoder_backward(enc, x, dy):
    enc.zero_grad(set_to_none=True)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    y = enc(xd)
    (y * dy.cuda()).sum().backward()
    return y.detach(), {**{k: (p.grad.clone() if p.grad is not None else None) for k, p in enc.named_parameters()},
                        "dx": xd.grad.clone()}


@pytest.mark.parametrize("name", ENCODER_CASES)
def test_encoder_gradients(name):
    enc, cfg, state, x = make_encoder(name)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        one_call = enc(xd)
    with pytest.raises(NotImplementedError, match="no_grad"):
        enc(xd)                                              # off by default: the refusal is unchanged
    assert enc.enable_training() is enc
    dy = cot(name, "dy", x.shape)
    y, got = encoder_backward(enc, x, dy)
    y2, again = encoder_backward(enc, x, dy)
    assert same_bits(y, y2)
    for k in got:
        assert (got[k] is None and again[k] is None) or same_bits(got[k], again[k]), f"{k}: two backward passes differ in their bits"
    with torch.no_grad():
        assert same_bits(enc(xd), one_call)                  # no graph: the one-call path's bits
    (y64, r64), (y32, r32) = (encoder_reference(x, state, cfg, dy, dt) for dt in (torch.float64, torch.float32))
    grp, fails = "encoder " + ("bag" if NC.is_bag(cfg) else "regions"), []
    judge_forward(grp, name, "y (graph)", y, y64, y32, fails)
    assert set(got) == set(r64)
    seen = 0
    for k in r64:
        if r64[k] is None:
            assert got[k] is None, k
            continue
        assert got[k] is not None, k
        judge_1e3(grp, name, "d " + k.replace("layers.", "l").replace(".weight", ".w").replace(".bias", ".b"), got[k], r64[k],
                  r32[k], fails)
        seen += 1
    assert seen >= 16
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ("bag_n300", "reg_n200_rn2"))
def test_encoder_seeded_train_step_and_modified_parameter(name):
    enc, _cfg, _state, x = make_encoder(name, drop_out=0.1, drop_path=0.2)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="eval"):
        enc.train()(xd)                                      # off by default: the refusal is unchanged
    enc.enable_training().train()
    dy = cot(name, "dy_train", x.shape)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        runs.append(encoder_backward(enc, x, dy))
    assert same_bits(runs[0][0], runs[1][0])
    for k, v in runs[0][1].items():
        assert v is not None and bool(torch.isfinite(v).all()) and same_bits(v, runs[1][1][k]), k
    torch.manual_seed(12)
    assert not same_bits(encoder_backward(enc, x, dy)[0], runs[0][0])
    with torch.no_grad():
        assert enc(xd).shape == xd.shape                     # train() without a graph: the same layer path
        torch.manual_seed(13)
        want = enc(xd)
        out = torch.full_like(xd, float("nan"))
        torch.manual_seed(13)
        assert enc.forward_bag(xd, out=out) is out and same_bits(out, want)      # out= is written, not ignored
        outs = [torch.full_like(xd, float("nan"))]
        torch.manual_seed(13)
        assert enc.forward_bags([xd], outs=outs) is outs and same_bits(outs[0], want)
    with pytest.raises(NotImplementedError, match="out="):
        enc.forward_bag(xd, out=torch.empty_like(xd))        # a result with a graph cannot go into out=
    assert not enc.forward_bags([xd])[0].requires_grad       # forward_bags runs under no_grad: it never records a graph
    # eval() with gradients enabled: the same graph without dropout or drop-path, deterministic
    enc.eval()
    a, b = encoder_backward(enc, x, dy), encoder_backward(enc, x, dy)
    assert same_bits(a[0], b[0]) and all(same_bits(a[1][k], b[1][k]) for k in a[1])
    # a parameter modified between forward and backward raises: one the tail's kernels read, one an attention layer's read
    for param in (enc.norm.weight, enc._nystrom_of(next(iter(enc.layers.children()))).to_qkv.weight):
        y = enc(xd)
        with torch.no_grad():
            param.mul_(1.5)
        with pytest.raises(RuntimeError, match="modified"):
            y.sum().backward()
    with pytest.raises(NotImplementedError, match="batch > 1"):
        enc(torch.stack([xd, xd]))
    enc.enable_training(False)
    with pytest.raises(NotImplementedError, match="no_grad"):
        enc(xd)


# ------------------------------------------------------------------ RRTMIL around it
@pytest.mark.parametrize("name", list(NC.MIL_CASES))
def test_rrtmil_training_step(name):
    from rrt_mil_amd import RRTMIL
    cfg, state, x = NC.mil_inputs(name)
    model = RRTMIL(input_dim=NC.MIL_INPUT_DIM, **cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    model = model.cuda().eval()
    xd = torch.from_numpy(x).cuda()
    label = torch.tensor([GC.LABEL])
    with torch.no_grad():
        logits_eval = model(xd[None])
    with pytest.raises(NotImplementedError, match="no_grad"):
        model(xd[None])
    assert model.online_encoder.enable_training() is model.online_encoder
    logits = model(xd[None])
    F.cross_entropy(logits, label.cuda()).backward()
    got = {k: p.grad for k, p in model.named_parameters()}

    def reference(dtype):
        p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in state.items()}
        lg = NR.rrtmil(torch.from_numpy(x).to(dtype), p, cfg, dtype=dtype)
        F.cross_entropy(lg[None], label).backward()
        return lg.detach(), {k: v.grad for k, v in p.items()}
    (l64, r64), (l32, r32) = reference(torch.float64), reference(torch.float32)
    fails = []
    judge_forward("RRTMIL", name, "logits (graph)", logits[0], l64, l32, fails)
    judge_forward("RRTMIL", name, "logits (eval)", logits_eval[0], l64, l32, fails)
    assert set(got) == set(r64)
    for k in r64:
        if r64[k] is None:
            assert got[k] is None, k
            continue
        assert got[k] is not None, k
        judge_1e3("RRTMIL", name, "d " + k.replace("online_encoder.", "enc.").replace(".weight", ".w").replace(".bias", ".b"),
                  got[k], r64[k], r32[k], fails)
    assert not fails, "\n".join(fails)
    # one optimiser step in train() runs and changes every parameter that has a gradient; the one-call head entries keep raising
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    opt.zero_grad()
    torch.manual_seed(5)
    loss = F.cross_entropy(model(xd[None]), label.cuda())
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    opt.step()
    model.eval()
    with torch.no_grad():
        for call in (lambda: model.forward_bag(xd), lambda: model.forward_bags([xd, xd])):
            with pytest.raises(NotImplementedError, match="ntrans"):
                call()
