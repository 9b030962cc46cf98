"""GPU (-m gpu): TransMIL's one-call training step (rrt_transmil_forward_train_f32 / rrt_transmil_backward_f32 behind
``TransMIL.enable_training(one_call=True)``), its own kernels one stage at a time (csrc/transmil_bwd.hip, the PPEG-side adjoint
of csrc/peg.hip) and its API -- against float64 autograd of the restatements tests/nystrom_ref.py (pinned to the reference's
own float64 run) and tests/transmil_step_ref.py, never against another kernel.

Error of a gradient: max |got - ref64| / max |ref64| (every judged quantity must have max |ref64| > 1e-4).  Bound:
max(2e-5, 8 x e32), e32 = the fp32 CPU autograd of the same restatement on the same inputs against the float64 one -- measured
here, never read off a kernel.  Outputs are NaN-filled with canary rows behind them (a seeded prefill where a stage zeroes or
may leave an output alone), stashes and workspaces have exactly the queried size with canary bytes behind them, every call runs
twice and must give the same bits.  The helpers (judge, Out, Ws, twice) are those of tests/test_nystrom_grad_gpu.py.  With
RRT_TRANSMIL_STEP_ERRORS_OUT=<file> the module writes its error table (kept as profiles/transmil_step_errors.txt)."""
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import nystrom_grad_cases as GC
import nystrom_ref as R
import test_nystrom_grad_gpu as G
import transmil_cases as TC
import transmil_step_ref as SR
from conftest import load_golden
from rrt_mil_amd import _lib, synth

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad")]

RECORDS = []
ACTS = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU}
DROP_SEED = 0x5EED1234ABCD
Out, Ws, twice, dev, stream, size_of, FILLS = G.Out, G.Ws, G.twice, G.dev, G.stream, G.size_of, G.FILLS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_TRANSMIL_STEP_ERRORS_OUT")
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


def judge(grp, case, what, got, ref64, ref32, fails, e32_floor=0.0):
    """tests/test_nystrom_grad_gpu.py's judge (same error, same bound), recorded in this module's table"""
    n = len(G.RECORDS)
    G.judge(grp, case, what, got, ref64, ref32, fails, e32_floor)
    RECORDS.extend(G.RECORDS[n:])
    del G.RECORDS[n:]


def normal(name, shape, scale=1.0):
    return torch.from_numpy(synth.normal("transmil_step/" + name, tuple(shape))) * scale


def ptr(t):
    return t.data_ptr() if t is not None else None


def ptrs3(ts):
    return (C.c_void_p * 3)(*[t.ptr() if isinstance(t, Out) else t.data_ptr() for t in ts])


# ------------------------------------------------------------------ the step
def make_model(input_dim, act, N, dropout=False):
    from rrt_mil_amd import TransMIL
    state, x = TC.model_inputs(input_dim, N)
    model = TransMIL(input_dim, 2, dropout, act)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return model.cuda().eval(), state, x


@functools.lru_cache(maxsize=None)
def reference(input_dim, act, N, dtype, mask_key=None):
    """(logits, {parameter gradients, dx}) of cross-entropy(transmil_step) by CPU autograd in `dtype`; computed once per case"""
    state, x = TC.model_inputs(input_dim, N)
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).to(dtype).requires_grad_(True)
    logits = SR.transmil_step(xd, p, act, dtype=dtype, masks=MASKS.get(mask_key))
    F.cross_entropy(logits[None], torch.tensor([GC.LABEL])).backward()
    return logits.detach(), {**{k: v.grad for k, v in p.items()}, "dx": xd.grad}


MASKS = {}       # mask_key -> {"fc1", "attn1", "attn2"}: CPU multipliers regenerated through rrt_debug_drop_mask_f32


def step_backward(model, x, x_grad=True):
    model.zero_grad(set_to_none=True)
    xd = torch.from_numpy(x).cuda().requires_grad_(x_grad)
    logits = model(xd)
    assert logits.requires_grad and logits.shape == (1, 2)
    F.cross_entropy(logits, torch.tensor([GC.LABEL], device="cuda")).backward()
    got = {k: p.grad.clone() for k, p in model.named_parameters()}
    if x_grad:
        got["dx"] = xd.grad.clone()
    else:
        assert xd.grad is None
    return logits.detach(), got


def judge_step(grp, case, logits, got, input_dim, act, N, fails, mask_key=None):
    l64, r64 = reference(input_dim, act, N, torch.float64, mask_key)
    l32, r32 = reference(input_dim, act, N, torch.float32, mask_key)
    judge(grp, case, "logits", logits[0], l64, l32, fails)
    assert set(got) == set(r64) and len(got) == 26
    for k in r64:
        judge(grp, case, k, got[k].reshape(r64[k].shape), r64[k], r32[k], fails)
    return l64, l32


@pytest.mark.parametrize("input_dim,act,N", SR.STEP_CASES + [(64, "none", 37)], ids=lambda v: str(v))
def test_step_gradients(input_dim, act, N):
    model, _state, x = make_model(input_dim, act, N)
    with torch.no_grad():
        inference = model(torch.from_numpy(x).cuda())
    assert model.enable_training(one_call=True) is model
    logits, got = step_backward(model, x)
    logits2, again = step_backward(model, x)
    assert torch.equal(logits.view(torch.int32), logits2.view(torch.int32))
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{k}: two steps differ in their bits"
    with torch.no_grad():
        assert torch.equal(model(torch.from_numpy(x).cuda()), inference)     # no graph: still the one-call inference path
    case, fails = f"TransMIL({input_dim}, {act}) N{N}", []
    l64, l32 = judge_step("step", case, logits, got, input_dim, act, N, fails)
    # ... and the inference call's logits as values, within the same bound
    big = float(l64.abs().max())
    e32 = float((l32.double() - l64).abs().max()) / big
    err = float((logits[0].double().cpu() - inference[0].double().cpu()).abs().max()) / big
    print(f"{case} logits vs the inference call: {err:.3e} (e32 {e32:.2e})")
    if not err <= max(G.TOL, G.E32_FACTOR * e32):
        fails.append(f"{case} logits vs the inference call: {err:.3e}")
    if (input_dim, act, N) in GC.GOLDEN_MODEL_CASES:
        gold, key = load_golden("transmil_grad"), "model/" + GC.model_key(input_dim, act, N)
        for k in got:
            ref = torch.from_numpy(gold[f"{key}/{k}"])
            g2 = got[k].cpu()
            rows = torch.stack([g2[0], g2[-1]]) if k == "dx" else GC.golden_rows(g2)
            judge("step", case, k + " golden", rows, ref, ref, fails, e32_floor=float(gold[f"{key}/e32/{k}"]))
    assert not fails, "\n".join(fails)


def test_step_without_an_input_gradient():
    model, _state, x = make_model(64, "gelu", 37)
    model.enable_training(one_call=True)
    logits, got = step_backward(model, x)
    logits2, nodx = step_backward(model, x, x_grad=False)
    assert torch.equal(logits, logits2) and set(nodx) == set(got) - {"dx"}
    for k in nodx:
        assert torch.equal(got[k].view(torch.int32), nodx[k].view(torch.int32)), f"{k} depends on whether dx is computed"


# ------------------------------------------------------------------ the C ABI itself: canaries, exact sizes, two runs
def make_masks(N, fc1_p, attn_p):
    """the step's three masks as CPU multipliers, regenerated through rrt_debug_drop_mask_f32 -> their key in MASKS"""
    rows, key = 1 + SR.side_of(N) ** 2, (N, DROP_SEED, fc1_p, attn_p)
    if key not in MASKS:
        MASKS[key] = {"fc1": drop_mask(N * 512, fc1_p, DROP_SEED, SR.DROP_TAGS["fc1"]).reshape(N, 512),
                      "attn1": drop_mask(rows * 512, attn_p, DROP_SEED, SR.DROP_TAGS["attn1"]).reshape(rows, 512),
                      "attn2": drop_mask(512, attn_p, DROP_SEED, SR.DROP_TAGS["attn2"])}
    return key


@pytest.mark.parametrize("N,fc1_p,attn_p,row", [(37, 0.0, 0.0, False), (250, 0.25, 0.1, False), (37, 0.0, 0.0, True),
                                                (250, 0.25, 0.1, True), (1000, 0.0, 0.0, True)], ids=lambda v: str(v))
def test_step_c_abi_canaries_and_bits(N, fc1_p, attn_p, row):
    """both export families called directly (row: the cls-row twin), cross-entropy's d_logits formed in between; held to
    float64 like the module's step"""
    lib = _lib.load()
    model, _state, x = make_model(64, "gelu", N)
    params = model._step_params()
    names = {id(p): k for k, p in model.named_parameters()}
    keep = []
    d, w = model._desc_weights(keep)
    xd = torch.from_numpy(x).cuda()
    sizes, fwd, bwd = ((lib.rrt_debug_transmil_train_sizes_row, lib.rrt_debug_transmil_forward_train_row_f32,
                        lib.rrt_debug_transmil_backward_row_f32) if row else
                       (lib.rrt_transmil_train_sizes, lib.rrt_transmil_forward_train_f32, lib.rrt_transmil_backward_f32))
    sb, wb = C.c_size_t(), C.c_size_t()
    _lib.check(sizes(C.byref(d), N, C.byref(sb), C.byref(wb)), "train_sizes")
    onehot = F.one_hot(torch.tensor([GC.LABEL]), 2).float().cuda()
    runs = []
    for run in range(2):
        logits, stash, ws = Out(1, 2), Ws(sb.value, FILLS[run]), Ws(wb.value, FILLS[1 - run])
        grads, dx = [Out(*p.shape) for p in params], Out(N, 64)
        gs = _lib.TransmilGrads()
        slots = (C.c_void_p * 25).from_buffer(gs)
        for i, g in enumerate(grads):
            slots[i] = g.ptr()
        _lib.check(fwd(C.byref(d), C.byref(w), xd.data_ptr(), logits.ptr(), N, stash.ptr(), stash.n, fc1_p, attn_p, DROP_SEED,
                       stream()), "forward_train")
        d_logits = (torch.softmax(logits.t, dim=1) - onehot)[0].contiguous()       # d cross-entropy / d logits
        _lib.check(bwd(C.byref(d), C.byref(w), xd.data_ptr(), d_logits.data_ptr(), stash.ptr(), stash.n, C.byref(gs), dx.ptr(), N,
                       ws.ptr(), ws.n, fc1_p, attn_p, DROP_SEED, stream()), "backward")
        torch.cuda.synchronize()
        for o in [logits, stash, ws, dx] + grads:
            o.check("the step")
        outs = [logits, dx] + grads
        assert all(bool(torch.isfinite(o.t).all()) for o in outs), "an output was not written everywhere"
        runs.append(outs)
    for a, b in zip(*runs):
        assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)), "two runs differ in their bits"
    got = {names[id(p)]: g.t for p, g in zip(params, runs[0][2:])}
    got["dx"] = runs[0][1].t
    case, fails = f"C ABI {'cls-row twin' if row else 'step'} N{N} p {fc1_p} {attn_p}", []
    judge_step("step, cls-row twin" if row else "step, C ABI", case, runs[0][0].t, got, 64, "gelu", N, fails,
               mask_key=make_masks(N, fc1_p, attn_p) if fc1_p or attn_p else None)
    assert not fails, "\n".join(fails)
    if not row and fc1_p == 0.0:
        # what the module returns is this call
        model.enable_training(one_call=True)
        xg = xd.clone().requires_grad_(True)
        out = model(xg)
        assert torch.equal(out[0], runs[0][0].t[0])
        F.cross_entropy(out, torch.tensor([GC.LABEL], device="cuda")).backward()
        assert float((xg.grad - runs[0][1].t).abs().max()) <= 1e-5 * float(xg.grad.abs().max())     # (torch's own d_logits)


# ------------------------------------------------------------------ dropout: the library's stateless mask
def drop_mask(n, p, seed, tag):
    """the multipliers (0 or 1 / (1 - p)) of n elements, through rrt_debug_drop_mask_f32"""
    src, dst = torch.ones(n, device="cuda"), torch.empty(n, device="cuda")
    _lib.check(_lib.load().rrt_debug_drop_mask_f32(src.data_ptr(), dst.data_ptr(), n, p, seed, tag, 1.0, stream()),
               "rrt_debug_drop_mask_f32")
    torch.cuda.synchronize()
    return dst.cpu()


@pytest.mark.parametrize("input_dim,act,N", SR.DROPOUT_CASES, ids=lambda v: str(v))
def test_step_dropout(input_dim, act, N):
    model, _state, x = make_model(input_dim, act, N, dropout=True)
    model.enable_training(one_call=True).train()
    fc1_p, attn_p = model._fc1[-1].p, model.layer1.attn.to_out[1].p
    assert (fc1_p, attn_p) == (0.25, 0.1)
    model.drop_seed = DROP_SEED
    key = make_masks(N, fc1_p, attn_p)
    for k, p in (("fc1", fc1_p), ("attn1", attn_p), ("attn2", attn_p)):
        m = MASKS[key][k]
        kept = float((m != 0).float().mean())
        assert bool(((m == 0) | ((m - 1 / (1 - p)).abs() < 1e-6)).all())
        assert abs(kept - (1 - p)) < (0.1 if k == "attn2" else 0.02), (k, kept)
    logits, got = step_backward(model, x)
    logits2, again = step_backward(model, x)
    assert torch.equal(logits, logits2)
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{k}: two steps differ in their bits"
    case, fails = f"TransMIL({input_dim}, {act}, dropout) N{N}", []
    judge_step("step, dropout", case, logits, got, input_dim, act, N, fails, mask_key=key)
    assert not fails, "\n".join(fails)
    model.drop_seed = DROP_SEED + 1
    other, _ = step_backward(model, x)
    assert not torch.equal(other, logits), "a second seed must change the logits"
    # without a pinned seed it comes from torch's CPU generator
    model.drop_seed = None
    torch.manual_seed(11)
    a, _ = step_backward(model, x)
    torch.manual_seed(11)
    b, _ = step_backward(model, x)
    c, _ = step_backward(model, x)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # eval(): no mask at all
    model.eval()
    e, _ = step_backward(model, x)
    l64, l32 = reference(input_dim, act, N, torch.float64)[0], reference(input_dim, act, N, torch.float32)[0]
    fails = []
    judge("step, dropout", case, "logits in eval()", e[0], l64, l32, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ stages
@pytest.mark.parametrize("side,Cc", SR.PPEG_CASES, ids=lambda v: str(v))
def test_ppeg_side_backward(side, Cc):
    lib, n = _lib.load(), side * side
    case = f"ppeg side {side} C {Cc}"
    x, dy = normal(f"ppeg/x/{side}/{Cc}", (n, Cc)), normal(f"ppeg/dy/{side}/{Cc}", (n, Cc))
    ws = [normal(f"ppeg/w{k}/{Cc}", (Cc, 1, k, k), 1.0 / k) for k in (7, 5, 3)]
    bs = [normal(f"ppeg/b{k}/{Cc}", (Cc,), 0.1) for k in (7, 5, 3)]
    r64, r32 = G.both(lambda x_, a, b, c, d, e, f: SR.ppeg_side(x_, [a, b, c], [d, e, f]), (x, *ws, *bs), dy)
    xd, dyd, wd = dev(x), dev(dy), [dev(w) for w in ws]
    need = size_of(lib.rrt_ppeg_side_backward_workspace_size, side, Cc)

    def call(dx, w7, w5, w3, b7, b5, b3, wk):
        return lib.rrt_ppeg_side_backward_f32(xd.data_ptr(), dyd.data_ptr(), ptrs3(wd), dx.ptr(), ptrs3([w7, w5, w3]),
                                              ptrs3([b7, b5, b3]), side, Cc, wk.ptr(), wk.n, stream())

    outs = twice(call, lambda run: (Out(n, Cc), Out(Cc, 1, 7, 7), Out(Cc, 1, 5, 5), Out(Cc, 1, 3, 3), Out(Cc), Out(Cc), Out(Cc),
                                    Ws(need, FILLS[run])), "rrt_ppeg_side_backward_f32")
    fails = []
    for name, o, a, b in zip(("dx", "dw7", "dw5", "dw3", "db7", "db5", "db3"), outs, r64, r32):
        judge("ppeg_side_backward", case, name, o.t, a, b, fails)
    assert not fails, "\n".join(fails)
    # db is optional, as a whole and entry by entry: the other outputs keep their bits
    dx2, w7, w5, w3, b5, wk = Out(n, Cc), Out(Cc, 1, 7, 7), Out(Cc, 1, 5, 5), Out(Cc, 1, 3, 3), Out(Cc), Ws(need)
    some = (C.c_void_p * 3)(None, b5.ptr(), None)
    for db in (None, some):
        _lib.check(lib.rrt_ppeg_side_backward_f32(xd.data_ptr(), dyd.data_ptr(), ptrs3(wd), dx2.ptr(), ptrs3([w7, w5, w3]), db,
                                                  side, Cc, wk.ptr(), wk.n, stream()), "rrt_ppeg_side_backward_f32")
        torch.cuda.synchronize()
        for got, want in zip((dx2, w7, w5, w3), outs):
            assert torch.equal(got.t, want.t)
    assert torch.equal(b5.t, outs[5].t)


ASSEMBLE_N = sorted({n for _, _, n in SR.STEP_CASES})


@pytest.mark.parametrize("act", ["none", "relu", "gelu"])
@pytest.mark.parametrize("N", ASSEMBLE_N)
def test_assemble_backward(N, act):
    lib, D, side = _lib.load(), 512, SR.side_of(N)
    rows, case = 1 + side * side, f"assemble N {N} side {side} {act}"
    hpre, cls, d_seq = normal(f"asm/h/{N}", (N, D)), normal("asm/cls", (D,)), normal(f"asm/d_seq/{N}", (rows, D))
    hd, dd = dev(hpre), dev(d_seq)
    fails = []
    for p in (0.0, 0.25):
        mask = drop_mask(N * D, p, DROP_SEED, SR.DROP_TAGS["fc1"]).reshape(N, D) if p else None
        r64, r32 = G.both(lambda h, c: SR.assemble(h, c, act, mask), (hpre, cls), d_seq)
        # d_emb is written everywhere (NaN-filled); hpre is not read without an activation
        d_emb, d_cls = twice(lambda a, b: lib.rrt_transmil_assemble_backward_f32(
            dd.data_ptr(), hd.data_ptr() if act != "none" else None, a.ptr(), b.ptr(), N, D, ACTS[act], p, DROP_SEED, stream()),
            lambda run: (Out(N, D), Out(D)), "rrt_transmil_assemble_backward_f32")
        judge("assemble_backward", case, f"d_emb p {p}", d_emb.t, r64[0], r32[0], fails)
        judge("assemble_backward", case, f"d_cls p {p}", d_cls.t, r64[1], r32[1], fails)
        assert torch.equal(d_cls.t.cpu(), d_seq[0])
    assert not fails, "\n".join(fails)


@functools.lru_cache(maxsize=4)
def row_inputs(dim, heads, npad, gain):
    """the float64 run's qkv, kl, wz of a sequence of npad rows, rounded to fp32 (the stage's inputs)"""
    state, x = TC.attn_inputs(dim, heads, npad, gain)
    with torch.no_grad():
        r64 = R.nystrom(x, state, heads, dtype=torch.float64)
    assert r64["qkv"].shape[0] == npad
    return {k: r64[k].float() for k in ("qkv", "kl", "wz")}, torch.from_numpy(state["res_conv.weight"]).reshape(heads, -1)


def check_output_row(case, dim, heads, npad, gain, row, conv_w, fails):
    lib = _lib.load()
    st, _ = row_inputs(dim, heads, npad, gain)
    qkv, kl, wz = st["qkv"], st["kl"], st["wz"]
    ks = conv_w.shape[1] if conv_w is not None else 33
    hd = heads * 64
    d_o = normal(f"row/d_o/{case}", (hd,))
    qd, kd, wd, cd, dod = dev(qkv), dev(kl), dev(wz), dev(conv_w) if conv_w is not None else None, dev(d_o)
    # forward: against float64 with the error of the fp32 CPU evaluation
    fn = lambda q, k, w, c: SR.output_row(q, k, w, heads, c, row)      # noqa: E731
    with torch.no_grad():
        o64 = fn(qkv.double(), kl.double(), wz.double(), conv_w.double() if conv_w is not None else None)
        o32 = fn(qkv, kl, wz, conv_w)
    (o_row,) = twice(lambda a: lib.rrt_nystrom_output_row_f32(qd.data_ptr(), kd.data_ptr(), wd.data_ptr(), ptr(cd), a.ptr(), row,
                                                            npad, heads, ks, stream()),
                     lambda run: (Out(hd),), "rrt_nystrom_output_row_f32")
    judge("output_row", case, "o_row", o_row.t, o64, o32, fails)
    # backward: d_qkv is zeroed by the stage, d_conv_w is left alone without a conv: both on a seeded prefill
    r64, r32 = G.both(fn, (qkv, kl, wz, conv_w), d_o)
    pre_q, pre_c = normal(f"row/pre_q/{case}", (npad, 3 * hd)), normal(f"row/pre_c/{case}", (heads, ks))
    d_qkv, d_kl, d_wz, d_cw = twice(lambda a, b, c, d: lib.rrt_nystrom_output_row_backward_f32(
        qd.data_ptr(), kd.data_ptr(), wd.data_ptr(), ptr(cd), dod.data_ptr(), a.ptr(), b.ptr(), c.ptr(),
        d.ptr() if conv_w is not None else None, row, npad, heads, ks, stream()),
        lambda run: (Out(npad, 3 * hd, prefill=pre_q), Out(heads, 256, 64), Out(heads, 256, 64), Out(heads, ks, prefill=pre_c)),
        "rrt_nystrom_output_row_backward_f32")
    judge("output_row_backward", case, "d_qkv", d_qkv.t, r64[0], r32[0], fails)
    judge("output_row_backward", case, "d_kl", d_kl.t, r64[1], r32[1], fails)
    judge("output_row_backward", case, "d_wz", d_wz.t, r64[2], r32[2], fails)
    g = d_qkv.t.cpu()
    half = ks // 2 if conv_w is not None else -1
    reach = torch.zeros(npad, dtype=torch.bool)
    reach[max(0, row - half):min(npad, row + half + 1)] = conv_w is not None
    only_row = torch.zeros(npad, dtype=torch.bool)
    only_row[row] = True
    assert not bool(g[:, hd:2 * hd].any()), "the k third must be zero"
    assert not bool(g[~only_row, :hd].any()), "the q third must be zero outside the row"
    assert not bool(g[~reach, 2 * hd:].any()), "the v third must be zero outside the stencil's reach"
    if conv_w is not None:
        judge("output_row_backward", case, "d_conv_w", d_cw.t, r64[3], r32[3], fails)
    else:
        assert torch.equal(d_cw.t.cpu(), pre_c), "d_conv_w must stay untouched without a conv"


@pytest.mark.parametrize("gain", GC.GAINS)
@pytest.mark.parametrize("npad,row", list(SR.ROW_POSITIONS), ids=lambda v: str(v))
def test_output_row_pair(npad, row, gain):
    _, conv_w = row_inputs(128, 2, npad, gain)
    fails = []
    check_output_row(f"np{npad}_r{row}_g{int(gain)}", 128, 2, npad, gain, row, conv_w, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("ks", [None, 1, 33, 63], ids=lambda v: f"k{v}")
def test_output_row_pair_conv_kernels(ks):
    conv_w = None if ks is None else normal(f"row/conv_w/{ks}", (2, ks), ks ** -0.5)
    fails = []
    for npad, row in ((256, 20), (512, 500)):       # (row 20's softmax is all but one-hot: 0.99998 on one landmark)
        check_output_row(f"np{npad}_r{row}_k{ks}", 128, 2, npad, 6.0, row, conv_w, fails)
    assert not fails, "\n".join(fails)


def test_output_row_pair_wide():
    _, conv_w = row_inputs(512, 8, 1280, 6.0)
    fails = []
    check_output_row("d512_h8_np1280_r255", 512, 8, 1280, 6.0, 255, conv_w, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ API
def test_step_api():
    model, _state, x = make_model(64, "gelu", 37, dropout=True)
    xd = torch.from_numpy(x).cuda()
    label = torch.tensor([GC.LABEL], device="cuda")
    # the layer path before anything else: its bits are what one_call=False must give again afterwards
    model.enable_training()
    layer_logits = model(xd).detach().clone()
    model.enable_training(one_call=True)
    # retain_graph: a second backward through the same node gives the same bits
    loss = F.cross_entropy(model(xd), label)
    loss.backward(retain_graph=True)
    first = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    loss.backward()
    for k, p in model.named_parameters():
        assert torch.equal(p.grad.view(torch.int32), first[k].view(torch.int32)), k
    # torch.autograd.grad: the returned tensors are not overwritten by a later backward
    ps = list(model.parameters())
    out = model(xd)
    g1 = torch.autograd.grad(F.cross_entropy(out, label), ps, retain_graph=True)
    snap = [g.clone() for g in g1]
    torch.autograd.grad(2.0 * F.cross_entropy(out, label), ps)
    assert all(torch.equal(a, b) for a, b in zip(g1, snap))
    # return_features with a graph keeps taking the layer path
    logits, feat = model.forward_bag(xd, return_features=True)
    assert logits.requires_grad and feat.shape == (50, 512) and torch.equal(logits.detach(), layer_logits)
    # under autocast: exact fp32 all the same
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = model(xd)
    assert y.dtype == torch.float32 and torch.equal(y.detach(), out.detach())
    # an in-place parameter update between forward and backward must not go unnoticed
    loss = F.cross_entropy(model(xd), label)
    saved = model._fc2.bias.detach().clone()
    with torch.no_grad():
        model._fc2.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()
    with torch.no_grad():
        model._fc2.bias.copy_(saved)                         # (x + 1 - 1 is not x in fp32)
    # one_call=False afterwards: the layer path again, bit for bit
    model.enable_training()
    assert torch.equal(model(xd).detach(), layer_logits)
    # one Adam step in train() (dropout in _fc1 and in both attentions) changes every parameter
    model.enable_training(one_call=True).train()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(3)
    loss = F.cross_entropy(model(xd), label)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), k
    opt.step()
    for k, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[k]), f"{k} did not change"
    # opting out altogether: the refusals are back
    model.enable_training(False)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="eval"):
        model(xd)
