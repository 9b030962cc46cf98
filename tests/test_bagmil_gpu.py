"""GPU (-m gpu): the ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL heads.  The kernels of csrc/bag_pool.hip alone (mean pool,
its adjoint, the deconfounder), the five classes on their one-call path, their API and their training path, against the
float64 restatement tests/bagmil_ref.py (pinned to the reference's own float64 run by tests/test_bagmil_cpu.py) and against
the reference's goldens (tools/make_golden_bagmil.py) -- never against another kernel.

Bound per forward quantity, the project's stage rule: err <= max(2e-5, 8 x e32) relative to max(1, max |float64 reference|),
e32 = the error of the same restatement evaluated in plain fp32 on the CPU on the same inputs; against a golden the
reference's own recorded e32 is the floor of e32.  Arg-maxima are exact (every max-pool case holds a float64 margin of 1e-3
of the largest |logit|: tests/test_bagmil_cpu.py).  Gradients, the project's gradient rule: within 1e-3 of that gradient
tensor's own largest entry.  Two tensors have no largest entry to be relative to, because their float64 gradient cancels
identically (~1e-17): the EPEG bias, held to exactly zero (tests/test_dsmil_gpu.py), and the bias of an attention pool's
score Linear and of IBMIL's W_k (a constant added to every score of a softmax: the softmax adjoint sums to zero), which fp32
cannot cancel exactly and which is held, by the `_grad_tol` rule of tests/test_clam_gpu.py for that very tensor, to 1e-5 of
the term whose cancellation makes the zero, taken from the float64 restatement (test_gradients says which; measured:
errors of 2e-9 .. 6e-8 against bounds of 5e-7 .. 3e-6).  The bf16-autocast cases: 2e-2 on the logits, the bound of
tests/test_clam_gpu.py's autocast case.

Every output is NaN-filled with canary rows behind it, workspaces have exactly the queried size with canary bytes behind them,
every call runs twice and must give the same bits; nothing more runs after a device error.  The case lists are module data
of tests/bagmil_cases.py; importing this module needs no device."""
import copy
import ctypes as C
import functools
import pickle
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bagmil_cases as BC
import bagmil_ref as R
from conftest import load_golden
from rrt_mil_amd import ABMIL, GatedABMIL, IBMIL, MaxMIL, MeanMIL, RRTEncoder, _lib

pytestmark = pytest.mark.gpu

CLASSES = {"attmil": ABMIL, "gattmil": GatedABMIL, "ibmil": IBMIL, "meanmil": MeanMIL, "maxmil": MaxMIL}
TOL, E32_FACTOR, GRAD_TOL, AUTOCAST_TOL = 2e-5, 8.0, 1e-3, 2e-2
CANARY = 1234.5
_TMP = tempfile.TemporaryDirectory()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """a device error is sticky: nothing more is started on a device that reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is run on it: {e}", returncode=3)


def judge(case, what, got, ref64, ref32, fails, e32_floor=0.0):
    """one quantity against float64: bound max(TOL, 8 x e32); e32_floor: the reference's own recorded e32 (golden cases)"""
    ref64, ref32 = torch.as_tensor(ref64).detach(), torch.as_tensor(ref32).detach()
    e32 = max(R.rel_err(ref32, ref64), e32_floor)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (case, what, got.shape, ref64.shape)
    err = R.rel_err(got, ref64) if bool(torch.isfinite(got).all()) else float("inf")
    bound = max(TOL, E32_FACTOR * e32)
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


def dev(a):
    return torch.as_tensor(np.asarray(a)).to(torch.float32).contiguous().cuda()


class Out:
    """an output of `shape`, NaN-filled, with 8 canary rows behind it"""

    def __init__(self, *shape, dtype=torch.float32):
        row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        fill = float("nan") if dtype.is_floating_point else -7
        self.buf = torch.full((shape[0] + 8, row), fill, dtype=dtype, device="cuda")
        self.buf[shape[0]:] = 1234 if not dtype.is_floating_point else CANARY
        self.shape = shape

    @property
    def t(self):
        return self.buf[:self.shape[0]].view(self.shape)

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.shape[0]:] == (CANARY if self.buf.dtype.is_floating_point else 1234)).all()), \
            f"{what}: wrote behind its output"


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
            assert torch.equal(a.t.view(torch.int32) if a.t.dtype == torch.float32 else a.t,
                               b.t.view(torch.int32) if b.t.dtype == torch.float32 else b.t), f"{what}: two runs differ in their bits"
    return res[0]


def size_of(fn, *args):
    need = C.c_size_t()
    _lib.check(fn(*args, C.byref(need)), fn.__name__)
    return need.value


# ------------------------------------------------------------------ kernels alone: the mean pool and its adjoint
def run_mean(y, w, b, want_colmean=True):
    lib = _lib.load()
    (n, dim), c = y.shape, w.shape[0]
    need = size_of(lib.rrt_bag_mean_workspace_size, n, dim, c)
    lg, cm, _ = twice(lambda a, m, s: lib.rrt_bag_mean_f32(y.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                                          a.ptr(), m.ptr() if want_colmean else None, n, dim, c, s.ptr(), s.n,
                                                          stream()),
                      lambda: (Out(c), Out(dim), Ws(need)), "rrt_bag_mean_f32")
    if not want_colmean:
        assert bool(torch.isnan(cm.t).all())
    return lg.t, cm.t


def run_mean_backward(dl, cm, w, n):
    lib = _lib.load()
    c, dim = w.shape
    dy, dw, db = twice(lambda a, b_, c_: lib.rrt_bag_mean_backward_f32(dl.data_ptr(), cm.data_ptr(), w.data_ptr(), a.ptr(), b_.ptr(),
                                                                       c_.ptr(), n, dim, c, stream()),
                       lambda: (Out(n, dim), Out(c, dim), Out(c)), "rrt_bag_mean_backward_f32")
    return dy.t, dw.t, db.t


@pytest.mark.parametrize("c", BC.MEAN_CS)
@pytest.mark.parametrize("dim", BC.MEAN_DIMS)
def test_bag_mean_forward_and_adjoint(dim, c):
    fails = []
    for n in BC.MEAN_NS:
        y, w, b, dl = BC.mean_inputs(n, dim, c)
        case = f"mean n{n} d{dim} c{c}"
        (l64, m64), (l32, m32) = R.bag_mean(y, w, b, torch.float64), R.bag_mean(y, w, b, torch.float32)
        yd, wd, bd = dev(y), dev(w), dev(b)
        lg, cm = run_mean(yd, wd, bd)
        judge(case, "logits", lg, l64, l32, fails)
        judge(case, "colmean", cm, m64, m32, fails)
        # the adjoint, from the fp32 rounding of the float64 column mean
        cmi = m64.float()
        dy, dw, db = run_mean_backward(dev(dl), dev(cmi), wd, n)
        r64, r32 = R.bag_mean_backward(dl, cmi, w, n, torch.float64), R.bag_mean_backward(dl, cmi, w, n, torch.float32)
        for name, got, a, b_ in zip(("dy", "dW", "db"), (dy, dw, db), r64, r32):
            judge(case, name, got, a, b_, fails)
        assert torch.equal(dy.view(torch.int32), dy[:1].view(torch.int32).expand(n, -1)), f"{case}: dy rows differ in their bits"
        assert torch.equal(db.cpu(), torch.from_numpy(dl)), f"{case}: db is d_logits"
    lg2, _ = run_mean(yd, wd, bd, want_colmean=False)               # colmean is optional: the same logits bits
    assert torch.equal(lg2, lg)
    lg3, _ = run_mean(yd, wd, None)                                 # no bias
    judge(case, "logits no bias", lg3, R.bag_mean(y, w, None, torch.float64)[0], R.bag_mean(y, w, None, torch.float32)[0], fails)
    assert not fails, "\n".join(fails)


def test_bag_mean_nan_propagates():
    y, w, b, _ = BC.mean_inputs(2049, 512, 2)
    y = y.copy()
    y[1500, 7] = np.nan
    lg, cm = run_mean(dev(y), dev(w), dev(b))
    assert bool(torch.isnan(lg).all()) and bool(torch.isnan(cm[7])) and int(torch.isnan(cm).sum()) == 1


# ------------------------------------------------------------------ kernels alone: the deconfounder
def run_deconf(arrs, dims, want=True):
    lib = _lib.load()
    dim, v, j, c, k = dims
    t = [dev(a) for a in arrs]
    lg, a, cf = twice(lambda o1, o2, o3: lib.rrt_deconf_head_f32(*[x.data_ptr() for x in t], o1.ptr(), o2.ptr() if want else None,
                                                                o3.ptr() if want else None, dim, k, v, j, c, stream()),
                      lambda: (Out(c), Out(k), Out(v)), "rrt_deconf_head_f32")
    if not want:
        assert bool(torch.isnan(a.t).all()) and bool(torch.isnan(cf.t).all())
    return lg.t, a.t, cf.t


@pytest.mark.parametrize("k", BC.DECONF_KS)
@pytest.mark.parametrize("dim,v,j,c", BC.DECONF_SHAPES, ids=lambda x: str(x))
def test_deconf_head(dim, v, j, c, k):
    fails = []
    for gain in BC.DECONF_GAINS:
        arrs = BC.deconf_inputs(dim, v, j, c, k, gain)
        r64, r32 = R.deconf_head(*arrs, dtype=torch.float64), R.deconf_head(*arrs, dtype=torch.float32)
        peak = float(r64[3].abs().max())
        assert abs(peak - 1.0) < 1e-5 if gain == 1.0 else BC.PEAK_RANGE[0] <= peak <= BC.PEAK_RANGE[1], peak
        case = f"deconf d{dim} v{v} j{j} c{c} k{k} gain {gain:g}"
        lg, a, cf = run_deconf(arrs, (dim, v, j, c, k))
        for name, got, x, y in zip(("logits", "a", "cf"), (lg, a, cf), r64, r32):
            judge(case, name, got, x, y, fails)
        assert abs(float(a.double().sum()) - 1.0) < 1e-5
        bare = run_deconf(arrs, (dim, v, j, c, k), want=False)[0]   # optional outputs absent: the same logits bits
        assert torch.equal(bare, lg)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ whole heads
def make_model(kind, rrt):
    m = BC.construct(CLASSES, kind, rrt=RRTEncoder(drop_out=0., **BC.ENC_CFG) if rrt else None,
                     conf_path=BC.conf_file(_TMP.name) if kind == "ibmil" else False, bias=rrt)
    state = BC.head_state(m.state_dict(), kind)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    return m.cuda().eval(), state


@functools.lru_cache(maxsize=2)
def reference(kind, rrt, n):
    """the restatement on the case's inputs in float64 (with a graph for the gradient cases) and in fp32; computed once"""
    _m, state = make_model(kind, rrt)
    x = BC.bag(kind, rrt, n)
    kw = dict(enc_cfg=BC.ENC_CFG, act=BC.ACT[kind], gate_act=BC.ACT[kind])
    return (R.head(kind, x, state, dtype=torch.float64, grad=(kind, rrt, n) in BC.GRAD_CASES, **kw),
            R.head(kind, x, state, dtype=torch.float32, **kw))


EXTRAS = {"attmil": dict(return_attn=True, return_features=True), "gattmil": dict(return_attn=True, return_features=True),
          "ibmil": dict(return_attn=True, return_features=True, return_deconf=True), "meanmil": dict(return_features=True),
          "maxmil": dict(return_argmax=True)}
# forward_bag's names -> the restatement's
NAMES = {"logits": "logits", "attn": "attn", "features": "pooled", "deconf_a": "deconf_a", "deconf_cf": "deconf_cf"}


@pytest.mark.parametrize("kind,rrt,n", BC.WHOLE_CASES, ids=lambda v: str(v))
def test_whole_head(kind, rrt, n):
    model, _state = make_model(kind, rrt)
    r64, r32 = reference(kind, rrt, n)
    x = torch.from_numpy(BC.bag(kind, rrt, n)).cuda()
    with torch.no_grad():
        out = model.forward_bag(x, **EXTRAS[kind])
        out2 = model.forward_bag(x, **EXTRAS[kind])
        bare = model.forward_bag(x)
    torch.cuda.synchronize()
    for k_ in out:
        assert torch.equal(out[k_], out2[k_]), f"{k_}: two runs differ in their bits"
    assert torch.equal(bare, out["logits"]) and bare.shape == (1, BC.N_CLASSES[kind])
    cid, fails = BC.case_id(kind, rrt, n), []
    gold = load_golden(f"bagmil_{kind}")
    for mine, theirs in NAMES.items():
        if mine not in out:
            continue
        theirs = "colmean" if (kind == "meanmil" and mine == "features") else theirs
        judge(cid, mine, out[mine], r64[theirs], r32[theirs], fails)
        if f"{cid}/{theirs}" in gold:
            got = out[mine][torch.from_numpy(gold[f"{cid}/attn_idx"]).cuda()] if mine == "attn" else out[mine]
            g = torch.from_numpy(gold[f"{cid}/{theirs}"])
            judge(cid, mine + " golden", got, g, g, fails, e32_floor=float(gold[f"{cid}/e32_{theirs}"]))
    if kind == "maxmil":
        assert out["argmax"].cpu().tolist() == r64["argmax"].tolist() == gold[f"{cid}/argmax"].tolist()
    assert not fails, "\n".join(fails)


def test_max_pool_tie_reports_the_lower_index():
    """two identical rows hold the maximum of class 0 (rrt=None: identical rows give identical scores): the lower index"""
    model, state = make_model("maxmil", False)
    x = BC.bag("maxmil", False, 300).copy()
    s = R.head("maxmil", x, state, act=BC.ACT["maxmil"])["scores"]
    top = int(s[:, 0].argmax())
    for other in (top + 150) % 300, (top + 1) % 300:
        x2 = x.copy()
        x2[other] = x2[top]
        with torch.no_grad():
            out = model.forward_bag(torch.from_numpy(x2).cuda(), return_argmax=True)
        ref = R.head("maxmil", x2, state, act=BC.ACT["maxmil"])
        assert float(ref["scores"][other, 0]) == float(ref["scores"][top, 0]) == float(ref["scores"][:, 0].max())
        assert int(out["argmax"][0]) == min(top, other)
        assert R.rel_err(out["logits"].cpu(), ref["logits"]) <= TOL


@pytest.mark.parametrize("kind,rrt,n", BC.AUTOCAST_CASES, ids=lambda v: str(v))
def test_attention_heads_autocast_bf16(kind, rrt, n):
    model, _state = make_model(kind, rrt)
    x = torch.from_numpy(BC.bag(kind, rrt, n)).cuda()
    g = load_golden(f"bagmil_{kind}")[f"{BC.case_id(kind, rrt, n)}/logits"]
    with torch.no_grad():
        f32 = model(x[None])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lo, lo2 = model(x[None]), model(x[None])
    torch.cuda.synchronize()
    err = float(np.abs(lo.float().cpu().numpy() - g).max())
    print(f"{kind}: bf16 logits err {err:.3e}; distance to the fp32 run {float((lo.float() - f32).abs().max()):.3e}")
    assert lo.dtype == torch.float32 and err <= AUTOCAST_TOL
    assert float((lo - f32).abs().max()) > 1e-5                   # visibly not the fp32 result: the mode is on
    assert torch.equal(lo, lo2)


# ------------------------------------------------------------------ API
@pytest.mark.parametrize("rrt", [False, True])
@pytest.mark.parametrize("kind", BC.HEADS)
def test_api(kind, rrt):
    """forward_bag == model(x) == forward_bags(streams=1), forward_bags(streams=4) == forward_bag(solo=False), bit for bit,
    on a mixed list; a dirtied workspace changes nothing; pickling and deepcopy drop the workspace"""
    model, _state = make_model(kind, rrt)
    ind = BC.INPUT_DIM[kind]
    bags = [torch.from_numpy(BC.synth.bag(n, ind, tag=f"bagmil/api/{i}", nonneg=True)).cuda() for i, n in enumerate((250, 37, 2, 700))]
    with torch.no_grad():
        solo = [model.forward_bag(b) for b in bags]
        shared = [model.forward_bag(b, solo=False) for b in bags]
        assert all(a.shape == (1, BC.N_CLASSES[kind]) for a in solo)
        for b, a in zip(bags, solo):
            assert torch.equal(model(b[None]), a) and torch.equal(model(b), a)
        mixed = [bags[0], bags[1][None], bags[2], bags[3][None]]
        for o, a in zip(model.forward_bags(mixed, streams=1), solo):
            assert torch.equal(o, a)
        for o, a in zip(model.forward_bags(mixed, streams=4), shared):
            assert torch.equal(o, a)
        if not rrt:
            assert all(torch.equal(a, b) for a, b in zip(solo, shared))
        kw = EXTRAS[kind]
        for o, b in zip(model.forward_bags(mixed, streams=4, **kw), bags):
            r = model.forward_bag(b, solo=False, **kw)
            assert set(o) == set(r) and all(torch.equal(o[k_], r[k_]) for k_ in r)
        assert model._ws is not None
        model._ws.fill_(0xFF)                                      # NaN patterns everywhere in the workspace
        assert torch.equal(model.forward_bag(bags[0]), solo[0])
        with pytest.raises(ValueError):
            model(torch.stack([bags[0], bags[0]]))
        with pytest.raises(ValueError):
            model.forward_bag(bags[0], **{"return_argmax" if kind != "maxmil" else "return_attn": True})
    for clone in (copy.deepcopy(model), pickle.loads(pickle.dumps(model))):
        assert clone._ws is None and "_slots" not in clone.__dict__ and "_w16_key" not in clone.__dict__
        with torch.no_grad():
            assert torch.equal(clone.forward_bag(bags[1]), solo[1])
    if kind == "attmil":                                           # the reference's return values
        with torch.no_grad():
            y, a = model(bags[1][None], return_attn=True)
            y2, raw = model(bags[1][None], return_attn=True, no_norm=True)
        assert a.shape == (1, 37) and raw.shape == (37, 1) and torch.equal(y, solo[1]) and torch.equal(y2, solo[1])
        assert abs(float(a.sum()) - 1.0) < 1e-5
        assert torch.allclose(torch.softmax(raw[:, 0], 0), a[0], atol=1e-6)
    # in train() the one-call entries refuse, the module call takes the layer path and records a graph
    stochastic = kind == "gattmil"                                 # (its Dropout(0.25) is always there)
    model.train()
    if stochastic:
        with pytest.raises(NotImplementedError):
            model.forward_bag(bags[1])
        with pytest.raises(NotImplementedError):
            model.forward_bags(bags[:2])
    out = model(bags[1][None])
    assert out.shape == (1, BC.N_CLASSES[kind]) and out.grad_fn is not None


# ------------------------------------------------------------------ training
@pytest.mark.parametrize("kind,rrt,n", BC.GRAD_CASES, ids=lambda v: str(v))
def test_gradients(kind, rrt, n):
    model, _state = make_model(kind, rrt)
    r64, _r32 = reference(kind, rrt, n)
    gold = load_golden(f"bagmil_{kind}")
    cid = BC.case_id(kind, rrt, n)
    info = gold["cfg"]["cases"][cid]
    x = torch.from_numpy(BC.bag(kind, rrt, n)).cuda()[None].requires_grad_(True)
    logits = model(x)                                              # eval() with a graph: the layer path, nothing stochastic
    assert logits.grad_fn is not None
    loss = F.cross_entropy(logits, torch.tensor([info["label"]], device="cuda"))
    loss.backward()
    torch.cuda.synchronize()
    loss64 = F.cross_entropy(r64["logits"], torch.tensor([info["label"]]))
    names = [k for k, v in r64["params"].items() if v.is_floating_point() and k != "confounder_feat"]
    ref = dict(zip(["x"] + names, torch.autograd.grad(loss64, [r64["x_leaf"]] + [r64["params"][k] for k in names],
                                                      allow_unused=True, retain_graph=True)))
    loss64_t = loss64
    loss, loss64 = float(loss.detach()), float(loss64.detach())
    assert abs(loss - loss64) <= 1e-3 * abs(loss64) and abs(loss64 - float(gold[f"{cid}/loss"])) < 1e-9
    # the terms whose cancellation makes a score bias's zero (module docstring): sum_n A_n dA_n = M . dM for the pool's; for
    # W_k.bias, added to every confounder's key, sum_i a_i da_i q_j / sqrt(J) = (cf . dcf) q_j / sqrt(J)
    dot = lambda node: abs(float((r64[node].detach() * torch.autograd.grad(loss64_t, r64[node], retain_graph=True)[0]).sum()))   # noqa: E731
    naturals = {}
    if "M" in r64:
        naturals["attention.2.bias"] = naturals["attention_c.bias"] = dot("M")
    if "cf_node" in r64:
        q = r64["q_node"].detach()
        naturals["W_k.bias"] = dot("cf_node") * float(q.abs().max()) / q.shape[1] ** 0.5
    fails, seen = [], 0
    for name, grad in [("x", x.grad[0])] + [(k, p.grad) for k, p in model.named_parameters()]:
        if name in info["none"]:
            assert grad is None or float(grad.abs().max()) == 0.0, name
            continue
        assert grad is not None and ref[name] is not None, name
        got, want = grad.detach().double().cpu(), ref[name].detach()
        scale = float(want.abs().max())
        key = f"{cid}/g__" + name.replace(".", "__")
        if name.endswith("pe.bias"):
            assert scale < 1e-12 and float(gold[key + "__max"]) < 1e-12 and float(got.abs().max()) == 0.0, name
            seen += 1
            continue
        zero = name in naturals                                    # an identically-zero reference: a score bias
        assert scale <= 1e-9 * naturals[name] if zero else scale > 1e-12, (name, scale)
        tol = 1e-5 * naturals[name] if zero else GRAD_TOL * scale
        assert zero or abs(scale - float(gold[key + "__max"])) <= 1e-6 * scale, name
        err = float((got.reshape(want.shape) - want).abs().max())
        if key + "__full" in gold:
            g2, gref = got.reshape(gold[key + "__full"].shape).numpy(), gold[key + "__full"]
        else:
            g2, gref = got.reshape(got.shape[0], -1).numpy()[gold[key + "__rows"]], gold[key + "__vals"]
        err = max(err, float(np.abs(g2 - gref).max()))
        print(f"{cid} {name}: err {err:.3e} scale {scale:.3e} tol {tol:.3e}")
        if not (bool(torch.isfinite(got).all()) and err <= tol):
            fails.append(f"{name}: {err:.3e} > {tol:.3e} (scale {scale:.3e})")
        seen += 1
    assert seen >= 20 and not fails, "\n".join(fails)
