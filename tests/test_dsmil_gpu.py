"""GPU: the DSMIL head.  Stage kernels (csrc/dsmil_pool.hip: instance max, one-pass bag pool) against float64 torch
restatements of the reference's op order, MILNet against the reference's goldens (tools/make_golden_dsmil.py), and the
one-call / multi-bag entry points against the layer path.

Bounds (none of them taken from this code's own output):
  * stage forward: what tests/test_hip_parity.py::test_attn_pool_forward_backward and the branch-pool tests hold their
    kernels to -- B 2e-5, classes / cmax / A / a_raw 2e-5 * max(1, largest reference entry), logits 1e-4 * max(1, ...),
    columns of A sum to 1 within 1e-5; arg-maxima exact on inputs whose column maxima are separated by >= 0.1;
  * module against the goldens: logits, classes max, B 1e-4, A 1e-6, critical ids exact (the goldens guarantee a gap of
    1e-2 between the two largest instance scores of a column; dsmil_n2_wide 0.2 for the 2e-2 bf16 bound);
  * every gradient: 1e-3 of that tensor's own largest reference entry.  ONE tensor has no largest entry to be relative to:
    the EPEG bias ``rrt.layers.0.attn.attn.pe.bias`` -- a constant added to every score of a softmax row, whose adjoint
    sum_k P[q, k] (dP[q, k] - sum_j P[q, j] dP[q, j]) cancels identically (float64 leaves ~5e-17).  The encoder's backward
    returns exactly zero for it (tests/test_hip_parity.py holds it to that), which is what is asserted here: stricter than
    the `_grad_tol` rule of tests/test_clam_gpu.py (1e-5 of the largest cancelling term P dP) for any value of that term.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import golden_names, load_golden
from rrt_mil_amd import MILNet, RRTEncoder, _lib, synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda:0"
CASES = [n for n in golden_names("dsmil_") if n != "dsmil_keys"]
CANARY = 777.0
# 31 / 32 / 33: the bag stream's 32-token chunk; 127 / 128 / 129: the instance stream's 128-token block; 300, 1000: several
NS = (1, 8, 31, 32, 33, 100, 127, 128, 129, 300, 1000)


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(tag, shape):
    return torch.from_numpy(synth.normal(tag, shape)).to(DEV)


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.abs(got - ref).max())
    print(f"{what}: err {err:.3e} tol {tol:.1e}")
    assert np.isfinite(got).all() and err <= tol, (what, err, tol)


def _rel(ref):
    return max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ instance max stage
def _imax(y, w, b, want_classes=True):
    """rrt_instance_max_f32 on NaN-filled outputs with a canary row behind them and an exact-size workspace with canary bytes"""
    lib = _lib.load()
    (N, dim), K = y.shape, w.shape[0]
    need = C.c_size_t()
    _lib.check(lib.rrt_instance_max_workspace_size(N, dim, K, C.byref(need)), "ws")
    ws = torch.full((need.value + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[need.value:] = 0xA5
    classes = torch.full((N + 1, K), float("nan"), device=DEV)
    cmax = torch.full((K + 1,), float("nan"), device=DEV)
    idx = torch.full((K + 1,), -7, dtype=torch.int64, device=DEV)
    classes[N], cmax[K], idx[K] = CANARY, CANARY, 777
    _lib.check(lib.rrt_instance_max_f32(_p(y), _p(w), _p(b), _p(classes) if want_classes else None, _p(cmax), _p(idx), N, dim, K,
                                        _p(ws), need.value, _st()), "rrt_instance_max_f32")
    torch.cuda.synchronize()
    assert bool((ws[need.value:] == 0xA5).all()), "workspace overrun"
    assert bool((classes[N] == CANARY).all()) and float(cmax[K]) == CANARY and int(idx[K]) == 777, "output overrun"
    if not want_classes:
        assert bool(torch.isnan(classes[:N]).all())
    return classes[:N], cmax[:K], idx[:K]


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("dim", [64, 512])
def test_instance_max(dim, K):
    """classes / cmax against float64; the arg-max exact with every column's maximum lifted 0.5 above the rest and moved, for
    column 0, into the first, a middle and the last 128-token block"""
    for N in NS:
        y = _gen(f"dsT/y/{N}/{dim}/{K}", (N, dim))
        w = _gen(f"dsT/w/{dim}/{K}", (K, dim)) / np.sqrt(dim)
        b = _gen(f"dsT/b/{K}", (K,)) * 0.1
        ref = y.double() @ w.double().t() + b.double()
        for j in range(K):                               # lift column j's largest row by 1.0 along w[j]: a separated maximum
            y[int(ref[:, j].argmax())] += w[j] / float((w[j].double() ** 2).sum())
        top = int((y.double() @ w.double().t() + b.double())[:, 0].argmax())
        got0 = None
        for where in sorted({0, (N // 256) * 128 + min(5, N - 1 - (N // 256) * 128), N - 1}):
            y2 = y.clone()
            y2[[top, where]] = y2[[where, top]]
            ref = y2.double() @ w.double().t() + b.double()
            s2 = torch.sort(ref, 0, descending=True)[0]
            if N > 1:
                assert float((s2[0] - s2[1]).min()) >= 0.1
            assert int(ref[:, 0].argmax()) == where
            classes, cmax, idx = _imax(y2, w, b)
            tol = 2e-5 * _rel(ref)
            _close(classes.cpu(), ref.cpu(), tol, f"classes N={N} max at {where}")
            _close(cmax.cpu(), ref.max(0)[0].cpu(), tol, f"cmax N={N}")
            assert torch.equal(idx, ref.argmax(0)), (N, where, idx.tolist(), ref.argmax(0).tolist())
            assert torch.equal(cmax, classes[idx, torch.arange(K, device=DEV)])          # the maximum IS the selected score
            got0 = (y2, cmax, idx)
        y2, cmax, idx = got0
        _c, cmax2, idx2 = _imax(y2, w, b, want_classes=False)                            # classes is optional; same bits twice
        assert torch.equal(cmax2, cmax) and torch.equal(idx2, idx)
        _c, cmax3, idx3 = _imax(y2, w, None, want_classes=False)                         # no bias
        assert torch.equal(idx3, (y2.double() @ w.double().t()).argmax(0))


def test_instance_max_ties_and_nan():
    """equal scores: the lowest index (rows in another wave, another block); NaN is never selected; a column with no
    non-NaN value selects index 0 and its maximum is NaN"""
    N, dim = 300, 64
    y = torch.zeros(N, dim, device=DEV)
    w = torch.zeros(3, dim, device=DEV)
    w[0, 0], w[1, 1], w[2, 2] = 1.0, 1.0, float("nan")
    y[[200, 40, 5, 299], 0] = 3.0                        # column 0: four equal maxima
    y[:, 1] = -1.0                                       # column 1: every row equal -> row 0 ... unless it is NaN
    y[0, 1] = float("nan")
    y[1, 1] = float("nan")
    classes, cmax, idx = _imax(y, w, None)
    assert idx.tolist() == [5, 2, 0]
    assert float(cmax[0]) == 3.0 and float(cmax[1]) == -1.0 and math.isnan(float(cmax[2]))
    assert bool(torch.isnan(classes[:2, 1]).all()) and bool(torch.isnan(classes[:, 2]).all())
    y[:, 1] = -3.0e38                                    # a huge negative score is a value, not a missing one
    y[:130, 1] = float("nan")                            # (0 * NaN: rows 0..129 are NaN in EVERY column, rows 5 and 40 too)
    _c, cmax, idx = _imax(y, w, None)
    assert idx.tolist() == [200, 130, 0] and float(cmax[0]) == 3.0 and float(cmax[1]) == float(np.float32(-3.0e38))


# ------------------------------------------------------------------ bag pool stage
def _pool_inputs(N, dim, Q, K, tag):
    feats = _gen(f"dsP/f/{tag}", (N, dim))
    qw = _gen(f"dsP/qw/{dim}/{Q}", (Q, dim)) / np.sqrt(dim)
    qb = _gen(f"dsP/qb/{Q}", (Q,)) * 0.1
    fw = _gen(f"dsP/fw/{dim}/{K}", (K, K, dim)) / np.sqrt(K * dim)
    fb = _gen(f"dsP/fb/{K}", (K,)) * 0.1
    idx = torch.from_numpy(np.floor(synth.uniform(f"dsP/idx/{tag}", (K,), 0.0, 1.0) * N).astype(np.int64)).clamp_(0, N - 1).to(DEV)
    return feats, idx, qw, qb, fw, fb


def _pool_ref64(feats, idx, qw, qb, fw, fb):
    """dsmil.py:78-94 as written, in float64 (the 1 / sqrt(Q) factor through a float32 tensor, as there)"""
    f, qw, qb = feats.double(), qw.double(), (qb.double() if qb is not None else 0.0)
    Qm = f @ qw.t() + qb
    q_max = torch.index_select(f, 0, idx) @ qw.t() + qb
    raw = torch.mm(Qm, q_max.t()) / torch.sqrt(torch.tensor(Qm.shape[1], dtype=torch.float32, device=f.device))
    A = F.softmax(raw, 0)
    B = torch.mm(A.t(), f)
    logits = F.conv1d(B.unsqueeze(0), fw.double(), fb.double() if fb is not None else None).view(-1)
    return logits, A, B, raw


def _pool(feats, idx, qw, qb, fw, fb, want=(True, True, True)):
    """rrt_dsmil_pool_f32 on NaN-filled outputs with a canary row behind them and an exact-size workspace with canary bytes"""
    lib = _lib.load()
    (N, dim), Q, K = feats.shape, qw.shape[0], fw.shape[0]
    need = C.c_size_t()
    _lib.check(lib.rrt_dsmil_pool_workspace_size(N, dim, Q, K, C.byref(need)), "ws")
    ws = torch.full((need.value + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[need.value:] = 0xA5
    logits = torch.full((K + 1,), float("nan"), device=DEV)
    A, B, raw = (torch.full(s, float("nan"), device=DEV) for s in ((N + 1, K), (K + 1, dim), (N + 1, K)))
    logits[K], A[N], B[K], raw[N] = CANARY, CANARY, CANARY, CANARY
    _lib.check(lib.rrt_dsmil_pool_f32(_p(feats), _p(idx), _p(qw), _p(qb), _p(fw), _p(fb), _p(logits), _p(A) if want[0] else None,
                                      _p(B) if want[1] else None, _p(raw) if want[2] else None, N, dim, Q, K, _p(ws),
                                      need.value, _st()), "rrt_dsmil_pool_f32")
    torch.cuda.synchronize()
    assert bool((ws[need.value:] == 0xA5).all()), "workspace overrun"
    assert float(logits[K]) == CANARY and all(bool((o[-1] == CANARY).all()) for o in (A, B, raw)), "output overrun"
    for o, wnt in zip((A, B, raw), want):
        if not wnt:
            assert bool(torch.isnan(o[:-1]).all())
    return logits[:K], A[:N], B[:K], raw[:N]


def _check_pool(got, ref, what):
    logits, A, B, raw = got
    rl, rA, rB, rraw = ref
    for g, r, name, tol in ((B, rB, "B", 2e-5), (A, rA, "A", 2e-5 * _rel(rA)), (raw, rraw, "a_raw", 2e-5 * _rel(rraw)),
                            (logits, rl, "logits", 1e-4 * _rel(rl))):
        _close(g.cpu(), r.cpu(), tol, f"{what} {name}")
    assert float(A.double().sum(0).sub(1).abs().max()) < 1e-5


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("dim,Q", [(64, 32), (64, 128), (512, 32), (512, 128)])
def test_dsmil_pool_plain(dim, Q, K):
    for N in NS:
        args = _pool_inputs(N, dim, Q, K, f"{N}/{dim}/{Q}/{K}")
        got = _pool(*args)
        _check_pool(got, _pool_ref64(*args), f"plain N={N}")
    bare = _pool(*args, want=(False, False, False))          # optional outputs absent: the same logits bits
    assert torch.equal(bare[0], got[0])
    again = _pool(*args)                                      # two identical calls: identical bits
    for a, b in zip(again, got):
        assert torch.equal(a, b)
    if K >= 2:                                                # two classes pick the same instance
        feats, idx, qw, qb, fw, fb = args
        idx = idx.clone()
        idx[1] = idx[0]
        got = _pool(feats, idx, qw, qb, fw, fb)
        _check_pool(got, _pool_ref64(feats, idx, qw, qb, fw, fb), "repeated critical id")
        assert torch.equal(got[1][:, 0], got[1][:, 1]) and torch.equal(got[2][0], got[2][1])
    _check_pool(_pool(args[0], args[1], args[2], None, args[4], None), _pool_ref64(args[0], args[1], args[2], None, args[4], None),
                "no biases")


@pytest.mark.parametrize("N", [1057, 32801])
def test_dsmil_pool_plain_past_one_merge_trip(N):
    """nb = 34: the merge block's first chunk-group trip past 32; nb = 1026: a second trip of its 1024-stride loops, the last
    chunk ragged (one token).  K = 3: classes 1 and 2 reach m, l and their rows through the class offsets of the part layout."""
    dim, Q, K = 64, 32, 3
    args = _pool_inputs(N, dim, Q, K, f"{N}/{dim}/{Q}/{K}")
    _check_pool(_pool(*args), _pool_ref64(*args), f"plain N={N}")


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("dim,Q", [(64, 32), (64, 128), (512, 32), (512, 128)])
def test_dsmil_pool_peaked(dim, Q, K):
    """q rescaled so that max |s| = 50 (inside 40..60); the critical instance of class 0 -- the row that holds column 0's
    maximum -- in the first, a middle and the last 32-token chunk in turn; then a tie of the two largest scores"""
    for N in NS:
        feats0, idx, qw, qb, fw, fb = _pool_inputs(N, dim, Q, K, f"pk/{N}/{dim}/{Q}/{K}")
        qb = qb * 0
        for where in sorted({0, (N // 64) * 32 + min(5, N - 1 - (N // 64) * 32), N - 1}):
            idx2 = idx.clone()
            idx2[0] = where
            feats = feats0.clone()
            feats[where] *= 1.5                               # the critical row is the longest: its own score is the largest
            s = _pool_ref64(feats, idx2, qw, qb, fw, fb)[3]
            qw2 = (qw * math.sqrt(50.0 / float(s.abs().max()))).contiguous()          # scores are quadratic in q_w
            ref = _pool_ref64(feats, idx2, qw2, qb, fw, fb)
            assert 40.0 <= float(ref[3].abs().max()) <= 60.0
            assert int(ref[3][:, 0].argmax()) == where
            _check_pool(_pool(feats, idx2, qw2, qb, fw, fb), ref, f"peaked N={N} max at {where}")
        if N >= 2:
            top = int(ref[3][:, 0].argmax())
            other = (top + N // 2) % N if (top + N // 2) % N != top else (top + 1) % N
            f2 = feats.clone()
            f2[other] = f2[top]
            got = _pool(f2, idx2, qw2, qb, fw, fb)
            ref = _pool_ref64(f2, idx2, qw2, qb, fw, fb)
            assert float(ref[3][other, 0]) == float(ref[3][top, 0]) == float(ref[3][:, 0].max())
            assert float(got[3][other, 0]) == float(got[3][top, 0])
            _check_pool(got, ref, f"tie N={N}")


@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("N", [1, 33, 1000])
def test_one_pass_pool_against_branch_pool_composition(N, K):
    """the composition the layer path runs -- q_max and the folded score rows in torch ops, rrt_branch_pool_f32 with
    y = hid_a = feats, torch's conv1d -- on the same inputs, within the stage bounds"""
    lib = _lib.load()
    dim, Q = 512, 128
    feats, idx, qw, qb, fw, fb = _pool_inputs(N, dim, Q, K, f"cmp/{N}/{K}")
    got = _pool(feats, idx, qw, qb, fw, fb)
    q_max = F.linear(feats.index_select(0, idx), qw, qb)
    c_w = (torch.mm(q_max, qw) / math.sqrt(Q)).contiguous()
    c_b = (torch.mv(q_max, qb) / math.sqrt(Q)).contiguous()
    need = C.c_size_t()
    _lib.check(lib.rrt_branch_pool_workspace_size(N, dim, dim, K, C.byref(need)), "ws")
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    B, A, raw = (torch.empty(s, device=DEV) for s in ((K, dim), (K, N), (K, N)))
    _lib.check(lib.rrt_branch_pool_f32(_p(feats), _p(feats), None, _p(c_w), _p(c_b), _p(B), _p(A), _p(raw), N, dim, dim, K, _p(ws),
                                       need.value, _st()), "rrt_branch_pool_f32")
    logits = F.conv1d(B.unsqueeze(0), fw, fb).view(-1)
    torch.cuda.synchronize()
    _check_pool(got, (logits.double(), A.t().double(), B.double(), raw.t().double()), f"vs composition N={N}")


# ------------------------------------------------------------------ the module against the reference goldens
def _model(g, train=False):
    cfg = g["cfg"]
    shapes = {k: tuple(s) for k, s in cfg["ref_keys"] if not k.startswith("rrt.")}
    st = synth.dsmil_head_state(shapes, cfg["name"])
    if cfg["rrt"]:
        st.update({"rrt." + k: v for k, v in synth.encoder_state(**{k: v for k, v in cfg["enc"].items() if k != "region_num"}).items()})
    m = MILNet(cfg["n_classes"], 0., cfg["act"], input_dim=cfg["input_dim"],
               rrt=RRTEncoder(drop_out=0., **cfg["enc"]) if cfg["rrt"] else None)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()}, strict=True)
    m = m.to(DEV)
    x = torch.from_numpy(synth.bag(int(g["n"]), cfg["input_dim"], tag=cfg["tag"], nonneg=True)).to(DEV).unsqueeze(0)
    if cfg["bce"]:
        crit, lab = nn.BCEWithLogitsLoss(), torch.tensor(g["label"], device=DEV)
        target = lab.view(1, -1).float()
    else:
        crit, lab = nn.CrossEntropyLoss(), torch.tensor([int(g["label"])], device=DEV)
        target = lab
    return (m.train() if train else m.eval()), x, lab, crit, target


@pytest.mark.parametrize("name", CASES)
def test_dsmil_forward_matches_reference(name):
    g = load_golden(name)
    cfg = g["cfg"]
    m, x, lab, crit, _target = _model(g)
    N, nc = int(g["n"]), cfg["n_classes"]
    with torch.no_grad():
        out = m.forward_bag(x[0], return_attn=True, return_features=True, return_critical=True)
        bare = m.forward_bag(x[0])
        pred_e, cmax_e = m(x)
        m.train()
        pred_t, max_loss, ps = m(x, label=lab, loss=crit)
        streams = m._streams(m._embed(x[0]))
        m.eval()
    torch.cuda.synchronize()
    assert out["logits"].shape == (1, nc) and out["classes_max"].shape == (nc,) and out["attn"].shape == (N, nc)
    assert out["features"].shape == (nc, 512) and out["critical"].dtype == torch.int64 and ps == cfg["ps"] == N
    _close(out["logits"].cpu(), g["logits"], 1e-4, name + " logits")
    _close(out["classes_max"].cpu(), g["classes_max"], 1e-4, name + " classes max")
    _close(out["features"].cpu(), g["features"], 1e-4, name + " B")
    _close(out["attn"].cpu(), g["attn"], 1e-6, name + " A")
    assert out["critical"].cpu().tolist() == g["critical"].tolist()
    # the same kernels: the same bits
    assert torch.equal(bare["logits"], out["logits"]) and torch.equal(bare["classes_max"], out["classes_max"])
    assert torch.equal(pred_e, out["logits"]) and torch.equal(cmax_e, out["classes_max"])
    # the layer path (encoder Function, _InstanceMax, _BranchPool, torch's conv1d): within the bounds
    _close(pred_t.cpu(), g["logits"], 1e-4, name + " logits (train path)")
    _close(float(max_loss), float(g["max_loss"]), 1e-4, name + " max_loss")
    _close(streams[1].cpu(), g["classes_max"], 1e-4, name + " classes max (train path)")
    assert streams[2].cpu().tolist() == g["critical"].tolist()
    _close(streams[3].cpu(), g["attn"], 1e-6, name + " A (train path)")
    _close(streams[4].cpu(), g["features"], 1e-4, name + " B (train path)")


@pytest.mark.parametrize("name", CASES)
def test_dsmil_gradients_match_reference(name):
    """loss = criterion(bag logits) + max_loss, CE and BCE.  pe.bias: an identically-zero reference (module docstring), held
    to exactly zero.  With rrt: the bag loss alone leaves every encoder parameter without a gradient."""
    g = load_golden(name)
    cfg = g["cfg"]
    m, x, lab, crit, target = _model(g, train=True)
    x = x.clone().requires_grad_(True)
    pred, max_loss, _ps = m(x, label=lab, loss=crit)
    loss = crit(pred, target) + max_loss
    loss.backward()
    torch.cuda.synchronize()
    _close(float(loss), float(g["loss"]), 1e-3 * abs(float(g["loss"])), name + " loss")
    none = set(bytes(g["none"]).decode().split("\n")) - {""}
    seen = 0
    for pname, grad in [("x", x.grad[0])] + [(n, p.grad) for n, p in m.named_parameters()]:
        if pname in none:
            assert grad is None or float(grad.abs().max()) == 0.0, pname
            continue
        key = "g__" + pname.replace(".", "__")
        assert grad is not None, pname
        got = grad.detach().double().cpu().numpy()
        scale = float(g[key + "__max"])
        if pname.endswith("pe.bias"):
            assert scale < 1e-12 and float(np.abs(got).max()) == 0.0, pname
            seen += 1
            continue
        if key + "__full" in g:
            got, ref = got.reshape(g[key + "__full"].shape), g[key + "__full"]
        else:
            got, ref = got.reshape(got.shape[0], -1)[g[key + "__rows"]], g[key + "__vals"]
        err = float(np.abs(got - ref).max())
        print(f"{name} {pname}: err {err:.3e} scale {scale:.3e}")
        assert np.isfinite(got).all() and err <= 1e-3 * scale, (pname, err, scale)
        seen += 1
    assert seen >= (20 if cfg["rrt"] else 9)
    if cfg["rrt"]:
        m.zero_grad(set_to_none=True)
        pred, _ml, _ps = m(x.detach(), label=lab, loss=crit)
        crit(pred, target).backward()
        torch.cuda.synchronize()
        enc = [(n, p.grad) for n, p in m.named_parameters() if n.startswith("rrt.")]
        assert len(enc) >= 12
        for n, gr in enc:
            assert gr is None or float(gr.abs().max()) == 0.0, n
        assert m.b_classifier.q.weight.grad is not None and m.patch_to_emb[0].weight.grad is not None
        assert m.i_classifier.weight.grad is None or float(m.i_classifier.weight.grad.abs().max()) == 0.0


@pytest.mark.parametrize("dt", [None, torch.bfloat16])
def test_forward_bags_bit_for_bit(dt):
    torch.manual_seed(5)
    m = MILNet(3, 0., "relu", input_dim=256, rrt=RRTEncoder()).to(DEV).eval()
    if dt is not None:
        m.rrt.compute_dtype = dt
    sizes = [3000, 700, 1, 2200]
    bags = [torch.from_numpy(synth.bag(n, 256, tag=f"dsmilbags/{i}", nonneg=True)).to(DEV) for i, n in enumerate(sizes)]
    kw = dict(return_attn=True, return_features=True, return_critical=True)
    with torch.no_grad():
        outs = m.forward_bags(bags, streams=4, **kw)
        ref = [m.forward_bag(b, solo=False, **kw) for b in bags]
        again = m.forward_bags([b.unsqueeze(0) for b in bags], streams=4, **kw)
    torch.cuda.synchronize()
    for o, r, o2 in zip(outs, ref, again):
        for k in ("logits", "classes_max", "attn", "features", "critical"):
            assert torch.equal(o[k], r[k]) and torch.equal(o2[k], r[k]), k
    one = ref[2]                                              # the bag of one instance: A = 1, B = feats[0]
    assert float(one["attn"].min()) == 1.0 and int(one["critical"].max()) == 0 and bool(torch.isfinite(one["logits"]).all())
    assert m.forward_bags([]) == []


def test_dsmil_autocast_bf16():
    g = load_golden("dsmil_n2_wide")
    m, x, _lab, _crit, _target = _model(g)
    with torch.no_grad():
        f32 = m.forward_bag(x[0], return_critical=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lo = m.forward_bag(x[0], return_critical=True)
            lo2 = m.forward_bag(x[0], return_critical=True)
            pred, _cmax = m(x)
    torch.cuda.synchronize()
    assert lo["critical"].cpu().tolist() == g["critical"].tolist() == f32["critical"].cpu().tolist()
    err = float(np.abs(lo["logits"].float().cpu().numpy() - g["logits"]).max())
    dist = float((lo["logits"].float() - f32["logits"]).abs().max())
    print(f"bf16 logits err {err:.3e}; distance to the fp32 run {dist:.3e}")
    assert lo["logits"].dtype == torch.float32 and err <= 2e-2
    assert dist > 1e-5                                        # visibly not the fp32 result: the mode is on
    assert torch.equal(lo["logits"], lo2["logits"]) and torch.equal(lo["classes_max"], lo2["classes_max"])
    assert torch.equal(pred, lo["logits"])


def test_dsmil_fails_loudly_and_works_without_rrt():
    m = MILNet(2, 0., "relu", input_dim=64).to(DEV).eval()
    with pytest.raises(ValueError):
        m.forward_bag(torch.zeros(10, 96, device=DEV))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 10, 96, device=DEV))
    lab = torch.tensor([1], device=DEV)
    dm = MILNet(2, 0.25, "gelu", input_dim=64).to(DEV).train()
    out = dm(torch.randn(1, 40, 64, device=DEV), label=lab, loss=nn.CrossEntropyLoss())
    assert out[0].grad_fn is not None and out[0].shape == (1, 2) and out[1].grad_fn is not None and out[2] == 40
    with pytest.raises(NotImplementedError):
        dm.forward_bag(torch.zeros(10, 64, device=DEV))
    with pytest.raises(NotImplementedError):
        dm.forward_bags([torch.zeros(10, 64, device=DEV)])
    with pytest.raises(TypeError):
        MILNet(2, 0., "relu", input_dim=64).to(DEV).train()(torch.randn(1, 40, 64, device=DEV), label=lab)
    # rrt=None: the reference allows it; the eval outputs against its op sequence in float64 on the same embedding
    x = torch.randn(1, 40, 64, device=DEV)
    pred, cmax = m(x)                                         # eval() with a graph: the layer path
    assert pred.shape == (1, 2) and cmax.shape == (2,) and pred.grad_fn is not None
    pred, cmax = pred.detach(), cmax.detach()
    with torch.no_grad():
        feats = m._embed(x[0]).double()
        m64 = MILNet(2, 0., "relu", input_dim=64).to(DEV).double()
        m64.load_state_dict(m.state_dict())
        classes = m64.i_classifier(feats)
        e_pred, _A, _B = m64.b_classifier._eager(feats, classes)
    _close(pred.cpu(), e_pred.cpu(), 1e-4, "rrt=None logits")
    _close(cmax.cpu(), classes.max(0)[0].cpu(), 1e-4, "rrt=None classes max")
    with torch.no_grad():
        pred1, cmax1 = m(x)                                   # ... and without one: the one-call path
    _close(pred1.cpu(), e_pred.cpu(), 1e-4, "rrt=None logits (one call)")
    _close(cmax1.cpu(), classes.max(0)[0].cpu(), 1e-4, "rrt=None classes max (one call)")
    one = m.forward_bag(torch.randn(1, 64, device=DEV), return_attn=True, return_features=True)     # N = 1
    assert float(one["attn"].min()) == 1.0 and bool(torch.isfinite(one["logits"]).all())
