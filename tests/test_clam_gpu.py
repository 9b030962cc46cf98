"""GPU: the CLAM heads.  Stage kernels (csrc/clam_pool.hip: branch pool forward / backward, top-k of rows) against float64
torch restatements, CLAM_SB / CLAM_MB against the reference's goldens (tools/make_golden_clam.py), and the one-call /
multi-bag entry points against the layer path.

Bounds (none of them taken from this code's own output):
  * stage forward: what tests/test_hip_parity.py::test_attn_pool_forward_backward holds rrt_attn_pool_f32 to -- pooled 2e-5,
    attention and raw scores 2e-5 * max(1, largest reference entry);
  * every gradient: 1e-3 of that tensor's own largest reference entry.  Some tensors have NO largest entry to be relative to,
    because the reference is zero identically (float64 leaves 0 or ~1e-18): without a gradient into the raw scores
    d c_b[c] = sum_n ds[c, n] (the softmax adjoint sums to zero), and at N = 1 every ds (A = 1, dA - A dA = 0).  fp32 cannot
    cancel exactly; such a tensor (ONE rule in both tests, `_grad_tol`: its largest reference entry is below 1e-9 of the
    largest term whose cancellation makes the zero) is held to 1e-5 of that term (fp32 rounds each term to 6e-8 of it).
    The term is A[c, n] dA[c, n] in the stage test; the golden test, which has no dA, takes their per-class sum over the
    bag, sum_n A dA = M . dM = dlogit_j (logit_j - cls_b[j]), from the reference logits;
  * module against the goldens: logits, A_raw, features 1e-4 and attention 1e-6 (test_rrtmil_variants_match_reference on
    G11), bf16 autocast 2e-2 (test_rrtmil_autocast_bf16).  Top-k ids: the k ids of every evaluated end exact (the goldens
    guarantee a gap of 100x those bounds between the k-th and the (k+1)-th value) and in the reference's order; only two
    neighbours whose reference attention values differ by less than 2e-6 (both may be off by the 1e-6 bound; the goldens
    guarantee nothing inside the top k) may come in either order.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_names, load_golden
from rrt_mil_amd import CLAM_MB, CLAM_SB, RRTEncoder, _lib, synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda:0"
CASES = [n for n in golden_names("clam_") if n != "clam_keys"]
CANARY = 777.0


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(tag, shape):
    return torch.from_numpy(synth.normal(tag, shape)).to(DEV)


def _inputs(N, dim, hid, K, gated, tag):
    y = _gen(f"clamT/y/{tag}", (N, dim))
    ha = torch.tanh(_gen(f"clamT/ha/{tag}", (N, hid)))
    hb = torch.sigmoid(_gen(f"clamT/hb/{tag}", (N, hid))) if gated else None
    cw = _gen(f"clamT/cw/{tag}", (K, hid)) / np.sqrt(hid)
    cb = _gen(f"clamT/cb/{tag}", (K,)) * 0.1
    return y, ha, hb, cw, cb


def _ref64(y, ha, hb, cw, cb):
    h = ha.double() * hb.double() if hb is not None else ha.double()
    s = cw.double() @ h.t() + cb.double()[:, None]
    A = torch.softmax(s, dim=1)
    return A @ y.double(), A, s


def _branch_pool(y, ha, hb, cw, cb, want_attn=True):
    """rrt_branch_pool_f32 on NaN-filled outputs with a canary row behind them and an exact-size workspace with canary bytes"""
    lib = _lib.load()
    (N, dim), hid, K = y.shape, ha.shape[1], cw.shape[0]
    need = C.c_size_t()
    _lib.check(lib.rrt_branch_pool_workspace_size(N, dim, hid, K, C.byref(need)), "ws")
    ws = torch.full((need.value + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[need.value:] = 0xA5
    outs = [torch.full((K + 1, w), float("nan"), device=DEV) for w in (dim, N, N)]
    for o in outs:
        o[K] = CANARY
    pooled, attn, raw = outs
    _lib.check(lib.rrt_branch_pool_f32(_p(y), _p(ha), _p(hb), _p(cw), _p(cb), _p(pooled), _p(attn) if want_attn else None, _p(raw),
                                       N, dim, hid, K, _p(ws), need.value, _st()), "rrt_branch_pool_f32")
    torch.cuda.synchronize()
    assert bool((ws[need.value:] == 0xA5).all()), "workspace overrun"
    for o in outs:
        assert bool((o[K] == CANARY).all()), "output overrun"
    if not want_attn:
        assert bool(torch.isnan(attn[:K]).all())
    return pooled[:K], attn[:K], raw[:K]


def _grad_tol(scale, natural):
    """the gradient criterion: 1e-3 of the tensor's largest reference entry `scale`; an identically-zero reference (see the
    module docstring) is held to 1e-5 of `natural`, the largest of the terms that cancel"""
    return 1e-3 * scale if scale > 1e-9 * natural else 1e-5 * natural


def _check_fwd(got, ref, what):
    for g, r, name, rel in zip(got, ref, ("pooled", "attn", "a_raw"), (False, True, True)):
        tol = 2e-5 * (max(1.0, float(r.abs().max())) if rel else 1.0)
        err = float((g.double() - r).abs().max())
        print(f"{what} {name}: err {err:.3e} tol {tol:.1e}")
        assert bool(torch.isfinite(g).all()) and err <= tol, (what, name, err, tol)


NS = (1, 8, 31, 32, 33, 100, 1000)


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("dim,hid", [(64, 12), (64, 256), (512, 12), (512, 256)])
def test_branch_pool_forward_plain(dim, hid, K, gated):
    lib = _lib.load()
    for N in NS:
        y, ha, hb, cw, cb = _inputs(N, dim, hid, K, gated, f"{N}/{dim}/{hid}/{K}")
        got = _branch_pool(y, ha, hb, cw, cb)
        _check_fwd(got, _ref64(y, ha, hb, cw, cb), f"plain N={N}")
        assert abs(float(got[1].double().sum(1).sub(1).abs().max())) < 1e-5
        if K == 1:          # one branch: rrt_attn_pool_f32 on the same inputs, within the same bound
            need = C.c_size_t()
            _lib.check(lib.rrt_attn_pool_workspace_size(N, dim, hid, C.byref(need)), "ws")
            ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
            po, at, ra = (torch.empty(w, device=DEV) for w in (dim, N, N))
            _lib.check(lib.rrt_attn_pool_f32(_p(y), _p(ha), _p(hb), _p(cw), _p(cb), _p(po), _p(at), _p(ra), N, dim, hid, _p(ws),
                                             need.value, _st()), "rrt_attn_pool_f32")
            torch.cuda.synchronize()
            _check_fwd(got, (po.double()[None], at.double()[None], ra.double()[None]), f"vs attn_pool N={N}")
    got2 = _branch_pool(y, ha, hb, cw, cb, want_attn=False)
    assert torch.equal(got2[0], got[0]) and torch.equal(got2[2], got[2])          # attn is optional; same bits twice


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("N", [1057, 32801])
def test_branch_pool_forward_plain_past_one_merge_trip(N, gated):
    """nb = 34: the merge block's first chunk-group trip past 32; nb = 1026: a second trip of its 1024-stride loops, the last
    chunk ragged (one token).  K = 3: branches 1 and 2 reach m, l and their rows through the branch offsets of the part layout."""
    dim, hid, K = 64, 12, 3
    y, ha, hb, cw, cb = _inputs(N, dim, hid, K, gated, f"{N}/{dim}/{hid}/{K}")
    got = _branch_pool(y, ha, hb, cw, cb)
    _check_fwd(got, _ref64(y, ha, hb, cw, cb), f"plain N={N}")
    assert abs(float(got[1].double().sum(1).sub(1).abs().max())) < 1e-5


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("dim,hid", [(64, 12), (64, 256), (512, 12), (512, 256)])
def test_branch_pool_forward_peaked(dim, hid, K, gated):
    """scores scaled to max |s| = 50 (inside 40..60); the row maximum of branch 0 moved into the first, a middle and the last
    32-token chunk in turn; then a tie of the two largest scores"""
    for N in NS:
        y, ha, hb, cw, cb = _inputs(N, dim, hid, K, gated, f"pk/{N}/{dim}/{hid}/{K}")
        cb = cb * 0
        s = _ref64(y, ha, hb, cw, cb)[2]
        cw = (cw * (50.0 / float(s.abs().max()))).contiguous()
        s = _ref64(y, ha, hb, cw, cb)[2]
        assert 40.0 <= float(s.abs().max()) <= 60.0
        top = int(s[0].argmax())
        for where in sorted({0, (N // 64) * 32 + min(5, N - 1 - (N // 64) * 32), N - 1}):
            a2, b2 = ha.clone(), (hb.clone() if gated else None)
            for t in (a2, b2):
                if t is not None:
                    t[[top, where]] = t[[where, top]]
            got = _branch_pool(y, a2, b2, cw, cb)
            ref = _ref64(y, a2, b2, cw, cb)
            assert int(ref[2][0].argmax()) == where
            _check_fwd(got, ref, f"peaked N={N} max at {where}")
        if N >= 2:
            other = (top + N // 2) % N if (top + N // 2) % N != top else (top + 1) % N
            a2, b2 = ha.clone(), (hb.clone() if gated else None)
            for t in (a2, b2):
                if t is not None:
                    t[other] = t[top]
            got = _branch_pool(y, a2, b2, cw, cb)
            ref = _ref64(y, a2, b2, cw, cb)
            assert float(ref[2][0, other]) == float(ref[2][0, top]) == float(ref[2][0].max())
            assert float(got[2][0, other]) == float(got[2][0, top])
            _check_fwd(got, ref, f"tie N={N}")


@pytest.mark.parametrize("with_raw", [False, True])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 33, 1000])
def test_branch_pool_backward(N, K, gated, with_raw):
    lib = _lib.load()
    for dim, hid in ((64, 12), (512, 256)):
        y, ha, hb, cw, cb = _inputs(N, dim, hid, K, gated, f"bw/{N}/{dim}/{hid}/{K}")
        cw = cw * 3
        r1, r2 = _gen(f"clamT/r1/{K}/{dim}", (K, dim)), (_gen(f"clamT/r2/{K}/{N}", (K, N)) if with_raw else None)
        leaves = [t.double().requires_grad_(True) if t is not None else None for t in (y, ha, hb, cw, cb)]
        pooled64, A64, s64 = _ref64(*leaves)
        loss = (pooled64 * r1.double()).sum() + ((s64 * r2.double()).sum() if with_raw else 0.0)
        loss.backward()
        dA = leaves[0].detach() @ r1.double().t()
        natural = float((A64.detach() * dA.t()).abs().max())

        def tol(scale):
            return _grad_tol(scale, natural)
        pooled, attn, _raw = _branch_pool(y, ha, hb, cw, cb)
        pooled, attn = pooled.contiguous(), attn.contiguous()
        need = C.c_size_t()
        _lib.check(lib.rrt_branch_pool_workspace_size(N, dim, hid, K, C.byref(need)), "ws")
        ws = torch.full((need.value + 256,), 0xFF, dtype=torch.uint8, device=DEV)
        ws[need.value:] = 0xA5
        dy, dha = torch.full((N + 1, dim), float("nan"), device=DEV), torch.full((N + 1, hid), float("nan"), device=DEV)
        dhb = torch.full((N + 1, hid), float("nan"), device=DEV) if gated else None
        dwcb = torch.full((K * hid + 8 + 4,), float("nan"), device=DEV)
        for t in (dy, dha, dhb):
            if t is not None:
                t[N] = CANARY
        dwcb[K * hid + 8:] = CANARY
        _lib.check(lib.rrt_branch_pool_backward_f32(_p(y), _p(ha), _p(hb), _p(cw), _p(attn), _p(pooled), _p(r1), _p(r2), _p(dy),
                                                    _p(dha), _p(dhb), _p(dwcb), N, dim, hid, K, _p(ws), need.value, _st()),
                   "rrt_branch_pool_backward_f32")
        torch.cuda.synchronize()
        assert bool((ws[need.value:] == 0xA5).all()) and bool((dwcb[K * hid + 8:] == CANARY).all())
        got = {"dy": dy, "dhid_a": dha, "dhid_b": dhb}
        for (name, g), leaf in zip(got.items(), leaves[:3]):
            if g is None:
                continue
            assert bool((g[N] == CANARY).all()), name
            ref = leaf.grad
            err, scale = float((g[:N].double() - ref).abs().max()), float(ref.abs().max())
            print(f"{name} N={N} dim={dim}: err {err:.3e} scale {scale:.3e}")
            assert err <= tol(scale), (name, err, scale)
        dcw, dcb = dwcb[:K * hid].reshape(K, hid).double(), dwcb[K * hid:K * hid + K].double()
        err, scale = float((dcw - leaves[3].grad).abs().max()), float(leaves[3].grad.abs().max())
        assert err <= tol(scale), ("d c_w", err, scale)
        scale_b = float(leaves[4].grad.abs().max())
        err = float((dcb - leaves[4].grad).abs().max())
        print(f"d c_b N={N}: err {err:.3e} scale {scale_b:.3e} natural {natural:.3e}")
        assert err <= tol(scale_b), ("d c_b", err, scale_b)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("N", [8, 33, 1000, 70001])
def test_topk_rows(N, k, K):
    from rrt_mil_amd.clam import topk_rows
    if N < k:
        with pytest.raises(_lib.RRTHipError):
            topk_rows(torch.zeros(K, N, device=DEV), k)
        return
    g = torch.Generator().manual_seed(N * 100 + k)
    x = torch.stack([torch.randperm(N, generator=g).float() * 0.37 - 11.0 for _ in range(K)]).to(DEV)    # distinct values
    ids = topk_rows(x, k)
    torch.cuda.synchronize()
    assert ids.shape == (K, 2, k) and ids.dtype == torch.int64
    assert torch.equal(ids[:, 0], torch.topk(x, k, dim=1)[1]) and torch.equal(ids[:, 1], torch.topk(-x, k, dim=1)[1])


def test_topk_ties_take_the_lower_index():
    from rrt_mil_amd.clam import topk_rows
    x = torch.zeros(2, 1000, device=DEV)
    x[0, [900, 17, 555, 300]] = 5.0          # four equal maxima, everything else equal too
    x[1] = torch.arange(1000, device=DEV) % 7
    ids = topk_rows(x, 6).cpu()
    assert ids[0, 0].tolist() == [17, 300, 555, 900, 0, 1] and ids[0, 1].tolist() == [0, 1, 2, 3, 4, 5]
    assert ids[1, 0].tolist() == [6, 13, 20, 27, 34, 41] and ids[1, 1].tolist() == [0, 7, 14, 21, 28, 35]


# ------------------------------------------------------------------ modules against the reference goldens
def _model(g, train=False):
    cfg = g["cfg"]
    pre = cfg["rrt_prefix"]
    shapes = {k: tuple(s) for k, s in cfg["ref_keys"] if not k.startswith(pre)}
    st = synth.clam_head_state(shapes, cfg["name"])
    st.update({pre + k: v for k, v in synth.encoder_state(**{k: v for k, v in cfg["enc"].items() if k != "region_num"}).items()})
    cls = CLAM_SB if cfg["kind"] == "sb" else CLAM_MB
    m = cls(cfg["input_dim"], gate=cfg["gate"], size_arg=cfg["size_arg"], k_sample=cfg["k_sample"], n_classes=cfg["n_classes"],
            subtyping=cfg["subtyping"], rrt=RRTEncoder(drop_out=0., **cfg["enc"]))
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()}, strict=True)
    m = m.to(DEV)
    x = torch.from_numpy(synth.bag(int(g["n"]), cfg["input_dim"], tag=cfg["tag"], nonneg=True)).to(DEV).unsqueeze(0)
    return (m.train() if train else m.eval()), x, torch.tensor([int(g["label"])], device=DEV)


def _close(got, ref, tol, what):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max())
    print(f"{what}: err {err:.3e} tol {tol:.1e}")
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and err <= tol, (what, err, tol)


@pytest.mark.parametrize("name", CASES)
def test_clam_forward_matches_reference(name):
    g = load_golden(name)
    cfg = g["cfg"]
    m, x, lab = _model(g)
    N, K, nc = int(g["n"]), g["a_raw"].shape[0], cfg["n_classes"]
    with torch.no_grad():
        out = m.forward_bag(x[0], return_features=True, return_attn=True, return_topk=True)
        raw = m(x, attention_only=True)
        logits_only = m(x)                                  # label=None: the instance branch is skipped
        logits_ne = m(x, label=lab, instance_eval=False, return_features=True)
        logits_i, inst_loss, ps = m(x, label=lab)
    torch.cuda.synchronize()
    assert out["logits"].shape == (1, nc) and raw.shape == (K, N) and out["features"].shape == (K, 512)
    assert logits_only.shape == (1, nc) and logits_ne.shape == (1, nc) and logits_i.shape == (1, nc) and ps == cfg["ps"] == N
    assert m.last_features.shape == (K, 512)
    _close(out["logits"].cpu(), g["logits"], 1e-4, name + " logits")
    _close(logits_i.cpu(), g["logits"], 1e-4, name + " logits (instance path)")
    _close(raw.cpu(), g["a_raw"], 1e-4, name + " A_raw")
    _close(out["features"].cpu(), g["features"], 1e-4, name + " features")
    _close(out["attn"].cpu(), torch.softmax(torch.from_numpy(g["a_raw"]), 1), 1e-6, name + " attention")
    ids = out["topk"].cpu().numpy()
    A64 = torch.softmax(torch.from_numpy(g["a_raw"]).double(), 1).numpy()
    for row, both, _i in cfg["branches"]:
        for end, sign in ((0, 1.0), (1, -1.0))[:2 if both else 1]:
            got, ref = ids[row, end].tolist(), g["topk"][row, end].tolist()
            assert sorted(got) == sorted(ref), (name, row, end, got, ref)
            v = sign * A64[row, got]
            assert bool((v[:-1] >= v[1:] - 2e-6).all()), (name, row, end, "order", got, ref)
    ref = float(g["inst_loss"])
    _close(float(inst_loss), ref, 1e-3 * abs(ref), name + " instance loss")
    assert torch.equal(logits_only, out["logits"]) and torch.equal(logits_ne, out["logits"])


@pytest.mark.parametrize("name", CASES)
def test_clam_gradients_match_reference(name):
    g = load_golden(name)
    m, x, lab = _model(g, train=True)
    x = x.clone().requires_grad_(True)
    logits, inst_loss, _ps = m(x, label=lab)
    loss = F.cross_entropy(logits, lab) + inst_loss
    loss.backward()
    torch.cuda.synchronize()
    _close(float(loss), float(g["loss"]), 1e-3 * abs(float(g["loss"])), name + " loss")
    none = set(bytes(g["none"]).decode().split("\n")) - {""}
    # the terms whose cancellation makes d c_b zero: per class j, sum_n A dA = dlogit_j * (logit_j - cls_b[j])
    lg = torch.from_numpy(g["logits"]).double().reshape(-1)
    dlg = torch.softmax(lg, 0) - F.one_hot(lab.cpu()[0], lg.numel())
    natural = float((dlg * (lg - m._cls_packed()[1].detach().double().cpu().reshape(-1))).abs().max())
    seen = 0
    for pname, grad in [("x", x.grad[0])] + [(n, p.grad) for n, p in m.named_parameters()]:
        if pname in none:
            assert grad is None or float(grad.abs().max()) == 0.0, pname
            continue
        key = "g__" + pname.replace(".", "__")
        assert grad is not None, pname
        got = grad.detach().double().cpu().numpy()
        scale = float(g[key + "__max"])
        if key + "__full" in g:
            got, ref = got.reshape(g[key + "__full"].shape), g[key + "__full"]
        else:
            got, ref = got.reshape(got.shape[0], -1)[g[key + "__rows"]], g[key + "__vals"]
        err = float(np.abs(got - ref).max())
        tol = _grad_tol(scale, natural)          # (the score bias: an identically-zero reference, see the module docstring)
        print(f"{name} {pname}: err {err:.3e} scale {scale:.3e}")
        assert np.isfinite(got).all() and err <= tol, (pname, err, scale)
        seen += 1
    assert seen >= 20


@pytest.mark.parametrize("cls,nc", [(CLAM_SB, 2), (CLAM_MB, 8)])
def test_ungated_big_head_against_eager(cls, nc):
    """gate=False, size_arg='big' (hidden 384): the one-call forward and the HIP layer path with its backward (CLAM_MB with 8
    classes: the backward block's LDS, 8 * (512 + 4 * 384) + 32 floats, is past 64 KiB) against the reference's op sequence
    for the head in float64 torch ops on the same encoder output.  Forward bounds as for the goldens; gradients: `_grad_tol`
    with the per-class sums of the cancelling terms, dlogit_j (logit_j - cls_b[j])."""
    import copy
    torch.manual_seed(11)
    m = cls(128, gate=False, size_arg="big", n_classes=nc, rrt=RRTEncoder()).to(DEV).eval()
    with torch.no_grad():
        for p_ in m.attention_net[-1].parameters():          # scores of O(1) instead of xavier's O(0.1)
            p_.mul_(3.0)
    N, K = 333, (nc if cls is CLAM_MB else 1)
    x = torch.from_numpy(synth.bag(N, 128, tag="clam/ungated_big", nonneg=True)).to(DEV).unsqueeze(0)
    w = torch.from_numpy(synth.normal("clam/ungated_big/w", (1, nc))).to(DEV)
    with torch.no_grad():
        out = m.forward_bag(x[0], return_features=True, return_attn=True)
        raw = m(x, attention_only=True)
        y = m._embed_encode(x[0])
    # the float64 head: copies of the attention net and the bag classifiers
    net64, cls64 = copy.deepcopy(m.attention_net[-1]).double(), copy.deepcopy(m.classifiers).double()
    y64 = y.double().requires_grad_(True)
    e_raw = net64(y64)[0].transpose(1, 0)
    e_A = torch.softmax(e_raw, dim=1)
    e_M = torch.mm(e_A, y64)
    e_logits = cls64(e_M) if cls is CLAM_SB else torch.cat([cls64[c](e_M[c]) for c in range(nc)]).unsqueeze(0)
    (e_logits.reshape(1, nc) * w.double()).sum().backward()
    assert raw.shape == (K, N) and out["features"].shape == (K, 512) and out["logits"].shape == (1, nc)
    _close(out["logits"].cpu(), e_logits.detach().cpu().reshape(1, nc), 1e-4, "ungated big logits")
    _close(raw.cpu(), e_raw.detach().cpu(), 1e-4, "ungated big A_raw")
    _close(out["features"].cpu(), e_M.detach().cpu(), 1e-4, "ungated big features")
    _close(out["attn"].cpu(), e_A.detach().cpu(), 1e-6, "ungated big attention")
    # the HIP layer path on the same (detached) encoder output, so that only the head's adjoint is compared
    t = y.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    (m._bag_logits(m._attend(t)[0]).reshape(1, nc) * w).sum().backward()
    torch.cuda.synchronize()
    idx = len(m.attention_net) - 1
    ref = {"y": y64.grad} | {f"attention_net.{idx}.{n}": p_.grad for n, p_ in net64.named_parameters()}
    ref |= {f"classifiers.{n}": p_.grad for n, p_ in cls64.named_parameters()}
    got = {"y": t.grad} | {n: p_.grad for n, p_ in m.named_parameters() if p_.grad is not None}
    assert got.keys() == ref.keys() and len(ref) == 5 + 2 * (nc if cls is CLAM_MB else 1)
    cb = m._cls_packed()[1].detach().double().reshape(-1)
    natural = float((w.double().reshape(-1) * (e_logits.detach().reshape(-1) - cb)).abs().max())
    for n, r in ref.items():
        err, scale = float((got[n].double() - r).abs().max()), float(r.abs().max())
        print(f"ungated big {n}: err {err:.3e} scale {scale:.3e} natural {natural:.3e}")
        assert err <= _grad_tol(scale, natural), (n, err, scale)


def test_topk_rows_nan_slots():
    """NaN is never selected; a row with fewer than k other values has -1 in its unused slots"""
    from rrt_mil_amd.clam import topk_rows
    x = torch.full((2, 300), float("nan"), device=DEV)
    x[0, [7, 250, 100]] = torch.tensor([1.0, 3.0, 2.0], device=DEV)
    x[1] = torch.arange(300, device=DEV).float()
    x[1, 299] = float("nan")
    ids = topk_rows(x, 4).cpu()
    assert ids[0, 0].tolist() == [250, 100, 7, -1] and ids[0, 1].tolist() == [7, 100, 250, -1]
    assert ids[1, 0].tolist() == [298, 297, 296, 295] and ids[1, 1].tolist() == [0, 1, 2, 3]


def test_forward_bag_equals_eager_head_and_is_deterministic():
    for name in ("clam_sb_n2", "clam_mb_n3_sub"):
        g = load_golden(name)
        m, x, _lab = _model(g)
        with torch.no_grad():
            a = m.forward_bag(x[0], return_features=True, return_attn=True)
            b = m.forward_bag(x[0], return_features=True, return_attn=True)
            eager, _M, _A, eager_raw = m._eager_head(m._embed_encode(x[0]))
            raw = m(x, attention_only=True)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), k                                   # two identical calls: the same bits
        _close(a["logits"].cpu(), eager.double().cpu(), 1e-4, name + " one call vs eager head: logits")
        _close(raw.cpu(), eager_raw.double().cpu(), 1e-4, name + " one call vs eager head: A_raw")


@pytest.mark.parametrize("dt", [None, torch.bfloat16])
def test_forward_bags_bit_for_bit(dt):
    torch.manual_seed(5)
    m = CLAM_MB(256, n_classes=3, rrt=RRTEncoder()).to(DEV).eval()
    if dt is not None:
        m.rrt.compute_dtype = dt
    sizes = [3000, 700, 1, 2200]
    bags = [torch.from_numpy(synth.bag(n, 256, tag=f"clambags/{i}", nonneg=True)).to(DEV) for i, n in enumerate(sizes)]
    with torch.no_grad():
        outs = m.forward_bags(bags, streams=4, return_attn=True, return_features=True)
        ref = [m.forward_bag(b, return_attn=True, return_features=True, solo=False) for b in bags]
        again = m.forward_bags([b.unsqueeze(0) for b in bags], streams=4, return_attn=True, return_features=True)
    torch.cuda.synchronize()
    for o, r, o2 in zip(outs, ref, again):
        for k in ("logits", "attn", "features"):
            assert torch.equal(o[k], r[k]) and torch.equal(o2[k], r[k]), k
    assert m.forward_bags([]) == []


def test_clam_autocast_bf16():
    g = load_golden("clam_mb_n3")
    m, x, _lab = _model(g)
    with torch.no_grad():
        f32 = m(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lo = m(x)
            lo2 = m(x)
    torch.cuda.synchronize()
    err = float(np.abs(lo.float().cpu().numpy() - g["logits"]).max())
    print(f"bf16 logits err {err:.3e}; distance to the fp32 run {float((lo.float() - f32).abs().max()):.3e}")
    assert err <= 2e-2
    assert float((lo.float() - f32).abs().max()) > 1e-5              # visibly not the fp32 result: the mode is on
    assert torch.equal(lo, lo2)


@pytest.mark.parametrize("N", [33, 300])
def test_clam_no_encoder_autocast_bf16(N):
    """rrt=None under bf16 autocast: the heads' shared front runs the 16-bit embedding (cast launch + 16-bit-operand GEMM),
    there is no encoder and the head reads the embedding itself (y == emb), its gate Linears on fp32 rows.  The one-call
    forward against the reference's op sequence for the head (fp32 torch ops) behind the layer path's embedding, within
    test_clam_autocast_bf16's bound; two calls give the same bits."""
    torch.manual_seed(7)
    m = CLAM_SB(input_dim=128, rrt=None).to(DEV).eval()
    x = torch.from_numpy(synth.bag(N, 128, tag=f"clam/no_rrt_bf16/{N}", nonneg=True)).to(DEV)
    with torch.no_grad():
        f32 = m.forward_bag(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lo = m.forward_bag(x, return_features=True, return_attn=True)
            lo2 = m.forward_bag(x, return_features=True, return_attn=True)
            y = m._embed_encode(x)
        eager, _M, _A, _raw = m._eager_head(y)
    torch.cuda.synchronize()
    assert lo["logits"].shape == (1, 2) and lo["attn"].shape == (1, N) and lo["features"].shape == (1, 512)
    err = float((lo["logits"] - eager).abs().max())
    print(f"N={N}: bf16 logits err vs eager head {err:.3e}; distance to the fp32 run {float((lo['logits'] - f32).abs().max()):.3e}")
    assert err <= 2e-2
    for k in lo:
        assert torch.equal(lo[k], lo2[k]), k


def test_clam_fails_loudly():
    m = CLAM_SB(64).to(DEV).eval()
    with pytest.raises(ValueError):
        m.forward_bag(torch.zeros(10, 96, device=DEV))
    out = CLAM_SB(64, dropout=0.25).to(DEV).train()(torch.randn(1, 40, 64, device=DEV), label=torch.tensor([1], device=DEV))
    assert out[0].grad_fn is not None and out[0].shape == (1, 2) and out[2] == 40
    with pytest.raises(NotImplementedError):
        CLAM_SB(64, dropout=0.25).to(DEV).train().forward_bag(torch.zeros(10, 64, device=DEV))
    assert m(torch.randn(1, 40, 64, device=DEV)).shape == (1, 2)              # rrt=None: the reference allows it
