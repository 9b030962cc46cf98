"""CPU: the ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL heads without a device -- the float64 restatement
(tests/bagmil_ref.py) against the reference's goldens (tools/make_golden_bagmil.py), the state_dict surface against the
reference's key lists, the C-ABI surface (exports, argument checks, workspace sizes), the quirk cases, the MaxMIL margins and
what the case lists of tests/bagmil_cases.py claim to cover.  No GPU compute."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import bagmil_cases as BC
import bagmil_ref as R
from conftest import ROOT, load_golden
import rrt_mil_amd
from rrt_mil_amd import ABMIL, GatedABMIL, IBMIL, MaxMIL, MeanMIL, RRTEncoder, _lib
from rrt_mil_amd.build import build

CLASSES = {"attmil": ABMIL, "gattmil": GatedABMIL, "ibmil": IBMIL, "meanmil": MeanMIL, "maxmil": MaxMIL}
P = 0x1000          # a non-NULL pointer for calls that must stop at a check before anything is launched
NEW = ("rrt_bag_mean_workspace_size", "rrt_bag_mean_f32", "rrt_bag_mean_backward_f32", "rrt_deconf_head_f32",
       "rrt_bagmil_workspace_size", "rrt_bagmil_forward_f32")


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


@pytest.fixture(scope="module")
def conf(tmp_path_factory):
    return BC.conf_file(tmp_path_factory.mktemp("conf"))


@functools.lru_cache(maxsize=None)
def ref64(kind, rrt, n):
    """the restatement in float64 on a whole-head case (computed once, shared)"""
    g = load_golden(f"bagmil_{kind}")
    info = g["cfg"]["cases"][BC.case_id(kind, rrt, n)]
    state = BC.head_state({k: np.empty(s) for k, s in info["ref_keys"]}, kind)
    want_grad = (kind, rrt, n) in BC.GRAD_CASES
    return R.head(kind, BC.bag(kind, rrt, n), state, BC.ENC_CFG, act=BC.ACT[kind], gate_act=BC.ACT[kind], grad=want_grad), g


# ------------------------------------------------------------------ the restatement is the reference
@pytest.mark.parametrize("kind,rrt,n", BC.WHOLE_CASES, ids=lambda v: str(v))
def test_restatement_matches_reference(kind, rrt, n):
    out, g = ref64(kind, rrt, n)
    cid = BC.case_id(kind, rrt, n)
    for q in ("logits", "pooled", "attn", "deconf_cf"):
        if f"{cid}/{q}" not in g:
            assert q not in out or (kind == "meanmil" and q == "pooled"), (cid, q)
            continue
        got = out[q].detach()
        got = got[g[f"{cid}/attn_idx"]] if q == "attn" else got
        err = R.rel_err(got, g[f"{cid}/{q}"])
        print(f"{cid} {q}: {err:.2e}")
        assert err <= 1e-10, (cid, q, err)
    assert f"{cid}/logits" in g and (kind in ("meanmil", "maxmil") or f"{cid}/attn" in g)
    if kind == "maxmil":
        assert out["argmax"].tolist() == g[f"{cid}/argmax"].tolist()


@pytest.mark.parametrize("kind,rrt,n", BC.GRAD_CASES, ids=lambda v: str(v))
def test_restatement_gradients_match_reference(kind, rrt, n):
    out, g = ref64(kind, rrt, n)
    cid = BC.case_id(kind, rrt, n)
    info = g["cfg"]["cases"][cid]
    loss = torch.nn.functional.cross_entropy(out["logits"], torch.tensor([info["label"]]))
    grads = torch.autograd.grad(loss, [out["x_leaf"]] + [v for v in out["params"].values() if v.is_floating_point()],
                                allow_unused=True, retain_graph=True)
    names = ["x"] + [k for k, v in out["params"].items() if v.is_floating_point()]
    assert abs(float(loss.detach()) - float(g[f"{cid}/loss"])) <= 1e-10
    seen = 0
    for name, gr in zip(names, grads):
        if name in info["none"] or name == "confounder_feat":
            continue
        key = f"{cid}/g__" + name.replace(".", "__")
        assert key + "__max" in g and gr is not None, name
        got, scale = gr.detach().numpy(), float(g[key + "__max"])
        if key + "__full" in g:
            got, ref = got.reshape(g[key + "__full"].shape), g[key + "__full"]
        else:
            got, ref = got.reshape(got.shape[0], -1)[g[key + "__rows"]], g[key + "__vals"]
        # (the fixture keeps fp32 roundings of the float64 gradients)
        assert float(np.abs(got - ref).max()) <= 2e-7 * max(scale, 1e-30) + 1e-12, name
        seen += 1
    assert seen >= 20


# ------------------------------------------------------------------ the state_dict surface
def test_state_dict_surface_every_combination(conf):
    combos = load_golden("bagmil_keys")["cfg"]["combos"]
    assert len(combos) == 64 and {c["kind"] for c in combos} == set(BC.HEADS)
    for kind in BC.HEADS:
        mine = [c for c in combos if c["kind"] == kind]
        assert {(c["dropout"] > 0, c["rrt"]) for c in mine} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {"relu", "gelu"} <= {c["act"] for c in mine}
    for c in combos:
        m = BC.construct(CLASSES, c["kind"], rrt=RRTEncoder(**BC.ENC_CFG) if c["rrt"] else None, dropout=c["dropout"], act=c["act"],
                         conf_path=conf if c["conf"] else False, bias=c["bias"])
        sd = m.state_dict()
        got = [[k, list(v.shape)] for k, v in sd.items()]
        assert got == c["keys"], (c["kind"], c["dropout"], c["rrt"], c["act"], c["conf"])
        st = BC.head_state(sd, c["kind"])
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()}, strict=True)
    # the index of rrt inside the Sequential moves with dropout (and, for MeanMIL / MaxMIL, with act)
    where = {(c["kind"], c["dropout"] > 0, c["act"]): R.rrt_prefix([k for k, _ in c["keys"]]) for c in combos if c["rrt"]}
    assert where[("attmil", False, "relu")] == "feature.2." and where[("attmil", True, "relu")] == "feature.3."
    assert where[("gattmil", False, "relu")] == "feature.3." and where[("ibmil", True, "gelu")] == "embedding.rrt."
    assert where[("meanmil", False, "none")] == "head.1." and where[("maxmil", True, "gelu")] == "head.3."


def test_exports_and_abi(lib):
    assert _lib.ABI_VERSION == 29 and lib.rrt_abi_version() == 29
    with open(os.path.join(ROOT, "include", "rrt_hip.h")) as fh:
        header = fh.read()
    assert "#define RRT_ABI_VERSION 29" in header
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "typedef struct rrt_bagmil_desc" in header and "typedef struct rrt_bagmil_weights" in header
    assert {"ABMIL", "GatedABMIL", "IBMIL", "MeanMIL", "MaxMIL"} <= set(rrt_mil_amd.__all__)
    from rrt_mil_amd import _head, attmil, attmil_ibmil, dsmil, mean_max, mil
    assert ABMIL is attmil.DAttention and GatedABMIL is attmil.AttentionGated and IBMIL is attmil_ibmil.Dattention_ori
    assert rrt_mil_amd.DAttention is mil.DAttention and rrt_mil_amd.AttentionGated is mil.AttentionGated
    assert hasattr(attmil_ibmil, "FCLayer") and MeanMIL is mean_max.MeanMIL
    assert dsmil._InstanceMax is _head._InstanceMax and dsmil.instance_max is _head.instance_max


# ------------------------------------------------------------------ argument checks and workspace sizes
def _unsupported(lib, rc, word):
    assert rc == -2 and word in lib.rrt_strerror(rc), (rc, lib.rrt_strerror(rc))


def test_bag_mean_argument_checks(lib):
    n = C.c_size_t()
    ws = lambda N, D, K: lib.rrt_bag_mean_workspace_size(N, D, K, C.byref(n))   # noqa: E731
    assert ws(100, 512, 1) == 0 and ws(100, 512, 8) == 0 and ws(1, 32, 2) == 0 and ws(1000000, 2048, 8) == 0
    for bad, word in (((100, 512, 0), b"n_classes"), ((100, 512, 9), b"n_classes"), ((100, 48, 2), b"dim"),
                      ((100, 2080, 2), b"dim"), ((1000001, 512, 2), b"1e6")):
        _unsupported(lib, ws(*bad), word)
    assert ws(0, 512, 2) == -1 and lib.rrt_bag_mean_workspace_size(100, 512, 2, None) == -1
    fwd = lambda y=P, w=P, lg=P, N=100, D=512, K=2, wsp=P, wsb=0: lib.rrt_bag_mean_f32(y, w, None, lg, None, N, D, K, wsp, wsb, None)   # noqa: E731
    assert fwd(y=None) == -1 and fwd(w=None) == -1 and fwd(lg=None) == -1 and fwd(N=0) == -1
    _unsupported(lib, fwd(K=9), b"n_classes")
    _unsupported(lib, fwd(D=48), b"dim")
    _unsupported(lib, fwd(N=1000001), b"1e6")
    assert ws(100, 512, 2) == 0
    assert fwd() == -3 and fwd(wsb=n.value - 1) == -3 and fwd(wsp=None, wsb=n.value) == -3
    bwd = lambda dl=P, cm=P, w=P, dy=P, dw=P, db=P, N=100, D=512, K=2: lib.rrt_bag_mean_backward_f32(dl, cm, w, dy, dw, db, N, D, K, None)   # noqa: E731
    assert bwd(dl=None) == -1 and bwd(w=None) == -1 and bwd(cm=None) == -1 and bwd(dy=None, dw=None, db=None) == -1 and bwd(N=0) == -1
    _unsupported(lib, bwd(K=0), b"n_classes")
    _unsupported(lib, bwd(D=2080), b"dim")
    _unsupported(lib, bwd(N=1000001), b"1e6")


def test_deconf_argument_checks(lib):
    def call(pooled=P, conf=P, qw=P, kw=P, hw=P, lg=P, dim=512, K=8, V=512, J=128, Cn=2):
        return lib.rrt_deconf_head_f32(pooled, conf, qw, None, kw, None, hw, None, lg, None, None, dim, K, V, J, Cn, None)
    for null in ("pooled", "conf", "qw", "kw", "hw", "lg"):
        assert call(**{null: None}) == -1, null
    assert call(Cn=0) == -1 and call(dim=0) == -1
    for bad, word in ((dict(K=0), b"n_conf"), (dict(K=65), b"n_conf"), (dict(dim=48), b"dim"), (dict(dim=2080), b"dim"),
                      (dict(V=48), b"conf_dim"), (dict(V=4096), b"conf_dim"), (dict(J=126), b"joint_dim"), (dict(J=516), b"joint_dim")):
        _unsupported(lib, call(**bad), word)


def _desc(kind, conf, rrt=True, **kw):
    m = BC.construct(CLASSES, kind, rrt=RRTEncoder() if rrt else None, conf_path=conf if kind == "ibmil" else False, **kw)
    return m, m._desc_weights(True)


@pytest.mark.parametrize("kind", BC.HEADS)
def test_bagmil_forward_argument_checks(lib, conf, kind):
    n = C.c_size_t()
    m, (d, w) = _desc(kind, conf)
    assert d.pool == {"meanmil": 0, "maxmil": 1, "attmil": 2, "gattmil": 3, "ibmil": 4}[kind] and d.has_rrt == 1
    size = lambda N=100: lib.rrt_bagmil_workspace_size(C.byref(d), N, C.byref(n))   # noqa: E731

    def fwd(x=P, lg=P, N=100, wsp=P, wsb=0, attn=None, pooled=None, amax=None, da=None, dcf=None):
        return lib.rrt_bagmil_forward_f32(C.byref(d), C.byref(w), x, lg, attn, 0, pooled, amax, da, dcf, N, wsp, wsb, None)
    assert size() == 0 and n.value > 0
    assert fwd(x=None) == -1 and fwd(lg=None) == -1 and fwd(N=0) == -1 and size(0) == -1
    assert lib.rrt_bagmil_workspace_size(None, 100, C.byref(n)) == -1 and lib.rrt_bagmil_workspace_size(C.byref(d), 100, None) == -1
    assert size() == 0
    assert fwd() == -3 and fwd(wsb=n.value - 1) == -3 and fwd(wsp=None, wsb=n.value) == -3
    _unsupported(lib, size(1000001), b"1e6")
    _unsupported(lib, fwd(N=1000001), b"1e6")
    # an output the pool does not produce is refused before anything is launched
    att = kind in ("attmil", "gattmil", "ibmil")
    if not att:
        assert fwd(wsb=n.value, attn=P) == -1
    if kind != "maxmil":
        assert fwd(wsb=n.value, amax=P) == -1
    else:
        assert fwd(wsb=n.value, pooled=P) == -1
    if kind != "ibmil":
        assert fwd(wsb=n.value, da=P) == -1 and fwd(wsb=n.value, dcf=P) == -1
    bad = [("input_dim", 48, b"input_dim"), ("emb_act", 4, b"emb_act"), ("pool", 5, b"pool"), ("pool", -1, b"pool")]
    if kind in ("meanmil", "maxmil"):
        bad += [("n_classes", 9, b"n_classes")]
    else:
        bad += [("pool_hidden", 126, b"hidden")]
    if kind == "ibmil":
        bad += [("deconf_k", 0, b"n_conf"), ("deconf_k", 65, b"n_conf"), ("deconf_v", 48, b"conf_dim"), ("deconf_j", 126, b"joint_dim")]
    for field, val, word in bad:
        was = getattr(d, field)
        setattr(d, field, val)
        _unsupported(lib, size(), word)
        _unsupported(lib, fwd(), word)
        setattr(d, field, was)
    d.n_classes = 0
    assert size() == -1
    d.n_classes = m._classifier().out_features
    d.enc.dim = 48
    _unsupported(lib, size(), b"dim")
    d.enc.dim = 512
    w.cls_w = None                                  # a missing weight: invalid before anything is launched
    assert size() == 0 and fwd(wsb=n.value) == -1


def test_workspace_sizes_monotone(lib, conf):
    n = C.c_size_t()

    def mean(N, K=3, dim=512):
        assert lib.rrt_bag_mean_workspace_size(N, dim, K, C.byref(n)) == 0
        return n.value
    Ns = (1, 31, 32, 33, 2047, 2048, 2049, 4097, 9000, 100000, 1000000)
    a = [mean(N) for N in Ns]
    assert a == sorted(a) and a[0] > 0 and a[-1] > a[0]
    assert mean(9000) >= (282 + 5) * 512 * 4 and mean(1000, dim=2048) > mean(1000, dim=512)
    for kind in BC.HEADS:
        (_m, (d, _w)), (_m0, (d0, _w0)) = _desc(kind, conf), _desc(kind, conf, rrt=False)

        def whole(dd, N):
            assert lib.rrt_bagmil_workspace_size(C.byref(dd), N, C.byref(n)) == 0
            return n.value
        a = [whole(d, N) for N in (2, 10, 100, 1000, 9000)]
        assert a == sorted(a) and a[-1] > a[0], kind
        assert whole(d, 1000) > whole(d0, 1000), kind


# ------------------------------------------------------------------ quirks
def test_quirks_raise_as_stated(conf):
    for bad in (1024, 256):
        g = GatedABMIL(bad)                                         # constructs, its checkpoint surface exists ...
        assert g.attention_a[0].in_features == bad and g.classifier[0].in_features == bad and g.feature[0].in_features == 1024
        with pytest.raises(ValueError, match="input_dim=512"):      # ... and cannot run
            g.eval()(torch.zeros(1, 10, 1024))
        with pytest.raises(ValueError, match="input_dim=512"):
            g.forward_bag(torch.zeros(10, 1024))
    assert GatedABMIL(512).classifier[0].out_features == 2 and isinstance(GatedABMIL(512).feature[2], torch.nn.Dropout)
    assert MaxMIL(256).head[0].in_features == 1024 and MeanMIL(256).head[0].in_features == 256
    ib = IBMIL(out_dim=2, in_size=64, confounder_path=conf)
    assert ib.confounder_feat.shape == (BC.N_CONF, 512) and ib.head.in_features == 1024 and isinstance(ib.dropout, torch.nn.Dropout)
    assert ib._dropouts() == [ib.embedding.embed[2]]                # self.dropout (p = 0.5) is never applied
    ib2 = IBMIL(out_dim=2, in_size=64, confounder_path=[conf, conf])
    assert ib2.confounder_feat.shape == (2 * BC.N_CONF, 512)
    with pytest.raises(ValueError, match="one instance"):
        ib.eval()(torch.zeros(1, 1, 64))
    with pytest.raises(ValueError, match="one instance"):
        ib.forward_bag(torch.zeros(1, 64))
    plain = IBMIL(out_dim=3, in_size=64)                            # confounder_path=False: the plain head
    assert plain.head.in_features == 512 and not hasattr(plain, "W_q") and "confounder_feat" not in plain.state_dict()
    assert plain._desc_weights(True)[0].pool == _lib.BAGPOOL_ATTN and ib._desc_weights(True)[0].pool == _lib.BAGPOOL_ATTN_DECONF


def test_cpu_tensor_and_bad_rrt_raise(conf):
    for kind in BC.HEADS:
        m = BC.construct(CLASSES, kind, conf_path=conf if kind == "ibmil" else False).eval()
        x = torch.zeros(10, BC.INPUT_DIM[kind])
        with pytest.raises(_lib.RRTHipError):
            m(x[None])
        with pytest.raises(_lib.RRTHipError):
            m.forward_bag(x)
        with pytest.raises(_lib.RRTHipError):
            m.forward_bags([x])
        with pytest.raises(ValueError):
            m.forward_bag(torch.zeros(10, 96))
        with pytest.raises(TypeError):
            BC.construct(CLASSES, kind, rrt=torch.nn.Identity(), conf_path=conf if kind == "ibmil" else False)
        with pytest.raises(ValueError):
            BC.construct(CLASSES, kind, rrt=RRTEncoder(mlp_dim=256), conf_path=conf if kind == "ibmil" else False)
        assert m.forward_bags([]) == []


# ------------------------------------------------------------------ the cases
def test_every_max_pool_case_holds_its_margin():
    cases = [c for c in BC.WHOLE_CASES if c[0] == "maxmil"]
    assert len(cases) == 6 and set(cases) == set(BC.SEED)
    for kind, rrt, n in cases:
        out, g = ref64(kind, rrt, n)
        s = out["scores"].detach()
        if n > 1:
            top = torch.sort(s, 0, descending=True)[0]
            gap = float((top[0] - top[1]).min())
            print(f"{BC.case_id(kind, rrt, n)}: gap {gap:.3e}, {gap / float(s.abs().max()):.3e} of the largest |logit|")
            assert gap >= BC.MARGIN * float(s.abs().max()), (kind, rrt, n)
        assert g["cfg"]["cases"][BC.case_id(kind, rrt, n)]["margin"] >= BC.MARGIN


def test_case_lists_cover_what_they_claim():
    src = open(os.path.join(ROOT, "rrt-mil_amd", "csrc", "internal.h")).read()
    for name, val in (("MEAN_CHUNK", BC.MEAN_CHUNK), ("MEAN_FAN", BC.MEAN_FAN), ("MEAN_BWD_ROWS", BC.MEAN_BWD_ROWS)):
        assert re.search(rf"constexpr int {name} = {val};", src), name
    for edge in BC.MEAN_EDGES:
        assert {edge - 1, edge, edge + 1} <= set(BC.MEAN_NS), edge
    assert {1, 2} <= set(BC.MEAN_NS)
    nb1 = -(-BC.MEAN_ALL_LEVELS // BC.MEAN_CHUNK)
    assert BC.MEAN_ALL_LEVELS in BC.MEAN_NS and nb1 > BC.MEAN_FAN and -(-nb1 // BC.MEAN_FAN) > 1
    assert BC.MEAN_ALL_LEVELS % BC.MEAN_CHUNK and nb1 % BC.MEAN_FAN                 # ragged at both levels
    assert BC.MEAN_DIMS == (32, 512, 2048) and BC.MEAN_CS == (1, 2, 8) and BC.DECONF_KS == (1, 2, 8, 64)
    assert (512, 512, 128) in {s[:3] for s in BC.DECONF_SHAPES} and BC.DECONF_GAINS == (1.0, 6.0)
    for dim, v, j, c in BC.DECONF_SHAPES:
        for k in BC.DECONF_KS:
            for gain in BC.DECONF_GAINS:
                raw = R.deconf_head(*BC.deconf_inputs(dim, v, j, c, k, gain), dtype=torch.float64)[3]
                peak = float(raw.abs().max())
                if gain == 1.0:
                    assert abs(peak - 1.0) < 1e-5, (dim, k, peak)
                else:
                    assert BC.PEAK_RANGE[0] <= peak <= BC.PEAK_RANGE[1], (dim, k, peak)
    want = {(k, False, n) for k in BC.HEADS for n in (1, 2, 300)} - {("ibmil", False, 1)} | \
           {(k, True, n) for k in BC.HEADS for n in (30, 300, 1000)}
    assert set(BC.WHOLE_CASES) == want and len(BC.WHOLE_CASES) == 29
    assert {c[0] for c in BC.GRAD_CASES} == set(BC.HEADS) and all(c[1] and c[2] == 300 for c in BC.GRAD_CASES)
    assert {c[0] for c in BC.AUTOCAST_CASES} == {"attmil", "gattmil", "ibmil"} and set(BC.AUTOCAST_CASES) <= set(BC.WHOLE_CASES)
    for kind in BC.HEADS:
        g = load_golden(f"bagmil_{kind}")
        assert set(g["cfg"]["cases"]) == {BC.case_id(*c) for c in BC.WHOLE_CASES if c[0] == kind}
