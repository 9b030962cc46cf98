"""CPU: DTFD-MIL without a device -- the float64 restatement (tests/dtfd_ref.py) reproduces the reference's goldens
(tests/golden/dtfd.npz, tools/make_golden_dtfd.py), the module keeps the reference's state_dict surface and refuses what it
cannot run, the C ABI refuses bad shapes from its size queries before anything is launched, and header, binding and library
agree on the new symbols."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dtfd_cases as DC
import dtfd_ref as R
from conftest import GOLDEN, ROOT, load_golden
import rrt_mil_amd
from rrt_mil_amd import DTFD, _lib, dtfd
from rrt_mil_amd.build import SOURCES, build

NEW_SYMBOLS = ("rrt_segment_pool_workspace_size", "rrt_gate_scores_f32", "rrt_segment_pool_f32", "rrt_segment_pool_backward_f32",
               "rrt_dtfd_workspace_size", "rrt_dtfd_forward_f32")
E_INVALID, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


@pytest.fixture(scope="module")
def G():
    return load_golden("dtfd")


def new(case=None, **kw):
    args = dict(DC.model_kwargs(case)) if case else dict(input_dim=DC.INPUT_DIM)
    args.update(kw)
    return DTFD(1e-4, 1e-5, 10, R.nll_surv, **args)


def test_golden_is_small_and_pins_its_inputs(G):
    assert os.path.getsize(os.path.join(GOLDEN, "dtfd.npz")) < 200 * 1024
    assert set(G["cfg"]["cases"]) == set(DC.CASES)
    for cid, c in G["cfg"]["cases"].items():
        assert {k: c[k] for k in DC.CASES[cid]} == DC.CASES[cid]
        assert DC.state_sum(DC.state(c["n_classes"])) == c["state_sum"]
        assert float(DC.bag(cid).astype(np.float64).sum()) == c["bag_sum"]
    seen = lambda k: {c[k] for c in DC.CASES.values()}   # noqa: E731
    assert seen("n") == {8, 37, 300} and seen("group") == {1, 3, 8} and seen("n_classes") == {2, 4}
    assert seen("distill") == {"MaxMinS", "MaxS", "AFS"}


@pytest.mark.parametrize("cid", list(DC.CASES))
def test_restatement_reproduces_the_reference_eval(G, cid):
    c = DC.CASES[cid]
    r = R.eval_forward(DC.bag(cid), DC.state(c["n_classes"]), G[f"{cid}/perm"], c["group"], c["distill"])
    assert np.array_equal(r["sel"], G[f"{cid}/sel"])          # every group, by the library's rule from the float64 p
    assert R.rel_err(r["p"], G[f"{cid}/p32"]) <= 4 * max(float(G[f"{cid}/e32_p"]), 1e-7)
    for q in ("logits", "hazards", "S"):
        assert R.rel_err(r[q], G[f"{cid}/{q}64"]) <= 1e-12, q
    # the golden's own selections follow the rule from the recorded fp32 p as well
    assert np.array_equal(R.select_from_p(G[f"{cid}/p32"], G[f"{cid}/perm"], c["group"]), G[f"{cid}/sel"])


@pytest.mark.parametrize("cid", DC.TRAIN_CASES)
def test_restatement_reproduces_the_reference_training_step(G, cid):
    c = DC.CASES[cid]
    r = R.train_step(DC.bag(cid), DC.state(c["n_classes"]), c["group"], c["distill"], **DC.LABEL)
    assert np.array_equal(r["sel"], G[f"{cid}/train_sel"])
    for q in ("hazards", "S", "loss0", "loss"):
        assert R.rel_err(r[q], G[f"{cid}/train_{q}"]) <= 1e-12, q
    pairs = [(f"{w}/{k}", r[w][k]) for w in ("inner", "outer") for k in r[w]] + [("dx", r["dx"])]
    assert len(pairs) == 2 * len(DC.shapes_of(c["n_classes"])) + 1
    for name, got in pairs:
        want, got = G[f"{cid}/{name}"], DC.grad_summary(got.detach().numpy())
        # Sums of many terms: relative to the sum of magnitudes, want[1].  The gradient of either attention_weights.bias is a
        # sum that cancels to zero in exact arithmetic (a softmax does not see a shift of its scores): float64 roundoff on both
        # sides, measured against the weight gradient of the same Linear, which adds up the same terms.
        scale = G[f"{cid}/{name[:-4]}weight"][1] if name.endswith("attention_weights.bias") else want[1]
        assert np.abs(got - want).max() <= 1e-9 * max(scale, 1e-30), (name, np.abs(got - want).max(), scale)


def test_array_split_sizes_in_closed_form():
    for n in range(1, 201):
        for g in range(1, 65):
            want = [len(a) for a in np.array_split(np.arange(n), g)]
            assert R.split_sizes(n, g) == want and dtfd.split_sizes(n, g) == want


def test_selection_rule_of_the_restatement():
    nan = np.nan
    assert R.select(np.array([0.5, 0.7, 0.7, 0.1, 0.1])) == (1, 3)
    assert R.select(np.array([nan, 0.2, nan, 0.2])) == (1, 1)
    assert R.select(np.array([nan, nan])) == (0, 0) and R.select(np.array([0.3])) == (0, 0)
    assert R.select(np.array([0.0, -0.0, 0.0])) == (0, 0)


@pytest.mark.parametrize("n_classes", [2, 4])
def test_state_dict_surface_is_the_references(G, n_classes):
    cid = next(k for k, c in DC.CASES.items() if c["n_classes"] == n_classes)
    want = [(k, tuple(s)) for k, s in G["cfg"]["cases"][cid]["keys"]]
    m = new(cid)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert list(DC.shapes_of(n_classes).items()) == want
    st = {k: torch.from_numpy(np.array(v)) for k, v in DC.state(n_classes).items()}
    m.load_state_dict(st, strict=True)                       # the reference's checkpoint into the module ...
    back = m.state_dict()
    assert list(back) == list(st) and all(torch.equal(back[k], st[k]) for k in st)      # ... and the module's into the reference


def test_constructor_signature_and_attributes():
    sig = inspect.signature(DTFD.__init__)
    assert list(sig.parameters) == ["self", "lr", "weight_decay", "steps", "criterion", "rrt", "epeg_k", "crmsa_k", "input_dim",
                                    "inner_dim", "n_classes", "group", "distill"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(rrt=None, epeg_k=15, crmsa_k=3, input_dim=1024, inner_dim=512, n_classes=2, group=8, distill="MaxMinS")
    m = new()
    assert isinstance(m.optimizer0, torch.optim.Adam) and isinstance(m.scheduler0, torch.optim.lr_scheduler.CosineAnnealingLR)
    held = {id(p) for grp in m.optimizer0.param_groups for p in grp["params"]}
    want = {id(p) for mod in (m.classifier, m.attention, m.dimReduction) for p in mod.parameters()}
    assert held == want and not held & {id(p) for p in m.UClassifier.parameters()}
    assert m.group == 8 and m.distill == "MaxMinS" and m.criterion is R.nll_surv
    assert "DTFD" in rrt_mil_amd.__all__ and "dtfd" in rrt_mil_amd.__all__ and rrt_mil_amd.DTFD is dtfd.DTFD
    for name in ("DTFD", "DimReduction", "Attention", "Classifier_1fc", "Attention_with_Classifier", "get_cam_1d"):
        assert hasattr(dtfd, name), name
    drops = [mod.p for mod in m.modules() if isinstance(mod, torch.nn.Dropout)]
    assert drops == [0.25, 0.25, 0.25]                        # classifier, dimReduction.drop, UClassifier.classifier


def test_get_cam_1d_uses_the_weight_without_the_bias():
    cls = dtfd.Classifier_1fc(16, 3)
    with torch.no_grad():
        cls.fc.bias.fill_(5.0)
    f = torch.randn(1, 7, 16, generator=torch.Generator().manual_seed(1))
    assert torch.allclose(dtfd.get_cam_1d(cls, f), torch.einsum("bgf,cf->bcg", f, cls.fc.weight))


def test_constructor_refusals():
    with pytest.raises(ValueError, match="inner_dim"):
        new(inner_dim=256)
    with pytest.raises(ValueError, match="distill"):
        new(distill="MinS")
    with pytest.raises(ValueError, match="group"):
        new(group=0)
    with pytest.raises(ValueError, match="group"):
        new(group=65)
    with pytest.raises(ValueError, match="n_classes"):
        new(n_classes=9)
    with pytest.raises(TypeError, match="RRTEncoder"):
        new(rrt=torch.nn.Identity())
    with pytest.raises(ValueError, match="final_dim"):
        new(rrt=rrt_mil_amd.RRTEncoder(mlp_dim=256))


def test_call_refusals_need_no_device():
    m = new().eval()
    with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
        m(torch.zeros(1, 40, DC.INPUT_DIM))
    with pytest.raises(ValueError, match="refuses the bag"):
        m(torch.zeros(1, 7, DC.INPUT_DIM))                   # fewer instances than pseudo-bags
    with pytest.raises(ValueError, match="expected a bag"):
        m(torch.zeros(1, 40, DC.INPUT_DIM + 32))
    with pytest.raises(ValueError, match="one bag per call"):
        m(torch.zeros(2, 40, DC.INPUT_DIM))
    with pytest.raises(ValueError, match="refuses the bag"):
        m.train()(torch.zeros(1, 7, DC.INPUT_DIM), label=DC.LABEL)
    with pytest.raises(ValueError, match="refuses the bag"):
        m.forward_bag(torch.zeros(7, DC.INPUT_DIM))


def code(lib, *a):
    b = C.c_size_t(12345)
    rc = lib.rrt_segment_pool_workspace_size(*a, C.byref(b))
    assert rc == 0 or b.value == 12345
    return rc


def test_segment_pool_size_query_refusals(lib):
    assert code(lib, 4099, 512, 2, 8) == 0
    assert code(lib, 0, 512, 2, 8) == E_INVALID and code(lib, 100, 0, 2, 8) == E_INVALID
    assert code(lib, 100, 512, 0, 8) == E_INVALID and code(lib, 100, 512, 2, 0) == E_INVALID
    assert lib.rrt_segment_pool_workspace_size(100, 512, 2, 8, None) == E_INVALID
    for args, word in (((100, 48, 2, 8), "multiple of 32"), ((100, 2080, 2, 8), "2048"), ((100, 512, 9, 8), "n_classes"),
                       ((100, 512, 2, 65), "n_groups"), ((7, 512, 2, 8), "n_tokens < n_groups"),
                       ((1000001, 512, 2, 8), "1e6")):
        assert code(lib, *args) == E_UNSUPPORTED, args
        assert word in lib.rrt_strerror(E_UNSUPPORTED).decode(), (args, lib.rrt_strerror(E_UNSUPPORTED))
    # the size is what the layout says: (m, l) per group, a partial per (group, chunk of 32), the class scores
    b = C.c_size_t()
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    for n, dim, c, g in ((1, 32, 1, 1), (65, 512, 2, 64), (4099, 2048, 8, 3)):
        assert lib.rrt_segment_pool_workspace_size(n, dim, c, g, C.byref(b)) == 0
        parts = sum((s + 31) // 32 for s in R.split_sizes(n, g))
        assert b.value == up(2 * g * 4) + up(parts * (dim + 4) * 4) + up(n * c * 4)


def test_stage_calls_refuse_before_any_launch(lib):
    """no device here: a call that got as far as a launch would return a HIP error (> 0), these return their own codes"""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert lib.rrt_gate_scores_f32(None, None, p, None, p, 10, 128, None) == E_INVALID
    assert lib.rrt_gate_scores_f32(p, None, p, None, p, 0, 128, None) == E_INVALID
    assert lib.rrt_gate_scores_f32(p, None, p, None, p, 10, 126, None) == E_UNSUPPORTED
    assert lib.rrt_gate_scores_f32(p, None, p, None, p, 1000001, 128, None) == E_UNSUPPORTED
    ok = (100, 512, 2, 8)
    assert lib.rrt_segment_pool_f32(None, p, None, p, p, p, None, None, *ok, p, 1 << 30, None) == E_INVALID
    assert lib.rrt_segment_pool_f32(p, p, None, p, p, None, None, None, *ok, p, 1 << 30, None) == E_INVALID
    assert lib.rrt_segment_pool_f32(p, p, None, p, p, p, None, None, 7, 512, 2, 8, p, 1 << 30, None) == E_UNSUPPORTED
    assert lib.rrt_segment_pool_f32(p, p, None, p, p, p, None, None, 100, 512, 9, 8, p, 1 << 30, None) == E_UNSUPPORTED
    assert lib.rrt_segment_pool_f32(p, p, None, p, p, p, None, None, *ok, p, 16, None) == -3
    assert lib.rrt_segment_pool_f32(p, p, None, p, p, p, None, None, *ok, None, 1 << 30, None) == -3
    assert lib.rrt_segment_pool_f32(p + 4, p, None, p, p, p, None, None, *ok, p, 1 << 30, None) == E_INVALID
    assert lib.rrt_segment_pool_backward_f32(p, p, None, p, None, p, p, 100, 512, 8, p, 1 << 30, None) == E_INVALID
    assert lib.rrt_segment_pool_backward_f32(p, p, None, p, p, p, p, 7, 512, 8, p, 1 << 30, None) == E_UNSUPPORTED
    assert lib.rrt_segment_pool_backward_f32(p, p, None, p, p, p, p, 100, 48, 8, p, 1 << 30, None) == E_UNSUPPORTED
    assert lib.rrt_segment_pool_backward_f32(p, p, None, p, p, p, p, 100, 512, 8, p, 16, None) == -3


def test_dtfd_size_query_refusals(lib):
    m = new()
    d, w = m._desc_weights()
    b = C.c_size_t()
    assert lib.rrt_dtfd_workspace_size(C.byref(d), 300, C.byref(b)) == 0 and b.value > 300 * 512 * 4
    assert lib.rrt_dtfd_workspace_size(None, 300, C.byref(b)) == E_INVALID
    assert lib.rrt_dtfd_workspace_size(C.byref(d), 300, None) == E_INVALID
    assert lib.rrt_dtfd_workspace_size(C.byref(d), 0, C.byref(b)) == E_INVALID
    assert lib.rrt_dtfd_workspace_size(C.byref(d), 7, C.byref(b)) == E_UNSUPPORTED
    for field, bad in (("distill", 3), ("group", 65), ("n_classes", 9), ("hidden", 126), ("input_dim", 48), ("emb_act", 3)):
        was = getattr(d, field)
        setattr(d, field, bad)
        assert lib.rrt_dtfd_workspace_size(C.byref(d), 300, C.byref(b)) == E_UNSUPPORTED, field
        setattr(d, field, was)
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert lib.rrt_dtfd_forward_f32(C.byref(d), C.byref(w), None, None, p, None, None, 300, p, 1 << 40, None) == E_INVALID
    assert lib.rrt_dtfd_forward_f32(C.byref(d), C.byref(w), p, None, p, None, None, 7, p, 1 << 40, None) == E_UNSUPPORTED
    assert lib.rrt_dtfd_forward_f32(C.byref(d), C.byref(w), p, None, p, None, None, 300, p, 16, None) == -3
    empty = _lib.DtfdWeights()
    assert lib.rrt_dtfd_forward_f32(C.byref(d), C.byref(empty), p, None, p, None, None, 300, p, 1 << 40, None) == E_INVALID


def test_header_binding_and_library_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert re.search(r"#define\s+RRT_ABI_VERSION\s+29\b", hdr) and _lib.ABI_VERSION == 29 and lib.rrt_abi_version() == 29
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", plain)
        assert proto, name
        n_args = len([a for a in proto.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, (name, n_args)
        assert hasattr(lib, name)
    fields = lambda s: re.findall(r"\*?\s*(\w+)\s*[;,]", re.search(r"typedef struct " + s + r" \{(.*?)\} " + s, plain, re.S).group(1))   # noqa: E731
    assert fields("rrt_dtfd_desc") == [f[0] for f in _lib.DtfdDesc._fields_]
    assert fields("rrt_dtfd_weights") == [f[0] for f in _lib.DtfdWeights._fields_]
    assert (_lib.DTFD_MAXMINS, _lib.DTFD_MAXS, _lib.DTFD_AFS) == (0, 1, 2)
    assert re.search(r"RRT_DTFD_MAXMINS = 0, RRT_DTFD_MAXS = 1, RRT_DTFD_AFS = 2", plain)
    assert "segment_pool.hip" in SOURCES and "api_dtfd.hip" in SOURCES
