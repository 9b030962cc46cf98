"""CPU: the DSMIL head's C-ABI surface (exports, argument checks, workspace sizes) and the state_dict surface of MILNet
against the reference's key lists (tools/make_golden_dsmil.py).  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_names, load_golden
import rrt_mil_amd
from rrt_mil_amd import DSMIL, MILNet, RRTEncoder, _lib, synth
from rrt_mil_amd.build import build

CASES = [n for n in golden_names("dsmil_") if n != "dsmil_keys"]
P = 0x1000          # a non-NULL pointer for calls that must stop at a check before anything is launched
NEW = ("rrt_instance_max_workspace_size", "rrt_instance_max_f32", "rrt_dsmil_pool_workspace_size", "rrt_dsmil_pool_f32",
       "rrt_dsmil_workspace_size", "rrt_dsmil_forward_f32")


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def test_exports_and_abi(lib):
    assert _lib.ABI_VERSION == 29 and lib.rrt_abi_version() == 29
    with open(os.path.join(ROOT, "include", "rrt_hip.h")) as fh:
        header = fh.read()
    assert "#define RRT_ABI_VERSION 29" in header
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "typedef struct rrt_dsmil_desc" in header and "typedef struct rrt_dsmil_weights" in header
    assert {"MILNet", "DSMIL"} <= set(rrt_mil_amd.__all__) and DSMIL is MILNet


def _unsupported(lib, rc, word):
    assert rc == -2 and word in lib.rrt_strerror(rc), (rc, lib.rrt_strerror(rc))


def test_instance_max_argument_checks(lib):
    n = C.c_size_t()
    ws = lambda N, D, K: lib.rrt_instance_max_workspace_size(N, D, K, C.byref(n))   # noqa: E731
    assert ws(100, 512, 1) == 0 and ws(100, 512, 8) == 0 and ws(1, 64, 2) == 0 and ws(1000000, 2048, 8) == 0
    for bad, word in (((100, 512, 0), b"n_classes"), ((100, 512, 9), b"n_classes"), ((100, 48, 2), b"dim"),
                      ((100, 2080, 2), b"dim"), ((1000001, 512, 2), b"1e6")):
        _unsupported(lib, ws(*bad), word)
    assert ws(0, 512, 2) == -1 and lib.rrt_instance_max_workspace_size(100, 512, 2, None) == -1
    fwd = lambda y=P, w=P, am=P, N=100, D=512, K=2, wsp=P, wsb=0: lib.rrt_instance_max_f32(   # noqa: E731
        y, w, None, None, None, am, N, D, K, wsp, wsb, None)
    assert fwd(y=None) == -1 and fwd(w=None) == -1 and fwd(am=None) == -1 and fwd(N=0) == -1
    _unsupported(lib, fwd(K=0), b"n_classes")
    _unsupported(lib, fwd(K=9), b"n_classes")
    _unsupported(lib, fwd(D=48), b"dim")
    _unsupported(lib, fwd(N=1000001), b"1e6")
    assert ws(100, 512, 2) == 0
    assert fwd() == -3 and fwd(wsb=n.value - 1) == -3 and fwd(wsp=None, wsb=n.value) == -3


def test_dsmil_pool_argument_checks(lib):
    n = C.c_size_t()
    ws = lambda N, D, Q, K: lib.rrt_dsmil_pool_workspace_size(N, D, Q, K, C.byref(n))   # noqa: E731
    assert ws(100, 512, 128, 1) == 0 and ws(100, 512, 128, 8) == 0 and ws(1, 64, 32, 2) == 0
    for bad, word in (((100, 512, 128, 0), b"n_classes"), ((100, 512, 128, 9), b"n_classes"), ((100, 48, 128, 2), b"dim"),
                      ((100, 2080, 128, 2), b"dim"), ((100, 512, 126, 2), b"q_dim"), ((1000001, 512, 128, 2), b"1e6")):
        _unsupported(lib, ws(*bad), word)
    assert ws(0, 512, 128, 2) == -1 and ws(100, 512, 0, 2) == -1 and lib.rrt_dsmil_pool_workspace_size(100, 512, 128, 2, None) == -1

    def fwd(feats=P, am=P, qw=P, fw=P, lg=P, N=100, D=512, Q=128, K=2, wsp=P, wsb=0):
        return lib.rrt_dsmil_pool_f32(feats, am, qw, None, fw, None, lg, None, None, None, N, D, Q, K, wsp, wsb, None)
    for null in ("feats", "am", "qw", "fw", "lg"):
        assert fwd(**{null: None}) == -1, null
    assert fwd(N=0) == -1
    _unsupported(lib, fwd(K=0), b"n_classes")
    _unsupported(lib, fwd(K=9), b"n_classes")
    _unsupported(lib, fwd(D=48), b"dim")
    _unsupported(lib, fwd(Q=126), b"q_dim")
    _unsupported(lib, fwd(N=1000001), b"1e6")
    assert ws(100, 512, 128, 2) == 0
    assert fwd() == -3 and fwd(wsb=n.value - 1) == -3 and fwd(wsp=None, wsb=n.value) == -3


def test_dsmil_forward_argument_checks(lib):
    n = C.c_size_t()
    m = MILNet(2, 0., "relu", input_dim=128, rrt=RRTEncoder())
    d, w = m._desc_weights(128, True)
    size = lambda N=100: lib.rrt_dsmil_workspace_size(C.byref(d), N, C.byref(n))   # noqa: E731
    fwd = lambda x=P, lg=P, N=100, wsp=P, wsb=0: lib.rrt_dsmil_forward_f32(C.byref(d), C.byref(w), x, lg, None, None, None, None,   # noqa: E731
                                                                          N, wsp, wsb, None)
    assert size() == 0 and n.value > 0
    assert fwd(x=None) == -1 and fwd(lg=None) == -1 and fwd(N=0) == -1 and size(0) == -1
    assert lib.rrt_dsmil_workspace_size(None, 100, C.byref(n)) == -1 and lib.rrt_dsmil_workspace_size(C.byref(d), 100, None) == -1
    assert lib.rrt_dsmil_forward_f32(None, C.byref(w), P, P, None, None, None, None, 100, P, 0, None) == -1
    assert lib.rrt_dsmil_forward_f32(C.byref(d), None, P, P, None, None, None, None, 100, P, 0, None) == -1
    assert size() == 0
    assert fwd() == -3 and fwd(wsb=n.value - 1) == -3 and fwd(wsp=None, wsb=n.value) == -3
    _unsupported(lib, size(1000001), b"1e6")
    _unsupported(lib, fwd(N=1000001), b"1e6")
    for field, bad, word in (("n_classes", 0, b"n_classes"), ("n_classes", 9, b"n_classes"), ("q_dim", 126, b"q_dim"),
                             ("input_dim", 48, b"input_dim"), ("emb_act", 4, b"emb_act")):
        was = getattr(d, field)
        setattr(d, field, bad)
        _unsupported(lib, size(), word)
        _unsupported(lib, fwd(), word)
        setattr(d, field, was)
    d.enc.dim = 48
    _unsupported(lib, size(), b"dim")
    d.enc.dim = 512
    w.q_w = None                                    # a missing weight: invalid before anything is launched
    assert size() == 0 and fwd(wsb=n.value) == -1


def test_workspace_sizes_monotone(lib):
    n = C.c_size_t()

    def im(N, K):
        assert lib.rrt_instance_max_workspace_size(N, 512, K, C.byref(n)) == 0
        return n.value

    def pool(N, K):
        assert lib.rrt_dsmil_pool_workspace_size(N, 512, 128, K, C.byref(n)) == 0
        return n.value

    def whole(model, N):
        d, _w = model._desc_weights(128, True)
        assert lib.rrt_dsmil_workspace_size(C.byref(d), N, C.byref(n)) == 0
        return n.value
    Ns = (1, 31, 32, 33, 127, 128, 129, 1000, 9000, 100000, 1000000)
    for fn in (im, pool):
        a = [fn(N, 3) for N in Ns]
        assert a == sorted(a) and a[0] > 0 and a[-1] > a[0]
        b = [fn(100000, K) for K in range(1, 9)]
        assert b == sorted(b) and b[-1] > b[0]
    # bag stream partials: K * dim + 16 floats per 32-token chunk, plus the raw scores
    assert pool(1000, 8) >= (32 * (8 * 512 + 16) + 1000 * 8) * 4
    models = [MILNet(K, 0., "relu", input_dim=128, rrt=RRTEncoder()) for K in (1, 2, 8)]
    a = [whole(models[1], N) for N in (1, 10, 100, 1000, 9000)]
    assert a == sorted(a) and a[-1] > a[0]
    b = [whole(m, 1000) for m in models]
    assert b == sorted(b) and b[-1] > b[0]
    assert whole(models[1], 1000) > whole(MILNet(2, 0., "relu", input_dim=128), 1000)


def test_state_dict_surface_every_combination():
    """keys, order and shapes of state_dict() equal the reference's for every dropout x rrt x act combination"""
    combos = load_golden("dsmil_keys")["cfg"]["combos"]
    assert len(combos) == 8
    for c in combos:
        m = MILNet(c["n_classes"], c["dropout"], c["act"], input_dim=c["input_dim"],
                   rrt=RRTEncoder(**c["enc"]) if c["rrt"] else None)
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == c["keys"], (c["dropout"], c["rrt"], c["act"])
        heads = [k for k, _ in got if not k.startswith("rrt.")]
        assert heads == ["patch_to_emb.0.weight", "patch_to_emb.0.bias", "i_classifier.weight", "i_classifier.bias",
                         "b_classifier.q.weight", "b_classifier.q.bias", "b_classifier.fcc.weight", "b_classifier.fcc.bias"]


@pytest.mark.parametrize("name", CASES)
def test_golden_state_loads_strict(name):
    cfg = load_golden(name)["cfg"]
    m = MILNet(cfg["n_classes"], 0., cfg["act"], input_dim=cfg["input_dim"],
               rrt=RRTEncoder(drop_out=0., **cfg["enc"]) if cfg["rrt"] else None)
    shapes = {k: tuple(s) for k, s in cfg["ref_keys"] if not k.startswith("rrt.")}
    st = synth.dsmil_head_state(shapes, cfg["name"])
    if cfg["rrt"]:
        st.update({"rrt." + k: v for k, v in synth.encoder_state(**{k: v for k, v in cfg["enc"].items() if k != "region_num"}).items()})
    sd = {k: torch.from_numpy(np.array(v)) for k, v in st.items()}
    assert set(sd) == {k for k, _ in cfg["ref_keys"]} and [[k, list(v.shape)] for k, v in m.state_dict().items()] == cfg["ref_keys"]
    m.load_state_dict(sd, strict=True)


def test_goldens_hold_their_gap():
    assert set(CASES) == {"dsmil_n2", "dsmil_n3", "dsmil_n2_norrt", "dsmil_n2_bce", "dsmil_n2_wide"}
    for name in CASES:
        assert load_golden(name)["cfg"]["gap"] >= (0.2 if name == "dsmil_n2_wide" else 1e-2), name


def test_cpu_tensor_and_bad_rrt_raise():
    m = MILNet(2, 0., "relu", input_dim=64).eval()
    with pytest.raises(_lib.RRTHipError):
        m(torch.zeros(1, 10, 64))
    with pytest.raises(_lib.RRTHipError):
        m.forward_bag(torch.zeros(10, 64))
    with pytest.raises(_lib.RRTHipError):
        m.forward_bags([torch.zeros(10, 64)])
    with pytest.raises(TypeError):
        MILNet(2, 0., "relu", input_dim=64, rrt=torch.nn.Identity())
    with pytest.raises(ValueError):
        MILNet(2, 0., "relu", input_dim=64, rrt=RRTEncoder(mlp_dim=256))
    from rrt_mil_amd.dsmil import BClassifier
    for kw in ({"nonlinear": True}, {"passing_v": True}):
        with pytest.raises(NotImplementedError):
            BClassifier(512, 2, **kw)
