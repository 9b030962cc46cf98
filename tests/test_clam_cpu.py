"""CPU: the CLAM heads' C-ABI surface (argument checks, workspace sizes), the state_dict surface of CLAM_SB / CLAM_MB against
the reference's key lists, and the smooth top-1 SVM loss against the reference's value.  No GPU compute."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden
import rrt_mil_amd
from rrt_mil_amd import CLAM_MB, CLAM_SB, RRTEncoder, _lib, synth
from rrt_mil_amd.build import build
from rrt_mil_amd.clam import SmoothTop1SVM

CASES = [n for n in golden_names("clam_") if n != "clam_keys"]
P = 0x1000          # a non-NULL pointer for calls that must stop at a check before anything is launched


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def test_exports_and_abi(lib):
    assert _lib.ABI_VERSION == 29 and lib.rrt_abi_version() == 29
    for name in ("rrt_branch_pool_workspace_size", "rrt_branch_pool_f32", "rrt_branch_pool_backward_f32", "rrt_topk_rows_f32",
                 "rrt_clam_workspace_size", "rrt_clam_forward_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert {"CLAM_SB", "CLAM_MB"} <= set(rrt_mil_amd.__all__)


def test_branch_pool_argument_checks(lib):
    n = C.c_size_t()
    ws = lambda N, D, H, K: lib.rrt_branch_pool_workspace_size(N, D, H, K, C.byref(n))   # noqa: E731
    assert ws(100, 512, 256, 1) == 0 and ws(100, 512, 256, 8) == 0
    for bad, word in (((100, 512, 256, 0), b"n_branches"), ((100, 512, 256, 9), b"n_branches"), ((100, 512, 254, 2), b"hidden"),
                      ((100, 2080, 256, 2), b"dim"), ((100, 48, 256, 2), b"dim"), ((1000001, 512, 256, 2), b"1e6")):
        rc = ws(*bad)
        assert rc == -2 and word in lib.rrt_strerror(rc), bad
    assert ws(0, 512, 256, 1) == -1 and lib.rrt_branch_pool_workspace_size(100, 512, 256, 1, None) == -1
    # forward / backward: NULL pointers -> invalid, unsupported shapes -> unsupported, a short workspace -> workspace
    fwd = lambda y, K=2, H=256, wsb=0: lib.rrt_branch_pool_f32(y, P, None, P, None, P, None, P, 100, 512, H, K, P, wsb, None)   # noqa: E731
    assert fwd(None) == -1 and fwd(P, K=9) == -2 and fwd(P, H=254) == -2 and fwd(P) == -3
    assert lib.rrt_branch_pool_f32(P, P, None, P, None, None, None, P, 100, 512, 256, 2, P, 0, None) == -1       # pooled
    assert lib.rrt_branch_pool_f32(P, P, None, P, None, P, None, None, 100, 512, 256, 2, P, 0, None) == -1       # a_raw
    bwd = lambda dy, K=2, hb=None, dhb=None: lib.rrt_branch_pool_backward_f32(P, P, hb, P, P, P, P, None, dy, P, dhb, P, 100, 512,   # noqa: E731
                                                                            256, K, P, 0, None)
    assert bwd(None) == -1 and bwd(P, hb=P) == -1 and bwd(P, K=0) == -2 and bwd(P) == -3 and bwd(P, hb=P, dhb=P) == -3
    # the adjoint's own limit (its block's LDS): the workspace query and the forward do not have it
    assert ws(100, 2048, 4096, 8) == 0
    assert lib.rrt_branch_pool_f32(P, P, None, P, None, P, None, P, 100, 2048, 4096, 8, P, 0, None) == -3
    rc = lib.rrt_branch_pool_backward_f32(P, P, None, P, P, P, P, None, P, P, None, P, 100, 2048, 4096, 8, P, 0, None)
    assert rc == -2 and b"backward" in lib.rrt_strerror(rc)


def test_topk_argument_checks(lib):
    tk = lambda x, idx, rows, N, k: lib.rrt_topk_rows_f32(x, idx, rows, N, k, None)   # noqa: E731
    assert tk(None, P, 1, 100, 8) == -1 and tk(P, None, 1, 100, 8) == -1 and tk(P, P, 0, 100, 8) == -1
    rc = tk(P, P, 1, 100, 33)
    assert rc == -2 and b"k <= 32" in lib.rrt_strerror(rc)
    assert tk(P, P, 1, 7, 8) == -1 and tk(P, P, 1, 100, 0) == -1           # N < k -> invalid


def test_workspace_sizes_monotone(lib):
    n = C.c_size_t()

    def ws(N, K, H=256, D=512):
        assert lib.rrt_branch_pool_workspace_size(N, D, H, K, C.byref(n)) == 0
        return n.value
    sizes_n = [ws(N, 3) for N in (1, 31, 32, 33, 1000, 9000, 100000)]
    assert sizes_n == sorted(sizes_n) and sizes_n[0] > 0 and sizes_n[-1] > sizes_n[0]
    sizes_k = [ws(1000, K) for K in range(1, 9)]
    assert sizes_k == sorted(sizes_k) and sizes_k[-1] > sizes_k[0]
    # forward partials: K * dim + 16 floats per 32-token chunk; backward partials: K * hidden + 8 per 32 tokens
    assert ws(1000, 8) >= 32 * (8 * 512 + 16) * 4 and ws(1000, 8, H=1024, D=64) >= 32 * (8 * 1024 + 8) * 4

    def cws(model, N):
        d, _w, _k = model._desc_weights(128, True)
        assert lib.rrt_clam_workspace_size(C.byref(d), N, C.byref(n)) == 0
        return n.value
    sb, mb = CLAM_SB(128, rrt=RRTEncoder()), CLAM_MB(128, n_classes=4, rrt=RRTEncoder())
    a = [cws(sb, N) for N in (10, 100, 1000, 9000)]
    assert a == sorted(a) and cws(mb, 1000) > cws(sb, 1000) > cws(CLAM_SB(128), 1000)
    d, w, _k = mb._desc_weights(128, True)
    assert lib.rrt_clam_forward_f32(C.byref(d), C.byref(w), None, P, None, None, None, None, 100, P, 0, None) == -1
    assert lib.rrt_clam_workspace_size(C.byref(d), 0, C.byref(n)) == -1
    d.n_classes = 9
    rc = lib.rrt_clam_workspace_size(C.byref(d), 100, C.byref(n))
    assert rc == -2 and b"n_classes" in lib.rrt_strerror(rc)


def test_state_dict_surface_every_combination():
    """keys, order and shapes of state_dict() equal the reference's for every kind x dropout x rrt x gate combination (the
    indices inside attention_net shift with dropout / rrt); instance_loss_fn.labels included"""
    combos = load_golden("clam_keys")["cfg"]["combos"]
    assert len(combos) == 16
    for c in combos:
        cls = CLAM_SB if c["kind"] == "sb" else CLAM_MB
        m = cls(c["input_dim"], gate=c["gate"], size_arg=c["size_arg"], dropout=c["dropout"], n_classes=c["n_classes"],
                rrt=RRTEncoder(**c["enc"]) if c["rrt"] else None)
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == c["keys"], (c["kind"], c["dropout"], c["rrt"], c["gate"])
        assert any(k == "instance_loss_fn.labels" for k, _ in got)


def _state(g):
    cfg = g["cfg"]
    pre = cfg["rrt_prefix"]
    shapes = {k: tuple(s) for k, s in cfg["ref_keys"] if not k.startswith(pre)}
    st = synth.clam_head_state(shapes, cfg["name"])
    st.update({pre + k: v for k, v in synth.encoder_state(**{k: v for k, v in cfg["enc"].items() if k != "region_num"}).items()})
    return {k: torch.from_numpy(np.array(v)) for k, v in st.items()}


@pytest.mark.parametrize("name", CASES)
def test_golden_state_loads_strict(name):
    g = load_golden(name)
    cfg = g["cfg"]
    cls = CLAM_SB if cfg["kind"] == "sb" else CLAM_MB
    m = cls(cfg["input_dim"], gate=cfg["gate"], size_arg=cfg["size_arg"], k_sample=cfg["k_sample"], n_classes=cfg["n_classes"],
            subtyping=cfg["subtyping"], rrt=RRTEncoder(drop_out=0., **cfg["enc"]))
    sd = _state(g)
    assert set(sd) == {k for k, _ in cfg["ref_keys"]} and [[k, list(v.shape)] for k, v in m.state_dict().items()] == cfg["ref_keys"]
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.instance_loss_fn.labels, torch.arange(2))


@pytest.mark.parametrize("name", CASES)
def test_svm_loss_matches_reference(name):
    """our smooth top-1 SVM on the reference's instance logits (float64) gives the reference's instance loss: one call per
    evaluated branch, summed, divided by n_classes with subtyping (clam.py:184-201)"""
    g = load_golden(name)
    cfg, k = g["cfg"], g["cfg"]["k_sample"]
    x, y = torch.from_numpy(g["inst_logits"]).double(), torch.from_numpy(g["inst_targets"])
    fn, total, o = SmoothTop1SVM(2).double(), 0.0, 0
    for _row, both, _i in cfg["branches"]:
        rows = 2 * k if both else k
        total = total + fn(x[o:o + rows], y[o:o + rows])
        o += rows
    assert o == x.shape[0]
    if cfg["subtyping"]:
        total = total / cfg["n_classes"]
    assert abs(float(total) - float(g["inst_loss"])) <= 1e-12 * max(1.0, abs(float(g["inst_loss"])))


def test_svm_loss_hard_branch():
    """rows whose top-2 gap reaches tau ln(1000) take the hard form max_j(x_j + [j != y]) - x_y; the others the smooth one"""
    g = load_golden(CASES[0])
    x = torch.from_numpy(g["inst_logits"]).double()[:6].clone()
    y = torch.from_numpy(g["inst_targets"])[:6]
    x[0] = x[0] * (2 * np.log(1000.0) / float((x[0, 0] - x[0, 1]).abs()))        # scaled: gap = 2 ln 1000 -> hard
    x[1] = torch.tensor([0.0, np.log(1000.0)])                                    # exactly at the threshold -> hard
    gap = (x[:, 0] - x[:, 1]).abs()
    hard = gap >= np.log(1000.0)
    assert hard[0] and hard[1] and not hard[2:].any()
    m = x + (y[:, None] != torch.arange(2)[None, :]).double()
    xy = x.gather(1, y[:, None]).squeeze(1)
    want = torch.where(hard, m.max(1)[0] - xy, torch.logsumexp(m - xy[:, None], 1)).mean()
    got = SmoothTop1SVM(2)(x, y)
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, float(want))
    assert abs(float(m.max(1)[0][0] - xy[0]) - float(torch.logsumexp(m - xy[:, None], 1)[0])) < 1e-3   # the smooth form's limit


def test_cpu_tensor_and_bad_rrt_raise():
    m = CLAM_SB(64).eval()
    with pytest.raises(_lib.RRTHipError):
        m(torch.zeros(1, 10, 64))
    with pytest.raises(_lib.RRTHipError):
        m.forward_bag(torch.zeros(10, 64))
    with pytest.raises(_lib.RRTHipError):
        CLAM_MB(64).forward_bags([torch.zeros(10, 64)])
    with pytest.raises(TypeError):
        CLAM_SB(64, rrt=torch.nn.Identity())
    with pytest.raises(ValueError):
        CLAM_MB(64, rrt=RRTEncoder(mlp_dim=256))
