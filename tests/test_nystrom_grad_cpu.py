"""CPU: the C ABI surface and the argument checks of the Nystrom-attention backward, the ``enable_training`` switch, the float64
autograd of tests/nystrom_ref.py against the reference's own float64 gradients (tests/golden/transmil_grad.npz), and the case
lists of tests/test_nystrom_grad_gpu.py."""
import copy
import ctypes as C
import math
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nystrom_grad_cases as GC
import nystrom_ref as R
import transmil_cases as TC
from conftest import load_golden
from rrt_mil_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rrt_nystrom_train_sizes", "rrt_nystrom_attention_forward_train_f32", "rrt_nystrom_attention_backward_f32",
       "rrt_nystrom_output_backward_workspace_size", "rrt_nystrom_output_backward_f32", "rrt_nystrom_zav_backward_f32",
       "rrt_nystrom_landmark_attn_backward_workspace_size", "rrt_nystrom_landmark_attn_backward_f32",
       "rrt_nystrom_pinv_sim_backward_workspace_size", "rrt_nystrom_pinv_sim_backward_f32",
       "rrt_nystrom_landmarks_backward_f32")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x1000            # a non-NULL pointer no call may touch: every check happens before the first launch
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def why(lib):
    return lib.rrt_strerror(UNSUPPORTED).decode()


def desc(**kw):
    d = _lib.NystromDesc()
    d.dim, d.heads, d.dim_head, d.num_landmarks, d.pinv_iterations, d.residual, d.residual_conv_kernel = 512, 8, 64, 256, 6, 1, 33
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def four(cls, p=P):
    s = cls()
    s.qkv_w = s.out_w = s.out_b = s.conv_w = p
    return s


# ------------------------------------------------------------------ exports
def test_exports(lib):
    hdr = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert "#define RRT_ABI_VERSION 29" in hdr and lib.rrt_abi_version() == 29 and _lib.ABI_VERSION == 29
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rrt_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    body = re.search(r"typedef struct rrt_nystrom_grads \{(.*?)\} rrt_nystrom_grads;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*?(\w+)\s*[;,]", body)) == ("qkv_w", "out_w", "out_b", "conv_w")
    assert [n for n, _ in _lib.NystromGrads._fields_] == ["qkv_w", "out_w", "out_b", "conv_w"]
    build = __import__("rrt_mil_amd.build", fromlist=["SOURCES"])
    assert "nystrom_bwd.hip" in build.SOURCES and not build.PACKED_FP32_OK
    for s in GC.STAGES:
        assert "rrt_nystrom_%s_backward_f32" % s in NEW


# ------------------------------------------------------------------ argument checks (nothing is launched: no device needed)
@pytest.mark.parametrize("kw,word", [(dict(dim_head=32), "dim_head"), (dict(num_landmarks=128), "num_landmarks"),
                                     (dict(residual_conv_kernel=32), "residual_conv_kernel"), (dict(heads=17), "heads"),
                                     (dict(dim=48), "dim"), (dict(pinv_iterations=17), "pinv_iterations")],
                         ids=lambda v: str(v))
def test_unsupported_fields_are_named(lib, kw, word):
    a, b = C.c_size_t(), C.c_size_t()
    d, w, g = desc(**kw), four(_lib.NystromWeights), four(_lib.NystromGrads)
    assert lib.rrt_nystrom_train_sizes(C.byref(d), 1000, C.byref(a), C.byref(b)) == UNSUPPORTED and word in why(lib)
    assert lib.rrt_nystrom_attention_forward_train_f32(C.byref(d), C.byref(w), P, P, 1000, P, BIG, None) == UNSUPPORTED
    assert word in why(lib)
    assert lib.rrt_nystrom_attention_backward_f32(C.byref(d), C.byref(w), P, P, P, BIG, C.byref(g), P, 1000, P, BIG,
                                                  None) == UNSUPPORTED
    assert word in why(lib)


def test_null_pointers_and_bad_sizes(lib):
    a, b = C.c_size_t(), C.c_size_t()
    d, w, g = desc(), four(_lib.NystromWeights), four(_lib.NystromGrads)
    assert lib.rrt_nystrom_train_sizes(None, 10, C.byref(a), C.byref(b)) == INVALID
    assert lib.rrt_nystrom_train_sizes(C.byref(d), 10, None, C.byref(b)) == INVALID
    assert lib.rrt_nystrom_train_sizes(C.byref(d), 10, C.byref(a), None) == INVALID
    assert lib.rrt_nystrom_train_sizes(C.byref(d), 0, C.byref(a), C.byref(b)) == INVALID
    assert lib.rrt_nystrom_train_sizes(C.byref(d), 1000001, C.byref(a), C.byref(b)) == UNSUPPORTED and "n above 1e6" in why(lib)
    for args in ((None, C.byref(w), P, P, 10), (C.byref(d), None, P, P, 10), (C.byref(d), C.byref(w), None, P, 10),
                 (C.byref(d), C.byref(w), P, None, 10), (C.byref(d), C.byref(w), P, P, 0),
                 (C.byref(d), C.byref(four(_lib.NystromWeights, None)), P, P, 10)):
        assert lib.rrt_nystrom_attention_forward_train_f32(*args, P, BIG, None) == INVALID, args
    bw = lib.rrt_nystrom_attention_backward_f32
    assert bw(None, C.byref(w), P, P, P, BIG, C.byref(g), P, 10, P, BIG, None) == INVALID
    assert bw(C.byref(d), C.byref(w), None, P, P, BIG, C.byref(g), P, 10, P, BIG, None) == INVALID
    assert bw(C.byref(d), C.byref(w), P, None, P, BIG, C.byref(g), P, 10, P, BIG, None) == INVALID
    assert bw(C.byref(d), C.byref(w), P, P, P, BIG, None, P, 10, P, BIG, None) == INVALID
    assert bw(C.byref(d), C.byref(w), P, P, P, BIG, C.byref(four(_lib.NystromGrads, None)), P, 10, P, BIG, None) == INVALID
    noconv = four(_lib.NystromGrads)
    noconv.conv_w = None
    assert bw(C.byref(d), C.byref(w), P, P, P, BIG, C.byref(noconv), P, 10, P, BIG, None) == INVALID
    # residual = 0: conv_w is unused; dx is optional: both reach the workspace check
    assert bw(C.byref(desc(residual=0)), C.byref(w), P, P, P, BIG, C.byref(noconv), None, 10, None, 0, None) == WORKSPACE
    assert bw(C.byref(d), C.byref(w), P, P, None, BIG, C.byref(g), P, 10, P, BIG, None) == WORKSPACE
    for heads in (0, 17):
        assert lib.rrt_nystrom_output_backward_workspace_size(256, heads, C.byref(a)) == UNSUPPORTED and "heads" in why(lib)
        assert lib.rrt_nystrom_output_backward_f32(*[P] * 9, 256, heads, 33, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_zav_backward_f32(*[P] * 5, heads, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmark_attn_backward_workspace_size(256, heads, C.byref(a)) == UNSUPPORTED
        assert lib.rrt_nystrom_landmark_attn_backward_f32(*[P] * 5, 256, heads, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_pinv_sim_backward_workspace_size(heads, 6, C.byref(a)) == UNSUPPORTED
        assert lib.rrt_nystrom_pinv_sim_backward_f32(*[P] * 5, heads, 6, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmarks_backward_f32(*[P] * 3, 256, heads, None) == UNSUPPORTED
    for bad in (1000448, 100):                               # beyond 1e6 rounded up; not a multiple of 256
        assert lib.rrt_nystrom_output_backward_workspace_size(bad, 8, C.byref(a)) == UNSUPPORTED
        assert lib.rrt_nystrom_output_backward_f32(*[P] * 9, bad, 8, 33, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmark_attn_backward_f32(*[P] * 5, bad, 8, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmarks_backward_f32(*[P] * 3, bad, 8, None) == UNSUPPORTED
    assert lib.rrt_nystrom_output_backward_f32(*[P] * 9, 256, 8, 32, P, BIG, None) == UNSUPPORTED
    assert "residual_conv_kernel" in why(lib)
    for it in (0, 17):
        assert lib.rrt_nystrom_pinv_sim_backward_workspace_size(8, it, C.byref(a)) == UNSUPPORTED and "pinv_iterations" in why(lib)
        assert lib.rrt_nystrom_pinv_sim_backward_f32(*[P] * 5, 8, it, P, BIG, None) == UNSUPPORTED
    for i in (0, 1, 2, 4, 5, 6, 7):                          # conv_w (3) may be NULL; then d_conv_w (8) may be too
        args = [P] * 9
        args[i] = None
        assert lib.rrt_nystrom_output_backward_f32(*args, 256, 8, 33, P, BIG, None) == INVALID, i
    args = [P] * 9
    args[8] = None
    assert lib.rrt_nystrom_output_backward_f32(*args, 256, 8, 33, P, BIG, None) == INVALID
    args[3] = None
    assert lib.rrt_nystrom_output_backward_f32(*args, 256, 8, 33, None, 0, None) == WORKSPACE
    for fn, extra in ((lib.rrt_nystrom_zav_backward_f32, (8, None)),
                      (lib.rrt_nystrom_landmark_attn_backward_f32, (256, 8, P, BIG, None)),
                      (lib.rrt_nystrom_pinv_sim_backward_f32, (8, 6, P, BIG, None))):
        for i in range(5):
            args = [P] * 5
            args[i] = None
            assert fn(*args, *extra) == INVALID, (fn.__name__, i)
    for i in range(3):
        args = [P] * 3
        args[i] = None
        assert lib.rrt_nystrom_landmarks_backward_f32(*args, 256, 8, None) == INVALID
    assert lib.rrt_nystrom_landmarks_backward_f32(P, P, P, 0, 8, None) == INVALID
    for fn, args in ((lib.rrt_nystrom_output_backward_workspace_size, (256, 8)),
                     (lib.rrt_nystrom_landmark_attn_backward_workspace_size, (256, 8)),
                     (lib.rrt_nystrom_pinv_sim_backward_workspace_size, (8, 6))):
        assert fn(*args, None) == INVALID


def test_short_workspaces_and_stashes(lib):
    a, b, need = C.c_size_t(), C.c_size_t(), C.c_size_t()
    w, g = four(_lib.NystromWeights), four(_lib.NystromGrads)
    for kw in (dict(), dict(dim=128, heads=2), dict(residual=0), dict(pinv_iterations=1)):
        d = desc(**kw)
        prev = (0, 0)
        for n in (1, 256, 257, 2600, 9000):
            assert lib.rrt_nystrom_train_sizes(C.byref(d), n, C.byref(a), C.byref(b)) == 0 and a.value > 0 and b.value > 0
            assert a.value % 256 == 0 and b.value % 256 == 0 and a.value >= prev[0] and b.value >= prev[1]
            prev = (a.value, b.value)
            lib.rrt_nystrom_workspace_size(C.byref(d), n, C.byref(need))
            assert a.value >= need.value                       # the stash holds the forward's stage tensors
            fw, bw = lib.rrt_nystrom_attention_forward_train_f32, lib.rrt_nystrom_attention_backward_f32
            assert fw(C.byref(d), C.byref(w), P, P, n, P, a.value - 1, None) == WORKSPACE
            assert fw(C.byref(d), C.byref(w), P, P, n, None, a.value, None) == WORKSPACE
            assert bw(C.byref(d), C.byref(w), P, P, P, a.value - 1, C.byref(g), P, n, P, b.value, None) == WORKSPACE
            assert bw(C.byref(d), C.byref(w), P, P, P, a.value, C.byref(g), P, n, P, b.value - 1, None) == WORKSPACE
            assert bw(C.byref(d), C.byref(w), P, P, P, a.value, C.byref(g), P, n, None, b.value, None) == WORKSPACE
    # the stash at N = 9000 x 512, eight heads (DESIGN.md states it): qkv 56.6 MB + o 18.9 MB + the landmark tensors
    lib.rrt_nystrom_train_sizes(C.byref(desc()), 9000, C.byref(a), C.byref(b))
    assert 75e6 < a.value < 110e6
    for npad in (256, 2816):
        assert lib.rrt_nystrom_output_backward_workspace_size(npad, 8, C.byref(need)) == 0 and need.value > 0
        assert lib.rrt_nystrom_output_backward_f32(*[P] * 9, npad, 8, 33, P, need.value - 1, None) == WORKSPACE
        assert lib.rrt_nystrom_landmark_attn_backward_workspace_size(npad, 8, C.byref(need)) == 0 and need.value > 0
        assert lib.rrt_nystrom_landmark_attn_backward_f32(*[P] * 5, npad, 8, P, need.value - 1, None) == WORKSPACE
        assert lib.rrt_nystrom_landmark_attn_backward_f32(*[P] * 5, npad, 8, None, need.value, None) == WORKSPACE
    for it in GC.PINV_ITERATIONS:
        assert lib.rrt_nystrom_pinv_sim_backward_workspace_size(8, it, C.byref(need)) == 0
        assert need.value >= (it + 11) * 8 * 256 * 256 * 4      # every iterate is kept, plus a2 and ten matrices of scratch
        assert lib.rrt_nystrom_pinv_sim_backward_f32(*[P] * 5, 8, it, P, need.value - 1, None) == WORKSPACE


# ------------------------------------------------------------------ enable_training, without a device
def test_enable_training_switch():
    from rrt_mil_amd import NystromAttention, TransMIL
    attn, model = NystromAttention(128, heads=2), TransMIL(64, 2, True, "gelu")
    assert attn._train_enabled is False and model._train_enabled is False
    keys_a, keys_m = list(attn.state_dict()), list(model.state_dict())
    assert attn.enable_training() is attn and model.enable_training() is model
    assert attn._train_enabled and model._train_enabled and model.layer1.attn._train_enabled and model.layer2.attn._train_enabled
    assert list(attn.state_dict()) == keys_a and list(model.state_dict()) == keys_m and len(keys_m) == 25
    for clone in (pickle.loads(pickle.dumps(model)), copy.deepcopy(model)):
        assert clone._train_enabled and clone.layer1.attn._train_enabled and clone.layer2.attn._train_enabled
    assert pickle.loads(pickle.dumps(attn))._train_enabled and copy.deepcopy(attn)._train_enabled
    fresh = TransMIL(64, 2, True, "gelu")
    fresh.load_state_dict(model.state_dict(), strict=True)
    assert fresh._train_enabled is False                         # not part of the state_dict
    assert model.enable_training(False) is model and not model._train_enabled and not model.layer2.attn._train_enabled
    # on or off, there is no CPU path, and mask= / return_attn=True keep raising
    attn.enable_training()
    with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
        attn(torch.zeros(1, 10, 128, requires_grad=True))
    with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
        model.enable_training()(torch.zeros(1, 10, 64))
    with pytest.raises(NotImplementedError, match="mask"):
        attn(torch.zeros(1, 10, 128), mask=torch.ones(1, 10, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="return_attn"):
        attn(torch.zeros(1, 10, 128), return_attn=True)


# ------------------------------------------------------------------ the restatement's autograd against the reference's gradients
def attention_grads64(dim, heads, n, gain):
    state, x = TC.attn_inputs(dim, heads, n, gain)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).double().requires_grad_(True)
    dy = torch.from_numpy(GC.cotangent(f"dy/{GC.case_key(dim, heads, n, gain)}", (n, dim))).double()
    (R.nystrom(xd, p, heads, dtype=torch.float64)["y"] * dy).sum().backward()
    return {**{k: v.grad for k, v in p.items()}, "dx": xd.grad}


def model_grads64(input_dim, act, N):
    state, x = TC.model_inputs(input_dim, N)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).double().requires_grad_(True)
    logits = R.transmil(xd, p, act, dtype=torch.float64)["logits"]
    F.cross_entropy(logits[None], torch.tensor([GC.LABEL])).backward()
    return {**{k: v.grad for k, v in p.items()}, "dx": xd.grad}


def against_golden(gold, key, grads):
    seen = 0
    for name, g in grads.items():
        ref = gold[f"{key}/{name}"]
        rows = torch.stack([g[0], g[-1]]) if name == "dx" else GC.golden_rows(g)
        assert rows.shape == ref.shape, (key, name, rows.shape, ref.shape)
        assert np.abs(ref).max() > 0, (key, name)
        err = GC.rel_grad(rows.numpy(), ref)
        assert err <= 1e-9, (key, name, err)
        assert f"{key}/e32/{name}" in gold
        seen += 1
    return seen


@pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad")
@pytest.mark.parametrize("dim,heads,n,gain", GC.GOLDEN_ATTN_CASES, ids=lambda v: str(v))
def test_restatement_autograd_reproduces_the_reference_attention_gradients(dim, heads, n, gain):
    assert against_golden(load_golden("transmil_grad"), "attn/" + GC.case_key(dim, heads, n, gain),
                          attention_grads64(dim, heads, n, gain)) == 5


@pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad")
@pytest.mark.parametrize("input_dim,act,N", GC.GOLDEN_MODEL_CASES, ids=lambda v: str(v))
def test_restatement_autograd_reproduces_the_reference_model_gradients(input_dim, act, N):
    assert against_golden(load_golden("transmil_grad"), "model/" + GC.model_key(input_dim, act, N),
                          model_grads64(input_dim, act, N)) == 26


# ------------------------------------------------------------------ the GPU file's case lists cover what they claim
def test_case_lists_cover_what_the_gpu_file_claims():
    assert set(GC.LENGTHS) == {2, 17, 255, 256, 257, 513, 1030, 2600} and GC.GAINS == (1.0, 6.0)
    for n in GC.LENGTHS:
        for g in GC.GAINS:
            assert (128, 2, n, g) in GC.STAGE_CASES
    assert (512, 8, 257, 6.0) in GC.STAGE_CASES and (512, 8, 2600, 6.0) in GC.STAGE_CASES
    assert len(GC.STAGE_CASES) == len(set(GC.STAGE_CASES)) == 18
    assert GC.PINV_ITERATIONS == (1, 6) and GC.RESIDUAL == (True, False)
    pad, l = TC.pad_of, lambda n: math.ceil(n / 256)          # noqa: E731
    assert pad(2) + 16 >= 256 - 16 and pad(17) == 239 and pad(257) == 255 and l(257) == 2
    assert pad(257) % l(257) and pad(2600) % l(2600)             # a landmark that mixes pad rows and real rows
    assert pad(513) == 85 * l(513) and pad(1030) == 50 * l(1030)  # landmarks that are all pad, at l = 3 and l = 5
    assert (2600 + pad(2600)) // 64 > 32                        # more token tiles than chunk records: tiles share a block
    # n = 17: the 239 all-zero landmarks (the pad is in front) give column sums that are equal bit for bit; the largest
    # column sum is another, single column there -- the tie AT the maximum is test_pinv_den_gradient_with_tied_columns' case
    state, x = TC.attn_inputs(128, 2, 17, 6.0)
    cs = R.nystrom(x, state, 2, dtype=torch.float32)["a2"].sum(-2)
    assert bool((cs[:, :239] == cs[:, :1]).all()) and int((cs == cs.max()).sum()) == 1
    assert "def test_pinv_den_gradient_with_tied_columns" in open(os.path.join(ROOT, "tests", "test_nystrom_grad_gpu.py")).read()
    assert GC.MODEL_CASES == [(64, "gelu", n) for n in (1, 3, 10, 37, 250, 1000)] + [(1024, "relu", 1000)]
    for c in GC.GOLDEN_ATTN_CASES:
        assert c in GC.STAGE_CASES
    for c in GC.GOLDEN_MODEL_CASES:
        assert c in GC.MODEL_CASES
    assert len(GC.GOLDEN_ATTN_CASES) == 3 and len(GC.GOLDEN_MODEL_CASES) == 3
    src = open(os.path.join(ROOT, "tests", "test_nystrom_grad_gpu.py")).read()
    for s in GC.STAGES:
        assert "lib.rrt_nystrom_%s_backward_f32(" % s in src, s
    for name in ("rrt_nystrom_attention_forward_train_f32", "rrt_nystrom_attention_backward_f32", "enable_training"):
        assert name in src
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "transmil_grad.npz")) < 450_000
    # the cotangents are seeded: the same name gives the same array
    assert np.array_equal(GC.cotangent("x", (3, 4)), GC.cotangent("x", (3, 4)))
    assert synth.normal("nystrom_grad/x", (3, 4)).tobytes() == GC.cotangent("x", (3, 4)).tobytes()
