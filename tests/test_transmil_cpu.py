"""CPU: the C ABI surface, the argument checks and the Python surface of Nystrom attention / TransMIL, the float64 restatement
tests/nystrom_ref.py against the reference's goldens, and the case lists of tests/test_transmil_gpu.py."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import nystrom_ref as R
import transmil_cases as TC
from conftest import load_golden
from rrt_mil_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rrt_nystrom_workspace_size", "rrt_nystrom_attention_f32", "rrt_nystrom_landmarks_f32", "rrt_nystrom_landmark_sim_f32",
       "rrt_nystrom_landmark_attn_workspace_size", "rrt_nystrom_landmark_attn_f32", "rrt_nystrom_pinv_workspace_size",
       "rrt_nystrom_pinv_f32", "rrt_nystrom_zav_f32", "rrt_nystrom_output_f32", "rrt_ppeg_side_f32",
       "rrt_transmil_workspace_size", "rrt_transmil_forward_f32")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x1000            # a non-NULL pointer no call may touch: every check happens before the first launch


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def why(lib):
    return lib.rrt_strerror(UNSUPPORTED).decode()


def nystrom_desc(**kw):
    d = _lib.NystromDesc()
    d.dim, d.heads, d.dim_head, d.num_landmarks, d.pinv_iterations, d.residual, d.residual_conv_kernel = 512, 8, 64, 256, 6, 1, 33
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def nystrom_weights(p=P):
    w = _lib.NystromWeights()
    w.qkv_w = w.out_w = w.out_b = w.conv_w = p
    return w


def transmil_desc(**kw):
    d = _lib.TransmilDesc()
    d.input_dim, d.n_classes, d.act = 1024, 2, _lib.ACT_RELU
    d.attn = nystrom_desc(**{k: v for k, v in kw.items() if k in dict(_lib.NystromDesc._fields_)})
    for k, v in kw.items():
        if k in ("input_dim", "n_classes", "act"):
            setattr(d, k, v)
    return d


def transmil_weights(p=P):
    w = _lib.TransmilWeights()
    for name in ("fc1_w", "fc1_b", "cls_token", "norm_w", "norm_b", "fc2_w", "fc2_b"):
        setattr(w, name, p)
    for i in range(2):
        w.layer[i].norm_w = w.layer[i].norm_b = p
        w.layer[i].attn = nystrom_weights(p)
    for i in range(3):
        w.pos_w[i] = w.pos_b[i] = p
    return w


# ------------------------------------------------------------------ exports
def test_exports(lib):
    hdr = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert "#define RRT_ABI_VERSION 29" in hdr and lib.rrt_abi_version() == 29
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rrt_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    for struct, fields in (("rrt_nystrom_desc", ("dim", "heads", "dim_head", "num_landmarks", "pinv_iterations", "residual",
                                                 "residual_conv_kernel")),
                           ("rrt_nystrom_weights", ("qkv_w", "out_w", "out_b", "conv_w"))):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        assert tuple(re.findall(r"\*?(\w+)\s*[;,]", body)) == fields, (struct, body)
    assert [n for n, _ in _lib.NystromDesc._fields_] == ["dim", "heads", "dim_head", "num_landmarks", "pinv_iterations",
                                                         "residual", "residual_conv_kernel"]
    import rrt_mil_amd
    assert "TransMIL" in rrt_mil_amd.__all__ and "NystromAttention" in rrt_mil_amd.__all__
    assert "nystrom.hip" in __import__("rrt_mil_amd.build", fromlist=["SOURCES"]).SOURCES
    assert not __import__("rrt_mil_amd.build", fromlist=["PACKED_FP32_OK"]).PACKED_FP32_OK


# ------------------------------------------------------------------ argument checks (nothing is launched: no device needed)
UNSUPPORTED_FIELDS = [(dict(dim_head=32), "dim_head"), (dict(num_landmarks=128), "num_landmarks"),
                      (dict(residual_conv_kernel=32), "residual_conv_kernel"), (dict(residual_conv_kernel=65), "residual_conv_kernel"),
                      (dict(heads=17), "heads"), (dict(heads=0), "heads"), (dict(dim=48), "dim"), (dict(dim=1056), "dim"),
                      (dict(pinv_iterations=0), "pinv_iterations"), (dict(pinv_iterations=17), "pinv_iterations")]


@pytest.mark.parametrize("kw,word", UNSUPPORTED_FIELDS, ids=lambda v: str(v))
def test_unsupported_fields_are_named(lib, kw, word):
    need = C.c_size_t()
    d, w = nystrom_desc(**kw), nystrom_weights()
    assert lib.rrt_nystrom_workspace_size(C.byref(d), 1000, C.byref(need)) == UNSUPPORTED and word in why(lib)
    assert lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), P, P, 1000, P, 1 << 40, None) == UNSUPPORTED
    assert word in why(lib)
    t, tw = transmil_desc(**kw), transmil_weights()
    assert lib.rrt_transmil_workspace_size(C.byref(t), 1000, C.byref(need)) == UNSUPPORTED and word in why(lib)
    assert lib.rrt_transmil_forward_f32(C.byref(t), C.byref(tw), P, P, None, 1000, P, 1 << 40, None) == UNSUPPORTED
    assert word in why(lib)


def test_n_above_a_million_is_unsupported(lib):
    need = C.c_size_t()
    d, w = nystrom_desc(), nystrom_weights()
    assert lib.rrt_nystrom_workspace_size(C.byref(d), 1000000, C.byref(need)) == 0
    assert lib.rrt_nystrom_workspace_size(C.byref(d), 1000001, C.byref(need)) == UNSUPPORTED and "n above 1e6" in why(lib)
    assert lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), P, P, 1000001, P, 1 << 40, None) == UNSUPPORTED
    t, tw = transmil_desc(), transmil_weights()
    assert lib.rrt_transmil_workspace_size(C.byref(t), 1000001, C.byref(need)) == UNSUPPORTED and "n_tokens" in why(lib)
    assert lib.rrt_transmil_forward_f32(C.byref(t), C.byref(tw), P, P, None, 1000001, P, 1 << 40, None) == UNSUPPORTED
    for bad in (1000448, 100):                               # stage entry points: beyond 1e6 rounded up; not a multiple of 256
        assert lib.rrt_nystrom_landmarks_f32(P, P, P, bad, 8, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmark_attn_workspace_size(bad, 8, C.byref(need)) == UNSUPPORTED
        assert lib.rrt_nystrom_landmark_attn_f32(P, P, P, bad, 8, P, 1 << 40, None) == UNSUPPORTED
        assert lib.rrt_nystrom_output_f32(P, P, P, P, P, bad, 8, 33, None) == UNSUPPORTED
    for kw, word in ((dict(input_dim=48), "input_dim"), (dict(n_classes=0), "n_classes"), (dict(act=_lib.ACT_TANH), "act")):
        t = transmil_desc(**kw)
        assert lib.rrt_transmil_workspace_size(C.byref(t), 100, C.byref(need)) == UNSUPPORTED and word in why(lib)


def test_null_and_non_positive_sizes(lib):
    need = C.c_size_t()
    d, w, t, tw = nystrom_desc(), nystrom_weights(), transmil_desc(), transmil_weights()
    assert lib.rrt_nystrom_workspace_size(None, 10, C.byref(need)) == INVALID
    assert lib.rrt_nystrom_workspace_size(C.byref(d), 10, None) == INVALID
    assert lib.rrt_nystrom_workspace_size(C.byref(d), 0, C.byref(need)) == INVALID
    for args in ((None, C.byref(w), P, P, 10), (C.byref(d), None, P, P, 10), (C.byref(d), C.byref(w), None, P, 10),
                 (C.byref(d), C.byref(w), P, None, 10), (C.byref(d), C.byref(w), P, P, 0), (C.byref(d), C.byref(w), P, P, -5),
                 (C.byref(d), C.byref(nystrom_weights(None)), P, P, 10)):
        assert lib.rrt_nystrom_attention_f32(*args, P, 1 << 40, None) == INVALID, args
    nores = nystrom_weights()
    nores.conv_w = None
    assert lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(nores), P, P, 10, P, 1 << 40, None) == INVALID
    assert lib.rrt_nystrom_attention_f32(C.byref(nystrom_desc(residual=0)), C.byref(nores), P, P, 10, None, 0, None) == WORKSPACE
    for heads in (0, 17):
        assert lib.rrt_nystrom_landmarks_f32(P, P, P, 256, heads, None) == UNSUPPORTED and "heads" in why(lib)
        assert lib.rrt_nystrom_landmark_sim_f32(P, P, P, heads, None) == UNSUPPORTED
        assert lib.rrt_nystrom_pinv_workspace_size(heads, C.byref(need)) == UNSUPPORTED
        assert lib.rrt_nystrom_pinv_f32(P, P, heads, 6, P, 1 << 40, None) == UNSUPPORTED
        assert lib.rrt_nystrom_zav_f32(P, P, P, heads, None) == UNSUPPORTED
    assert lib.rrt_nystrom_landmarks_f32(None, P, P, 256, 8, None) == INVALID
    assert lib.rrt_nystrom_landmarks_f32(P, P, None, 256, 8, None) == INVALID
    assert lib.rrt_nystrom_landmarks_f32(P, P, P, 0, 8, None) == INVALID
    assert lib.rrt_nystrom_landmark_sim_f32(P, None, P, 8, None) == INVALID
    assert lib.rrt_nystrom_landmark_attn_workspace_size(256, 8, None) == INVALID
    assert lib.rrt_nystrom_landmark_attn_f32(P, None, P, 256, 8, P, 1 << 40, None) == INVALID
    assert lib.rrt_nystrom_pinv_workspace_size(8, None) == INVALID
    assert lib.rrt_nystrom_pinv_f32(None, P, 8, 6, P, 1 << 40, None) == INVALID
    assert lib.rrt_nystrom_pinv_f32(P, P, 8, 0, P, 1 << 40, None) == UNSUPPORTED and "pinv_iterations" in why(lib)
    assert lib.rrt_nystrom_zav_f32(P, P, None, 8, None) == INVALID
    assert lib.rrt_nystrom_output_f32(P, P, None, P, P, 256, 8, 33, None) == INVALID
    assert lib.rrt_nystrom_output_f32(P, P, P, P, P, 256, 8, 32, None) == UNSUPPORTED and "residual_conv_kernel" in why(lib)
    three = (C.c_void_p * 3)(P, P, P)
    assert lib.rrt_ppeg_side_f32(None, three, three, P, 4, 64, None) == INVALID
    assert lib.rrt_ppeg_side_f32(P, None, three, P, 4, 64, None) == INVALID
    assert lib.rrt_ppeg_side_f32(P, (C.c_void_p * 3)(P, None, P), three, P, 4, 64, None) == INVALID
    assert lib.rrt_ppeg_side_f32(P, three, three, P, 0, 64, None) == INVALID
    assert lib.rrt_ppeg_side_f32(P, three, three, P, 4, 66, None) == UNSUPPORTED and "dim" in why(lib)
    assert lib.rrt_ppeg_side_f32(P, three, three, P, 1001, 64, None) == UNSUPPORTED and "side" in why(lib)
    assert lib.rrt_transmil_workspace_size(None, 10, C.byref(need)) == INVALID
    assert lib.rrt_transmil_workspace_size(C.byref(t), 0, C.byref(need)) == INVALID
    for args in ((None, C.byref(tw), P, P), (C.byref(t), None, P, P), (C.byref(t), C.byref(tw), None, P),
                 (C.byref(t), C.byref(tw), P, None), (C.byref(t), C.byref(transmil_weights(None)), P, P)):
        assert lib.rrt_transmil_forward_f32(*args, None, 10, P, 1 << 40, None) == INVALID, args
    assert lib.rrt_transmil_forward_f32(C.byref(t), C.byref(tw), P, P, None, 0, P, 1 << 40, None) == INVALID


def test_short_workspaces(lib):
    need = C.c_size_t()
    d, w, t, tw = nystrom_desc(), nystrom_weights(), transmil_desc(), transmil_weights()
    for n in (1, 256, 2600):
        assert lib.rrt_nystrom_workspace_size(C.byref(d), n, C.byref(need)) == 0 and need.value > 0
        assert lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), P, P, n, P, need.value - 1, None) == WORKSPACE
        assert lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), P, P, n, None, need.value, None) == WORKSPACE
        assert lib.rrt_transmil_workspace_size(C.byref(t), n, C.byref(need)) == 0
        assert lib.rrt_transmil_forward_f32(C.byref(t), C.byref(tw), P, P, None, n, P, need.value - 1, None) == WORKSPACE
        npad = (n + 255) // 256 * 256
        assert lib.rrt_nystrom_landmark_attn_workspace_size(npad, 8, C.byref(need)) == 0
        assert lib.rrt_nystrom_landmark_attn_f32(P, P, P, npad, 8, P, need.value - 1, None) == WORKSPACE
    assert lib.rrt_nystrom_pinv_workspace_size(8, C.byref(need)) == 0
    assert lib.rrt_nystrom_pinv_f32(P, P, 8, 6, P, need.value - 1, None) == WORKSPACE
    assert lib.rrt_nystrom_pinv_f32(P, P, 8, 6, None, need.value, None) == WORKSPACE


_WORKSPACE_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from rrt_mil_amd import _lib
import test_transmil_cpu as T
lib = _lib.load()
n_dev = C.c_int(-1)
C.CDLL(_lib.LIB_PATH).hipGetDeviceCount(C.byref(n_dev))
if n_dev.value != 0 or torch.cuda.device_count() != 0:
    sys.exit(f"a GPU is visible ({n_dev.value} devices): the host-pointer forward calls must not run")
keep = torch.zeros(4096)
for kw in (dict(), dict(dim=128, heads=2), dict(heads=16, dim=1024), dict(residual=0), dict(pinv_iterations=1)):
    for n in (1, 17, 256, 257, 2600, 9217):
        d, w = T.nystrom_desc(**kw), T.nystrom_weights(keep.data_ptr())
        need = C.c_size_t()
        assert lib.rrt_nystrom_workspace_size(C.byref(d), n, C.byref(need)) == 0
        buf = (C.c_char * need.value)()
        x, y = torch.zeros(n, d.dim), torch.zeros(n, d.dim)
        rc = lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), x.data_ptr(), y.data_ptr(), n, C.addressof(buf), need.value, None)
        assert rc > 0, (kw, n, rc)
        assert lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), x.data_ptr(), y.data_ptr(), n, C.addressof(buf),
                                             need.value - 1, None) == -3
for kw in (dict(input_dim=64), dict(input_dim=1024)):
    for n in (1, 10, 250, 2500):
        t, tw = T.transmil_desc(**kw), T.transmil_weights(keep.data_ptr())
        need = C.c_size_t()
        assert lib.rrt_transmil_workspace_size(C.byref(t), n, C.byref(need)) == 0
        buf = (C.c_char * need.value)()
        x, lg = torch.zeros(n, t.input_dim), torch.zeros(2)
        rc = lib.rrt_transmil_forward_f32(C.byref(t), C.byref(tw), x.data_ptr(), lg.data_ptr(), None, n, C.addressof(buf),
                                          need.value, None)
        assert rc > 0, (kw, n, rc)
        assert lib.rrt_transmil_forward_f32(C.byref(t), C.byref(tw), x.data_ptr(), lg.data_ptr(), None, n, C.addressof(buf),
                                            need.value - 1, None) == -3
print("workspace checks ok")
"""


def test_workspace_queries_cover_what_the_forwards_check():
    """The size a query returns is the size the forward checks against.  No GPU in the child that makes the host-pointer calls:
    a call that passes validation fails at its first launch with a HIP error (> 0); a sizing bug shows up as RRT_E_WORKSPACE
    (-3) before anything is launched."""
    out = subprocess.run([sys.executable, "-c", _WORKSPACE_CHILD, ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0 and "workspace checks ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ------------------------------------------------------------------ the Python surface
def test_constructor_signatures_and_state_dict_surface():
    from rrt_mil_amd import NystromAttention, TransMIL
    keys = load_golden("transmil_keys")["cfg"]

    def sig(cls):
        return [[n, None if p.default is inspect.Parameter.empty else p.default]
                for n, p in list(inspect.signature(cls.__init__).parameters.items())[1:]]

    assert sig(TransMIL) == keys["transmil_signature"]
    assert sig(NystromAttention) == keys["nystrom_signature"]
    model = TransMIL(1024, 2, False, "relu")
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == keys["transmil"] and len(keys["transmil"]) == 25
    attn = NystromAttention(512)
    assert [[k, list(v.shape)] for k, v in attn.state_dict().items()] == keys["nystrom"]
    for dropout, act in ((True, "gelu"), (False, "none")):          # Dropout / no activation add no keys
        assert list(TransMIL(1024, 2, dropout, act).state_dict()) == [k for k, _ in keys["transmil"]]
    state = synth.transmil_state(1024, 2)
    assert sorted([k, list(v.shape)] for k, v in state.items()) == sorted(keys["transmil"])
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    nstate = synth.nystrom_state(512, 8)
    attn.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in nstate.items()}, strict=True)
    # initialize_weights + the tiny cls token
    fresh = TransMIL(64, 3, False, "relu")
    assert float(fresh.cls_token.detach().abs().max()) < 1e-4 and float(fresh._fc1[0].bias.abs().max()) == 0.0
    assert bool((fresh.norm.weight == 1).all()) and fresh._fc2.weight.shape == (3, 512)
    assert float(fresh.pos_layer.proj.bias.abs().max()) == 0.0
    import copy
    import pickle
    assert torch.equal(pickle.loads(pickle.dumps(fresh))._fc2.weight, fresh._fc2.weight)
    copy.deepcopy(fresh)


def test_what_must_raise_on_the_cpu():
    from rrt_mil_amd import NystromAttention, TransMIL
    model, attn = TransMIL(64, 2, False, "relu").eval(), NystromAttention(128, heads=2).eval()
    with torch.no_grad():
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            model(torch.zeros(1, 10, 64))
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            model.forward_bag(torch.zeros(10, 64))
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            attn(torch.zeros(1, 10, 128))
        with pytest.raises(NotImplementedError, match="mask"):
            attn(torch.zeros(1, 10, 128), mask=torch.ones(1, 10, dtype=torch.bool))
        with pytest.raises(NotImplementedError, match="return_attn"):
            attn(torch.zeros(1, 10, 128), return_attn=True)


def test_encoder_ablations_still_raise_and_point_here():
    from rrt_mil_amd import RRTEncoder
    for kw in (dict(attn="ntrans"), dict(region_attn="ntrans")):
        with pytest.raises(NotImplementedError, match="NystromAttention"):
            RRTEncoder(mlp_dim=64, **kw)


# ------------------------------------------------------------------ the restatement against the reference's float64 goldens
def test_restatement_reproduces_the_reference_attention():
    gold, stages = load_golden("transmil_attn"), load_golden("transmil_stages")
    seen = 0
    for dim, heads, n, gain in TC.ATTN_CASES:
        state, x = TC.attn_inputs(dim, heads, n, gain)
        r = R.nystrom(x, state, heads, dtype=torch.float64)
        key = f"d{dim}_h{heads}_n{n}_g{int(gain)}"
        assert R.rel_err(torch.stack([r["y"][0], r["y"][-1]]), gold[key + "/y"]) <= 1e-12, key
        assert abs(r["peak"] - float(gold[key + "/peak"])) <= 1e-9 * max(1.0, r["peak"]), key
        assert float(gold[key + "/e32"]) <= 1e-5, key          # the reference itself stays well inside the stage rule
        if (dim, heads, n, gain) in TC.STAGE_GOLDEN_CASES:
            for name in ("ql", "kl", "a2", "av", "z", "wz"):
                assert R.rel_err(r[name][:, ::TC.STAGE_ROWS], stages[f"{key}/{name}"]) <= 1e-12, (key, name)
            assert R.rel_err(r["o"][-4:], stages[key + "/o"]) <= 1e-12, key
            seen += 1
    assert seen == len(TC.STAGE_GOLDEN_CASES)


@pytest.mark.parametrize("input_dim,act,N", TC.MODEL_CASES, ids=lambda v: str(v))
def test_restatement_reproduces_the_reference_model(input_dim, act, N):
    gold = load_golden("transmil_model")
    state, x = TC.model_inputs(input_dim, N)
    r = R.transmil(x, state, act, dtype=torch.float64)
    key = f"i{input_dim}_{act}_n{N}"
    assert R.rel_err(r["logits"], gold[key + "/logits"]) <= 1e-12
    f = r["feat"]
    H = math.isqrt(N - 1) + 1 if N > 1 else 1
    assert f.shape == (1 + H * H, 512)
    assert R.rel_err(torch.stack([f[0], f[1], f[-1]]), gold[key + "/feat"]) <= 1e-12
    assert float(gold[key + "/e32_logits"]) <= 1e-5 and float(gold[key + "/e32_feat"]) <= 1e-5


# ------------------------------------------------------------------ the GPU file's case lists cover what they claim
def test_case_lists_cover_what_the_gpu_file_claims():
    assert TC.CONFIGS == ((128, 2), (512, 8)) and TC.GAINS == (1.0, 6.0) and TC.PEAK_RANGE == (20.0, 80.0)
    table = {2: (1, 254), 17: (1, 239), 255: (1, 1), 256: (1, 0), 257: (2, 255), 512: (2, 0), 513: (3, 255),
             1030: (5, 250), 2600: (11, 216)}
    assert set(TC.LENGTHS) == set(table)
    for n, (l, pad) in table.items():
        assert math.ceil(n / 256) == l and TC.pad_of(n) == pad and 256 * l == n + pad
    assert len(TC.ATTN_CASES) == len(set(TC.ATTN_CASES)) == 2 * 9 * 2
    for cfg in TC.CONFIGS:
        for n in table:
            for gain in TC.GAINS:
                assert (*cfg, n, gain) in TC.ATTN_CASES
    pads = [TC.pad_of(n) for n in TC.LENGTHS]
    ls = {n: math.ceil(n / 256) for n in TC.LENGTHS}
    assert 0 in pads and any(p % 2 for p in pads)
    assert sum(1 for n in TC.LENGTHS if TC.pad_of(n) % ls[n]) >= 2           # a landmark that mixes pad rows and real rows
    assert any(TC.pad_of(n) >= 256 - 16 and n < 33 for n in TC.LENGTHS)      # the stencil window wider than the data
    assert max(TC.LENGTHS) + TC.pad_of(max(TC.LENGTHS)) > 2048               # several key chunks (32 chunks of 64 keys and up)
    assert TC.PINV_ITERATIONS == (1, 6)
    assert TC.STAGES == ("landmarks", "landmark_sim", "landmark_attn", "pinv", "zav", "output")
    for s in TC.STAGES:
        assert "rrt_nystrom_%s_f32" % s in NEW
    src = open(os.path.join(ROOT, "tests", "test_transmil_gpu.py")).read()
    for s in TC.STAGES:
        assert "lib.rrt_nystrom_%s_f32(" % s in src, s
    for c in TC.STAGE_GOLDEN_CASES:
        assert c in TC.ATTN_CASES
    want = [(64, "gelu", n) for n in (1, 3, 10, 36, 37, 250, 1000, 2500)] + [(1024, "relu", 1000)]
    assert TC.MODEL_CASES == want
    sides = {N: (math.isqrt(N - 1) + 1 if N > 1 else 1) for _, _, N in want}
    assert sides[1] == 1 and sides[3] ** 2 - 3 == 1 and sides[10] == 4 and sides[36] == 6 and sides[37] == 7
    assert 1 + sides[250] ** 2 == 257 and 1 + sides[2500] ** 2 == 2501
    gold, attn = load_golden("transmil_model"), load_golden("transmil_attn")
    for input_dim, act, N in want:
        assert f"i{input_dim}_{act}_n{N}/logits" in gold
    for dim, heads, n, gain in TC.ATTN_CASES:
        key = f"d{dim}_h{heads}_n{n}_g{int(gain)}"
        assert key + "/y" in attn
        if gain > 1:
            assert TC.PEAK_RANGE[0] <= float(attn[key + "/peak"]) <= TC.PEAK_RANGE[1], key
        else:
            assert float(attn[key + "/peak"]) < 5.0, key
    total = sum(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                if f.startswith("transmil_"))
    assert total < 1_000_000
    # the cls token of the model cases is of visible size
    assert 0.3 < float(np.std(TC.model_inputs(64, 3)[0]["cls_token"])) < 0.7
