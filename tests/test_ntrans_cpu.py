"""CPU: the Nystrom ablations of RRTEncoder (attn='ntrans', region_attn='ntrans') and the batched Nystrom attention under them.
The restatement tests/ntrans_ref.py is pinned to the reference's own float64 run (tests/golden/ntrans_*.npz, written by
tools/make_golden_ntrans.py); the fp32 error e32 of every case of tests/test_ntrans_gpu.py is small enough for its bound
max(2e-5, 8 x e32) to mean something; the ABI, the state-dict surface and everything that must raise without a device."""
import json
import re

import numpy as np
import pytest
import torch

import ntrans_cases as NC
import ntrans_ref as NR
from conftest import load_golden
from rrt_mil_amd import RRTEncoder, RRTMIL, NystromAttention, _lib

E32_MAX = 1e-4
NEW_EXPORTS = ["rrt_nystrom_batched_workspace_size", "rrt_nystrom_attention_batched_f32", "rrt_encoder_nystrom_workspace_size",
               "rrt_encoder_nystrom_forward_f32", "rrt_nystrom_landmark_attn_batched_workspace_size",
               "rrt_nystrom_pinv_batched_workspace_size"] + [f"rrt_nystrom_{s}_batched_f32" for s in NC.STAGES]


def sd_torch(state):
    return {k: torch.from_numpy(v.copy()) for k, v in state.items()}


# ------------------------------------------------------------------ the restatement against the reference's goldens
@pytest.mark.parametrize("name", list(NC.ATTN_CASES))
def test_restatement_reproduces_the_reference_batched_attention(name):
    b, n, peaked = NC.ATTN_CASES[name]
    state, x = NC.batch_inputs(b, n, peaked)
    gold = load_golden("ntrans_attn")
    r64 = NR.nystrom_batched(x, state, NC.HEADS, dtype=torch.float64)
    assert NR.rel_err(r64["y"][:, [0, n - 1]], gold[name + "/y"]) <= 1e-12
    e32 = NR.rel_err(NR.nystrom_batched(x, state, NC.HEADS, dtype=torch.float32)["y"], r64["y"])
    print(name, "e32 of y", e32, "the reference's", float(gold[name + "/e32"]))
    assert e32 <= E32_MAX and float(gold[name + "/e32"]) <= E32_MAX


@pytest.mark.parametrize("name", list(NC.ENCODER_CASES))
def test_restatement_reproduces_the_reference_encoder(name):
    cfg, state, x = NC.encoder_inputs(name)
    gold = load_golden("ntrans_encoder")
    y64 = NR.encoder(x, state, cfg, dtype=torch.float64)
    assert NR.rel_err(y64[NC.golden_rows(x.shape[0])], gold[name + "/y"]) <= 1e-12
    e32 = NR.rel_err(NR.encoder(x, state, cfg, dtype=torch.float32), y64)
    print(name, "e32", e32, "the reference's", float(gold[name + "/e32"]))
    assert e32 <= E32_MAX and float(gold[name + "/e32"]) <= E32_MAX


@pytest.mark.parametrize("name", list(NC.MIL_CASES))
def test_restatement_reproduces_the_reference_rrtmil(name):
    cfg, state, x = NC.mil_inputs(name)
    gold = load_golden("ntrans_encoder")
    l64 = NR.rrtmil(x, state, cfg, dtype=torch.float64)
    assert NR.rel_err(l64, gold[name + "/logits"]) <= 1e-12
    e32 = NR.rel_err(NR.rrtmil(x, state, cfg, dtype=torch.float32), l64)
    assert e32 <= E32_MAX and float(gold[name + "/e32"]) <= E32_MAX


# ------------------------------------------------------------------ the stage cases
@pytest.mark.parametrize("name", list(NC.STAGE_CASES))
def test_stage_cases_have_a_small_e32(name):
    """every stage on the fp32 roundings of the float64 run's tensors, as tests/test_ntrans_gpu.py feeds it"""
    b, n, peaked = NC.STAGE_CASES[name]
    state, x = NC.batch_inputs(b, n, peaked)
    r64 = NR.nystrom_batched(x, state, NC.HEADS, dtype=torch.float64)
    pad = (256 - n % 256) % 256
    assert r64["qkv"].shape == (b, n + pad, 3 * NC.HEADS * 64) and not r64["qkv"][:, :pad].any()
    i32 = {k: r64[k].float() for k in ("qkv", "ql", "kl", "a2", "av", "z", "wz")}
    i64 = {k: v.double() for k, v in i32.items()}
    conv = torch.from_numpy(state["res_conv.weight"]).reshape(NC.HEADS, -1)
    worst = {}
    for what, fn in (("landmarks", lambda t, c: NR.st_landmarks(t["qkv"], NC.HEADS)[1]),
                     ("landmark_sim", lambda t, c: NR.st_landmark_sim(t["ql"], t["kl"])),
                     ("landmark_attn", lambda t, c: NR.st_landmark_attn(t["qkv"], t["ql"], NC.HEADS)),
                     ("pinv", lambda t, c: NR.pinv_iter(t["a2"], NC.PINV_ITERATIONS)),
                     ("zav", lambda t, c: NR.st_zav(t["z"], t["av"])),
                     ("output", lambda t, c: NR.st_output(t["qkv"], t["kl"], t["wz"], NC.HEADS, c))):
        worst[what] = NR.rel_err(fn(i32, conv), fn(i64, conv.double()))
    print(name, worst)
    assert set(worst) == set(NC.STAGES) and max(worst.values()) <= E32_MAX


def test_the_peaked_case_tells_a_per_item_scale_from_the_global_one():
    b, n, peaked = NC.STAGE_CASES["b3_n144_peaked"]
    assert peaked
    state, x = NC.batch_inputs(b, n, True)
    plain = NC.batch_inputs(b, n, False)[1]
    assert np.array_equal(x[0], plain[0]) and np.allclose(x[1], plain[1] * np.sqrt(NC.PEAK))     # logits x 6 in item 1 alone
    a2 = NR.nystrom_batched(x, state, NC.HEADS, dtype=torch.float64)["a2"]
    z_global, z_item = NR.pinv_iter(a2, NC.PINV_ITERATIONS), NR.pinv_iter_per_item(a2, NC.PINV_ITERATIONS)
    diff = NR.rel_err(z_item, z_global)
    print("per-item against global z:", diff)
    assert diff > 0.1
    # ... while a batch of one has nothing to tell apart
    assert torch.equal(NR.pinv_iter(a2[:1], 6), NR.pinv_iter_per_item(a2[:1], 6))


def test_case_geometry_is_what_the_lists_claim():
    import rrt_oracle as O
    geo = {name: O.grid(N, cfg.get("region_num", 8), cfg.get("region_size", 0), 0, cfg.get("min_region_ratio", 0.0))
           for name, (cfg, N) in NC.ENCODER_CASES.items() if not NC.is_bag(cfg)}
    assert geo["reg_n200_rn2"][:2] == (16, 8) and geo["reg_n1300_rn2_sc"][:2] == (38, 19) and geo["reg_n1000_rn4"][:2] == (32, 8)
    assert geo["reg_n500_rsize9"][:2] == (27, 9) and geo["reg_n300_fallback"][:2] == (18, 18)
    assert sorted(n for _, n, _ in NC.STAGE_CASES.values()) == [144, 144, 256, 300] and NC.ATTN_CASES["b16_n16"][:2] == (16, 16)


# ------------------------------------------------------------------ the ABI
def test_new_exports_exist_and_the_abi_is_29():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rrt_hip.h")).read()
    assert re.search(r"#define\s+RRT_ABI_VERSION\s+29\b", hdr) and _lib.ABI_VERSION == 29
    lib = _lib.load()
    assert lib.rrt_abi_version() == 29
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", hdr), name
        getattr(lib, name)
    assert "RRT_NYSTROM_BAG = 1, RRT_NYSTROM_REGIONS = 2" in hdr
    assert (_lib.NYSTROM_BAG, _lib.NYSTROM_REGIONS) == (1, 2)
    import ctypes as C
    assert C.sizeof(_lib.EncoderNystromDesc) == 4 + C.sizeof(_lib.NystromDesc)


def test_envelope_errors_name_the_field():
    import ctypes as C
    lib = _lib.load()
    d = NystromAttention(128, heads=2)._desc()
    need = C.c_size_t()
    for b in (0, -1, 4097):
        assert lib.rrt_nystrom_batched_workspace_size(C.byref(d), b, 100, C.byref(need)) == -2
        assert b"batch" in lib.rrt_strerror(-2)
    assert lib.rrt_nystrom_batched_workspace_size(C.byref(d), 4096, 16, C.byref(need)) == 0
    one = C.c_size_t()
    assert lib.rrt_nystrom_batched_workspace_size(C.byref(d), 1, 300, C.byref(need)) == 0
    assert lib.rrt_nystrom_workspace_size(C.byref(d), 300, C.byref(one)) == 0 and one.value == need.value
    assert lib.rrt_nystrom_pinv_batched_workspace_size(0, 2, C.byref(need)) == -2
    assert lib.rrt_nystrom_landmark_attn_batched_workspace_size(3, 300, 2, C.byref(need)) == -2      # n_padded % 256
    enc = RRTEncoder(**NC.ENC_BASE, region_attn="ntrans", region_num=2)
    nd = enc._nystrom_desc()
    assert nd.mode == _lib.NYSTROM_REGIONS and nd.attn.heads == 2 and nd.attn.dim == 128
    assert lib.rrt_encoder_nystrom_workspace_size(C.byref(enc._desc), C.byref(nd), 200, C.byref(need)) == 0 and need.value > 0
    enc._desc.compute = _lib.COMPUTE_BF16
    assert lib.rrt_encoder_nystrom_workspace_size(C.byref(enc._desc), C.byref(nd), 200, C.byref(need)) == -2
    assert b"compute" in lib.rrt_strerror(-2)
    enc._desc.compute = _lib.COMPUTE_F32
    nd.mode = 3
    assert lib.rrt_encoder_nystrom_workspace_size(C.byref(enc._desc), C.byref(nd), 200, C.byref(need)) == -2
    assert b"mode" in lib.rrt_strerror(-2)


# ------------------------------------------------------------------ the Python surface
def test_state_dict_keys_match_the_reference_and_load_strict():
    gold = load_golden("ntrans_keys")
    for mode, kw in (("bag", dict(attn="ntrans")), ("regions", dict(region_attn="ntrans"))):
        ref = json.loads(bytes(gold[mode]).decode())
        enc = RRTEncoder(**NC.ENC_BASE, **kw)
        assert [[k, list(v.shape)] for k, v in enc.state_dict().items()] == ref
        sub = "layers.0.attn." + ("" if mode == "bag" else "attn.")
        assert {sub + k for k in NR.NYS_KEYS} <= set(enc.state_dict())
    for name in NC.ENCODER_CASES:
        cfg, state, _ = NC.encoder_inputs(name)
        RRTEncoder(**cfg).load_state_dict(sd_torch(state), strict=True)
    for name in NC.MIL_CASES:
        cfg, state, _ = NC.mil_inputs(name)
        RRTMIL(input_dim=NC.MIL_INPUT_DIM, **cfg).load_state_dict(sd_torch(state), strict=True)


def test_modules_hold_the_reference_nystrom_attention():
    a = RRTEncoder(**NC.ENC_BASE, attn="ntrans", drop_out=0.3).layers[0].attn
    assert isinstance(a, NystromAttention) and (a.dim_head, a.heads, a.num_landmarks, a.pinv_iterations) == (64, 2, 256, 6)
    assert a.residual and a.to_out[1].p == 0.3
    r = RRTEncoder(**NC.ENC_BASE, region_attn="ntrans").layers[0].attn
    assert isinstance(r.attn, NystromAttention) and (r.attn.dim_head, r.attn.heads) == (64, 2)
    # CR-MSA accepts and ignores region_attn; an encoder without attention layers is the plain one
    assert RRTEncoder(**NC.ENC_BASE, region_attn="ntrans", n_layers=1)._nys_mode == 0
    assert RRTEncoder(**NC.ENC_BASE)._nys_mode == 0


def test_outside_the_envelope_construction_raises_and_names_nystrom_attention():
    for kw in (dict(mlp_dim=64, attn="ntrans"), dict(mlp_dim=64, region_attn="ntrans"),
               dict(mlp_dim=128, n_heads=2, attn="ntrans", trans_dim=32), dict(mlp_dim=512, n_heads=4, region_attn="ntrans"),
               dict(mlp_dim=512, n_heads=4, attn="ntrans")):
        with pytest.raises(NotImplementedError, match="NystromAttention"):
            RRTEncoder(**kw)


def test_what_must_raise_raises_without_a_device():
    for kw in (dict(attn="ntrans"), dict(region_attn="ntrans", region_num=2)):
        enc = RRTEncoder(**NC.ENC_BASE, **kw).eval()
        with torch.no_grad(), pytest.raises(_lib.RRTHipError):
            enc(torch.zeros(1, 10, 128))                      # no CPU fallback
        mil = RRTMIL(**kw).eval()
        with pytest.raises(NotImplementedError, match="NystromAttention"):
            mil._mil_desc(1024)                               # the one shared place every one-call entry goes through
    from rrt_mil_amd import ABMIL
    from rrt_mil_amd._head import copy_encoder_desc
    enc = RRTEncoder(attn="ntrans")
    with pytest.raises(NotImplementedError, match="ntrans"):
        copy_encoder_desc(_lib.EncoderDesc(), enc, "x")
    head = ABMIL(1024, 2, False, "relu", rrt=enc)
    with pytest.raises(NotImplementedError, match="ntrans"):
        head._desc_weights(True)
    attn = NystromAttention(128, heads=2)
    with torch.no_grad(), pytest.raises(ValueError, match="b = 1"):
        attn.attention_row(_FakeCuda(torch.zeros(2, 10, 128)))
    with torch.no_grad(), pytest.raises(ValueError, match="forward_batch"):
        attn(_FakeCuda(torch.zeros(2, 10, 128)))                 # forward itself keeps one sequence
    with pytest.raises(NotImplementedError, match="b = 1"):
        attn.forward_batch(_FakeCuda(torch.zeros(2, 10, 128)))   # grad mode is on: the training path keeps b = 1


class _FakeCuda:
    """a tensor's shape with is_cuda set: the shape checks run in front of every device access"""

    def __init__(self, t):
        self._t, self.is_cuda, self.shape, self.requires_grad = t, True, t.shape, False

    def dim(self):
        return self._t.dim()
