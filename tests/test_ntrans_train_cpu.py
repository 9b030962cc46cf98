"""CPU: training the Nystrom ablations of RRTEncoder -- the C ABI surface and the argument checks of the batched Nystrom
backward and of the encoder's tail pair, the ``enable_training`` switches, the refusals that stay without the opt-in, and
the float64 autograd of the restatement tests/ntrans_ref.py against the reference's own float64 gradients
(tests/golden/ntrans_grad.npz, written by tools/make_golden_ntrans_grad.py).  Nothing here launches a kernel."""
import copy
import ctypes as C
import os
import pickle
import re

import pytest
import torch

import ntrans_cases as NC
import ntrans_grad_cases as NG
import ntrans_ref as NR
from conftest import load_golden
from rrt_mil_amd import RRTEncoder, RRTMIL, NystromAttention, _lib
from test_ntrans_cpu import _FakeCuda

pytestmark = pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("output", "zav", "landmark_attn", "pinv_sim", "landmarks")
NEW = (["rrt_nystrom_batched_train_sizes", "rrt_nystrom_attention_batched_forward_train_f32",
        "rrt_nystrom_attention_batched_backward_f32", "rrt_nystrom_output_batched_backward_workspace_size",
        "rrt_nystrom_landmark_attn_batched_backward_workspace_size", "rrt_nystrom_pinv_sim_batched_backward_workspace_size",
        "rrt_encoder_tail_forward_train_f32", "rrt_encoder_tail_backward_f32"]
       + [f"rrt_nystrom_{s}_batched_backward_f32" for s in STAGES])
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x1000            # a non-NULL pointer no call may touch: every check happens before the first launch
BIG = 1 << 44
GOLD_TOL = 1e-12      # the bound tests/test_ntrans_cpu.py pins the forward with


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
def test_new_exports_exist_and_the_abi_is_29(lib):
    hdr = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert re.search(r"#define\s+RRT_ABI_VERSION\s+29\b", hdr) and lib.rrt_abi_version() == 29 and _lib.ABI_VERSION == 29
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rrt_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [n for n, _ in _lib.NystromGrads._fields_] == ["qkv_w", "out_w", "out_b", "conv_w"]


# ------------------------------------------------------------------ sizes and argument checks (nothing is launched)
def test_batched_sizes_at_b1_are_the_single_sequence_ones_and_grow_with_b(lib):
    a, b, a1, b1, need, need1 = (C.c_size_t() for _ in range(6))
    for kw in (dict(), dict(dim=128, heads=2), dict(residual=0), dict(pinv_iterations=1)):
        d = desc(**kw)
        for n in (1, 144, 256, 257, 2600):
            assert lib.rrt_nystrom_batched_train_sizes(C.byref(d), 1, n, C.byref(a), C.byref(b)) == 0
            assert lib.rrt_nystrom_train_sizes(C.byref(d), n, C.byref(a1), C.byref(b1)) == 0
            assert (a.value, b.value) == (a1.value, b1.value)
            prev = (a.value, b.value)
            for bb in (2, 3, 64):
                assert lib.rrt_nystrom_batched_train_sizes(C.byref(d), bb, n, C.byref(a), C.byref(b)) == 0
                assert a.value % 256 == 0 and b.value % 256 == 0 and a.value > prev[0] and b.value > prev[1]
                prev = (a.value, b.value)
                lib.rrt_nystrom_batched_workspace_size(C.byref(d), bb, n, C.byref(need))
                assert a.value >= need.value                       # the stash holds the batched forward's stage tensors
    for npad, heads in ((256, 8), (2816, 2)):
        for fn, fn1 in ((lib.rrt_nystrom_output_batched_backward_workspace_size, lib.rrt_nystrom_output_backward_workspace_size),
                        (lib.rrt_nystrom_landmark_attn_batched_backward_workspace_size,
                         lib.rrt_nystrom_landmark_attn_backward_workspace_size)):
            assert fn(1, npad, heads, C.byref(need)) == 0 and fn1(npad, heads, C.byref(need1)) == 0 and need.value == need1.value
            assert fn(5, npad, heads, C.byref(need)) == 0 and need.value > need1.value
    for it in (1, 6):
        assert lib.rrt_nystrom_pinv_sim_batched_backward_workspace_size(1, 8, it, C.byref(need)) == 0
        assert lib.rrt_nystrom_pinv_sim_backward_workspace_size(8, it, C.byref(need1)) == 0 and need.value == need1.value
        # (iterations + 10) matrices per (item, head), plus a2: 2 GiB and more at b = 64, eight heads, six iterations
        assert lib.rrt_nystrom_pinv_sim_batched_backward_workspace_size(64, 8, it, C.byref(need)) == 0
        assert need.value >= (it + 11) * 64 * 8 * 256 * 256 * 4
    lib.rrt_nystrom_batched_train_sizes(C.byref(desc()), 64, 144, C.byref(a), C.byref(b))
    assert b.value > 2 ** 31


def test_the_bound_on_b_is_refused_and_named(lib):
    a, b = C.c_size_t(), C.c_size_t()
    d, w, g = desc(), four(_lib.NystromWeights), four(_lib.NystromGrads)
    assert lib.rrt_nystrom_batched_train_sizes(C.byref(d), NG.TRAIN_B_MAX, 16, C.byref(a), C.byref(b)) == 0
    for bad in (0, -1, NG.TRAIN_B_MAX + 1, 4096):
        assert lib.rrt_nystrom_batched_train_sizes(C.byref(d), bad, 16, C.byref(a), C.byref(b)) == UNSUPPORTED
        assert re.search(r"\bb\b", why(lib)) and "2048" in why(lib)
        assert lib.rrt_nystrom_attention_batched_forward_train_f32(C.byref(d), C.byref(w), P, P, bad, 16, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_attention_batched_backward_f32(C.byref(d), C.byref(w), P, P, P, BIG, C.byref(g), P, bad, 16, P, BIG,
                                                              None) == UNSUPPORTED
        assert lib.rrt_nystrom_output_batched_backward_workspace_size(bad, 256, 8, C.byref(a)) == UNSUPPORTED
        assert lib.rrt_nystrom_output_batched_backward_f32(*[P] * 9, bad, 256, 8, 33, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_zav_batched_backward_f32(*[P] * 5, bad, 8, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmark_attn_batched_backward_workspace_size(bad, 256, 8, C.byref(a)) == UNSUPPORTED
        assert lib.rrt_nystrom_landmark_attn_batched_backward_f32(*[P] * 5, bad, 256, 8, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_pinv_sim_batched_backward_workspace_size(bad, 8, 6, C.byref(a)) == UNSUPPORTED
        assert lib.rrt_nystrom_pinv_sim_batched_backward_f32(*[P] * 5, bad, 8, 6, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmarks_batched_backward_f32(*[P] * 3, bad, 256, 8, None) == UNSUPPORTED
        assert re.search(r"\bb\b", why(lib))
    # b * n beyond what one linear takes, and the single-sequence envelope
    assert lib.rrt_nystrom_batched_train_sizes(C.byref(d), 2048, 2000, C.byref(a), C.byref(b)) == UNSUPPORTED and "b * n" in why(lib)
    for kw, word in ((dict(dim_head=32), "dim_head"), (dict(heads=17), "heads"), (dict(pinv_iterations=17), "pinv_iterations")):
        assert lib.rrt_nystrom_batched_train_sizes(C.byref(desc(**kw)), 3, 100, C.byref(a), C.byref(b)) == UNSUPPORTED
        assert word in why(lib)
    for heads in (0, 17):
        assert lib.rrt_nystrom_zav_batched_backward_f32(*[P] * 5, 3, heads, None) == UNSUPPORTED and "heads" in why(lib)
    for bad in (1000448, 100):                               # beyond 1e6 rounded up; not a multiple of 256
        assert lib.rrt_nystrom_output_batched_backward_f32(*[P] * 9, 3, bad, 8, 33, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmark_attn_batched_backward_f32(*[P] * 5, 3, bad, 8, P, BIG, None) == UNSUPPORTED
        assert lib.rrt_nystrom_landmarks_batched_backward_f32(*[P] * 3, 3, bad, 8, None) == UNSUPPORTED
    assert lib.rrt_nystrom_pinv_sim_batched_backward_f32(*[P] * 5, 3, 8, 17, P, BIG, None) == UNSUPPORTED


def test_null_pointers_and_short_buffers(lib):
    a, b, need = C.c_size_t(), C.c_size_t(), C.c_size_t()
    d, w, g = desc(dim=128, heads=2), four(_lib.NystromWeights), four(_lib.NystromGrads)
    assert lib.rrt_nystrom_batched_train_sizes(None, 3, 10, C.byref(a), C.byref(b)) == INVALID
    assert lib.rrt_nystrom_batched_train_sizes(C.byref(d), 3, 10, None, C.byref(b)) == INVALID
    assert lib.rrt_nystrom_batched_train_sizes(C.byref(d), 3, 0, C.byref(a), C.byref(b)) == INVALID
    fw, bw = lib.rrt_nystrom_attention_batched_forward_train_f32, lib.rrt_nystrom_attention_batched_backward_f32
    for args in ((None, C.byref(w), P, P), (C.byref(d), None, P, P), (C.byref(d), C.byref(w), None, P),
                 (C.byref(d), C.byref(w), P, None), (C.byref(d), C.byref(four(_lib.NystromWeights, None)), P, P)):
        assert fw(*args, 3, 10, P, BIG, None) == INVALID
    assert bw(C.byref(d), C.byref(w), None, P, P, BIG, C.byref(g), P, 3, 10, P, BIG, None) == INVALID
    assert bw(C.byref(d), C.byref(w), P, None, P, BIG, C.byref(g), P, 3, 10, P, BIG, None) == INVALID
    assert bw(C.byref(d), C.byref(w), P, P, P, BIG, None, P, 3, 10, P, BIG, None) == INVALID
    assert bw(C.byref(d), C.byref(w), P, P, P, BIG, C.byref(four(_lib.NystromGrads, None)), P, 3, 10, P, BIG, None) == INVALID
    for bb, n in ((1, 300), (3, 144), (3, 256), (40, 16)):
        assert lib.rrt_nystrom_batched_train_sizes(C.byref(d), bb, n, C.byref(a), C.byref(b)) == 0
        assert fw(C.byref(d), C.byref(w), P, P, bb, n, P, a.value - 1, None) == WORKSPACE
        assert fw(C.byref(d), C.byref(w), P, P, bb, n, None, a.value, None) == WORKSPACE
        assert bw(C.byref(d), C.byref(w), P, P, P, a.value - 1, C.byref(g), P, bb, n, P, b.value, None) == WORKSPACE
        assert bw(C.byref(d), C.byref(w), P, P, P, a.value, C.byref(g), P, bb, n, P, b.value - 1, None) == WORKSPACE
        assert bw(C.byref(d), C.byref(w), P, P, P, a.value, C.byref(g), None, bb, n, None, b.value, None) == WORKSPACE
    assert lib.rrt_nystrom_output_batched_backward_workspace_size(3, 256, 2, C.byref(need)) == 0
    assert lib.rrt_nystrom_output_batched_backward_f32(*[P] * 9, 3, 256, 2, 33, P, need.value - 1, None) == WORKSPACE
    assert lib.rrt_nystrom_landmark_attn_batched_backward_workspace_size(3, 256, 2, C.byref(need)) == 0
    assert lib.rrt_nystrom_landmark_attn_batched_backward_f32(*[P] * 5, 3, 256, 2, P, need.value - 1, None) == WORKSPACE
    assert lib.rrt_nystrom_pinv_sim_batched_backward_workspace_size(3, 2, 6, C.byref(need)) == 0
    assert lib.rrt_nystrom_pinv_sim_batched_backward_f32(*[P] * 5, 3, 2, 6, P, need.value - 1, None) == WORKSPACE
    for fn, extra in ((lib.rrt_nystrom_zav_batched_backward_f32, (3, 2, None)),
                      (lib.rrt_nystrom_landmark_attn_batched_backward_f32, (3, 256, 2, P, BIG, None)),
                      (lib.rrt_nystrom_pinv_sim_batched_backward_f32, (3, 2, 6, P, BIG, None))):
        for i in range(5):
            args = [P] * 5
            args[i] = None
            assert fn(*args, *extra) == INVALID, (fn.__name__, i)
    for i in range(3):
        args = [P] * 3
        args[i] = None
        assert lib.rrt_nystrom_landmarks_batched_backward_f32(*args, 3, 256, 2, None) == INVALID
    for i in (0, 1, 2, 4, 5, 6, 7):
        args = [P] * 9
        args[i] = None
        assert lib.rrt_nystrom_output_batched_backward_f32(*args, 3, 256, 2, 33, P, BIG, None) == INVALID, i


def test_tail_pair_checks_its_descriptor(lib):
    enc = RRTEncoder(**NC.ENC_BASE, region_attn="ntrans", region_num=2, all_shortcut=True)
    w, g = enc._weights(), _lib.EncoderGrads()
    full, tail = enc._desc, enc._tail_desc()
    assert (tail.n_rmsa_layers, tail.pos, tail.all_shortcut, tail.cr_msa) == (0, _lib.POS_NONE, 1, 1) and full.n_rmsa_layers == 1
    fw, bw = lib.rrt_encoder_tail_forward_train_f32, lib.rrt_encoder_tail_backward_f32
    assert fw(C.byref(full), C.byref(w), P, P, P + 64, 200, P, BIG, 0.0, 0, None, None) == UNSUPPORTED and "n_rmsa_layers" in why(lib)
    assert bw(C.byref(full), C.byref(w), P, P, P, BIG, C.byref(g), P, P, 200, P, BIG, 0.0, 0, None, None) == UNSUPPORTED
    assert fw(None, C.byref(w), P, P, P + 64, 200, P, BIG, 0.0, 0, None, None) == INVALID
    assert fw(C.byref(tail), C.byref(w), P, None, P + 64, 200, P, BIG, 0.0, 0, None, None) == INVALID     # all_shortcut needs x0
    assert bw(C.byref(tail), C.byref(w), P, P, P, BIG, C.byref(g), P, None, 200, P, BIG, 0.0, 0, None, None) == INVALID
    assert fw(C.byref(tail), C.byref(w), P, P, P + 64, 200, P, 0, 0.0, 0, None, None) == WORKSPACE
    assert fw(C.byref(tail), C.byref(w), P, P, P + 64, 200, P, BIG, 1.5, 0, None, None) == INVALID         # drop_p


# ------------------------------------------------------------------ the switches, without a device
def test_enable_training_switches():
    for kw in (dict(attn="ntrans"), dict(region_attn="ntrans", region_num=2)):
        enc = RRTEncoder(**NC.ENC_BASE, n_layers=3, **kw)
        held = [enc._nystrom_of(l) for l in enc.layers.children()]
        assert len(held) == 2 and all(isinstance(a, NystromAttention) for a in held)
        assert enc._train_enabled is False and not any(a._train_enabled for a in held)
        keys = list(enc.state_dict())
        assert enc.enable_training() is enc and enc._train_enabled and all(a._train_enabled for a in held)
        assert list(enc.state_dict()) == keys and not any("train" in k for k in keys)
        for clone in (pickle.loads(pickle.dumps(enc)), copy.deepcopy(enc)):
            assert clone._train_enabled and all(clone._nystrom_of(l)._train_enabled for l in clone.layers.children())
        fresh = RRTEncoder(**NC.ENC_BASE, n_layers=3, **kw)
        fresh.load_state_dict(enc.state_dict(), strict=True)
        assert fresh._train_enabled is False                         # not part of the state_dict
        # on or off, there is no CPU path
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            enc(torch.zeros(1, 10, 128))
        assert enc.enable_training(False) is enc and not enc._train_enabled and not any(a._train_enabled for a in held)
        mil = RRTMIL(**kw)
        assert mil.online_encoder.enable_training() is mil.online_encoder
        assert pickle.loads(pickle.dumps(mil)).online_encoder._train_enabled
        with pytest.raises(NotImplementedError, match="NystromAttention"):
            mil._mil_desc(1024)                                      # the one-call head entries keep raising
    # an R-MSA encoder has the switch too; it changes nothing there
    plain = RRTEncoder(**NC.ENC_BASE)
    assert plain.enable_training() is plain and plain._nys_mode == 0


def test_refusals_without_the_opt_in_are_unchanged():
    attn = NystromAttention(128, heads=2)
    with pytest.raises(NotImplementedError, match="b = 1") as e:
        attn.forward_batch(_FakeCuda(torch.zeros(2, 10, 128)))       # grad mode is on
    assert str(e.value) == ("rrt_mil_amd.NystromAttention.forward_batch is an inference entry (the training path keeps "
                            "b = 1: the backward kernels take one sequence): call it in eval() under torch.no_grad()")
    drop = NystromAttention(128, heads=2, dropout=0.1).train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="b = 1"):
        drop.forward_batch(_FakeCuda(torch.zeros(2, 10, 128)))
    for kw in (dict(attn="ntrans"), dict(region_attn="ntrans", region_num=2)):
        enc = RRTEncoder(**NC.ENC_BASE, **kw).eval()
        x = torch.zeros(10, 128)
        with pytest.raises(NotImplementedError) as e:
            enc._forward_bag_nystrom(x, None)                        # the checks stand in front of every device access
        assert str(e.value) == ("rrt_mil_amd.RRTEncoder with NystromAttention layers (attn='ntrans' / region_attn="
                                "'ntrans') has no backward: call it in eval() under torch.no_grad()")
        with torch.no_grad(), pytest.raises(NotImplementedError) as e:
            enc.train()._forward_bag_nystrom(x, None)
        assert str(e.value) == ("rrt_mil_amd.RRTEncoder with NystromAttention layers (attn='ntrans' / region_attn="
                                "'ntrans') in train() with dropout: inference only, call eval() under torch.no_grad()")
        with pytest.raises(NotImplementedError, match="one bag per call"):
            enc.forward_batch(torch.zeros(2, 10, 128))
        with pytest.raises(NotImplementedError, match="one bag per call"):
            enc.enable_training().forward_batch(torch.zeros(2, 10, 128))       # batch > 1 stays refused


# ------------------------------------------------------------------ the restatement's autograd against the reference's gradients
def against_golden(gold, key, grads):
    seen = 0
    for name, g in grads.items():
        ref = torch.from_numpy(gold[f"{key}/{name}"])
        got = NG.rows(name, g)
        assert tuple(got.shape) == tuple(ref.shape), (key, name, got.shape, ref.shape)
        assert float(ref.abs().max()) > 0, (key, name)
        assert NR.rel_err(got, ref) <= GOLD_TOL, (key, name, NR.rel_err(got, ref))
        assert f"{key}/{name}/e32" in gold
        seen += 1
    return seen


@pytest.mark.parametrize("name", NG.GOLDEN_ENCODER_CASES)
def test_restatement_autograd_reproduces_the_reference_encoder_gradients(name):
    cfg, state, x = NC.encoder_inputs(name)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).double().requires_grad_(True)
    dy = torch.from_numpy(NG.cotangent(name, "dy", x.shape)).double()
    (NR.encoder(xd, p, cfg, dtype=torch.float64) * dy).sum().backward()
    grads = {**{k: v.grad for k, v in p.items()}, "dx": xd.grad}
    assert all(g is not None for g in grads.values())                # every parameter receives a gradient
    assert against_golden(load_golden("ntrans_grad"), "enc/" + name, grads) == 16
    assert NC.is_bag(cfg) == (name == "bag_n300")


def test_restatement_autograd_reproduces_the_reference_batched_attention_gradients():
    name = NG.GOLDEN_ATTN_CASE
    b, n, peaked = NC.ATTN_CASES[name]
    state, x = NC.batch_inputs(b, n, peaked)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in state.items()}
    xd = torch.from_numpy(x).double().requires_grad_(True)
    dy = torch.from_numpy(NG.cotangent(name, "dy", x.shape)).double()
    (NR.nystrom_batched(xd, p, NC.HEADS, dtype=torch.float64)["y"] * dy).sum().backward()
    grads = {**{k: v.grad for k, v in p.items()}, "dx": xd.grad}
    assert against_golden(load_golden("ntrans_grad"), "attn/" + name, grads) == 5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ntrans_grad.npz")) < 300_000
