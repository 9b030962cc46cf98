"""CPU: the C ABI surface and the argument checks of TransMIL's one-call training step (rrt_transmil_forward_train_f32 /
rrt_transmil_backward_f32, their stage entries and the cls-row A/B twins), the ``enable_training(one_call=True)`` switch, the
restatement tests/transmil_step_ref.py against tests/nystrom_ref.py, and that the float64 reference alone keeps every judged
quantity of tests/test_transmil_step_gpu.py above 1e-4."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import nystrom_grad_cases as GC
import nystrom_ref as R
import transmil_cases as TC
import transmil_step_ref as SR
from rrt_mil_amd import _lib

pytestmark = pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP =("rrt_transmil_train_sizes", "rrt_transmil_forward_train_f32", "rrt_transmil_backward_f32")
STAGES = ("rrt_ppeg_side_backward_workspace_size", "rrt_ppeg_side_backward_f32", "rrt_transmil_assemble_backward_f32",
          "rrt_nystrom_output_row_f32", "rrt_nystrom_output_row_backward_f32")
ROW = ("rrt_debug_transmil_train_sizes_row", "rrt_debug_transmil_forward_train_row_f32",
        "rrt_debug_transmil_backward_row_f32")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x1000            # a non-NULL pointer no call may touch: every check happens before the first launch
BIG = 1 << 40
GRAD_FIELDS = ["fc1_w", "fc1_b", "cls_token", "layer", "pos_w", "pos_b", "norm_w", "norm_b", "fc2_w", "fc2_b"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def why(lib):
    return lib.rrt_strerror(UNSUPPORTED).decode()


def desc(**kw):
    d = _lib.TransmilDesc()
    d.input_dim, d.n_classes, d.act = 64, 2, _lib.ACT_GELU
    a = d.attn
    a.dim, a.heads, a.dim_head, a.num_landmarks, a.pinv_iterations, a.residual, a.residual_conv_kernel = 512, 8, 64, 256, 6, 1, 33
    for k, v in kw.items():
        setattr(a if hasattr(a, k) and not hasattr(d, k) else d, k, v)
    return d


def filled(cls, p=P):
    """a weights or grads struct with every pointer set to p"""
    s = cls()
    slots = (C.c_void_p * (C.sizeof(cls) // C.sizeof(C.c_void_p))).from_buffer(s)
    for i in range(len(slots)):
        slots[i] = p
    return s


def fwd_args(d, w, x=P, logits=P, n=100, stash=P, stash_bytes=BIG, p1=0.0, pa=0.0):
    return (C.byref(d) if d is not None else None, C.byref(w) if w is not None else None, x, logits, n, stash, stash_bytes, p1,
            pa, 0, None)


def bwd_args(d, w, g, x=P, dl=P, stash=P, stash_bytes=BIG, dx=P, n=100, ws=P, ws_bytes=BIG, p1=0.0, pa=0.0):
    return (C.byref(d) if d is not None else None, C.byref(w) if w is not None else None, x, dl, stash, stash_bytes,
            C.byref(g) if g is not None else None, dx, n, ws, ws_bytes, p1, pa, 0, None)


# ------------------------------------------------------------------ exports
def test_exports(lib):
    hdr = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert "#define RRT_ABI_VERSION 29" in hdr and lib.rrt_abi_version() == 29 and _lib.ABI_VERSION == 29
    for tag in ("200", "201", "202"):
        assert tag in re.search(r"TransMIL, training:.*?\*/", hdr, flags=re.S).group(0), "the header states the drop tags"
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rrt_[a-z0-9_]+)\s*\(", hdr))
    for name in STEP + STAGES + ROW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"typedef struct rrt_transmil_grads \{(.*?)\} rrt_transmil_grads;", hdr, flags=re.S)
    assert [n for n, _ in _lib.TransmilGrads._fields_] == GRAD_FIELDS
    assert [n for n, _ in _lib.TransmilGrads._fields_] == [n for n, _ in _lib.TransmilWeights._fields_]     # same layout
    assert C.sizeof(_lib.TransmilGrads) == C.sizeof(_lib.TransmilWeights) == 25 * C.sizeof(C.c_void_p)
    build = __import__("rrt_mil_amd.build", fromlist=["SOURCES"])
    assert "transmil_bwd.hip" in build.SOURCES and not build.PACKED_FP32_OK


def test_step_params_follow_the_grads_struct():
    from rrt_mil_amd import TransMIL
    model = TransMIL(64, 2, True, "gelu")
    ps = model._step_params()
    names = {id(p): k for k, p in model.named_parameters()}
    assert len(ps) == 25 == len(list(model.parameters())) and len({id(p) for p in ps}) == 25
    order = [names[id(p)] for p in ps]
    assert order[:3] == ["_fc1.0.weight", "_fc1.0.bias", "cls_token"]
    assert order[3:9] == ["layer1.norm.weight", "layer1.norm.bias", "layer1.attn.to_qkv.weight", "layer1.attn.to_out.0.weight",
                          "layer1.attn.to_out.0.bias", "layer1.attn.res_conv.weight"]
    assert order[9:15] == [k.replace("layer1", "layer2") for k in order[3:9]]
    assert order[15:21] == [f"pos_layer.{n}.{t}" for t in ("weight", "bias") for n in ("proj", "proj1", "proj2")]
    assert order[21:] == ["norm.weight", "norm.bias", "_fc2.weight", "_fc2.bias"]


# ------------------------------------------------------------------ sizes
def test_train_sizes(lib):
    a, b = C.c_size_t(), C.c_size_t()
    prev = (0, 0)
    for n in (1, 37, 250, 1000, 9000):
        d = desc()
        assert lib.rrt_transmil_train_sizes(C.byref(d), n, C.byref(a), C.byref(b)) == 0
        assert a.value > prev[0] and b.value >= prev[1] and a.value % 256 == 0 and b.value % 256 == 0
        prev = (a.value, b.value)
        rows = 1 + SR.side_of(n) ** 2
        npad = (rows + 255) // 256 * 256
        s1, w1 = C.c_size_t(), C.c_size_t()
        assert lib.rrt_nystrom_train_sizes(C.byref(d.attn), rows, C.byref(s1), C.byref(w1)) == 0
        # two attention stashes and the step's own rows on top
        assert a.value > 2 * s1.value - npad * 512 * 4
        assert a.value < 2 * s1.value + (6 * rows + n) * 512 * 4 + (1 << 16)
        assert b.value > w1.value
        # the cls-row twin keeps neither layer 2's o nor a [rows, dim] attention output of layer 2
        ra, rb = C.c_size_t(), C.c_size_t()
        assert lib.rrt_debug_transmil_train_sizes_row(C.byref(d), n, C.byref(ra), C.byref(rb)) == 0
        assert 2 * s1.value - npad * 512 * 4 < ra.value <= a.value - (npad + rows) * 512 * 4 and rb.value == b.value
    plain, gelu = C.c_size_t(), C.c_size_t()
    assert lib.rrt_transmil_train_sizes(C.byref(desc(act=_lib.ACT_NONE)), 1000, C.byref(plain), C.byref(b)) == 0
    assert lib.rrt_transmil_train_sizes(C.byref(desc()), 1000, C.byref(gelu), C.byref(b)) == 0
    assert gelu.value - plain.value >= 1000 * 512 * 4, "the pre-activation is kept only when there is an activation"


# ------------------------------------------------------------------ argument checks (nothing is launched: no device needed)
@pytest.mark.parametrize("kw,word", [(dict(dim_head=32), "dim_head"), (dict(num_landmarks=128), "num_landmarks"),
                                     (dict(residual_conv_kernel=32), "residual_conv_kernel"), (dict(heads=17), "heads"),
                                     (dict(dim=48), "dim"), (dict(pinv_iterations=17), "pinv_iterations"),
                                     (dict(input_dim=40), "input_dim"), (dict(act=3), "act"), (dict(n_classes=65), "n_classes")],
                         ids=lambda v: str(v))
def test_unsupported_fields_are_named(lib, kw, word):
    a, b = C.c_size_t(), C.c_size_t()
    d, w, g = desc(**kw), filled(_lib.TransmilWeights), filled(_lib.TransmilGrads)
    for sizes in (lib.rrt_transmil_train_sizes, lib.rrt_debug_transmil_train_sizes_row):
        assert sizes(C.byref(d), 1000, C.byref(a), C.byref(b)) == UNSUPPORTED and word in why(lib)
    for fw in (lib.rrt_transmil_forward_train_f32, lib.rrt_debug_transmil_forward_train_row_f32):
        assert fw(*fwd_args(d, w)) == UNSUPPORTED and word in why(lib)
    for bw in (lib.rrt_transmil_backward_f32, lib.rrt_debug_transmil_backward_row_f32):
        assert bw(*bwd_args(d, w, g)) == UNSUPPORTED and word in why(lib)


def test_null_pointers_and_bad_values(lib):
    a, b = C.c_size_t(), C.c_size_t()
    d, w, g = desc(), filled(_lib.TransmilWeights), filled(_lib.TransmilGrads)
    assert lib.rrt_transmil_train_sizes(None, 10, C.byref(a), C.byref(b)) == INVALID
    assert lib.rrt_transmil_train_sizes(C.byref(d), 10, None, C.byref(b)) == INVALID
    assert lib.rrt_transmil_train_sizes(C.byref(d), 10, C.byref(a), None) == INVALID
    assert lib.rrt_transmil_train_sizes(C.byref(d), 0, C.byref(a), C.byref(b)) == INVALID
    assert lib.rrt_transmil_train_sizes(C.byref(d), 998002, C.byref(a), C.byref(b)) == UNSUPPORTED and "n_tokens" in why(lib)
    fw, bw = lib.rrt_transmil_forward_train_f32, lib.rrt_transmil_backward_f32
    for kw in (dict(d=None), dict(w=None), dict(x=None), dict(logits=None), dict(n=0), dict(p1=1.0), dict(pa=-0.1),
               dict(p1=float("nan"))):
        args = dict(d=d, w=w)
        args.update(kw)
        assert fw(*fwd_args(**args)) == INVALID, kw
    for i in range(25):                                        # every weight pointer is needed
        wi = filled(_lib.TransmilWeights)
        (C.c_void_p * 25).from_buffer(wi)[i] = None
        assert fw(*fwd_args(d, wi)) == INVALID, i
        gi = filled(_lib.TransmilGrads)
        (C.c_void_p * 25).from_buffer(gi)[i] = None
        assert bw(*bwd_args(d, w, gi)) == INVALID, i
    for kw in (dict(d=None), dict(w=None), dict(g=None), dict(x=None), dict(dl=None), dict(n=0), dict(p1=1.0), dict(pa=2.0)):
        args = dict(d=d, w=w, g=g)
        args.update(kw)
        assert bw(*bwd_args(**args)) == INVALID, kw
    # residual = 0: neither conv_w is needed; dx is optional: both reach the workspace check
    noconv_w, noconv_g = filled(_lib.TransmilWeights), filled(_lib.TransmilGrads)
    for i in (0, 1):
        noconv_w.layer[i].attn.conv_w = None
        noconv_g.layer[i].attn.conv_w = None
    assert bw(*bwd_args(desc(residual=0), noconv_w, noconv_g, dx=None, ws=None, ws_bytes=0)) == WORKSPACE
    assert bw(*bwd_args(d, w, noconv_g)) == INVALID


def test_short_stash_and_workspace(lib):
    a, b = C.c_size_t(), C.c_size_t()
    d, w, g = desc(), filled(_lib.TransmilWeights), filled(_lib.TransmilGrads)
    assert lib.rrt_transmil_train_sizes(C.byref(d), 100, C.byref(a), C.byref(b)) == 0
    fw, bw = lib.rrt_transmil_forward_train_f32, lib.rrt_transmil_backward_f32
    assert fw(*fwd_args(d, w, stash_bytes=a.value - 1)) == WORKSPACE
    assert fw(*fwd_args(d, w, stash=None)) == WORKSPACE
    assert bw(*bwd_args(d, w, g, stash_bytes=a.value - 1)) == WORKSPACE
    assert bw(*bwd_args(d, w, g, stash=None)) == WORKSPACE
    assert bw(*bwd_args(d, w, g, stash_bytes=a.value, ws_bytes=b.value - 1)) == WORKSPACE
    assert bw(*bwd_args(d, w, g, stash_bytes=a.value, ws=None)) == WORKSPACE
    # the cls-row twin has a smaller stash of its own: the step does not fit into it
    ra, rb = C.c_size_t(), C.c_size_t()
    assert lib.rrt_debug_transmil_train_sizes_row(C.byref(d), 100, C.byref(ra), C.byref(rb)) == 0 and ra.value < a.value
    assert fw(*fwd_args(d, w, stash_bytes=ra.value)) == WORKSPACE
    assert bw(*bwd_args(d, w, g, stash_bytes=ra.value)) == WORKSPACE
    assert lib.rrt_debug_transmil_forward_train_row_f32(*fwd_args(d, w, stash_bytes=ra.value - 1)) == WORKSPACE
    assert lib.rrt_debug_transmil_backward_row_f32(*bwd_args(d, w, g, stash_bytes=ra.value - 1)) == WORKSPACE


def test_stage_entry_checks(lib):
    a = C.c_size_t()
    size, pb = lib.rrt_ppeg_side_backward_workspace_size, lib.rrt_ppeg_side_backward_f32
    assert size(8, 64, None) == INVALID and size(0, 64, C.byref(a)) == INVALID and size(8, 0, C.byref(a)) == INVALID
    assert size(8, 66, C.byref(a)) == UNSUPPORTED and "dim" in why(lib)
    assert size(1001, 64, C.byref(a)) == UNSUPPORTED and "side" in why(lib)
    sizes = []
    for side in (1, 7, 8, 9, 32):
        assert size(side, 512, C.byref(a)) == 0
        sizes.append(a.value)
    assert sizes == sorted(sizes) and sizes[0] >= 2 * 49 * 512 * 4
    three = (C.c_void_p * 3)(P, P, P)
    assert size(8, 64, C.byref(a)) == 0
    assert pb(P, P, three, P, three, three, 8, 64, P, a.value - 1, None) == WORKSPACE
    assert pb(P, P, three, P, three, three, 8, 64, None, BIG, None) == WORKSPACE
    assert pb(P, P, three, P, three, None, 8, 64, None, 0, None) == WORKSPACE          # db is optional
    for i in (0, 1, 2, 3, 4):
        args = [P, P, three, P, three]
        args[i] = None
        assert pb(*args, three, 8, 64, P, BIG, None) == INVALID, i
    assert pb(P, P, (C.c_void_p * 3)(P, None, P), P, three, three, 8, 64, P, BIG, None) == INVALID
    assert pb(P, P, three, P, (C.c_void_p * 3)(P, P, None), three, 8, 64, P, BIG, None) == INVALID
    assert pb(P, P, three, P, three, three, 8, 66, P, BIG, None) == UNSUPPORTED
    ab = lib.rrt_transmil_assemble_backward_f32
    for i in (0, 2, 3):
        args = [P] * 4
        args[i] = None
        assert ab(*args, 10, 512, _lib.ACT_GELU, 0.0, 0, None) == INVALID, i
    assert ab(P, None, P, P, 10, 512, _lib.ACT_GELU, 0.0, 0, None) == INVALID          # the derivative needs hpre
    assert ab(P, P, P, P, 0, 512, _lib.ACT_GELU, 0.0, 0, None) == INVALID
    assert ab(P, P, P, P, 10, 512, _lib.ACT_GELU, 1.0, 0, None) == INVALID
    assert ab(P, P, P, P, 10, 510, _lib.ACT_GELU, 0.0, 0, None) == UNSUPPORTED and "dim" in why(lib)
    assert ab(P, P, P, P, 10, 512, _lib.ACT_TANH, 0.0, 0, None) == UNSUPPORTED and "act" in why(lib)
    assert ab(P, P, P, P, 998002, 512, _lib.ACT_GELU, 0.0, 0, None) == UNSUPPORTED and "n_tokens" in why(lib)
    row, rowb = lib.rrt_nystrom_output_row_f32, lib.rrt_nystrom_output_row_backward_f32
    for r in (-1, 256):
        assert row(*[P] * 5, r, 256, 2, 33, None) == UNSUPPORTED and "row" in why(lib)
        assert rowb(*[P] * 9, r, 256, 2, 33, None) == UNSUPPORTED and "row" in why(lib)
    for bad_np in (100, 1000448):
        assert row(*[P] * 5, 0, bad_np, 2, 33, None) == UNSUPPORTED
        assert rowb(*[P] * 9, 0, bad_np, 2, 33, None) == UNSUPPORTED
    for heads in (0, 17):
        assert row(*[P] * 5, 0, 256, heads, 33, None) == UNSUPPORTED and "heads" in why(lib)
        assert rowb(*[P] * 9, 0, 256, heads, 33, None) == UNSUPPORTED and "heads" in why(lib)
    assert row(*[P] * 5, 0, 256, 2, 32, None) == UNSUPPORTED and "residual_conv_kernel" in why(lib)
    assert rowb(*[P] * 9, 0, 256, 2, 65, None) == UNSUPPORTED and "residual_conv_kernel" in why(lib)
    for i in (0, 1, 2, 4):                                     # conv_w (3) may be NULL
        args = [P] * 5
        args[i] = None
        assert row(*args, 0, 256, 2, 33, None) == INVALID, i
    for i in (0, 1, 2, 4, 5, 6, 7, 8):                         # conv_w (3) may be NULL; only then d_conv_w (8) may be too
        args = [P] * 9
        args[i] = None
        assert rowb(*args, 0, 256, 2, 33, None) == INVALID, i


# ------------------------------------------------------------------ the module's switch
def test_enable_training_one_call_switch():
    from rrt_mil_amd import TransMIL
    model = TransMIL(64, 2, True, "relu")
    assert model._one_call is False and model._train_enabled is False
    assert model.enable_training(one_call=True) is model
    assert model._one_call and model._train_enabled and model.layer1.attn._train_enabled and model.layer2.attn._train_enabled
    assert model.enable_training() is model and not model._one_call and model._train_enabled      # one_call=False: the layer path
    model.enable_training(False, one_call=True)
    assert not model._one_call and not model._train_enabled
    assert "_one_call" not in model.state_dict() and len(model.state_dict()) == 25
    with pytest.raises(_lib.RRTHipError, match="cuda"):
        model.enable_training(one_call=True)(torch.zeros(5, 64))


# ------------------------------------------------------------------ the restatement
def test_step_restatement_is_the_reference_model():
    """without masks transmil_step IS nystrom_ref.transmil (which the reference's own float64 run pins), values and gradients"""
    for input_dim, act, N in ((64, "gelu", 3), (64, "relu", 36), (64, "none", 37)):
        state, x = TC.model_inputs(input_dim, N)
        want = R.transmil(x, state, act)["logits"]
        got = SR.transmil_step(x, state, act)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (act, N)
    state, x = TC.model_inputs(64, 37)
    grads = []
    for fn in (lambda xd, p: R.transmil(xd, p, "gelu")["logits"], lambda xd, p: SR.transmil_step(xd, p, "gelu")):
        p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in state.items()}
        xd = torch.from_numpy(x).double().requires_grad_(True)
        F.cross_entropy(fn(xd, p)[None], torch.tensor([GC.LABEL])).backward()
        grads.append({**{k: v.grad for k, v in p.items()}, "dx": xd.grad})
    for k in grads[0]:
        assert float((grads[0][k] - grads[1][k]).abs().max()) <= 1e-10 * float(grads[0][k].abs().max()), k
    # the masks act where they say: fc1 on h before the wrap, attn2 on row 0 of layer 2's branch alone
    ones = {"fc1": torch.ones(37, 512), "attn1": torch.ones(50, 512), "attn2": torch.ones(512)}
    assert torch.equal(SR.transmil_step(x, state, "gelu", masks=ones), SR.transmil_step(x, state, "gelu"))
    for k in ones:
        m = dict(ones)
        m[k] = torch.zeros_like(ones[k])
        assert not torch.equal(SR.transmil_step(x, state, "gelu", masks=m), SR.transmil_step(x, state, "gelu")), k


def test_single_row_and_glue_restatements():
    state, x = TC.attn_inputs(128, 2, 512, 1.0)
    st = R.nystrom(x, state, 2)
    cw = torch.from_numpy(state["res_conv.weight"]).double().reshape(2, -1)
    full = R.st_output(st["qkv"], st["kl"], st["wz"], 2, cw)
    for row in (0, 255, 256, 511):
        assert torch.equal(SR.output_row(st["qkv"], st["kl"], st["wz"], 2, cw, row), full[row])
    h, cls = torch.randn(10, 8, dtype=torch.float64), torch.randn(8, dtype=torch.float64)
    seq = SR.assemble(h, cls, "none")
    assert seq.shape == (17, 8) and torch.equal(seq[0], cls) and torch.equal(seq[1:11], h) and torch.equal(seq[11:], h[:6])
    # a 2 x 2 grid under the 7 x 7 kernel: every output sees every input through the kernel's centre block
    w7, xg = torch.randn(1, 1, 7, 7, dtype=torch.float64), torch.randn(4, 1, dtype=torch.float64)
    z5, z3 = torch.zeros(1, 1, 5, 5, dtype=torch.float64), torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    y = SR.ppeg_side(xg, [w7, z5, z3], [torch.zeros(1, dtype=torch.float64)] * 3)
    want = xg[:, 0] + torch.stack([sum(w7[0, 0, 3 + (j // 2) - (i // 2), 3 + (j % 2) - (i % 2)] * xg[j, 0] for j in range(4))
                                   for i in range(4)])
    assert float((y[:, 0] - want).abs().max()) < 1e-12


def test_float64_reference_keeps_every_judged_gradient_above_the_floor():
    """the step cases new to this suite (N = 36, act none): max |ref64| > 1e-4 for the logits, all 25 gradients and dx"""
    for input_dim, act, N in ((64, "gelu", 36), (64, "none", 37)):
        state, x = TC.model_inputs(input_dim, N)
        p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in state.items()}
        xd = torch.from_numpy(x).double().requires_grad_(True)
        logits = SR.transmil_step(xd, p, act)
        F.cross_entropy(logits[None], torch.tensor([GC.LABEL])).backward()
        assert float(logits.abs().max()) > 1e-4
        for k, v in {**p, "dx": xd}.items():
            assert float(v.grad.abs().max()) > 1e-4, (act, N, k)
