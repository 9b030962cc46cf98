"""What the one-call TransMIL training step adds to the restatement tests/nystrom_ref.py: explicit dropout masks, the single-row
forms of layer 2's tail, and the two glue adjoints (sequence assembly, TransMIL's PPEG on an exact side x side grid).  Plain
torch ops parametrised by dtype, differentiable by autograd; float64 is the reference, fp32 on the CPU gives e32.  Imports
without a device."""
import math

import torch
import torch.nn.functional as F

import nystrom_ref as R

DROP_TAGS = {"fc1": 200, "attn1": 201, "attn2": 202}      # include/rrt_hip.h, the step's drop_layer tags
# (input_dim, act, N) -> the geometry it covers
STEP_CASES = [(64, "gelu", 1), (64, "gelu", 3), (64, "gelu", 36), (64, "gelu", 37), (64, "gelu", 250), (64, "gelu", 1000),
              (1024, "relu", 1000)]
STEP_WHY = {1: "side 1, no wrap", 3: "wrap 1", 36: "side 6: every PPEG kernel larger than the grid, no wrap", 37: "side 7, wrap 12",
            250: "257 rows, 255 pad rows, l = 2", 1000: "1025 rows, l = 5"}
DROPOUT_CASES = [(64, "relu", 37), (64, "relu", 250)]
PPEG_CASES = [(s, 64) for s in (1, 2, 3, 6, 7, 8, 32)] + [(8, 512)]     # (side, C)
# (n_padded, row) -> what the stencil does there
ROW_POSITIONS = {(256, 0): "stencil cut at the front", (256, 255): "stencil cut at the back", (512, 255): "straddling",
                 (512, 256): "straddling"}


def side_of(N):
    return math.isqrt(N - 1) + 1 if N > 1 else 1


def act_fn(h, act):
    if act == "relu":
        return torch.relu(h)
    if act == "gelu":
        return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return h


def assemble(hpre, cls, act, mask=None):
    """hpre [N, D] (_fc1's Linear output), cls [D] -> seq [1 + H * H, D] = [cls | h | wrap], h = act(hpre) * mask"""
    h = act_fn(hpre, act)
    if mask is not None:
        h = h * mask.to(h.dtype)
    N = h.shape[0]
    H = side_of(N)
    return torch.cat([cls.reshape(1, -1), h, h[:H * H - N]])


def ppeg_side(x, ws, bs):
    """x [side * side, C] -> x + conv7(x) + conv5(x) + conv3(x) on the exact side x side grid, zero borders"""
    n, C = x.shape
    side = math.isqrt(n)
    img = x.t().reshape(1, C, side, side)
    pe = img
    for w, b in zip(ws, bs):
        pe = pe + F.conv2d(img, w, b, padding=w.shape[-1] // 2, groups=C)
    return pe.reshape(C, n).t()


def output_row(qkv, kl, wz, heads, conv_w, row):
    """one query row of the output stage, [h d]"""
    return R.st_output(qkv, kl, wz, heads, conv_w)[row]


def transmil_step(x, sd, act, dtype=torch.float64, masks=None, heads=8):
    """nystrom_ref.transmil with the step's three masks (multipliers keep / (1 - p): "fc1" [N, D], "attn1" [1 + H * H, D],
    "attn2" [D], any may be missing) and layer 2 read in row 0 alone -> logits [n_classes]"""
    g = lambda k: R._t(sd[k], dtype)      # noqa: E731
    m = masks or {}
    mk = lambda k: m[k].to(dtype) if k in m else None      # noqa: E731
    hpre = R._t(x, dtype) @ g("_fc1.0.weight").t() + g("_fc1.0.bias")
    N, D = hpre.shape
    H = side_of(N)
    h = assemble(hpre, g("cls_token"), act, mk("fc1"))

    def attn(h, name):
        ln = F.layer_norm(h, (D,), g(name + ".norm.weight"), g(name + ".norm.bias"))
        p = {k: sd[f"{name}.attn.{k}"] for k in ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias", "res_conv.weight")}
        return R.nystrom(ln, p, heads, dtype=dtype)["y"]

    y = attn(h, "layer1")
    h = h + (y * mk("attn1") if "attn1" in m else y)
    pe = ppeg_side(h[1:], [g(f"pos_layer.{n}.weight") for n in ("proj", "proj1", "proj2")],
                   [g(f"pos_layer.{n}.bias") for n in ("proj", "proj1", "proj2")])
    h = torch.cat([h[:1], pe])
    y = attn(h, "layer2")[0]
    row0 = h[0] + (y * mk("attn2") if "attn2" in m else y)
    row0 = F.layer_norm(row0[None], (D,), g("norm.weight"), g("norm.bias"))
    return (row0 @ g("_fc2.weight").t() + g("_fc2.bias"))[0]
