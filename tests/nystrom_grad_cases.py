"""Case lists and seeded cotangents shared by tests/test_nystrom_grad_cpu.py, tests/test_nystrom_grad_gpu.py and
tools/make_golden_transmil_grad.py (the backward of Nystrom attention and the training path of TransMIL)."""
import numpy as np

from rrt_mil_amd import synth

M = 256                      # landmarks
# sequence length -> what a backward kernel can get wrong there (l = ceil(n / 256), pad = 256 l - n)
LENGTHS = {
    2: "a stencil window wider than the data",
    17: "239 all-zero landmarks with exactly tied column sums",
    255: "one pad row",
    256: "no pad",
    257: "a landmark that is half pad, half real: its 1 / l share also lands on the dropped pad row",
    513: "l = 3 with 85 landmarks that are all pad",
    1030: "l = 5 with 50 landmarks that are all pad",
    2600: "pad % l != 0 at l = 11; several chunks of partial records (44 token tiles: 22 chunks of 2), merged in chunk order",
}
GAINS = (1.0, 6.0)
SMALL, WIDE = (128, 2), (512, 8)                                    # (dim, heads)
# (dim, heads, n, gain); the (512, 8) cases put the global den over eight heads
STAGE_CASES = [(*SMALL, n, g) for n in LENGTHS for g in GAINS] + [(*WIDE, 257, 6.0), (*WIDE, 2600, 6.0)]
PINV_ITERATIONS = (1, 6)
RESIDUAL = (True, False)
STAGES = ("output", "zav", "landmark_attn", "pinv_sim", "landmarks")

# (input_dim, act, N): TransMIL(input_dim, 2, False, act) in eval() with grad on, cross-entropy against LABEL
MODEL_CASES = [(64, "gelu", n) for n in (1, 3, 10, 37, 250, 1000)] + [(1024, "relu", 1000)]
LABEL = 1

# what tests/golden/transmil_grad.npz holds (the reference's own float64 gradients)
GOLDEN_ATTN_CASES = [(*SMALL, 17, 6.0), (*SMALL, 257, 6.0), (*SMALL, 1030, 1.0)]
GOLDEN_MODEL_CASES = [(64, "gelu", 3), (64, "gelu", 37), (64, "gelu", 250)]
GOLDEN_ROWS = 32             # every 32nd row of a parameter gradient ...
GOLDEN_ROWS_WIDE = 256       # ... every 256th of the matrices with 2^16 entries and more (to_qkv / to_out at width 512)


def cotangent(name, shape):
    """a seeded N(0, 1) cotangent: d_o, d_z, d_av, dy, ... of a case"""
    return synth.normal(f"nystrom_grad/{name}", tuple(shape))


def case_key(dim, heads, n, gain):
    return f"d{dim}_h{heads}_n{n}_g{int(gain)}"


def model_key(input_dim, act, N):
    return f"i{input_dim}_{act}_n{N}"


def golden_rows(g):
    """the rows of a gradient the golden holds: g as [shape[0], -1], strided"""
    g2 = g.reshape(g.shape[0], -1)
    return g2[::GOLDEN_ROWS_WIDE if g2.numel() >= 65536 else GOLDEN_ROWS]


def rel_grad(got, ref):
    """max |got - ref| / max |ref| in float64: relative to the gradient's own largest entry"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())
