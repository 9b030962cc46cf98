"""Case lists shared by tests/test_transmil_cpu.py, tests/test_transmil_gpu.py and tools/make_golden_transmil.py."""
from rrt_mil_amd import synth

M = 256                      # landmarks
CONFIGS = ((128, 2), (512, 8))                       # (dim, heads)
# sequence length -> what a kernel can get wrong there (l = ceil(n / 256), pad = 256 l - n)
LENGTHS = {
    2: "a stencil window wider than the data",
    17: "239 all-zero landmarks",
    255: "one pad row",
    256: "no pad",
    257: "odd pad: one landmark is half pad, half real",
    512: "no pad, l = 2",
    513: "pad 255 at l = 3",
    1030: "pad 250 at l = 5",
    2600: "pad % l != 0 again, several key chunks, several token tiles per head",
}
GAINS = (1.0, 6.0)
ATTN_CASES = [(dim, heads, n, gain) for dim, heads in CONFIGS for n in LENGTHS for gain in GAINS]
STAGES = ("landmarks", "landmark_sim", "landmark_attn", "pinv", "zav", "output")
PINV_ITERATIONS = (1, 6)
PEAK_RANGE = (20.0, 80.0)    # peak |logit| of the float64 run at gain 6

# the cases whose stage tensors the goldens hold (every STAGE_ROWS-th landmark row)
STAGE_GOLDEN_CASES = [(128, 2, 17, 6.0), (128, 2, 257, 6.0)]
STAGE_ROWS = 32

# (input_dim, act, N): TransMIL(input_dim, 2, False, act)
MODEL_CASES = [(64, "gelu", n) for n in (1, 3, 10, 36, 37, 250, 1000, 2500)] + [(1024, "relu", 1000)]
MODEL_WHY = {1: "H = 1", 3: "a wrapped row", 10: "H = 4 < 7: the PPEG side trap", 36: "H = 6", 37: "H = 7",
             250: "n = 257", 1000: "H = 32", 2500: "n = 2501"}


def pad_of(n):
    return (M - n % M) % M


def attn_inputs(dim, heads, n, gain, residual=True):
    return synth.nystrom_state(dim, heads, gain=gain, residual=residual), synth.nystrom_input(n, dim)


def model_inputs(input_dim, N):
    """(state_dict as numpy, bag [N, input_dim]); the cls token has sigma 0.5 so that row 0 matters"""
    return synth.transmil_state(input_dim, 2, cls_sigma=0.5), synth.bag(N, input_dim, tag="transmil")
