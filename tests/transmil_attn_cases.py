"""Case lists shared by tests/test_transmil_attn_cpu.py, tests/test_transmil_attn_gpu.py and
tools/make_golden_transmil_attn.py (inputs come from tests/transmil_cases.py: attn_inputs, model_inputs)."""
from transmil_cases import GAINS, PEAK_RANGE  # noqa: F401

# (dim, heads) -> sequence length -> what the row kernels can get wrong there
LENGTHS = {
    (128, 2): {1: "the only key", 2: "two keys", 17: "239 all-zero landmarks", 255: "one pad row", 256: "no pad",
               257: "a landmark that is half pad", 513: "pad 255 at l = 3", 1030: "pad 250 at l = 5"},
    (512, 8): {257: "8 heads, a landmark that is half pad", 2600: "several key tiles per head, 8 heads"},
}
ATTN_CASES = [(dim, heads, n, gain) for (dim, heads), ns in LENGTHS.items() for n in ns for gain in GAINS]


def rows_of(n):
    """the query rows a case is checked at: the first, the middle and the last"""
    return sorted({0, n // 2, n - 1})


# the reference's own return_attn is row 0 without column 0 only where n % 256 == 0 (elsewhere it reads a zero pad row)
GOLDEN_CASES = [(128, 2, 256, 1.0), (128, 2, 512, 6.0), (512, 8, 256, 6.0)]

# (input_dim, act, N): TransMIL(input_dim, 2, False, act)
MODEL_CASES = [(64, "gelu", n) for n in (1, 3, 10, 37, 250, 1000)] + [(1024, "relu", 1000)]
MODEL_WHY = {1: "H = 1: the cls token and one patch", 3: "H = 2: one wrapped row to fold", 10: "H = 4: six wrapped rows, the PPEG side trap",
             37: "H = 7: twelve wrapped rows", 250: "n = 257", 1000: "H = 32: 24 wrapped rows, n = 1025"}


def golden_key(dim, heads, n, gain):
    return f"d{dim}_h{heads}_n{n}_g{int(gain)}"
