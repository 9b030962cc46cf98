"""What tests/golden/ntrans_grad.npz holds and how its rows are picked: shared by tools/make_golden_ntrans_grad.py and
tests/test_ntrans_train_cpu.py.  Inputs regenerate from tests/ntrans_cases.py, cotangents from tests/nystrom_grad_cases.py."""
import nystrom_grad_cases as GC

GOLDEN_ENCODER_CASES = ("bag_n300", "reg_n200_rn2")          # one per mode
GOLDEN_ATTN_CASE = "b3_n300"                                 # the batched attention
TRAIN_B_MAX = 2048                                           # the batched backward's bound on b (include/rrt_hip.h)


def cotangent(case, name, shape):
    return GC.cotangent(f"ntrans/{name}/{case}", tuple(shape))


def rows(name, g):
    """the rows of a gradient the golden holds: first and last row of dx (of every item, for a batch), every 32nd row of a
    parameter gradient as [shape[0], -1]"""
    if name == "dx":
        return g[..., [0, -1], :]
    return GC.golden_rows(g)
