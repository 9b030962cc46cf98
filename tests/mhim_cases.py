"""Case lists and closed-form inputs of the MHIM-MIL tests (tests/test_mhim_cpu.py checks the goldens against the restatement
on the CPU; tests/test_mask_select_gpu.py and tests/test_mhim_gpu.py run the device side; tools/make_golden_mhim.py records the
reference's answers).  Importing this module needs no device."""
import numpy as np

from rrt_mil_amd import synth

INPUT_DIM, N_CLASSES = 64, 2
# whole-model cases: the reference's MHIM(baseline='attn', dropout=0) on one bag of N instances
CASES = {
    "n37_std": dict(n=37, mask_ratio=0.7, mask_ratio_l=0.2, mask_ratio_h=0.02, mask_ratio_hr=0., select_inv=False),
    "n300_std": dict(n=300, mask_ratio=0.7, mask_ratio_l=0.2, mask_ratio_h=0.02, mask_ratio_hr=0., select_inv=False),
    "n300_inv": dict(n=300, mask_ratio=0.7, mask_ratio_l=0.2, mask_ratio_h=0.02, mask_ratio_hr=0., select_inv=True),
    "n300_hr": dict(n=300, mask_ratio=0.5, mask_ratio_l=0.2, mask_ratio_h=0.1, mask_ratio_hr=0.5, select_inv=False,
                    act="gelu", da_act="tanh"),
    "n37_hr_inv": dict(n=37, mask_ratio=0.5, mask_ratio_l=0.2, mask_ratio_h=0.1, mask_ratio_hr=0.5, select_inv=True),
    "n300_high_only": dict(n=300, mask_ratio=0., mask_ratio_l=0., mask_ratio_h=0.3, mask_ratio_hr=0.5, select_inv=False),
}
RATIO_KEYS = ("mask_ratio", "mask_ratio_l", "mask_ratio_h", "mask_ratio_hr")
GRAD_CASES = ("n300_std", "n300_hr")
# the parameters of Survival/main.py:138-149 (the flagship use) and a small schedule for the scheduler's equality test
MAIN_PARAMS = dict(num_epoch=200, niter_per_ep=100, input_dim=1024, mlp_dim=512, mask_ratio=0.7, mask_ratio_l=0.2,
                   mask_ratio_h=0.02, baseline="attn", teacher_init=None)
SCHEDULES = ((0.02, 0., 3, 5, 0, 0), (0.9999, 1., 3, 5, 0, 1.), (0.5, 0.1, 4, 7, 2, 0.05))

# ---- the selection kernels alone (tests/test_mask_select_gpu.py)
SELECT_NS = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 4099, 20011)
PATTERNS = ("distinct", "levels5", "equal", "zeros", "inf", "nan")
ROW_DIMS = (4, 64, 1024)
ROW_NS = (1, 65, 4099)


def model_kwargs(case):
    c = CASES[case]
    kw = dict(input_dim=INPUT_DIM, mlp_dim=512, n_classes=N_CLASSES, dropout=0., baseline="attn", act=c.get("act", "relu"),
              da_act=c.get("da_act", "relu"), select_inv=c["select_inv"])
    kw.update({k: c[k] for k in RATIO_KEYS})
    return kw


def state(shapes, who):
    """closed-form parameters for the MHIM keys `shapes` {key: shape}; who = 'student' / 'teacher' (two different sets)"""
    return synth.bagmil_head_state({k: tuple(s) for k, s in shapes.items()}, f"mhim/{who}")


def shapes_of(input_dim=INPUT_DIM, n_classes=N_CLASSES):
    pre = "online_encoder.attention."
    return {"patch_to_emb.0.weight": (512, input_dim), "patch_to_emb.0.bias": (512,), pre + "attention_a.0.weight": (128, 512),
            pre + "attention_b.0.weight": (128, 512), pre + "attention_c.weight": (1, 128), "predictor.weight": (n_classes, 512),
            "predictor.bias": (n_classes,)}


def bag(case):
    return synth.bag(CASES[case]["n"], INPUT_DIM, tag=f"mhim/{case}", nonneg=True)


def scores(pattern, n):
    """fp32 scores [n] of one value pattern of the selection tests"""
    base = synth.normal(f"mhim/select/{pattern}/{n}", (n,)).astype(np.float32)
    if pattern == "distinct":
        return (np.argsort(np.argsort(base, kind="stable")).astype(np.float32) - n // 2) / np.float32(max(n, 1))
    if pattern == "levels5":
        return np.floor(np.abs(base) * 2.5).clip(0, 4).astype(np.float32) - 2
    if pattern == "equal":
        return np.full(n, 0.25, dtype=np.float32)
    if pattern == "zeros":                                   # +0, -0 and a few values either side of them
        out = np.where(base > 0.3, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        out[::7] = np.float32(1e-30)
        out[3::11] = np.float32(-1e-30)
        return out
    if pattern == "inf":
        out = base.copy()
        out[::5], out[2::9] = np.inf, -np.inf
        return out
    if pattern == "nan":
        out = np.round(base * 4).astype(np.float32) / 4      # ties among the numbers too
        out[1::4] = np.nan
        out[::13] = np.float32(np.nan) * -1
        return out
    raise KeyError(pattern)


def select_settings(n):
    """[(stages, invert)] for a bag of n: stages = [(largest, k, pick kind)], pick kind None / 'sparse' / 'zero'"""
    k3 = max(1, n // 3)
    return [
        ([(False, 1, None)], False),
        ([(True, k3, None)], True),
        ([(False, n, "sparse")], False),
        ([(True, n, "zero")], False),
        ([(False, k3, None), (True, k3, "sparse")], False),
        ([(False, n, "sparse"), (False, k3, None), (True, max(1, (2 * n) // 3), "sparse")], False),      # overlapping selections
        ([(False, n, "sparse"), (False, k3, None), (True, n, "sparse")], True),
        ([(True, 1, "zero"), (True, n, None)], True),
    ]


def pick(kind, k, tag):
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros(k, dtype=np.uint8)
    p = (synth.uniform(f"mhim/pick/{tag}/{k}", (k,), 0.0, 1.0) < 0.3).astype(np.uint8)
    p[::2] *= np.uint8(3)                                    # any non-zero byte selects
    return p
