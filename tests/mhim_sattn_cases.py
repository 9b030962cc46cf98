"""Case lists and closed-form inputs of the MHIM-MIL tests with the TransMIL baseline (rrt_mil_amd.mhim_sattn):
tests/test_mhim_sattn_cpu.py checks the goldens against the restatement on the CPU, tests/test_mhim_sattn_gpu.py runs the device
side, tools/make_golden_mhim_sattn.py records the reference's answers.  Importing this module needs no device."""
import numpy as np

from rrt_mil_amd import synth

INPUT_DIM, N_CLASSES, D = 64, 2, 512
STD = dict(mask_ratio=0.7, mask_ratio_l=0.2, mask_ratio_h=0.02, mask_ratio_hr=0.)
# whole-model cases: the reference's MHIM(baseline='selfattn', dropout=0) on one bag of N instances.
#   N = 37: the student keeps about 10 rows -- a sequence padded to 256, PPEG's side lifted to 7
#   N = 255, 511: (N + 1) % 256 == 0, where the reference's attention row is the cls token's own
CASES = {
    "n37_std": dict(n=37, head=2, select_inv=False, **STD),
    "n255_inv": dict(n=255, head=2, select_inv=True, **STD),
    "n300_hr": dict(n=300, head=2, mask_ratio=0.5, mask_ratio_l=0.2, mask_ratio_h=0.1, mask_ratio_hr=0.5, select_inv=False,
                    act="gelu"),
    "n255_std_h8": dict(n=255, head=8, select_inv=False, **STD),
    "n511_high_only": dict(n=511, head=2, mask_ratio=0., mask_ratio_l=0., mask_ratio_h=0.3, mask_ratio_hr=0.5, select_inv=False,
                           attn_layer=-1),
}
RATIO_KEYS = ("mask_ratio", "mask_ratio_l", "mask_ratio_h", "mask_ratio_hr")
GRAD_CASES = ("n37_std", "n300_hr")
CLS_ROW_CASES = tuple(c for c, v in CASES.items() if (v["n"] + 1) % 256 == 0)
# the stage property of the vote (every token above the threshold vote is in, none below it): N x heads
PROPERTY_NS, PROPERTY_HEADS = (37, 255, 300, 511), (2, 8)
VOTE_HEADS = (1, 2, 3, 8, 16)
ARRANGEMENTS = ("tagged", "same", "negated", "all_equal")


def model_kwargs(case):
    c = CASES[case]
    kw = dict(input_dim=INPUT_DIM, mlp_dim=512, n_classes=N_CLASSES, dropout=0., baseline="selfattn", act=c.get("act", "relu"),
              select_inv=c["select_inv"], head=c["head"], attn_layer=c.get("attn_layer", 0))
    kw.update({k: c[k] for k in RATIO_KEYS})
    return kw


def ratios(case):
    return {k: CASES[case][k] for k in RATIO_KEYS}


def state(head, who, input_dim=INPUT_DIM, n_classes=N_CLASSES):
    """closed-form parameters for the 25 keys of mhim_sattn.MHIM; who = 'student' / 'teacher' (two different sets).  The
    attention layers are synth.nystrom_state at dim 512 with `head` heads of 64; the cls token is of visible size."""
    t = f"mhim_sattn/{who}/h{head}"
    u = synth.uniform
    out = {"patch_to_emb.0.weight": (u(f"{t}/emb.w", (D, input_dim), -1, 1) / np.sqrt(input_dim)),
           "patch_to_emb.0.bias": u(f"{t}/emb.b", (D,), -0.05, 0.05)}
    pre = "online_encoder."
    out[pre + "cls_token"] = synth.normal(f"{t}/cls", (1, 1, D)) * 0.5
    out[pre + "norm.weight"] = 1.0 + u(f"{t}/norm.w", (D,), -0.25, 0.25)
    out[pre + "norm.bias"] = u(f"{t}/norm.b", (D,), -0.1, 0.1)
    for name in ("layer1", "layer2"):
        out[f"{pre}{name}.norm.weight"] = 1.0 + u(f"{t}/{name}.norm.w", (D,), -0.25, 0.25)
        out[f"{pre}{name}.norm.bias"] = u(f"{t}/{name}.norm.b", (D,), -0.1, 0.1)
        for k, v in synth.nystrom_state(D, head, 64, 33, tag=f"{t}/{name}").items():
            out[f"{pre}{name}.attn.{k}"] = v
    for name, kk in (("proj", 7), ("proj1", 5), ("proj2", 3)):
        out[f"{pre}pos_embedding.{name}.weight"] = u(f"{t}/pos.{name}.w", (D, 1, kk, kk), -1.0 / kk, 1.0 / kk)
        out[f"{pre}pos_embedding.{name}.bias"] = u(f"{t}/pos.{name}.b", (D,), -0.05, 0.05)
    out["predictor.weight"] = u(f"{t}/pred.w", (n_classes, D), -1, 1) / np.sqrt(D)
    out["predictor.bias"] = u(f"{t}/pred.b", (n_classes,), -0.05, 0.05)
    return {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}


def bag(case):
    return synth.bag(CASES[case]["n"], INPUT_DIM, tag=f"mhim_sattn/{case}", nonneg=True)


def property_bag(n, seed):
    """a bag of the stage-property list; the golden records the first seed whose teacher rows are pairwise distinct per head
    (the reference's row at (n + 1) % 256 != 0 is nearly flat: 300 fp32 values within 3e-5 of each other collide now and then)"""
    return synth.bag(n, INPUT_DIM, tag=f"mhim_sattn/property/{n}/{seed}", nonneg=True)


def head_rows(arrangement, pattern, n, heads):
    """fp32 rows [heads, n] of the vote tests: mhim_cases.scores patterns, one draw per head, or an arrangement of heads"""
    import mhim_cases as MC
    if arrangement == "tagged":                              # every head its own row of the pattern: a rotation and a sign
        base = MC.scores(pattern, n)
        rows = [np.roll(base, (h * 7) % max(n, 1)) * np.float32(-1 if h % 3 == 2 else 1) for h in range(heads)]
        return np.stack(rows).astype(np.float32)
    if arrangement == "same":                                # votes in {0, heads}
        return np.tile(MC.scores(pattern, n), (heads, 1))
    if arrangement == "negated":                             # head 1 = -head 0, then alternating
        base = MC.scores(pattern, n)
        return np.stack([base if h % 2 == 0 else -base for h in range(heads)]).astype(np.float32)
    if arrangement == "all_equal":                           # the first k indices win in every head
        return np.full((heads, n), 0.25, dtype=np.float32)
    raise KeyError(arrangement)
