"""Case lists and closed-form inputs of the DTFD-MIL tests (tests/test_dtfd_cpu.py checks the goldens against the restatement
on the CPU; tests/test_segment_pool_gpu.py and tests/test_dtfd_gpu.py run the device side; tools/make_golden_dtfd.py records
the reference's answers).  Importing this module needs no device."""
import numpy as np

from rrt_mil_amd import synth

INPUT_DIM, INNER_DIM, HIDDEN = 64, 512, 128
# whole-model cases: the reference's DTFD(rrt=False) on one bag of n instances; `seed` keys the bag and seeds random.shuffle.
# Every value of n in {8, 37, 300}, group in {1, 3, 8}, n_classes in {2, 4} and every distill mode appears.  The seeds were
# chosen by tools/make_golden_dtfd.py --search so that every group of every case has a unique highest and lowest CAM
# probability, clear of the runner-up by 64 x the reference's own fp32 error (the tool asserts it when it records).
CASES = {
    "n8_g8_c2_maxmin": dict(n=8, group=8, n_classes=2, distill="MaxMinS", seed=0),
    "n8_g3_c2_maxs": dict(n=8, group=3, n_classes=2, distill="MaxS", seed=0),
    "n37_g3_c2_maxmin": dict(n=37, group=3, n_classes=2, distill="MaxMinS", seed=0),
    "n37_g8_c4_maxs": dict(n=37, group=8, n_classes=4, distill="MaxS", seed=0),
    "n37_g1_c2_afs": dict(n=37, group=1, n_classes=2, distill="AFS", seed=0),
    "n300_g8_c2_maxmin": dict(n=300, group=8, n_classes=2, distill="MaxMinS", seed=0),
    "n300_g3_c4_afs": dict(n=300, group=3, n_classes=4, distill="AFS", seed=0),
    "n300_g1_c4_maxmin": dict(n=300, group=1, n_classes=4, distill="MaxMinS", seed=0),
}
TRAIN_CASES = ("n37_g3_c2_maxmin", "n37_g8_c4_maxs", "n300_g8_c2_maxmin", "n300_g3_c4_afs")
LABEL = dict(label=1, censorship=0)            # an observed event in bin 1: both terms of the loss carry a gradient
GRAD_SAMPLES = 48                              # entries of every gradient the golden keeps (beside its sums)


def model_kwargs(case):
    c = CASES[case]
    return dict(input_dim=INPUT_DIM, inner_dim=INNER_DIM, n_classes=c["n_classes"], group=c["group"], distill=c["distill"])


def shapes_of(n_classes, input_dim=INPUT_DIM):
    """ordered {state_dict key: shape} of DTFD without an encoder"""
    def attention(pre):
        return {pre + "attention_V.0.weight": (HIDDEN, INNER_DIM), pre + "attention_V.0.bias": (HIDDEN,),
                pre + "attention_U.0.weight": (HIDDEN, INNER_DIM), pre + "attention_U.0.bias": (HIDDEN,),
                pre + "attention_weights.weight": (1, HIDDEN), pre + "attention_weights.bias": (1,)}
    sh = {"classifier.fc.weight": (n_classes, INNER_DIM), "classifier.fc.bias": (n_classes,)}
    sh.update(attention("attention."))
    sh["dimReduction.fc1.weight"] = (INNER_DIM, input_dim)
    sh.update(attention("UClassifier.attention."))
    sh.update({"UClassifier.classifier.fc.weight": (n_classes, INNER_DIM), "UClassifier.classifier.fc.bias": (n_classes,)})
    return sh


def state(n_classes, input_dim=INPUT_DIM, tag="dtfd"):
    """Closed-form parameters under the reference's keys.  Weights N(0, 1) * gain / sqrt(fan_in): gain 3 on both score Linears
    (``attention_weights``: an attention that is visibly non-uniform inside a pseudo-bag) and 6 on the tier-1 classifier's
    weight (the CAM logits are w_i * (mid_i . W_c) with w_i ~ 1 / n: a visible spread of p over a pseudo-bag); biases uniform
    in +-0.1."""
    out = {}
    for key, shape in shapes_of(n_classes, input_dim).items():
        name = f"{tag}/c{n_classes}/{key}"
        if key.endswith(".bias"):
            out[key] = synth.uniform(name, shape, -0.1, 0.1)
        else:
            gain = 3.0 if "attention_weights" in key else (6.0 if key == "classifier.fc.weight" else 1.0)
            out[key] = (synth.normal(name, shape) * (gain / np.sqrt(shape[-1]))).astype(np.float32)
    return out


def state_sum(st):
    return float(sum(np.asarray(v, np.float64).sum() for v in st.values()))


def bag(case):
    c = CASES[case]
    return synth.bag(c["n"], INPUT_DIM, tag=f"dtfd/{case}/s{c['seed']}", nonneg=True)


def grad_summary(g):
    """what the golden keeps of one gradient tensor: [sum, sum |.|, max |.|] and GRAD_SAMPLES evenly spread entries (float64)"""
    g = np.asarray(g, np.float64).reshape(-1)
    idx = np.unique(np.linspace(0, g.size - 1, min(GRAD_SAMPLES, g.size)).round().astype(np.int64))
    return np.concatenate([[g.sum(), np.abs(g).sum(), np.abs(g).max()], g[idx]])


# ---- the stage entries alone (tests/test_segment_pool_gpu.py): (n, group) around the chunk of 32 positions
# groups of 1 (n == group), of 1 and 2 (n == group + 1), of 31 / 32 / 33 / 64 / 65 members and mixed q / q + 1 sizes
STAGE_SHAPES = ((1, 1), (8, 8), (9, 8), (64, 64), (65, 64), (31, 1), (32, 1), (33, 1), (64, 1), (65, 1), (95, 3), (97, 3),
                (130, 2), (259, 8), (4099, 1), (4099, 3), (4099, 8), (4099, 64))
STAGE_DIMS = (32, 512, 2048)
STAGE_CLASSES = (1, 2, 4, 8)
SCORE_PATTERNS = ("mild", "peaked", "offset+", "offset-", "flat", "pairs")
PERMS = ("none", "reversed", "shuffle")


def stage_mid(n, dim, tag="mid"):
    return synth.bag(n, dim, tag=f"dtfd/stage/{tag}", nonneg=True)


def stage_cls_w(c, dim):
    return (synth.normal(f"dtfd/stage/cls/{c}x{dim}", (c, dim)) * (6.0 / np.sqrt(dim))).astype(np.float32)


def stage_scores(pattern, n):
    base = synth.normal(f"dtfd/stage/a/{pattern}/{n}", (n,)).astype(np.float32)
    if pattern == "mild":
        return base
    if pattern == "peaked":
        return (base * np.float32(50.0 / max(1e-6, np.abs(base).max()))).astype(np.float32)
    if pattern == "offset+":
        return base + np.float32(100)
    if pattern == "offset-":
        return base - np.float32(100)
    if pattern == "flat":
        return np.full(n, 0.25, np.float32)
    if pattern == "pairs":                       # neighbours share a score
        return np.repeat(base[::2], 2)[:n].copy()
    raise KeyError(pattern)


def stage_perm(kind, n):
    if kind == "none":
        return None
    if kind == "reversed":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    return np.argsort(synth.uniform(f"dtfd/stage/perm/{n}", (n,), 0.0, 1.0), kind="stable").astype(np.int64)
