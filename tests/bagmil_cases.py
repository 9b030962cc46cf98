"""Case lists and closed-form inputs of the ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL tests (tests/test_bagmil_cpu.py
checks on the CPU that the lists cover what they claim; tests/test_bagmil_gpu.py runs them; tools/make_golden_bagmil.py
records the reference's answers for the whole-head cases).  Importing this module needs no device."""
import os

import numpy as np

from rrt_mil_amd import synth

ENC_CFG = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
HEADS = ("attmil", "gattmil", "ibmil", "meanmil", "maxmil")
# (module, class) -- the same names in the reference's modules/ and in the package
CLASS_OF = {"attmil": ("attmil", "DAttention"), "gattmil": ("attmil", "AttentionGated"), "ibmil": ("attmil_ibmil", "Dattention_ori"),
            "meanmil": ("mean_max", "MeanMIL"), "maxmil": ("mean_max", "MaxMIL")}
# AttentionGated and MaxMIL hard-code Linear(1024, 512); AttentionGated's classifier has 2 classes
INPUT_DIM = {"attmil": 128, "gattmil": 1024, "ibmil": 128, "meanmil": 128, "maxmil": 1024}
N_CLASSES = {"attmil": 2, "gattmil": 2, "ibmil": 2, "meanmil": 3, "maxmil": 3}
ACT = {"attmil": "gelu", "gattmil": "tanh", "ibmil": "relu", "meanmil": "gelu", "maxmil": "relu"}
N_CONF = 8                      # confounders of the whole-head IBMIL cases

# ---- kernels alone
# the sizes the mean pool's kernels switch at (csrc/internal.h): 32 rows per first-level partial, 64 partials per second-level
# one (so 2048 rows: above it the second level runs), 64 rows of dy per block of the adjoint
MEAN_CHUNK, MEAN_FAN, MEAN_BWD_ROWS = 32, 64, 64
MEAN_EDGES = (MEAN_CHUNK, MEAN_BWD_ROWS, MEAN_CHUNK * MEAN_FAN)
MEAN_ALL_LEVELS = 4097          # 129 first-level partials (the last of ONE row) -> 3 second-level ones (64, 64, 1) -> the final block
MEAN_NS = (1, 2, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, MEAN_ALL_LEVELS)
MEAN_DIMS = (32, 512, 2048)
MEAN_CS = (1, 2, 8)
DECONF_KS = (1, 2, 8, 64)
DECONF_SHAPES = ((512, 512, 128, 2), (32, 64, 4, 1), (2048, 2048, 512, 8))      # (dim, V, J, C)
DECONF_GAINS = (1.0, 6.0)       # mild: peak |logit| = 1 by construction; peaked: gain 6 on W_q and on W_k (|logit| up to 36)
PEAK_RANGE = (20.0, 80.0)

# ---- whole heads: (kind, with rrt, N)
WHOLE_CASES = [(k, False, n) for k in HEADS for n in (1, 2, 300) if not (k == "ibmil" and n == 1)] + \
              [(k, True, n) for k in HEADS for n in (30, 300, 1000)]
GRAD_CASES = [(k, True, 300) for k in HEADS]
AUTOCAST_CASES = [("attmil", True, 300), ("gattmil", True, 300), ("ibmil", True, 300)]
# MaxMIL margin: in float64 the two largest instance logits of every class are >= MARGIN * max |logit| apart.  The seed is
# part of the bag's tag; tests/test_bagmil_cpu.py checks the margin of every case below on the CPU.
MARGIN = 1e-3
SEED = {("maxmil", False, 1): 0, ("maxmil", False, 2): 0, ("maxmil", False, 300): 0, ("maxmil", True, 30): 0,
        ("maxmil", True, 300): 0, ("maxmil", True, 1000): 0}


def case_id(kind, rrt, n):
    return f"{kind}_{'rrt' if rrt else 'norrt'}_n{n}"


def mean_inputs(n, dim, c):
    """y with a column offset (a mean that is not ~0), classifier rows and bias"""
    y = synth.normal(f"bagmil/mean/y/{n}x{dim}", (n, dim)) + synth.uniform(f"bagmil/mean/off/{dim}", (1, dim), -1.0, 1.0)
    w = synth.normal(f"bagmil/mean/w/{c}x{dim}", (c, dim)) / np.float32(np.sqrt(dim))
    b = synth.uniform(f"bagmil/mean/b/{c}", (c,), -0.1, 0.1)
    d_logits = synth.uniform(f"bagmil/mean/dl/{c}", (c,), -1.0, 1.0)
    return y.astype(np.float32), w.astype(np.float32), b, d_logits


def deconf_inputs(dim, v, j, c, k, gain):
    """fp32 arrays (pooled, conf, q_w, q_b, k_w, k_b, head_w, head_b).  At gain 1 the largest |k_i . q| / sqrt(J) over the
    confounders is 1 (W_q carries the normalisation, computed in float64); ``gain`` multiplies both
    Linears (weights and biases): every logit grows by gain^2."""
    tag = f"bagmil/deconf/{dim}/{v}/{j}/{k}"
    pooled = synth.normal(tag + "/pooled", (dim,), np.float64)
    conf = synth.normal(tag + "/conf", (k, v), np.float64) * 0.7
    q_w = synth.normal(tag + "/q_w", (j, dim), np.float64) / np.sqrt(dim)
    k_w = synth.normal(tag + "/k_w", (j, v), np.float64) / np.sqrt(v)
    q_b = synth.uniform(tag + "/q_b", (j,), -0.1, 0.1, np.float64)
    k_b = synth.uniform(tag + "/k_b", (j,), -0.1, 0.1, np.float64)
    peak = np.abs((conf @ k_w.T + k_b) @ (q_w @ pooled + q_b)).max() / np.sqrt(j)
    q_w, q_b = q_w / peak, q_b / peak
    head_w = synth.normal(f"{tag}/head_w/{c}", (c, dim + v), np.float64) / np.sqrt(dim + v)
    head_b = synth.uniform(f"{tag}/head_b/{c}", (c,), -0.1, 0.1, np.float64)
    arrs = (pooled, conf, gain * q_w, gain * q_b, gain * k_w, gain * k_b, head_w, head_b)
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in arrs)


def conf_file(directory, k=N_CONF):
    """a confounder .npy as IBMIL's constructor loads it (the values are replaced by the state dict's buffer)"""
    path = os.path.join(str(directory), f"confounders_{k}.npy")
    if not os.path.exists(path):
        np.save(path, (synth.normal(f"bagmil/conf_file/{k}", (k, 512)) * 0.7).astype(np.float32))
    return path


def construct(classes, kind, rrt=None, dropout=0., act=None, conf_path=None, n_classes=None, input_dim=None, bias=True):
    """the head `kind` from `classes` {kind: class} (the package's or the reference's: the constructors are the same)"""
    act = ACT[kind] if act is None else act
    nc = N_CLASSES[kind] if n_classes is None else n_classes
    ind = INPUT_DIM[kind] if input_dim is None else input_dim
    cls = classes[kind]
    if kind == "attmil":
        return cls(ind, nc, dropout, act, rrt=rrt)
    if kind == "gattmil":
        return cls(512, act=act, bias=bias, dropout=bool(dropout), rrt=rrt)
    if kind == "ibmil":
        return cls(out_dim=nc, in_size=ind, dropout=dropout, confounder_path=conf_path, act=act, rrt=rrt)
    return cls(ind, n_classes=nc, dropout=bool(dropout), act=act, rrt=rrt)


def head_state(state_dict, tag):
    """closed-form values for a head's state_dict (keys and shapes as given): synth.bagmil_head_state for the head's own
    entries, synth.encoder_state under the encoder's prefix"""
    from bagmil_ref import rrt_prefix
    keys = list(state_dict)
    pre = rrt_prefix(keys)
    shapes = {k: tuple(state_dict[k].shape) for k in keys if not (pre and k.startswith(pre))}
    st = synth.bagmil_head_state(shapes, tag)
    if pre:
        st.update({pre + k: v for k, v in synth.encoder_state(**{k: v for k, v in ENC_CFG.items() if k != "region_num"}).items()})
    return {k: st[k] for k in keys}


def bag(kind, rrt, n):
    seed = SEED.get((kind, rrt, n), 0)
    return synth.bag(n, INPUT_DIM[kind], tag=f"bagmil/{case_id(kind, rrt, n)}/s{seed}", nonneg=True)
