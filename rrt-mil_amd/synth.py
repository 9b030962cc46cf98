"""Closed-form synthetic parameters and bags (pure numpy, no RNG stream).

Every value is splitmix64(tensor-name hash, element index) mapped to a uniform,
so the golden-fixture generator (tools/make_golden.py, run next to the
reference), the tests and bench.py regenerate bit-identical arrays on any box
without sharing a torch RNG stream.

State-dict names / shapes are the reference's (modules/rrt.py:134-163,
modules/rmsa.py:57-89, :233-259); see SURVEY.md §3.3.
"""
import zlib
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(z: np.ndarray) -> np.ndarray:
    z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def uniform(name: str, shape, lo=-1.0, hi=1.0, dtype=np.float32) -> np.ndarray:
    """Deterministic U[lo,hi) array keyed by ``name``."""
    n = int(np.prod(shape)) if len(shape) else 1
    key = np.uint64(zlib.crc32(name.encode()) & 0xFFFFFFFF) << np.uint64(32)
    with np.errstate(over="ignore"):
        h = _splitmix64(key + np.arange(n, dtype=np.uint64))
    u = (h >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    return (lo + (hi - lo) * u).astype(dtype).reshape(shape)


def normal(name: str, shape, dtype=np.float32) -> np.ndarray:
    """Deterministic N(0,1) array (Box-Muller on two keyed uniforms)."""
    u1 = uniform(name + "/u1", shape, 0.0, 1.0, np.float64)
    u2 = uniform(name + "/u2", shape, 0.0, 1.0, np.float64)
    z = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
    return z.astype(dtype)


def encoder_state_shapes(mlp_dim=512, n_layers=2, n_heads=8, epeg=True, epeg_k=15,
                         cr_msa=True, crmsa_k=3, crmsa_mlp=False, qkv_bias=True,
                         epeg_bias=True, ffn=False, mlp_ratio=4., pos='none', peg_k=7, peg_1d=False,
                         peg_bias=True, epeg_2d=False, epeg_type='attn', **_unused):
    """Ordered {state_dict key: shape} of the default-path RRTEncoder."""
    D = mlp_dim
    sh = {"norm.weight": (D,), "norm.bias": (D,)}

    def inner(prefix, with_pe):
        sh[prefix + "qkv.weight"] = (3 * D, D)
        if qkv_bias:
            sh[prefix + "qkv.bias"] = (3 * D,)
        sh[prefix + "proj.weight"] = (D, D)
        sh[prefix + "proj.bias"] = (D,)
        if with_pe:                    # modules/rmsa.py:74-87: channels = heads ('attn') or features ('value_*')
            ch = n_heads if epeg_type == 'attn' else D
            sh[prefix + "pe.weight"] = (ch, 1, epeg_k, epeg_k if epeg_2d else 1)
            if epeg_bias:
                sh[prefix + "pe.bias"] = (ch,)

    def mlp(prefix):                       # TransLayer(ffn=True): norm2 + Mlp, modules/rrt.py:25-41,48,106
        if ffn:
            hid = int(D * mlp_ratio)
            sh[prefix + "norm2.weight"] = (D,)
            sh[prefix + "norm2.bias"] = (D,)
            sh[prefix + "mlp.fc1.weight"] = (hid, D)
            sh[prefix + "mlp.fc1.bias"] = (hid,)
            sh[prefix + "mlp.fc2.weight"] = (D, hid)
            sh[prefix + "mlp.fc2.bias"] = (D,)

    for i in range(n_layers - 1):
        sh[f"layers.{i}.norm.weight"] = (D,)
        sh[f"layers.{i}.norm.bias"] = (D,)
        inner(f"layers.{i}.attn.attn.", epeg)
        mlp(f"layers.{i}.")
    if cr_msa:
        sh["cr_msa.norm.weight"] = (D,)
        sh["cr_msa.norm.bias"] = (D,)
        inner("cr_msa.attn.attn.", False)
        if crmsa_mlp:
            sh["cr_msa.attn.phi.0.weight"] = (D // 4, D)
            sh["cr_msa.attn.phi.2.weight"] = (crmsa_k, D // 4)
        else:
            sh["cr_msa.attn.phi"] = (D, crmsa_k)
        mlp("cr_msa.")
    if pos in ("peg", "ppeg"):            # modules/emb_position.py:24-82 under pos_embedding.*
        for name, kk in (("proj", peg_k), ("proj1", 5), ("proj2", 3)):
            if name != "proj" and pos == "peg":
                continue
            sh[f"pos_embedding.{name}.weight"] = (D, 1, kk, 1 if peg_1d else kk)
            if peg_bias:
                sh[f"pos_embedding.{name}.bias"] = (D,)
    return sh


def encoder_state(**cfg):
    """Closed-form fp32 parameters, scaled like the reference's default inits
    (Linear/Conv ~ U(+-1/sqrt(fan_in)); LayerNorm gamma ~ 1+-0.25, beta ~ +-0.1
    so that gamma/beta mistakes show up in parity tests)."""
    out = {}
    for k, shape in encoder_state_shapes(**cfg).items():
        if k.endswith(("norm.weight", "norm2.weight")):
            out[k] = 1.0 + uniform(k, shape, -0.25, 0.25)
        elif k.endswith(("norm.bias", "norm2.bias")):
            out[k] = uniform(k, shape, -0.1, 0.1)
        elif k.startswith("pos_embedding.") and k.endswith(".weight"):
            b = 1.0 / np.sqrt(shape[2] * shape[3])
            out[k] = uniform(k, shape, -b, b)
        elif k.endswith("pe.weight"):
            b = 1.0 / np.sqrt(shape[2] * shape[3])
            out[k] = uniform(k, shape, -b, b)
        elif k.endswith("pe.bias"):
            out[k] = uniform(k, shape, -0.25, 0.25)
        elif k.endswith(".bias"):
            out[k] = uniform(k, shape, -0.05, 0.05)
        elif k.endswith("phi"):
            b = 1.0 / np.sqrt(shape[0])
            out[k] = uniform(k, shape, -3 * b, 3 * b)
        else:  # Linear weights (out, in)
            b = 1.0 / np.sqrt(shape[-1])
            out[k] = uniform(k, shape, -b, b)
    return out


def bag(n_tokens: int, dim: int = 512, tag: str = "bag", nonneg: bool = False) -> np.ndarray:
    """Synthetic (N, D) patch-embedding bag: N(0,1), or relu(N(0,1)) like pooled
    ResNet-50 features."""
    x = normal(f"{tag}/{n_tokens}x{dim}", (n_tokens, dim))
    return np.maximum(x, 0.0) if nonneg else x


def mil_state(input_dim=1024, n_classes=2, da_bias=False, da_gated=False, da_act="relu", **enc_cfg):
    """Closed-form parameters of RRTMIL (modules/rrt.py:204-225): encoder state under
    ``online_encoder.`` plus patch_to_emb / pool_fn / predictor tensors (state_dict names of
    modules/datten.py: ``attention.{0,2}`` -- ``{0,1}`` without an activation -- or the gated
    ``attention_a.0 / attention_b.0 / attention_c``)."""
    out = {"patch_to_emb.0.weight": uniform("mil/fc.w", (512, input_dim), -1, 1) / np.sqrt(input_dim),
           "patch_to_emb.0.bias": uniform("mil/fc.b", (512,), -0.05, 0.05)}
    out = {k: v.astype(np.float32) for k, v in out.items()}
    for k, v in encoder_state(**enc_cfg).items():
        out["online_encoder." + k] = v
    D = enc_cfg.get("mlp_dim", 512)
    w0 = (uniform("mil/da0", (128, D), -1, 1) / np.sqrt(D)).astype(np.float32)
    w2 = (uniform("mil/da2", (1, 128), -1, 1) / np.sqrt(128) * 4).astype(np.float32)
    if da_gated:
        names = ("pool_fn.attention.attention_a.0", "pool_fn.attention.attention_c")
        out["pool_fn.attention.attention_b.0.weight"] = (uniform("mil/dab", (128, D), -1, 1) / np.sqrt(D)).astype(np.float32)
        if da_bias:
            out["pool_fn.attention.attention_b.0.bias"] = uniform("mil/dabb", (128,), -0.05, 0.05)
    else:
        last = 2 if da_act in ("relu", "gelu", "tanh") else 1
        names = ("pool_fn.attention.attention.0", f"pool_fn.attention.attention.{last}")
    out[names[0] + ".weight"], out[names[1] + ".weight"] = w0, w2
    if da_bias:
        out[names[0] + ".bias"] = uniform("mil/da0b", (128,), -0.05, 0.05)
        out[names[1] + ".bias"] = uniform("mil/da2b", (1,), -0.05, 0.05)
    out["predictor.weight"] = (uniform("mil/pred.w", (n_classes, D), -1, 1) / np.sqrt(D)).astype(np.float32)
    out["predictor.bias"] = uniform("mil/pred.b", (n_classes,), -0.05, 0.05)
    return out


def clam_head_state(shapes, tag):
    """Closed-form parameters for a CLAM head (rrt_mil_amd.CLAM_SB / CLAM_MB without the encoder's entries): ``shapes`` is an
    ordered {state_dict key: shape}.  Weights N(0, 1) * gain / sqrt(fan_in) -- gain 1.2 on the score Linear (attention_c / the
    last Linear of Attn_Net.module), so that the attention over a bag is visibly non-uniform -- biases uniform in +-0.1,
    ``instance_loss_fn.labels`` = arange."""
    out = {}
    for key, shape in shapes.items():
        shape = tuple(shape)
        if key.endswith("labels"):
            out[key] = np.arange(shape[0], dtype=np.int64)
        elif key.endswith(".bias"):
            out[key] = uniform(f"clam/{tag}/{key}", shape, -0.1, 0.1)
        else:
            score = "attention_c" in key or (".module." in key and ".module.0." not in key)
            out[key] = (normal(f"clam/{tag}/{key}", shape) * ((1.2 if score else 1.0) / np.sqrt(shape[-1]))).astype(np.float32)
    return out


def dsmil_head_state(shapes, tag):
    """Closed-form parameters for a DSMIL head (rrt_mil_amd.MILNet without the encoder's entries): ``shapes`` is an ordered
    {state_dict key: shape}.  Weights N(0, 1) * gain / sqrt(fan_in) -- gain 1.5 on ``i_classifier`` (instance scores of O(1)
    on the encoder's LayerNorm-ed rows, so that the critical instances stand out) and 2.0 on ``b_classifier.q`` (the scores
    q . q_max / sqrt(128) are a product of two of them: an attention that is visibly non-uniform over the bag); biases
    uniform in +-0.1."""
    out = {}
    for key, shape in shapes.items():
        shape = tuple(shape)
        if key.endswith(".bias"):
            out[key] = uniform(f"dsmil/{tag}/{key}", shape, -0.1, 0.1)
        else:
            gain = 1.5 if key.startswith("i_classifier") else (2.0 if ".q." in key else 1.0)
            fan_in = int(np.prod(shape[1:]))
            out[key] = (normal(f"dsmil/{tag}/{key}", shape) * (gain / np.sqrt(fan_in))).astype(np.float32)
    return out


def bagmil_head_state(shapes, tag):
    """Closed-form parameters for an ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL head (without the encoder's entries):
    ``shapes`` is an ordered {state_dict key: shape}.  Weights N(0, 1) * gain / sqrt(fan_in) -- gain 1.5 on the score Linear
    of an attention pool (``attention.2`` / ``attention_c``: an attention that is visibly non-uniform over the bag) and on
    the last Linear of a ``head`` Sequential (MeanMIL / MaxMIL: instance scores of O(1), so that the maxima stand out), 2.0
    on ``W_q`` / ``W_k`` (their product is the confounder score); biases uniform in +-0.1; ``confounder_feat`` N(0, 0.7^2)."""
    head_last = max([int(k.split(".")[1]) for k in shapes if k.startswith("head.") and k.count(".") == 2], default=-1)
    out = {}
    for key, shape in shapes.items():
        shape = tuple(shape)
        name = f"bagmil/{tag}/{key}"
        if key == "confounder_feat":
            out[key] = (normal(name, shape) * 0.7).astype(np.float32)
        elif key.endswith(".bias"):
            out[key] = uniform(name, shape, -0.1, 0.1)
        else:
            score = key.startswith(("attention.2.", "attention_c.")) or key.startswith(f"head.{head_last}.")
            gain = 1.5 if score else (2.0 if key.startswith(("W_q.", "W_k.")) else 1.0)
            out[key] = (normal(name, shape) * (gain / np.sqrt(shape[-1]))).astype(np.float32)
    return out


K_ALIGN, K_NOISE = 0.33, 0.4    # nystrom_state: k rows = K_ALIGN * q rows + K_NOISE * their own draw


def nystrom_state(dim=512, heads=8, dim_head=64, residual_conv_kernel=33, gain=1.0, residual=True, tag="nys"):
    """Closed-form parameters of NystromAttention (modules/nystrom_attention.py:54-65): ``to_qkv.weight`` (no bias),
    ``to_out.0.{weight, bias}``, ``res_conv.weight``.  Linear weights U(+-1/sqrt(fan_in)); ``gain`` multiplies the q and the k
    rows of ``to_qkv`` (gain 6 on LayerNorm-ed rows peaks the three softmaxes: |logit| of a few tens); the conv taps are
    U(+-1/sqrt(k)), far from the delta a trained filter starts near, so that every tap counts."""
    inner = heads * dim_head
    wq = uniform(f"{tag}/to_qkv.w", (3 * inner, dim), -1, 1) / np.sqrt(dim)
    # the k rows lean on the q rows, as trained attention does: a token's logit with itself and its neighbours has a
    # systematic part, so that the peak |logit| depends little on how many tokens there are to take the maximum over
    wq[inner:2 * inner] = K_ALIGN * wq[:inner] + K_NOISE * wq[inner:2 * inner]
    wq[:2 * inner] *= gain
    out = {"to_qkv.weight": wq.astype(np.float32),
           "to_out.0.weight": (uniform(f"{tag}/to_out.w", (dim, inner), -1, 1) / np.sqrt(inner)).astype(np.float32),
           "to_out.0.bias": uniform(f"{tag}/to_out.b", (dim,), -0.05, 0.05)}
    if residual:
        out["res_conv.weight"] = (uniform(f"{tag}/res_conv.w", (heads, 1, residual_conv_kernel, 1), -1, 1) /
                                  np.sqrt(residual_conv_kernel)).astype(np.float32)
    return out


def nystrom_input(n, dim, tag="nys"):
    """(n, dim) rows shaped like a LayerNorm output whose neighbours are correlated (a slide's patches): a per-token N(0, 1)
    part plus a component that varies slowly along the sequence, so that the landmark means of long sequences keep a
    magnitude comparable to single rows."""
    t = np.arange(n, dtype=np.float64)[:, None]
    f = uniform(f"{tag}/in.f/{dim}", (1, dim), 0.5, 3.0, np.float64)
    ph = uniform(f"{tag}/in.p/{dim}", (1, dim), 0.0, 2 * np.pi, np.float64)
    slow = np.sqrt(2.0) * np.sin(2 * np.pi * f * t / max(n, 256) + ph)
    return (0.6 * normal(f"{tag}/in/{n}x{dim}", (n, dim), np.float64) + 0.8 * slow).astype(np.float32)


def transmil_state(input_dim=1024, n_classes=2, cls_sigma=0.5, tag="transmil"):
    """Closed-form parameters of TransMIL (modules/transmil.py:64-88), the reference's 25 state_dict keys: ``_fc1.0``,
    ``cls_token`` (N(0, cls_sigma^2): of visible size, so that row 0 matters), ``layer{1,2}.{norm, attn}``,
    ``pos_layer.{proj, proj1, proj2}``, ``norm``, ``_fc2``."""
    D = 512
    out = {"_fc1.0.weight": (uniform(f"{tag}/fc1.w", (D, input_dim), -1, 1) / np.sqrt(input_dim)).astype(np.float32),
           "_fc1.0.bias": uniform(f"{tag}/fc1.b", (D,), -0.05, 0.05),
           "cls_token": (normal(f"{tag}/cls", (1, 1, D)) * cls_sigma).astype(np.float32)}
    for name in ("layer1", "layer2"):
        out[f"{name}.norm.weight"] = 1.0 + uniform(f"{tag}/{name}.norm.w", (D,), -0.25, 0.25)
        out[f"{name}.norm.bias"] = uniform(f"{tag}/{name}.norm.b", (D,), -0.1, 0.1)
        for k, v in nystrom_state(D, 8, 64, 33, tag=f"{tag}/{name}").items():
            out[f"{name}.attn.{k}"] = v
    for name, kk in (("proj", 7), ("proj1", 5), ("proj2", 3)):
        out[f"pos_layer.{name}.weight"] = uniform(f"{tag}/pos.{name}.w", (D, 1, kk, kk), -1.0 / kk, 1.0 / kk)
        out[f"pos_layer.{name}.bias"] = uniform(f"{tag}/pos.{name}.b", (D,), -0.05, 0.05)
    out["norm.weight"] = 1.0 + uniform(f"{tag}/norm.w", (D,), -0.25, 0.25)
    out["norm.bias"] = uniform(f"{tag}/norm.b", (D,), -0.1, 0.1)
    out["_fc2.weight"] = (uniform(f"{tag}/fc2.w", (n_classes, D), -1, 1) / np.sqrt(D)).astype(np.float32)
    out["_fc2.bias"] = uniform(f"{tag}/fc2.b", (n_classes,), -0.05, 0.05)
    return {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}
