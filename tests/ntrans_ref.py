"""Restatement, in plain torch ops written from the maths, of what the Nystrom ablations of RRTEncoder compute: Nystrom
attention on a BATCH of sequences (one pseudo-inverse scale over the whole batch and all heads) and the two encoder modes
around it -- attn='ntrans' (modules/rrt.py:49-58: a whole-bag NystromAttention per layer) and region_attn='ntrans'
(modules/rmsa.py:167-230: NystromAttention inside the regions, the regions as its batch).  Parametrised by dtype: in float64 it
is the reference value (pinned to the reference's own float64 run by tests/golden/ntrans_*.npz), in float32 on the CPU it gives
the error e32 a correct fp32 evaluation has on the same inputs.  Built on tests/nystrom_ref.py; geometry from
oracle/rrt_oracle.py.  Imports without a device.

Batched stage tensors use the layouts of the C ABI: qkv [b, np, 3 h d] (q scaled, each item's pad rows in FRONT),
ql / kl / av / wz [b, h, m, d], a2 / z [b, h, m, m], o [b, np, h d]."""
import math
import os
import sys

import torch
import torch.nn.functional as F

import nystrom_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import rrt_oracle as O  # noqa: E402

NYS_KEYS = ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias", "res_conv.weight")
rel_err = R.rel_err


def _t(a, dtype):
    """numpy -> a CPU tensor; a tensor stays on its device (tools/bench_ntrans.py runs the restatement on the GPU)"""
    return torch.as_tensor(a).to(dtype=dtype)


# ------------------------------------------------------------------ batched stages
def per_item(fn, *tensors):
    return torch.stack([fn(*(t[i] for t in tensors)) for i in range(tensors[0].shape[0])])


def st_landmarks(qkv, heads):
    pairs = [R.st_landmarks(q, heads) for q in qkv]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


def st_landmark_sim(ql, kl):
    return (ql @ kl.transpose(-1, -2)).softmax(-1)


def st_landmark_attn(qkv, ql, heads):
    return per_item(lambda q, l: R.st_landmark_attn(q, l, heads), qkv, ql)


def pinv_iter(a2, iters):
    """a2 [b, h, m, m]: ONE initial scale, the maxima over all b * h matrices (torch.max over the whole tensor)"""
    b, h, m, _ = a2.shape
    return R.pinv_iter(a2.reshape(b * h, m, m), iters).reshape(b, h, m, m)


def pinv_iter_per_item(a2, iters):
    """what a host loop over the items would compute: a scale per item -- NOT the reference"""
    return per_item(lambda a: R.pinv_iter(a, iters), a2)


def st_zav(z, av):
    return z @ av


def st_output(qkv, kl, wz, heads, conv_w=None):
    """the stencil runs along each item's own padded sequence (zero rows at both of ITS ends)"""
    return per_item(lambda q, k, w: R.st_output(q, k, w, heads, conv_w), qkv, kl, wz)


def stages_from_qkv(qkv, heads, conv_w=None, iters=6):
    ql, kl = st_landmarks(qkv, heads)
    a2 = st_landmark_sim(ql, kl)
    av = st_landmark_attn(qkv, ql, heads)
    z = pinv_iter(a2, iters)
    wz = st_zav(z, av)
    return {"ql": ql, "kl": kl, "a2": a2, "av": av, "z": z, "wz": wz, "o": st_output(qkv, kl, wz, heads, conv_w)}


def nystrom_batched(x, p, heads, iters=6, residual=True, m=256, dtype=torch.float64):
    """x [b, n, dim], p = {to_qkv.weight, to_out.0.weight, to_out.0.bias, res_conv.weight} -> the stages, qkv and y [b, n, dim]"""
    x = _t(x, dtype)
    wq, wo, bo = (_t(p[k], dtype) for k in NYS_KEYS[:3])
    b, n, dim = x.shape
    d = wq.shape[0] // (3 * heads)
    pad = (m - n % m) % m
    xp = torch.cat([x.new_zeros(b, pad, dim), x], dim=1)            # the pad rows go in FRONT of every item
    qkv = xp @ wq.t()
    qkv = torch.cat([qkv[..., :heads * d] * d ** -0.5, qkv[..., heads * d:]], dim=-1)
    conv_w = _t(p["res_conv.weight"], dtype).reshape(heads, -1) if residual else None
    st = stages_from_qkv(qkv, heads, conv_w, iters)
    st["qkv"] = qkv
    st["y"] = (st["o"] @ wo.t() + bo)[:, pad:]
    return st


# ------------------------------------------------------------------ the encoder around it
def _ln(x, sd, pfx, dtype):
    return F.layer_norm(x, (x.shape[-1],), _t(sd[pfx + ".weight"], dtype), _t(sd[pfx + ".bias"], dtype))


def _act(h, name):
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0))) if name == "gelu" else torch.relu(h)


def _ffn(x, sd, pfx, act, dtype):
    g = lambda k: _t(sd[pfx + k], dtype)      # noqa: E731
    h = _act(_ln(x, sd, pfx + "norm2", dtype) @ g("mlp.fc1.weight").t() + g("mlp.fc1.bias"), act)
    return x + h @ g("mlp.fc2.weight").t() + g("mlp.fc2.bias")


def _msa(x, sd, pfx, heads, dtype):
    """plain multi-head attention without EPEG on x [batch, seq, D] (modules/rmsa.py:91-133): CR-MSA's inner attention"""
    g = lambda k: _t(sd[pfx + k], dtype)      # noqa: E731
    B, S, D = x.shape
    qkv = x @ g("qkv.weight").t()
    if pfx + "qkv.bias" in sd:
        qkv = qkv + g("qkv.bias")
    q, k, v = (t.reshape(B, S, heads, D // heads).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    a = ((q * (D // heads) ** -0.5) @ k.transpose(-1, -2)).softmax(-1)
    return (a @ v).transpose(1, 2).reshape(B, S, D) @ g("proj.weight").t() + g("proj.bias")


def _partition(u, N, H, s):
    """u [N, D] -> ([R, P, D], perm): zero rows appended to H * H, region-major slots"""
    perm = torch.from_numpy(O.partition_index(H, s))
    up = torch.cat([u, u.new_zeros(H * H - N, u.shape[1])])
    return up[perm].reshape(-1, s * s, u.shape[1]), perm


def _unpartition(z, perm, N):
    out = z.new_empty(perm.numel(), z.shape[-1])
    out[perm] = z.reshape(-1, z.shape[-1])
    return out[:N]


def _crmsa(x, sd, c, dtype):
    """modules/rmsa.py:290-337 on the fixed 8 x 8 grid: x + dispatch(MSA(combine(LN(x))))"""
    N, D = x.shape
    p = "cr_msa."
    H, s, _ = O.grid(N, 8, 0, 0, 0.0)
    V, perm = _partition(_ln(x, sd, p + "norm", dtype), N, H, s)                 # [R, P, D]
    lg = (V @ _t(sd[p + "attn.phi"], dtype)).transpose(1, 2)                     # [R, k, P]
    cw, dw = lg.softmax(-1), lg.softmax(1)
    mn, mx = lg.min(-1, keepdim=True).values, lg.max(-1, keepdim=True).values
    mm = (lg - mn) / (mx - mn + 1e-8)
    rep = (cw @ V).transpose(0, 1)                                               # [k, R, D]
    rep2 = _msa(rep, sd, p + "attn.attn.", c["crmsa_heads"], dtype)
    out = torch.einsum("rnp,nrd->rpd", mm * dw, rep2)
    x = x + _unpartition(out, perm, N)
    return _ffn(x, sd, p, c["ffn_act"], dtype) if c["ffn"] else x


def _pos(x, sd, kind, dtype):
    """PEG / PPEG (modules/emb_position.py:24-82): the tokens wrapped to an H x H grid (PPEG: zero rows up to 7 x 7), depth-wise
    convs with zero borders + identity, the first N tokens kept"""
    N, D = x.shape
    H = math.isqrt(N - 1) + 1 if N > 1 else 1
    xh = torch.cat([x, x[:H * H - N]])
    if kind == "ppeg" and H < 7:
        xh, H = torch.cat([xh, x.new_zeros(49 - H * H, D)]), 7
    img = xh.t().reshape(1, D, H, H)
    out = img
    for name in ("proj", "proj1", "proj2") if kind == "ppeg" else ("proj",):
        w = _t(sd[f"pos_embedding.{name}.weight"], dtype)
        b = _t(sd[f"pos_embedding.{name}.bias"], dtype) if f"pos_embedding.{name}.bias" in sd else None
        out = out + F.conv2d(img, w, b, padding=(w.shape[2] // 2, w.shape[3] // 2), groups=D)
    return out.reshape(D, H * H).t()[:N]


def nys_params(sd, pfx):
    return {k: sd[pfx + k] for k in NYS_KEYS}


def encoder(x, sd, cfg, dtype=torch.float64):
    """x [N, D], sd = the reference RRTEncoder's state_dict (numpy or torch), cfg = its constructor arguments (attn='ntrans' or
    region_attn='ntrans') -> y [N, D]"""
    c = dict(O._DEFAULTS, attn="rmsa", region_attn="native", trans_dim=64)
    c.update(cfg)
    assert not c["crmsa_mlp"]
    x = _t(x, dtype)
    x0, (N, D) = x, x.shape
    use_pos = c["pos"] in ("peg", "ppeg")
    if use_pos and c["pos_pos"] == -1:
        x = _pos(x, sd, c["pos"], dtype)
    for li in range(c["n_layers"] - 1):
        if use_pos and li == 1 and c["pos_pos"] == 0:
            x = _pos(x, sd, c["pos"], dtype)
        p = f"layers.{li}."
        u = _ln(x, sd, p + "norm", dtype)
        if c["attn"] == "ntrans":
            x = x + nystrom_batched(u[None], nys_params(sd, p + "attn."), c["n_heads"], dtype=dtype)["y"][0]
        else:
            assert c["region_attn"] == "ntrans"
            H, s, _ = O.grid(N, c["region_num"], c["region_size"], c["min_region_num"], c["min_region_ratio"])
            U, perm = _partition(u, N, H, s)
            z = nystrom_batched(U, nys_params(sd, p + "attn.attn."), c["n_heads"], dtype=dtype)["y"]
            x = x + _unpartition(z, perm, N)
        if c["ffn"]:
            x = _ffn(x, sd, p, c["ffn_act"], dtype)
    if c["cr_msa"]:
        x = _crmsa(x, sd, c, dtype)
    if c["all_shortcut"]:
        x = x + x0
    return _ln(x, sd, "norm", dtype)


def rrtmil(feats, sd, cfg, dtype=torch.float64):
    """RRTMIL (modules/rrt.py:204-245, relu embedding, DAttention with relu, not gated, no bias): feats [N, input_dim] ->
    logits [n_classes]"""
    g = lambda k: _t(sd[k], dtype)      # noqa: E731
    h = torch.relu(_t(feats, dtype) @ g("patch_to_emb.0.weight").t() + g("patch_to_emb.0.bias"))
    enc_sd = {k[len("online_encoder."):]: v for k, v in sd.items() if k.startswith("online_encoder.")}
    y = encoder(h, enc_sd, cfg, dtype)
    a = (torch.relu(y @ g("pool_fn.attention.attention.0.weight").t()) @ g("pool_fn.attention.attention.2.weight").t()).t()
    pooled = a.softmax(-1) @ y
    return (pooled @ g("predictor.weight").t() + g("predictor.bias"))[0]
