"""Restatement of Nystrom attention and TransMIL in plain torch ops, written from the maths (the issue's "maths to reproduce"),
parametrised by dtype, returning every stage.  The yardstick of tests/test_transmil_{cpu,gpu}.py: in float64 it is the
reference value (pinned to the reference's own float64 run by tests/golden/transmil_*.npz), in float32 on the CPU it gives the
error e32 a correct fp32 evaluation has on the same inputs.  Imports without a device.

Stage tensors use the layouts of the C ABI (include/rrt_hip.h): qkv [np, 3 h d] with q scaled and the pad rows in FRONT,
ql / kl / av / wz [h, m, d], a2 / z [h, m, m], o [np, h d] (heads merged, before to_out).
"""
import math

import torch
import torch.nn.functional as F


def _t(a, dtype, device="cpu"):
    return torch.as_tensor(a).to(device=device, dtype=dtype)


def pinv_iter(a2, iters):
    """a2 [h, m, m] -> z: z0 = a2^T / (max row abs sum * max column abs sum), both maxima over all heads."""
    ab = a2.abs()
    z = a2.transpose(-1, -2) / (ab.sum(-1).max() * ab.sum(-2).max())
    eye = torch.eye(a2.shape[-1], dtype=a2.dtype, device=a2.device)
    for _ in range(iters):
        xz = a2 @ z
        z = 0.25 * z @ (13 * eye - xz @ (15 * eye - xz @ (7 * eye - xz)))
    return z


def split_heads(qkv, heads):
    """qkv [np, 3 h d] -> q, k, v [h, np, d]"""
    npad, d = qkv.shape[0], qkv.shape[1] // (3 * heads)
    return tuple(t.reshape(npad, heads, d).transpose(0, 1) for t in qkv.chunk(3, dim=-1))


def st_landmarks(qkv, heads, m=256):
    """means of l consecutive rows of q and of k (the divisor is always l): ql, kl [h, m, d]"""
    q, k, _ = split_heads(qkv, heads)
    l = qkv.shape[0] // m
    return q.reshape(heads, m, l, -1).sum(2) / l, k.reshape(heads, m, l, -1).sum(2) / l


def st_landmark_sim(ql, kl):
    return (ql @ kl.transpose(-1, -2)).softmax(-1)


def st_landmark_attn(qkv, ql, heads):
    """softmax(ql k^T) v over ALL np keys: the pad keys have logit 0 and take their share of the denominator"""
    _, k, v = split_heads(qkv, heads)
    return (ql @ k.transpose(-1, -2)).softmax(-1) @ v


def st_zav(z, av):
    return z @ av


def st_output(qkv, kl, wz, heads, conv_w=None):
    """o [np, h d] = softmax(q kl^T) wz + conv(v), heads merged; conv_w [h, ks]: a cross-correlation along the padded
    sequence with zero rows at both ends, one filter per head"""
    q, _, v = split_heads(qkv, heads)
    npad = qkv.shape[0]
    out = (q @ kl.transpose(-1, -2)).softmax(-1) @ wz
    if conv_w is not None:
        ks = conv_w.shape[1]
        vp = F.pad(v, (0, 0, ks // 2, ks // 2))
        for j in range(ks):
            out = out + conv_w[:, j, None, None] * vp[:, j:j + npad]
    return out.transpose(0, 1).reshape(npad, -1)


def peak_logit(qkv, ql, kl, heads):
    q, k, _ = split_heads(qkv, heads)
    return max(float((a @ b.transpose(-1, -2)).abs().max()) for a, b in ((q, kl), (ql, kl), (ql, k)))


def stages_from_qkv(qkv, heads, conv_w=None, iters=6, m=256):
    """Everything behind the qkv linear: qkv [np, 3 h d] (q scaled, pad rows zero) -> dict of stage tensors."""
    ql, kl = st_landmarks(qkv, heads, m)
    a2 = st_landmark_sim(ql, kl)
    av = st_landmark_attn(qkv, ql, heads)
    z = pinv_iter(a2, iters)
    wz = st_zav(z, av)
    o = st_output(qkv, kl, wz, heads, conv_w)
    return {"ql": ql, "kl": kl, "a2": a2, "av": av, "z": z, "wz": wz, "o": o, "peak": peak_logit(qkv, ql, kl, heads)}


def nystrom(x, p, heads, iters=6, residual=True, m=256, dtype=torch.float64, device="cpu"):
    """x [n, dim] (already normalised) and p = {to_qkv.weight, to_out.0.weight, to_out.0.bias, res_conv.weight} ->
    dict: the stages above plus qkv [np, 3 h d] and y [n, dim]."""
    x = _t(x, dtype, device)
    wq, wo, bo = (_t(p[k], dtype, device) for k in ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias"))
    n, d = x.shape[0], wq.shape[0] // (3 * heads)
    pad = (m - n % m) % m
    xp = torch.cat([x.new_zeros(pad, x.shape[1]), x])                # the pad rows go in FRONT
    qkv = xp @ wq.t()
    qkv = torch.cat([qkv[:, :heads * d] * d ** -0.5, qkv[:, heads * d:]], dim=1)   # q scaled before the landmarks
    conv_w = _t(p["res_conv.weight"], dtype, device).reshape(heads, -1) if residual else None
    st = stages_from_qkv(qkv, heads, conv_w, iters, m)
    st["qkv"] = qkv
    st["y"] = (st["o"] @ wo.t() + bo)[pad:]
    return st


def transmil(x, sd, act, dtype=torch.float64, device="cpu", heads=8):
    """x [N, input_dim], sd = the TransMIL state_dict (numpy or torch) -> {logits [n_classes], feat [1 + H^2, 512]}"""
    g = lambda k: _t(sd[k], dtype, device)      # noqa: E731
    h = _t(x, dtype, device) @ g("_fc1.0.weight").t() + g("_fc1.0.bias")
    if act == "relu":
        h = torch.relu(h)
    elif act == "gelu":
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    N, D = h.shape
    H = math.isqrt(N - 1) + 1 if N > 1 else 1                          # ceil(sqrt(N))
    h = torch.cat([g("cls_token").reshape(1, D), h, h[:H * H - N]])   # wrap, then the cls token in front

    def layer(h, name):
        ln = F.layer_norm(h, (D,), g(name + ".norm.weight"), g(name + ".norm.bias"))
        p = {k: sd[f"{name}.attn.{k}"] for k in ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias", "res_conv.weight")}
        return h + nystrom(ln, p, heads, dtype=dtype, device=device)["y"]

    h = layer(h, "layer1")
    img = h[1:].t().reshape(1, D, H, H)
    pe = img
    for name, k in (("proj", 7), ("proj1", 5), ("proj2", 3)):
        pe = pe + F.conv2d(img, g(f"pos_layer.{name}.weight"), g(f"pos_layer.{name}.bias"), padding=k // 2, groups=D)
    h = torch.cat([h[:1], pe.reshape(D, H * H).t()])
    h = layer(h, "layer2")
    row0 = F.layer_norm(h[:1], (D,), g("norm.weight"), g("norm.bias"))
    return {"logits": (row0 @ g("_fc2.weight").t() + g("_fc2.bias"))[0], "feat": h}


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|) in float64"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))
