"""Restatement of the attention map: one query row of the Nystrom-approximated attention matrix, and TransMIL's class-token
maps around it, in plain torch ops on top of tests/nystrom_ref.py, parametrised by dtype.  In float64 it is the reference value
(pinned to the reference's own ``return_attn=True`` run by tests/golden/transmil_attn_row.npz at lengths with n % 256 == 0,
where the reference's row 0 is a real row); in float32 on the CPU it gives the error e32 a correct fp32 evaluation has on the
same inputs.  Imports without a device.

Per head, for query row t of the unpadded sequence (pad = np - n zero rows in front):
    a1      = softmax(q[pad + t] kl^T)                     [m]
    r       = a1 z                                         [m]
    lse3_i  = logsumexp_j(ql_i . k_j) over ALL np keys     [m]
    attn[j] = sum_i r_i exp(ql_i . k_j - lse3_i)           j = 0 .. np - 1
The pad keys keep their share (the n real columns do not sum to 1), and entries can be negative.
"""
import math

import torch
import torch.nn.functional as F

import nystrom_ref as R


def lse3_of(qkv, ql, heads):
    """row log-sum-exp of ql k^T over all np keys: [h, m]"""
    _, k, _ = R.split_heads(qkv, heads)
    return torch.logsumexp(ql @ k.transpose(-1, -2), dim=-1)


def st_attn_row(qkv, ql, kl, z, lse3, row_padded, heads):
    """the stage: (r [h, m], attn [h, np]) from the stage tensors, row_padded = pad + t"""
    q, k, _ = R.split_heads(qkv, heads)
    a1 = (q[:, row_padded:row_padded + 1] @ kl.transpose(-1, -2)).softmax(-1)        # [h, 1, m]
    r = (a1 @ z)[:, 0]                                                               # [h, m]
    a3 = torch.exp(ql @ k.transpose(-1, -2) - lse3[..., None])                       # [h, m, np]
    return r, (r[:, None, :] @ a3)[:, 0]


def attn_row(st, heads, row, n):
    """row `row` of the unpadded sequence from R.nystrom's dict -> {r [h, m], lse3 [h, m], full [h, np], attn [h, n]}"""
    pad = st["qkv"].shape[0] - n
    lse3 = lse3_of(st["qkv"], st["ql"], heads)
    r, full = st_attn_row(st["qkv"], st["ql"], st["kl"], st["z"], lse3, pad + row, heads)
    return {"r": r, "lse3": lse3, "full": full, "attn": full[:, pad:]}


def fold(rows, N):
    """rows [..., 1 + H*H] (the cls token's row over [cls, h_0 .. h_{N-1}, h_0 .. h_{H*H-N-1}]) -> [..., N]: without the cls
    column, the wrapped rows' columns added to their patches"""
    out = rows[..., 1:1 + N].clone()
    wrap = rows.shape[-1] - 1 - N
    out[..., :wrap] += rows[..., 1 + N:]
    return out


def transmil_attn(x, sd, act, dtype=torch.float64, device="cpu", heads=8):
    """R.transmil with the class token's row of both layers: {logits, feat, rows [2, heads, 1 + H*H], attn [2, heads, N]}"""
    g = lambda k: R._t(sd[k], dtype, device)      # noqa: E731
    h = R._t(x, dtype, device) @ g("_fc1.0.weight").t() + g("_fc1.0.bias")
    if act == "relu":
        h = torch.relu(h)
    elif act == "gelu":
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    N, D = h.shape
    H = math.isqrt(N - 1) + 1 if N > 1 else 1
    h = torch.cat([g("cls_token").reshape(1, D), h, h[:H * H - N]])
    rows = []

    def layer(h, name):
        ln = F.layer_norm(h, (D,), g(name + ".norm.weight"), g(name + ".norm.bias"))
        p = {k: sd[f"{name}.attn.{k}"] for k in ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias", "res_conv.weight")}
        st = R.nystrom(ln, p, heads, dtype=dtype, device=device)
        rows.append(attn_row(st, heads, 0, h.shape[0])["attn"])
        return h + st["y"]

    h = layer(h, "layer1")
    img = h[1:].t().reshape(1, D, H, H)
    pe = img
    for name, k in (("proj", 7), ("proj1", 5), ("proj2", 3)):
        pe = pe + F.conv2d(img, g(f"pos_layer.{name}.weight"), g(f"pos_layer.{name}.bias"), padding=k // 2, groups=D)
    h = torch.cat([h[:1], pe.reshape(D, H * H).t()])
    h = layer(h, "layer2")
    row0 = F.layer_norm(h[:1], (D,), g("norm.weight"), g("norm.bias"))
    rows = torch.stack(rows)
    return {"logits": (row0 @ g("_fc2.weight").t() + g("_fc2.bias"))[0], "feat": h, "rows": rows, "attn": fold(rows, N)}


def rel_err_max(got, ref, scale=None):
    """max |got - ref| / max |ref| in float64 (NOT max(1, ...): the entries of a row are about 1 / n); ``scale`` replaces
    max |ref| where a test states another yardstick"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    s = float(ref.abs().max()) if scale is None else float(scale)
    return float((got - ref).abs().max() / s)
