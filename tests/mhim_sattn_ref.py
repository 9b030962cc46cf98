"""CPU restatement of MHIM-MIL with the TransMIL baseline (the reference's Survival/models/MHIM/network.py with
baseline='selfattn') in float64 or fp32: the yardstick of tests/test_mask_select_vote_gpu.py and tests/test_mhim_sattn_gpu.py,
pinned to the reference's own run by tests/test_mhim_sattn_cpu.py (tools/make_golden_mhim_sattn.py).

The vote restates rrt_mask_select_vote_f32's contract (include/rrt_hip.h): mhim_ref.order per head, the votes, a lexsort by
(-vote, index).  SAttention is written on tests/nystrom_ref.py and tests/transmil_attn_ref.py; it takes the kept rows in an
explicit order, and ``ref_row=True`` reads the reference's row (row 0 of the front-padded sequence) where the library reads the
cls token's own.  Importing this module needs no device."""
import numpy as np
import torch
import torch.nn.functional as F

import mhim_ref as MR
import nystrom_ref as NR
import transmil_attn_ref as TA
from mhim_ref import ema, rel_err  # noqa: F401  (the tests take them from here)

PRE = "online_encoder."


# ---------------------------------------------------------------------- selection
def orders(a):
    """every head's order, ascending and descending: {largest: [order of head h]} (it does not depend on k: compute it once per a)"""
    return {largest: [MR.order(row, largest) for row in np.asarray(a)] for largest in (False, True)}


def votes(a, largest, k, cache=None):
    """a [heads, n] -> vote [n]: the number of heads that hold a token among the first k of their own order"""
    a = np.asarray(a)
    v = np.zeros(a.shape[1], dtype=np.int64)
    for h, row in enumerate(a):
        v[(cache[bool(largest)][h] if cache is not None else MR.order(row, largest))[:k]] += 1
    return v


def fused_order(vote):
    """the tokens by vote descending, equal votes by index"""
    return np.lexsort((np.arange(vote.size), -vote))


def select_vote(a, stages, invert, cache=None):
    """rrt_mask_select_vote_f32: a [heads, n], stages = [(largest, k, pick or None)] -> (ids [n] int64, count, mask [n] uint8);
    cache = orders(a)"""
    n = np.asarray(a).shape[1]
    sel = np.zeros(n, dtype=bool)
    for largest, k, pick in stages:
        cand = fused_order(votes(a, largest, k, cache))[:k]
        sel[cand if pick is None else cand[np.asarray(pick).astype(bool)]] = True
    kept = sel if invert else ~sel
    ids = np.concatenate([np.nonzero(kept)[0], np.nonzero(~kept)[0]]).astype(np.int64)
    return ids, int(kept.sum()), (~kept).astype(np.uint8)


def get_mask(ps, attn, perms, select_inv=False, **ratios):
    """mhim_ref.get_mask on per-head rows attn [heads, ps] -> (len_keep, ids [ps]), ids[:len_keep] the kept instances ascending"""
    perms = list(perms)
    stages = []
    for largest, k, m in MR.stage_plan(ps, **ratios):
        stages.append((largest, k, None if m is None else MR.pick_of(perms.pop(0), k, m)))
    assert not perms, "more permutations than stages that draw one"
    if not stages:
        return ps, None
    ids, count, _ = select_vote(attn, stages, select_inv)
    return count, ids


def threshold_property(a, largest, k, chosen):
    """what every valid answer to 'the k tokens of the most votes' shares, whatever it does with ties: exactly k tokens, every
    token above the threshold vote among them, none below it -> (ok, size of the tie class at the threshold)"""
    v = votes(a, largest, k)
    thr = np.sort(v)[::-1][k - 1]
    chosen = np.asarray(chosen).reshape(-1).astype(np.int64)     # (the reference's ids are floats when its kept part is empty)
    inside = np.zeros(v.size, dtype=bool)
    inside[chosen] = True
    ok = chosen.size == k and np.unique(chosen).size == k and bool(inside[v > thr].all()) and not bool(inside[v < thr].any())
    return ok, int((v == thr).sum())


# ---------------------------------------------------------------------- the model
def ppeg(x, st, dtype):
    """network.py:259-293 on x [n, D]: the ceil(sqrt(n)) square, wrapped; a side below 7 lifted to 7 with zero rows"""
    n, D = x.shape
    H = int(np.ceil(np.sqrt(n)))
    add = H * H - n
    x = torch.cat([x, x[:add]])
    if H < 7:
        H = 7
        x = torch.cat([x, x.new_zeros(H * H - x.shape[0], D)])
    img = x.t().reshape(1, D, H, H)
    out = img
    for name in ("proj", "proj1", "proj2"):
        w = st[f"{PRE}pos_embedding.{name}.weight"]
        out = out + F.conv2d(img, w, st[f"{PRE}pos_embedding.{name}.bias"], padding=w.shape[-1] // 2, groups=D)
    return out.reshape(D, H * H).t()[:n]


def sattention(y, st, heads, return_attn=False, ref_row=False):
    """SAttention.forward at dropout 0 on the embedded rows y [n, 512] (torch, already in the kept order; on y's device) -> (the
    cls row (1, 512), [a1, a2] each (1, heads, n) or None)"""
    D = y.shape[1]
    h = torch.cat([st[PRE + "cls_token"].reshape(1, D), y])
    rows = []

    def layer(h, name):
        ln = F.layer_norm(h, (D,), st[f"{PRE}{name}.norm.weight"], st[f"{PRE}{name}.norm.bias"])
        p = {k: st[f"{PRE}{name}.attn.{k}"] for k in ("to_qkv.weight", "to_out.0.weight", "to_out.0.bias", "res_conv.weight")}
        s = NR.nystrom(ln, p, heads, dtype=ln.dtype, device=ln.device)
        if return_attn:
            n_seq = h.shape[0]
            pad = s["qkv"].shape[0] - n_seq
            lse3 = TA.lse3_of(s["qkv"], s["ql"], heads)
            _, full = TA.st_attn_row(s["qkv"], s["ql"], s["kl"], s["z"], lse3, 0 if ref_row else pad, heads)
            rows.append(full[:, pad + 1:][None])
        return h + s["y"]

    h = layer(h, "layer1")
    h = torch.cat([h[:1], ppeg(h[1:], st, h.dtype)])
    h = layer(h, "layer2")
    out = F.layer_norm(h[:1], (D,), st[PRE + "norm.weight"], st[PRE + "norm.bias"])
    return out, (rows if return_attn else None)


def embed(x, st, act):
    return MR._act(F.linear(x, st["patch_to_emb.0.weight"], st["patch_to_emb.0.bias"]), act.lower() if act.lower() in ("relu", "gelu") else "")


def teacher(x, state, heads, act="relu", dtype=torch.float64, ref_row=False):
    """forward_teacher without dropout -> (the cls row (1, 512), [a1, a2])"""
    st = MR.to_state(state, dtype)
    with torch.no_grad():
        return sattention(embed(torch.as_tensor(np.asarray(x)).to(dtype), st, act), st, heads, True, ref_row)


def forward_test(x, state, heads, act="relu", dtype=torch.float64, ref_row=False):
    """-> (logits (1, C), [a1, a2])"""
    st = MR.to_state(state, dtype)
    with torch.no_grad():
        feat, rows = sattention(embed(torch.as_tensor(np.asarray(x)).to(dtype), st, act), st, heads, True, ref_row)
        return F.linear(feat, st["predictor.weight"], st["predictor.bias"]), rows


def student(x, state, kept, heads, teacher_feat=None, act="relu", temp_t=1., temp_s=1., dtype=torch.float64, grad=False):
    """MHIM.forward at dropout 0 on the rows `kept` (indices in the order they enter the sequence, or None = the whole bag) ->
    dict logits (1, C), feat (1, 512), cls_loss (a tensor, or 0. without a teacher row); grad=True: leaves ``x_leaf`` / ``params``"""
    st = MR.to_state(state, dtype, grad)
    x = torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        y = embed(x, st, act)                                  # the reference embeds the whole bag, then gathers
        if kept is not None:
            y = y[torch.as_tensor(np.asarray(kept), dtype=torch.int64)]
        feat, _ = sattention(y, st, heads)
        out = {"feat": feat, "logits": F.linear(feat, st["predictor.weight"], st["predictor.bias"])}
        out["cls_loss"] = 0. if teacher_feat is None else MR.cl_loss(feat, torch.as_tensor(np.asarray(teacher_feat)).to(dtype).detach(),
                                                                     temp_t, temp_s)
    if grad:
        out["x_leaf"], out["params"] = x, st
    return out
