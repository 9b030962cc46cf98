"""CPU restatement of MHIM-MIL (the reference's Survival/models/MHIM/network.py with baseline='attn') in float64 or fp32: the
yardstick of tests/test_mask_select_gpu.py and tests/test_mhim_gpu.py, pinned to the reference's own run by
tests/test_mhim_cpu.py (tools/make_golden_mhim.py).

Selection restates rrt_mask_select_f32's contract (include/rrt_hip.h) as a stable sort: by value, equal values by index
(-0.0 == +0.0), NaN greater than every number.  The three-stage arithmetic of get_mask / select_mask_fn is the reference's, in
Python floats.  Importing this module needs no device."""
import numpy as np
import torch
import torch.nn.functional as F

from bagmil_ref import rel_err  # noqa: F401  (the tests take it from here)

PRE = "online_encoder.attention."
KEYS = ("patch_to_emb.0.weight", "patch_to_emb.0.bias", PRE + "attention_a.0.weight", PRE + "attention_b.0.weight",
        PRE + "attention_c.weight", "predictor.weight", "predictor.bias")


# ---------------------------------------------------------------------- selection
def order(a, largest):
    """the indices of `a` in the order of a stage: descending if largest, equal values by index, NaN greatest"""
    v = np.asarray(a, dtype=np.float64).reshape(-1)
    idx = np.arange(v.size)
    nan = np.isnan(v)
    val = np.where(nan, 0.0, v) + 0.0                       # (+ 0.0: -0.0 becomes +0.0, whatever the sort compares)
    if largest:
        return np.lexsort((idx, -val, ~nan))                # NaNs first, then by falling value, then by index
    return np.lexsort((idx, val, nan))


def select(a, stages, invert):
    """rrt_mask_select_f32: stages = [(largest, k, pick or None)], pick a 0/1 array [k] -> (ids [n] int64, count, mask [n] uint8)"""
    n = np.asarray(a).size
    sel = np.zeros(n, dtype=bool)
    for largest, k, pick in stages:
        cand = order(a, largest)[:k]
        sel[cand if pick is None else cand[np.asarray(pick).astype(bool)]] = True
    kept = sel if invert else ~sel
    ids = np.concatenate([np.nonzero(kept)[0], np.nonzero(~kept)[0]]).astype(np.int64)
    return ids, int(kept.sum()), (~kept).astype(np.uint8)


def pick_of(perm, k, m):
    """a stage's pick from its permutation of 0..k-1: zeros, then pick[perm[:m]] = 1"""
    p = np.zeros(k, dtype=np.uint8)
    p[np.asarray(perm)[:m]] = 1
    return p


def stage_sizes(ps, ratio, random_ratio):
    """one stage's sizes in the reference's float arithmetic (network.py:480-518) -> (k candidates, m of them drawn at random,
    or None = all of them).  The candidates' share is ratio / (random_ratio + 1e-8); when that exceeds 1 the whole bag is the
    candidate list and `ratio` itself becomes the share drawn from it."""
    share = ratio / (random_ratio + 1e-8)
    draw = random_ratio
    if share > 1:
        share, draw = 1., ratio
    k = int(np.ceil(ps * share))
    return k, (int(np.ceil(k * draw)) if draw < 1. else None)


def stage_plan(ps, mask_ratio=0., mask_ratio_l=0., mask_ratio_h=0., mask_ratio_hr=0.):
    """get_mask's stages (network.py:537-575) for a bag of ps instances -> [(largest, k, m)] in the reference's order: the
    random stage (random_ratio = 0.001), the low stage, the high stage (random_ratio = mask_ratio_hr)"""
    plan = []
    if mask_ratio > 0.:
        plan.append((False,) + stage_sizes(ps, mask_ratio, 0.001))
    if mask_ratio_l > 0.:
        plan.append((False,) + stage_sizes(ps, mask_ratio_l, 1.))
    if mask_ratio_h > 0.:
        plan.append((True,) + stage_sizes(ps, mask_ratio_h, mask_ratio_hr))
    return plan


def get_mask(ps, attn, perms, select_inv=False, **ratios):
    """-> (len_keep, ids [ps]) with ids[:len_keep] the kept instances ascending; `perms`: the permutations in call order"""
    perms = list(perms)
    stages = []
    for largest, k, m in stage_plan(ps, **ratios):
        stages.append((largest, k, None if m is None else pick_of(perms.pop(0), k, m)))
    assert not perms, "more permutations than stages that draw one"
    if not stages:
        return ps, None
    ids, count, _ = select(attn, stages, select_inv)
    return count, ids


# ---------------------------------------------------------------------- the model
def _act(t, name):
    return {"relu": F.relu, "gelu": F.gelu, "tanh": torch.tanh}.get(name, lambda v: v)(t)


def to_state(state, dtype, grad=False):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(grad) for k, v in state.items()}


def gated_pool(y, st):
    """AttentionGated (bias=False) on y (n, 512) -> (pooled (1, 512), attn (n,), raw (n,)); st['da_act'] is set by the caller"""
    a = _act(F.linear(y, st[PRE + "attention_a.0.weight"]), st["da_act"])
    b = torch.sigmoid(F.linear(y, st[PRE + "attention_b.0.weight"]))
    raw = F.linear(a * b, st[PRE + "attention_c.weight"])[:, 0]
    attn = F.softmax(raw, dim=0)
    return attn[None] @ y, attn, raw


def embed(x, st, act):
    return _act(F.linear(x, st["patch_to_emb.0.weight"], st["patch_to_emb.0.bias"]), act.lower() if act.lower() in ("relu", "gelu") else "")


def cl_loss(student_feat, teacher_feat, temp_t=1., temp_s=1.):
    """SoftTargetCrossEntropy_v2 on (1, 512) rows"""
    return torch.sum(-F.softmax(teacher_feat / temp_t, dim=-1) * F.log_softmax(student_feat / temp_s, dim=-1), dim=-1).mean()


def teacher(x, state, act="relu", da_act="relu", dtype=torch.float64):
    """forward_teacher without dropout -> (pooled (1, 512), attn (1, n))"""
    st = dict(to_state(state, dtype), da_act=da_act)
    with torch.no_grad():
        pooled, attn, _ = gated_pool(embed(torch.as_tensor(np.asarray(x)).to(dtype), st, act), st)
    return pooled, attn[None]


def forward_test(x, state, act="relu", da_act="relu", dtype=torch.float64):
    """-> (logits (1, C), attn (1, n), raw (1, n))"""
    st = dict(to_state(state, dtype), da_act=da_act)
    with torch.no_grad():
        pooled, attn, raw = gated_pool(embed(torch.as_tensor(np.asarray(x)).to(dtype), st, act), st)
        return F.linear(pooled, st["predictor.weight"], st["predictor.bias"]), attn[None], raw[None]


def student(x, state, kept, teacher_feat=None, act="relu", da_act="relu", temp_t=1., temp_s=1., dtype=torch.float64, grad=False):
    """MHIM.forward at dropout 0 on the kept rows (`kept`: indices, or None = the whole bag) -> dict logits (1, C), pooled
    (1, 512), cls_loss (a tensor, or 0. without a teacher row); grad=True: leaves as ``x_leaf`` / ``params``"""
    st = to_state(state, dtype, grad)
    x = torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        y = embed(x, st, act)                                  # the reference embeds the whole bag, then gathers
        if kept is not None:
            y = y[torch.as_tensor(np.asarray(kept), dtype=torch.int64)]
        pooled, _, _ = gated_pool(y, dict(st, da_act=da_act))
        out = {"pooled": pooled, "logits": F.linear(pooled, st["predictor.weight"], st["predictor.bias"])}
        out["cls_loss"] = 0. if teacher_feat is None else cl_loss(pooled, torch.as_tensor(np.asarray(teacher_feat)).to(dtype).detach(),
                                                                  temp_t, temp_s)
    if grad:
        out["x_leaf"], out["params"] = x, st
    return out


def ema(teacher_state, student_state, mm):
    """ema_update in float64: mm * k + (1 - mm) * q"""
    return {k: float(mm) * np.asarray(teacher_state[k], np.float64) + (1. - float(mm)) * np.asarray(student_state[k], np.float64)
            for k in teacher_state}
