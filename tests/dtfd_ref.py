"""Restatement of DTFD-MIL for the tests, written from the math (not from the reference's code).  Importing needs no device.

The stage functions (the kernels' contracts: tests/test_segment_pool_gpu.py) are numpy, float64 by default and fp32 on request
(``dtype=np.float32``: the e32 of the project's value rule).  The whole-model functions are torch on the CPU in the dtype of
the state they are given, so that autograd provides the training step's gradients in float64.

Notation: L = 512 embedding width, D = 128 attention hidden, C classes, G pseudo-bags.  Groups: the N rows, taken in the
order ``perm``, are split as np.array_split splits them: q = N // G, r = N % G; the first r groups hold q + 1 positions, the
others q."""
import numpy as np
import torch


def rel_err(got, ref):
    """max |got - ref| relative to max(1, max |ref|); NaNs must sit at the same places (else inf)"""
    got, ref = np.asarray(torch.as_tensor(got).detach().cpu().double()), np.asarray(torch.as_tensor(ref).detach().cpu().double())
    ng, nr = np.isnan(got), np.isnan(ref)
    if not np.array_equal(ng, nr):
        return float("inf")
    if nr.all():
        return 0.0
    return float(np.abs(got[~nr] - ref[~nr]).max() / max(1.0, np.abs(ref[~nr]).max()))


def split_sizes(n, g):
    q, r = divmod(int(n), int(g))
    return [q + 1] * r + [q] * (g - r)


def group_positions(n, g):
    """[(start, size)] of the groups in position space"""
    out, s = [], 0
    for sz in split_sizes(n, g):
        out.append((s, sz))
        s += sz
    return out


def gate_scores(hid_a, hid_b, c_w, c_b, dtype=np.float64):
    h = hid_a.astype(dtype) * (hid_b.astype(dtype) if hid_b is not None else dtype(1))
    return h @ c_w.astype(dtype).reshape(-1) + (dtype(c_b) if c_b is not None else dtype(0))


def select(p):
    """(argmax, argmin) of a group's p under the library's rule: the lower position among equals (-0 == +0), a NaN never
    selected, position 0 at both ends when every p is NaN"""
    ok = ~np.isnan(p)
    if not ok.any():
        return 0, 0
    idx = np.flatnonzero(ok)
    v = p[idx]
    return int(idx[np.flatnonzero(v == v.max())[0]]), int(idx[np.flatnonzero(v == v.min())[0]])


def segment_pool(mid, a, perm, cls_w, g, dtype=np.float64):
    """-> dict(pooled [G, L], sel [G, 2] original rows (of THIS evaluation's p), attn [N], p [N], m [G], l [G])"""
    n = mid.shape[0]
    mid, a, cls_w = mid.astype(dtype), a.astype(dtype), cls_w.astype(dtype)
    perm = np.arange(n) if perm is None else np.asarray(perm)
    pooled = np.zeros((g, mid.shape[1]), dtype)
    sel = np.zeros((g, 2), np.int64)
    attn, p = np.zeros(n, dtype), np.zeros(n, dtype)
    ms, ls = np.zeros(g, dtype), np.zeros(g, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (s, sz) in enumerate(group_positions(n, g)):
            rows = perm[s:s + sz]
            ag = a[rows]
            m = np.nanmax(ag) if not np.isnan(ag).all() else dtype(np.nan)
            e = np.exp(ag - m)
            l = e.sum()
            w = e / l
            pooled[k] = (w[:, None] * mid[rows]).sum(0)
            logit = w[:, None] * (mid[rows] @ cls_w.T)
            ex = np.exp(logit - np.nanmax(np.where(np.isnan(logit), -np.inf, logit), axis=1, keepdims=True))
            pg = ex[:, -1] / ex.sum(1)
            attn[rows], p[rows] = w, pg
            imax, imin = select(pg)
            sel[k] = rows[imax], rows[imin]
            ms[k], ls[k] = m, l
    return dict(pooled=pooled, sel=sel, attn=attn, p=p, m=ms, l=ls)


def select_from_p(p, perm, g):
    """sel [G, 2] (original rows) that the rule gives for a p [N] in original row order"""
    n = p.shape[0]
    perm = np.arange(n) if perm is None else np.asarray(perm)
    out = np.zeros((g, 2), np.int64)
    for k, (s, sz) in enumerate(group_positions(n, g)):
        rows = perm[s:s + sz]
        imax, imin = select(np.asarray(p)[rows])
        out[k] = rows[imax], rows[imin]
    return out


def segment_pool_backward(mid, a, perm, d_pooled, g, dtype=np.float64):
    """-> (d_mid [N, L], d_a [N]): d_mid_i = w_i d_pooled_g, d_a_i = w_i (mid_i . d_pooled_g - pooled_g . d_pooled_g)"""
    n = mid.shape[0]
    f = segment_pool(mid, a, perm, np.zeros((1, mid.shape[1])), g, dtype)
    mid, d_pooled = mid.astype(dtype), d_pooled.astype(dtype)
    perm = np.arange(n) if perm is None else np.asarray(perm)
    d_mid, d_a = np.zeros_like(mid), np.zeros(n, dtype)
    for k, (s, sz) in enumerate(group_positions(n, g)):
        rows = perm[s:s + sz]
        w = f["attn"][rows]
        d_mid[rows] = w[:, None] * d_pooled[k][None]
        d_a[rows] = w * (mid[rows] @ d_pooled[k] - f["pooled"][k] @ d_pooled[k])
    return d_mid, d_a


# ---------------------------------------------------------------------------------------------------- the whole model (torch)
def nll_surv(hazards, S, Y, c, alpha=0.0, eps=1e-7):
    """Discrete-time hazard negative log-likelihood (mean over the rows): with S_0 = 1 in front of S, an observed event in
    bin Y costs -log S_Y - log h_Y, a censored one -log S_{Y+1}; alpha weighs the uncensored term up"""
    Y, c = Y.reshape(-1, 1).long(), c.reshape(-1, 1).to(hazards.dtype)
    S_pad = torch.cat([torch.ones_like(c), S], 1)
    unc = -(1 - c) * (torch.log(S_pad.gather(1, Y).clamp(min=eps)) + torch.log(hazards.gather(1, Y).clamp(min=eps)))
    cen = -c * torch.log(S_pad.gather(1, Y + 1).clamp(min=eps))
    return ((1 - alpha) * (cen + unc) + alpha * unc).mean()


def _t(st, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in st.items()}


def front(x, st, act="relu"):
    mid = x @ st["dimReduction.fc1.weight"].T
    return torch.relu(mid) if act == "relu" else torch.nn.functional.gelu(mid)


def gate(x, st, pre):
    v = torch.tanh(x @ st[pre + "attention_V.0.weight"].T + st[pre + "attention_V.0.bias"])
    u = torch.sigmoid(x @ st[pre + "attention_U.0.weight"].T + st[pre + "attention_U.0.bias"])
    return (v * u) @ st[pre + "attention_weights.weight"].T.reshape(-1) + st[pre + "attention_weights.bias"]


def tier1(mid, a, perm, cls_w, g, sel=None):
    """torch, differentiable through pooled: -> pooled [G, L], p [N], sel [G, 2] (given, or by the rule from this p)"""
    n = mid.shape[0]
    perm = np.arange(n) if perm is None else np.asarray(perm)
    pooled, p = [], torch.zeros(n, dtype=mid.dtype)
    for s, sz in group_positions(n, g):
        rows = torch.as_tensor(perm[s:s + sz])
        w = torch.softmax(a[rows], 0)
        pooled.append((w[:, None] * mid[rows]).sum(0))
        p[rows] = torch.softmax(w[:, None] * (mid[rows] @ cls_w.T), 1)[:, -1].detach()
    if sel is None:
        sel = select_from_p(p.numpy(), perm, g)
    return torch.stack(pooled), p, np.asarray(sel)


def distilled(mid, pooled, sel, distill):
    if distill == "MaxMinS":
        return mid[torch.as_tensor(sel.reshape(-1))]
    if distill == "MaxS":
        return mid[torch.as_tensor(sel[:, 0].copy())]
    return pooled


def tier2(rows, st):
    w = torch.softmax(gate(rows, st, "UClassifier.attention."), 0)
    logits = ((w[:, None] * rows).sum(0) @ st["UClassifier.classifier.fc.weight"].T + st["UClassifier.classifier.fc.bias"])[None]
    hazards = torch.sigmoid(logits)
    return logits, hazards, torch.cumprod(1 - hazards, 1)


def eval_forward(x, st, perm, g, distill, act="relu", dtype=torch.float64, sel=None):
    """test_forward: -> dict(logits, hazards, S (1, C), p (N,), sel (G, 2))"""
    st, x = _t(st, dtype), torch.as_tensor(np.asarray(x)).to(dtype)
    mid = front(x, st, act)
    pooled, p, sel = tier1(mid, gate(mid, st, "attention."), perm, st["classifier.fc.weight"], g, sel)
    logits, hazards, S = tier2(distilled(mid, pooled, sel, distill), st)
    return dict(logits=logits, hazards=hazards, S=S, p=p, sel=sel)


def train_step(x, st, g, distill, label, censorship, act="relu", dtype=torch.float64, sel=None):
    """One train_forward (dropout 0) and the outer criterion(...).backward(), as two gradient sets: -> dict(hazards, S, loss0,
    loss, sel, inner {key: grad of loss0}, outer {key: grad of loss0 + loss}, dx (N, input_dim) of both).  The inner backward
    reaches the classifier, the attention and dimReduction; their .grad is not zeroed before the outer one, which adds to it."""
    st = {k: v.requires_grad_() for k, v in _t(st, dtype).items()}
    x = torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_()
    mid = front(x, st, act)
    pooled, _p, sel = tier1(mid, gate(mid, st, "attention."), None, st["classifier.fc.weight"], g, sel)
    t_h = torch.sigmoid(pooled @ st["classifier.fc.weight"].T + st["classifier.fc.bias"])
    t_S = torch.cumprod(1 - t_h, 1)
    Y, c = torch.full((g,), int(label)), torch.full((g,), float(censorship))
    loss0 = nll_surv(t_h, t_S, Y, c)
    keys = list(st)
    g0 = torch.autograd.grad(loss0, [st[k] for k in keys] + [x], retain_graph=True, allow_unused=True)
    _logits, hazards, S = tier2(distilled(mid, pooled, sel, distill), st)
    loss = nll_surv(hazards, S, Y[:1], c[:1])
    g1 = torch.autograd.grad(loss, [st[k] for k in keys] + [x], allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t   # noqa: E731
    inner = {k: z(g0[i], st[k]) for i, k in enumerate(keys)}
    outer = {k: inner[k] + z(g1[i], st[k]) for i, k in enumerate(keys)}
    return dict(hazards=hazards.detach(), S=S.detach(), loss0=loss0.detach().reshape(1), loss=loss.detach().reshape(1), sel=sel,
                inner=inner, outer=outer, dx=z(g0[-1], x) + z(g1[-1], x))
