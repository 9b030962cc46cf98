"""CPU restatement of the reference's plain MIL heads (modules/attmil.py DAttention / AttentionGated, attmil_ibmil.py
Dattention_ori, mean_max.py MeanMIL / MaxMIL) in torch ops, in float64 or fp32, in the reference's op order: the yardstick of
tests/test_bagmil_gpu.py, pinned to the reference's own float64 run by tests/test_bagmil_cpu.py (tools/make_golden_bagmil.py).
The encoder inside a head is oracle/rrt_oracle.py's eager port.  Stage functions (mean pool and its adjoint, deconfounder)
restate the kernels' contracts of include/rrt_hip.h."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rrt_oracle as O

EMB_KEY = {"attmil": "feature.0", "gattmil": "feature.0", "ibmil": "embedding.embed.0", "meanmil": "head.0", "maxmil": "head.0"}


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|) in float64"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


def rrt_prefix(keys):
    """the state_dict prefix of the encoder inside a head ('feature.3.', 'embedding.rrt.', 'head.2.', ...), or None"""
    hits = [k[:-len("cr_msa.norm.weight")] for k in keys if k.endswith("cr_msa.norm.weight")]
    return hits[0] if hits else None


def cls_key(kind, keys):
    if kind in ("attmil", "gattmil"):
        return "classifier.0"
    if kind == "ibmil":
        return "head"
    pre = rrt_prefix(keys)
    return "head.%d" % max(int(k.split(".")[1]) for k in keys if k.startswith("head.") and not (pre and k.startswith(pre)))


def _act(t, name):
    return {"relu": F.relu, "gelu": F.gelu, "tanh": torch.tanh}.get(name, lambda v: v)(t)


def head(kind, x, state, enc_cfg=None, act="relu", gate_act="relu", dtype=torch.float64, grad=False):
    """One bag x (N, input_dim) through head `kind` with the state_dict `state` (arrays, the reference's keys).  ``act``: the
    embedding's activation as the constructor got it; ``gate_act``: AttentionGated's.  Returns a dict: logits (1, C), y (N, 512)
    and, by pool: pooled (512,) (= M[0]; M (1, 512) is the node the tail reads), raw (N,), attn (N,) / scores (N, C), argmax (C,) /
    colmean (512,) / deconf_a (K,), deconf_cf (V,) (= cf_node[0]; q_node (1, J) is the bag query).
    grad=True: leaves that require grad, as ``x_leaf`` and ``params`` {key: tensor} in the dict."""
    keys = list(state)
    st = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()}
    st = {k: (v.to(dtype).requires_grad_(grad) if v.is_floating_point() else v) for k, v in st.items()}
    x = torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        lin = lambda t, name: F.linear(t, st[name + ".weight"], st.get(name + ".bias"))   # noqa: E731
        if kind == "gattmil":
            emb_act = "relu"
        elif kind in ("attmil", "ibmil"):
            emb_act = "gelu" if act.lower() == "gelu" else "relu"
        else:
            emb_act = act.lower()
        emb = _act(lin(x, EMB_KEY[kind]), emb_act)
        pre = rrt_prefix(keys)
        if pre is not None:
            enc_state = {k[len(pre):]: v for k, v in st.items() if k.startswith(pre)}
            y = O.forward_eager(emb, enc_state, enc_cfg, grad=True, grad_dtype=dtype)[0] if grad else \
                O.forward_eager(emb, enc_state, enc_cfg)
        else:
            y = emb
        out = {"y": y}
        ck = cls_key(kind, keys)
        if kind in ("meanmil", "maxmil"):
            scores = lin(y, ck)                                         # (N, C)
            out["scores"] = scores
            if kind == "meanmil":
                out["logits"] = scores.mean(0, keepdim=True)
                out["colmean"] = y.mean(0)
            else:
                out["logits"], out["argmax"] = (t.unsqueeze(0) for t in scores.max(0))
                out["argmax"] = out["argmax"][0]
        else:
            if kind == "gattmil":
                a = _act(lin(y, "attention_a.0"), gate_act)
                raw = lin(a * torch.sigmoid(lin(y, "attention_b.0")), "attention_c")
            else:
                raw = lin(torch.tanh(lin(y, "attention.0")), "attention.2")
            A = F.softmax(raw.transpose(0, 1), dim=1)                   # (1, N)
            M = torch.mm(A, y)                                          # (1, 512)
            out.update(raw=raw[:, 0], attn=A[0], pooled=M[0], M=M)
            if kind == "ibmil" and "confounder_feat" in st:
                conf = st["confounder_feat"].to(dtype)
                a_, cf = deconf_tail(M, conf, st["W_q.weight"], st["W_q.bias"], st["W_k.weight"], st["W_k.bias"])
                out.update(deconf_a=a_, deconf_cf=cf[0], cf_node=cf, q_node=F.linear(M, st["W_q.weight"], st["W_q.bias"]))
                M = torch.cat((M, cf), dim=1)
            out["logits"] = lin(M, ck)
    if grad:
        out["x_leaf"], out["params"] = x, st
    return out


def deconf_tail(M, conf, q_w, q_b, k_w, k_b):
    """attmil_ibmil.py:94-98 on M (1, dim): -> (a (K,), cf (1, V)); the 1 / sqrt(J) factor through a float32 tensor, as there"""
    bag_q = F.linear(M, q_w, q_b)
    conf_k = F.linear(conf, k_w, k_b)
    s = torch.mm(conf_k, bag_q.transpose(0, 1))
    a = F.softmax(s / torch.sqrt(torch.tensor(conf_k.shape[1], dtype=torch.float32)).to(s.dtype), 0)
    return a[:, 0], torch.mm(a.transpose(0, 1), conf)


def deconf_head(pooled, conf, q_w, q_b, k_w, k_b, head_w, head_b, dtype):
    """rrt_deconf_head_f32's contract -> (logits (C,), a (K,), cf (V,), raw scores (K,))"""
    t = lambda v: None if v is None else torch.as_tensor(np.asarray(v)).to(dtype)   # noqa: E731
    pooled, conf, q_w, q_b, k_w, k_b, head_w, head_b = map(t, (pooled, conf, q_w, q_b, k_w, k_b, head_w, head_b))
    M = pooled[None]
    a, cf = deconf_tail(M, conf, q_w, q_b, k_w, k_b)
    raw = torch.mm(F.linear(conf, k_w, k_b), F.linear(M, q_w, q_b).t())[:, 0] / math.sqrt(k_w.shape[0])
    return F.linear(torch.cat((M, cf), 1), head_w, head_b)[0], a, cf[0], raw


def bag_mean(y, w, b, dtype):
    """rrt_bag_mean_f32's contract in the reference's order, Linear(y).mean(0) -> (logits (C,), colmean (dim,))"""
    y, w = (torch.as_tensor(np.asarray(v)).to(dtype) for v in (y, w))
    b = None if b is None else torch.as_tensor(np.asarray(b)).to(dtype)
    return F.linear(y, w, b).mean(0), y.mean(0)


def bag_mean_backward(d_logits, colmean, w, n, dtype):
    """autograd of mean_n(y_n . w[j] + b[j]) -> (dy (n, dim), dW (C, dim), db (C,))"""
    g, cm, w = (torch.as_tensor(np.asarray(v)).to(dtype) for v in (d_logits, colmean, w))
    row = (g[:, None] * w).sum(0) / n
    return row[None].expand(n, -1), g[:, None] * cm[None], g
