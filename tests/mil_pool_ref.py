"""Restatements of csrc/mil_pool.hip and of the pooling core its kernels are built on (csrc/pool_core.h: gate score, chunk sum,
merge block) for tests/test_mil_pool_matrix.py and tests/test_mil_pool_cases_cpu.py (no device).

``ref64`` is the operation of the file's header comment in float64 torch on the CPU:
    s_n = c_w . h_n (+ c_b)   h = hid_a, or hid_a * hid_b (gated)      attn = softmax_n(s)
    pooled = sum_n attn_n y_n                                          logits = pred_w pooled (+ pred_b)
and its adjoint by float64 autograd for any subset of the upstream gradients (d_pooled, the gradient through the returned
attention row, the gradient through the returned raw scores).

``emulate32`` evaluates the same thing in fp32 on the CPU in the SHAPE of the kernels -- 32-token chunks that emit
(m_b, l_b, v_b), a merge with exp(m_b - M), the backward as ds = a (da - c) + d_raw -- and can seed one value-only defect at a
time (``DEFECTS``).  It is what the case lists are measured against on a machine without a GPU: without a defect it has to sit
inside every bound, and every defect has to be caught by a case."""
import numpy as np
import torch

CHUNK = 32                      # POOL_CHUNK (csrc/internal.h); tests/test_mil_pool_cases_cpu.py reads the compiled value
BWD_ROWS = 32                   # POOL_BWD_ROWS
MERGE_THREADS = 1024            # the merge block (pool_merge_core): the stride of its loops over the partials
HID_STRIDE = 256                # floats of a hidden row one wave covers per trip
DIM_PASS = 512                  # columns per pass of the weighted sums
CLASS_STRIDE = 16               # classes per trip of the predictor (one wave each)
SENTINEL = np.float32(-3.0e38)  # the kernels' "no maximum yet"

DEFECTS = {
    "no_max_sub": "a chunk's exp without the maximum subtraction (m_b reported as 0)",
    "no_merge_rescale": "the merge adds l_b, v_b without exp(m_b - M)",
    "merge_first_1024": "the merge ignores the partials b >= 1024 (its strided loops take one trip)",
    "chunk_max_over_32": "the chunk maximum over 32 slots instead of cnt (stale slots read as 0)",
    "chunk_sum_over_32": "the chunk sum over 32 slots instead of cnt (stale slots read as score 0)",
    "norm_missing_last": "the merge's normaliser misses the last partial",
    "attn_own_chunk_max": "attn normalised with the chunk's own m_b instead of M",
    "hid_stops_256": "the loop over the hidden row stops after its first trip (256 floats)",
    "dim_stops_512": "the loop over the columns stops after its first pass (512 columns)",
    "classes_stop_16": "the predictor stops after its first trip (16 classes)",
    "bwd_drop_c_ext": "the backward drops c_ext",
    "bwd_drop_d_raw": "the backward drops d_raw",
    "bwd_drop_c": "the backward drops the - c of the softmax adjoint",
    "bwd_skip_tail_rows": "the backward skips the rows n >= 32 floor(N / 32)",
    "bwd_gate_swapped": "gated: dhid_a and dhid_b swapped",
}
FWD_DEFECTS = tuple(d for d in DEFECTS if not d.startswith("bwd_"))
BWD_DEFECTS = tuple(d for d in DEFECTS if d.startswith("bwd_")) + ("hid_stops_256", "dim_stops_512")


def _t64(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64))


def ref64(y, hid_a, hid_b, c_w, c_b=None, pred_w=None, pred_b=None, d_pooled=None, d_attn=None, d_raw=None):
    """-> dict of float64 CPU tensors: s, attn, pooled (, logits with pred_w) (, dy, dhid_a, dhid_b, dcw, dcb with any upstream
    gradient).  dcb is returned whether or not c_b is given: the kernel always emits sum_n ds_n."""
    want_grad = any(g is not None for g in (d_pooled, d_attn, d_raw))
    y, ha, hb, cw = _t64(y), _t64(hid_a), _t64(hid_b), _t64(c_w).reshape(-1)
    cb = torch.zeros(1, dtype=torch.float64) if c_b is None else _t64(c_b).reshape(1)
    leaves = [t for t in (y, ha, hb, cw, cb) if t is not None]
    if want_grad:
        for t in leaves:
            t.requires_grad_(True)
    h = ha * hb if hb is not None else ha
    s = h @ cw + cb
    attn = torch.softmax(s, dim=0)
    pooled = attn @ y
    out = {"s": s, "attn": attn, "pooled": pooled}
    if pred_w is not None:
        out["logits"] = _t64(pred_w) @ pooled.detach() + (0 if pred_b is None else _t64(pred_b))
    if want_grad:
        loss = 0.0
        if d_pooled is not None:
            loss = loss + (pooled * _t64(d_pooled)).sum()
        if d_attn is not None:
            loss = loss + (attn * _t64(d_attn)).sum()
        if d_raw is not None:
            loss = loss + (s * _t64(d_raw)).sum()
        loss.backward()
        out.update(dy=y.grad if y.grad is not None else torch.zeros_like(y), dhid_a=ha.grad, dcw=cw.grad, dcb=cb.grad)
        if hb is not None:
            out["dhid_b"] = hb.grad
    return {k: v.detach() for k, v in out.items()}


def _f32(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _scores32(ha, hb, cw, cb, defect):
    h = ha * hb if hb is not None else ha
    if defect == "hid_stops_256":
        h, cw = h[:, :HID_STRIDE], cw[:HID_STRIDE]
    s = (h * cw[None, :]).sum(axis=1, dtype=np.float32)          # (every row in the same order, as one wave per token does)
    return s + np.float32(0.0 if cb is None else np.asarray(cb).reshape(-1)[0])


def emulate32(y, hid_a, hid_b, c_w, c_b=None, pred_w=None, pred_b=None, defect=None):
    """the forward in fp32, chunk by chunk -> dict of fp32 arrays: s, attn, pooled (, logits)"""
    assert defect is None or defect in DEFECTS, defect
    y, ha, hb, cw = _f32(y), _f32(hid_a), _f32(hid_b), _f32(c_w).reshape(-1)
    N, dim = y.shape
    nb = -(-N // CHUNK)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        s = _scores32(ha, hb, cw, c_b, defect)
        pad = nb * CHUNK - N
        valid = (np.arange(nb * CHUNK) < N).reshape(nb, CHUNK)
        sp = np.concatenate([s, np.zeros(pad, np.float32)]).reshape(nb, CHUNK)          # stale slots: score 0
        yp = (np.concatenate([y, np.zeros((pad, dim), np.float32)]) if pad else y).reshape(nb, CHUNK, dim)
        in_max = np.ones_like(valid) if defect == "chunk_max_over_32" else valid
        in_sum = np.ones_like(valid) if defect == "chunk_sum_over_32" else valid
        m = np.maximum(SENTINEL, np.where(in_max, sp, -np.inf).max(axis=1)).astype(np.float32)
        if defect == "no_max_sub":
            m = np.zeros_like(m)
        e = np.where(in_sum, np.exp(sp - m[:, None]), np.float32(0)).astype(np.float32)
        l = e.sum(axis=1, dtype=np.float32)
        v = np.einsum("bt,btd->bd", np.where(valid, e, np.float32(0)).astype(np.float32), yp).astype(np.float32)
        # ---- merge
        seen = slice(0, MERGE_THREADS) if defect == "merge_first_1024" else slice(None)
        M = np.maximum(SENTINEL, m[seen].max()).astype(np.float32)
        sc = np.ones_like(m) if defect == "no_merge_rescale" else np.exp(m - M).astype(np.float32)
        if defect == "merge_first_1024":
            sc[MERGE_THREADS:] = 0
        lsc = (l * sc).astype(np.float32)
        L = (lsc[:-1] if defect == "norm_missing_last" else lsc).sum(dtype=np.float32)
        invL = np.float32(1.0) / np.float32(L)
        pooled = ((sc[None, :] @ v).reshape(dim).astype(np.float32) * invL).astype(np.float32)
        if defect == "dim_stops_512":
            pooled[DIM_PASS:] = 0
        m_of = np.repeat(m, CHUNK)[:N] if defect == "attn_own_chunk_max" else M
        attn = (np.exp(s - m_of).astype(np.float32) * invL).astype(np.float32)
        out = {"s": s, "attn": attn, "pooled": pooled}
        if pred_w is not None:
            logits = (_f32(pred_w) @ pooled).astype(np.float32)
            if pred_b is not None:
                logits = logits + _f32(pred_b)
            if defect == "classes_stop_16":
                logits[CLASS_STRIDE:] = 0
            out["logits"] = logits
    return out


def emulate32_backward(y, hid_a, hid_b, c_w, attn, pooled, d_pooled, d_attn=None, d_raw=None, c_ext=None, defect=None):
    """the backward in fp32 from the given attn / pooled -> dict of fp32 arrays: dy, dhid_a (, dhid_b), dcw, dcb"""
    assert defect is None or defect in DEFECTS, defect
    y, ha, hb, cw = _f32(y), _f32(hid_a), _f32(hid_b), _f32(c_w).reshape(-1)
    a, po, dp = _f32(attn), _f32(pooled), _f32(d_pooled)
    N, dim = y.shape
    cols = DIM_PASS if defect == "dim_stops_512" else dim
    hcols = HID_STRIDE if defect == "hid_stops_256" else ha.shape[1]
    da = (y[:, :cols] @ dp[:cols]).astype(np.float32)
    if d_attn is not None:
        da = da + _f32(d_attn)
    cc = np.float32(po @ dp)
    if c_ext is not None and defect != "bwd_drop_c_ext":
        cc = np.float32(cc + np.float32(np.asarray(c_ext).reshape(-1)[0]))
    ds = (a * da if defect == "bwd_drop_c" else a * (da - cc)).astype(np.float32)
    if d_raw is not None and defect != "bwd_drop_d_raw":
        ds = ds + _f32(d_raw)
    dy = (a[:, None] * dp[None, :]).astype(np.float32)
    dy[:, cols:] = 0
    if defect == "bwd_skip_tail_rows":
        ds[BWD_ROWS * (N // BWD_ROWS):] = 0
        dy[BWD_ROWS * (N // BWD_ROWS):] = 0
    g = (ds[:, None] * cw[None, :]).astype(np.float32)
    g[:, hcols:] = 0
    out = {"dy": dy}
    if hb is not None:
        da_, db_ = (g * hb).astype(np.float32), (g * ha).astype(np.float32)
        out["dhid_a"], out["dhid_b"] = (db_, da_) if defect == "bwd_gate_swapped" else (da_, db_)
        h = ha * hb
    else:
        out["dhid_a"], h = g, ha
    dcw = (ds @ h).astype(np.float32)
    dcw[hcols:] = 0
    out["dcw"], out["dcb"] = dcw, np.float32(ds.sum(dtype=np.float32)).reshape(1)
    return out
