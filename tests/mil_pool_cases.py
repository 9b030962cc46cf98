"""Case lists and closed-form inputs of the attention-pooling tests (csrc/mil_pool.hip on csrc/pool_core.h): tests/test_mil_pool_cases_cpu.py checks
on the CPU that the lists cover what they claim and that every premise holds; tests/test_mil_pool_matrix.py runs them on the
GPU.  Importing this module needs no device.

Every list is an edge on ONE axis at a time around a base case (dim 64, hidden 12, N 100), never a full cross product."""
import collections
import functools

import numpy as np

from mil_pool_ref import BWD_ROWS, CHUNK, MERGE_THREADS, ref64
from rrt_mil_amd import synth

# ---- launch_pool_merge's dynamic LDS, restated (tests/test_mil_pool_cases_cpu.py reads the compiled formula and thresholds)
LDS_DEFAULT, LDS_MERGE_MAX = 64 * 1024, 150 * 1024
MAX_TOKENS = 1000000


def nb_of(N):
    return -(-N // CHUNK)


def merge_lds(N, dim):
    return 4 * (((nb_of(N) + 3) & ~3) + dim) + 8 * 128 * 16


def backward_lds(dim, hid):
    return 4 * (dim + 4 * (hid + 4))


def largest_default_lds_N(dim):
    """the largest N whose merge launch stays at or under the default 64 KB"""
    nb = (LDS_DEFAULT - 8 * 128 * 16) // 4 - dim
    assert merge_lds(nb * CHUNK, dim) <= LDS_DEFAULT < merge_lds(nb * CHUNK + 1, dim)
    return nb * CHUNK


def align256(b):
    return (b + 255) & ~255


def attn_pool_workspace(N, dim, hid):
    """rrt_attn_pool_workspace_size: the larger of the forward's chunk partials and the backward's block partials"""
    return max(align256(4 * nb_of(N) * (dim + 4)), align256(4 * (-(-N // BWD_ROWS)) * (hid + 4)))


def pool_workspace(N, dim, hid, gated):
    """rrt_pool_workspace_size: hidden rows (twice when gated), raw scores, chunk partials, each piece aligned to 256 bytes"""
    return (1 + bool(gated)) * align256(4 * N * hid) + align256(4 * N) + align256(4 * nb_of(N) * (dim + 4))


BASE = dict(N=100, dim=64, hid=12)
LDS_DIM, LDS_HID = 32, 4
LDS_EDGE = largest_default_lds_N(LDS_DIM)               # 392 192 with today's constants
# cnt edges; nb on both sides of 8 (four chunk groups in flight), 32 (one trip of b0) and 1024 (one trip of the merge's strided
# loops), with full and one-token last chunks
FWD_NS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 224, 225, 256, 257, 992, 993, 1024, 1025, 1057, 32736, 32768, 32769, 32801, 65537)
FWD_DIMS = (32, 64, 512, 544, 1024)
FWD_HIDS = (4, 12, 252, 256, 260)
LDS_NS = (LDS_EDGE, LDS_EDGE + 1, MAX_TOKENS)
PEAK, PEAK_RANGE = 50.0, (40.0, 60.0)
OFFSET = 100.0
UNDERFLOW_GAP = 110.0

FwdCase = collections.namedtuple("FwdCase", "N dim hid gated bias kind where")
PredCase = collections.namedtuple("PredCase", "N dim hid ncls pred_bias no_norm want_pooled want_attn act gated kind")
BwdCase = collections.namedtuple("BwdCase", "N dim hid gated has_dattn has_draw kind")


def fwd_id(c):
    return f"{c.kind}{'' if c.where is None else '@' + str(c.where)}-N{c.N}-d{c.dim}-h{c.hid}-{'g' if c.gated else 'u'}{'b' if c.bias else ''}"


def pred_id(c):
    return (f"{c.kind}-N{c.N}-c{c.ncls}-{c.act}-{'g' if c.gated else 'u'}{'b' if c.pred_bias else ''}{'r' if c.no_norm else ''}"
            f"{'P' if c.want_pooled else ''}{'A' if c.want_attn else ''}")


def bwd_id(c):
    return f"{c.kind}-N{c.N}-d{c.dim}-h{c.hid}-{'g' if c.gated else 'u'}{'A' if c.has_dattn else ''}{'R' if c.has_draw else ''}"


def peak_positions(N):
    """token indices the bag's maximum is moved to: the first chunk, a middle chunk, the last token (of a ragged last chunk
    where N has one), and for N > 32 768 a chunk with index >= 1024"""
    pos = {0, (N // 64) * CHUNK + min(5, N - 1 - (N // 64) * CHUNK), N - 1}
    if N > MERGE_THREADS * CHUNK:
        pos.add(MERGE_THREADS * CHUNK)
    return sorted(pos)


def _fwd_cases():
    out = []
    for i, N in enumerate(FWD_NS):
        g = bool(i % 2)
        out.append(FwdCase(N, 64, 12, g, bool((i // 2) % 2), "mild", None))
        out += [FwdCase(N, 64, 12, not g, False, "peaked", w) for w in peak_positions(N)]
        out += [FwdCase(N, 64, 12, g, True, k, None) for k in ("offset+", "offset-")]
        out.append(FwdCase(N, 64, 12, not g, False, "flat", None))
        if N >= 2:
            out.append(FwdCase(N, 64, 12, g, False, "tie", None))
        if nb_of(N) >= 2:
            out.append(FwdCase(N, 64, 12, not g, True, "underflow", None))
            out.append(FwdCase(N, 64, 12, g, True, "masked", None))
    for dim in FWD_DIMS:
        for g in (False, True):
            out += [FwdCase(100, dim, 12, g, g, "mild", None), FwdCase(100, dim, 12, g, False, "peaked", 99),
                    FwdCase(100, dim, 12, g, True, "offset+", None)]
    for hid in FWD_HIDS:
        for g in (False, True):
            out += [FwdCase(100, 64, hid, g, not g, "mild", None), FwdCase(100, 64, hid, g, False, "peaked", 99),
                    FwdCase(100, 64, hid, g, True, "offset-", None)]
    return list(dict.fromkeys(out))


FWD_CASES = _fwd_cases()
# the large-LDS bags (dim 32, hidden 4): the kinds run on ONE y per N
LDS_KINDS = {LDS_EDGE: (("mild", None),), LDS_EDGE + 1: (("mild", None), ("peaked", LDS_EDGE), ("tie", None), ("offset+", None)),
             MAX_TOKENS: (("mild", None), ("peaked", MAX_TOKENS - 1))}
LDS_CASES = [FwdCase(N, LDS_DIM, LDS_HID, False, k == "offset+", k, w) for N in LDS_NS for k, w in LDS_KINDS[N]]

ACTS = ("none", "relu", "gelu", "tanh")
PRED_BASE = PredCase(33, 64, 12, 2, True, 0, True, True, "relu", False, "mild")


def _pred_cases():
    b = PRED_BASE
    out = [b]
    out += [b._replace(ncls=c) for c in (1, 16, 17)]
    out += [b._replace(pred_bias=False), b._replace(no_norm=1), b._replace(want_pooled=False), b._replace(want_attn=False),
            b._replace(want_pooled=False, want_attn=False), b._replace(gated=True), b._replace(gated=True, no_norm=1)]
    out += [b._replace(act=a) for a in ACTS]
    out += [b._replace(kind="peaked"), b._replace(kind="peaked", gated=True, ncls=17)]
    out += [b._replace(N=32801, kind=k, gated=g, ncls=17 if g else 2) for k in ("mild", "peaked") for g in (False, True)]
    return list(dict.fromkeys(out))


PRED_CASES = _pred_cases()

BWD_NS = (1, 2, 3, 5, 31, 32, 33, 35, 64, 1000, 40001)
BWD_DIMS = (32, 512, 544, 1024)
BWD_HIDS = (4, 12, 252, 256, 260)
BWD_KINDS = ("mild", "runner-up", "flat")
EXT_COMBOS = ((False, False), (True, False), (False, True), (True, True))


def _bwd_cases():
    out = []
    for i, N in enumerate(BWD_NS):
        for j, kind in enumerate(BWD_KINDS):
            if kind == "runner-up" and N < 3:          # (N = 2: d c_w = ds_1 (h_1 - h_2) cancels to 2 % by construction)
                continue
            da, dr = EXT_COMBOS[(i + j) % 4]
            dr = dr or kind == "flat"            # (flat rows without d_raw: d c_w = h sum_n ds_n is one more identically-zero tensor)
            out.append(BwdCase(N, 64, 12, bool((i + j) % 2), da, dr, kind))
    for N in (1, 33, 100):                       # every (d_attn + c_ext, d_raw, gated) combination
        out += [BwdCase(N, 64, 12, g, da, dr, "mild") for g in (False, True) for da, dr in EXT_COMBOS]
    out += [BwdCase(100, 64, 12, g, da, dr, "runner-up") for g in (False, True) for da, dr in EXT_COMBOS]
    for dim in BWD_DIMS:
        out += [BwdCase(100, dim, 12, g, g, not g, k) for g in (False, True) for k in ("mild", "runner-up")]
    for hid in BWD_HIDS:
        out += [BwdCase(100, 64, hid, g, not g, g, k) for g in (False, True) for k in ("mild", "runner-up")]
    return list(dict.fromkeys(out))


BWD_CASES = _bwd_cases()


# ------------------------------------------------------------------ closed-form inputs
@functools.lru_cache(maxsize=6)
def _y(N, dim):
    y = synth.normal(f"milpool/y/{N}x{dim}", (N, dim))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=8)
def _hidden(N, hid, gated):
    ha = np.tanh(synth.normal(f"milpool/ha/{N}x{hid}", (N, hid))).astype(np.float32)
    hb = (1.0 / (1.0 + np.exp(-synth.normal(f"milpool/hb/{N}x{hid}", (N, hid))))).astype(np.float32) if gated else None
    cw = (synth.normal(f"milpool/cw/{hid}", (hid,)) * np.float32(1.5 / np.sqrt(hid))).astype(np.float32)
    return ha, hb, cw


def _scores64(ha, hb, cw, cb):
    h = ha.astype(np.float64) * hb.astype(np.float64) if hb is not None else ha.astype(np.float64)
    return h @ cw.astype(np.float64) + (0.0 if cb is None else float(cb[0]))


def _swap_rows(ha, hb, i, j):
    for t in (ha, hb):
        if t is not None and i != j:
            t[[i, j]] = t[[j, i]]


def _peak(ha, hb, cw):
    """c_w rescaled (and its sign chosen) so that the largest |s| is +PEAK -> (c_w, index of the top score)"""
    s = _scores64(ha, hb, cw, None)
    top = int(np.abs(s).argmax())
    return (cw * np.float32(PEAK / s[top])).astype(np.float32), top


def _other_chunk_token(N, top):
    """a token in another chunk than `top` (N > 32 768: one of the two in a chunk >= 1024); N <= 32: another token"""
    if N > MERGE_THREADS * CHUNK:
        return N - 1 if top < MERGE_THREADS * CHUNK else 3
    for t in ((top + N // 2) % N, (top + CHUNK) % N, N - 1, 0):
        if t // CHUNK != top // CHUNK:
            return t
    return (top + 1) % N


def forward_inputs(c):
    """-> (y, hid_a, hid_b, c_w, c_b, meta): fp32 arrays (hid_b / c_b None when absent); meta holds what the kind promises.

    mild       scores of a few units: the plain case, every loop edge with nothing else going on
    peaked     c_w rescaled to max |s| = 50 and the top row moved to token `where`: a softmax that a missing exp(m_b - M), a
               maximum over the wrong count or a stale normaliser gets visibly wrong
    tie        the top row of the peaked inputs copied to a token of another chunk: two maxima, bit-equal scores
    offset+/-  c_b = +-100 on mild scores: exp without the maximum subtraction overflows / flushes in fp32
    underflow  one whole chunk >= 110 below the bag's maximum (which lies in another chunk): its exp(m_b - M) is 0 in fp32
    flat       every hidden row equal: attn = 1 / N, all entries the same bits
    masked     a few scores and one whole chunk at -inf (through hid_a; y finite): exact zeros, nothing turns NaN"""
    N, kind = c.N, c.kind
    y = _y(N, c.dim)
    ha, hb, cw = _hidden(N, c.hid, c.gated)
    ha, hb = ha.copy(), (hb.copy() if hb is not None else None)
    cb = (synth.uniform("milpool/cb", (1,), 0.05, 0.15)).astype(np.float32) if c.bias else None
    meta = {}
    if kind in ("peaked", "tie"):
        cw, top = _peak(ha, hb, cw)
        where = c.where if kind == "peaked" else top
        _swap_rows(ha, hb, top, where)
        meta["top"] = where
        if kind == "tie":
            other = _other_chunk_token(N, top)
            ha[other] = ha[top]
            if hb is not None:
                hb[other] = hb[top]
            meta["pair"] = (top, other)
    elif kind in ("offset+", "offset-"):
        cb = np.array([OFFSET if kind == "offset+" else -OFFSET], np.float32)
    elif kind == "flat":
        ha[:] = ha[0]
        if hb is not None:
            hb[:] = hb[0]
    elif kind == "underflow":
        # c_w rescaled to PEAK first (the top score is +50); one other chunk's hidden rows are -1.4 x the top token's, so
        # every score of that chunk is -70 = M - 120
        cw, top = _peak(ha, hb, cw)
        b = next(k for k in (nb_of(N) - 2, nb_of(N) - 1, 0) if k != top // CHUNK)
        lo, hi = b * CHUNK, min(N, (b + 1) * CHUNK)
        ha[lo:hi] = -1.4 * ha[top]
        if hb is not None:
            hb[lo:hi] = hb[top]
        meta["top"], meta["chunk"] = top, b
    elif kind == "masked":
        b = nb_of(N) // 2
        lo, hi = b * CHUNK, min(N, (b + 1) * CHUNK)
        idx = sorted(set(range(lo, hi)) | {1, N - 1, N // 3})
        j = int(np.abs(cw).argmax())
        ha[idx, j] = np.float32(-np.inf) if cw[j] > 0 else np.float32(np.inf)
        others = [k for k in range(c.hid) if k != j]
        ha[np.ix_(idx, others)] = 0.0                                     # (0 * inf never forms: one infinite term, the rest 0)
        meta["masked"], meta["chunk"] = np.array(idx), b
    else:
        assert kind == "mild", kind
    return y, ha, hb, cw, cb, meta


# ---- predictor stage: the hidden Linear(s) in front of the pool, then the predictor
ACT_CODE = {"none": 0, "relu": 1, "gelu": 2, "tanh": 3}


def _act_torch(t, act):
    import torch
    return {"none": lambda v: v, "relu": torch.relu, "gelu": torch.nn.functional.gelu, "tanh": torch.tanh}[act](t)


def hidden_rows(y, a_w, a_b, b_w, b_b, act, dtype):
    """act(y a_w^T + a_b) and sigmoid(y b_w^T + b_b) by torch on the CPU in `dtype` -> (hid_a, hid_b or None) as numpy"""
    import torch
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)          # noqa: E731
    ha = _act_torch(t(y) @ t(a_w).t() + t(a_b), act)
    hb = torch.sigmoid(t(y) @ t(b_w).t() + t(b_b)) if b_w is not None else None
    return ha.numpy(), (hb.numpy() if hb is not None else None)


def predict_inputs(c):
    """-> dict of fp32 arrays y, a_w, a_b, b_w, b_b (None unless gated), c_w, c_b, pred_w, pred_b (None without bias).
    peaked: the gain goes on c_w, behind the hidden Linear, so that max |s| = 50 in float64"""
    import torch
    tag = f"milpool/pred/{c.dim}/{c.hid}"
    d = dict(y=_y(c.N, c.dim),
             a_w=synth.normal(tag + "/a_w", (c.hid, c.dim)) / np.float32(np.sqrt(c.dim)), a_b=synth.uniform(tag + "/a_b", (c.hid,), -0.1, 0.1),
             b_w=synth.normal(tag + "/b_w", (c.hid, c.dim)) / np.float32(np.sqrt(c.dim)) if c.gated else None,
             b_b=synth.uniform(tag + "/b_b", (c.hid,), -0.1, 0.1) if c.gated else None,
             c_w=synth.normal(tag + "/c_w", (c.hid,)) * np.float32(1.5 / np.sqrt(c.hid)), c_b=synth.uniform(tag + "/c_b", (1,), 0.05, 0.15),
             pred_w=synth.normal(f"{tag}/pred_w/{c.ncls}", (c.ncls, c.dim)) / np.float32(np.sqrt(c.dim)),
             pred_b=synth.uniform(f"{tag}/pred_b/{c.ncls}", (c.ncls,), -0.1, 0.1) if c.pred_bias else None)
    d = {k: (None if v is None else np.ascontiguousarray(v, dtype=np.float32)) for k, v in d.items()}
    if c.kind == "peaked":
        ha, hb = hidden_rows(d["y"], d["a_w"], d["a_b"], d["b_w"], d["b_b"], c.act, torch.float64)
        s = _scores64(ha, hb, d["c_w"], None)
        d["c_w"] = (d["c_w"] * np.float32(PEAK / s[int(np.abs(s).argmax())])).astype(np.float32)
        d["c_b"] = np.zeros(1, np.float32)
    return d


# ---- backward stage
def backward_inputs(c):
    """-> dict: y, hid_a, hid_b, c_w (fp32), attn, pooled (the float64 reference's, rounded to fp32: an error is then the
    backward's own), d_pooled, d_attn, d_raw, c_ext (None when absent), ref (ref64's float64 gradients), natural.

    mild        scores of a few units
    runner-up   max |s| = 50, a second token whose hidden row is 0.98 x the top one's (score 49) and a third one at score 48:
                the top weight stays away from 1, so ds is a value and not rounding noise
    flat        every hidden row equal (attn = 1 / N)"""
    N = c.N
    y = _y(N, c.dim)
    ha, hb, cw = _hidden(N, c.hid, c.gated)
    ha, hb = ha.copy(), (hb.copy() if hb is not None else None)
    meta = {}
    if c.kind == "runner-up":
        cw, top = _peak(ha, hb, cw)
        second = _other_chunk_token(N, top)
        ha[second] = np.float32(0.98) * ha[top]
        if hb is not None:
            hb[second] = hb[top]
        # a third token at score 48 whose hidden row is NOT parallel to the top one's (its own row, rescaled): with the two
        # parallel rows alone d c_w = sum_n ds_n h_n cancels to 2 % and would sit at the floor of the gradient rule
        s = _scores64(ha, hb, cw, None)
        rest = np.setdiff1d(np.arange(N), [top, second])
        third = int(rest[np.abs(s[rest]).argmax()])
        ha[third] = (ha[third].astype(np.float64) * (0.96 * PEAK / s[third])).astype(np.float32)
        meta["top"], meta["second"], meta["third"] = top, second, third
    elif c.kind == "flat":
        ha[:] = ha[0]
        if hb is not None:
            hb[:] = hb[0]
    d_pooled = synth.normal(f"milpool/dp/{c.dim}", (c.dim,))
    d_attn = synth.normal(f"milpool/dattn/{N}", (N,)) if c.has_dattn else None
    d_raw = (synth.normal(f"milpool/draw/{N}", (N,)) * np.float32(0.1)) if c.has_draw else None
    ref = ref64(y, ha, hb, cw, None, d_pooled=d_pooled, d_attn=d_attn, d_raw=d_raw)
    attn64 = ref["attn"].numpy()
    da = y.astype(np.float64) @ d_pooled.astype(np.float64) + (0.0 if d_attn is None else d_attn.astype(np.float64))
    c_ext = np.array([(attn64 * d_attn.astype(np.float64)).sum()], np.float32) if c.has_dattn else None
    return dict(y=y, hid_a=ha, hid_b=hb, c_w=cw, attn=attn64.astype(np.float32), pooled=ref["pooled"].numpy().astype(np.float32),
                d_pooled=d_pooled, d_attn=d_attn, d_raw=d_raw, c_ext=c_ext, ref=ref, natural=float(np.abs(attn64 * da).max()),
                meta=meta)


def floor_expected(c, name):
    """whether `name`'s float64 reference is identically zero, so that _grad_tol's floor decides: d c_b without d_raw (the
    softmax adjoint sums to zero), and at N = 1 without d_raw every ds (attn = 1, da - c = 0)"""
    if c.has_draw:
        return False
    return name == "dcb" or (c.N == 1 and name in ("dhid_a", "dhid_b", "dcw"))


# ------------------------------------------------------------------ the bounds (none of them new)
def grad_tol(scale, natural):
    """tests/test_clam_gpu.py::_grad_tol, the project's gradient criterion: 1e-3 of the tensor's largest reference entry `scale`;
    an identically-zero reference is held to 1e-5 of `natural`, the largest of the terms that cancel"""
    return 1e-3 * scale if scale > 1e-9 * natural else 1e-5 * natural


def forward_errors(got, ref):
    """{name: (err, tol)} under the bounds of tests/test_clam_gpu.py::_check_fwd (pooled 2e-5; attn and raw scores 2e-5 *
    max(1, largest reference entry)), tests/test_hip_parity.py::test_pool_predict (logits 2e-5 * max(1, max |pooled_ref|)) and
    |sum attn - 1| < 1e-5.  `got`: fp32 arrays (absent / None: not checked); `ref`: ref64's dict.  Where the reference is
    -inf (masked scores) the entry has to be -inf too (an infinite error otherwise) and is left out of the maxima."""
    out = {}
    for name in ("pooled", "attn", "s", "logits"):
        if got.get(name) is None:
            continue
        g, r = np.asarray(got[name], dtype=np.float64).reshape(-1), ref[name].numpy().reshape(-1)
        fin = np.isfinite(r)
        with np.errstate(invalid="ignore"):
            err = float(np.abs(g[fin] - r[fin]).max()) if fin.any() else 0.0
        if not np.isfinite(g[fin]).all() or not np.array_equal(g[~fin], r[~fin]):
            err = float("inf")
        scale = float(np.abs(r[fin]).max()) if fin.any() else 0.0
        tol = {"pooled": 2e-5, "attn": 2e-5 * max(1.0, scale), "s": 2e-5 * max(1.0, scale),
               "logits": 2e-5 * max(1.0, float(ref["pooled"].abs().max()))}[name]
        out[name] = (err, tol)
    if got.get("attn") is not None:
        tot = float(np.asarray(got["attn"], dtype=np.float64).sum())
        out["sum"] = (abs(tot - 1.0) if np.isfinite(tot) else float("inf"), 1e-5)
    return out


GRADS = ("dy", "dhid_a", "dhid_b", "dcw", "dcb")


def backward_errors(got, inp):
    """{name: (err, tol, scale)} under grad_tol; `got`: fp32 arrays by name, `inp`: backward_inputs' dict"""
    out = {}
    for name in GRADS:
        if name not in inp["ref"]:
            continue
        g, r = np.asarray(got[name], dtype=np.float64).reshape(-1), inp["ref"][name].numpy().reshape(-1)
        err = float(np.abs(g - r).max()) if np.isfinite(g).all() else float("inf")
        scale = float(np.abs(r).max())
        out[name] = (err, grad_tol(scale, inp["natural"]), scale)
    return out
