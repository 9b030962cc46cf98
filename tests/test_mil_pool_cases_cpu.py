"""CPU: the case lists of tests/test_mil_pool_matrix.py (tests/mil_pool_cases.py) cover what they claim, and the Python
restatement of the constants of csrc/mil_pool.hip and of the pooling core it is built on, csrc/pool_core.h
(tests/mil_pool_ref.py), is the compiled one.

  * the chunk size, the backward's rows per block, every loop stride and the merge launch's LDS formula with its two thresholds
    are read out of the sources; the two workspace-size queries are compared with the restated formulas over a sweep;
  * the lists reach every cnt, both sides of nb = 8 / 32 / 1024 and of the 64 KB threshold, the dim / hidden / class edges and
    every (d_attn, d_raw, gated) combination;
  * every case's premise holds in float64 (conditions, not measurements);
  * the fp32 chunked evaluation `emulate32` sits inside every bound on every case, and every defect it can seed is caught by a
    named case by at least 10x its bound;
  * every refusal comes back before anything is launched (dummy pointers, never followed), the LDS refusals included."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mil_pool_cases as K
import mil_pool_ref as R
from rrt_mil_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
P = 0x1000                                  # a non-null "device pointer": every call below is refused before it is followed
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from rrt_mil_amd.build import build
    build()
    return _lib.load()


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


# ------------------------------------------------------------------ the restated constants are the compiled ones
def test_restated_constants_are_the_compiled_ones(lib):
    hdr, src, core = _src("internal.h"), _src("mil_pool.hip"), _src("pool_core.h")
    assert int(re.search(r"constexpr int POOL_CHUNK = (\d+);", hdr).group(1)) == R.CHUNK == 32
    assert int(re.search(r"constexpr int POOL_BWD_ROWS = (\d+);", src).group(1)) == R.BWD_ROWS == 32
    # the merge block: 1024 threads striding over the partials (maximum, then scale / normaliser) and over attn; every head's
    # merge kernel is that block
    assert "__launch_bounds__(1024) void pool_merge_kernel" in src and "kern<<<dim3(1), dim3(1024), lds, st>>>" in src
    for unit, kern in (("clam_pool.hip", "branch_merge_kernel"), ("dsmil_pool.hip", "dsmil_merge_kernel")):
        text = _src(unit)
        assert f"__launch_bounds__(1024) void {kern}" in text and f"auto kern = {kern};" in text
        assert "kern<<<dim3(K), dim3(1024), lds, st>>>" in text
    assert "auto kern = pool_merge_kernel;" in src
    assert len(re.findall(r"for \(int b = tid; b < nb; b \+= 1024\)", core)) == 2 and R.MERGE_THREADS == 1024
    assert "for (int n = tid; n < N; n += 1024)" in src
    assert "for (int b0 = grp; b0 < nb; b0 += 32)" in core and "const int b = b0 + 8 * u;" in core        # 8 groups, 4 in flight
    assert "for (int j = wave; j < n_classes; j += 16)" in src and R.CLASS_STRIDE == 16
    assert len(re.findall(r"for \(int cb = 0; cb < dim; cb \+= 512\)", core)) == 2 and R.DIM_PASS == 512   # chunk sum, merge
    hid_loop = r"for \(int c = lane \* 4; c < hid; c \+= 256\)"                                            # gate score | backward
    assert len(re.findall(hid_loop, core)) == 1 and len(re.findall(hid_loop, src)) == 1 and R.HID_STRIDE == 256
    dim_loop = r"for \(int c = lane \* 4; c < dim; c \+= 256\)"                                            # row dot | backward
    assert len(re.findall(dim_loop, core)) == 1 and len(re.findall(dim_loop, src)) == 1
    assert "for (int t0 = rg; t0 < cnt; t0 += 8)" in core and "const int t = t0 + 2 * u;" in core
    assert "for (int t = wave; t < POOL_BWD_ROWS; t += 4)" in src and "if (n >= N) break;" in src
    assert "float m = -3.0e38f;" in src and "float m = -3.0e38f;" in core and R.SENTINEL == np.float32(-3.0e38)
    # the LDS formulas and thresholds
    m = re.search(r"constexpr size_t POOL_LDS_DEFAULT = (\d+) \* 1024, POOL_MERGE_LDS_MAX = (\d+) \* 1024;", hdr)
    assert (int(m.group(1)) * 1024, int(m.group(2)) * 1024) == (K.LDS_DEFAULT, K.LDS_MERGE_MAX)
    assert "return (((nb + 3) & ~(size_t)3) + dim) * sizeof(float) + (size_t)8 * 128 * sizeof(float4);" in hdr
    assert "return ((size_t)dim + 4 * ((size_t)hid + 4)) * sizeof(float);" in src
    assert "if (lds > POOL_MERGE_LDS_MAX) return hipErrorInvalidValue;" in src and "if (lds > POOL_LDS_DEFAULT)\n" in hdr
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in hdr and "pool_raise_lds_limit((const void*)kern, lds);" in src
    assert K.LDS_EDGE == 392192 and K.merge_lds(K.LDS_EDGE, 32) == 65536 and K.merge_lds(K.LDS_EDGE + 1, 32) == 65552
    assert K.merge_lds(K.MAX_TOKENS, K.LDS_DIM) <= K.LDS_MERGE_MAX
    need = C.c_size_t()
    for N in (1, 31, 32, 33, 100, 1000, 4097, 32768, 32769, 65537, K.LDS_EDGE + 1, K.MAX_TOKENS):
        for dim in (32, 64, 512, 544, 1024):
            for hid in (4, 12, 128, 252, 260):
                if K.merge_lds(N, dim) > K.LDS_MERGE_MAX:
                    continue
                assert lib.rrt_attn_pool_workspace_size(N, dim, hid, C.byref(need)) == OK
                assert need.value == K.attn_pool_workspace(N, dim, hid), (N, dim, hid)
                for gated in (0, 1):
                    assert lib.rrt_pool_workspace_size(N, dim, hid, gated, C.byref(need)) == OK
                    assert need.value == K.pool_workspace(N, dim, hid, gated), (N, dim, hid, gated)


# ------------------------------------------------------------------ the lists cover what they claim
def test_lists_cover_their_edges():
    fwd = K.FWD_CASES + K.LDS_CASES
    cnt = {c.N - (K.nb_of(c.N) - 1) * R.CHUNK for c in fwd}
    assert {1, 2, 7, 8, 9, 31, 32} <= cnt
    nbs = {K.nb_of(c.N) for c in fwd}
    for edge in (8, 32, R.MERGE_THREADS):                    # four chunk groups in flight / one b0 trip / one strided trip
        assert {edge - 1, edge, edge + 1} <= nbs, edge
    assert any(K.nb_of(c.N) == R.MERGE_THREADS + 1 and c.N % R.CHUNK == 1 for c in fwd)                   # a one-token chunk 1024
    lds = {K.merge_lds(c.N, c.dim) > K.LDS_DEFAULT for c in K.LDS_CASES}
    assert lds == {False, True} and {c.N for c in K.LDS_CASES} == {K.LDS_EDGE, K.LDS_EDGE + 1, K.MAX_TOKENS}
    assert all(K.merge_lds(c.N, c.dim) <= K.LDS_DEFAULT for c in K.FWD_CASES)
    assert all(K.merge_lds(c.N, c.dim) <= K.LDS_MERGE_MAX for c in fwd)
    for cases in (fwd, K.BWD_CASES):
        dims = {c.dim for c in cases}
        assert any(d < R.DIM_PASS for d in dims) and R.DIM_PASS in dims and 2 * R.DIM_PASS in dims          # predicated, exact
        assert any(R.DIM_PASS < d < 2 * R.DIM_PASS for d in dims)                                           # ragged second pass
        hids = {c.hid for c in cases}
        assert {4, R.HID_STRIDE - 4, R.HID_STRIDE, R.HID_STRIDE + 4} <= hids
    assert {c.kind for c in K.FWD_CASES} == {"mild", "peaked", "tie", "offset+", "offset-", "underflow", "flat", "masked"}
    for kind in ("mild", "peaked", "tie", "offset+", "offset-", "flat"):
        assert {c.N for c in K.FWD_CASES if c.kind == kind and c.dim == 64 and c.hid == 12} >= set(K.FWD_NS) - {1}, kind
    assert {(c.gated, c.bias) for c in K.FWD_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    big = [c for c in K.FWD_CASES if c.N > R.MERGE_THREADS * R.CHUNK and c.kind == "peaked"]
    assert any(c.where // R.CHUNK >= R.MERGE_THREADS for c in big) and any(c.where == c.N - 1 and c.N % R.CHUNK == 1 for c in big)
    # predictor stage
    pc = K.PRED_CASES
    assert {c.ncls for c in pc} >= {1, 2, R.CLASS_STRIDE, R.CLASS_STRIDE + 1}
    assert {c.pred_bias for c in pc} == {c.gated for c in pc} == {False, True} and {c.no_norm for c in pc} == {0, 1}
    assert {(c.want_pooled, c.want_attn) for c in pc} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c.act for c in pc} == set(K.ACTS) and {c.N for c in pc} == {33, 32801}
    assert {(c.N, c.kind) for c in pc} == {(n, k) for n in (33, 32801) for k in ("mild", "peaked")}
    # backward stage
    bc = K.BWD_CASES
    assert {c.N for c in bc} >= set(K.BWD_NS) and {c.N % R.BWD_ROWS for c in bc} >= {0, 1, 2, 3, 5, 31}
    assert {(c.has_dattn, c.has_draw, c.gated) for c in bc} == {(a, b, g) for a in (0, 1) for b in (0, 1) for g in (0, 1)}
    assert {(c.has_dattn, c.has_draw, c.gated) for c in bc if c.kind == "runner-up"} == {(a, b, g) for a in (0, 1) for b in (0, 1) for g in (0, 1)}
    assert {c.kind for c in bc} == set(K.BWD_KINDS)
    assert all(K.backward_lds(c.dim, c.hid) <= K.LDS_DEFAULT for c in bc)
    assert len({K.fwd_id(c) for c in fwd}) == len(fwd) and len({K.bwd_id(c) for c in bc}) == len(bc)
    assert len({K.pred_id(c) for c in pc}) == len(pc)


# ------------------------------------------------------------------ premises, the emulation inside every bound
@pytest.fixture(scope="module")
def forward_table():
    """[(case, inputs, meta, ref64)] for every forward case but the 1e6-token ones (those: test_large_lds_cases)"""
    out = []
    for c in K.FWD_CASES:
        y, ha, hb, cw, cb, meta = K.forward_inputs(c)
        out.append((c, (y, ha, hb, cw, cb), meta, R.ref64(y, ha, hb, cw, cb)))
    return out


def _check_premise(c, inputs, meta, ref):
    y, ha, hb, cw, cb = inputs
    s = ref["s"].numpy()
    N, top_chunk = c.N, None
    if c.kind in ("peaked", "tie", "underflow"):
        # (underflow: the chunk pushed down lies below -PEAK by construction; the range is the maximum's)
        peak = float(s.max()) if c.kind == "underflow" else float(np.abs(s).max())
        assert K.PEAK_RANGE[0] <= peak <= K.PEAK_RANGE[1], K.fwd_id(c)
        assert float(s[meta["top"]]) == float(s.max())
        top_chunk = meta["top"] // R.CHUNK
    if c.kind == "peaked":
        assert meta["top"] == c.where == int(s.argmax())
    elif c.kind == "tie":
        a, b = meta["pair"]
        assert a != b and float(s[a]) == float(s[b]) == float(s.max())
        assert a // R.CHUNK != b // R.CHUNK or N <= R.CHUNK
        assert N <= R.MERGE_THREADS * R.CHUNK or max(a, b) // R.CHUNK >= R.MERGE_THREADS
    elif c.kind in ("offset+", "offset-"):
        sign = 1.0 if c.kind == "offset+" else -1.0
        assert float(cb[0]) == sign * K.OFFSET and float((sign * s).min()) > K.OFFSET - 15.0
        with np.errstate(over="ignore", under="ignore"):          # exp without the maximum subtraction: inf / below the normals
            e = np.exp(np.float32(s.max()))
        assert not np.isfinite(e) if sign > 0 else e < np.float32(1.2e-38)
    elif c.kind == "underflow":
        b = meta["chunk"]
        lo, hi = b * R.CHUNK, min(N, (b + 1) * R.CHUNK)
        assert b != top_chunk and float(s.max() - s[lo:hi].max()) >= K.UNDERFLOW_GAP
        with np.errstate(under="ignore"):
            assert np.exp(np.float32(s[lo:hi].max()) - np.float32(s.max()), dtype=np.float32) == 0.0
    elif c.kind == "flat":
        assert float(s.max()) == float(s.min()) and abs(float(ref["attn"][0]) - 1.0 / N) < 1e-12
    elif c.kind == "masked":
        idx, b = meta["masked"], meta["chunk"]
        assert set(range(b * R.CHUNK, min(N, (b + 1) * R.CHUNK))) <= set(idx.tolist()) and len(idx) < N
        assert np.isneginf(s[idx]).all() and np.isfinite(np.delete(s, idx)).all() and np.isfinite(y).all()
        assert float(ref["attn"][idx].abs().max()) == 0.0 and bool(np.isfinite(ref["pooled"].numpy()).all())


def test_forward_premises_hold(forward_table):
    for c, inputs, meta, ref in forward_table:
        _check_premise(c, inputs, meta, ref)


def _worst(errs):
    return max((e / t, n) for n, (e, t, *_) in errs.items())


def test_emulation_sits_inside_every_forward_bound(forward_table):
    for c, inputs, meta, ref in forward_table:
        got = R.emulate32(*inputs)
        for name, (err, tol) in K.forward_errors(got, ref).items():
            assert err <= tol, (K.fwd_id(c), name, err, tol)
        if c.kind == "masked":
            assert float(np.abs(got["attn"][meta["masked"]]).max()) == 0.0 and np.isfinite(got["pooled"]).all()
        if c.kind == "tie":
            a, b = meta["pair"]
            assert got["s"][a] == got["s"][b] and got["attn"][a] == got["attn"][b]
        if c.kind == "flat":
            assert (got["attn"] == got["attn"][0]).all()


def test_large_lds_cases():
    """the bags of the large-LDS launches: premises and the emulation inside the bounds (one y per N)"""
    for c in K.LDS_CASES:
        y, ha, hb, cw, cb, meta = K.forward_inputs(c)
        ref = R.ref64(y, ha, hb, cw, cb)
        _check_premise(c, (y, ha, hb, cw, cb), meta, ref)
        for name, (err, tol) in K.forward_errors(R.emulate32(y, ha, hb, cw, cb), ref).items():
            assert err <= tol, (K.fwd_id(c), name, err, tol)


@pytest.fixture(scope="module")
def predict_table():
    import torch
    out = []
    for c in K.PRED_CASES:
        d = K.predict_inputs(c)
        h64 = K.hidden_rows(d["y"], d["a_w"], d["a_b"], d["b_w"], d["b_b"], c.act, torch.float64)
        out.append((c, d, R.ref64(d["y"], h64[0], h64[1], d["c_w"], d["c_b"], d["pred_w"], d["pred_b"])))
    return out


def _emulate_predict(c, d, defect=None):
    import torch
    h32 = K.hidden_rows(d["y"], d["a_w"], d["a_b"], d["b_w"], d["b_b"], c.act, torch.float32)
    return R.emulate32(d["y"], h32[0], h32[1], d["c_w"], d["c_b"], d["pred_w"], d["pred_b"], defect=defect)


def test_predictor_cases(predict_table):
    for c, d, ref in predict_table:
        s = ref["s"].numpy()
        if c.kind == "peaked":
            assert K.PEAK_RANGE[0] <= float(np.abs(s).max()) <= K.PEAK_RANGE[1]
        for name, (err, tol) in K.forward_errors(_emulate_predict(c, d), ref).items():
            assert err <= tol, (K.pred_id(c), name, err, tol)


@pytest.fixture(scope="module")
def backward_table():
    return [(c, K.backward_inputs(c)) for c in K.BWD_CASES]


BWD_ARGS = ("y", "hid_a", "hid_b", "c_w", "attn", "pooled", "d_pooled", "d_attn", "d_raw", "c_ext")


def test_backward_premises_and_emulation(backward_table):
    for c, inp in backward_table:
        ref, nat = inp["ref"], inp["natural"]
        if c.kind == "runner-up":
            s = ref["s"].numpy()
            assert K.PEAK_RANGE[0] <= float(np.abs(s).max()) <= K.PEAK_RANGE[1]
            assert int(s.argmax()) == inp["meta"]["top"] and float(ref["attn"].max()) <= 0.9
            assert abs(float(s[inp["meta"]["second"]]) - 0.98 * K.PEAK) < 1e-3
            assert abs(float(s[inp["meta"]["third"]]) - 0.96 * K.PEAK) < 1e-3
            for name in ("dhid_a", "dcw"):          # the floor rule never decides a case meant to test values
                assert float(ref[name].abs().max()) >= 1e-2 * nat, (K.bwd_id(c), name)
        errs = K.backward_errors(R.emulate32_backward(*(inp[k] for k in BWD_ARGS)), inp)
        assert set(errs) == set(K.GRADS) - (set() if c.gated else {"dhid_b"})
        for name, (err, tol, scale) in errs.items():
            assert (scale <= 1e-9 * nat) == K.floor_expected(c, name), (K.bwd_id(c), name, scale, nat)   # the floor: only where named
            assert err <= tol, (K.bwd_id(c), name, err, tol)


# ------------------------------------------------------------------ the lists have teeth
def test_every_seeded_defect_is_caught(forward_table, predict_table, backward_table):
    """for every defect of the emulation: a case that misses a bound by at least 10x (the first one found is named)"""
    caught = {}
    for defect in R.DEFECTS:
        hit = None
        if defect in R.FWD_DEFECTS:
            for c, inputs, _meta, ref in forward_table:
                if c.N > 2100 and defect not in ("merge_first_1024",):      # (the long bags only where the defect needs them)
                    continue
                ratio, name = _worst(K.forward_errors(R.emulate32(*inputs, defect=defect), ref))
                if ratio >= 10.0:
                    hit = ("forward", K.fwd_id(c), name, ratio)
                    break
            if hit is None:
                for c, d, ref in predict_table:
                    if c.N > 2100:
                        continue
                    ratio, name = _worst(K.forward_errors(_emulate_predict(c, d, defect), ref))
                    if ratio >= 10.0:
                        hit = ("predict", K.pred_id(c), name, ratio)
                        break
        if hit is None and defect in R.BWD_DEFECTS:
            for c, inp in backward_table:
                got = R.emulate32_backward(*(inp[k] for k in BWD_ARGS), defect=defect)
                ratio, name = _worst(K.backward_errors(got, inp))
                if ratio >= 10.0:
                    hit = ("backward", K.bwd_id(c), name, ratio)
                    break
        caught[defect] = hit
        print(f"{defect}: {hit}")
    assert all(caught.values()), {d: R.DEFECTS[d] for d, h in caught.items() if h is None}
    # the loop-trip defects are caught in BOTH directions they exist in
    for defect in ("hid_stops_256", "dim_stops_512"):
        assert any(_worst(K.backward_errors(R.emulate32_backward(*(inp[k] for k in BWD_ARGS), defect=defect), inp))[0] >= 10.0
                   for c, inp in backward_table if c.hid > R.HID_STRIDE or c.dim > R.DIM_PASS), defect


# ------------------------------------------------------------------ refusals, before anything is launched
def _unsupported(lib, rc, word):
    assert rc == UNSUPPORTED and word in lib.rrt_strerror(rc), (rc, lib.rrt_strerror(rc))


# shapes whose launches would not fit: the merge block above 150 KB; the backward block above 64 KB
MERGE_OVERSIZE = ((K.MAX_TOKENS, 4096, 128), (K.MAX_TOKENS, 3072, 4), (900000, 8192, 12))
BACKWARD_OVERSIZE = ((100, 512, 4096), (1, 32, 4088), (1000, 16384, 4))


def test_oversize_shapes_are_refused_everywhere(lib):
    need = C.c_size_t()
    for N, dim, hid in MERGE_OVERSIZE:
        assert K.merge_lds(N, dim) > K.LDS_MERGE_MAX
    for N, dim, hid in BACKWARD_OVERSIZE:
        assert K.backward_lds(dim, hid) > K.LDS_DEFAULT and K.merge_lds(N, dim) <= K.LDS_MERGE_MAX
    assert K.backward_lds(32, 4084) == K.LDS_DEFAULT and lib.rrt_attn_pool_workspace_size(1, 32, 4084, C.byref(need)) == OK
    assert K.merge_lds(K.MAX_TOKENS, 2048) <= K.LDS_MERGE_MAX and lib.rrt_pool_workspace_size(K.MAX_TOKENS, 2048, 128, 1, C.byref(need)) == OK
    fwd = lambda N, dim, hid: lib.rrt_attn_pool_f32(P, P, None, P, None, P, P, P, N, dim, hid, P, 1 << 40, None)      # noqa: E731
    bwd = lambda N, dim, hid: lib.rrt_attn_pool_backward_f32(P, P, None, P, P, P, P, None, None, None, P, P, None, P, N, dim, hid, P,   # noqa: E731
                                                             1 << 40, None)
    pred = lambda N, dim, hid: lib.rrt_pool_predict_f32(P, P, None, None, None, P, None, P, None, P, P, P, 0, N, dim, hid, 1, 2, 0, P,   # noqa: E731
                                                        1 << 40, None)
    for shape in MERGE_OVERSIZE:
        for rc in (lib.rrt_attn_pool_workspace_size(*shape, C.byref(need)), lib.rrt_pool_workspace_size(*shape, 0, C.byref(need)),
                   fwd(*shape), bwd(*shape), pred(*shape)):
            _unsupported(lib, rc, b"merge block's LDS")
    for shape in BACKWARD_OVERSIZE:
        for rc in (lib.rrt_attn_pool_workspace_size(*shape, C.byref(need)), fwd(*shape), bwd(*shape)):
            _unsupported(lib, rc, b"backward block's LDS")
        # (the inference entries have no backward: nothing changes for them)
        assert lib.rrt_pool_workspace_size(*shape, 0, C.byref(need)) == OK
    # the heads' size queries that include this pool
    from test_workspace_sizes_cpu import _head_desc
    for pool in (_lib.BAGPOOL_ATTN, _lib.BAGPOOL_ATTN_GATED, _lib.BAGPOOL_ATTN_DECONF):
        d = _head_desc(_lib.BagmilDesc, None, input_dim=64, emb_act=_lib.ACT_RELU, n_classes=2, pool=pool, pool_hidden=128,
                       pool_act=_lib.ACT_TANH, deconf_k=8, deconf_v=512, deconf_j=128)
        d.enc.dim = 4096
        _unsupported(lib, lib.rrt_bagmil_workspace_size(C.byref(d), K.MAX_TOKENS, C.byref(need)), b"merge block's LDS")
        _unsupported(lib, lib.rrt_bagmil_forward_f32(C.byref(d), C.byref(_lib.BagmilWeights()), P, P, None, 0, None, None, None, None,
                                                    K.MAX_TOKENS, P, 1 << 40, None), b"merge block's LDS")
    d = _head_desc(_lib.MilDesc, "default", input_dim=64, emb_act=_lib.ACT_RELU, n_classes=2, pool_hidden=128, pool_act=_lib.ACT_RELU)
    d.enc.dim, d.enc.ffn_hidden = 4096, 16384
    assert lib.rrt_mil_workspace_size(C.byref(d), K.MAX_TOKENS, C.byref(need)) == UNSUPPORTED
    assert lib.rrt_mil_forward_f32(C.byref(d), C.byref(_lib.MilWeights()), P, P, None, 0, None, K.MAX_TOKENS, P, 1 << 40, None) == UNSUPPORTED


def test_argument_checks(lib):
    need = C.c_size_t()
    ws = lambda N=100, dim=64, hid=12: lib.rrt_attn_pool_workspace_size(N, dim, hid, C.byref(need))      # noqa: E731
    assert ws() == OK and lib.rrt_attn_pool_workspace_size(100, 64, 12, None) == INVALID
    assert ws(N=0) == INVALID and ws(N=-5) == INVALID
    _unsupported(lib, ws(dim=48), b"multiple of 32")
    _unsupported(lib, ws(hid=10), b"multiple of 4")
    _unsupported(lib, ws(N=K.MAX_TOKENS + 1), b"1e6")
    assert ws() == OK
    size = need.value

    def fwd(N=100, dim=64, hid=12, wsp=P, wsb=size, **null):
        a = {k: P for k in ("y", "hid_a", "c_w", "pooled", "attn", "a_raw")} | {"hid_b": None, "c_b": None} | null
        return lib.rrt_attn_pool_f32(a["y"], a["hid_a"], a["hid_b"], a["c_w"], a["c_b"], a["pooled"], a["attn"], a["a_raw"], N, dim, hid,
                                     wsp, wsb, None)
    for name in ("y", "hid_a", "c_w", "pooled", "attn", "a_raw"):
        assert fwd(**{name: None}) == INVALID, name
    assert fwd(N=0) == INVALID
    _unsupported(lib, fwd(dim=48), b"multiple of 32")
    _unsupported(lib, fwd(hid=10), b"multiple of 4")
    _unsupported(lib, fwd(N=K.MAX_TOKENS + 1), b"1e6")
    assert fwd(wsb=size - 1) == WORKSPACE and fwd(wsp=None) == WORKSPACE

    def bwd(N=100, dim=64, hid=12, wsp=P, wsb=size, **over):
        a = {k: P for k in ("y", "hid_a", "c_w", "attn", "pooled", "d_pooled", "dy", "dhid_a", "dwcb")}
        a |= {k: None for k in ("hid_b", "d_attn", "d_raw", "c_ext", "dhid_b")} | over
        return lib.rrt_attn_pool_backward_f32(a["y"], a["hid_a"], a["hid_b"], a["c_w"], a["attn"], a["pooled"], a["d_pooled"],
                                              a["d_attn"], a["d_raw"], a["c_ext"], a["dy"], a["dhid_a"], a["dhid_b"], a["dwcb"], N, dim,
                                              hid, wsp, wsb, None)
    for name in ("y", "hid_a", "c_w", "attn", "pooled", "d_pooled", "dy", "dhid_a", "dwcb"):
        assert bwd(**{name: None}) == INVALID, name
    assert bwd(N=0) == INVALID
    assert bwd(d_attn=P) == INVALID                   # d_attn without c_ext
    assert bwd(hid_b=P) == INVALID                    # hid_b without dhid_b
    _unsupported(lib, bwd(dim=48), b"multiple of 32")
    _unsupported(lib, bwd(hid=10), b"multiple of 4")
    _unsupported(lib, bwd(N=K.MAX_TOKENS + 1), b"1e6")
    assert bwd(wsb=size - 1) == WORKSPACE and bwd(wsp=None) == WORKSPACE
    assert bwd(d_attn=P, c_ext=P, wsb=size - 1) == WORKSPACE and bwd(hid_b=P, dhid_b=P, d_raw=P, wsb=size - 1) == WORKSPACE

    pws = lambda N=100, dim=64, hid=12, gated=0: lib.rrt_pool_workspace_size(N, dim, hid, gated, C.byref(need))      # noqa: E731
    assert pws() == OK
    psize = need.value

    def pred(N=100, dim=64, hid=12, act=1, ncls=2, compute=0, wsp=P, wsb=psize, **null):
        a = {k: P for k in ("y", "a_w", "c_w", "pred_w", "logits")} | null
        return lib.rrt_pool_predict_f32(a["y"], a["a_w"], None, None, None, a["c_w"], None, a["pred_w"], None, None, a["logits"], None, 0,
                                        N, dim, hid, act, ncls, compute, wsp, wsb, None)
    for name in ("y", "a_w", "c_w", "pred_w", "logits"):
        assert pred(**{name: None}) == INVALID, name
    assert pred(N=0) == INVALID and pred(ncls=0) == INVALID
    _unsupported(lib, pred(dim=48), b"multiple of 32")
    _unsupported(lib, pred(hid=10), b"multiple of 4")
    _unsupported(lib, pred(act=9), b"act")
    _unsupported(lib, pred(compute=7), b"compute")
    _unsupported(lib, pred(N=K.MAX_TOKENS + 1), b"1e6")
    assert pred(wsb=psize - 1) == WORKSPACE and pred(wsp=None) == WORKSPACE
