"""CPU: the case lists of tests/test_train_blocks_matrix.py cover what that module claims, and its Python restatement of the
dispatch rules is the compiled one.  The split-K rule of csrc/linear_bwd.hip has no export of its own: the number of row chunks
is recovered from rrt_linear_backward_workspace_size = align256(4 N K) + align256(4 S N K) + align256(4 SB N) and compared with
the restatement over a sweep of shapes.  The instantiations the two files compile (gemm_tn_kernel<FAST>, ln_backward_kernel<NV>,
reduce_partials_kernel<NWV>) are read out of the sources and must all be reached; so must every cell of {FAST, general} x
{direct, 3-D, XCD} the rule can produce over the sweep, every (dX, dW, db) combination, the last-chunk sizes {1, < 32, 32, full}
and both colsum arms.  The fp32 CPU evaluation of every synth case sits inside its tolerance, the integer cases stay below 2^24,
and every refusal of the entries involved comes back before anything is launched (dummy pointers, never followed)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import test_train_blocks_matrix as T
from rrt_mil_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
PTR = 0x1000                                # a non-null "device pointer": every call below is refused before it is followed
SWEEP_NK = (5, 32, 126, 128, 129, 256, 384, 1536)
SWEEP_M = sorted({m for k in range(0, 4200 // 32 + 1) for m in (32 * k - 1, 32 * k, 32 * k + 1) if 1 <= m <= 4200} | {4200})


@pytest.fixture(scope="module")
def lib():
    from rrt_mil_amd.build import build
    build()
    return _lib.load()


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def chunks_from_workspace(lib, M, N, K):
    """the S values the library's workspace size allows for (one, unless 4 N K < 256 hides it in the alignment)"""
    need = C.c_size_t()
    assert lib.rrt_linear_backward_workspace_size(M, N, K, C.byref(need)) == 0
    mid = need.value - T.align256(4 * N * K) - T.align256(4 * (-(-M // 128)) * N)
    return [S for S in range(1, 2 * (M // 128) + 4) if T.align256(4 * S * N * K) == mid]


def test_restatement_is_the_compiled_rule(lib):
    """linear_bwd_chunks in Python against the S the library sizes its workspace for: every case and the sweep"""
    shapes = {(c.M, c.N, c.K) for c in T.LIN_CASES} | set(itertools.product(SWEEP_M, SWEEP_NK, SWEEP_NK))
    for M, N, K in sorted(shapes):
        S, rpc = T.linear_bwd_chunks(M, N, K)
        got = chunks_from_workspace(lib, M, N, K)
        assert S in got and (len(got) == 1 or 4 * N * K < 256), (M, N, K, S, got)
        assert rpc % 32 == 0 and rpc >= 32 and (S - 1) * rpc < M <= S * rpc                  # no empty chunk
        need = C.c_size_t()
        lib.rrt_linear_backward_workspace_size(M, N, K, C.byref(need))
        assert need.value == T.linear_bwd_workspace(M, N, K)
    src = _src("linear_bwd.hip")
    assert "constexpr int TN_BN = 128, TN_BK = 128, TN_BM = 32" in src and ": 768;" in src
    assert "if (S % 8 == 0 && !plain)" in src and "const int SB = (M + 127) / 128;" in src
    assert 'rrt_tune_env("RRT_TN_BLOCKS")' in src and 'rrt_tune_env("RRT_TN_PLAIN_GRID")' in src    # tuning builds only
    ln = _src("ln_bwd.hip")
    assert "constexpr int LNB_BLOCKS = 512;" in ln and "need < 4096 ? need : 4096" in ln
    assert re.search(r"if \(dim <= 256\) RRT_LNB\(1\);\s+else if \(dim <= 512\) RRT_LNB\(2\);\s+else if \(dim <= 1024\) RRT_LNB\(4\);"
                     r"\s+else RRT_LNB\(8\);", ln)
    assert "if (S >= 64 && nb <= 64) reduce_partials_kernel<16>" in src


def test_every_instantiation_is_reached():
    src, ln = _src("linear_bwd.hip"), _src("ln_bwd.hip")
    tn = set(re.findall(r"gemm_tn_kernel<(true|false)><<<", src))
    assert tn == {"true", "false"}
    reached = {"true" if T.tn_cell(c.M, c.N, c.K)[0] else "false" for c in T.LIN_CASES if "W" in c.outs}
    assert reached == tn
    nvs = {int(v) for v in re.findall(r"RRT_LNB\((\d)\);", ln)}
    assert nvs == {1, 2, 4, 8} == {T.ln_nv(c.dim) for c in T.LN_CASES}
    # each NV with every lane of its last float4 group in the row, and with lanes past the row
    assert {(T.ln_nv(c.dim), c.dim == 256 * T.ln_nv(c.dim)) for c in T.LN_CASES} == set(itertools.product((1, 2, 4, 8), (True, False)))
    nwv = {int(v) for v in re.findall(r"reduce_partials_kernel<(\d+)><<<", src)}
    assert nwv == {4, 16}
    got = {T.reduce_waves(T.ln_blocks(c.L), 2 * c.dim) for c in T.LN_CASES}
    for c in T.LIN_CASES:                       # dW with db: reduce<4> with two segments; dW alone / db alone: launch_reduce_partials
        S, _ = T.linear_bwd_chunks(c.M, c.N, c.K)
        if "W" in c.outs and S > 1:
            got.add(4 if "b" in c.outs else T.reduce_waves(S, c.N * c.K))
    assert got == nwv
    # both sides of the reduce<16> switch at 64 partials, fewer waves than a block, the grid-stride loop past 512 blocks
    blocks = {T.ln_blocks(c.L) for c in T.LN_CASES}
    assert {1, 2, 63, 64, 65, 512} <= blocks and any(c.L < 4 for c in T.LN_CASES) and any(c.L > 2048 for c in T.LN_CASES)
    for dim, Ls in T.LN_SHAPES.items():
        assert len(set(Ls)) == 3 and dim % 4 == 0 and dim <= 2048
    for L in T.LN_LS:
        assert sum(L in Ls for Ls in T.LN_SHAPES.values()) >= 2, L
    assert set(T.LN_SHAPES) == {4, 64, 256, 260, 512, 516, 768, 1024, 1028, 2048}
    assert {1, 3, 4, 5, 255, 256, 257, 2047, 2049} <= set(T.LN_LS) == {L for Ls in T.LN_SHAPES.values() for L in Ls}
    assert {c.family for c in T.LN_CASES} == set(T.LN_FAMILIES) and len(T.LN_CASES) == 120


# cells of {FAST, general} x {direct, 3d, xcd} that no shape of the sweep produces: none today (kept explicit: a cell that
# stops being produced must be listed here, not dropped silently)
UNREACHABLE_CELLS = set()


def test_grid_cells_and_output_combinations():
    cells = {T.tn_cell(M, N, K) for M, N, K in itertools.product(SWEEP_M, SWEEP_NK, SWEEP_NK)}
    every = set(itertools.product((True, False), ("direct", "3d", "xcd")))
    assert every - cells == UNREACHABLE_CELLS, (every - cells, UNREACHABLE_CELLS)
    tn = [c for c in T.LIN_CASES if "W" in c.outs]
    assert {T.tn_cell(c.M, c.N, c.K) for c in tn} == cells
    # every non-empty (dX, dW, db) at an S == 1 and an S > 1 shape
    for want_direct in (True, False):
        assert any({c.outs for c in T.LIN_CASES if (c.M, c.N, c.K) == s} >= set(T.ALL_COMBOS)
                   and (T.linear_bwd_chunks(*s)[0] == 1) == want_direct for s in T.COMBO_SHAPES)
    # last chunk: 1 row, less than a 32-row stage, exactly one stage, a full chunk
    last = {(T.last_chunk(c.M, c.N, c.K), T.linear_bwd_chunks(c.M, c.N, c.K)) for c in tn}
    assert any(l == 1 and S > 1 for l, (S, r) in last) and any(1 < l < 32 and S > 1 for l, (S, r) in last)
    assert any(l == 32 and S > 1 for l, (S, r) in last) and any(l == r and S > 1 for l, (S, r) in last)
    # the scalar-load arms of fetch (N or K no multiple of 4), tiles_n / tiles_k > 1 under the XCD order, two rounds of XCDs
    assert any(c.N % 4 and c.K % 4 for c in tn) and any(c.N < 128 and T.tn_cell(c.M, c.N, c.K)[1] == "xcd" for c in tn)
    xcd = [c for c in tn if T.tn_cell(c.M, c.N, c.K)[1] == "xcd"]
    assert any(c.K > 128 for c in xcd) and any(c.N > 128 for c in xcd) and any(T.linear_bwd_chunks(c.M, c.N, c.K)[0] == 16 for c in xcd)
    # dW alone at N = crmsa_k <= 8
    assert any(c.outs == "W" and c.N <= 8 for c in T.LIN_CASES)
    # colsum: SB == 1 writes directly, SB > 1 goes through the reduce; the 4-row loop's tail of 0 .. 3 rows; N past one block
    col = [c for c in T.LIN_CASES if c.outs == "b"]
    assert {c.form.split("/")[1] for c in col} == {"direct", "reduce"}
    assert {int(c.form.rsplit("tail", 1)[1]) for c in col} == {0, 1, 2, 3} and any(c.N > 256 for c in col) and any(c.M == 1 for c in col)
    # dX through ragged transposes
    assert {(c.N, c.K % 4 != 0) for c in T.LIN_CASES if c.outs == "X" and c.form.endswith("ragged")} >= {(32, True), (96, True)}
    for c in T.LIN_CASES:
        assert "X" not in c.outs or c.N % 32 == 0
        assert T.lin_form(c.M, c.N, c.K, c.outs) == c.form
    ids = [T.lin_id(c) for c in T.LIN_CASES]
    assert len(set(ids)) == len(ids)


def test_element_wise_case_lists(lib):
    assert set(T.ACT_NS) == {4, 1020, 1024, 1028, 262148} and all(n % 4 == 0 for n in T.ACT_NS)
    assert {(c.which, c.act, c.p) for c in T.ACT_CASES} == set(itertools.product(("forward", "backward"), ("gelu", "relu"), (0.0, 0.5, 0.1)))
    g = T.act_grid()
    assert len(g) == 4 + 193 + 6 and np.signbit(g[1]) and g[1] == 0 and g[2] == np.float32(2.0 ** -130) > 0
    assert {-12.0, 12.0, 0.125, 20.0, -88.0, 100.0} <= set(g.tolist())
    x, dh = T.act_inputs(1020)
    assert np.array_equal(x[:len(g)], g) and np.abs(x[len(g):]).max() > 6
    xi, di = T.act_inputs(1024, integer=True)
    assert set(np.unique(xi)) == set(range(-3, 4)) and (xi == np.round(xi)).all()
    # partition_rows: a grid that fits the launch and one that loops over it, rows of one and of several 256-column passes
    forms = {c.form for c in T.part_cases()}
    assert forms >= {"partition_rows/once/cols-once", "partition_rows/once/cols-loop", "partition_rows/stride/cols-once"}
    assert {(L, rn, d) for L, rn, d in T.PART_SHAPES} >= set(itertools.product((1, 50, 777, 4097), (4, 8), (4, 260, 512)))
    for L, rn, d in T.PART_SHAPES:
        assert T._grid_np(L, rn) > L                        # pad slots in every case
    assert set(T.MASK_NS) == {1, 255, 256, 257, 100003}
    assert T.TR_JOBS == (1, 2, _lib.TRANSPOSE_MAX_JOBS) and "TRANSPOSE_MAX_JOBS = 2 * RRT_MAX_RMSA_LAYERS + 2;" in _src("internal.h")
    assert {s for n in T.TR_JOBS for s in T.tr_shapes(n)} == set(T.TR_SHAPES)
    # the mask reference at the entry's own float p differs from the double's threshold, which is what is passed on
    assert int(np.float32(0.1) * 4294967296.0) != int(0.1 * 4294967296.0)


@pytest.mark.parametrize("c", T.LIN_CASES, ids=T.lin_id)
def test_linear_references_on_the_cpu(c):
    """integer: every entry an integer below 2^24 (and the family is no fixed point of a row shift); synth / cancel: numpy's fp32
    evaluation lies inside the tolerance, and the cancelling variant's dW, db are small against their terms"""
    for family, compute in T.lin_runs(c):
        ref, tol = T.lin_reference(c, family, compute)
        r32 = T.lin_reference32(c, family, compute)
        for name, r in ref.items():
            if family == "integer":
                assert np.abs(r).max() < 2 ** 24 and np.array_equal(r, np.round(r)) and np.array_equal(r32[name], r), (name, compute)
                assert c.M < 3 or np.abs(r).max() > 0
                continue
            chain, t = tol[name]
            err = float(np.abs(r32[name].astype(np.float64) - r).max())
            assert np.isfinite(err) and err <= t, (T.lin_id(c), family, compute, name, err, t, chain)
        if family == "cancel" and c.M >= 64:
            plain, _ = T.lin_reference(c, "synth", 0)
            for name in ("dW", "db"):
                if name in ref:
                    assert np.abs(ref[name]).max() < 0.05 * np.abs(plain[name]).max(), name


@pytest.mark.parametrize("dim,L", [(dim, L) for dim, Ls in T.LN_SHAPES.items() for L in Ls])
def test_layernorm_references_on_the_cpu(dim, L):
    """what the families are for: a one-pass variance fails the offset rows, eps dominates rstd on the flat ones; the fp32
    evaluation is finite and within each tolerance by construction"""
    for fam in T.LN_FAMILIES:
        x, dy, add, gamma = T.ln_inputs(fam, L, dim)
        assert np.isfinite(x).all()
        ref, bounds = T.ln_bounds(fam, L, dim, True)
        for name, (e32, tol) in bounds.items():
            assert np.isfinite(e32) and e32 <= tol and tol > 0, (fam, name)
        x64 = x.astype(np.float64)
        var = x64.var(-1)
        if fam == "flat":
            assert (var < 1e-5 / 100).all() and (L < 2 or dim < 2 or var[1] > 0) and var[0] == 0
        if fam == "offset" and dim >= 64:
            onepass = (x * x).mean(-1, dtype=np.float32) - x.mean(-1, dtype=np.float32) ** 2      # E[x^2] - E[x]^2 in fp32
            assert np.abs(onepass - var).max() > 1e-4 * var.max()         # four orders above fp32's rounding
        if fam == "outlier":
            assert (np.abs(x).max(-1) == 1e4).all()


def test_linear_backward_refusals(lib):
    need = C.c_size_t()
    assert lib.rrt_linear_backward_workspace_size(77, 32, 40, C.byref(need)) == 0

    def call(dY=PTR, X=PTR, W=PTR, dX=PTR, dW=PTR, db=PTR, M=77, N=32, K=40, compute=0, ws=PTR, nbytes=None):
        return lib.rrt_linear_backward_f32(dY, X, W, dX, dW, db, M, N, K, compute, ws, need.value if nbytes is None else nbytes, None)
    assert call(N=40) == -2 and b"multiple of 32" in lib.rrt_strerror(-2)       # dX with N % 32
    assert call(compute=3) == -2 and call(compute=-1) == -2
    assert call(nbytes=need.value - 1) == -3 and call(ws=None) == -3             # a short workspace
    assert call(dY=None) == -1 and call(M=0) == -1 and call(N=0) == -1 and call(K=0) == -1
    assert call(W=None) == -1 and call(X=None) == -1                             # dX needs W, dW needs X
    assert lib.rrt_linear_backward_workspace_size(0, 32, 40, C.byref(need)) == -1
    assert lib.rrt_linear_backward_workspace_size(77, 32, 40, None) == -1


def test_layernorm_backward_refusals(lib):
    g = _lib.region_grid(300, 8)

    def call(dy=PTR, x=PTR, gamma=PTR, dx=PTR, dgb=PTR, L=300, dim=64, grid=None, ws=PTR, nbytes=None):
        return lib.rrt_layernorm_backward_f32(dy, x, gamma, None, dx, dgb, L, dim, grid, ws, 512 * 2 * dim * 4 if nbytes is None else nbytes,
                                              None)
    assert call(dim=66) == -1 and call(dim=2052) == -2 and call(dim=0) == -1
    assert call(L=299, grid=C.byref(g)) == -1                                    # g->L != L
    assert call(nbytes=512 * 2 * 64 * 4 - 1) == -3 and call(ws=None) == -3
    assert call(dy=None) == -1 and call(x=None) == -1 and call(gamma=None) == -1 and call(dx=None) == -1 and call(dgb=None) == -1
    assert call(L=0) == -1


def test_stage_entry_refusals(lib):
    """every refusal of the five rrt_debug_* stage entries comes back on the host"""
    for name in ("rrt_debug_act_forward_f32", "rrt_debug_act_backward_f32", "rrt_debug_partition_rows_f32", "rrt_debug_drop_mask_f32",
                 "rrt_debug_transpose_batch_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    hdr = open(os.path.join(os.path.dirname(CSRC), os.pardir, "include", "rrt_hip.h")).read()
    assert all(f"int {n}(" in hdr for n in _lib.SIGNATURES if n.startswith("rrt_debug_"))
    Q = PTR + 0x1000
    for fn in (lib.rrt_debug_act_forward_f32, lib.rrt_debug_act_backward_f32):
        def act(a=PTR, b=Q, n=1024, code=_lib.ACT_GELU, p=0.0, layer=0):
            return fn(a, b, n, code, p, 1, layer, None)
        assert act(a=None) == -1 and act(b=None) == -1 and act(n=0) == -1 and act(n=-4) == -1
        assert act(n=1022) == -2 and b"multiple of 4" in lib.rrt_strerror(-2)
        for code in (_lib.ACT_NONE, _lib.ACT_TANH, _lib.ACT_SIGMOID, 7, -1):
            assert act(code=code) == -2, code
        assert act(p=1.0) == -1 and act(p=-0.1) == -1 and act(p=float("nan")) == -1 and act(layer=-1) == -1
    assert lib.rrt_debug_act_backward_f32(PTR, PTR, 1024, _lib.ACT_RELU, 0.0, 1, 0, None) == -1      # dh == hpre
    g = _lib.region_grid(300, 8)

    def part(src=PTR, dst=Q, dim=64, grid=C.byref(g), p=0.0, layer=0, scale=1.0):
        return lib.rrt_debug_partition_rows_f32(src, dst, dim, grid, p, 1, layer, scale, None)
    assert part(src=None) == -1 and part(dst=None) == -1 and part(dst=PTR) == -1 and part(grid=None) == -1 and part(dim=0) == -1
    assert part(dim=66) == -2 and part(p=1.0) == -1 and part(layer=-1) == -1 and part(scale=-1.0) == -1 and part(scale=float("nan")) == -1
    for field, value in (("L", 0), ("L", g.H * g.H + 1), ("H", 0), ("s", 0), ("regions_side", g.regions_side + 1), ("H", 5000)):
        bad = _lib.Grid(g.L, g.H, g.s, g.regions_side, g.add)
        setattr(bad, field, value)
        assert part(grid=C.byref(bad)) == -1, (field, value)

    def mask(src=PTR, dst=Q, n=100, p=0.5, layer=0, scale=1.0):
        return lib.rrt_debug_drop_mask_f32(src, dst, n, p, 1, layer, scale, None)
    assert mask(src=None) == -1 and mask(dst=None) == -1 and mask(n=0) == -1 and mask(n=2 ** 31) == -1
    assert mask(p=1.0) == -1 and mask(p=-1.0) == -1 and mask(layer=-1) == -1 and mask(scale=-0.5) == -1

    def tr(n=2, ins=(PTR, PTR), outs=(Q, Q), R=(3, 3), Cc=(5, 5), arrays=(True,) * 4):
        m = max(n, 1)
        a = [(C.c_void_p * m)(*(list(ins) + [PTR] * m)[:m]), (C.c_void_p * m)(*(list(outs) + [Q] * m)[:m]),
             (C.c_int32 * m)(*(list(R) + [3] * m)[:m]), (C.c_int32 * m)(*(list(Cc) + [5] * m)[:m])]
        a = [x if on else None for x, on in zip(a, arrays)]
        return lib.rrt_debug_transpose_batch_f32(a[0], a[1], a[2], a[3], n, None)
    assert tr(n=0) == -1 and tr(n=-1) == -1 and tr(n=_lib.TRANSPOSE_MAX_JOBS + 1) == -2
    for k in range(4):
        assert tr(arrays=tuple(i != k for i in range(4))) == -1
    assert tr(ins=(PTR, None)) == -1 and tr(outs=(None, Q)) == -1 and tr(outs=(Q, PTR)) == -1        # in == out
    assert tr(R=(3, 0)) == -1 and tr(Cc=(-5, 5)) == -1 and tr(R=(2 ** 20, 3), Cc=(2 ** 20, 5)) == -1
