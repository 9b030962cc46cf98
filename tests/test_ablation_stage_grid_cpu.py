"""CPU: the case lists of tests/test_ablation_stage_matrix.py cover what that module claims -- every K instantiation of
csrc/peg.hip in both kinds, both LDS / global branches of both score-map kernels by the restated formulas, the edge of the
value EPEG's tap table -- the new size exports equal their restatements, every refusal of the stage entry points returns its
code before anything is launched, the restatements are the oracle's own lines, and the criteria pass and fail where they
should.  Nothing is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import test_ablation_stage_matrix as M
from oracle import rrt_oracle as O
from rrt_mil_amd import _lib
from rrt_mil_amd.build import build

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
PTR = 0x1000                       # a non-null pointer no refusal may touch


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


# ------------------------------------------------------------------ A. PEG / PPEG
def test_peg_cases_are_the_table_of_the_issue():
    assert M.PEG_KS == (1, 3, 5, 7, 9, 11) and M.PEG_CS == (64, 96) and M.PEG_NS == (1, 2, 3, 5, 36, 37, 49, 50, 64, 65, 290)
    assert len(M.PEG_CASES) == len(set(M.PEG_CASES)) == 2 * 6 * 2 * 2 * 2 * 11
    assert {c[:2] for c in M.PEG_CASES} == set(M.PEG_GROUPS)
    side = {N: M.peg_sides(N, "peg")[0] for N in M.PEG_NS}
    assert side == {1: 1, 2: 2, 3: 2, 5: 3, 36: 6, 37: 7, 49: 7, 50: 8, 64: 8, 65: 9, 290: 18}
    wrap = {N: side[N] ** 2 - N for N in M.PEG_NS}
    assert wrap[2] == 2 and wrap[5] == 4 and wrap[36] == wrap[49] == wrap[64] == 0 and wrap[37] == 12 and wrap[50] == 14
    assert all(0 <= wrap[N] <= N for N in M.PEG_NS)                     # the wrapped tail never outgrows the bag
    assert M.peg_sides(36, "ppeg") == (6, 7) and M.peg_sides(37, "ppeg") == (7, 7) and M.peg_sides(5, "ppeg") == (3, 7)
    tiles = {N: ((side[N] + 7) // 8) ** 2 for N in M.PEG_NS}
    assert tiles[64] == 1 and tiles[65] == 4 and tiles[290] == 9 and side[290] % 8 != 0
    for N in range(1, 2000):                                             # the exact ceil(sqrt(N))
        H0 = M.peg_sides(N, "peg")[0]
        assert (H0 - 1) ** 2 < N <= H0 * H0


def test_every_peg_instantiation_is_reached_and_fits_the_cu():
    src = _src("peg.hip")
    fwd = sorted(int(k) for k in re.findall(r"RRT_PEG\((\d+)\);", src))
    bwd = sorted(int(k) for k in re.findall(r"RRT_PEGW\((\d+)\);", src))
    assert fwd == bwd == [3, 5, 7, 9, 11]
    reached = {kind: {M.peg_kk(kind, k) for kd, k, *_ in M.PEG_CASES if kd == kind} for kind in M.PEG_KINDS}
    assert reached["peg"] == set(fwd)
    assert reached["ppeg"] == {K for K in fwd if K >= 5}                 # PPEG's 5 x 5 conv: no smaller template
    assert src.count("static_assert(lds <= PEG_LDS_MAX") == 2
    for K in fwd:
        assert M.peg_fwd_lds(K) <= M.LDS_MAX and M.peg_dw_lds(K) <= M.LDS_MAX, K
    assert M.peg_dw_lds(11) == 92928
    # what the kernel asked for while the partial sums sat behind the patch: over the CU at K = 11
    assert ((8 + 10) ** 2 * 64 + 3 * 121 * 64) * 4 == 175872 > M.LDS_MAX


def test_peg_workspace_export_is_the_restated_formula(lib):
    n = C.c_size_t()
    for kind in M.PEG_KINDS:
        for k in M.PEG_KS:
            for Cc in (4, 64, 96, 512):
                for N in M.PEG_NS + (899, 900, 901, 4097):
                    assert lib.rrt_peg_backward_workspace_size(N, Cc, k, int(kind == "ppeg"), C.byref(n)) == 0
                    assert n.value == M.peg_workspace_bytes(N, Cc, k, kind), (kind, k, Cc, N)


def test_pos_restatement_is_the_oracles():
    for case in [c for c in M.PEG_CASES if c[4] == 64 and c[5] in (2, 5, 36, 37, 65)]:
        kind, k, one_d, bias, Cc, N = case
        x, _ = M.peg_bag(N, Cc)
        y64 = O._pos64(x.astype(np.float64), M.peg_params(kind, k, one_d, bias, Cc), kind, one_d)
        ref = M.peg_reference(*case, torch.float64)
        assert np.abs(ref["y"] - y64).max() <= 1e-12 * max(1.0, np.abs(y64).max()), case
        assert set(ref) == {"y", "dx"} | {f"dw{i}" for i in range(len(M.peg_names(kind)))} | \
            ({f"db{i}" for i in range(len(M.peg_names(kind)))} if bias else set())


def test_peg_criteria_pass_and_fail_where_they_should():
    """float32 eager passes its own bound; a dropped wrapped copy (dx of the wrapped rows loses its second contribution)
    and a dropped border tap fail"""
    case = ("peg", 3, False, True, 64, 5)
    ref, ref32 = M.peg_reference(*case, torch.float64), M.peg_reference(*case, torch.float32)
    before = len(M.RECORDS)
    fails = []
    for what in ref:
        M.judge("A", "cpu", "cpu", what, ref32[what], ref[what], ref32[what], what != "y", fails)
    assert fails == []
    # dx without the wrapped copies' gradient: the adjoint stencil's output on the first N positions only
    x, dy = M.peg_bag(5, 64)
    st = M.peg_params("peg", 3, False, True, 64)
    xl = M._t(np.concatenate([x, x[:4]]), torch.float64, True)
    w = M._t(st["pos_embedding.proj.weight"], torch.float64)
    feat = xl.t().reshape(1, 64, 3, 3)
    y = (feat + torch.nn.functional.conv2d(feat, w, None, padding=1, groups=64)).flatten(2)[0].t()[:5]
    (y * M._t(dy, torch.float64)).sum().backward()
    unfolded = xl.grad.numpy()[:5].astype(np.float32)
    assert np.abs(unfolded[4] - ref["dx"][4]).max() < 1e-5               # the one token that was not wrapped
    M.judge("A", "cpu", "cpu", "dx", unfolded, ref["dx"], ref32["dx"], True, fails)
    assert len(fails) == 1
    bad = ref32["y"].copy()
    bad[0] -= np.float32(1e-3)                                           # one row off by 1e-3
    M.judge("A", "cpu", "cpu", "y", bad, ref["y"], ref32["y"], False, fails)
    assert len(fails) == 2
    del M.RECORDS[before:]


# ------------------------------------------------------------------ B. the score map
def test_scoremap_cases_reach_every_branch_of_both_kernels():
    assert M.SM_PS == (1, 4, 16, 64, 81, 100, 121, 144, 196, 225) and M.SM_HEADS == ((2, 64), (3, 16), (2, 80))
    assert len(M.SM_CASES) == len(set(M.SM_CASES)) == (10 * 3 + 2) * 3 * 2
    for P, heads, hd, k, fam in M.SM_CASES:
        assert M.sm_path(P, k, 1) == M.SM_FWD_PATH[P] and M.sm_path(P, k, 3) == M.SM_BWD_PATH[P], (P, k)
        assert (k == 63) <= (P in (4, 16)) and (k // 2 >= P or k != 63)
    assert {M.sm_path(P, k, 1) for P, _, _, k, _ in M.SM_CASES} == {"lds", "lds>64K", "global"}
    assert {M.sm_path(P, k, 3) for P, _, _, k, _ in M.SM_CASES} == {"lds", "lds>64K", "global"}
    # the thresholds the issue names: the first P (a square) of each branch, and the last map that fits
    sq = [s * s for s in range(1, 17)]
    first = lambda maps, path, k: min(P for P in sq if M.sm_path(P, k, maps) == path)
    assert first(1, "lds>64K", 3) == 144 and first(1, "global", 3) == 225 and first(3, "lds>64K", 3) == 81 and first(3, "global", 3) == 121
    assert M.sm_path(196, 15, 1) == "lds>64K" and (196 * 196 + 225 + 4 * 196) * 4 == 157700
    assert M.sm_path(100, 15, 3) == "lds>64K"
    # the launchers use the same expressions
    src = _src("epeg_variants.hip")
    assert "((size_t)maps * P * P + (size_t)k * k + 4 * (size_t)P) * sizeof(float)" in src and "lds <= 160 * 1024 ? 0" in src
    assert {c[:3] for c in M.SM_CASES} == set(M.SM_GROUPS) and {c[:3] for c in M.VP_CASES} == set(M.VP_GROUPS)
    assert {hd for _, hd in M.SM_HEADS} == {64, 16, 80}                 # one round of the lane loops, a quarter, two rounds


def test_scoremap_scratch_export_is_the_restated_formula(lib):
    n = C.c_size_t()
    for R in (1, 2, 3, 64):
        for P in M.SM_PS + (143, 169, 195, 197, 224, 256):
            for heads in (1, 3, 8):
                for k in (1, 3, 15, 63):
                    for backward in (0, 1):
                        assert lib.rrt_attn_scoremap_scratch_size(R, P, heads, k, backward, C.byref(n)) == 0
                        assert n.value == M.sm_scratch_bytes(R, P, heads, k, backward), (R, P, heads, k, backward)


@pytest.mark.parametrize("P", [P for P in M.SM_PS if P <= 81])
def test_scoremap_families_hold_what_they_promise(P):
    """the peaked window, the numpy restatement against the torch one, fp32 eager inside its own bound"""
    before = len(M.RECORDS)
    for case in [c for c in M.SM_CASES if c[0] == P and c[1:3] != (2, 80)]:
        _, heads, hd, k, fam = case
        qkv, pw, dO, top = M.sm_inputs(*case)
        assert (M.PEAK_WINDOW[0] <= top <= M.PEAK_WINDOW[1]) if fam == "peaked" else top < 25.0, (case, top)
        ref, ref32 = M.sm_reference(*case, torch.float64), M.sm_reference(*case, torch.float32)
        assert np.abs(ref["o"] - M.scoremap64(qkv, pw, M.sm_regions(P), P, heads, hd)[0]).max() <= 1e-12
        fails = []
        for what in ref:
            err, e32, bound = M.judge("B", "cpu", "cpu", what, ref32[what], ref[what], ref32[what], what != "o", fails)
            assert np.isfinite(e32) and e32 < 2e-4, (case, what, e32)
        assert fails == []
    del M.RECORDS[before:]


# ------------------------------------------------------------------ C. the value EPEG
def test_value_cases_are_the_table_of_the_issue():
    assert M.VP_HEADS == ((8, 64), (3, 16), (2, 160), (4, 4)) and M.VP_SS == (1, 2, 3, 7, 11, 16) and M.VP_RS == (1, 3)
    assert len(M.VP_CASES) == len(set(M.VP_CASES)) == 4 * (6 * 5 + 1) * 2 * 2 * 2
    dims = [h * d for h, d in M.VP_HEADS]
    assert max(dims) > 256 and any(d % 64 for d in dims) and all(d % 4 == 0 for d in dims)
    for heads, hd in M.VP_HEADS:                                       # (c % h) * hd + c / h is a permutation; told from its
        src = [M.vp_src_col(c, heads, hd) for c in range(heads * hd)]  # inverse wherever heads != hd
        inv = [(c % hd) * heads + c // hd for c in range(heads * hd)]
        assert sorted(src) == list(range(heads * hd)) and [src[i] for i in inv] == list(range(heads * hd))
        assert (src != inv) == (heads != hd)
    assert sum(h != d for h, d in M.VP_HEADS) >= 3
    kinds = {(k, two_d) for *_, k, two_d, _, _, _ in M.VP_CASES}
    assert kinds == {(3, False), (9, False), (15, False), (3, True), (5, True), (63, True)}
    assert {s for _, _, s, k, *_ in M.VP_CASES if k == 63} == {2}
    assert any(k // 2 >= s for _, _, s, k, *_ in M.VP_CASES)             # a stencil wider than the image


def test_value_tap_table_edge():
    """63 x 63 taps: the bias is tap 3969, thread 129's sixteenth slot; one more tap per side would not fit"""
    ntap = 63 * 63
    assert ntap == 3969 and ntap // M.VP_THREADS == M.VP_QMAX - 1 and ntap % M.VP_THREADS == 129
    assert ntap + 1 <= M.VP_QMAX * M.VP_THREADS < 65 * 65 + 1
    src = _src("epeg_variants.hip")
    assert "constexpr int QMAX = 16;" in src and "(size_t)k * (two_d ? k : 1) + 1 > 16 * 256" in src


def test_value_restatement_is_the_oracles():
    """the torch lines against O._inner_attention64's image layout and O._conv_dw64, and against the channel map"""
    for heads, hd, s, k, two_d, R in [(3, 16, 3, 3, True, 3), (4, 4, 2, 63, True, 1), (2, 160, 7, 9, False, 1), (8, 64, 1, 15, False, 3)]:
        dim, P = heads * hd, s * s
        a = M.vp_inputs(heads, hd, s, k, two_d, R)
        ref = M.vp_reference(heads, hd, s, k, two_d, R, False, True, torch.float64)
        v = a["qkv"][:, 2 * dim:].astype(np.float64).reshape(R, P, heads, hd).transpose(0, 2, 1, 3)      # [B_, h, P, hd]
        img = v.transpose(0, 3, 1, 2).reshape(R, dim, s, s)                                              # rmsa.py:115
        pe = O._conv_dw64(img, a["w"].astype(np.float64), a["b"].astype(np.float64), two_d)
        assert np.abs(ref["pe"] - pe.reshape(R, dim, P).transpose(0, 2, 1).reshape(R * P, dim)).max() <= 1e-12
        for c in (0, 1, dim // 2 + 1, dim - 1):
            assert np.array_equal(img[:, c].reshape(R * P), a["qkv"][:, 2 * dim + M.vp_src_col(c, heads, hd)].astype(np.float64))


# ------------------------------------------------------------------ D. the encoder cases
def test_encoder_cases_hold_pads_and_the_train_cases_exist():
    import test_hip_parity as T
    assert len(M.ENC_CASES) == 20 and set(M.ENC_VARIANTS) == {"epeg_2d", "value_bf_1d", "value_bf_2d", "value_af_1d", "value_af_2d"}
    for variant, N, rs, dim, heads in M.ENC_CASES:
        H, s, add = O.grid(N, 8, rs, 0, 0.0)
        real = (O.partition_index(H, s) < N).reshape(-1, s * s)
        assert s == rs and any(r.any() and not r.all() for r in real), (N, rs)
        cfg = M.enc_cfg(variant, N, rs, dim, heads)
        assert cfg["n_layers"] == 2 and cfg["cr_msa"] is False
    assert {(d, h) for _, _, _, d, h in M.ENC_CASES} == {(128, 4), (512, 8)}
    assert M.POS_CASES["peg_k11"]["peg_k"] == 11 and M.POS_CASES["ppeg_k9_1d"] == dict(pos="ppeg", pos_pos=-1, peg_k=9, peg_1d=True)
    cfgs = [c for _, c in T.TRAIN_CASES.values()]
    assert any(c.get("epeg_type") == "value_af" and not c.get("epeg_2d") for c in cfgs)
    assert any(c.get("epeg_type") == "value_bf" and c.get("epeg_2d") for c in cfgs)
    assert any(c.get("pos") == "peg" and c.get("peg_k") == 11 for c in cfgs)
    assert any(c.get("pos") == "ppeg" and c.get("peg_k") == 9 and c.get("peg_1d") for c in cfgs)


# ------------------------------------------------------------------ the refusals, without a device
def test_stage_entry_points_refuse_before_the_first_launch(lib):
    w3 = (C.c_void_p * 3)(PTR, PTR, PTR)
    n = C.c_size_t()
    peg = lambda k, dim=64, N=50: lib.rrt_peg_f32(PTR, w3, None, PTR, N, dim, k, 0, 0, None)
    pegb = lambda k, dim=64, ws=1 << 30: lib.rrt_peg_backward_f32(PTR, PTR, w3, PTR, w3, None, 50, dim, k, 0, 1, PTR, ws, None)
    for k in (0, 2, 4, 13, 15):
        assert peg(k) == pegb(k) == lib.rrt_peg_backward_workspace_size(50, 64, k, 0, C.byref(n)) == E_UNSUPPORTED, k
        assert b"peg_k" in lib.rrt_strerror(E_UNSUPPORTED)
    assert peg(3, dim=66) == pegb(3, dim=66) == E_UNSUPPORTED
    assert peg(3, N=0) == E_INVALID and lib.rrt_peg_f32(None, w3, None, PTR, 50, 64, 3, 0, 0, None) == E_INVALID
    assert lib.rrt_peg_f32(PTR, (C.c_void_p * 3)(PTR, None, None), None, PTR, 50, 64, 3, 0, 1, None) == E_INVALID      # PPEG: three convs
    assert lib.rrt_peg_backward_workspace_size(50, 64, 11, 1, C.byref(n)) == 0
    assert pegb(11, ws=n.value - 1) == E_WORKSPACE

    sm = lambda P=16, dim=128, heads=2, k=3, sb=0, sp=None: lib.rrt_attn_scoremap_f32(PTR, PTR, PTR, 2, P, dim, heads, k, sp, sb, None)
    smb = lambda P=16, dim=128, heads=2, k=3, sb=1 << 30: lib.rrt_attn_scoremap_backward_f32(PTR, PTR, PTR, PTR, PTR, 2, P, dim, heads, k,
                                                                                             PTR, sb, None)
    vp = lambda P=9, s=3, dim=128, heads=2, k=3: lib.rrt_value_pe_f32(PTR, PTR, None, PTR, 2, P, s, dim, heads, k, 1, None)
    vpb = lambda P=9, s=3, dim=128, heads=2, k=3: lib.rrt_value_pe_backward_f32(PTR, PTR, None, PTR, PTR, PTR, None, 2, P, s, dim, heads, k,
                                                                                1, None)
    for f in (sm, smb, vp, vpb):
        for k in (0, 2, 64, 65):
            assert f(k=k) == E_UNSUPPORTED, (f, k)
        assert f(dim=126) == E_UNSUPPORTED and f(dim=128, heads=3) == E_UNSUPPORTED
    assert b"n_heads" in lib.rrt_strerror(E_UNSUPPORTED)
    for k in (2, 65):
        assert lib.rrt_attn_scoremap_scratch_size(2, 16, 2, k, 0, C.byref(n)) == E_UNSUPPORTED
    for f in (vp, vpb):
        assert f(P=10, s=3) == E_UNSUPPORTED and f(P=9, s=0) == E_INVALID
    # scratch too small: the forward needs none until the map leaves the LDS
    assert lib.rrt_attn_scoremap_scratch_size(2, 225, 2, 3, 0, C.byref(n)) == 0 and n.value == 2 * 2 * 225 * 225 * 4
    assert sm(P=225, sb=n.value - 1, sp=PTR) == E_WORKSPACE and sm(P=225, sb=n.value, sp=None) == E_WORKSPACE
    assert lib.rrt_attn_scoremap_scratch_size(2, 16, 2, 3, 1, C.byref(n)) == 0 and n.value == 2 * 2 * 9 * 4
    assert smb(sb=n.value - 1) == E_WORKSPACE
    assert lib.rrt_attn_scoremap_backward_f32(PTR, PTR, PTR, PTR, None, 2, 16, 128, 2, 3, PTR, 1 << 30, None) == E_INVALID
