"""CPU: the case list of tests/test_linear_form_matrix.py covers what that module claims.  The instantiations csrc/linear_f32.hip
compiles (read back out of its dispatch macros) are all reached by a case, according to rrt_linear_plan -- the function the
launchers dispatch from -- except an explicit list that a sweep of the plan over the documented shapes never selects; every
deferred form has its K depths, every kernel its ragged-N and scalar-tail case, every form its epilogues; the integer family
is distinct where it has to be; the fp32 evaluation of every synth case sits inside its tolerance; and the forms the
documented configurations run are among the reached ones.  Nothing is launched: the library is loaded and rrt_linear_plan is
the only entry called."""
import itertools
import os
import re

import numpy as np
import pytest

import test_linear_form_matrix as M
from rrt_mil_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
PRECS = ("f32", "bf16", "f16")


def _source():
    with open(os.path.join(CSRC, "linear_f32.hip")) as fh:
        text = fh.read()
    return re.sub(r"#ifdef RRT_TUNING.*?#endif", "", text, flags=re.S)       # shapes only a tuning build can select


def compiled():
    """(kernel, MT, NT, mode, precision, defer) of every instantiation a product build can launch.  launch_cfg sends tiles of
    96 rows and more to the warp-specialised kernel (both DEFER values) and the others to linear_kernel; the switch that sends
    the large tiles to linear_kernel too (RRT_LINEAR_NO_WS) is read in tuning builds only, so those are not counted."""
    src = _source()
    assert 'rrt_tune_env("RRT_LINEAR_NO_WS")' in src and "if constexpr (MT >= 6)" in src
    tiles = [(int(a), int(b)) for a, b in re.findall(r"^  RRT_CASE\((\d), (\d)\);", src, flags=re.M)]
    tiles16 = [(int(a), int(b)) for a, b in re.findall(r"^  RRT_CASE16\((\d), (\d)\);", src, flags=re.M)]
    tiles_x3 = [(int(a), int(b)) for a, b in re.findall(r"^  RRT_SPLIT_CASE\((\d), (\d)\);", src, flags=re.M)]
    assert len(tiles) == 7 and len(tiles16) == 8 and len(tiles_x3) == 4
    out = set()
    for mt, nt in tiles:
        forms = [("ws", 0), ("ws", 1)] if mt >= 6 else [("plain", 0)]
        for kern, d in forms:
            for mode, prec in itertools.product(("plain", "act", "unpart"), PRECS):
                out.add((kern, mt, nt, mode, prec, d))
            out.add((kern, mt, nt, "drop", "f32", d))
            out.add((kern, mt, nt, "unpart+drop", "f32", d))
    for mt, nt in tiles16:
        for mode, prec, d in itertools.product(("plain", "act", "unpart"), PRECS[1:], (0, 1)):
            out.add(("ws16", mt, nt, mode, prec, d))
    for mt, nt in tiles_x3:
        assert mt >= 6
        for mode, d in itertools.product(("plain", "unpart"), (0, 1)):
            out.add(("ws", mt, nt, mode, "x3", d))
    assert "constexpr int KG = 4;" in src
    chunks = src.split("constexpr int MT = ")[1:]
    splitk = set()
    for ch in chunks:
        for drop in re.findall(r"auto kern = linear_splitk_kernel<MT, KG(, true)?>;", ch.split("RRT_CASE")[0]):
            splitk.add(("splitk", int(ch[0]), 4, "drop" if drop else "plain", "f32", 0))
    assert len(splitk) == 3
    return out | splitk


# ---- what no shape selects.  Tile shapes per operand kind and precision class ("low": bf16 / fp16), every epilogue of each;
# justified by test_unreached_forms_stay_unreached, which sweeps the plan and fails if one of them turns up (or if the
# sweep finds a form that no case reaches).  These instantiations are compiled and never launched by a product build.
UNREACHED_TILES = {
    # fp32 operands, exact: choose()'s candidates {9,2,512}, {8,2,512}, {8,2,256} never win, {9,2,256} wins for 16-bit MFMAs only;
    # 96-row tiles run in one round only (N == 512, 640 .. 768 tiles)
    ("ws", "f32"): {(9, 2, 0), (9, 2, 1), (8, 2, 0), (8, 2, 1), (6, 1, 1)},
    # fp32 operands rounded behind LDS: the 96-row rule takes every product of 512 tiles and more, so the other shapes never
    # get a second tile per block; {8,2} never wins, {9,2} is the single-round K >= 1024 rule
    ("ws", "low"): {(9, 1, 1), (8, 1, 1), (9, 2, 1), (8, 2, 0), (8, 2, 1)},
    # 16-bit images: small tiles are skipped above 1024 rows, so they run in one round; 144-row and 128-column tiles in one round
    # except the 128 x 128 tiles of several bags in flight
    ("ws16", "low"): {(2, 1, 1), (4, 1, 1), (9, 1, 1), (9, 2, 1), (6, 2, 1)},
    # split images: the 128-column candidates never win
    ("ws", "x3"): {(9, 2, 0), (9, 2, 1), (8, 2, 0), (8, 2, 1)},
}


def unreached():
    out = set()
    for (kern, pc), tiles in UNREACHED_TILES.items():
        precs = {"f32": ("f32",), "low": ("bf16", "f16"), "x3": ("x3",)}[pc]
        modes = ("plain", "unpart") if pc == "x3" else ("plain", "act", "unpart") + (("drop", "unpart+drop") if pc == "f32" else ())
        for (mt, nt, d), mode, prec in itertools.product(tiles, modes, precs):
            out.add((kern, mt, nt, mode, prec, d))
    return out


def _reached():
    return {M.instantiation(c.ops, M.plan_of(c)) for c in M.CASES}


def test_every_reachable_instantiation_is_reached():
    comp, un, got = compiled(), unreached(), _reached()
    assert un <= comp, sorted(un - comp)
    assert got == comp - un, (sorted(got - (comp - un)), sorted((comp - un) - got))


def test_unreached_forms_stay_unreached():
    """rrt_linear_plan over M = 1 .. 40000 (step 61 and the case list's own M), the usual N and K, both solo values, every
    operand kind and precision, with and without the dropout / zero64 bits that steer the split-K predicate: the tile
    forms it returns are exactly those the cases reach -- none of UNREACHED_TILES, and none the matrix misses."""
    lib = _lib.load()
    import ctypes as C
    buf = (C.c_int32 * _lib.LINEAR_PLAN_INTS)()
    seen = set()
    Ms = sorted(set(range(1, 40001, 61)) | {c.M for c in M.CASES} | {40000})
    kinds = [("f32", 0, 0), ("f32", 0, 1), ("f32", 0, 2), ("16", 1, 1), ("16", 1, 2), ("x3", 2, 3)]
    for (ops, oc, comp), N, K, solo in itertools.product(kinds, (64, 130, 192, 256, 384, 512, 768, 1024, 1536, 2048),
                                                         (32, 64, 128, 256, 512, 1024, 2048), (0, 1)):
        if ops == "16" and K % 64:
            continue
        epis = (0, 4) if (comp == 0 and solo) else (0,)
        for m, epi in itertools.product(Ms, epis):
            assert lib.rrt_linear_plan(m, N, K, comp, oc, epi, solo, 0, buf) == 0
            kern = "splitk" if buf[0] == 2 else "plain" if buf[0] == 0 else "ws16" if ops == "16" else "ws"
            pc = "x3" if ops == "x3" else "f32" if buf[10] == 0 else "low"
            seen.add((kern, pc, buf[1], buf[2] if kern != "splitk" else buf[7], buf[6], buf[8]))
    want = set()
    for c in M.CASES:
        p = M.plan_of(c)
        if EPI_IS_BASE(c):
            kern = M.instantiation(c.ops, p)[0]
            pc = "x3" if c.ops == "x3" else "f32" if p["prec"] == 0 else "low"
            want.add((kern, pc, p["mt"], p["nt"] if kern != "splitk" else p["kg"], p["defer"], p["drop"]))
    assert seen == want, (sorted(seen - want), sorted(want - seen))
    for (kern, pc), tiles in UNREACHED_TILES.items():
        for mt, nt, d in tiles:
            assert (kern, pc, mt, nt, d, 0) not in seen


def EPI_IS_BASE(c):
    """the epilogues the sweep asks for (plain, dropout): the others change the mode of the instantiation, not its tile"""
    return c.epi in ("bias+q", "nobias", "drop") and not c.zero64


def test_axes_of_every_form():
    ids = [M.case_id(c) for c in M.CASES]
    assert len(set(ids)) == len(ids)
    by_row = {}
    for c in M.CASES:
        p = M.plan_of(c)
        assert M.form_of(c.ops, p) == c.form, (M.case_id(c), M.form_of(c.ops, p))
        kern, mt, nt, mode, prec, d = M.instantiation(c.ops, p)
        by_row.setdefault((kern, mt, nt, p["cap"], prec if "drop" not in c.epi else PRECS[c.compute], d,
                           p["ntiles"] > p["grid"]), []).append((c, p))
        if c.H:                                   # pad slots and a ragged last row tile
            g = M.grid_of(c)
            assert g.H == c.H and g.H * g.H == c.M and g.L < c.M and c.M % (16 * p["mt"]) != 0 and c.rn > 1, M.case_id(c)
    for (kern, mt, nt, cap, prec, d, rounds), cs in by_row.items():
        epis = {c.epi for c, _ in cs}
        if kern == "splitk":
            continue
        want = {"bias+q", "nobias", "unpart", "unpart+q"} | (set() if prec == "x3" else {"relu"})
        if prec == "f32":
            want |= {"drop", "unpart+drop"}
        assert want <= epis, (kern, mt, nt, cap, prec, d, want - epis)
        # un-partition in both forms where the tile's width allows the straight-line one (N = 130 rows take the per-row one)
        assert any(not M.straight_unpart(c, nt) for c, _ in cs if c.epi.startswith("unpart"))
    # the straight-line un-partition store and the buffer-store deferred form, per kernel and operand kind
    for kern, prec in (("plain", "f32"), ("ws", "f32"), ("ws", "bf16"), ("ws16", "bf16"), ("ws16", "f16"), ("ws", "x3")):
        for d in ((0,) if kern == "plain" else (0, 1)):
            assert any(M.straight_unpart(c, p["nt"]) for c in M.CASES for p in [M.plan_of(c)]
                       if M.instantiation(c.ops, p)[::5] == (kern, d) and M.instantiation(c.ops, p)[4] == prec), (kern, prec, d)
    # all four activations on the plain kernel, the warp-specialised kernel (once and deferred) and the 16-bit one
    for kern in ("plain", "ws", "ws16"):
        assert {"relu", "gelu", "tanh", "sigmoid"} <= {c.epi for c in M.CASES if M.instantiation(c.ops, M.plan_of(c))[0] == kern}
    # ragged N (not a multiple of 64) and a scalar store tail (not a multiple of 4) per kernel; M off the 16-row grid
    for kern in ("plain", "ws", "ws16", "splitk"):
        ns = {c.N for c in M.CASES if M.instantiation(c.ops, M.plan_of(c))[0] == kern}
        assert any(n % 4 for n in ns) and any(n % 64 for n in ns), kern
    assert any(c.N % 4 for c in M.CASES if c.ops == "x3")
    assert any(c.M % 16 for c in M.CASES if c.ops == "16") and any(c.M % 16 for c in M.CASES if c.ops == "x3")
    # zero64 on one plain-kernel and one warp-specialised case
    assert {M.instantiation(c.ops, M.plan_of(c))[0] for c in M.CASES if c.zero64} >= {"plain", "ws"}


def test_every_deferred_form_has_its_k_depths():
    """nk = K / 32 in {1, 2, 3, MT - 1, MT, MT + 1, 16} (16-bit images: K / 64 in {1, 2, 3, 8}) for every deferred tile form
    whose rule does not pin K, with the plain epilogue (the flush loop behind the K loop) and the straight-line un-partition
    (the buffer-store form: its kt <= MT branch, its odd-nk copy).  Pinned by N == K == 512: ws16<8,2>."""
    depth = {}
    for c in M.CASES:
        p = M.plan_of(c)
        kern, mt, nt, mode, prec, d = M.instantiation(c.ops, p)
        if d and (c.epi == "bias+q" or M.straight_unpart(c, nt)):
            depth.setdefault((kern, mt, nt, prec, mode), set()).add(c.K // (64 if c.ops == "16" else 32))
    forms = {k[:4] for k in depth}
    assert forms == {("ws", 8, 1, "f32"), ("ws", 9, 1, "f32"), ("ws", 6, 1, "bf16"), ("ws", 6, 1, "f16"), ("ws16", 6, 1, "bf16"),
                     ("ws16", 6, 1, "f16"), ("ws16", 8, 1, "bf16"), ("ws16", 8, 1, "f16"), ("ws16", 8, 2, "bf16"),
                     ("ws16", 8, 2, "f16"), ("ws", 8, 1, "x3"), ("ws", 9, 1, "x3")}
    for (kern, mt, nt, prec), mode in itertools.product(forms, ("plain", "unpart")):
        if (kern, mt, nt) == ("ws16", 8, 2):
            assert depth[(kern, mt, nt, prec, mode)] == {8}
            continue
        assert set(M.k_depths("16" if kern == "ws16" else "f32", mt)) <= depth[(kern, mt, nt, prec, mode)], (kern, mt, nt, prec, mode)


def test_integer_family_is_a_structural_witness():
    """no two rows of A or of B within 144 rows of each other coincide, no two 32-wide K tiles of a row coincide, |C| < 2^24"""
    shapes = {(c.M, c.K, 251) for c in M.CASES} | {(c.N, c.K, 241) for c in M.CASES}
    # (the value depends on the element index row * K + k alone: a matrix of fewer rows is the head of the tallest of its K)
    shapes = {(max(r for r, k, p in shapes if (k, p) == (K, prime)), K, prime) for _, K, prime in shapes}
    for rows, K, prime in sorted(shapes):
        a = M._ints((rows, K), prime)
        assert a.min() == -3 and a.max() == 3 or rows * K < 64
        h = (a.astype(np.int64) + 3) @ (np.int64(7) ** (np.arange(K) % 22)) + ((a.astype(np.int64) + 3) * (np.arange(K) + 1)).sum(1) * 1000003
        order = np.argsort(h, kind="stable")
        same = np.nonzero(h[order][1:] == h[order][:-1])[0]
        for i in same:                                  # equal hashes: equal rows only if 144 rows or more apart
            r0, r1 = order[i], order[i + 1]
            assert abs(int(r1) - int(r0)) >= 144 or not np.array_equal(a[r0], a[r1]), (rows, K, prime, r0, r1)
        if K > 32:
            t = np.ascontiguousarray(a.reshape(rows, K // 32, 32) + 4, dtype=np.uint8)      # 1 .. 7: a tile is 32 non-zero bytes
            key = np.sort(t.view("S32").reshape(rows, K // 32), axis=1)                     # equal strings <=> equal tiles
            assert (key[:, 1:] != key[:, :-1]).all(), (rows, K, prime, np.argwhere(key[:, 1:] == key[:, :-1])[:3].tolist())
    assert max(9 * c.K + 6 for c in M.CASES) * 2 < 2 ** 24


ROWS_FOR_NUMPY = sorted({(c.ops, c.compute, c.M, c.N, c.K) for c in M.CASES})


@pytest.mark.parametrize("ops,compute,m,n,k", ROWS_FOR_NUMPY)
def test_fp32_evaluation_sits_inside_every_tolerance(ops, compute, m, n, k):
    """what keeps the tolerance honest: numpy's fp32 matmul of the same operands + the fp32 epilogue lies within each synth
    case's tolerance of float64; no tolerance of an exact-fp32 case exceeds the per-stage 2e-5 at |C| = O(1)"""
    for c in [c for c in M.CASES if (c.ops, c.compute, c.M, c.N, c.K) == (ops, compute, m, n, k)]:
        r = M.reference(c, "synth", M.plan_of(c)["mt"])
        err = float(np.abs(M.reference32(c, "synth").astype(np.float64) - r["ref"]).max())
        assert np.isfinite(err) and err <= r["tol"], (M.case_id(c), err, r["tol"], r["chain"])
        if c.compute == 0:
            assert r["tol"] <= 2e-5 * max(1.0, float(np.abs(r["ref"]).max())), (M.case_id(c), r["tol"])


# ---- what users run: the GEMMs of the documented configurations -> the form rrt_linear_plan reports for them.
# (configuration, operand kind, compute, M, N, K, epilogue, solo); Np = H^2 of the default region grid (region_num 8; 16 at
# N = 30000); the representatives' GEMMs have M = 64 k rows.
def _np(n, rn):
    g = _lib.region_grid(n, rn)
    return g.H * g.H


def product_callers():
    out = []
    for D in (256, 384, 512, 1024):
        for n, rn in ((9000, 8), (30000, 16)):
            for solo in (1, 0):
                out.append((f"qkv D={D} N={n} solo={solo} fp32", "f32", 0, _np(n, rn), 3 * D, D, "bias+q", solo))
                out.append((f"proj D={D} N={n} solo={solo} fp32", "f32", 0, _np(n, rn), D, D, "unpart", solo))
                out.append((f"proj D={D} N={n} solo={solo} bf16", "16", 1, _np(n, rn), D, D, "unpart", solo))
                out.append((f"proj D={D} N={n} solo={solo} f32x3", "x3", 3, _np(n, rn), D, D, "unpart", solo))
                out.append((f"patch_to_emb 1024->{D} N={n} solo={solo} fp32", "f32", 0, n, D, 1024, "relu", solo))
                out.append((f"patch_to_emb 1024->{D} N={n} solo={solo} bf16", "f32", 1, n, D, 1024, "relu", solo))
        for k in (3, 8):
            for solo in (1, 0):
                out.append((f"representatives qkv D={D} k={k} solo={solo}", "f32", 0, 64 * k, 3 * D, D, "bias+q", solo))
                out.append((f"representatives proj D={D} k={k} solo={solo}", "f32", 0, 64 * k, D, D, "nobias", solo))
            out.append((f"representatives proj D={D} k={k} training", "f32", 0, 64 * k, D, D, "drop", 1))
    return out


PRODUCT_CALLERS = product_callers()


def test_product_callers_run_reached_forms():
    got = _reached()
    missing = []
    for name, ops, compute, m, n, k, epi, solo in PRODUCT_CALLERS:
        c = M.Case(ops, compute, m, n, k, epi, solo, 0, 0, 0, "")
        inst = M.instantiation(ops, M.plan_of(c))
        if inst not in got:
            missing.append((name, inst))
    assert not missing, missing
