"""CPU: the case lists of tests/rmsa_fused_cases.py cover what tests/test_rmsa_fused_peaked.py claims -- every row-tile
count of every fused R-MSA dispatch ladder (read back out of the source text) with the row maximum planted in each key tile
in turn, a dominant last key next to masked ones on every ladder, both wave forms and every step count of the pair kernel's
stencil -- the planted inputs are as peaked as claimed (on the float64 restatement alone), and the restatement is the
oracle's arithmetic.  Nothing is launched."""
import os
import re

import numpy as np
import pytest
import torch

import rmsa_fused_cases as F
from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth
from test_hip_parity import _attn_ref

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
IDS = [F.case_id(c) for c in F.CASES]


def _ladder(fname, macro):
    """[(largest P, MT)] of a dispatch ladder `if (P > a) { MACRO(m) } ... MACRO(last)`, read out of the source text"""
    with open(os.path.join(CSRC, fname)) as fh:
        text = fh.read()
    rungs = [(int(a), int(m)) for a, m in re.findall(r"if \(P > (\d+)\) \{ " + macro + r"\((\d+)\) \}", text)]
    last = [int(m) for m in re.findall(r"^\s*" + macro + r"\((\d+)\)\s*$", text, re.M)]
    assert len(last) == 1 and rungs == sorted(rungs, reverse=True), (fname, macro)
    mts = [last[0]] + [m for _, m in reversed(rungs)]
    return list(zip([a for a, _ in reversed(rungs)], mts)), mts[-1]


def _pred_range(fname, func):
    """(P >, P <=) of a *_supported predicate"""
    with open(os.path.join(CSRC, fname)) as fh:
        body = fh.read().split("bool " + func + "(")[1].split("\n}")[0]
    lo, hi = re.search(r"P > (\d+) && P <= (\d+)", body).groups()
    return int(lo), int(hi)


SOURCES = {"fused_f32": ("rmsa_fused.hip", "RRT_FUSED", "rmsa_fused_supported"),
           "fused16": ("rmsa_fused16.hip", "RRT_FUSED16", "rmsa_fused16_supported"),
           "pair16": ("rmsa_pair16.hip", "RRT_PAIR16", "rmsa_pair16_supported"),
           "x3": ("rmsa_fused_x3.hip", "RRT_X3", "rmsa_fused_x3_supported")}


@pytest.mark.parametrize("kernel", sorted(SOURCES))
def test_ladders_match_the_source(kernel):
    fname, macro, pred = SOURCES[kernel]
    rungs, top_mt = _ladder(fname, macro)
    lo, hi = _pred_range(fname, pred)
    assert rungs + [(hi, top_mt)] == F.LADDERS[kernel] and lo + 1 == F.P_MIN[kernel]
    for P in range(lo + 1, hi + 1):
        assert 16 * F.mt_of(kernel, P) >= P > 0
    with open(os.path.join(CSRC, "rmsa_fused.hip")) as fh:
        text = fh.read()
    assert "SPLIT_LAST = MT == 9" in text and "P > 64 && n_items >= 2 * lag" in text
    assert F.split_last("fused_f32", 129) and F.split_last("fused_proj", 144) and not F.split_last("fused_f32", 128)
    assert not F.split_last("fused16", 144)


def test_stencil_geometry_and_pair_choice_match_the_source():
    with open(os.path.join(CSRC, "rmsa_pair16.hip")) as fh:
        text = fh.read()
    for line in ("g.H8 = (half + 7) & ~7;", "g.nstep = (16 + 2 * g.H8 + 31) / 32;", "const int qw = BM - 16 + 32 * g.nstep;",
                 "g.pitch = qw * 2;", "n_regions >= 8", "MT_ >= 6 && MT_ <= 9", "PAIR16_NH2_DEFAULT = true",
                 "return g.pitch <= VT_PITCH && g.nstep <= 3;"):
        assert line in text, line
    assert [F.stencil_geo(144, ek)[1] for ek in (0, 15, 21, 63)] == [1, 1, 2, 3]
    assert F.stencil_geo(176, 63) == (32, 3, 512) and F.takes_pair(9, 176, 63) and not F.takes_pair(9, 177, 15)
    assert not F.takes_pair(7, 144, 15) and not F.takes_pair(9, 16, 15)
    assert [F.pair_waves(P) for P in (32, 64, 96, 112, 128, 144, 176)] == [8, 8, 16, 16, 16, 16, 8]


def _of(kernel, variant=None, compute=None):
    return [c for c in F.CASES if c.kernel == kernel and variant in (None, c.variant) and compute in (None, c.compute)]


@pytest.mark.parametrize("kernel", sorted(F.LADDERS))
def test_every_form_has_a_case(kernel):
    mts = [m for _, m in F.LADDERS[kernel]]
    runmax = _of(kernel, "runmax")
    if kernel == "fused_proj":                           # two bags: the nine-tile form and one other
        assert {F.mt_of(kernel, c.P) for c in runmax} == {9, 6} and all(c.R * c.heads >= 512 for c in runmax)
        assert {c.L for c in runmax} == {9000, 5000}
        return
    assert sorted({F.mt_of(kernel, c.P) for c in runmax}) == mts
    assert _of(kernel, "masked") and all(c.P % 16 == 1 for c in _of(kernel, "masked"))
    assert any(c.variant == "plain" and c.D == 512 and c.heads == 8 for c in _of(kernel))
    assert {0, 63} <= {c.ek for c in _of(kernel)} and {c.ek for c in _of(kernel)} <= set(F.EKS)
    for c in runmax:                                     # one region per key tile, the planted key inside its tile
        tiles = [t for _, _, t in F.planted(c)]
        assert set(tiles) == set(range(F.mt_used(c.P))) and all(16 * t <= j < min(c.P, 16 * t + 16) for _, j, t in F.planted(c))
    if kernel == "fused_f32":
        exact = _of(kernel, compute=0)
        full = {c.P for c in exact if c.variant == "runmax" and c.P % 16 == 0}
        ragged = {c.P for c in exact if c.variant == "runmax" and c.P % 16}
        assert {F.mt_of(kernel, P) for P in full} == {F.mt_of(kernel, P) for P in ragged} == set(mts)
        assert {c.P for c in exact if c.variant == "masked"} == {49, 65, 97, 113, 129, 145, 177}
        assert {F.mt_of(kernel, c.P) for c in exact if c.variant == "masked"} == set(mts)
        for v in ("plain", "ties_k", "ties_q"):
            assert {c.P for c in exact if c.variant == v and c.D == 128} == {144, 137}
        assert any(c.P == 49 and c.ek == 63 for c in exact)           # a stencil wider than the region
        assert any(c.variant == "runmax" and c.P == 144 for c in exact) and any(c.variant == "masked" and c.P == 129 for c in exact)
        for compute in (1, 2):
            assert {(c.variant, c.P) for c in _of(kernel, compute=compute)} == {(v, P) for v in ("plain", "runmax") for P in (144, 81)}
    if kernel == "fused16":
        assert {c.P for c in _of(kernel, "masked")} == {17, 33, 129, 209, 241}
        assert {c.P for c in _of(kernel, compute=2)} == {144, 256}
        # the library takes the one-region kernel: P > 176, or the call is cut into pieces of at most 7 regions
        assert all(not F.takes_pair(min(c.R, 7) if c.P <= 176 else c.R, c.P, c.ek) for c in _of(kernel))
    if kernel == "pair16":
        mine = _of(kernel)
        assert all(F.takes_pair(c.R, c.P, c.ek) for c in mine)
        assert all(c.R % 2 == 1 and c.R == (max(F.mt_used(c.P), 8) + 1) | 1 for c in mine if c.variant == "runmax")
        assert {F.pair_waves(c.P) for c in runmax} == {8, 16}
        steps = {F.stencil_geo(16 * F.mt_of(kernel, c.P), c.ek)[1] if c.ek else 0 for c in runmax}
        assert steps == {0, 1, 2, 3}
        assert {c.P for c in _of(kernel, "masked")} == {65, 129, 145} and any(c.compute == 2 and c.P == 144 for c in mine)
    if kernel == "x3":
        assert any(c.variant == "masked" and c.P == 129 for c in _of(kernel)) and any(c.variant == "plain" and c.P == 137 for c in _of(kernel))


def test_no_case_is_left_out_or_excused():
    """neither new test module names pytest's marks for a case that is passed over or expected to fail (the two words are put
    together from halves here, so that this file passes its own check); no case is listed twice"""
    import test_rmsa_fused_peaked as G                  # importing it needs no device
    words = ("sk" + "ip", "xf" + "ail")
    for mod in (F.__file__, G.__file__, __file__):
        with open(mod) as fh:
            text = fh.read().lower()
        assert not any(w in text for w in words), mod
    assert len(set(F.CASES)) == len(F.CASES) and len(set(IDS)) == len(IDS)
    assert all(c.variant in F.VARIANTS and c.D == c.heads * F.HD for c in F.CASES)


# ------------------------------------------------------------------ the inputs are as peaked as claimed
@pytest.mark.parametrize("c", F.CASES, ids=IDS)
def test_input_conditions(c):
    """on the float64 reference alone: the key-only channel, the peak window, the share of rows whose largest / smallest
    score lies in the planted key tile, and for nine row tiles the last row tile's rows per key tile"""
    i = F.inputs(c)
    R, P, D = c.R, c.P, c.D
    assert (i.u[:, 0] != 0).sum() == len(F.planted(c)) and not i.W[:D, 0].any() and not i.W[2 * D:, 0].any()
    assert i.u.shape[0] == (R + (c.variant == "masked")) * P
    st = F.storage(c)
    if st != "f32":                                      # representable, and no operand an fp16 subnormal
        assert np.array_equal(F._np16(i.u, st), i.u) and np.array_equal(F._np16(i.W, st), i.W)
    if c.variant != "ties_q":
        nz = np.abs(i.W[:, 1:])
        assert nz.min() >= 2.0 ** -14 and np.abs(i.u[:, 1:]).min() >= 2.0 ** -7
    o, S = F.reference(c, exact=True)
    smax = float(np.abs(S).max())
    top = np.exp(S - S.max(-1, keepdims=True))
    top = (1.0 / top.sum(-1)).reshape(-1)                # the largest probability of every row
    print(f"{F.case_id(c)}: largest |score| {smax:.2f}; rows with a top probability > 0.9: {100 * (top > 0.9).mean():.0f} %")
    if c.variant in ("plain", "runmax", "masked"):
        assert F.PEAK_WINDOW[0] <= smax <= F.PEAK_WINDOW[1], smax
    if c.variant in ("runmax", "masked"):
        tile = np.array([t for _, _, t in F.planted(c)])[:, None, None]
        hi = (S.argmax(-1) // 16 == tile)
        lo = (S.argmin(-1) // 16 == tile)
        print(f"    largest score in the planted tile: {100 * hi.mean():.0f} % of rows, smallest: {100 * lo.mean():.0f} %")
        assert hi.mean() >= 0.25 and lo.mean() >= 0.25
        jj = np.array([j for _, j, _ in F.planted(c)])[:, None, None]
        print(f"    ... the planted key itself: {100 * (S.argmax(-1) == jj).mean():.0f} % / {100 * (S.argmin(-1) == jj).mean():.0f} %")
    if c.variant == "runmax" and P == 144:               # nine row tiles, the last one full: its rows, per key tile in turn
        for r, _, t in F.planted(c):
            assert (S[r, :, 128:].argmax(-1) // 16 == t).sum() >= 4, (r, t)
    if c.variant == "ties_q":
        v = (i.u[:R * P].astype(np.float64) @ i.W[2 * D:].astype(np.float64).T + i.b[2 * D:]).reshape(R, P, D)
        assert np.abs(o.reshape(R, P, D) - v.mean(1, keepdims=True)).max() < 1e-12
    if c.variant == "ties_k":
        v = (i.u[:R * P].astype(np.float64) @ i.W[2 * D:].astype(np.float64).T + i.b[2 * D:]).reshape(R, P, D)
        assert np.abs(o.reshape(R, P, D) - v[:, :1]).max() < 1e-12


# ------------------------------------------------------------------ the restatement is the oracle's arithmetic
def _mild(c):
    """the inputs of test_rmsa_fused16 at the case's shape, representable in its storage format"""
    tag = f"rfp/mild/{c.kernel}/{c.compute}"
    u = synth.normal(tag + "/u", (c.R * c.P, c.D))
    W = (synth.uniform(tag + "/w", (3 * c.D, c.D), -1, 1) / np.sqrt(c.D) * 1.5).astype(np.float32)
    st = F.storage(c)
    if st != "f32":
        u, W = F._np16(u, st), F._np16(W, st)
    return F.Inputs(u, W, synth.uniform(tag + "/b", (3 * c.D,), -0.2, 0.2),
                    synth.uniform(tag + "/pe", (c.heads, max(c.ek, 1)), -0.3, 0.3))


def _oracle(c, i):
    R, P, D, heads, ek = c.R, c.P, c.D, c.heads, c.ek
    u = i.u[:R * P]
    mode = F.mode(c)
    if mode is None or mode[0] == "ops":
        if mode:
            u, W = O.round_lowp(u, mode[1]), O.round_lowp(i.W, mode[1])
        else:
            u, W = u.astype(np.float64), i.W.astype(np.float64)
        qkv = u @ W.T + i.b
        qkv[:, :D] *= (D // heads) ** -0.5
        return _attn_ref(qkv, i.taps, R, P, D, heads, ek)
    st = {"qkv.weight": i.W, "qkv.bias": i.b, "proj.weight": np.eye(D), "proj.bias": np.zeros(D)}
    if ek:
        st["pe.weight"] = i.taps.reshape(heads, 1, ek, 1)
    x = u.astype(np.float64).reshape(R, P, D)
    if mode[0] == "x3":
        taps = {}
        O._inner_attention64(x, st, "", heads, ek, taps, O.SplitX3(), None)
        return taps["proj_in"].reshape(R * P, D)

    class NoRound:                                      # u / W are exact already; O is compared before its rounding
        r = staticmethod(lambda a: a)
    return O._inner_attention64(x, st, "", heads, ek, None, NoRound, O.LowP(mode[1], True, stencil16=mode[0] == "pair16")
                                ).reshape(R * P, D)


PINNED = [F._c("fused_f32", "runmax", 144, 15), F._c("fused_f32", "masked", 49, 63), F._c("fused_f32", "runmax", 81, 21, compute=1),
          F._c("fused_f32", "runmax", 81, 21, compute=2), F._c("fused16", "runmax", 144, 21, compute=1),
          F._c("fused16", "runmax", 144, 15, compute=2), F._c("fused16", "masked", 33, 0, compute=1),
          F._c("pair16", "runmax", 144, 21, compute=1), F._c("pair16", "runmax", 144, 15, compute=2),
          F._c("pair16", "runmax", 112, 0, compute=1), F._c("x3", "runmax", 144, 15), F._c("x3", "runmax", 96, 0)]


@pytest.mark.parametrize("c", PINNED, ids=[F.case_id(c) for c in PINNED])
def test_restatement_is_the_oracles(c):
    """in float64, on one mild and one peaked input per rounding mode: within 1e-12 of the largest entry"""
    assert c in F.CASES
    for what, i in (("mild", _mild(c)), ("peaked", F.inputs(c))):
        mine, _ = F.restate(i.u, i.W, i.b, i.taps, c.R, c.P, c.D, c.heads, c.ek, torch.float64, F.mode(c))
        ref = _oracle(c, i)
        err = np.abs(mine.numpy() - ref).max() / np.abs(ref).max()
        print(f"{F.case_id(c)} {what}: {err:.2e}")
        assert err <= 1e-12, (what, err)
    assert {F.mode(p) for p in PINNED} == {F.mode(k) for k in F.CASES}


def test_flushed_probabilities_differ_only_in_fp16():
    c = F._c("fused16", "runmax", 144, 15, compute=2)
    kept, _ = F.reference(c)
    flushed, _ = F.reference(c, flush=True)
    assert np.abs(kept - flushed).max() > 0              # these inputs do put probabilities below 2^-14
    c = F._c("fused16", "runmax", 144, 15, compute=1)
    assert np.array_equal(F.reference(c)[0], F.reference(c, flush=True)[0])


def test_error_table_lists_every_form():
    import test_rmsa_fused_peaked as G
    recs = [G.Record("fused_f32 MT9", "runmax", "O", 1e-6, 2e-6, 5e-5, None, None),
            G.Record("fused_f32 MT9", "runmax", "O", 3e-6, 1e-6, 5e-5, None, None),
            G.Record("pair16 f16 MT9 w16", "runmax", "O", 1e-4, 2e-4, 1e-3, 3e-5, "kept")]
    lines = G.error_table(recs).splitlines()
    assert len(lines) == 3 and "3.00e-06" in lines[1] and " 2 " in lines[1] and "kept" in lines[2]
