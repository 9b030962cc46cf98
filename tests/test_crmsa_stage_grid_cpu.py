"""CPU: the case lists of tests/test_crmsa_stage_matrix.py cover what that module claims -- every instantiation of the three
dispatch switches at the end of csrc/crmsa.hip and every GK of crmsa_region_kernel, the peaked logits inside 40 .. 60 with
the region maximum in every block's share of the rows, pads that really bound a representative, row records that reproduce
the float64 logits -- and the fp32 eager evaluation sits inside every bound.  Nothing is launched."""
import os
import re

import numpy as np
import pytest

import test_crmsa_stage_matrix as M
from rrt_mil_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
SHAPES = sorted({(D, L) for D, L, _, _, _ in M.FRONT_CASES})


def _source():
    with open(os.path.join(CSRC, "crmsa.hip")) as fh:
        text = fh.read()
    return re.sub(r"#ifdef RRT_TUNING.*?#endif", "", text, flags=re.S)       # shapes only a tuning build can select


def _reached():
    return {M.instantiation(f, D, k, M.region_P(L)) for D, L, k, _, _ in M.FRONT_CASES for f in M.case_forms(D, k, M.region_P(L))}


def test_table_of_the_issue():
    assert [(L, M.region_P(L)) for L, _ in M.FRONT_SHAPES] == M.FRONT_SHAPES
    assert [P for _, P in M.FRONT_SHAPES] == [1, 9, 25, 49, 144, 169, 289, 576]
    for L in (2305, 9217, 16385):                          # one token more than the grid below holds
        assert M.region_P(L - 1) < M.region_P(L), L
    b = M.base(9217, 512)
    assert b.add == 1599 and not b.real[56:].any() and M.mixed_regions(9217) == list(range(48, 56))
    assert M.base(36864, 512).add == 0
    for P in (144, 169):
        assert M.front_ks(P) == tuple(range(1, 9))
    assert M.front_ks(289) == M.front_ks(576) == (3, 8)
    assert {(D, L) for D, L in M.SMALL_DIM_SHAPES} == {(d, l) for d in (64, 192) for l in (300, 1100)}
    for D, L in M.SMALL_DIM_SHAPES:
        assert M.case_forms(D, 3, M.region_P(L)) == ["two", "parts"]


def test_every_instantiation_of_the_dispatch_switches_is_reached():
    src, got = _source(), _reached()
    s4 = re.findall(r"RRT_S4\((\d+), (\d+), (\d+)\)", src)
    assert len(s4) == 8 and {f"stream4<{a},{b},{c}>" for a, b, c in s4} == {i for i in got if i.startswith("stream4")}
    cb, lg = re.findall(r"RRT_CB512\((\d)\)", src), re.findall(r"RRT_LG512\((\d)\)", src)
    assert sorted(cb) == sorted(lg) == list("12345678")
    assert {f"logits512<{k}>+combine512<{k}>" for k in cb} == {i for i in got if i.startswith("logits512")}
    gk = re.findall(r"launch_region_gk<(\d)>\(", src)
    assert sorted(set(gk)) == list("0123") and {f"region<GK={g}>" for g in gk} == {i for i in got if i.startswith("region<")}
    # region4: RRT_R4(NB, NW, NR) stands for KM = 3 and KM = 8; RRT_R4G(K) for <4, 12, 3, K, GPR>; one explicit five-representative
    # form.  <8, 4, 5, 3> is chosen by an environment variable of the tuning builds only.
    want = {f"region4<{a},{b},{c},{km}>" for a, b, c in re.findall(r"RRT_R4\((\d+), (\d+), (\d+)\);", src) for km in (3, 8)}
    want |= {f"region4<4,12,3,{k},GPR>" for k in re.findall(r"RRT_R4G\((\d)\);", src)}
    explicit = set(re.findall(r"launch_region4_cfg<(\d+), (\d+), (\d+), (\d+)>\(", src)) - {("8", "4", "5", "3")}
    want |= {"region4<%s,%s,%s,%s>" % e for e in explicit}
    assert len(want) == 10 and want == {i for i in got if i.startswith("region4")}
    assert {"combine_parts<KM=4>", "combine_parts<KM=4,COAL>", "combine_parts<KM=8>", "logits+combine(generic)"} <= got


def test_unaligned_phi_only_where_the_launcher_allows_it():
    for D, L, k, _, _ in M.FRONT_CASES:
        P, forms = M.region_P(L), M.case_forms(D, k, M.region_P(L))
        assert ("four_u" in forms) == (D == 512 and k in (4, 5) and 4 <= P <= 144)
        assert ("one_u" in forms) == ("one" in forms)
    assert M.instantiation("four_u", 512, 5, 144) == "region4<4,12,3,8>"          # the non-GPR fallback


def test_no_case_is_left_out():
    ids = [M.front_id(*c) for c in M.FRONT_CASES]
    assert len(set(ids)) == len(ids)
    for L, P in M.FRONT_SHAPES:
        for k in M.front_ks(P):
            fams = {(sc, pad) for D, l, kk, sc, pad in M.FRONT_CASES if (D, l, kk) == (512, L, k)}
            assert fams == set(M.FAMILIES if M.mixed_regions(L) else M.FAMILIES[:2]), (L, k)
    assert [L for L, _ in M.FRONT_SHAPES if not M.mixed_regions(L)] == [50, 36864]


@pytest.mark.parametrize("D,L", SHAPES)
def test_families_hold_what_they_promise(D, L):
    """per case of the shape: make_case's own float64 assertions (window, arg-max slots, one-signed logits, pads), the
    arg-max in every block of every form's split, the row records against the float64 logits, fp32 eager inside the bounds"""
    b = M.base(L, D)
    for case in [c for c in M.FRONT_CASES if c[:2] == (D, L)]:
        _, _, k, scale, pad = case
        c = M.make_case(*case)
        forms = M.case_forms(D, k, b.P)
        if scale == "peaked":
            assert M.PEAK_WINDOW[0] <= c["maxlg"] <= M.PEAK_WINDOW[1]
        else:
            assert c["maxlg"] < 12.0 * (2.5 if pad else 1.0)
        if scale == "peaked" and not pad:
            slots = [p for _, p in c["peaks"]]
            assert 0 in slots and len({r for r, _ in c["peaks"]}) == len(c["peaks"])
            r_last, p_last = c["peaks"][-1]
            assert p_last == np.nonzero(b.real[r_last])[0].max() and (not M.mixed_regions(L) or r_last in M.mixed_regions(L))
            for f in forms:
                blocks = {M.share(f, b.P, k, p)[0] for p in slots}
                assert blocks == {M.share(f, b.P, k, p)[0] for p in range(b.P)}, (case, f)
                if b.P >= 16:
                    assert len({M.share(f, b.P, k, p)[1] for p in slots}) >= 3, (case, f)
        if "parts" in forms:
            # rstd sum_slab (d - mean sum_slab gamma phi) + beta . phi from the rounded records; their rounding: NS values of
            # relative 2^-24 each in d and in mean, times rstd
            part = M.parts_records(b, c).astype(np.float64)
            NS = D // 64
            m, q, d = part[..., 0], part[..., 1], part[..., 2:2 + k]
            mean = m.mean(-1, keepdims=True)
            rstd = 1 / np.sqrt((q.sum(-1, keepdims=True) + 64 * ((m - mean) ** 2).sum(-1, keepdims=True)) / D + 1e-5)
            gphi = (c["gm"].astype(np.float64)[:, None] * c["phi"].astype(np.float64)).reshape(NS, 64, k)
            lg = rstd * (d - mean[..., None] * gphi.sum(1)).sum(1) + c["bt"].astype(np.float64) @ c["phi"].astype(np.float64)
            want = M.logits64(b, c["rowsrc"], c["gm"], c["bt"], c["phi"])
            got = np.concatenate([lg, np.zeros((b.add, k))], 0)[b.perm].reshape(b.R, b.P, k).transpose(0, 2, 1)
            tol = 4 * NS * 2.0 ** -24 * float(rstd.max()) * float(np.abs(d).max() + np.abs(mean).max() * np.abs(gphi.sum(1)).max())
            assert np.abs(got - want).max() <= max(tol, 1e-12), (case, np.abs(got - want).max(), tol)
        # what the bounds rest on: the error of the fp32 eager evaluation itself, held to caps a quarter above the worst figure
        # measured over all cases (mild: logits 5.2e-6, representatives 1.6e-5, weights 8.5e-7, and 9.1e-6, 3.4e-5, 1.3e-6 with pad-bound logits; max |Lg| = 50, pad-bound
        # families included: 3.6e-5, 5.8e-5, 4.9e-6; y 1.7e-5, mean / rstd 1.0e-7) -- no bound of the GPU module can exceed
        # 8 x these.  At P8 = 144 / 169 for k = 1, 3, 5, 8 (the evaluation does not depend on the kernel instantiation).
        if b.P in (144, 169) and k not in (1, 3, 5, 8):
            continue
        e = {w: v[0] for w, v in M.bounds(c, M.restate(b, c, np.float64), M.restate(b, c, np.float32)).items()}
        cap = (dict(lg=1.15e-5, rep=4.3e-5, wd=1.7e-6) if pad else dict(lg=6.5e-6, rep=2.0e-5, wd=1.1e-6)) if scale == "mild" else dict(lg=4.5e-5, rep=7.2e-5, wd=6.1e-6)
        cap.update(y=2.1e-5, mr=1.3e-7)
        assert all(np.isfinite(e[w]) and e[w] <= cap[w] for w in cap), (case, e)

def test_backward_cases_are_the_table_of_the_issue():
    assert M.BWD_SHAPES == [(50, 3), (300, 1), (1100, 8), (2305, 5), (9217, 3)]
    assert [M.region_P(N) for N, _ in M.BWD_SHAPES] == [1, 9, 25, 49, 169]
    for N, k in M.BWD_SHAPES:
        got = [v for n, kk, mlp, v in M.BWD_CASES if (n, kk, mlp) == (N, k, False)]
        assert got == list(M.BWD_VARIANTS if M.mixed_regions(N) else M.BWD_VARIANTS[:2]), N
    assert [c for c in M.BWD_CASES if c[2]] == [(1100, 3, True, "synth"), (1100, 3, True, "peaked")]
    assert len(set(M.BWD_CASES)) == len(M.BWD_CASES)


@pytest.mark.parametrize("N,k,mlp,variant", [c for c in M.BWD_CASES if c[0] <= 1100 and c[3] != "synth"])
def test_backward_states_hold_what_they_promise(N, k, mlp, variant):
    """the window of the peaked logits and the sign of the pad-bound representative, on the states the GPU module builds"""
    cfg, st, x, G, n = M.bwd_state(N, k, mlp, variant)
    lg, real, tok = M.bwd_logits64(x, st, cfg)
    if "peaked" in variant:
        assert M.PEAK_WINDOW[0] <= np.abs(lg).max() <= M.PEAK_WINDOW[1]
    assert (lg.transpose(0, 2, 1)[~real] == 0).all()
    if n is not None:
        sign = 1 if variant.endswith("min") else -1
        assert (sign * lg[:, n][real] > 0).all()
        for r in M.mixed_regions(N):
            assert (lg[r, n].min() if sign > 0 else lg[r, n].max()) == 0.0


@pytest.mark.parametrize("N,k,mlp,variant", [c for c in M.BWD_CASES if c[0] <= 2305 and "pads" in c[3]])
def test_backward_criteria_pass_and_fail_where_they_should(N, k, mlp, variant):
    """check_backward on the CPU.  The cut-graph float64 run agrees with O.forward_eager outside the arg-min / arg-max rows and
    at least one region's normaliser term is visible (both asserted inside); gradients a rounding away from the reference
    pass; the same dx with the normaliser's term sent to the real row it would wrongly land on fails."""
    import torch
    from oracle import rrt_oracle as O
    from rrt_mil_amd import synth
    cfg, st, x, G, n = M.bwd_state(N, k, mlp, variant)
    lg, real, tok = M.bwd_logits64(x, st, cfg)
    y64, xl, params = O.forward_eager(x, st, cfg, grad=True)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    cut = (n,) + M.normaliser_terms64(x, st, cfg, G, n, 1 if variant.endswith("min") else -1)
    dx_ref = xl.grad.numpy()
    grads_ref = {m: v.grad.numpy() for m, v in params.items() if v.grad is not None}
    # a stand-in for the kernels: the reference rounded to fp32 plus noise of 1e-5 of each tensor's largest entry
    noisy = lambda a, tag: (a + 1e-5 * np.abs(a).max() * synth.uniform(tag, a.shape, -1, 1, np.float64)).astype(np.float32)
    dx = noisy(dx_ref, "crm/bwd/noise/dx")
    grads = {m: noisy(v, "crm/bwd/noise/" + m) for m, v in grads_ref.items()}
    before = len(M.RECORDS)
    assert M.check_backward("cpu", dx, grads, dx_ref, grads_ref, lg, real, tok, cut) == []
    bad = dx.copy()
    for r, (t, row) in cut[2].items():
        bad[t] += row.astype(np.float32)
    fails = M.check_backward("cpu", bad, grads, dx_ref, grads_ref, lg, real, tok, cut)
    assert any("normaliser" in m for m in fails), fails
    del M.RECORDS[before:]
