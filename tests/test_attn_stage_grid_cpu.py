"""CPU: the case lists of tests/test_attn_stage_matrix.py cover what that module claims -- every head dim the two dispatch
switches instantiate, every chunk / run / query-group edge of each, every head-dim-64 branch -- and leave nothing out.
Also the host side of its encoder cases: rrt_encoder_plan reports the head-dim kernel for them and training accepts them.
Nothing is launched."""
import ctypes as C
import os
import re

import pytest

import test_attn_stage_matrix as M
from rrt_mil_amd import RRTEncoder, _lib
from rrt_mil_amd import build as build_mod

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")


def _switch_head_dims(fname, macro):
    """the arguments of every use of `macro(<number>)` in a dispatch switch, read out of the source text"""
    with open(os.path.join(CSRC, fname)) as fh:
        return sorted(int(m) for m in re.findall(macro + r"\((\d+)\)", fh.read()))


def _fwd_cases(hd):
    return [(P, ek) for h, P, ek in M.STAGE_CASES if h == hd]


def test_constants_match_the_issue_table():
    """FwdCfg / StreamCfg restated in the test module, against the table the grid was designed from"""
    table = {80: (6, 6), 112: (4, 4), 144: (3, 3), 160: (3, 3), 176: (2, 2), 208: (2, 2), 224: (2, 2), 240: (2, 2),
             16: (9, 8), 32: (9, 8), 48: (9, 8), 96: (5, 5), 128: (4, 4), 192: (2, 2), 256: (2, 2)}
    for hd, (cf, cb) in table.items():
        assert (M.fwd_cfg(hd)["CT"], M.bwd_cfg(hd)["CT"]) == (cf, cb), hd
        assert M.fwd_cfg(hd)["G"] == (128 if hd <= 128 else 64) and M.bwd_cfg(hd)["G"] == (64 if hd >= 192 else 96)
        lds = 2 * M.fwd_cfg(hd)["CK"] * (hd + 4) * 4
        assert lds <= 80 * 1024
    assert 2 * M.fwd_cfg(80)["CK"] * 84 * 4 == 64512 and 2 * M.fwd_cfg(240)["CK"] * 244 * 4 == 62464


def test_every_instantiated_head_dim_has_cases():
    fwd = _switch_head_dims("region_attn_hd.hip", "RRT_HD_CASE")
    bwd = _switch_head_dims("attn_bwd.hip", "RRT_STREAM_HD")
    assert len(fwd) == 15 and fwd == bwd == sorted(M.HDS)
    for cases in (M.STAGE_CASES, [(h, P, ek) for _, h, P, ek in M.PEAKED_CASES]):
        assert sorted({h for h, _, _ in cases} - {64}) == fwd
    for variant in ("plain", "runmax", "ties_k", "ties_q", "masked"):
        assert sorted({h for v, h, _, _ in M.PEAKED_CASES if v == variant}) == sorted(fwd + [64]), variant


@pytest.mark.parametrize("hd", M.HDS)
def test_stage_grid_reaches_every_edge(hd):
    f, b = M.fwd_cfg(hd), M.bwd_cfg(hd)
    ps = {P for P, _ in _fwd_cases(hd)}
    assert ps == set(M.stage_P_grid(hd)) and max(ps) == M.P_MAX
    need = {1, 15, 16, 17, M.P_MAX}
    for c in (f, b):
        need |= {c["CK"] - 1, c["CK"], c["CK"] + 1, c["CK"] + 17, c["CK"] + 33, 2 * c["CK"] + 1, c["G"] - 1, c["G"], c["G"] + 1}
    assert {p for p in need if p <= M.P_MAX} <= ps
    # every P runs without EPEG, with epeg_k 15 and with a third width; 63 where the stencil crosses both ends of the region
    for P in ps:
        eks = sorted(ek for p_, ek in _fwd_cases(hd) if p_ == P)
        assert len(eks) == 3 and {0, 15} < set(eks) and set(eks) - {0, 15} < set(M.EKS), (P, eks)
    assert all((P, 63) in _fwd_cases(hd) for P in (15, 17))
    # forward: a last chunk of every tile count 1 .. CT, alone and behind a full chunk
    last = {(P - 1) % f["CK"] // 16 + 1 for P in ps}
    assert last == set(range(1, f["CT"] + 1)), sorted(last)
    behind = {(P - 1) % f["CK"] // 16 + 1 for P in ps if P > f["CK"]}
    assert behind == set(range(1, f["CT"] + 1)), sorted(behind)
    # forward: a final run of one, two and three tiles (a chunk of CT = 2 tiles never holds a run of three)
    final = {M.fwd_runs(hd, P)[-1][1] for P in ps}
    assert final == set(range(1, min(3, f["CT"]) + 1)), final
    # one and more than one query group, forward (16 NWMAX queries) and backward (16 NW)
    for g in (f["G"], b["G"]):
        assert any(P <= g for P in ps) and any(g < P <= 2 * g for P in ps) and any(P > 2 * g for P in ps)
    # the backward's two kernel families
    fams = {M.bwd_family(hd, P, ek) for P, ek in _fwd_cases(hd)}
    assert fams == {"valu_generic", "stream_hd"}


@pytest.mark.parametrize("hd", M.HDS)
def test_peaked_cases_per_head_dim(hd):
    ck = M.fwd_cfg(hd)["CK"]
    mine = [(v, P, ek) for v, h, P, ek in M.PEAKED_CASES if h == hd]
    for v in ("plain", "runmax", "ties_k"):
        assert {P for v_, P, _ in mine if v_ == v} == {ck, ck + 1, M.P_MAX}, v
    assert {(P, ek) for v, P, ek in mine if v == "runmax"} == {(P, ek) for P in (ck, ck + 1, M.P_MAX) for ek in (0, 15)}
    assert {(P, ek) for v, P, ek in mine if v == "masked"} == {(P, ek) for P in (17, ck + 1) for ek in (0, 15)}
    assert all(("ties_k", P, 0) in mine for P in (ck, ck + 1, M.P_MAX))     # the bit-identical rows assertion
    # the running maximum arrives in every run: one region per run
    assert len(M.fwd_runs(hd, M.P_MAX)) >= 4


def test_head_dim_64_reaches_every_dispatch_branch():
    mine = [(v, P, ek) for v, h, P, ek in M.PEAKED_CASES if h == 64]
    fwd = {M.fwd_family(64, P, ek) for _, P, ek in mine}
    assert {"tile16", "tile32", "tile48_nw3", "tile48_nw4", "attn64", "resident15", "resident16"} <= fwd
    assert any(f.endswith("_gt256") for f in fwd)
    bwd = {M.bwd_family(64, P, ek) for _, P, ek in mine}
    assert bwd == {"resident64", "resident96", "resident112", "resident128", "resident144", "resident176", "resident208",
                   "stream64_lds_adjoint", "stream64_global_adjoint"}
    for v in ("plain", "runmax", "ties_k"):
        assert {P for v_, P, _ in mine if v_ == v} >= set(M.HD64_PS), v
    # both branches with and without EPEG where the branch allows it (attn64 is the no-EPEG branch at P = 64)
    for P in M.HD64_PS:
        assert {ek for v, p_, ek in mine if p_ == P and v == "plain"} == {0, 15}


def test_no_case_is_left_out_or_excused():
    """the grid may leave out nothing: neither new module names pytest's marks for a case that is passed over or expected
    to fail (the two words are put together from halves here, so that this file passes its own check), and no case is listed twice"""
    words = ("sk" + "ip", "xf" + "ail")
    for mod in (M.__file__, __file__):
        with open(mod) as fh:
            text = fh.read().lower()
        assert not any(w in text for w in words), mod
    assert len(set(M.STAGE_CASES)) == len(M.STAGE_CASES) and len(set(M.PEAKED_CASES)) == len(M.PEAKED_CASES)
    ids = [M.case_id(*c) for c in M.STAGE_CASES] + [M.case_id(h, P, k, v) for v, h, P, k in M.PEAKED_CASES]
    assert len(set(ids)) == len(ids)


def test_encoder_cases_plan_the_head_dim_kernel():
    """the encoder configurations of the GPU module: R-MSA head dims 80, 112, 160 and 240 -- rrt_encoder_plan reports the
    head-dim kernel, and the forward and training workspaces are accepted at every bag size used"""
    build_mod.build()
    lib = _lib.load()
    assert sorted(c["mlp_dim"] // c["n_heads"] for c in M.ENC_CFGS.values()) == [80, 112, 160, 240]
    fl, sz, sz2 = C.c_int32(-1), C.c_size_t(), C.c_size_t()
    for name, N in sorted(set(M.ENC_CASES + M.ENC_TRAIN_CASES)):
        enc = RRTEncoder(**M.ENC_CFGS[name])
        enc._desc.compute, enc._desc.solo = _lib.COMPUTE_F32, 1
        assert lib.rrt_encoder_plan(C.byref(enc._desc), N, C.byref(fl)) == 0 and fl.value == _lib.PLAN_ATTN_HD, (name, N)
        assert lib.rrt_encoder_workspace_size(C.byref(enc._desc), N, C.byref(sz)) == 0 and sz.value > 0, (name, N)
        assert lib.rrt_encoder_train_sizes(C.byref(enc._desc), N, C.byref(sz), C.byref(sz2)) == 0, (name, N)
    assert any(N > 3000 for _, N in M.ENC_CASES) and any(N > 3000 for _, N in M.ENC_TRAIN_CASES)
