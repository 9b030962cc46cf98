"""CPU: MHIM-MIL's float64 restatement (tests/mhim_ref.py) against the reference's own run (tests/golden/mhim.npz,
tools/make_golden_mhim.py) -- masks and counts exact, values to 1e-10 (float64 against float64: summation order only; far
inside the goldens' recorded fp32 error e32) -- the state_dict surface, the scheduler, the new exports and every argument
refusal of the four entries, none of which launches anything.  No GPU compute, on a machine with a GPU too."""
import ctypes as C

import numpy as np
import pytest
import torch

import mhim_cases as MC
import mhim_ref as R
from conftest import load_golden
from rrt_mil_amd import MHIM, MHIM_MIL, PURE_MHIM, _lib, mhim
from rrt_mil_amd.build import build

F64_TOL = 1e-10
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x10000       # a non-null, 16-byte aligned address nothing dereferences: every call below is refused before a launch


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


@pytest.fixture(scope="module")
def G():
    return load_golden("mhim")


def perms_of(G, cid):
    return [G[f"{cid}/perm{j}"] for j in range(G["cfg"]["cases"][cid]["n_perms"])]


def states(cid):
    return MC.state(MC.shapes_of(), "student"), MC.state(MC.shapes_of(), "teacher")


def test_golden_covers_what_the_cases_claim(G):
    cases = G["cfg"]["cases"]
    assert set(cases) == set(MC.CASES)
    assert {c["n"] for c in cases.values()} == {37, 300}
    assert {c["select_inv"] for c in cases.values()} == {False, True}
    assert {c["mask_ratio_hr"] for c in cases.values()} == {0., 0.5}
    assert any(c["mask_ratio"] == 0 and c["mask_ratio_l"] == 0 and c["mask_ratio_h"] > 0 for c in cases.values())
    for cid, c in cases.items():
        a = G[f"{cid}/attn32"]
        assert a.dtype == np.float32 and a.shape == (c["n"],) and not np.isnan(a).any() and np.unique(a).size == a.size, cid
        st, te = states(cid)
        sums = [float(sum(np.asarray(v, np.float64).sum() for v in s.values())) for s in (st, te)]
        assert np.allclose(sums, c["state_sum"], rtol=0, atol=1e-9) and abs(float(MC.bag(cid).astype(np.float64).sum()) - c["bag_sum"]) < 1e-9
        assert [k for k, _ in c["keys"]] == list(R.KEYS)


@pytest.mark.parametrize("cid", list(MC.CASES))
def test_restatement_masks_are_the_references(G, cid):
    c = G["cfg"]["cases"][cid]
    ratios = {k: c[k] for k in MC.RATIO_KEYS}
    len_keep, ids = R.get_mask(c["n"], G[f"{cid}/attn32"], perms_of(G, cid), select_inv=c["select_inv"], **ratios)
    assert len_keep == c["len_keep"]
    assert np.array_equal(ids[:len_keep], G[f"{cid}/kept"])
    assert np.array_equal(np.sort(ids), np.arange(c["n"])) and np.all(np.diff(ids[len_keep:]) > 0)
    # the stages that draw a permutation are the ones the reference drew one for, of the same length
    drew = [k for _, k, m in R.stage_plan(c["n"], **ratios) if m is not None]
    assert drew == [p.size for p in perms_of(G, cid)]


@pytest.mark.parametrize("cid", list(MC.CASES))
def test_restatement_values_are_the_references(G, cid):
    c = MC.CASES[cid]
    act, da = c.get("act", "relu"), c.get("da_act", "relu")
    st, te = states(cid)
    x = MC.bag(cid)
    tea, attn = R.teacher(x, te, act, da)
    out = R.student(x, st, G[f"{cid}/kept"], teacher_feat=tea, act=act, da_act=da)
    logits, tattn, raw = R.forward_test(x, st, act, da)
    for q, got in (("tea_feat", tea), ("tea_attn", attn), ("logits", out["logits"]), ("cls_loss", out["cls_loss"].reshape(1)),
                   ("test_logits", logits), ("test_attn", tattn), ("test_raw", raw)):
        err = R.rel_err(got, G[f"{cid}/{q}"])
        print(f"{cid} {q}: err {err:.2e} (golden e32 {float(G[f'{cid}/e32_{q}']):.2e})")
        assert tuple(got.shape) == G[f"{cid}/{q}"].shape and err <= F64_TOL, (cid, q, err)
    # the fp32 scores the reference selected on order the bag as the float64 ones do not have to; they ARE the recorded row
    _, attn32 = R.teacher(x, te, act, da, dtype=torch.float32)
    assert R.rel_err(attn32, G[f"{cid}/attn32"][None]) <= max(2e-5, 8 * float(G[f"{cid}/e32_tea_attn"]))


def test_selection_order_rule():
    a = np.array([0.0, -0.0, np.nan, 1.0, -np.inf, np.inf, 1.0, -np.nan, 0.0], dtype=np.float32)
    assert R.order(a, False).tolist() == [4, 0, 1, 8, 3, 6, 5, 2, 7]
    assert R.order(a, True).tolist() == [2, 7, 5, 3, 6, 0, 1, 8, 4]
    ids, count, mask = R.select(a, [(True, 3, None), (False, 2, np.array([0, 1], np.uint8))], False)
    assert count == 5 and ids.tolist() == [1, 3, 4, 6, 8, 0, 2, 5, 7] and mask.tolist() == [1, 0, 1, 0, 0, 1, 0, 1, 0]
    ids, count, _ = R.select(a, [(True, 3, None)], True)
    assert count == 3 and ids.tolist() == [2, 5, 7, 0, 1, 3, 4, 6, 8]


def test_state_dict_surface(G):
    keys = G["cfg"]["keys"]
    surface = lambda m: [[k, list(v.shape)] for k, v in m.state_dict().items()]   # noqa: E731
    assert surface(MHIM_MIL(**MC.MAIN_PARAMS)) == keys["MHIM_MIL"]
    assert surface(PURE_MHIM()) == keys["PURE_MHIM"]
    assert surface(MHIM(baseline="attn")) == keys["MHIM"]
    assert surface(MHIM(baseline="attn", act="gelu", dropout=0.)) == keys["MHIM_gelu_nodrop"]
    assert surface(MHIM(baseline="attn", act="none", da_act="none")) == keys["MHIM_noact"]
    # strict both ways: a state dict with exactly the reference's keys loads, and ours has no key beyond them
    m = MHIM_MIL(**MC.MAIN_PARAMS)
    sd = {k: torch.zeros(s) for k, s in keys["MHIM_MIL"]}
    m.load_state_dict(sd, strict=True)
    assert list(m.state_dict()) == [k for k, _ in keys["MHIM_MIL"]]
    for cid in MC.CASES:
        s = MHIM(**MC.model_kwargs(cid))
        s.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in MC.state(MC.shapes_of(), "student").items()}, strict=True)


def test_cosine_scheduler_is_the_references(G):
    for j, s in enumerate(MC.SCHEDULES):
        got = mhim.cosine_scheduler(s[0], s[1], epochs=s[2], niter_per_ep=s[3], warmup_epochs=s[4], start_warmup_value=s[5])
        assert got.dtype == np.float64 and np.array_equal(got, G[f"schedule{j}"]), j
    m = MHIM_MIL(**MC.MAIN_PARAMS)
    assert len(m.mm_sche) == len(m.student.mrh_sche) == 200 * 100 and m.student.mrh_sche[0] == 0.02 and m.mm_sche[0] == 0.9999
    assert MHIM_MIL(**dict(MC.MAIN_PARAMS, mm_sche=False)).mm_sche is None


def test_exports_and_abi(lib):
    for name in ("rrt_mask_select_workspace_size", "rrt_mask_select_f32", "rrt_gather_rows_f32", "rrt_scatter_rows_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rrt_abi_version() == _lib.ABI_VERSION == 29
    assert C.sizeof(_lib.MaskStage) == 24


def size(lib, n, stages=1):
    need = C.c_size_t()
    rc = lib.rrt_mask_select_workspace_size(n, stages, C.byref(need))
    return rc, need.value


def test_mask_select_refusals_launch_nothing(lib):
    st = (_lib.MaskStage * 3)()
    for s in st:
        s.largest, s.k, s.pick = 0, 5, None
    big = 1 << 24
    ok = dict(a=P, n=10, stages=st, n_stages=3, invert=0, ids=P, count=P, mask=None, ws=P, bytes=big)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.rrt_mask_select_f32(v["a"], v["n"], v["stages"], v["n_stages"], v["invert"], v["ids"], v["count"], v["mask"],
                                       v["ws"], v["bytes"], None)
    for kw in (dict(a=None), dict(stages=None), dict(ids=None), dict(count=None), dict(ws=None), dict(n=0), dict(n=-3),
               dict(n_stages=0), dict(n_stages=4), dict(n=4)):      # (n = 4: k = 5 > n)
        assert call(**kw) == INVALID, kw
    st[1].k = 0
    assert call() == INVALID
    st[1].k = 11
    assert call() == INVALID
    st[1].k = 10
    assert call(n=_lib.MASK_SELECT_MAX_N + 1) == UNSUPPORTED and b"262144" in lib.rrt_strerror(UNSUPPORTED)
    rc, need = size(lib, 10, 3)
    assert rc == 0 and call(bytes=need - 1) == WORKSPACE and call(bytes=0) == WORKSPACE
    with pytest.raises(NotImplementedError):
        _lib.check(call(n=_lib.MASK_SELECT_MAX_N + 1), "rrt_mask_select_f32")
    assert lib.rrt_mask_select_workspace_size(10, 1, None) == INVALID
    for n, s, want in ((0, 1, INVALID), (10, 0, INVALID), (10, 4, INVALID), (_lib.MASK_SELECT_MAX_N + 1, 1, UNSUPPORTED),
                       (_lib.MASK_SELECT_MAX_N, 3, 0), (1, 1, 0)):
        assert size(lib, n, s)[0] == want, (n, s)


@pytest.mark.parametrize("entry", ["rrt_gather_rows_f32", "rrt_scatter_rows_f32"])
def test_row_entries_refusals_launch_nothing(lib, entry):
    fn = getattr(lib, entry)
    ok = dict(src=P, ids=P, dst=P + 4096, n_rows=3, n_other=5, dim=8)

    def call(**kw):
        v = dict(ok, **kw)
        return fn(v["src"], v["ids"], v["dst"], v["n_rows"], v["n_other"], v["dim"], None)
    for kw in (dict(src=None), dict(ids=None), dict(dst=None), dict(n_rows=0), dict(n_other=0), dict(dim=0), dict(dim=-4),
               dict(src=P + 4), dict(dst=P + 8)):
        assert call(**kw) == INVALID, kw
    for dim in (1, 2, 3, 6, 1023):
        assert call(dim=dim) == UNSUPPORTED and b"multiple of 4" in lib.rrt_strerror(UNSUPPORTED)
    assert call(n_rows=1 << 38, dim=1024) == UNSUPPORTED


def test_workspace_size_never_shrinks(lib):
    ns = sorted(set(list(range(1, 600)) + list(range(1, _lib.MASK_SELECT_MAX_N + 1, 257)) + [_lib.MASK_SELECT_MAX_N]
                    + [256 * b + d for b in (1, 4, 64, 65, 128, 341, 342, 512, 1023) for d in (-1, 0, 1)]))
    last = 0
    for n in ns:
        rc, need = size(lib, n, 3)
        assert rc == 0 and need >= last and need >= n, n
        assert size(lib, n, 1)[1] == need                      # the stages live in the arguments, not in the workspace
        last = need
    assert last <= 4 << 20


def test_constructor_refusals():
    with pytest.raises(NotImplementedError, match="selfattn"):
        MHIM()                                                  # the reference's default baseline
    with pytest.raises(NotImplementedError, match="selfattn"):
        MHIM_MIL(**dict(MC.MAIN_PARAMS, baseline="selfattn"))
    with pytest.raises(NotImplementedError, match="selfattn"):
        PURE_MHIM(baseline="selfattn")
    with pytest.raises(NotImplementedError, match="mlp_dim"):
        MHIM(baseline="attn", mlp_dim=256)
    with pytest.raises(NotImplementedError, match="mlp_dim"):
        MHIM_MIL(**dict(MC.MAIN_PARAMS, mlp_dim=384))


def test_cpu_tensors_and_bad_attn_raise():
    m = MHIM(baseline="attn", input_dim=64, mask_ratio=0.5, mask_ratio_h=0.1)
    x = torch.zeros(1, 10, 64)
    for call in (lambda: m(x, attn=torch.zeros(1, 10)), lambda: m.forward_test(x), lambda: m.forward_teacher(x),
                 lambda: m.eval().pure(x), lambda: m.get_mask(10, None, torch.zeros(1, 10)),
                 lambda: mhim.mask_select(torch.zeros(10), [(False, 3, None)]),
                 lambda: mhim.gather_rows(torch.zeros(10, 8), torch.arange(10), 3)):
        with pytest.raises(_lib.RRTHipError, match="MI355X only"):
            call()
    with pytest.raises(NotImplementedError, match="selfattn"):
        m.get_mask(10, None, torch.zeros(1, 2, 10))
    with pytest.raises(ValueError, match="attn is None"):
        m.get_mask(10, None, None)                               # the high stage is on and has nothing to rank
    assert MHIM(baseline="attn", input_dim=64, mask_ratio=0.5).get_mask(10, None, None) == (10, None)
    assert MHIM(baseline="attn", input_dim=64).get_mask(10, None, torch.zeros(1, 10)) == (10, None)
    with pytest.raises(ValueError, match="scores"):
        m.get_mask(10, None, torch.zeros(1, 9))
    with pytest.raises(NotImplementedError, match="one stage"):
        m.select_mask_fn(10, torch.zeros(1, 10), False, 0.5, mask_ids_other=torch.zeros(1, 10))


def test_stage_sizes_are_the_restatements():
    for ps in (1, 2, 37, 300, 9000, 30011):
        for ratio in (0.02, 0.2, 0.5, 0.7, 1.0, np.float64(0.0137)):
            for rr in (0.001, 0., 0.5, 1., 0.9999):
                assert mhim._stage_sizes(ps, ratio, rr) == R.stage_sizes(ps, ratio, rr)
    assert R.stage_plan(300, 0.7, 0.2, 0.02, 0.) == [(False, 300, 210), (False, 60, None), (True, 300, 6)]
    assert R.stage_plan(300, 0.5, 0.2, 0.1, 0.5) == [(False, 300, 150), (False, 60, None), (True, 60, 30)]
