"""CPU: the float64 restatement of MHIM-MIL with the TransMIL baseline (tests/mhim_sattn_ref.py) against the reference's own
run (tests/golden/mhim_sattn.npz, tools/make_golden_mhim_sattn.py) -- values to 1e-10 (float64 against float64: summation order
only; far inside the goldens' recorded fp32 error), the kept ids exact -- the stage property that stands in for the
reference's unspecified vote ties, the state_dict surface, and every refusal of the new module and of the two new exports, none
of which launches anything.  No GPU compute, on a machine with a GPU too."""
import ctypes as C

import numpy as np
import pytest
import torch

import mhim_ref as MR
import mhim_sattn_cases as SC
import mhim_sattn_ref as R
from conftest import load_golden
from rrt_mil_amd import _lib, mhim, mhim_sattn
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
    return load_golden("mhim_sattn")


def perms_of(G, cid):
    return [G[f"{cid}/perm{j}"] for j in range(G["cfg"]["cases"][cid]["n_perms"])]


def sel_rows(G, cid):
    layer = SC.CASES[cid].get("attn_layer", 0)
    return G[f"{cid}/rows32"][1 if layer == -1 else layer]


def test_golden_covers_what_the_cases_claim(G):
    cases = G["cfg"]["cases"]
    assert set(cases) == set(SC.CASES)
    assert {c["n"] for c in SC.CASES.values()} == {37, 255, 300, 511} and {c["head"] for c in SC.CASES.values()} == {2, 8}
    assert {c["select_inv"] for c in SC.CASES.values()} == {False, True}
    assert any(c.get("attn_layer") == -1 for c in SC.CASES.values()) and any(c.get("act") == "gelu" for c in SC.CASES.values())
    assert any(c["mask_ratio"] == 0 and c["mask_ratio_l"] == 0 and c["mask_ratio_h"] > 0 for c in SC.CASES.values())
    assert len([c for c in cases.values() if "grad" in c]) == len(SC.GRAD_CASES) == 2
    for cid, c in SC.CASES.items():
        rows = G[f"{cid}/rows32"]
        assert rows.dtype == np.float32 and rows.shape == (2, c["head"], c["n"]) and np.isfinite(rows).all(), cid
        assert all(np.unique(r).size == c["n"] for layer in rows for r in layer), cid
        for who in ("student", "teacher"):
            s = float(sum(np.asarray(v, np.float64).sum() for v in SC.state(c["head"], who).values()))
            assert abs(s - cases[cid][f"{who}_sum"]) < 1e-9, (cid, who)
        assert abs(float(SC.bag(cid).astype(np.float64).sum()) - cases[cid]["x_sum"]) < 1e-9


@pytest.mark.parametrize("cid", list(SC.CASES))
def test_restatement_masks_and_stage_property(G, cid):
    c, rec = SC.CASES[cid], G["cfg"]["cases"][cid]
    rows = sel_rows(G, cid)
    len_keep, ids = R.get_mask(c["n"], rows, perms_of(G, cid), select_inv=c["select_inv"], **SC.ratios(cid))
    assert len_keep == rec["len_keep"] and np.array_equal(ids, G[f"{cid}/ids"])
    assert np.array_equal(np.sort(ids), np.arange(c["n"]))
    assert np.all(np.diff(ids[:len_keep]) > 0) and np.all(np.diff(ids[len_keep:]) > 0)
    plan = MR.stage_plan(c["n"], **SC.ratios(cid))
    assert [k for _, k, m in plan if m is not None] == [p.size for p in perms_of(G, cid)]
    for (largest, k, _), ties in zip(plan, rec["ties"]):
        ok, got = R.threshold_property(rows, largest, k, R.fused_order(R.votes(rows, largest, k))[:k])
        assert ok and got == ties, (cid, largest, k)


def test_stage_property_over_n_and_heads(G):
    """what the golden tool held the reference's own select_mask_fn to, here for the restatement; the tie class at the threshold
    is what makes the two sets differ"""
    prop = G["cfg"]["property"]
    assert {(p["n"], p["head"]) for p in prop} == {(n, h) for n in SC.PROPERTY_NS for h in SC.PROPERTY_HEADS}
    for p in prop:
        rows = G[f"property/n{p['n']}_h{p['head']}"]
        chosen = R.fused_order(R.votes(rows, p["largest"], p["k"]))[:p["k"]]
        ok, ties = R.threshold_property(rows, p["largest"], p["k"], chosen)
        assert ok and ties == p["ties"], p
        assert p["same_set"] or ties > 1, p                     # the sets differ only where there is a tie to break
    assert not all(p["same_set"] for p in prop)


def test_vote_rule_by_hand():
    a = np.array([[5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5], [5, 0, 4, 1, 3, 2]], dtype=np.float32)
    assert R.votes(a, True, 2).tolist() == [2, 1, 1, 0, 1, 1]
    assert R.fused_order(R.votes(a, True, 2)).tolist() == [0, 1, 2, 4, 5, 3]
    ids, count, mask = R.select_vote(a, [(True, 2, None)], False)
    assert count == 4 and ids.tolist() == [2, 3, 4, 5, 0, 1] and mask.tolist() == [1, 1, 0, 0, 0, 0]
    ids, count, _ = R.select_vote(a, [(True, 2, np.array([0, 1], np.uint8)), (False, 1, None)], True)
    assert R.votes(a, False, 1).tolist() == [1, 1, 0, 0, 0, 1] and count == 2 and ids.tolist() == [0, 1, 2, 3, 4, 5]
    one = MR.select(a[0], [(False, 3, None)], False)
    assert all(np.array_equal(u, v) for u, v in zip(one, R.select_vote(a[:1], [(False, 3, None)], False)))


@pytest.mark.parametrize("cid", list(SC.CASES))
def test_restatement_values_are_the_references(G, cid):
    c, rec = SC.CASES[cid], G["cfg"]["cases"][cid]
    act, heads = c.get("act", "relu"), c["head"]
    st, te = SC.state(heads, "student"), SC.state(heads, "teacher")
    x = SC.bag(cid)
    feat, rows = R.teacher(x, te, heads, act, ref_row=True)
    logits, _ = R.forward_test(x, te, heads, act, ref_row=True)
    out = R.student(x, st, G[f"{cid}/ids"][:rec["len_keep"]], heads, teacher_feat=feat, act=act)
    got = [("teacher_feat", feat), ("teacher_a1", rows[0][0]), ("teacher_a2", rows[1][0]), ("teacher_test_logits", logits),
           ("student_logits", out["logits"]), ("student_cls_loss", out["cls_loss"].reshape(1))]
    if cid in SC.CLS_ROW_CASES:                                 # (N + 1) % 256 == 0: the reference's row IS the cls token's own
        _, own = R.teacher(x, te, heads, act, ref_row=False)
        got += [("teacher_a1", own[0][0]), ("teacher_a2", own[1][0])]
    for q, t in got:
        err = R.rel_err(t, G[f"{cid}/{q}"])
        print(f"{cid} {q}: err {err:.2e} (golden e32 {rec['e32_' + q]:.2e})")
        assert tuple(t.shape) == G[f"{cid}/{q}"].shape and err <= F64_TOL, (cid, q, err)
    # rows are about 1 / n: hold them to their own size too
    for j, q in enumerate(("teacher_a1", "teacher_a2")):
        ref = G[f"{cid}/{q}"]
        assert float(np.abs(rows[j][0].numpy() - ref).max()) <= 1e-9 * float(np.abs(ref).max()), (cid, q)
    # the fp32 restatement gives the recorded fp32 rows within the reference's own fp32 error rule
    _, rows32 = R.teacher(x, te, heads, act, dtype=torch.float32, ref_row=True)
    for j, q in enumerate(("teacher_a1", "teacher_a2")):
        assert R.rel_err(rows32[j][0], G[f"{cid}/rows32"][j]) <= max(2e-5, 8 * rec["e32_" + q])
    if cid not in SC.CLS_ROW_CASES:                             # elsewhere the reference's row is a pad row: another, flatter row
        _, own = R.teacher(x, te, heads, act, ref_row=False)
        assert float((own[0][0] - rows[0][0]).abs().max()) > 1e-6


@pytest.mark.parametrize("cid", SC.GRAD_CASES)
def test_restatement_gradients_are_the_references(G, cid):
    c, rec = SC.CASES[cid], G["cfg"]["cases"][cid]
    heads, act = c["head"], c.get("act", "relu")
    feat, _ = R.teacher(SC.bag(cid), SC.state(heads, "teacher"), heads, act, ref_row=True)
    out = R.student(SC.bag(cid), SC.state(heads, "student"), G[f"{cid}/ids"][:rec["len_keep"]], heads, teacher_feat=feat, act=act,
                    grad=True)
    (out["logits"].sum() + out["cls_loss"]).backward()
    grads = dict({k: p.grad for k, p in out["params"].items()}, x=out["x_leaf"].grad)
    assert set(grads) == set(rec["grad"]) and len(grads) == 26
    for k, g in grads.items():
        r = rec["grad"][k]
        assert abs(float(g.abs().max()) - r["peak"]) <= 1e-9 * r["peak"] and abs(float(g.norm()) - r["norm"]) <= 1e-9 * r["norm"], (cid, k)
        assert float(np.abs(g.reshape(-1)[:32].numpy() - G[f"{cid}/grad/{k}"]).max()) <= 1e-9 * r["peak"], (cid, k)


def test_state_dict_surface(G):
    keys = G["cfg"]["keys"]
    surface = lambda m: [[k, list(v.shape)] for k, v in m.state_dict().items()]   # noqa: E731
    S = mhim_sattn
    assert sorted(surface(S.MHIM(input_dim=SC.INPUT_DIM))) == sorted(keys["MHIM"]) and len(keys["MHIM"]) == 25
    assert sorted(surface(S.PURE_MHIM(input_dim=SC.INPUT_DIM, baseline="selfattn"))) == sorted(keys["PURE_MHIM"])
    mil = S.MHIM_MIL(num_epoch=2, niter_per_ep=3, input_dim=SC.INPUT_DIM, mask_ratio_h=0.02)
    assert sorted(surface(mil)) == sorted(keys["MHIM_MIL"])
    mil.load_state_dict({k: torch.zeros(s) for k, s in keys["MHIM_MIL"]}, strict=True)
    assert isinstance(mil.student, S.MHIM) and isinstance(mil.teacher, S.MHIM) and isinstance(mil.student.online_encoder, S.SAttention)
    for cid, c in SC.CASES.items():
        m = S.MHIM(**SC.model_kwargs(cid))
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in SC.state(c["head"], "student").items()}, strict=True)
    layer = S.TransLayer(dim=512, head=2)
    assert layer.attn.heads == 2 and layer.attn.dim_head == 64 and layer.attn.num_landmarks == 256 and layer.attn._train_enabled
    assert layer.attn.to_out[1].p == 0.1 and layer.attn.pinv_iterations == 6 and layer.attn.residual


def test_constructor_refusals():
    S = mhim_sattn
    with pytest.raises(NotImplementedError, match="selfattn"):
        mhim.MHIM()                                             # the sibling module keeps refusing the reference's default
    with pytest.raises(NotImplementedError, match=r"rrt_mil_amd\.mhim "):
        S.MHIM(baseline="attn")
    with pytest.raises(NotImplementedError, match=r"rrt_mil_amd\.mhim "):
        S.PURE_MHIM()                                           # the reference's default here is 'attn'
    with pytest.raises(NotImplementedError, match=r"rrt_mil_amd\.mhim "):
        S.MHIM_MIL(num_epoch=2, niter_per_ep=3, mask_ratio_h=0.02, baseline="attn")
    with pytest.raises(NotImplementedError, match="mlp_dim"):
        S.MHIM(mlp_dim=256)
    with pytest.raises(NotImplementedError, match="msa_fusion"):
        S.MHIM(msa_fusion="mean")
    for head in (0, 17):
        with pytest.raises(NotImplementedError, match="head"):
            S.MHIM(head=head)
    for kw in (dict(pos_pos=-1), dict(pos_pos=-2), dict(pos="none")):
        with pytest.raises(NotImplementedError, match="pos"):
            S.SAttention(**kw)
    for kw in (dict(conv_1d=True), dict(bias=False), dict(k=13), dict(k=4)):
        with pytest.raises(NotImplementedError):
            S.PPEG(**kw)
    assert S.MHIM().online_encoder.layer1.attn.heads == 2      # the reference's defaults build


def test_cpu_tensors_and_bad_arguments_raise():
    S = mhim_sattn
    m = S.MHIM(input_dim=64, mask_ratio=0.5, mask_ratio_h=0.1)
    x = torch.zeros(1, 10, 64)
    rows = torch.zeros(1, 2, 10)
    for call in (lambda: m(x, attn=[rows, rows]), lambda: m.forward_test(x), lambda: m.forward_teacher(x),
                 lambda: m.eval().pure(x), lambda: m.get_mask(10, None, rows), lambda: m.forward_bags([x]),
                 lambda: m.online_encoder(torch.zeros(1, 10, 512)), lambda: m.online_encoder.pos_embedding(torch.zeros(1, 10, 512)),
                 lambda: S.mask_select_vote(torch.zeros(2, 10), [(False, 3, None)])):
        with pytest.raises(_lib.RRTHipError, match="MI355X only"):
            call()
    with pytest.raises(ValueError, match=r"rrt_mil_amd\.mhim"):
        m.get_mask(10, None, torch.zeros(1, 10))                # a 2-D attn is the ABMIL baseline's
    with pytest.raises(ValueError, match="heads"):
        m.get_mask(10, None, torch.zeros(1, 3, 10))
    with pytest.raises(ValueError, match="attn is None"):
        m.get_mask(10, None, None)
    with pytest.raises(ValueError, match="no_norm"):
        m.forward_test(x, return_attn=True, no_norm=True)
    with pytest.raises(ValueError, match="attn_layer"):
        S.MHIM(attn_layer=2)
    with pytest.raises(ValueError, match=r"\(heads, n\)"):
        S.mask_select_vote(torch.zeros(10), [(False, 3, None)])
    assert S.MHIM(input_dim=64).get_mask(10, None, rows) == (10, None)


def test_exports_and_abi(lib):
    for name in ("rrt_mask_select_vote_workspace_size", "rrt_mask_select_vote_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rrt_abi_version() == _lib.ABI_VERSION == 29 and C.sizeof(_lib.MaskStage) == 24
    assert "mhim_sattn" in __import__("rrt_mil_amd").__all__ and __import__("rrt_mil_amd").MHIM is mhim.MHIM


def size(lib, n, heads, stages=1):
    need = C.c_size_t()
    rc = lib.rrt_mask_select_vote_workspace_size(n, heads, stages, C.byref(need))
    return rc, need.value


def test_mask_select_vote_refusals_launch_nothing(lib):
    st = (_lib.MaskStage * 3)()
    for s in st:
        s.largest, s.k, s.pick = 0, 5, None
    ok = dict(a=P, n=10, heads=2, stages=st, n_stages=3, invert=0, ids=P, count=P, mask=None, ws=P, bytes=1 << 30)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.rrt_mask_select_vote_f32(v["a"], v["n"], v["heads"], v["stages"], v["n_stages"], v["invert"], v["ids"], v["count"],
                                            v["mask"], v["ws"], v["bytes"], None)
    for kw in (dict(a=None), dict(stages=None), dict(ids=None), dict(count=None), dict(ws=None), dict(n=0), dict(n=-3),
               dict(n_stages=0), dict(n_stages=4), dict(n=4), dict(heads=0), dict(heads=-1)):      # (n = 4: k = 5 > n)
        assert call(**kw) == INVALID, kw
    st[1].k = 0
    assert call() == INVALID
    st[1].k = 11
    assert call() == INVALID
    st[1].k = 10
    assert call(n=_lib.MASK_SELECT_MAX_N + 1) == UNSUPPORTED and b"262144" in lib.rrt_strerror(UNSUPPORTED)
    assert call(heads=17) == UNSUPPORTED and b"heads" in lib.rrt_strerror(UNSUPPORTED)
    rc, need = size(lib, 10, 2, 3)
    assert rc == 0 and call(bytes=need - 1) == WORKSPACE and call(bytes=0) == WORKSPACE
    with pytest.raises(NotImplementedError):
        _lib.check(call(heads=17), "rrt_mask_select_vote_f32")
    assert lib.rrt_mask_select_vote_workspace_size(10, 2, 1, None) == INVALID
    for n, h, s, want in ((0, 2, 1, INVALID), (10, 0, 1, INVALID), (10, 2, 0, INVALID), (10, 2, 4, INVALID),
                          (_lib.MASK_SELECT_MAX_N + 1, 2, 1, UNSUPPORTED), (10, 17, 1, UNSUPPORTED),
                          (_lib.MASK_SELECT_MAX_N, 16, 3, 0), (1, 1, 1, 0)):
        assert size(lib, n, h, s)[0] == want, (n, h, s)


def test_workspace_size_never_shrinks(lib):
    ns = sorted(set(list(range(1, 300)) + list(range(1, _lib.MASK_SELECT_MAX_N + 1, 1021)) + [_lib.MASK_SELECT_MAX_N]
                    + [256 * b + d for b in (1, 4, 64, 65, 128, 341, 342, 512, 1023) for d in (-1, 0, 1)]))
    last_h = [0] * 17
    for n in ns:
        prev = 0
        for h in range(1, 17):
            rc, need = size(lib, n, h, 3)
            assert rc == 0 and need >= last_h[h] and need >= prev and need >= n, (n, h)
            assert size(lib, n, h, 1)[1] <= need
            last_h[h], prev = need, need
    assert last_h[16] <= 48 << 20
