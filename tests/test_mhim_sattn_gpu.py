"""GPU (-m gpu): MHIM-MIL with the TransMIL baseline (rrt_mil_amd.mhim_sattn) against the reference's goldens
(tests/golden/mhim_sattn.npz, tools/make_golden_mhim_sattn.py) and the float64 restatement tests/mhim_sattn_ref.py (pinned to the
goldens by tests/test_mhim_sattn_cpu.py) -- never against another kernel.

Masks and counts: exact.  Values, the rule of tests/test_mhim_gpu.py: err <= max(2e-5, 8 x the reference's own recorded
fp32-against-float64 error of that quantity), relative to max(1, max |float64|).  Gradients: within max(1e-3, 8 x the
reference's own recorded fp32 gradient error) of that gradient's largest entry.  The EMA: 1e-6 relative to the float64 formula.
The library's rows are the cls token's own (the restatement with ref_row=False); the golden's are the reference's, which are the
same rows where (N + 1) % 256 == 0.  Nothing more runs after a device error.  Importing this module needs no device.
RRT_MHIM_SATTN_ERRORS_OUT=<file>: the error table kept as profiles/mhim_sattn_errors.txt."""
import os

import numpy as np
import pytest
import torch

import mhim_ref as MR
import mhim_sattn_cases as SC
import mhim_sattn_ref as R
from conftest import load_golden
from rrt_mil_amd import _lib, mhim_sattn as S

pytestmark = pytest.mark.gpu
TOL, E32_FACTOR, GRAD_TOL, EMA_TOL = 2e-5, 8.0, 1e-3, 1e-6
RECORDS = []


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_MHIM_SATTN_ERRORS_OUT")       # the table kept as profiles/mhim_sattn_errors.txt
    if out and RECORDS:
        with open(out, "w") as fh:
            fh.write("# rrt_mil_amd.mhim_sattn on the MI355X against float64 (tests/test_mhim_sattn_gpu.py)\n"
                     "# values: |got - f64| / max(1, max |f64|); gradients: / the gradient's largest entry; e32 = the reference's own\n"
                     f"# {'case':<16} {'quantity':<52} {'err':>10} {'e32':>10} {'bound':>10}\n")
            for r in RECORDS:
                fh.write("  {:<16} {:<52} {:>10.3e} {:>10.2e} {:>10.2e}\n".format(*r))


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """a device error is sticky: nothing more is started on a device that reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is run on it: {e}", returncode=3)


@pytest.fixture(scope="module")
def G():
    return load_golden("mhim_sattn")


def judge(case, what, got, ref64, e32, fails):
    ref64 = (ref64.detach() if torch.is_tensor(ref64) else torch.from_numpy(np.asarray(ref64))).double()
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (case, what, got.shape, ref64.shape)
    err = R.rel_err(got, ref64) if bool(torch.isfinite(got).all()) else float("inf")
    bound = max(TOL, E32_FACTOR * float(e32))
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
    RECORDS.append((case, what, err, float(e32), bound))
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


def judge_grad(case, what, got, ref64, e32, fails):
    ref64 = torch.as_tensor(ref64).detach().double()
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref64.shape), (case, what, got.shape, ref64.shape)
    peak = float(ref64.abs().max())
    err = float((got - ref64).abs().max()) / peak if bool(torch.isfinite(got).all()) and peak > 0 else float("inf")
    bound = max(GRAD_TOL, E32_FACTOR * float(e32))
    print(f"{case} grad {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e} peak {peak:.3e}")
    RECORDS.append((case, "grad " + what, err, float(e32), bound))
    if not err <= bound:
        fails.append(f"{case} grad {what}: {err:.3e} > {bound:.2e}")


def no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.
    return model


def load(model, who, head):
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in SC.state(head, who).items()}, strict=True)
    return no_dropout(model).cuda()


def perms_of(G, cid):
    return [G[f"{cid}/perm{j}"] for j in range(G["cfg"]["cases"][cid]["n_perms"])]


def replay(model, perms):
    """the stages draw the recorded permutations, in call order"""
    left = [torch.from_numpy(np.asarray(p)).cuda() for p in perms]
    model._randperm = lambda k, device: left.pop(0)
    return left


def golden_attn(G, cid):
    return [torch.from_numpy(G[f"{cid}/rows32"][j][None]).cuda() for j in range(2)]


@pytest.mark.parametrize("cid", list(SC.CASES))
def test_get_mask_on_the_golden_rows(G, cid):
    c, rec = SC.CASES[cid], G["cfg"]["cases"][cid]
    m = S.MHIM(**SC.model_kwargs(cid)).cuda()
    for _ in range(2):
        left = replay(m, perms_of(G, cid))
        len_keep, ids = m.get_mask(c["n"], 0, golden_attn(G, cid))
        assert not left and len_keep == rec["len_keep"] and ids.shape == (1, c["n"]) and ids.dtype == torch.int64
        assert np.array_equal(ids[0].cpu().numpy(), G[f"{cid}/ids"]), cid
    # one stage on its own, through select_mask_fn, is the restatement's stage
    rows = G[f"{cid}/rows32"][0]
    lk, one = m.select_mask_fn(c["n"], torch.from_numpy(rows[None]).cuda(), True, 0.3, select_inv=False)
    k, _ = MR.stage_sizes(c["n"], 0.3, 1.)
    ref_ids, ref_count, _ = R.select_vote(rows, [(True, k, None)], False)
    assert lk == ref_count and np.array_equal(one[0].cpu().numpy(), ref_ids)


@pytest.mark.parametrize("cid", list(SC.CASES))
def test_forwards_against_float64(G, cid):
    c, rec = SC.CASES[cid], G["cfg"]["cases"][cid]
    heads, act = c["head"], c.get("act", "relu")
    fails = []
    x = torch.from_numpy(SC.bag(cid)).cuda()[None]
    te = load(S.MHIM(**SC.model_kwargs(cid)), "teacher", heads)
    own64_feat, own64 = R.teacher(SC.bag(cid), SC.state(heads, "teacher"), heads, act, ref_row=False)
    for mode in ("train", "eval"):                             # dropout 0: train() and eval() are the same function
        getattr(te, mode)()
        feat, rows = te.forward_teacher(x, return_attn=True)
        assert feat.shape == (1, 512) and [tuple(r.shape) for r in rows] == [(1, heads, c["n"])] * 2
        judge(cid, f"teacher feat ({mode})", feat, G[f"{cid}/teacher_feat"], rec["e32_teacher_feat"], fails)
        for j in range(2):
            judge(cid, f"teacher a{j + 1} own row ({mode})", rows[j][0], own64[j][0], rec[f"e32_teacher_a{j + 1}"], fails)
            # rows are about 1 / n: the same rule at their own size (the row and the recorded error both times n)
            judge(cid, f"teacher a{j + 1} own row x n ({mode})", rows[j][0] * c["n"], own64[j][0] * c["n"],
                  rec[f"e32_teacher_a{j + 1}"] * c["n"], fails)
            if cid in SC.CLS_ROW_CASES:                         # there the reference's row is this row
                judge(cid, f"teacher a{j + 1} vs reference ({mode})", rows[j][0], G[f"{cid}/teacher_a{j + 1}"],
                      rec[f"e32_teacher_a{j + 1}"], fails)
        logits, rows_t = te.forward_test(x, return_attn=True)
        judge(cid, f"forward_test logits ({mode})", logits, G[f"{cid}/teacher_test_logits"], rec["e32_teacher_test_logits"], fails)
        assert all(torch.equal(a, b) for a, b in zip(rows, rows_t)) and torch.equal(te.forward_test(x), logits)
        assert torch.equal(te.forward_teacher(x)[0], feat) and te.forward_teacher(x)[1] is None
    assert R.rel_err(own64_feat, G[f"{cid}/teacher_feat"]) <= 1e-10
    # the student on the golden rows (so on the golden mask) and the golden teacher feature
    st = load(S.MHIM(**SC.model_kwargs(cid)), "student", heads).train()
    tea_feat = torch.from_numpy(G[f"{cid}/teacher_feat"]).float().cuda()
    outs = []
    for _ in range(2):
        replay(st, perms_of(G, cid))
        logits, cls_loss, ps, len_keep = st(x, attn=golden_attn(G, cid), teacher_cls_feat=tea_feat, i=0)
        assert ps == c["n"] and len_keep == rec["len_keep"]
        outs.append((logits.detach().clone(), cls_loss.detach().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the same bag twice, other bits"
    judge(cid, "student logits", outs[0][0], G[f"{cid}/student_logits"], rec["e32_student_logits"], fails)
    judge(cid, "student cls_loss", outs[0][1].reshape(1), G[f"{cid}/student_cls_loss"], rec["e32_student_cls_loss"], fails)
    # pure / forward_bags: the unmasked student
    st.eval()
    with torch.no_grad():
        pure = st.pure(x)
    ref = R.student(SC.bag(cid), SC.state(heads, "student"), None, heads, act=act)
    judge(cid, "pure logits", pure, ref["logits"], rec["e32_student_logits"], fails)
    assert torch.equal(st.forward_bags([x, x[0]])[1], st.forward_test(x)) and torch.equal(st.forward_test(x), pure)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", SC.GRAD_CASES)
def test_train_forward_and_gradients_against_float64(G, cid):
    """MHIM_MIL.train_forward end to end: the restatement runs on the library's OWN rows read back, so a last-bit difference in a
    row cannot flip a mask between the two; then every parameter's gradient and the bag's"""
    c, rec = SC.CASES[cid], G["cfg"]["cases"][cid]
    heads, act = c["head"], c.get("act", "relu")
    fails = []
    model = S.MHIM_MIL(num_epoch=2, niter_per_ep=3, **SC.model_kwargs(cid))
    load(model.student, "student", heads), load(model.teacher, "teacher", heads)
    model.train()
    x = torch.from_numpy(SC.bag(cid)).cuda()[None].requires_grad_(True)
    perms = perms_of(G, cid)
    replay(model.student, perms)
    logits, cls_loss = model(x, i=0)                           # i = 0: mrh_sche[0] = mask_ratio_h
    (logits.sum() + cls_loss).backward()
    with torch.no_grad():
        feat, rows = model.teacher.forward_teacher(x, return_attn=True)
    layer = 1 if c.get("attn_layer", 0) == -1 else c.get("attn_layer", 0)
    len_keep, ids = R.get_mask(c["n"], rows[layer][0].cpu().numpy(), perms, select_inv=c["select_inv"], **SC.ratios(cid))
    tea64, _ = R.teacher(SC.bag(cid), SC.state(heads, "teacher"), heads, act)
    ref = R.student(SC.bag(cid), SC.state(heads, "student"), ids[:len_keep], heads, teacher_feat=tea64, act=act, grad=True)
    (ref["logits"].sum() + ref["cls_loss"]).backward()
    judge(cid, "train_forward logits", logits, ref["logits"], rec["e32_student_logits"], fails)
    judge(cid, "train_forward cls_loss", cls_loss.reshape(1), ref["cls_loss"].reshape(1), rec["e32_student_cls_loss"], fails)
    named = dict(model.student.named_parameters())
    assert len(named) == 25 and set(named) == set(ref["params"])
    for k, p in named.items():
        assert p.grad is not None, k
        judge_grad(cid, k, p.grad, ref["params"][k].grad, rec["grad"][k]["e32"], fails)
    judge_grad(cid, "x", x.grad[0], ref["x_leaf"].grad, rec["grad"]["x"]["e32"], fails)
    assert all(p.grad is None for p in model.teacher.parameters())
    assert not fails, "\n".join(fails)


def test_update_teacher_is_the_ema():
    cid = "n37_std"
    model = S.MHIM_MIL(num_epoch=2, niter_per_ep=3, **SC.model_kwargs(cid))
    load(model.student, "student", 2), load(model.teacher, "teacher", 2)
    before = {k: v.detach().cpu().numpy().copy() for k, v in model.teacher.named_parameters()}
    stu = {k: v.detach().cpu().numpy() for k, v in model.student.named_parameters()}
    model.update_teacher(4)
    want = R.ema(before, stu, model.mm_sche[4])
    for k, v in model.teacher.named_parameters():
        assert R.rel_err(v, want[k]) <= EMA_TOL, k
    assert 0.9999 < model.mm_sche[4] < 1.0 and len(before) == 25


def test_one_host_visit_per_training_step():
    """the kept count's read-back is the step's only device-to-host copy: under torch's sync debug mode ("error") every other
    synchronising call would raise"""
    cid = "n300_hr"
    model = S.MHIM_MIL(num_epoch=2, niter_per_ep=3, **SC.model_kwargs(cid))
    load(model.student, "student", 2), load(model.teacher, "teacher", 2)
    model.train()
    x = torch.from_numpy(SC.bag(cid)).cuda()[None]
    logits, cls_loss = model(x, i=0)                           # warm: library load, allocator
    (logits.sum() + cls_loss).backward()
    visits = []
    real = model.student._select

    def counted(*a, **k):
        torch.cuda.set_sync_debug_mode("default")
        try:
            visits.append(1)
            return real(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    model.student._select = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits, cls_loss = model(x, i=1)
        (logits.sum() + cls_loss).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert visits == [1]


def test_training_step_with_every_dropout_on():
    """train() with the reference's dropouts (0.25 on the embedding, 0.1 in both attention layers, teacher and student): runs,
    finite, and reproducible under torch.manual_seed"""
    cid = "n300_hr"
    kw = dict(SC.model_kwargs(cid), dropout=0.25)
    runs = []
    for _ in range(2):
        model = S.MHIM_MIL(num_epoch=2, niter_per_ep=3, **kw)
        for who, m in (("student", model.student), ("teacher", model.teacher)):
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in SC.state(2, who).items()}, strict=True)
        model.cuda().train()
        assert sorted(m.p for m in model.student.modules() if isinstance(m, torch.nn.Dropout)) == [0.1, 0.1, 0.25]
        x = torch.from_numpy(SC.bag(cid)).cuda()[None]
        torch.manual_seed(1234)
        logits, cls_loss = model(x, i=0)
        (logits.sum() + cls_loss).backward()
        grads = torch.cat([p.grad.reshape(-1) for p in model.student.parameters()])
        assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(cls_loss)) and bool(torch.isfinite(grads).all())
        model.update_teacher(0)
        runs.append((logits.detach().clone(), cls_loss.detach().clone(), grads.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the same seed, other bits"
    model.eval()
    with torch.no_grad():
        assert model(x).shape == (1, SC.N_CLASSES) and torch.equal(model(x), model(x))


def test_refusals_on_the_device():
    m = load(S.MHIM(**SC.model_kwargs("n37_std")), "student", 2).train()
    x = torch.from_numpy(SC.bag("n37_std")).cuda()[None]
    rows = torch.zeros(1, 2, 37).cuda()
    with pytest.raises(_lib.RRTHipError, match="MI355X only"):
        m(x, attn=[rows.cpu(), rows.cpu()])
    with pytest.raises(ValueError, match=r"rrt_mil_amd\.mhim"):
        m(x, attn=torch.zeros(1, 37).cuda())
    with pytest.raises(ValueError, match="one bag per call"):
        m(torch.zeros(2, 37, SC.INPUT_DIM).cuda(), attn=[rows, rows])
    with pytest.raises(NotImplementedError, match="inference output"):
        m.pure(x, return_attn=True)                             # the rows with a graph
    with torch.no_grad():
        out = m.pure(x, return_attn=True)
    assert len(out) == 5 and out[1] == 0 and out[2] == out[3] == 37 and out[4][0].shape == (1, 2, 37)
    with pytest.raises(NotImplementedError, match="attention map"):
        m.online_encoder.layer1.attn.attention_row(torch.zeros(1, 38, 512).cuda(), 0)      # train(), without in_train: as before
