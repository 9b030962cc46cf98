"""GPU (-m gpu): MHIM-MIL (rrt_mil_amd.MHIM / MHIM_MIL / PURE_MHIM) against the reference's goldens (tests/golden/mhim.npz,
tools/make_golden_mhim.py) and the float64 restatement tests/mhim_ref.py (pinned to the goldens by tests/test_mhim_cpu.py) --
never against another kernel.

Masks and counts: exact.  Forward quantities, the project's stage rule: err <= max(2e-5, 8 x e32) relative to
max(1, max |float64 reference|), e32 = the error of the same restatement evaluated in plain fp32 on the CPU, with the golden's
recorded e32 as its floor.  Gradients, the project's gradient rule: within 1e-3 of that gradient tensor's own largest entry.
The EMA: 1e-6 relative to the float64 formula (two fp32 roundings and a possible contraction: ~2e-7).
Nothing more runs after a device error.  Importing this module needs no device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mhim_cases as MC
import mhim_ref as R
from conftest import load_golden
from rrt_mil_amd import MHIM, MHIM_MIL, PURE_MHIM, _lib

pytestmark = pytest.mark.gpu
TOL, E32_FACTOR, GRAD_TOL, EMA_TOL = 2e-5, 8.0, 1e-3, 1e-6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()


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
    return load_golden("mhim")


def judge(case, what, got, ref64, ref32, fails, e32_floor=0.0):
    ref64, ref32 = torch.as_tensor(ref64).detach().double(), torch.as_tensor(ref32).detach()
    e32 = max(R.rel_err(ref32, ref64), float(e32_floor))
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (case, what, got.shape, ref64.shape)
    err = R.rel_err(got, ref64) if bool(torch.isfinite(got).all()) else float("inf")
    bound = max(TOL, E32_FACTOR * e32)
    print(f"{case} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


def load(model, who):
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in MC.state(MC.shapes_of(), who).items()}, strict=True)
    return model.cuda()


class Recorded(MHIM):
    """MHIM whose stages draw the recorded permutations, in call order"""

    def _randperm(self, k, device):
        p = self.perms.pop(0)
        assert p.size == k, (p.size, k)
        return torch.from_numpy(p).to(device)


def student_of(cid, G, cls=Recorded):
    m = load(cls(**MC.model_kwargs(cid)), "student").train()        # dropout 0: train() draws nothing
    n_perms = G["cfg"]["cases"][cid]["n_perms"]
    m.perms = [G[f"{cid}/perm{j}"] for j in range(n_perms)]
    return m


def sides(cid):
    c = MC.CASES[cid]
    return c.get("act", "relu"), c.get("da_act", "relu")


@pytest.mark.parametrize("cid", list(MC.CASES))
def test_get_mask_is_the_references(G, cid):
    c = G["cfg"]["cases"][cid]
    m = student_of(cid, G)
    attn = torch.from_numpy(G[f"{cid}/attn32"]).cuda()[None]
    len_keep, mask_ids = m.get_mask(c["n"], None, attn)
    assert not m.perms and len_keep == c["len_keep"]
    assert mask_ids.shape == (1, c["n"]) and mask_ids.dtype == torch.int64 and mask_ids.is_cuda
    ids = mask_ids[0].cpu().numpy()
    assert np.array_equal(ids[:len_keep], G[f"{cid}/kept"])
    assert np.array_equal(np.sort(ids), np.arange(c["n"])) and np.all(np.diff(ids[len_keep:]) > 0)


@pytest.mark.parametrize("cid", list(MC.CASES))
def test_student_teacher_and_eval_paths_against_the_goldens(G, cid):
    fails = []
    act, da = sides(cid)
    st, te = MC.state(MC.shapes_of(), "student"), MC.state(MC.shapes_of(), "teacher")
    x = MC.bag(cid)
    xd = torch.from_numpy(x).cuda()[None]
    m, t = student_of(cid, G), load(MHIM(**MC.model_kwargs(cid)), "teacher").train()
    e = lambda q: float(G[f"{cid}/e32_{q}"])   # noqa: E731
    # teacher
    feat, attn = t.forward_teacher(xd, return_attn=True)
    r64, r32 = R.teacher(x, te, act, da), R.teacher(x, te, act, da, dtype=torch.float32)
    assert feat.shape == (1, 512) and attn.shape == (1, x.shape[0]) and t.forward_teacher(xd)[1] is None
    judge(cid, "tea_feat", feat, G[f"{cid}/tea_feat"], r32[0], fails, e("tea_feat"))
    judge(cid, "tea_attn", attn, G[f"{cid}/tea_attn"], r32[1], fails, e("tea_attn"))
    # student on the golden mask (the recorded scores and permutations), the golden's float64 teacher row
    tea = torch.from_numpy(G[f"{cid}/tea_feat"]).float().cuda()
    logits, cls_loss, ps, len_keep = m(xd, torch.from_numpy(G[f"{cid}/attn32"]).cuda()[None], tea, None)
    assert ps == x.shape[0] and len_keep == G["cfg"]["cases"][cid]["len_keep"]
    s32 = R.student(x, st, G[f"{cid}/kept"], teacher_feat=G[f"{cid}/tea_feat"], act=act, da_act=da, dtype=torch.float32)
    judge(cid, "logits", logits, G[f"{cid}/logits"], s32["logits"], fails, e("logits"))
    judge(cid, "cls_loss", cls_loss.reshape(1), G[f"{cid}/cls_loss"], s32["cls_loss"].reshape(1), fails, e("cls_loss"))
    # eval: forward_test and pure are the one-call path
    m.eval()
    f32 = R.forward_test(x, st, act, da, dtype=torch.float32)
    lg, a = m.forward_test(xd, return_attn=True)
    _, raw = m.forward_test(xd, return_attn=True, no_norm=True)
    judge(cid, "test_logits", lg, G[f"{cid}/test_logits"], f32[0], fails, e("test_logits"))
    judge(cid, "test_attn", a, G[f"{cid}/test_attn"], f32[1], fails, e("test_attn"))
    judge(cid, "test_raw", raw, G[f"{cid}/test_raw"], f32[2], fails, e("test_raw"))
    with torch.no_grad():
        pl, pa = m.pure(xd, return_attn=True)
    assert torch.equal(pl, m.forward_test(xd)) and torch.equal(pl, lg) and torch.equal(pa, a)
    m.train()
    out = m.pure(xd)
    assert len(out) == 4 and out[1:] == (0, x.shape[0], x.shape[0])
    judge(cid, "pure(train) logits", out[0], G[f"{cid}/test_logits"], f32[0], fails, e("test_logits"))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", ["n300_std", "n37_hr_inv", "n300_high_only"])
def test_end_to_end_teacher_mask_student(G, cid):
    """MHIM_MIL.train_forward: the restatement selects on the DEVICE's own fp32 attention row (exact), then runs the student
    in float64 on that mask"""
    fails = []
    act, da = sides(cid)
    c = MC.CASES[cid]
    kw = dict(MC.model_kwargs(cid), num_epoch=2, niter_per_ep=3)
    model = MHIM_MIL(**kw)
    load(model.student, "student"), load(model.teacher, "teacher")
    model.train()
    perms = []
    real = model.student._randperm
    model.student._randperm = lambda k, device: perms.append(real(k, device)) or perms[-1]
    seen = {}
    real_teacher = model.teacher.forward_teacher
    model.teacher.forward_teacher = lambda *a, **k: seen.setdefault("t", real_teacher(*a, **k))
    x = MC.bag(cid)
    step = 1
    logits, cls_loss = model(torch.from_numpy(x).cuda()[None], i=step)
    feat, attn = seen["t"]
    ratios = {k: c[k] for k in MC.RATIO_KEYS}
    ratios["mask_ratio_h"] = model.student.mrh_sche[step]
    len_keep, ids = R.get_mask(c["n"], attn[0].cpu().numpy(), [p.cpu().numpy() for p in perms], select_inv=c["select_inv"], **ratios)
    st = MC.state(MC.shapes_of(), "student")
    o64 = R.student(x, st, ids[:len_keep], teacher_feat=feat.cpu().numpy(), act=act, da_act=da)
    o32 = R.student(x, st, ids[:len_keep], teacher_feat=feat.cpu().numpy(), act=act, da_act=da, dtype=torch.float32)
    assert logits.shape == (1, MC.N_CLASSES)
    judge(cid, "e2e logits", logits, o64["logits"], o32["logits"], fails)
    judge(cid, "e2e cls_loss", cls_loss.reshape(1), o64["cls_loss"].reshape(1), o32["cls_loss"].reshape(1), fails)
    # the mask the device chose is the restatement's: the student's own report of it
    model.student._randperm = lambda k, device, it=iter(perms): next(it)
    lk, mids = model.student.get_mask(c["n"], step, attn)
    assert lk == len_keep and np.array_equal(mids[0].cpu().numpy(), ids)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", MC.GRAD_CASES)
def test_gradients(G, cid):
    """every student parameter and the bag, loss = CE(logits, 1) + 0.5 cls_loss as Survival's engine weighs it, at dropout 0"""
    act, da = sides(cid)
    m = student_of(cid, G)
    x = MC.bag(cid)
    xd = torch.from_numpy(x).cuda()[None].requires_grad_(True)
    tea = G[f"{cid}/tea_feat"]
    logits, cls_loss, _, len_keep = m(xd, torch.from_numpy(G[f"{cid}/attn32"]).cuda()[None], torch.from_numpy(tea).float().cuda(), None)
    (F.cross_entropy(logits, torch.tensor([1]).cuda()) + 0.5 * cls_loss).backward()
    ref = R.student(x, MC.state(MC.shapes_of(), "student"), G[f"{cid}/kept"], teacher_feat=tea, act=act, da_act=da, grad=True)
    (F.cross_entropy(ref["logits"], torch.tensor([1])) + 0.5 * ref["cls_loss"]).backward()
    fails = []
    pairs = [("x", xd.grad[0], ref["x_leaf"].grad)] + [(k, p.grad, ref["params"][k].grad) for k, p in m.named_parameters()]
    assert len(pairs) == 1 + len(R.KEYS)
    for name, got, want in pairs:
        assert got is not None and want is not None, name
        got, want = got.detach().cpu().double(), want.detach()
        top = float(want.abs().max())
        err = float((got - want).abs().max()) / top
        print(f"{cid} d {name}: err {err:.3e} of max {top:.3e}")
        if not (bool(torch.isfinite(got).all()) and err <= GRAD_TOL):
            fails.append(f"{cid} d {name}: {err:.3e} > {GRAD_TOL}")
    # the dropped rows of the bag receive exactly zero
    dropped = np.setdiff1d(np.arange(x.shape[0]), G[f"{cid}/kept"])
    assert bool((xd.grad[0][torch.from_numpy(dropped).cuda()] == 0).all())
    assert not fails, "\n".join(fails)


def test_update_teacher_is_the_float64_formula():
    model = MHIM_MIL(**dict(MC.model_kwargs("n300_std"), num_epoch=2, niter_per_ep=3))
    load(model.student, "student"), load(model.teacher, "teacher")
    for index, sched in ((2, True), (0, False)):
        if not sched:
            model.mm_sche, model.mm = None, 0.99
        mm = model.mm_sche[index] if sched else 0.99
        before = {k: v.detach().cpu().numpy() for k, v in model.teacher.named_parameters()}
        want = R.ema(before, {k: v.detach().cpu().numpy() for k, v in model.student.named_parameters()}, mm)
        model.update_teacher(index)
        for k, v in model.teacher.named_parameters():
            err = np.abs(v.detach().cpu().numpy().astype(np.float64) - want[k]).max() / max(np.abs(want[k]).max(), 1e-30)
            assert err <= EMA_TOL, (k, err)
        assert all(torch.equal(v, torch.from_numpy(np.array(MC.state(MC.shapes_of(), "student")[k])).cuda())
                   for k, v in model.student.named_parameters()), "the student moved"


def test_forward_bags_is_forward_bag_per_bag():
    m = load(MHIM(**MC.model_kwargs("n300_std")), "student").eval()
    bags = [torch.from_numpy(MC.bag(c)).cuda() for c in ("n300_std", "n37_std", "n300_hr", "n37_hr_inv", "n300_inv")]
    one = [m.forward_bag(b, solo=False) for b in bags]
    for streams in (1, 4):
        many = m.forward_bags(bags, streams=streams)
        ref = one if streams > 1 else [m.forward_bag(b, solo=True) for b in bags]
        assert all(torch.equal(a, b) for a, b in zip(many, ref)), streams
    full = m.forward_bags(bags[:2], streams=2, return_attn=True)
    assert full[1]["attn"].shape == (37,) and torch.equal(full[0]["logits"], one[0])


def test_manual_seed_reproduces_a_training_steps_mask():
    cid = "n300_std"
    model = MHIM_MIL(**dict(MC.model_kwargs(cid), num_epoch=2, niter_per_ep=3))
    load(model.student, "student"), load(model.teacher, "teacher")
    model.train()
    x = torch.from_numpy(MC.bag(cid)).cuda()[None]
    masks = []
    real = model.student.get_mask
    model.student.get_mask = lambda *a, **k: masks.append(real(*a, **k)) or masks[-1]
    outs = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        outs.append(model(x, i=0))
    (k0, m0), (k1, m1), (k2, m2) = masks
    assert k0 == k1 and torch.equal(m0, m1) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(m0, m2), "another seed drew the same mask"


def test_main_params_train_eval_and_checkpoints(tmp_path):
    """the parameters of Survival/main.py:138-149 on a bag of 1024-wide features: train step, teacher update, eval, reload"""
    model = MHIM_MIL(**MC.MAIN_PARAMS).cuda().train()
    opt = torch.optim.SGD(model.student.parameters(), lr=1e-3)
    x = torch.randn(1, 1500, 1024, generator=torch.Generator().manual_seed(3)).abs().cuda()
    torch.manual_seed(11)
    logits, cls_loss = model(x, i=5)
    assert logits.shape == (1, 2) and cls_loss.dim() == 0 and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(cls_loss))
    (F.cross_entropy(logits, torch.tensor([0]).cuda()) + 0.5 * cls_loss).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.student.parameters())
    assert all(p.grad is None for p in model.teacher.parameters())
    opt.step()
    model.update_teacher(5)
    model.eval()
    with torch.no_grad():
        ev = model(x)
    assert ev.shape == (1, 2)
    path = tmp_path / "mhim.pt"
    torch.save(model.state_dict(), path)
    again = MHIM_MIL(**MC.MAIN_PARAMS)
    again.load_state_dict(torch.load(path), strict=True)
    with torch.no_grad():
        assert torch.equal(again.cuda().eval()(x), ev)
    base = PURE_MHIM().cuda().eval()
    with torch.no_grad():
        assert base(x).shape == (1, 2)
    torch.save(base.model.state_dict(), tmp_path / "base.pt")
    init = MHIM_MIL(**dict(MC.MAIN_PARAMS, teacher_init=str(tmp_path / "base.pt")))
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(init.teacher.state_dict().values(), base.model.state_dict().values()))
    assert torch.equal(init.student.patch_to_emb[0].weight.cpu(), base.model.patch_to_emb[0].weight.cpu())


def test_one_host_visit_per_training_step():
    """the kept count's read-back is the step's only device-to-host copy: under torch's sync debug mode ("error") every other
    synchronising call would raise"""
    cid = "n300_std"
    model = MHIM_MIL(**dict(MC.model_kwargs(cid), num_epoch=2, niter_per_ep=3))
    load(model.student, "student"), load(model.teacher, "teacher")
    model.train()
    x = torch.from_numpy(MC.bag(cid)).cuda()[None]
    model(x, i=0)                                           # warm: library load, allocator
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


def test_refusals_on_the_device():
    with pytest.raises(NotImplementedError, match="selfattn"):
        MHIM_MIL(**dict(MC.MAIN_PARAMS, baseline="selfattn"))
    with pytest.raises(NotImplementedError, match="mlp_dim"):
        MHIM(baseline="attn", mlp_dim=256)
    m = load(MHIM(**MC.model_kwargs("n37_std")), "student").train()
    x = torch.from_numpy(MC.bag("n37_std"))[None]
    with pytest.raises(_lib.RRTHipError, match="MI355X only"):
        m(x, attn=torch.zeros(1, 37).cuda())
    with pytest.raises(_lib.RRTHipError, match="MI355X only"):
        m(x.cuda(), attn=torch.zeros(1, 37))
    with pytest.raises(NotImplementedError, match="selfattn"):
        m(x.cuda(), attn=torch.zeros(1, 2, 37).cuda())
    with pytest.raises(ValueError, match="attn is None"):
        m(x.cuda())
    with pytest.raises(ValueError, match="one bag per call"):
        m(torch.zeros(2, 37, MC.INPUT_DIM).cuda(), attn=torch.zeros(1, 37).cuda())
