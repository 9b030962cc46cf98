"""GPU (-m gpu): rrt_mil_amd.DTFD against the reference's goldens (tests/golden/dtfd.npz, tools/make_golden_dtfd.py) and the
float64 restatement tests/dtfd_ref.py (pinned to the goldens by tests/test_dtfd_cpu.py) -- never against another kernel.

Selections: exact, every group (the golden tool asserted that every group's extremes are unique and clear of the runner-up by
64 x the reference's own fp32 error).  Forward quantities, the project's value rule: err <= max(2e-5, 8 x e32) relative to
max(1, max |float64 reference|), e32 = the error of the same restatement evaluated in fp32 on the CPU, with the golden's
recorded e32 as its floor.  Gradients, the project's gradient rule: within 1e-3 of that gradient tensor's own largest entry;
the two ``attention_weights.bias`` gradients are sums that cancel to zero in exact arithmetic (a softmax does not see a shift
of its scores) and are measured against the largest entry of the weight gradient of the same Linear, which adds up the same
terms.  Nothing more runs after a device error.  Importing this module needs no device."""
import random

import numpy as np
import pytest
import torch

import dtfd_cases as DC
import dtfd_ref as R
from conftest import load_golden
from rrt_mil_amd import DTFD, RRTEncoder, _lib

pytestmark = pytest.mark.gpu
TOL, E32_FACTOR, GRAD_TOL = 2e-5, 8.0, 1e-3


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
    return load_golden("dtfd")


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


def model_of(cid, **kw):
    m = DTFD(1e-4, 1e-5, 10, R.nll_surv, **dict(DC.model_kwargs(cid), **kw))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    st = {k: torch.from_numpy(np.array(v)) for k, v in DC.state(DC.CASES[cid]["n_classes"]).items()}
    if "rrt" not in kw:
        m.load_state_dict(st, strict=True)
    else:
        missing, unexpected = m.load_state_dict(st, strict=False)
        assert not unexpected and all(k.startswith("dimReduction.rrt.") for k in missing)
    return m.cuda()


@pytest.mark.parametrize("cid", list(DC.CASES))
def test_eval_against_the_goldens(G, cid):
    c, fails = DC.CASES[cid], []
    m = model_of(cid).eval()
    x = torch.from_numpy(DC.bag(cid)).cuda()
    perm = G[f"{cid}/perm"]
    with torch.no_grad():
        logits, sel, p = m.forward_bag(x, perm=perm, return_sel=True, return_cam=True)
        assert sel.dtype == torch.int64 and sel.shape == (c["group"], 2) and p.shape == (c["n"],) and logits.shape == (1, c["n_classes"])
        # the reference's selection, every group
        assert np.array_equal(sel.cpu().numpy(), G[f"{cid}/sel"]), (sel.cpu().numpy().tolist(), G[f"{cid}/sel"].tolist())
        r64 = R.eval_forward(DC.bag(cid), DC.state(c["n_classes"]), perm, c["group"], c["distill"])
        r32 = R.eval_forward(DC.bag(cid), DC.state(c["n_classes"]), perm, c["group"], c["distill"], dtype=torch.float32,
                             sel=G[f"{cid}/sel"])
        e = lambda q: float(G[f"{cid}/e32_{q}"])   # noqa: E731
        judge(cid, "p", p, r64["p"], r32["p"], fails, e("p"))
        judge(cid, "logits", logits, G[f"{cid}/logits64"], r32["logits"], fails, e("logits"))
        hazards = torch.sigmoid(logits)
        judge(cid, "hazards", hazards, G[f"{cid}/hazards64"], r32["hazards"], fails, e("hazards"))
        judge(cid, "S", torch.cumprod(1 - hazards, 1), G[f"{cid}/S64"], r32["S"], fails, e("S"))
        # model(bag) draws the reference's permutation from the same seed: the same call, the same bits
        random.seed(c["seed"])
        h2, s2 = m(x[None])
        assert torch.equal(h2, hazards) and torch.equal(s2, torch.cumprod(1 - hazards, 1))
        assert torch.equal(m.forward_bag(x, perm=perm), logits)
        # the plain loop over bags, and the identity permutation as the default
        both = m.forward_bags([x, x[None]], perm=perm)
        assert torch.equal(both[0], logits) and torch.equal(both[1], logits)
        assert torch.equal(m.forward_bag(x), m.forward_bag(x, perm=np.arange(c["n"])))
    # the layer path (a graph) on the same permutation agrees with the one call
    random.seed(c["seed"])
    h3, s3 = m(x[None])
    assert h3.requires_grad
    judge(cid, "layer-path hazards", h3, G[f"{cid}/hazards64"], r32["hazards"], fails, e("hazards"))
    judge(cid, "layer-path S", s3, G[f"{cid}/S64"], r32["S"], fails, e("S"))
    judge(cid, "layer path against the one call", h3, hazards.cpu().double(), hazards.cpu(), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", DC.TRAIN_CASES)
def test_training_step_against_the_goldens(G, cid):
    c, fails = DC.CASES[cid], []
    m = model_of(cid).train()                     # dropout 0: train() draws nothing
    x = torch.from_numpy(DC.bag(cid)).cuda()[None].requires_grad_()
    ref = R.train_step(DC.bag(cid), DC.state(c["n_classes"]), c["group"], c["distill"], **DC.LABEL)
    ref32 = R.train_step(DC.bag(cid), DC.state(c["n_classes"]), c["group"], c["distill"], **DC.LABEL, dtype=torch.float32,
                         sel=G[f"{cid}/train_sel"])
    assert np.array_equal(ref["sel"], G[f"{cid}/train_sel"])

    def grads(which):
        for k, p_ in m.named_parameters():
            got = torch.zeros_like(p_) if p_.grad is None else p_.grad
            want = ref[which][k]
            yard = ref[which][k[:-4] + "weight"] if k.endswith("attention_weights.bias") else want
            top = float(yard.abs().max())
            if top == 0.0:                        # (UClassifier before the outer backward: no gradient at all)
                assert p_.grad is None or not bool(p_.grad.any()), (which, k)
                continue
            err = float((got.detach().cpu().double() - want).abs().max()) / top
            print(f"{cid} {which} d {k}: err {err:.3e} of max {top:.3e}")
            if not (bool(torch.isfinite(got).all()) and err <= GRAD_TOL):
                fails.append(f"{cid} {which} d {k}: {err:.3e} > {GRAD_TOL}")

    hazards, S = m(x, label=DC.LABEL)
    assert hazards.shape == (1, c["n_classes"]) and S.shape == (1, c["n_classes"]) and hazards.requires_grad
    e = lambda q: float(G[f"{cid}/e32_train_{q}"])   # noqa: E731
    judge(cid, "hazards", hazards, G[f"{cid}/train_hazards"], ref32["hazards"], fails, e("hazards"))
    judge(cid, "S", S, G[f"{cid}/train_S"], ref32["S"], fails, e("S"))
    judge(cid, "loss0", m.loss0.reshape(1), G[f"{cid}/train_loss0"], ref32["loss0"], fails, e("loss0"))
    grads("inner")                                # the forward alone has back-propagated the pseudo-bag loss
    loss = R.nll_surv(hazards=hazards, S=S, Y=torch.tensor([DC.LABEL["label"]]).cuda(), c=torch.tensor([DC.LABEL["censorship"]]).cuda())
    judge(cid, "loss", loss.reshape(1), G[f"{cid}/train_loss"], ref32["loss"], fails, e("loss"))
    loss.backward()
    grads("outer")
    top = float(ref["dx"].abs().max())
    err = float((x.grad[0].cpu().double() - ref["dx"]).abs().max()) / top
    print(f"{cid} d x: err {err:.3e} of max {top:.3e}")
    if not err <= GRAD_TOL:
        fails.append(f"{cid} d x: {err:.3e} > {GRAD_TOL}")
    assert not fails, "\n".join(fails)


def test_reference_checkpoints_load_strictly_both_ways():
    cid = "n37_g3_c2_maxmin"
    st = {k: torch.from_numpy(np.array(v)) for k, v in DC.state(2).items()}
    m = model_of(cid)
    back = {k: v.cpu() for k, v in m.state_dict().items()}
    assert list(back) == list(st) and all(torch.equal(back[k], st[k]) for k in st)
    m2 = DTFD(1e-4, 1e-5, 10, R.nll_surv, **DC.model_kwargs(cid))
    m2.load_state_dict(m.state_dict(), strict=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_one_call_under_autocast_keeps_the_pool_and_the_selection_in_fp32(dtype):
    """with an encoder under autocast the front and the gate Linears run on 16-bit operands; the scores, the pool, the CAM
    and the selection stay fp32: the selection is exactly the rule applied to the call's own p, and the answer stays near
    the fp32 call's unless another instance was selected"""
    cid = "n300_g8_c2_maxmin"
    c = DC.CASES[cid]
    torch.manual_seed(7)
    m = model_of(cid, rrt=RRTEncoder(mlp_dim=512, epeg_k=15, crmsa_k=3, drop_out=0.)).eval()
    x = torch.from_numpy(DC.bag(cid)).cuda()
    perm = np.array(load_golden("dtfd")[f"{cid}/perm"])
    with torch.no_grad():
        ref, ref_sel = m.forward_bag(x, perm=perm, return_sel=True)
        with torch.autocast("cuda", dtype=dtype):
            logits, sel, p = m.forward_bag(x, perm=perm, return_sel=True, return_cam=True)
            again = m.forward_bag(x, perm=perm)      # the second call reuses the 16-bit weight images of the first
    assert logits.dtype == torch.float32 and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(p).all())
    assert torch.equal(again, logits)
    assert np.array_equal(sel.cpu().numpy(), R.select_from_p(p.cpu().numpy(), perm, c["group"]))
    print(f"autocast {dtype}: max |logits - fp32| {float((logits - ref).abs().max()):.3e}, "
          f"{int((sel != ref_sel).sum())} of {sel.numel()} selections differ")
    if torch.equal(sel, ref_sel):
        # 16-bit operands (eps 2^-8 / 2^-11) through six GEMM layers, fp32 accumulation: well inside 0.1 on logits of O(1)
        assert float((logits - ref).abs().max()) < 0.1


def test_with_the_encoder_in_eval_and_for_one_training_step():
    """rrt=RRTEncoder at N = 300: the reference cannot provide a golden (its encoder file is missing); finite outputs, and the
    one call agrees with the layer path"""
    cid = "n300_g8_c2_maxmin"
    c = DC.CASES[cid]
    torch.manual_seed(7)
    m = model_of(cid, rrt=RRTEncoder(mlp_dim=512, epeg_k=15, crmsa_k=3, drop_out=0.)).eval()
    assert any(k.startswith("dimReduction.rrt.") for k in m.state_dict())
    x = torch.from_numpy(DC.bag(cid)).cuda()
    perm = np.array(load_golden("dtfd")[f"{cid}/perm"])
    with torch.no_grad():
        logits, sel, p = m.forward_bag(x, perm=perm, return_sel=True, return_cam=True)
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(p).all())
    assert np.array_equal(sel.cpu().numpy(), R.select_from_p(p.cpu().numpy(), perm, c["group"]))
    random.seed(c["seed"])
    hazards, S = m(x[None])                       # parameters require grad: the layer path, the same permutation
    assert hazards.requires_grad
    one = torch.sigmoid(logits)
    fails = []
    judge(cid, "rrt hazards", hazards, one.cpu().double(), one.cpu(), fails)
    judge(cid, "rrt S", S, torch.cumprod(1 - one, 1).cpu().double(), torch.cumprod(1 - one, 1).cpu(), fails)
    assert not fails, "\n".join(fails)
    m.train()
    for mod in m.modules():                       # (the encoder was built with drop_out=0)
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    xg = x[None].clone().requires_grad_()
    hazards, S = m(xg, label=DC.LABEL)
    inner = {k: p_.grad.clone() for k, p_ in m.named_parameters() if p_.grad is not None}
    assert any(k.startswith("dimReduction.rrt.") for k in inner) and not any(k.startswith("UClassifier.") for k in inner)
    R.nll_surv(hazards=hazards, S=S, Y=torch.tensor([1]).cuda(), c=torch.tensor([0]).cuda()).backward()
    assert bool(torch.isfinite(hazards).all()) and bool(torch.isfinite(S).all()) and bool(torch.isfinite(m.loss0))
    assert all(p_.grad is not None and bool(torch.isfinite(p_.grad).all()) for p_ in m.parameters())
    assert bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.any())
