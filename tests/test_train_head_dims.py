"""GPU (-m gpu): training at R-MSA head dims other than 64 -- the matrix-core attention backward at head dims 16 .. 256
(multiples of 16), any region size, the 1-D 'attn' EPEG with epeg_k <= 63 or none.  The stage against float64 autograd of
the explicit formulation; the encoder in train() against the float64 oracle, with dropout, drop-path and autocast; bitwise
reproducibility; RRTMIL(n_heads=4) end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import STATE_KEYS
from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()


def _cmp(got, ref, tol, what):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= tol, f"{what}: max-abs {err:.3e} > {tol:.1e}"
    return err


# ------------------------------------------------------------------ the stage
HDS = [16, 32, 48, 96, 128, 192, 256]
PS = [1, 4, 7, 49, 129, 144, 177, 256, 484]
EKS = [9, 21, 31, 63]


def _stage_cases():
    """every (head dim, P) with epeg_k 0, 15 and one of 9 / 21 / 31 / 63 in turn (31, wider than the region, at P = 4)"""
    out = []
    for a, hd in enumerate(HDS):
        for b, P in enumerate(PS):
            third = 31 if P == 4 else EKS[(a + b) % len(EKS)]
            out += [(hd, P, ek) for ek in (0, 15, third)]
    return out


def _stage_inputs(R, P, D, heads, ek):
    hd = D // heads
    raw = synth.normal(f"abh/qkv{R}x{P}x{D}", (R * P, 3 * D)) * 0.6
    pe = synth.uniform(f"abh/pe{heads}x{ek}", (heads, max(ek, 1)), -1, 1) / np.sqrt(max(ek, 1))
    pb = synth.uniform(f"abh/pb{heads}", (heads,), -0.3, 0.3)
    dO = synth.normal(f"abh/do{R}x{P}x{D}", (R * P, D))
    stash = raw.copy()
    stash[:, :D] *= hd ** -0.5                       # the forward stage stores q already scaled
    return raw, pe, pb, dO, stash


def _stage_backward(stash, pe, o, dO, R, P, D, heads, ek):
    """rrt_region_attention_backward_f32 with outputs and workspace pre-filled with NaN / 0xFF: unwritten output fails"""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    d_stash, d_pe, d_dO = dev(stash), dev(pe), dev(dO)
    dqkv = torch.full((R * P, 3 * D), float("nan"), device=DEV)
    dpe = torch.full((heads, max(ek, 1)), float("nan"), device=DEV)
    need = C.c_size_t()
    _lib.check(lib.rrt_region_attention_backward_workspace_size(R, P, D, heads, ek, C.byref(need)), "attn bwd ws")
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rrt_region_attention_backward_f32(p(d_stash), p(d_pe) if ek else None, p(o), p(d_dO), p(dqkv),
                                                     p(dpe) if ek else None, R, P, D, heads, ek, p(ws), ws.numel(),
                                                     stream()), "attention_backward")
    torch.cuda.synchronize()
    return dqkv.cpu().numpy(), dpe.cpu().numpy()


@pytest.mark.parametrize("hd,P,ek", _stage_cases())
def test_region_attention_backward_head_dims(hd, P, ek):
    """scores [P,P], a depth-wise conv along the query axis WITH a bias, softmax, A V -- float64 autograd against the HIP
    backward stage: d_qkv in the stash layout (q pre-scaled), the tap gradients, and the exactly-zero bias gradient"""
    from hip_util import dev, region_attention
    R, heads = 2, (3 if hd <= 96 else 2)
    D = hd * heads
    raw, pe, pb, dO, stash = _stage_inputs(R, P, D, heads, ek)
    tq = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    tw = torch.tensor(pe, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(pb, dtype=torch.float64, requires_grad=True)
    t = tq.reshape(R, P, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * hd ** -0.5, t[1], t[2]
    S = q @ k.transpose(-2, -1)
    if ek:
        S = S + torch.nn.functional.conv2d(S, tw.reshape(heads, 1, ek, 1), tb, padding=(ek // 2, 0), groups=heads)
    Oref = (S.softmax(-1) @ v).transpose(1, 2).reshape(R * P, D)
    (Oref * torch.tensor(dO, dtype=torch.float64)).sum().backward()
    o = region_attention(dev(stash), dev(pe) if ek else None, R, P, D, heads, ek)
    _cmp(o.cpu().numpy(), Oref.detach().numpy(), 5e-5, "forward O")
    got, dpe = _stage_backward(stash, pe, o, dO, R, P, D, heads, ek)
    ref = tq.grad.numpy()
    _cmp(got[:, :D], ref[:, :D], 1e-4, "dq")
    _cmp(got[:, D:2 * D], ref[:, D:2 * D], 1e-4, "dk")
    _cmp(got[:, 2 * D:], ref[:, 2 * D:], 1e-4, "dv")
    if ek:
        scale = max(1.0, np.sqrt(R * P))
        _cmp(dpe / scale, tw.grad.numpy() / scale, 1e-4, "d taps")
        assert np.abs(tb.grad.numpy()).max() < 1e-9 * R * P          # Identity 2: the bias gradient is zero


@pytest.mark.parametrize("hd,P,ek", [(128, 177, 15), (32, 484, 63), (256, 49, 0)])
def test_region_attention_backward_head_dims_reproducible(hd, P, ek):
    """the same backward twice: bit-identical d_qkv and taps (fixed-order sums, no atomics)"""
    from hip_util import dev, region_attention
    R, heads = 3, 2
    D = hd * heads
    _, pe, _, dO, stash = _stage_inputs(R, P, D, heads, ek)
    o = region_attention(dev(stash), dev(pe) if ek else None, R, P, D, heads, ek)
    a = _stage_backward(stash, pe, o, dO, R, P, D, heads, ek)
    b = _stage_backward(stash, pe, o, dO, R, P, D, heads, ek)
    assert np.array_equal(a[0], b[0])
    if ek:
        assert np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ the encoder in train()
CASES = {
    "h2_n9000": (9000, dict(mlp_dim=512, n_heads=2, epeg_k=15, crmsa_k=3)),             # head dim 256
    "h4_n9000": (9000, dict(mlp_dim=512, n_heads=4, epeg_k=15, crmsa_k=3)),             # 128
    "h16_n9000": (9000, dict(mlp_dim=512, n_heads=16, epeg_k=15, crmsa_k=3)),           # 32
    "h32_n9000": (9000, dict(mlp_dim=512, n_heads=32, epeg_k=15, crmsa_k=3)),           # 16
    "d1024_h8_n3000": (3000, dict(mlp_dim=1024, n_heads=8, epeg_k=15, crmsa_k=3)),      # 128
    "d768_h8_n15000": (15000, dict(mlp_dim=768, n_heads=8, epeg_k=15, crmsa_k=3)),      # 96, P = 256
    "d384_h8_n3000": (3000, dict(mlp_dim=384, n_heads=8, epeg_k=15, crmsa_k=3)),        # 48
    "d256_h8_rn16_n3000": (3000, dict(mlp_dim=256, n_heads=8, epeg_k=15, crmsa_k=3, region_num=16)),   # 32
    "h4_noepeg_n9000": (9000, dict(mlp_dim=512, n_heads=4, epeg=False, crmsa_k=3)),
    "h4_valuebf_n9000": (9000, dict(mlp_dim=512, n_heads=4, epeg_k=9, crmsa_k=3, epeg_type="value_bf")),
    "h4_crheads1_sc_n3000": (3000, dict(mlp_dim=512, n_heads=4, epeg_k=15, crmsa_k=3, crmsa_heads=1, all_shortcut=True)),
    "h4_n1": (1, dict(mlp_dim=512, n_heads=4, epeg_k=15, crmsa_k=3)),
    "h4_n50": (50, dict(mlp_dim=512, n_heads=4, epeg_k=15, crmsa_k=3)),
}


def _encoder(st, cfg, **kw):
    from hip_util import DEV
    from rrt_mil_amd import RRTEncoder
    enc = RRTEncoder(**kw, **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    return enc.to(DEV).train()


def _case(case):
    N, cfg = CASES[case]
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k in STATE_KEYS})
    x = synth.bag(N, cfg["mlp_dim"], tag="trainhd/" + case)
    G = synth.normal("trainhd/G/" + case, (N, cfg["mlp_dim"]))
    return N, cfg, st, x, G


@pytest.mark.parametrize("case", list(CASES))
def test_encoder_backward_head_dims(case):
    """loss = <y, G>: every parameter gradient and dL/dx against torch autograd of the reference's op sequence in float64
    (tolerances as test_hip_parity.py::test_encoder_backward_matches_autograd)"""
    from hip_util import dev
    N, cfg, st, x, G = _case(case)
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = _encoder(st, cfg, drop_out=0.)
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    assert y.grad_fn is not None
    _cmp(y.detach().cpu().numpy(), y64.detach().numpy(), 2e-4, case + " train forward")
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    floor = 1e-3 * max([float(x_leaf.grad.abs().max())] + [float(v.grad.abs().max()) for v in params.values()
                                                           if v.grad is not None])

    def rel(got, ref, what):
        ref = ref.astype(np.float64)
        scale = max(np.abs(ref).max(), floor, 1e-6)
        err = np.abs(got.astype(np.float64) - ref).max() / scale
        assert np.isfinite(got).all(), what
        assert err <= 2e-3, f"{case} {what}: max error {err:.2e} of the largest gradient entry"

    rel(xd.grad.cpu().numpy(), x_leaf.grad.numpy(), "dx")
    for name, prm in enc.named_parameters():
        ref = params[name].grad
        assert prm.grad is not None, name
        if name.endswith("pe.bias") and cfg.get("epeg_type", "attn") == "attn":
            assert float(prm.grad.abs().max()) == 0.0 and float(ref.abs().max()) < 1e-6     # Identity 2
            continue
        rel(prm.grad.cpu().numpy(), ref.numpy().reshape(prm.shape), name)


def _masks(seed, N, cfg, p):
    from hip_util import dropout_keep
    D = cfg["mlp_dim"]
    H, _, _ = O.grid(N, cfg.get("region_num", 8))
    n_layers = cfg.get("n_layers", 2) - 1
    masks = {li: dropout_keep(seed, li, H * H, D, p) for li in range(n_layers)}
    masks["cr_msa"] = dropout_keep(seed, 100, cfg.get("crmsa_k", 3) * 64, D, p)
    return masks


def _all_grads_close(enc, xd, x_leaf, params, tol, top_floor=0.0):
    for name, got, ref in [("dx", xd.grad, x_leaf.grad)] + [(n_, p_.grad, params[n_].grad.reshape(p_.shape))
                                                            for n_, p_ in enc.named_parameters()
                                                            if not n_.endswith("pe.bias")]:
        ref = ref.numpy().astype(np.float64)
        err = np.abs(got.float().cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-6, top_floor)
        assert err <= tol, f"{name}: {err:.2e}"


def test_encoder_backward_head_dim_128_with_dropout():
    """train-mode proj_drop at head dim 128: the kernels' stateless masks rebuilt in numpy for the float64 oracle"""
    from hip_util import dev
    N, cfg, st, x, G = _case("d1024_h8_n3000")
    p, seed = 0.1, 0x1234_5678_9ABC_DEF
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True, drop=(p, _masks(seed, N, cfg, p)))
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = _encoder(st, cfg, drop_out=p)
    enc.drop_seed = seed
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    _cmp(y.detach().cpu().numpy(), y64.detach().numpy(), 2e-4, "train forward with dropout")
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    _all_grads_close(enc, xd, x_leaf, params, 2e-3)


@pytest.mark.parametrize("draws", [[1 / 0.7, 0.0], [0.0, 1 / 0.7]])
def test_encoder_backward_head_dim_128_with_drop_path(draws):
    """drop_path with pinned draws (and proj dropout) at head dim 128; a dropped R-MSA branch leaves zero gradients"""
    from hip_util import dev
    N, cfg, st, x, G = _case("h4_n9000")
    p, seed = 0.1, 0x0F1E_2D3C_4B5A
    branch = dict(zip([(0, "attn"), ("cr_msa", "attn")], draws))
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True, drop=(p, _masks(seed, N, cfg, p)), branch=branch)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = _encoder(st, cfg, drop_out=p, drop_path=0.3)
    enc.drop_seed, enc.drop_path_draws = seed, draws
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    _cmp(y.detach().cpu().numpy(), y64.detach().numpy(), 2e-4, "forward with drop_path")
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    top = max(float(v.grad.abs().max()) for v in params.values() if v.grad is not None)
    _all_grads_close(enc, xd, x_leaf, params, 2e-3, 1e-6 * top)
    if draws[0] == 0.0:
        assert float(enc.layers[0].attn.attn.qkv.weight.grad.abs().max()) == 0.0


def test_training_head_dim_128_under_autocast():
    """bf16 autocast training at head dim 128: gradients close to the fp32 oracle's, and visibly not the fp32 run"""
    from hip_util import dev
    N, cfg, st, x, G = _case("h4_n9000")
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = _encoder(st, cfg, drop_out=0.)
    xd = dev(x).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = enc(xd.unsqueeze(0)).squeeze(0)
    (y.float() * dev(G)).sum().backward()
    torch.cuda.synchronize()
    _all_grads_close(enc, xd, x_leaf, params, 3e-2)
    err = float((xd.grad.double().cpu() - x_leaf.grad).abs().max() / x_leaf.grad.abs().max())
    assert err > 1e-5


def test_encoder_backward_head_dims_reproducible():
    """the same training step twice at head dims 128 and 32: every gradient bit-identical"""
    from hip_util import dev
    for case in ("h4_n9000", "h16_n9000"):
        N, cfg, st, x, G = _case(case)
        enc = _encoder(st, cfg, drop_out=0.)
        grads = []
        for _ in range(2):
            enc.zero_grad(set_to_none=True)
            xd = dev(x).requires_grad_(True)
            (enc(xd.unsqueeze(0)).squeeze(0) * dev(G)).sum().backward()
            torch.cuda.synchronize()
            grads.append([xd.grad.cpu()] + [p_.grad.cpu() for _, p_ in enc.named_parameters()])
        for a, b in zip(*grads):
            assert torch.equal(a, b), case


def test_rrtmil_n_heads_4_trains():
    """RRTMIL(n_heads=4).train(): a step gives finite gradients for exactly the parameters that get one at n_heads=8"""
    from rrt_mil_amd import RRTMIL
    dev_ = torch.device("cuda:0")
    x = torch.from_numpy(synth.bag(9000, 1024, tag="trainhd/mil")).unsqueeze(0).to(dev_)
    with_grad = {}
    for heads in (8, 4):
        torch.manual_seed(11)
        mil = RRTMIL(input_dim=1024, n_classes=2, n_heads=heads).to(dev_).train()
        loss = torch.nn.functional.cross_entropy(mil(x), torch.tensor([1], device=dev_))
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        with_grad[heads] = {n for n, p_ in mil.named_parameters() if p_.grad is not None}
        for n in with_grad[heads]:
            assert torch.isfinite(dict(mil.named_parameters())[n].grad).all(), n
    assert with_grad[4] == with_grad[8] and any(".qkv." in n for n in with_grad[4])


def test_training_limits_still_raise():
    """outside the envelope: head dim 8, head dim 512 with EPEG, dim > 1024"""
    from rrt_mil_amd import RRTEncoder
    x = torch.randn(1, 9000, 64, device="cuda:0", requires_grad=True)
    with pytest.raises(NotImplementedError):
        RRTEncoder(mlp_dim=64, drop_out=0.).to("cuda:0").train()(x)                   # head dim 8, P = 144
    x = torch.randn(1, 9000, 512, device="cuda:0", requires_grad=True)
    with pytest.raises(NotImplementedError):
        RRTEncoder(mlp_dim=512, n_heads=1, drop_out=0.).to("cuda:0").train()(x)       # head dim 512 with EPEG
    with pytest.raises(NotImplementedError):
        RRTEncoder(mlp_dim=2048, n_heads=32, crmsa_heads=32).to("cuda:0").train()(torch.randn(1, 64, 2048, device="cuda:0"))
