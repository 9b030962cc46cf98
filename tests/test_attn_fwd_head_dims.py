"""GPU (-m gpu): the matrix-core region attention forward at head dims 16 .. 256 (multiples of 16) other than 64 -- the
stage entry rrt_region_attention_hd_f32 against the explicit float64 formulation, the online-softmax rescale, the
dispatcher's routing, the encoder in eval() against the float64 oracle (fp32, bf16 autocast, forward_bags), and a training
step on top of the new forward."""
import numpy as np
import pytest
import torch

from conftest import STATE_KEYS
from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth

pytestmark = pytest.mark.gpu

CANARY_ROWS = 64
CANARY = -777.25


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()


def _cmp(got, ref, tol, what):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
    print(f"{what}: max-abs {err:.3e} (bound {tol:.1e})")
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= tol, f"{what}: max-abs {err:.3e} > {tol:.1e}"
    return err


# ------------------------------------------------------------------ the stage
HDS = [16, 32, 48, 96, 128, 192, 256]
PS = [1, 4, 7, 49, 129, 144, 177, 256, 484]
EKS = [9, 21, 31, 63]


def _stage_cases():
    """the grid of test_train_head_dims.py: every (head dim, P) with epeg_k 0, 15 and one of 9 / 21 / 31 / 63 in turn
    (31, wider than the region, at P = 4)"""
    out = []
    for a, hd in enumerate(HDS):
        for b, P in enumerate(PS):
            third = 31 if P == 4 else EKS[(a + b) % len(EKS)]
            out += [(hd, P, ek) for ek in (0, 15, third)]
    return out


def _heads(hd):
    return 3 if hd <= 96 else 2


def _stage_inputs(R, P, D, heads, ek):
    """as test_train_head_dims.py::_stage_inputs: qkv normal x 0.6, taps uniform / sqrt(k), a conv bias for the reference;
    the stage gets q already scaled"""
    hd = D // heads
    raw = synth.normal(f"abh/qkv{R}x{P}x{D}", (R * P, 3 * D)) * 0.6
    pe = synth.uniform(f"abh/pe{heads}x{ek}", (heads, max(ek, 1)), -1, 1) / np.sqrt(max(ek, 1))
    pb = synth.uniform(f"abh/pb{heads}", (heads,), -0.3, 0.3)
    stash = raw.copy()
    stash[:, :D] *= hd ** -0.5
    return raw, pe, pb, stash


def _ref64(raw, pe, pb, R, P, D, heads, ek):
    """scores [P, P], a depth-wise conv along the query axis WITH a bias, softmax, A V -- float64"""
    hd = D // heads
    t = torch.tensor(raw, dtype=torch.float64).reshape(R, P, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * hd ** -0.5, t[1], t[2]
    S = q @ k.transpose(-2, -1)
    if ek:
        S = S + torch.nn.functional.conv2d(S, torch.tensor(pe, dtype=torch.float64).reshape(heads, 1, ek, 1),
                                           torch.tensor(pb, dtype=torch.float64), padding=(ek // 2, 0), groups=heads)
    return (S.softmax(-1) @ v).transpose(1, 2).reshape(R * P, D).numpy()


def _run_stage(entry, qkv, pe, R, P, D, heads, ek):
    """one stage call into a NaN-filled o with canary rows behind it; returns (o, canary rows) as numpy"""
    from hip_util import DEV, p, stream
    lib = _lib.load()
    buf = torch.full((R * P + CANARY_ROWS, D), float("nan"), device=DEV)
    buf[R * P:] = CANARY
    _lib.check(getattr(lib, entry)(p(qkv), p(pe) if ek else None, p(buf), R, P, D, heads, ek, stream()), entry)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return out[:R * P], out[R * P:]


@pytest.mark.parametrize("hd,P,ek", _stage_cases())
def test_region_attention_hd_stage(hd, P, ek):
    """rrt_region_attention_hd_f32 against the explicit float64 formulation: max-abs <= 5e-5 (the bound the project holds
    the forward stage to on these inputs), every row written, the canary rows past n_regions * P untouched"""
    from hip_util import dev
    R, heads = (2 if P > 200 else 3), _heads(hd)
    D = hd * heads
    raw, pe, pb, stash = _stage_inputs(R, P, D, heads, ek)
    got, canary = _run_stage("rrt_region_attention_hd_f32", dev(stash), dev(pe), R, P, D, heads, ek)
    assert np.all(canary == CANARY), "rows past n_regions * P were written"
    _cmp(got, _ref64(raw, pe, pb, R, P, D, heads, ek), 5e-5, f"hd{hd} P{P} k{ek}")


@pytest.mark.parametrize("hd", [32, 128])
def test_region_attention_hd_online_softmax_rescale(hd):
    """the construction of test_hip_parity.py::test_region_attention_online_softmax_rescale at head dims 32 and 128: the
    largest score of some queries sits in the last key run / chunk, of others in the first"""
    from hip_util import dev
    R, P, D = 2, 144, 512
    heads = D // hd
    qkv = synth.normal("att/spike", (R * P, 3 * D)) * 0.3
    qkv[:, :D] *= hd ** -0.5
    qkv[P - 3, D:2 * D] *= 25.0          # key P-3 of region 0 dominates (last run)
    qkv[P + 5, D:2 * D] *= 25.0          # key 5 of region 1 dominates (first run)
    got, canary = _run_stage("rrt_region_attention_hd_f32", dev(qkv), None, R, P, D, heads, 0)
    t = qkv.astype(np.float64).reshape(R, P, 3, heads, hd).transpose(2, 0, 3, 1, 4)
    S = t[0] @ t[1].transpose(0, 1, 3, 2)
    A = np.exp(S - S.max(-1, keepdims=True))
    A /= A.sum(-1, keepdims=True)
    ref = (A @ t[2]).transpose(0, 2, 1, 3).reshape(R * P, D)
    assert np.all(canary == CANARY)
    _cmp(got, ref, 3e-5, f"online softmax rescale hd{hd}")


@pytest.mark.parametrize("hd,P,ek", [(16, 7, 15), (32, 144, 15), (48, 129, 9), (96, 484, 63), (128, 144, 0),
                                     (128, 177, 15), (192, 4, 31), (256, 256, 21)])
def test_dispatch_routes_to_the_hd_kernel(hd, P, ek):
    """rrt_region_attention_f32 and rrt_region_attention_hd_f32 give bit-identical o (the dispatcher routes there), and
    two calls of either are bit-identical (fixed-order sums, no atomics)"""
    from hip_util import dev
    R, heads = 3, _heads(hd)
    D = hd * heads
    _, pe, _, stash = _stage_inputs(R, P, D, heads, ek)
    d_q, d_pe = dev(stash), dev(pe)
    a1, _ = _run_stage("rrt_region_attention_hd_f32", d_q, d_pe, R, P, D, heads, ek)
    a2, _ = _run_stage("rrt_region_attention_hd_f32", d_q, d_pe, R, P, D, heads, ek)
    b1, c1 = _run_stage("rrt_region_attention_f32", d_q, d_pe, R, P, D, heads, ek)
    b2, _ = _run_stage("rrt_region_attention_f32", d_q, d_pe, R, P, D, heads, ek)
    assert np.isfinite(a1).all() and np.all(c1 == CANARY)
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
    assert np.array_equal(a1, b1), "the dispatcher did not take the head-dim kernel"


# ------------------------------------------------------------------ the encoder in eval()
CFGS = {
    "d512_h2": dict(mlp_dim=512, n_heads=2, epeg_k=15, crmsa_k=3),                    # head dim 256
    "d512_h4": dict(mlp_dim=512, n_heads=4, epeg_k=15, crmsa_k=3),                    # 128
    "d512_h16": dict(mlp_dim=512, n_heads=16, epeg_k=15, crmsa_k=3),                  # 32
    "d1024_h8": dict(mlp_dim=1024, n_heads=8, epeg_k=15, crmsa_k=3),                  # 128, CR-MSA's inner attention too
    "d256_h8": dict(mlp_dim=256, n_heads=8, epeg_k=15, crmsa_k=3),                    # 32, CR-MSA's inner attention too
    "d512_h4_rn16": dict(mlp_dim=512, n_heads=4, epeg_k=15, crmsa_k=3, region_num=16),
    "d512_h4_noepeg": dict(mlp_dim=512, n_heads=4, epeg=False, crmsa_k=3),
}
ENC_CASES = [(c, n) for c in ("d512_h2", "d512_h4", "d512_h16", "d1024_h8", "d256_h8") for n in (50, 3000, 9000)] + \
            [("d512_h4_rn16", 30000), ("d512_h4_noepeg", 9000)]


def _state(cfg):
    return synth.encoder_state(**{k: v for k, v in cfg.items() if k in STATE_KEYS})


@pytest.mark.parametrize("name,N", ENC_CASES)
def test_encoder_eval_head_dims(name, N):
    """eval() under no_grad against the float64 oracle on the reference's own state_dict keys: max-abs <= 2e-4"""
    from hip_util import dev, encoder_from_state
    cfg = CFGS[name]
    st = _state(cfg)
    x = synth.bag(N, cfg["mlp_dim"], tag=f"fwdhd/{name}/{N}")
    enc = encoder_from_state(st, cfg)
    with torch.no_grad():
        y = enc(dev(x).unsqueeze(0)).squeeze(0)
    torch.cuda.synchronize()
    _cmp(y.cpu().numpy(), O.forward_f64(x, st, cfg), 2e-4, f"{name} N={N}")


def test_encoder_eval_head_dim_128_under_autocast():
    """bf16 autocast at head dim 128 (16-bit projections, the attention stays fp32 on the new kernel) against the oracle's
    restatement of those rounding points: within 3e-2 of the largest output entry, the bound of
    test_train_head_dims.py::test_training_head_dim_128_under_autocast; and visibly not the fp32 result"""
    from hip_util import dev, encoder_from_state
    cfg, N = CFGS["d512_h4"], 9000
    st = _state(cfg)
    x = synth.bag(N, 512, tag="fwdhd/amp")
    enc = encoder_from_state(st, cfg)
    with torch.no_grad():
        y32 = enc(dev(x).unsqueeze(0)).squeeze(0)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = enc(dev(x).unsqueeze(0)).squeeze(0)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and torch.isfinite(y).all()
    ref = O.forward_f64(x, st, cfg, lowp=O.LowP("bf16", attn=False))
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"autocast bf16 h4 N=9000: {err:.3e} of the largest entry (bound 3.0e-02)")
    assert err <= 3e-2
    assert float((y - y32).abs().max()) > 1e-6


def test_forward_bags_head_dim_128_equals_bag_by_bag():
    """forward_bags on a mixed list of four bag sizes at n_heads = 4 == enc(bag) one at a time, bit for bit"""
    from hip_util import dev, encoder_from_state
    cfg = CFGS["d512_h4"]
    enc = encoder_from_state(_state(cfg), cfg)
    sizes = [3000, 9000, 50, 15000]
    bags = [dev(synth.bag(n, 512, tag=f"fwdhd/exec/{i}")) for i, n in enumerate(sizes)]
    with torch.no_grad():
        enc.solo = False
        ref = [enc(b.unsqueeze(0)).squeeze(0).clone() for b in bags]
        outs = enc.forward_bags(bags, streams=4)
    torch.cuda.synchronize()
    for i, n in enumerate(sizes):
        assert outs[i].shape == (n, 512) and torch.isfinite(outs[i]).all()
        assert torch.equal(outs[i], ref[i]), f"bag {i} (N={n}) differs from the one-at-a-time forward"


# ------------------------------------------------------------------ training on top of the new forward
@pytest.mark.parametrize("name", ["d512_h4", "d512_h16"])
def test_training_step_on_the_new_forward(name):
    """one training step at n_heads = 4 and 16: y within 2e-4 of the float64 oracle and every gradient within 2e-3 of the
    largest gradient entry (the bounds of test_train_head_dims.py::test_encoder_backward_head_dims)"""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTEncoder
    cfg, N = CFGS[name], 9000
    st = _state(cfg)
    x = synth.bag(N, 512, tag="fwdhd/train/" + name)
    G = synth.normal("fwdhd/G/" + name, (N, 512))
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = RRTEncoder(drop_out=0., **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    _cmp(y.detach().cpu().numpy(), y64.detach().numpy(), 2e-4, name + " train forward")
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    floor = 1e-3 * max([float(x_leaf.grad.abs().max())] + [float(v.grad.abs().max()) for v in params.values()
                                                           if v.grad is not None])

    def rel(got, ref, what):
        ref = ref.astype(np.float64)
        err = np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), floor, 1e-6)
        assert np.isfinite(got).all(), what
        assert err <= 2e-3, f"{name} {what}: max error {err:.2e} of the largest gradient entry"

    rel(xd.grad.cpu().numpy(), x_leaf.grad.numpy(), "dx")
    for pname, prm in enc.named_parameters():
        ref = params[pname].grad
        assert prm.grad is not None, pname
        if pname.endswith("pe.bias"):
            assert float(prm.grad.abs().max()) == 0.0 and float(ref.abs().max()) < 1e-6     # Identity 2
            continue
        rel(prm.grad.cpu().numpy(), ref.numpy().reshape(prm.shape), pname)
