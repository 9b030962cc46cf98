"""GPU (-m gpu): the HIP path, called through the C ABI, against the oracle
(oracle/rrt_oracle.py, float64 truth) and the golden vectors from the real reference.

Tolerances: BASELINE.json asks for <= 1e-3 max-abs (fp32) on the encoder output.
The kernels compute in exact fp32 (f32 MFMA), so the tests hold them to 2e-4 end to
end and ~1e-5 relative per stage; see DESIGN.md for the error budget.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden, synth_case
from conftest import STATE_KEYS as _STATE_KEYS
from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth

pytestmark = pytest.mark.gpu

TOL_E2E = 2e-4      # max-abs on LayerNorm-ed outputs (|y| ~ O(1)); north star allows 1e-3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()   # fails loudly if librrt_hip.so is not built


@pytest.fixture(autouse=True)
def _inference_runs_without_a_graph(request):
    """The reference's validation loops run under torch.no_grad() (main.py val loop); with gradients enabled a forward
    records a graph (eval() too) and takes the training kernels.  Inference tests therefore run under no_grad; the
    tests of the backward (names with backward / train / gradients / learns) keep gradients on."""
    name = request.node.name
    grad = any(k in name for k in ("backward", "train", "gradients", "learns"))
    with torch.set_grad_enabled(grad):
        yield


def _cmp(got, ref, tol, what):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= tol, f"{what}: max-abs {err:.3e} > {tol:.1e}"
    return err


# ------------------------------------------------------------------ stages
@pytest.mark.parametrize("L,rn,D", [(300, 8, 64), (9000, 8, 512), (50, 8, 512), (4096, 8, 512),
                                    (1000, 4, 1024), (30000, 16, 512), (777, 8, 96)])
def test_ln_partition(L, rn, D):
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    x = synth.bag(L, D, tag="lnp")
    gm = 1.0 + synth.uniform("lnp/g", (D,), -0.3, 0.3)
    bt = synth.uniform("lnp/b", (D,), -0.2, 0.2)
    g = _lib.region_grid(L, rn)
    u = torch.full((g.H * g.H, D), float("nan"), device=DEV)
    d_x, d_gm, d_bt = dev(x), dev(gm), dev(bt)      # keep alive: raw pointers cross the C ABI
    _lib.check(lib.rrt_ln_partition_f32(p(d_x), p(d_gm), p(d_bt), p(u), L, D, C.byref(g), stream()), "lnp")
    torch.cuda.synchronize()
    x64 = x.astype(np.float64)
    mu = x64.mean(-1, keepdims=True)
    ref = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * gm + bt
    ref = np.concatenate([ref, np.zeros((g.add, D))], 0)[O.partition_index(g.H, g.s)]
    got = u.cpu().numpy()
    _cmp(got, ref, 5e-6, "ln_partition")
    # pad rows are exact zeros
    pad_slots = np.nonzero(O.partition_index(g.H, g.s) >= L)[0]
    assert (got[pad_slots] == 0).all()


@pytest.mark.parametrize("M,N,K", [(9216, 1536, 512), (9216, 512, 512), (192, 1536, 512), (192, 512, 512),
                                   (100, 192, 64), (64, 64, 64), (1000, 130, 96), (129, 257, 32),
                                   (30976, 1536, 512)])
def test_linear(M, N, K):
    from hip_util import dev, linear
    A = synth.normal(f"lin/A{M}x{K}", (M, K))
    B = synth.uniform(f"lin/B{N}x{K}", (N, K), -1, 1) / np.sqrt(K)
    bias = synth.uniform(f"lin/b{N}", (N,), -0.5, 0.5)
    q_cols = N // 3
    dA, dB, db = dev(A), dev(B), dev(bias)
    got = linear(dA, dB, db, q_cols, 0.125).cpu().numpy()
    ref = A.astype(np.float64) @ B.astype(np.float64).T + bias
    ref[:, :q_cols] *= 0.125
    _cmp(got, ref, 2e-5, f"linear {M}x{N}x{K}")          # fp32 fma chain over K: ~1e-6 observed
    got2 = linear(dA, dB, None).cpu().numpy()
    _cmp(got2, A.astype(np.float64) @ B.astype(np.float64).T, 2e-5, "linear no-bias")


def test_linear_transpose_detecting():
    """A = I-like with asymmetric B catches operand / C-layout swaps (HIP guide rule 16)."""
    from hip_util import dev, linear
    M = N = K = 128
    A = np.eye(M, K, dtype=np.float32)
    B = (np.arange(N * K, dtype=np.float32).reshape(N, K) % 251) / 251.0
    dA, dB = dev(A), dev(B)
    got = linear(dA, dB).cpu().numpy()
    assert np.array_equal(got, B.T)


# 5000 .. 15000: one bag size per branch of the out-projection's tile-shape rule (linear_f32.hip::choose, round 3: 64-row tiles
# single round / 128-row / 96-row four per CU / 144-row / 64-row in rounds), each with a ragged last row tile
@pytest.mark.parametrize("L,rn", [(9000, 8), (300, 8), (30000, 16), (50, 8), (5000, 8), (7000, 8), (10500, 8), (12000, 8), (13000, 8),
                                  (15000, 8)])
def test_linear_unpartition_residual(L, rn):
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    D = 64 if L == 300 else 512
    g = _lib.region_grid(L, rn)
    Np = g.H * g.H
    A = synth.normal("unp/A", (Np, D))
    B = synth.uniform("unp/B", (D, D), -1, 1) / np.sqrt(D)
    bias = synth.uniform("unp/b", (D,), -0.5, 0.5)
    res = synth.normal("unp/r", (L, D))
    out = torch.full((L, D), float("nan"), device=DEV)
    dA, dB, db, dr = dev(A), dev(B), dev(bias), dev(res)
    _lib.check(lib.rrt_linear_unpartition_residual_f32(p(dA), p(dB), p(db), p(dr), p(out),
                                                       D, D, C.byref(g), 0, stream()), "unpart")
    torch.cuda.synchronize()
    Z = A.astype(np.float64) @ B.astype(np.float64).T + bias
    z = np.empty((Np, D))
    z[O.partition_index(g.H, g.s)] = Z
    _cmp(out.cpu().numpy(), res + z[:L], 2e-5, "linear_unpartition_residual")


def _attn_ref(qkv, pe_w, R, P, D, heads, epeg_k):
    """float64 restatement of rmsa.py:103-122 WITH the explicit [P,P] EPEG stencil."""
    hd = D // heads
    t = qkv.astype(np.float64).reshape(R, P, 3, heads, hd).transpose(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    S = q @ k.transpose(0, 1, 3, 2)
    if epeg_k:
        half = epeg_k // 2
        Sp = np.pad(S, ((0, 0), (0, 0), (half, half), (0, 0)))
        E = np.zeros_like(S)
        for tt in range(epeg_k):
            E += pe_w.astype(np.float64)[None, :, tt, None, None] * Sp[:, :, tt:tt + P, :]
        S = S + E + 0.37      # arbitrary per-head-constant bias: must not change the result
    S = S - S.max(-1, keepdims=True)
    A = np.exp(S)
    A /= A.sum(-1, keepdims=True)
    return (A @ v).transpose(0, 2, 1, 3).reshape(R * P, D)


@pytest.mark.parametrize("R,P,D,heads,ek", [(64, 144, 512, 8, 15), (8, 121, 512, 8, 15), (4, 256, 512, 8, 21),
                                            (3, 64, 512, 8, 0), (64, 9, 512, 8, 15), (64, 1, 512, 8, 15),
                                            (2, 49, 512, 8, 9), (2, 484, 512, 8, 15), (5, 100, 128, 2, 15),
                                            (3, 64, 512, 1, 0), (64, 9, 64, 8, 15), (2, 37, 96, 3, 5), (5, 64, 128, 2, 0)])
def test_region_attention(R, P, D, heads, ek):
    from hip_util import dev, region_attention
    qkv = synth.normal(f"att/{R}x{P}x{D}", (R * P, 3 * D)) * 0.7
    qkv[:, :D] *= (D // heads) ** -0.5
    pe = synth.uniform("att/pe", (heads, max(ek, 1)), -1, 1) / np.sqrt(max(ek, 1))
    d_qkv, d_pe = dev(qkv), dev(pe)
    got = region_attention(d_qkv, d_pe if ek else None, R, P, D, heads, ek).cpu().numpy()
    ref = _attn_ref(qkv, pe, R, P, D, heads, ek)
    _cmp(got, ref, 3e-5, f"region_attention R{R} P{P} D{D} h{heads} k{ek}")


def test_region_attention_online_softmax_rescale():
    """Force the online-softmax rescale branch: the largest score of some queries sits in the
    LAST key chunk (HIP guide rule 26)."""
    from hip_util import dev, region_attention
    R, P, D, heads = 2, 144, 512, 8
    qkv = synth.normal("att/spike", (R * P, 3 * D)) * 0.3
    qkv[:, :D] *= 0.125
    qkv[P - 3, D:2 * D] *= 25.0          # key P-3 of region 0 dominates (chunk 2 of 3)
    qkv[P + 5, D:2 * D] *= 25.0          # key 5 of region 1 dominates (chunk 0)
    d_qkv = dev(qkv)
    got = region_attention(d_qkv, None, R, P, D, heads, 0).cpu().numpy()
    _cmp(got, _attn_ref(qkv, None, R, P, D, heads, 0), 3e-5, "online softmax rescale")


@pytest.mark.parametrize("L,D,k", [(9000, 512, 3), (300, 64, 3), (3000, 512, 5), (50, 512, 1), (9000, 512, 8)])
def test_crmsa_stages(L, D, k):
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    g8 = _lib.region_grid(L, 8)
    Np8, R8, P8 = g8.H * g8.H, 64, g8.s * g8.s
    x1 = synth.normal("cr/x1", (L, D)) * 1.3 + 0.2
    x0 = synth.normal("cr/x0", (L, D))
    gm = 1.0 + synth.uniform("cr/g", (D,), -0.3, 0.3)
    bt = synth.uniform("cr/b", (D,), -0.2, 0.2)
    phi = synth.uniform("cr/phi", (D, k), -1, 1) * (3.0 / np.sqrt(D))
    rep2 = synth.normal("cr/rep2", (k, R8, D))
    gm3 = 1.0 + synth.uniform("cr/g3", (D,), -0.3, 0.3)
    bt3 = synth.uniform("cr/b3", (D,), -0.2, 0.2)
    d_x1, d_gm, d_bt = dev(x1), dev(gm), dev(bt)
    d_phi, d_x0, d_rep2, d_gm3, d_bt3 = dev(phi), dev(x0), dev(rep2), dev(gm3), dev(bt3)
    mr = torch.full((L, 2), float("nan"), device=DEV)
    lg = torch.full((Np8, k), float("nan"), device=DEV)
    wd = torch.full((Np8, k), float("nan"), device=DEV)
    rep = torch.full((k, R8, D), float("nan"), device=DEV)
    y = torch.full((L, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_crmsa_logits_f32(p(d_x1), p(d_gm), p(d_bt), p(d_phi), p(mr), p(lg), L, D, k,
                                        C.byref(g8), stream()), "logits")
    _lib.check(lib.rrt_crmsa_combine_f32(p(d_x1), p(d_gm), p(d_bt), p(mr), p(lg), p(wd), p(rep), L, D, k,
                                         C.byref(g8), stream()), "combine")
    _lib.check(lib.rrt_crmsa_dispatch_ln_f32(p(d_x1), p(d_x0), p(wd), p(d_rep2), p(d_gm3),
                                             p(d_bt3), p(y), L, D, k, C.byref(g8), stream()), "dispatch")
    torch.cuda.synchronize()
    # float64 restatement of rmsa.py:303-335
    x64 = x1.astype(np.float64)
    mu = x64.mean(-1, keepdims=True)
    v = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * gm + bt
    perm = O.partition_index(g8.H, g8.s)
    V = np.concatenate([v, np.zeros((g8.add, D))], 0)[perm].reshape(R8, P8, D)
    Lg = (V @ phi.astype(np.float64)).transpose(0, 2, 1)
    _cmp(lg.cpu().numpy().reshape(R8, P8, k).transpose(0, 2, 1), Lg, 2e-5, "crmsa logits")
    Cw = np.exp(Lg - Lg.max(-1, keepdims=True))
    Cw /= Cw.sum(-1, keepdims=True)
    _cmp(rep.cpu().numpy(), (Cw @ V).transpose(1, 0, 2), 2e-5, "crmsa combine")
    Dw = np.exp(Lg - Lg.max(1, keepdims=True))
    Dw /= Dw.sum(1, keepdims=True)
    mn, mx = Lg.min(-1, keepdims=True), Lg.max(-1, keepdims=True)
    Mm = (Lg - mn) / (mx - mn + 1e-8)
    _cmp(wd.cpu().numpy().reshape(R8, P8, k).transpose(0, 2, 1), Mm * Dw, 2e-5, "crmsa dispatch weights")
    out = np.einsum("rnp,nrd->rpd", Mm * Dw, rep2.astype(np.float64))
    z = np.empty((Np8, D))
    z[perm] = out.reshape(-1, D)
    x2 = x64 + z[:L] + x0
    mu = x2.mean(-1, keepdims=True)
    ref = (x2 - mu) / np.sqrt(((x2 - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * gm3 + bt3
    _cmp(y.cpu().numpy(), ref, 2e-5, "crmsa dispatch + LN")


@pytest.mark.gpu
@pytest.mark.parametrize("L,k", [(9000, 3), (9000, 1), (7000, 2), (3000, 3), (50, 3), (8100, 3),
                                 (9000, 5), (3000, 8), (13000, 5), (15000, 5), (15000, 3), (30000, 3), (30000, 8), (36000, 4),
                                 (10500, 1), (12000, 3), (20000, 5), (27000, 2), (1100, 3)])
def test_crmsa_region_kernel_matches_logits_plus_combine(L, k):
    """logits + combine in one pass (crmsa_region_kernel) against the two-kernel form on the same inputs: the LayerNorm
    statistics are the same arithmetic (bit-identical); since round 6 the two-kernel form at dim 512 takes the logits in the
    centered form rstd * sum (x - mean) gamma phi + B_n (crmsa_logits512_kernel), a few ulp from LN(x) . phi; the
    representatives differ by summation order."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    D = 512
    g8 = _lib.region_grid(L, 8)
    Np8, R8 = g8.H * g8.H, 64
    x1 = synth.normal("crr/x1", (L, D)) * 1.3 + 0.2
    gm = 1.0 + synth.uniform("crr/g", (D,), -0.3, 0.3)
    bt = synth.uniform("crr/b", (D,), -0.2, 0.2)
    phi = synth.uniform("crr/phi", (D, k), -1, 1) * (3.0 / np.sqrt(D))
    d_x1, d_gm, d_bt, d_phi = dev(x1), dev(gm), dev(bt), dev(phi)
    out = {}
    scratch = torch.full((256 + 64 * 16 * 8 * 520 * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    P8 = g8.s * g8.s
    tags = (("two",) + (("one",) if k <= 3 and P8 <= 144 else ()) + (("four", "four again") if 4 <= P8 <= 576 else ())
            + (("stream", "stream again") if 16 <= P8 <= 576 else ()))      # round 6: four STREAMING blocks per region
    for tag in tags:
        mr = torch.full((L, 2), float("nan"), device=DEV)
        lg = torch.full((Np8, k), float("nan"), device=DEV)
        wd = torch.full((Np8, k), float("nan"), device=DEV)
        rep = torch.full((k, R8, D), float("nan"), device=DEV)
        if tag == "two":
            _lib.check(lib.rrt_crmsa_logits_f32(p(d_x1), p(d_gm), p(d_bt), p(d_phi), p(mr), p(lg), L, D, k, C.byref(g8), stream()), "logits")
            _lib.check(lib.rrt_crmsa_combine_f32(p(d_x1), p(d_gm), p(d_bt), p(mr), p(lg), p(wd), p(rep), L, D, k, C.byref(g8), stream()), "combine")
        elif tag == "one":
            _lib.check(lib.rrt_crmsa_region_f32(p(d_x1), p(d_gm), p(d_bt), p(d_phi), p(mr), p(lg), p(wd), p(rep), L, D, k, C.byref(g8), stream()), "region")
        elif tag.startswith("stream"):          # crmsa_stream4_kernel: what the forward uses above 144 tokens per region
            _lib.check(lib.rrt_crmsa_stream4_f32(p(d_x1), p(d_gm), p(d_bt), p(d_phi), p(mr), p(lg), p(wd), p(rep), L, D, k, C.byref(g8),
                                                 p(scratch), scratch.numel(), stream()), "stream4")
        else:                                   # four blocks per region, the last arrival merges (twice: counters left at 0)
            _lib.check(lib.rrt_crmsa_region4_f32(p(d_x1), p(d_gm), p(d_bt), p(d_phi), p(mr), p(lg), p(wd), p(rep), L, D, k, C.byref(g8),
                                                 p(scratch), scratch.numel(), stream()), "region4")
        torch.cuda.synchronize()
        out[tag] = [t.cpu().numpy() for t in (mr, lg, wd, rep)]
    for tag in tags[1:]:
        # the one-pass kernels take their wave totals in groups of four since round 6 (wave_sum4: crmsa_stream4, crmsa_region4 for
        # k = 1, 3, 5, crmsa_region for k <= 3): another summation order than the two-pass form's, the last bits differ
        assert np.allclose(out[tag][0], out["two"][0], rtol=2e-6, atol=2e-6, equal_nan=True), f"{tag}: mean / rstd"
        assert np.array_equal(np.isnan(out[tag][1]), np.isnan(out["two"][1])), f"{tag}: logits"
        dl = np.abs(np.nan_to_num(out[tag][1]) - np.nan_to_num(out["two"][1]))
        assert dl.max() <= 4e-6 * max(1.0, np.abs(np.nan_to_num(out["two"][1])).max()), (tag, "logits", dl.max())
        dw = np.abs(np.nan_to_num(out[tag][2]) - np.nan_to_num(out["two"][2]))
        assert np.array_equal(np.isnan(out[tag][2]), np.isnan(out["two"][2])) and dw.max() <= 2e-5, (tag, "dispatch weights", dw.max())
        d = np.abs(out[tag][3].astype(np.float64) - out["two"][3])
        assert np.isfinite(out[tag][3]).all() and d.max() <= 3e-6 * max(1.0, np.abs(out["two"][3]).max()), (tag, d.max())
    if "four" in out:
        assert np.array_equal(out["four"][3], out["four again"][3])
    if "stream" in out:
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out["stream"], out["stream again"]))


# ------------------------------------------------------------------ whole path
SMALL = [n for n in golden_names("G") if not n.startswith(("G0", "G7", "G8", "G11", "G13", "G15", "G16", "G20")) and "mlp" not in n]
# crmsa_mlp needs dim % 128 == 0 on the HIP path (hidden = dim/4 is a GEMM K): D=64 golden is out of range


@pytest.mark.parametrize("name", SMALL)
def test_encoder_matches_reference_golden(name):
    """End to end against the REAL reference's outputs (tests/golden, tools/make_golden.py)."""
    from hip_util import run_encoder
    g = load_golden(name)
    x, st, cfg = synth_case(g)
    y = run_encoder(x, st, cfg)
    assert y.shape == x.shape
    if "y" in g:
        _cmp(y, g["y"], TOL_E2E, name)
    else:
        _cmp(y[g["rows"]], g["y_rows"], TOL_E2E, name)
        s = np.array([y.astype(np.float64).sum(), np.abs(y.astype(np.float64)).sum()])
        assert np.allclose(s, g["y_sums"][:2], rtol=1e-5, atol=N_ATOL(int(g["n"])))


def N_ATOL(n):
    return 1e-6 * n * 512     # checksum slack: ~1e-6 per element


@pytest.mark.parametrize("name", ["G1_d64_n300", "G2_d512_n512", "G6_d64_n700_heads1", "G5_d512_n3000_k21_c5"])
def test_encoder_matches_oracle_f64(name):
    from hip_util import run_encoder
    g = load_golden(name)
    x, st, cfg = synth_case(g)
    y = run_encoder(x, st, cfg)
    _cmp(y, O.forward_f64(x, st, cfg), 5e-5, name + " vs f64 oracle")


def test_crmsa_mlp_small_dim():
    """crmsa_mlp at a width whose hidden layer (dim / 4 = 16) is not a GEMM K tile: round 3 runs it (rounds 1-2 raised)"""
    from hip_util import run_encoder
    g = load_golden("G6_d64_n700_mlp")
    x, st, cfg = synth_case(g)
    y = run_encoder(x, st, cfg)
    _cmp(y, g["y"], TOL_E2E, "G6_d64_n700_mlp")
    _cmp(y, O.forward_f64(x, st, cfg), 5e-5, "G6_d64_n700_mlp vs f64 oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_names("G20"))
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encoder_batch_gt_1_matches_reference(name, mode):
    """(B, N, D) input with B = 2 / 3 (modules/rrt.py:165-202): the reference couples the bags of a batch inside CR-MSA
    (its inner attention runs over the representatives of all bags, rmsa.py:316-322).  rrt_encoder_forward_batch_f32
    against the reference's own outputs (G20, tools/make_golden_batch.py); bf16: the autocast-class bound."""
    from hip_util import encoder_from_state, dev
    from rrt_mil_amd import synth as sy
    g = load_golden(name)
    cfg, N, B = g["cfg"], int(g["n"]), int(g["b"])
    st = sy.encoder_state(**{k: v for k, v in cfg.items() if k in _STATE_KEYS})
    x = np.stack([sy.bag(N, 512, tag=f"batch/b{b}") for b in range(B)])
    enc = encoder_from_state(st, cfg)
    if mode == "bf16":
        enc.compute_dtype = torch.bfloat16
    xd = dev(x)
    y = enc(xd)
    torch.cuda.synchronize()
    assert y.shape == xd.shape
    got = y.cpu().numpy().astype(np.float64)
    err = np.abs(got[:, g["rows"]] - g["y_rows"]).max()
    assert np.isfinite(got).all() and err <= (2e-4 if mode == "f32" else 6e-2), err
    if mode == "f32":
        for b in range(B):
            s_ = np.array([got[b].sum(), np.abs(got[b]).sum()])
            assert np.allclose(s_, g["y_sums"][b][:2], rtol=1e-5, atol=N_ATOL(N))
        # the coupling is real: bag 0 alone gives something else, by what the reference recorded
        y0 = enc(xd[:1])
        torch.cuda.synchronize()
        assert abs(float((y0[0] - y[0]).abs().max()) - float(g["coupling"])) <= 2e-4
        # a batch of one is the single-bag path
        assert torch.equal(enc(xd[1:2])[0], enc(xd[1]))


@pytest.mark.parametrize("name", ["G7_d512_n2000_mlp", "G7_d128_n700_mlp"])
def test_crmsa_mlp(name):
    """MLP phi (crmsa_mlp=True, NSCLC-PLIP config): vs the reference golden and the f64 oracle."""
    from hip_util import run_encoder
    g = load_golden(name)
    x, st, cfg = synth_case(g)
    y = run_encoder(x, st, cfg)
    _cmp(y[g["rows"]], g["y_rows"], TOL_E2E, name)
    _cmp(y, O.forward_f64(x, st, cfg), 5e-5, name + " vs f64 oracle")


def test_input_ranks_and_purity():
    """(N,D), (1,N,D), (1,C,H,W) -> same rank/shape; input untouched (rrt.py:166-175, :197-201)."""
    from hip_util import encoder_from_state, dev
    cfg = dict(mlp_dim=64)
    st = synth.encoder_state(mlp_dim=64)
    enc = encoder_from_state(st, cfg)
    x = dev(synth.bag(400, 64))
    x_keep = x.clone()
    y3 = enc(x.unsqueeze(0))
    y2 = enc(x)
    y4 = enc(x.t().reshape(1, 64, 20, 20).contiguous())
    torch.cuda.synchronize()
    assert y3.shape == (1, 400, 64) and y2.shape == (400, 64) and y4.shape == (1, 64, 20, 20)
    assert torch.equal(x, x_keep)
    assert torch.equal(y2, y3[0])
    assert torch.equal(y4.reshape(1, 64, 400).transpose(1, 2)[0], y2)
    # batch > 1 (round 4): the reference's semantics -- a (2, C, H, W) input comes back (2, C, H, W), and the two bags are
    # coupled inside CR-MSA (test_encoder_batch_gt_1_matches_reference holds the values to the reference's)
    yb = enc(torch.stack([x, x]))
    yb4 = enc(torch.stack([x, x]).transpose(1, 2).reshape(2, 64, 20, 20).contiguous())
    torch.cuda.synchronize()
    assert yb.shape == (2, 400, 64) and yb4.shape == (2, 64, 20, 20) and torch.isfinite(yb).all()
    assert torch.equal(yb4.reshape(2, 64, 400).transpose(1, 2), yb)
    with pytest.raises(NotImplementedError):
        enc.train()(x)
    with pytest.raises(NotImplementedError):
        enc.train()(torch.stack([x, x]))                 # a graph / dropout at B > 1: not covered by the HIP backward


@pytest.mark.parametrize("extra", [dict(ffn=True), dict(ffn=True, ffn_act="relu", all_shortcut=True), dict(n_layers=3),
                                   dict(pos="ppeg", pos_pos=-1), dict(pos="peg", pos_pos=-1, n_layers=1), dict(cr_msa=False),
                                   dict(epeg=False, crmsa_k=8), dict(region_num=4, crmsa_k=2)])
def test_encoder_batch_gt_1_variants_match_oracle(extra):
    """The batch entry point on the constructor variants the G20 fixtures do not cover (FFN after every layer, three layers,
    PEG / PPEG in front, no CR-MSA, no EPEG, other region counts) against the oracle's eager port on the same (3, N, D)
    input -- the port is pinned to the reference at B > 1 by the G20 fixtures (tests/test_oracle_golden.py)."""
    from hip_util import encoder_from_state, dev
    cfg = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
    cfg.update(extra)
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k in _STATE_KEYS})
    B, N = 3, 1100
    x = np.stack([synth.bag(N, 512, tag=f"batchv/b{b}") for b in range(B)])
    ref = O.forward_eager(x, st, cfg).numpy()
    enc = encoder_from_state(st, cfg)
    y = enc(dev(x))
    torch.cuda.synchronize()
    _cmp(y.cpu().numpy(), ref, 2e-4, f"batch {extra}")


def test_repeatable_and_workspace_poison():
    """Bit-identical across calls, also after the cached workspace is filled with NaNs
    (no read-before-write of scratch)."""
    from hip_util import encoder_from_state, dev
    g = load_golden("G2_d512_n512")
    x, st, cfg = synth_case(g)
    enc = encoder_from_state(st, cfg)
    xd = dev(x)
    y1 = enc(xd).clone()
    enc._ws.view(torch.float32).fill_(float("nan"))
    y2 = enc(xd).clone()
    big = enc(dev(synth.bag(3000, 512)))          # grow the workspace, then shrink the bag again
    y3 = enc(xd)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.isfinite(big).all()


# ------------------------------------------------------------------ full-size properties
def test_full_size_properties():
    """BASELINE north-star size (N=9000): size-independent properties of the path.
    (a) output rows are LayerNorm-ed: per-row mean == beta-mean, variance == gamma-energy;
    (b) region locality of R-MSA: perturbing one token changes x1 only inside its region
        (cr_msa=False isolates the R-MSA layer);
    (c) token-permutation consistency of pad handling: N=9216 (pad=0) equals N=9216 built
        as 9000 real tokens + the values the pad rows would have -- not applicable (pads skip
        LN), so instead: all_shortcut linearity  y_sc(x) == LN(x2 + x)."""
    from hip_util import encoder_from_state, dev
    N, D = 9000, 512
    st = synth.encoder_state()
    x = synth.bag(N, D)
    enc = encoder_from_state(st, dict())
    y = enc(dev(x)).cpu().numpy().astype(np.float64)
    gam, bet = st["norm.weight"].astype(np.float64), st["norm.bias"].astype(np.float64)
    zn = (y - bet) / gam                        # undo affine: rows must be standardised
    assert np.abs(zn.mean(-1)).max() < 1e-4
    assert np.abs(zn.var(-1) - 1.0).max() < 1e-3
    # (b) locality
    cfg = dict(cr_msa=False)
    st2 = synth.encoder_state(cr_msa=False)
    st2["norm.weight"] = np.ones(D, np.float32)
    st2["norm.bias"] = np.zeros(D, np.float32)
    enc2 = encoder_from_state(st2, cfg)
    xa = dev(x)
    xb = xa.clone()
    tok = 37 * 96 + 50                          # grid (37,50) -> region (3,4)
    xb[tok] += 1.0
    ya, yb = enc2(xa).cpu().numpy(), enc2(xb).cpu().numpy()
    changed = np.nonzero(np.abs(ya - yb).max(-1) > 0)[0]
    ii, jj = changed // 96, changed % 96
    assert changed.size > 0 and set(ii // 12) == {3} and set(jj // 12) == {4}


@pytest.mark.parametrize("N,rn", [(100000, 8), (120000, 16)])
def test_huge_bag(N, rn):
    """Far beyond the golden sizes (regions of 1600 / 484 tokens: the streaming online-softmax attention, 64-bit
    row offsets, a 1 GB workspace).  R-MSA is region-local, so with cr_msa=False one whole region can be
    checked against the float64 restatement without running the oracle on the full bag; the full encoder
    (with CR-MSA) is checked through the LayerNorm property."""
    from hip_util import encoder_from_state, dev
    D = 512
    x = synth.bag(N, D, tag=f"huge{N}")
    H, s, add = O.grid(N, rn)
    P = s * s
    st = synth.encoder_state(cr_msa=False)
    enc = encoder_from_state(st, dict(cr_msa=False, region_num=rn))
    xd = dev(x)
    y = enc(xd).cpu().numpy()
    assert np.isfinite(y).all()
    for ri, rj in ((0, 0), (3, rn - 2), (rn - 1, rn - 1)):        # first, interior and last (padded) region
        ii, jj = np.meshgrid(ri * s + np.arange(s), rj * s + np.arange(s), indexing="ij")
        t = (ii * H + jj).reshape(-1)                             # token ids of the region, region order
        real = t < N
        u = np.zeros((P, D))
        u[real] = O._ln64(x[t[real]].astype(np.float64), st["layers.0.norm.weight"].astype(np.float64),
                          st["layers.0.norm.bias"].astype(np.float64))
        z = O._inner_attention64(u[None], st, "layers.0.attn.attn.", 8, 15)[0]
        ref = O._ln64(x[t[real]].astype(np.float64) + z[real], st["norm.weight"].astype(np.float64),
                      st["norm.bias"].astype(np.float64))
        _cmp(y[t[real]], ref, 2e-4, f"huge bag N={N} region ({ri},{rj})")
    del enc
    st = synth.encoder_state()
    enc = encoder_from_state(st, dict(region_num=rn))
    y = enc(xd).cpu().numpy().astype(np.float64)
    zn = (y - st["norm.bias"].astype(np.float64)) / st["norm.weight"].astype(np.float64)
    assert np.abs(zn.mean(-1)).max() < 1e-4 and np.abs(zn.var(-1) - 1.0).max() < 1e-3


@pytest.mark.parametrize("name", ["G8_rrtmil_n1000", "G8_rrtmil_n9000"])
def test_rrtmil_matches_reference(name):
    """BASELINE configs[2] (C16-R50): fc 1024->512 + ReLU -> encoder (HIP) -> DAttention -> predictor,
    against the real reference RRTMIL's logits and attention scores (modules/rrt.py:227-246)."""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTMIL
    g = load_golden(name)
    cfg, N = g["cfg"], int(g["n"])
    st = synth.mil_state(input_dim=1024, n_classes=2, epeg_k=15, crmsa_k=1)
    mil = RRTMIL(**cfg).eval()
    mil.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    mil = mil.to(DEV)
    feats = dev(synth.bag(N, 1024, tag="mil", nonneg=True)).unsqueeze(0)
    logits, attn = mil(feats, return_attn=True)
    torch.cuda.synchronize()
    assert logits.shape == (1, 2) and attn.shape == (1, N)
    _cmp(logits.cpu().numpy(), g["logits"], 1e-4, name + " logits")
    _cmp(attn.cpu().numpy(), g["attn"], 1e-6, name + " attention")    # softmax weights ~1/N
    assert torch.equal(mil(feats), logits)


# ------------------------------------------------------------------ row f1: RRTMIL around the encoder
@pytest.mark.parametrize("act", [1, 2, 3, 4])
@pytest.mark.parametrize("M,N,K", [(9000, 512, 1024), (1000, 130, 96), (9000, 128, 512)])
def test_linear_act(M, N, K, act):
    """nn.Linear + activation in the GEMM epilogue (patch_to_emb rrt.py:208-217, DAttention datten.py:14-22)."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    A = synth.normal(f"act/A{M}x{K}", (M, K))
    B = synth.uniform(f"act/B{N}x{K}", (N, K), -1, 1) / np.sqrt(K) * 2
    bias = synth.uniform(f"act/b{N}", (N,), -0.5, 0.5)
    dA, dB, db = dev(A), dev(B), dev(bias)
    out = torch.full((M, N), float("nan"), device=DEV)
    _lib.check(lib.rrt_linear_act_f32(p(dA), p(dB), p(db), p(out), M, N, K, act, 0, stream()), "linear_act")
    torch.cuda.synchronize()
    z = A.astype(np.float64) @ B.astype(np.float64).T + bias
    name = {1: "relu", 2: "gelu", 3: "tanh"}.get(act)
    ref = O._act64(z, name) if name else 1.0 / (1.0 + np.exp(-z))
    _cmp(out.cpu().numpy(), ref, 2e-5, f"linear+act{act} {M}x{N}x{K}")


@pytest.mark.parametrize("N,D,gated,bias,act,ncls", [(9000, 512, False, False, "relu", 2), (9000, 512, True, True, "tanh", 4),
                                                     (1, 512, False, True, "gelu", 2), (31, 64, True, False, "relu", 3),
                                                     (33, 512, False, False, "none", 1), (30000, 512, False, True, "tanh", 2),
                                                     (1000, 1024, True, True, "gelu", 5)])
def test_pool_predict(N, D, gated, bias, act, ncls):
    """DAttention pooling + predictor (online softmax over token chunks) against the float64 restatement of
    datten.py:28-38 / :69-83 and rrt.py:241; both forms of the returned attention row."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    st = synth.mil_state(input_dim=64, n_classes=ncls, da_bias=bias, da_gated=gated, da_act=act, mlp_dim=D)
    st = {k: v for k, v in st.items() if k.startswith(("pool_fn.", "predictor."))}
    y = synth.normal(f"pool/y{N}x{D}", (N, D)) * 1.5
    # a few dominant tokens: the softmax over the bag must be far from uniform somewhere
    y[:: max(1, N // 7)] *= 4.0
    logits_ref, attn_ref, raw_ref, pooled_ref = O.pool_predict_f64(y, st, act, gated)
    pf = "pool_fn.attention."
    if gated:
        na, nb_, nc = pf + "attention_a.0", pf + "attention_b.0", pf + "attention_c"
    else:
        na, nb_, nc = pf + "attention.0", None, pf + ("attention.2" if act in ("relu", "gelu", "tanh") else "attention.1")
    d = {k: dev(v) for k, v in st.items()}
    g = lambda n: d.get(n) if n else None
    need = C.c_size_t()
    _lib.check(lib.rrt_pool_workspace_size(N, D, 128, int(gated), C.byref(need)), "pool ws")
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=DEV)       # NaN-poisoned workspace
    dy = dev(y)
    for no_norm in (0, 1):
        pooled = torch.full((D,), float("nan"), device=DEV)
        logits = torch.full((ncls,), float("nan"), device=DEV)
        attn = torch.full((N,), float("nan"), device=DEV)
        rc = lib.rrt_pool_predict_f32(p(dy), p(g(na + ".weight")), p(g(na + ".bias")),
                                      p(g(nb_ + ".weight")) if nb_ else None, p(g(nb_ + ".bias")) if nb_ else None,
                                      p(g(nc + ".weight")), p(g(nc + ".bias")), p(d["predictor.weight"]),
                                      p(d["predictor.bias"]), p(pooled), p(logits), p(attn), no_norm, N, D, 128,
                                      _lib.ACT_BY_NAME.get(act, 0), ncls, 0, p(ws), ws.numel(), stream())
        _lib.check(rc, "pool_predict")
        torch.cuda.synchronize()
        # peaked softmax: an fp32 score error d moves every weight by a factor e^d -> tolerance relative
        # to the magnitude of the result
        scale = max(1.0, float(np.abs(pooled_ref).max()))
        _cmp(pooled.cpu().numpy(), pooled_ref, 2e-5 * scale, "pooled")
        _cmp(logits.cpu().numpy(), logits_ref, 2e-5 * scale, "logits")
        if no_norm:
            _cmp(attn.cpu().numpy(), raw_ref, 2e-5, "raw scores")
        else:
            got = attn.cpu().numpy()
            assert abs(got.astype(np.float64).sum() - 1.0) < 1e-5
            assert np.abs(got - attn_ref).max() <= 1e-6 + 1e-5 * attn_ref.max()


@pytest.mark.parametrize("name", golden_names("G11"))
def test_rrtmil_variants_match_reference(name):
    """RRTMIL constructor variants (gated / bias / activations / n_classes / input_dim) through the one-call
    HIP path (rrt_mil_forward_f32) against the real reference's logits, attention and raw scores."""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTMIL
    g = load_golden(name)
    cfg, N = g["cfg"], int(g["n"])
    enc_keys = {k: v for k, v in cfg.items() if k in ("epeg_k", "crmsa_k")}
    st = synth.mil_state(input_dim=cfg["input_dim"], n_classes=cfg["n_classes"], da_bias=cfg.get("da_bias", False),
                         da_gated=cfg.get("da_gated", False), da_act=cfg.get("da_act", "relu"), **enc_keys)
    mil = RRTMIL(**cfg).eval()
    mil.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    mil = mil.to(DEV)
    feats = dev(synth.bag(N, cfg["input_dim"], tag="mil/" + name[len("G11_rrtmil_"):], nonneg=True)).unsqueeze(0)
    logits, attn = mil(feats, return_attn=True)
    _, raw = mil(feats, return_attn=True, no_norm=True)
    torch.cuda.synchronize()
    assert logits.shape == (1, cfg["n_classes"]) and attn.shape == (1, N) and raw.shape == (1, N)
    _cmp(logits.cpu().numpy(), g["logits"], 1e-4, name + " logits")
    _cmp(attn.cpu().numpy(), g["attn"], 1e-6, name + " attention")
    _cmp(raw.cpu().numpy(), g["attn_raw"], 1e-4, name + " raw scores")
    # the composite path (other input ranks: reference op sequence in torch around the HIP encoder) agrees
    with torch.no_grad():
        x2 = mil.dp(mil.patch_to_emb(feats))
        y2 = mil.online_encoder(x2)
        l2 = mil.predictor(mil.pool_fn(y2))
    _cmp(l2.cpu().numpy(), logits.cpu().numpy(), 1e-4, name + " composite vs one-call")


@pytest.mark.parametrize("name", golden_names("G13"))
def test_rrtmil_readme_configs(name):
    """The six published training configs of the reference README (C16 / TCGA-BRCA / TCGA-NSCLC x R50 / PLIP:
    epeg_k 9..21, crmsa_k 1..5, crmsa_heads=1, crmsa_mlp, all_shortcut, da_act=tanh) as whole classifiers
    through rrt_mil_forward_f32, against the real reference's logits and attention."""
    from conftest import mil_case
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTMIL
    g, cfg, st, feats = mil_case(name)
    mil = RRTMIL(**cfg).eval()
    mil.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    mil = mil.to(DEV)
    logits, attn = mil(dev(feats).unsqueeze(0), return_attn=True)
    torch.cuda.synchronize()
    _cmp(logits.cpu().numpy(), g["logits"], 1e-4, name + " logits")
    _cmp(attn.cpu().numpy(), g["attn"], 1e-6, name + " attention")


@pytest.mark.gpu
@pytest.mark.parametrize("N,gated,bias,act,no_norm", [(3000, False, False, "relu", False), (9000, False, True, "gelu", False),
                                                      (1000, True, False, "tanh", False), (777, True, True, "relu", True),
                                                      (50, False, False, "tanh", True), (4097, False, True, "none", False)])
def test_attn_pool_forward_backward(N, gated, bias, act, no_norm):
    """DAttention's scores -> softmax over the bag -> weighted sum (modules/datten.py:28-38, :69-83) as one HIP call each way
    (rrt_attn_pool_f32 / rrt_attn_pool_backward_f32 behind mil._AttnPool): pooled, attention and every gradient -- x, both
    hidden Linears, the score Linear and its bias, including the gradient that flows through the RETURNED attention row --
    against the same module evaluated by torch in float64."""
    import copy
    from rrt_mil_amd.mil import RRTMIL
    torch.manual_seed(7)
    mil = RRTMIL(input_dim=64, n_classes=2, da_act=act, da_gated=gated, da_bias=bias, dropout=0.0).to("cuda:0").train()
    ref = copy.deepcopy(mil.pool_fn).double()
    x = torch.from_numpy(synth.normal(f"pool/x{N}", (1, N, 512))).to("cuda:0").requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    r1 = torch.from_numpy(synth.normal("pool/r1", (1, 512))).to("cuda:0")
    r2 = torch.from_numpy(synth.normal(f"pool/r2{N}", (1, N))).to("cuda:0")
    pooled, a = mil._pool(x, no_norm)
    p64, a64 = ref(x64, return_attn=True, no_norm=no_norm)
    assert pooled.shape == p64.shape and a.shape == a64.shape
    assert float((pooled.double() - p64).abs().max()) <= 2e-5 and float((a.double() - a64).abs().max()) <= 2e-5 * max(1.0, float(a64.abs().max()))
    ((pooled * r1).sum() + (a * r2).sum()).backward()
    ((p64 * r1.double()).sum() + (a64 * r2.double()).sum()).backward()
    torch.cuda.synchronize()

    def close(g, g64, what):
        scale = float(g64.abs().max()) + 1e-30
        err = float((g.double() - g64).abs().max())
        # (2e-6 absolute: the hidden Linear's bias shifts every score by one constant, its gradient is exactly 0)
        assert err <= 2e-4 * scale + 2e-6, (what, err, scale)
    close(x.grad, x64.grad, "dx")
    for (name, p), (_, p64_) in zip(mil.pool_fn.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (p64_.grad is None), name
        if p.grad is not None:
            close(p.grad, p64_.grad, name)


@pytest.mark.parametrize("dt", [None, torch.bfloat16])
def test_rrtmil_forward_bags(dt):
    """RRTMIL.forward_bags: a list of slides of mixed sizes, four in flight on the process's bag streams, each one
    rrt_mil_forward_f32 call with its own workspace == the same slides one at a time, bit for bit (logits and attention)."""
    from rrt_mil_amd.mil import RRTMIL
    torch.manual_seed(3)
    mil = RRTMIL(input_dim=256, n_classes=3, da_gated=True, dropout=0.25).to("cuda:0").eval()
    if dt is not None:
        mil.online_encoder.compute_dtype = dt
    sizes = [3000, 700, 5000, 1, 4096, 2200, 3000]
    bags = [torch.from_numpy(synth.bag(n, 256, tag=f"milbags/{i}", nonneg=True)).to("cuda:0") for i, n in enumerate(sizes)]
    with torch.no_grad():
        ref = [mil(b.unsqueeze(0), return_attn=True) for b in bags]
        outs = mil.forward_bags(bags, streams=4, return_attn=True)
        outs3 = mil.forward_bags([b.unsqueeze(0) for b in bags], streams=2)
        again = mil.forward_bags(bags, streams=4, return_attn=True)          # cached 16-bit weight images per stream slot
    torch.cuda.synchronize()
    for (lg, at), (rl, ra), l3, (lg2, _) in zip(outs, ref, outs3, again):
        # slides in flight: bit for bit among themselves, whatever the width of the call ...
        assert torch.equal(l3[0], lg) and torch.equal(lg2, lg)
        # ... and against the slide alone (rrt_encoder_desc.solo = 1: another CR-MSA front in exact fp32, ~1e-7; the 16-bit
        # modes take the same kernels either way -- only a tile shape differs, not the bits)
        if dt is None:
            assert torch.allclose(lg, rl[0], rtol=2e-5, atol=2e-6) and torch.allclose(at, ra[0], rtol=2e-5, atol=2e-6)
        else:
            assert torch.equal(lg, rl[0]) and torch.equal(at, ra[0])
    assert mil.forward_bags([]) == []


def test_rrtmil_fails_loudly():
    from rrt_mil_amd import RRTMIL
    mil = RRTMIL(input_dim=64, n_classes=2).eval()
    with pytest.raises(_lib.RRTHipError):
        mil.forward_bag(torch.zeros(10, 64))                 # CPU tensor: no fallback
    mil = mil.to("cuda:0")
    with pytest.raises(ValueError):
        mil.forward_bag(torch.zeros(10, 96, device="cuda:0"))
    with torch.enable_grad():
        out = mil.train()(torch.randn(1, 10, 64, device="cuda:0"))      # training records a graph (row f2)
    assert out.grad_fn is not None and out.shape == (1, 2)
    with pytest.raises(NotImplementedError):                            # the one-call inference path refuses train mode
        mil.forward_bag(torch.zeros(10, 64, device="cuda:0"))


# ------------------------------------------------------------------ batch-of-bags executor
@pytest.mark.parametrize("streams", [1, 2, 3, 4])
def test_forward_bags_mixed_sizes(streams):
    """BASELINE configs[4] shape of work: a batch of independent bags of mixed N through the executor
    (several bags in flight on the library's streams) == the same bags one at a time, bit for bit."""
    from hip_util import DEV, dev, encoder_from_state
    cfg = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
    enc = encoder_from_state(synth.encoder_state(**cfg), cfg)
    sizes = [3000, 9000, 50, 4096, 1, 15000, 9000, 777]
    bags = [dev(synth.bag(n, 512, tag=f"exec/{i}")) for i, n in enumerate(sizes)]
    # (rrt_encoder_desc.solo picks the representatives' GEMM kernel -- another summation order: the comparison is bit for
    #  bit at the executor's setting, solo = (streams == 1); across settings the outputs agree to ~1e-7, checked below)
    enc.solo = streams == 1
    ref = [enc(b.unsqueeze(0)).squeeze(0).clone() for b in bags]
    enc.solo = not enc.solo
    other = enc(bags[1].unsqueeze(0)).squeeze(0)
    assert float((other - ref[1]).abs().max()) <= 2e-6
    enc.solo = streams == 1
    small = enc.forward_bags(bags[:3], streams=streams)            # executor sized for N <= 9000 ...
    outs = enc.forward_bags(bags, streams=streams)                 # ... then has to grow for N = 15000
    again = enc.forward_bags([b.unsqueeze(0) for b in bags], streams=streams)
    torch.cuda.synchronize()
    for i, n in enumerate(sizes):
        assert outs[i].shape == (n, 512) and again[i].shape == (1, n, 512)
        assert torch.equal(outs[i], ref[i]), f"bag {i} (N={n}) differs from the one-at-a-time forward"
        assert torch.equal(again[i][0], ref[i])
    for i in range(3):
        assert torch.equal(small[i], ref[i])
    assert enc.forward_bags([]) == []


@pytest.mark.parametrize("streams", [2, 4])
def test_forward_bags_is_ordered_on_the_callers_stream(streams):
    """Round 4: slot 0 of an executor call runs on the CALLER's stream and the executor's other slots on streams handed over by
    the host framework (rrt_executor_create_on_streams).  The call must still behave like one op of the caller's stream:
    inputs produced on that stream just before the call are seen, outputs consumed on it right after are complete -- on a
    side stream (asynchronous) and on the default stream (four bags in flight: side stream + host wait) alike."""
    from hip_util import dev, encoder_from_state
    cfg = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
    enc = encoder_from_state(synth.encoder_state(**cfg), cfg)
    enc.solo = False
    base = [dev(synth.bag(n, 512, tag=f"ord/{i}")) for i, n in enumerate([4096, 3000, 5000, 2500, 4096, 700])]
    ref = [enc((b * 2.0 - 1.0).unsqueeze(0)).squeeze(0).clone() for b in base]
    torch.cuda.synchronize()
    for ctx in (torch.cuda.stream(torch.cuda.Stream()), contextlib.nullcontext()):
        with ctx:
            for rep in range(3):
                bags = [b * 2.0 - 1.0 for b in base]                 # produced on the caller's stream, no sync
                outs = enc.forward_bags(bags, streams=streams)
                sums = torch.stack([o.double().sum() for o in outs])  # consumed on the caller's stream, no sync
            torch.cuda.current_stream().synchronize()
        for o, r in zip(outs, ref):
            assert torch.equal(o, r)
        assert torch.allclose(sums, torch.stack([r.double().sum() for r in ref]), rtol=0, atol=1e-9)
    # two calls from two DIFFERENT caller streams back to back, no sync in between: slot 0 (its workspace) moves from one
    # caller's stream to the other's and must not be shared while the first call is still running
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    inputs = [b * 2.0 - 1.0 for b in base]
    torch.cuda.synchronize()
    for rep in range(4):
        with torch.cuda.stream(sa):
            oa = enc.forward_bags(inputs, streams=streams)
        with torch.cuda.stream(sb):
            ob = enc.forward_bags(list(reversed(inputs)), streams=streams)
    torch.cuda.synchronize()
    for o, r in zip(oa, ref):
        assert torch.equal(o, r)
    for o, r in zip(ob, reversed(ref)):
        assert torch.equal(o, r)


@pytest.mark.parametrize("dt", [None, torch.bfloat16])
def test_forward_bags_config4_hyperparameters(dt):
    """BASELINE configs[4] as bench.py runs it: epeg_k=21, crmsa_k=5, a mix of bag sizes through the executor (several
    streams, generic CR-MSA kernels, cached 16-bit weight images under bf16), every bag against the REAL reference:
    fp32 vs the G5 / G19 goldens; bf16 vs the reference's own autocast runs (G16) where they exist and the fp32
    goldens at the autocast bounds elsewhere."""
    from hip_util import dev, encoder_from_state
    names = ["G5_d512_n15000_k21_c5", "G19_d512_n5600_k21_c5", "G5_d512_n3000_k21_c5", "G19_d512_n11000_k21_c5"]
    gs = [load_golden(n) for n in names]
    x0, st, cfg = synth_case(gs[0])
    assert cfg["epeg_k"] == 21 and cfg["crmsa_k"] == 5
    enc = encoder_from_state(st, cfg)
    enc.compute_dtype = dt
    bags = [dev(synth_case(g)[0]) for g in gs]
    for rep in range(2):                       # second pass: the weight images are cached, bags land on other streams
        outs = enc.forward_bags(bags if rep == 0 else bags[::-1], streams=3)
        torch.cuda.synchronize()
        outs = outs if rep == 0 else outs[::-1]
        for g, name, y in zip(gs, names, outs):
            y = y.cpu().numpy()
            if dt is None:
                _cmp(y[g["rows"]], g["y_rows"], TOL_E2E, name)
                s = np.array([y.astype(np.float64).sum(), np.abs(y.astype(np.float64)).sum()])
                assert np.allclose(s, g["y_sums"][:2], rtol=1e-5, atol=N_ATOL(int(g["n"])))
            else:
                err = np.abs(y[g["rows"]] - g["y_rows"])
                assert np.isfinite(y).all() and err.max() <= TOL_AMP_MAX and err.mean() <= TOL_AMP_MEAN, (name, err.max(), err.mean())
                amp = "G16_amp_bf16_d512_n%d_k21_c5" % int(g["n"])
                if amp in golden_names("G16"):
                    ga = load_golden(amp)
                    to_fp32 = np.abs(y[ga["rows"]] - ga["y32_rows"])
                    amp_to_fp32 = np.abs(ga["y_rows"].astype(np.float64) - ga["y32_rows"])
                    assert to_fp32.mean() <= amp_to_fp32.mean() and to_fp32.max() <= 1.1 * amp_to_fp32.max(), name


def test_executor_rejects_bad_input():
    from hip_util import DEV, dev, encoder_from_state
    cfg = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
    enc = encoder_from_state(synth.encoder_state(**cfg), cfg)
    with pytest.raises(_lib.RRTHipError):
        enc.forward_bags([torch.zeros(10, 512)])                    # CPU bag: no fallback
    with pytest.raises(ValueError):
        enc.forward_bags([torch.zeros(10, 64, device=DEV)])
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rrt_executor_create(C.byref(enc._desc), 0, 9000, C.byref(h)) == -2      # n_streams out of range
    assert lib.rrt_executor_create(C.byref(enc._desc), 2, 0, C.byref(h)) == -1
    assert lib.rrt_executor_destroy(None) == 0


# ------------------------------------------------------------------ reduced-precision operand modes
def _round_bf16(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("M,N,K", [(9216, 1536, 512), (192, 512, 512), (1000, 130, 96), (9216, 512, 1024)])
def test_linear_reduced_precision(M, N, K, compute):
    """bf16 / fp16 MFMA operands, fp32 accumulate: must equal the float64 product of the ROUNDED
    operands (the rounding itself is the only approximation the mode introduces)."""
    from hip_util import dev, linear
    A = synth.normal(f"linr/A{M}x{K}", (M, K))
    B = synth.uniform(f"linr/B{N}x{K}", (N, K), -1, 1) / np.sqrt(K)
    bias = synth.uniform(f"linr/b{N}", (N,), -0.5, 0.5)
    dA, dB, db = dev(A), dev(B), dev(bias)
    got = linear(dA, dB, db, 0, 1.0, compute).cpu().numpy()
    rnd = _round_bf16 if compute == 1 else (lambda a: a.astype(np.float16).astype(np.float32))
    ref = rnd(A).astype(np.float64) @ rnd(B).astype(np.float64).T + bias
    # bf16: exact up to fp32 accumulation order.  fp16: mean error 3e-7, but rare elements whose
    # weight operand is an fp16 SUBNORMAL (|w| < 6.1e-5) differ by up to ~1.4e-4 (hardware denormal
    # handling vs numpy) -- far below the mode's own rounding error (~1e-3), hence the looser bound.
    _cmp(got, ref, 2e-5 if compute == 1 else 5e-4, f"linear compute={compute}")
    assert np.abs(got - ref).mean() < 2e-6
    exact = A.astype(np.float64) @ B.astype(np.float64).T + bias
    assert np.abs(got - exact).max() > 1e-4          # the mode really is reduced precision


# BASELINE.json configs[2..4] ask for bf16: autocast-class numerics, compared with the fp32
# reference at the bounds SURVEY.md §7.3 H2 proposes (2e-2 max, 2e-3 mean).
TOL_AMP_MAX, TOL_AMP_MEAN = 2e-2, 2e-3


@pytest.mark.parametrize("name,dt", [("G3_d512_n9000", torch.bfloat16), ("G3_d512_n9000", torch.float16),
                                     ("G4_d512_n30000_rn16", torch.bfloat16),
                                     ("G5_d512_n3000_k21_c5", torch.bfloat16),
                                     ("G5_d512_n15000_k21_c5", torch.bfloat16),
                                     ("G5_d512_n9000_c1_sc", torch.bfloat16)])
def test_encoder_amp_modes(name, dt):
    from hip_util import encoder_from_state, dev
    g = load_golden(name)
    x, st, cfg = synth_case(g)
    enc = encoder_from_state(st, cfg)
    xd = dev(x)
    enc.compute_dtype = dt
    y = enc(xd).cpu().numpy()
    err = np.abs(y[g["rows"]] - g["y_rows"])
    assert np.isfinite(y).all() and err.max() <= TOL_AMP_MAX and err.mean() <= TOL_AMP_MEAN, (err.max(), err.mean())
    assert err.max() > 1e-5                      # not silently the exact path
    # torch autocast selects the same mode
    enc.compute_dtype = None
    with torch.autocast("cuda", dtype=dt):
        y2 = enc(xd).cpu().numpy()
    y3 = enc(xd).cpu().numpy()                   # outside autocast: exact fp32 again
    assert np.array_equal(y, y2)
    _cmp(y3[g["rows"]], g["y_rows"], TOL_E2E, name + " fp32 after amp")


def test_rrtmil_autocast_bf16():
    """BASELINE configs[2]: C16-R50 RRTMIL under bf16 autocast (the reference's --amp path)."""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTMIL
    g = load_golden("G8_rrtmil_n9000")
    st = synth.mil_state(input_dim=1024, n_classes=2, epeg_k=15, crmsa_k=1)
    mil = RRTMIL(**g["cfg"]).eval()
    mil.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    mil = mil.to(DEV)
    feats = dev(synth.bag(9000, 1024, tag="mil", nonneg=True)).unsqueeze(0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = mil(feats)
    torch.cuda.synchronize()
    assert np.abs(logits.float().cpu().numpy() - g["logits"]).max() <= 2e-2


@pytest.mark.parametrize("n", [1, 7, 63, 200, 1111])
def test_rrtmil_autocast_small_bags(n):
    """Round 5: under autocast the classifier's patch_to_emb casts features + weight to 16 bits in one launch and multiplies
    16-bit operands (rrt_mil_forward_f32).  Bags far smaller than a GEMM tile, ragged row counts: finite logits within the
    bf16 tolerance of the fp32 classifier, twice in a row (the workspace's 16-bit images are rewritten every call)."""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTMIL
    cfg = dict(input_dim=1024, n_classes=2, epeg_k=15, crmsa_k=1)
    st = synth.mil_state(**cfg)
    mil = RRTMIL(**load_golden("G8_rrtmil_n9000")["cfg"]).eval()
    mil.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    mil = mil.to(DEV)
    feats = dev(synth.bag(n, 1024, tag=f"mil/small{n}", nonneg=True)).unsqueeze(0)
    with torch.no_grad():
        ref = mil(feats).float().cpu().numpy()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            a = mil(feats).float().cpu().numpy()
            b = mil(feats).float().cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b)
    assert np.abs(a - ref).max() <= 3e-2 * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------ fused R-MSA core
@pytest.mark.parametrize("R,P,D,heads,ek,compute", [(64, 144, 512, 8, 15, 0), (9, 121, 512, 8, 15, 0),
                                                    (3, 130, 512, 8, 0, 0), (2, 144, 512, 8, 21, 0),
                                                    (5, 113, 512, 8, 15, 0), (4, 128, 256, 4, 9, 0),
                                                    (64, 144, 512, 8, 15, 1),
                                                    # every row-tile count of the kernel: MT = 4, 6, 7, 11, 13
                                                    (64, 49, 512, 8, 15, 0), (10, 64, 512, 8, 21, 0),
                                                    (7, 81, 512, 8, 15, 0), (9, 100, 512, 8, 15, 0),
                                                    (64, 169, 512, 8, 15, 0), (11, 196, 512, 8, 21, 0),
                                                    (3, 208, 512, 8, 15, 0), (5, 177, 256, 4, 0, 0),
                                                    (6, 196, 512, 8, 15, 2), (8, 81, 512, 8, 15, 1)])
def test_rmsa_fused(R, P, D, heads, ek, compute):
    """qkv projection + EPEG + attention in one kernel (qkv never in HBM) against the float64
    restatement of rmsa.py:100-122 with the explicit [P,P] stencil."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    u = synth.normal(f"fus/u{R}x{P}", (R * P, D))
    W = synth.uniform(f"fus/w{D}", (3 * D, D), -1, 1) / np.sqrt(D)
    b = synth.uniform(f"fus/b{D}", (3 * D,), -0.3, 0.3)
    pe = synth.uniform("fus/pe", (heads, max(ek, 1)), -1, 1) / np.sqrt(max(ek, 1))
    d_u, d_W, d_b, d_pe = dev(u), dev(W), dev(b), dev(pe)
    o = torch.full((R * P, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_rmsa_fused_f32(p(d_u), p(d_W), p(d_b), p(d_pe) if ek else None, p(o), R, P, D, heads, ek,
                                      compute, stream()), "rmsa_fused")
    torch.cuda.synchronize()
    tol = 5e-5
    if compute == 1:
        qkv = _round_bf16(u).astype(np.float64) @ _round_bf16(W).astype(np.float64).T + b
    elif compute == 2:
        # fp16 operands (RNE); the hardware conversion may flush fp16 subnormals -> the looser bound of
        # test_linear_reduced_precision
        qkv = u.astype(np.float16).astype(np.float64) @ W.astype(np.float16).astype(np.float64).T + b
        tol = 5e-4
    else:
        qkv = u.astype(np.float64) @ W.astype(np.float64).T + b
    qkv[:, :D] *= (D // heads) ** -0.5
    ref = _attn_ref(qkv, pe, R, P, D, heads, ek)
    _cmp(o.cpu().numpy(), ref, tol, f"rmsa_fused R{R} P{P} D{D} k{ek} c{compute}")


def test_rmsa_fused_unsupported_shapes_report():
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    t = torch.zeros(256 * 3, 512 * 3, device=DEV)
    for P in (32, 48, 209, 256):                 # regions outside (48, 208] take the unfused kernels
        rc = lib.rrt_rmsa_fused_f32(p(t), p(t), None, None, p(t), 3, P, 512, 8, 0, 0, stream())
        assert rc == -2 and b"rmsa_fused" in lib.rrt_strerror(rc)


# every row-tile count the rule takes (MT = 6 ... 13) at region_num = 8 (64 regions = 512 items = two rounds of the chip),
# a real bag with pad slots, region_num = 16 (256 regions), the ragged-tail block order (region_num = 9: 81 regions)
@pytest.mark.parametrize("L,rn,D,heads,ek", [(9000, 8, 512, 8, 15), (5000, 8, 512, 8, 21), (6200, 8, 512, 8, 15), (7000, 8, 512, 8, 0),
                                             (8000, 8, 512, 8, 15), (10500, 8, 512, 8, 15), (12000, 8, 512, 8, 15),
                                             (30000, 16, 512, 8, 15), (9000, 9, 512, 8, 15)])
def test_rmsa_fused_proj(L, rn, D, heads, ek):
    """R-MSA core + out-projection + un-partition + residual in ONE launch (rmsa_fused_kernel<.., PROJ>: block b runs
    (region, head) item b, then the projection slab of a region whose items arrived a round earlier) against the
    two-launch pair it replaces -- bit for bit -- and against the float64 restatement of rmsa.py:100-131 / :41-54."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    g = _lib.region_grid(L, rn)
    Np, R, P = g.H * g.H, g.regions_side ** 2, g.s * g.s
    u = synth.normal(f"fp/u{Np}", (Np, D))
    W = synth.uniform(f"fp/w{D}", (3 * D, D), -1, 1) / np.sqrt(D)
    b = synth.uniform(f"fp/b{D}", (3 * D,), -0.3, 0.3)
    pe = synth.uniform("fp/pe", (heads, max(ek, 1)), -1, 1) / np.sqrt(max(ek, 1))
    Wp = synth.uniform(f"fp/wp{D}", (D, D), -1, 1) / np.sqrt(D)
    bp = synth.uniform(f"fp/bp{D}", (D,), -0.5, 0.5)
    res = synth.normal(f"fp/r{L}", (L, D))
    d_u, d_W, d_b, d_pe, d_Wp, d_bp, d_res = dev(u), dev(W), dev(b), dev(pe), dev(Wp), dev(bp), dev(res)
    o1 = torch.full((Np, D), float("nan"), device=DEV)
    out1 = torch.full((L, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_rmsa_fused_f32(p(d_u), p(d_W), p(d_b), p(d_pe) if ek else None, p(o1), R, P, D, heads, ek, 0,
                                      stream()), "rmsa_fused")
    _lib.check(lib.rrt_linear_unpartition_residual_f32(p(o1), p(d_Wp), p(d_bp), p(d_res), p(out1), D, D, C.byref(g), 0,
                                                       stream()), "unpart")
    o2 = torch.full((Np, D), float("nan"), device=DEV)
    out2 = torch.full((L, D), float("nan"), device=DEV)
    cnt = torch.full((R,), 12345, device=DEV, dtype=torch.int32)
    for _ in range(3):                                   # repeated launches on the same scratch (stale O rows, used counters)
        _lib.check(lib.rrt_rmsa_fused_proj_f32(p(d_u), p(d_W), p(d_b), p(d_pe) if ek else None, p(d_Wp), p(d_bp), p(d_res),
                                               p(out2), p(o2), p(cnt), D, heads, ek, C.byref(g), stream()), "rmsa_fused_proj")
    torch.cuda.synchronize()
    assert torch.equal(o1, o2), "attention output differs from the two-launch path"
    assert torch.equal(out1, out2), "projection differs from the two-launch path"
    if L <= 9000:
        qkv = u.astype(np.float64) @ W.astype(np.float64).T + b
        qkv[:, :D] *= (D // heads) ** -0.5
        o_ref = _attn_ref(qkv, pe, R, P, D, heads, ek)
        Z = o_ref @ Wp.astype(np.float64).T + bp
        z = np.empty((Np, D))
        z[O.partition_index(g.H, g.s)] = Z
        _cmp(out2.cpu().numpy(), res + z[:L], 1e-4, f"rmsa_fused_proj L{L} rn{rn}")


def test_rmsa_fused_proj_unsupported_shapes_report():
    """fewer than two rounds of items (region_num = 4: 16 regions) and regions outside the merged launch's range stay with
    the two launches"""
    from hip_util import p, stream, DEV
    lib = _lib.load()
    t = torch.zeros(16000, 512, device=DEV)
    t2 = torch.zeros(16000, 512, device=DEV)
    cnt = torch.zeros(1024, device=DEV, dtype=torch.int32)
    for L, rn in ((2000, 4), (15000, 8), (600, 8), (3000, 8), (4096, 8)):   # (regions of <= 64 tokens: the rule keeps two launches)
        g = _lib.region_grid(L, rn)
        rc = lib.rrt_rmsa_fused_proj_f32(p(t), p(t), None, None, p(t), None, p(t), p(t2), p(t), p(cnt), 512, 8, 0,
                                         C.byref(g), stream())
        assert rc == -2 and b"rmsa_fused_proj" in lib.rrt_strerror(rc), (L, rn, rc)


def _fused_proj_case(L, rn, D=512, heads=8, ek=15, tag="fp2"):
    """inputs of one merged launch + the two-launch pair's result for them (device tensors)"""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    g = _lib.region_grid(L, rn)
    Np, R, P = g.H * g.H, g.regions_side ** 2, g.s * g.s
    t = {"g": g, "Np": Np, "R": R, "P": P}
    t["u"] = dev(synth.normal(f"{tag}/u{Np}", (Np, D)))
    t["W"] = dev(synth.uniform(f"{tag}/w{D}", (3 * D, D), -1, 1) / np.sqrt(D))
    t["b"] = dev(synth.uniform(f"{tag}/b{D}", (3 * D,), -0.3, 0.3))
    t["pe"] = dev(synth.uniform(f"{tag}/pe", (heads, ek), -1, 1) / np.sqrt(ek))
    t["Wp"] = dev(synth.uniform(f"{tag}/wp{D}", (D, D), -1, 1) / np.sqrt(D))
    t["bp"] = dev(synth.uniform(f"{tag}/bp{D}", (D,), -0.5, 0.5))
    t["res"] = dev(synth.normal(f"{tag}/r{L}", (L, D)))
    o1 = torch.full((Np, D), float("nan"), device=DEV)
    out1 = torch.full((L, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_rmsa_fused_f32(p(t["u"]), p(t["W"]), p(t["b"]), p(t["pe"]), p(o1), R, P, D, heads, ek, 0, stream()), "rmsa_fused")
    _lib.check(lib.rrt_linear_unpartition_residual_f32(p(o1), p(t["Wp"]), p(t["bp"]), p(t["res"]), p(out1), D, D, C.byref(g), 0,
                                                       stream()), "unpart")
    torch.cuda.synchronize()
    t["o_ref"], t["out_ref"] = o1, out1
    return t


@pytest.mark.parametrize("L,rn", [(9000, 9), (8200, 10), (9000, 8)])
def test_rmsa_fused_proj_ragged_tail_fresh_inputs(L, rn):
    """Advisor (round 4, medium): with P < 16 MT a slab's loader used to over-read the first rows of region r + 1 -- whose
    counter it has not waited on -- into its XCD's L2; on ragged tails (81 / 100 regions: the tail regions' slabs run on
    every XCD) a later slab could then hit the stale lines.  Re-launching with IDENTICAL inputs cannot see that (stale ==
    fresh), so here the inputs CHANGE between launches on the same scratch: every launch must reproduce the two-launch
    pair of ITS inputs bit for bit."""
    from hip_util import p, stream, DEV
    lib = _lib.load()
    D, heads, ek = 512, 8, 15
    cases = [_fused_proj_case(L, rn, tag=f"rag{i}") for i in range(3)]
    g, Np, R = cases[0]["g"], cases[0]["Np"], cases[0]["R"]
    o2 = torch.full((Np, D), float("nan"), device=DEV)
    cnt = torch.full((R,), 777, device=DEV, dtype=torch.int32)
    outs = [torch.full((L, D), float("nan"), device=DEV) for _ in range(12)]
    for i in range(12):                                  # back to back, no host sync in between
        t = cases[i % 3]
        _lib.check(lib.rrt_rmsa_fused_proj_f32(p(t["u"]), p(t["W"]), p(t["b"]), p(t["pe"]), p(t["Wp"]), p(t["bp"]), p(t["res"]),
                                               p(outs[i]), p(o2), p(cnt), D, heads, ek, C.byref(g), stream()), "rmsa_fused_proj")
    torch.cuda.synchronize()
    for i in range(12):
        assert torch.equal(outs[i], cases[i % 3]["out_ref"]), f"launch {i}: projection differs from the two-launch pair of its inputs"
    assert lib.rrt_device_error(0) == 0


@pytest.mark.parametrize("lag", [250, 64, 504])
def test_rmsa_fused_proj_off_xcd_slabs_beside_a_cu_hog(lag):
    """The hand-over must not depend on where the dispatcher puts a block: with a lag that is not a multiple of 8 every
    slab runs on ANOTHER XCD than the items whose O rows it reads (write-through stores + first-touch loads), and a
    kernel on a second stream that occupies the CUs delays and reorders when the launch's blocks start.  Same bits as the
    two-launch pair, no hand-over error."""
    from hip_util import p, stream, DEV
    lib = _lib.load()
    L, rn, D, heads, ek = 9000, 8, 512, 8, 15
    t = _fused_proj_case(L, rn, tag="hog")
    g, Np, R = t["g"], t["Np"], t["R"]
    o2 = torch.full((Np, D), float("nan"), device=DEV)
    cnt = torch.zeros((R,), device=DEV, dtype=torch.int32)
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=DEV)
    big = torch.randn(64 * 1024 * 1024, device=DEV)
    outs = [torch.full((L, D), float("nan"), device=DEV) for _ in range(8)]
    torch.cuda.synchronize()
    for i in range(8):
        with torch.cuda.stream(side):                    # the hog: matrix products and streaming kernels of another "tenant"
            for _ in range(3):
                a = (a @ a).clamp_(-1, 1)
                big.mul_(1.0001)
        _lib.check(lib.rrt_debug_rmsa_fused_proj_f32(p(t["u"]), p(t["W"]), p(t["b"]), p(t["pe"]), p(t["Wp"]), p(t["bp"]),
                                                     p(t["res"]), p(outs[i]), p(o2), p(cnt), D, heads, ek, C.byref(g), lag, 0, 0,
                                                     stream()), "rmsa_fused_proj (debug)")
    torch.cuda.synchronize()
    for i in range(8):
        assert torch.equal(outs[i], t["out_ref"]), f"lag {lag}, launch {i}: differs from the two-launch pair"
    assert lib.rrt_device_error(0) == 0
    # lags outside [8 * heads, heads * regions] are refused (a slab would wait for an item with a HIGHER block index)
    for bad in (8, 63, 513):
        rc = lib.rrt_debug_rmsa_fused_proj_f32(p(t["u"]), p(t["W"]), p(t["b"]), p(t["pe"]), p(t["Wp"]), p(t["bp"]), p(t["res"]),
                                               p(outs[0]), p(o2), p(cnt), D, heads, ek, C.byref(g), bad, 0, 0, stream())
        assert rc == -2, (bad, rc)


def test_rmsa_fused_proj_bounded_wait_reports_and_recovers():
    """A slab whose region never 'arrives' (wait_extra = 1: one arrival more than a region gets) gives up after the spin
    limit instead of hanging the GPU, writes nothing, and raises the process's hand-over error word: every entry point that
    could launch the kernel then returns RRT_E_HANDOVER until rrt_device_error(1) has cleared it -- after which the same
    call works and is bit-identical again."""
    from hip_util import encoder_from_state, p, stream, DEV
    lib = _lib.load()
    L, rn, D, heads, ek = 9000, 8, 512, 8, 15
    t = _fused_proj_case(L, rn, tag="bw")
    g, Np, R = t["g"], t["Np"], t["R"]
    o2 = torch.full((Np, D), float("nan"), device=DEV)
    cnt = torch.zeros((R,), device=DEV, dtype=torch.int32)
    out = torch.full((L, D), 123.0, device=DEV)
    args = (p(t["u"]), p(t["W"]), p(t["b"]), p(t["pe"]), p(t["Wp"]), p(t["bp"]), p(t["res"]), p(out), p(o2), p(cnt), D, heads, ek,
            C.byref(g))
    assert lib.rrt_device_error(1) == 0
    _lib.check(lib.rrt_debug_rmsa_fused_proj_f32(*args, 0, 2000, 1, stream()), "rmsa_fused_proj (starved)")
    torch.cuda.synchronize()                              # returns: the wait is bounded
    assert torch.equal(o2, t["o_ref"]), "the items themselves ran"
    assert bool((out == 123.0).all()), "a slab that gave up must not write"
    code = lib.rrt_device_error(0)
    assert 1 <= code <= R, code
    assert lib.rrt_rmsa_fused_proj_f32(*args, stream()) == -4
    assert b"hand-over" in lib.rrt_strerror(-4)
    enc = encoder_from_state(synth.encoder_state(), dict(mlp_dim=512))
    x = torch.from_numpy(synth.bag(L, D, tag="bw/x")).to(DEV)
    with pytest.raises(_lib.RRTHipError, match="hand-over.*device_error"):
        enc(x.unsqueeze(0))
    import rrt_mil_amd                                    # the package-level recovery path (no reaching into _lib)
    assert rrt_mil_amd.device_error() == code
    assert rrt_mil_amd.device_error(clear=True) == code and rrt_mil_amd.device_error() == 0 and lib.rrt_device_error(0) == 0
    _lib.check(lib.rrt_rmsa_fused_proj_f32(*args, stream()), "rmsa_fused_proj after the clear")
    torch.cuda.synchronize()
    assert torch.equal(out, t["out_ref"])
    assert torch.isfinite(enc(x.unsqueeze(0))).all()


@pytest.mark.parametrize("L,rn,k,shift", [(9000, 8, 3, 0.0), (9000, 8, 5, 30.0), (5000, 8, 1, 0.0), (12000, 8, 8, -7.0),
                                          (30000, 16, 3, 0.0), (9000, 9, 3, 0.0)])
def test_rmsa_fused_proj_stats_and_combine_parts(L, rn, k, shift):
    """Round 5: the merged launch of the LAST R-MSA layer also leaves CR-MSA's row records -- per (token, 64-column slab) the
    mean and centred sum of squares of x1 there and d_n = sum x1 gamma phi_n -- and rrt_crmsa_combine_parts_f32 turns them
    and one pass over x1 into the dispatch weights and the representatives (rmsa.py:303-316).  (1) x1 is bit-identical to the
    launch without the by-product; (2) the records against float64 on that x1; (3) wdisp / rep against the float64
    restatement -- also with every row sitting at |mean| = 30 sigma (shift: the residual stream moved by a constant), where a
    one-pass E[x^2] - E[x]^2 variance would lose three digits; (4) region_num = 16 / 9: the R-MSA grid is not CR-MSA's 8 x 8
    grid, the records are per token."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    D, heads, ek = 512, 8, 15
    t = _fused_proj_case(L, rn, tag=f"st{k}")
    g, Np, R = t["g"], t["Np"], t["R"]
    res = t["res"] + shift
    gm = dev(1.0 + synth.uniform("st/g", (D,), -0.3, 0.3))
    bt = dev(synth.uniform("st/b", (D,), -0.2, 0.2))
    phi = dev(synth.uniform("st/phi", (D, k), -1, 1) * (3.0 / np.sqrt(D)))
    o2 = torch.full((Np, D), float("nan"), device=DEV)
    cnt = torch.zeros((R,), device=DEV, dtype=torch.int32)
    x1_plain = torch.full((L, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_rmsa_fused_proj_f32(p(t["u"]), p(t["W"]), p(t["b"]), p(t["pe"]), p(t["Wp"]), p(t["bp"]), p(res), p(x1_plain),
                                           p(o2), p(cnt), D, heads, ek, C.byref(g), stream()), "rmsa_fused_proj")
    K2, NS = (2 + k + 3) // 4 * 4, D // 64               # record stride: 2 + k floats rounded up to whole float4s
    x1 = torch.full((L, D), float("nan"), device=DEV)
    part = torch.full((L, NS, K2), float("nan"), device=DEV)
    for _ in range(2):
        _lib.check(lib.rrt_rmsa_fused_proj_stats_f32(p(t["u"]), p(t["W"]), p(t["b"]), p(t["pe"]), p(t["Wp"]), p(t["bp"]), p(res), p(x1),
                                                     p(o2), p(cnt), p(gm), p(phi), k, p(part), D, heads, ek, C.byref(g), stream()),
                   "rmsa_fused_proj_stats")
    torch.cuda.synchronize()
    assert torch.equal(x1, x1_plain), "the by-product must not change x1"
    x64 = x1.cpu().numpy().astype(np.float64)
    xs = x64.reshape(L, NS, 64)
    got = part.cpu().numpy().astype(np.float64)[..., :2 + k]
    assert np.isfinite(got).all()
    m_ref = xs.mean(-1)
    q_ref = ((xs - m_ref[..., None]) ** 2).sum(-1)
    gphi = (gm.cpu().numpy().astype(np.float64)[:, None] * phi.cpu().numpy().astype(np.float64)).reshape(NS, 64, k)
    d_ref = np.einsum("tsc,sck->tsk", xs, gphi)
    scale = max(1.0, abs(shift))
    assert np.abs(got[..., 0] - m_ref).max() <= 2e-6 * scale
    assert (np.abs(got[..., 1] - q_ref) / q_ref).max() <= 2e-5
    assert np.abs(got[..., 2:] - d_ref).max() <= 2e-5 * scale
    # combine from the records
    g8 = _lib.region_grid(L, 8)
    Np8, R8, P8 = g8.H * g8.H, 64, g8.s * g8.s
    wd = torch.full((Np8, k), float("nan"), device=DEV)
    rep = torch.full((k, R8, D), float("nan"), device=DEV)
    gbs = torch.full((16,), float("nan"), device=DEV)
    _lib.check(lib.rrt_crmsa_combine_parts_f32(p(x1), p(part), p(gm), p(bt), p(phi), p(wd), p(rep), L, D, k, C.byref(g8), stream()),
               "crmsa_combine_parts")
    torch.cuda.synchronize()
    gm64, bt64, phi64 = (a.cpu().numpy().astype(np.float64) for a in (gm, bt, phi))
    mu = x64.mean(-1, keepdims=True)
    v = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * gm64 + bt64
    perm = O.partition_index(g8.H, g8.s)
    V = np.concatenate([v, np.zeros((g8.add, D))], 0)[perm].reshape(R8, P8, D)
    Lg = (V @ phi64).transpose(0, 2, 1)
    Cw = np.exp(Lg - Lg.max(-1, keepdims=True))
    Cw /= Cw.sum(-1, keepdims=True)
    tol = 2e-5 if shift == 0.0 else 2e-4           # (|mean| = 30 sigma: the logits carry ~30 x the rounding of the dot products)
    _cmp(rep.cpu().numpy(), (Cw @ V).transpose(1, 0, 2), tol, "combine from the records")
    Dw = np.exp(Lg - Lg.max(1, keepdims=True))
    Dw /= Dw.sum(1, keepdims=True)
    mn, mx = Lg.min(-1, keepdims=True), Lg.max(-1, keepdims=True)
    _cmp(wd.cpu().numpy().reshape(R8, P8, k).transpose(0, 2, 1), (Lg - mn) / (mx - mn + 1e-8) * Dw, tol * 5,
         "dispatch weights from the records")
    # parameters NOT on 16-byte boundaries (the kernel's wide loads of gamma / beta / phi are the aligned path only): same
    # values one float further on -> same results within the reordering of two 512-term sums
    def off1(a):
        buf = torch.empty((a.numel() + 1,), device=DEV)
        buf[1:] = a.reshape(-1)
        return buf, buf[1:]
    (kg, gm1), (kb, bt1), (kp, phi1) = off1(gm), off1(bt), off1(phi)
    assert gm1.data_ptr() % 16 == 4 and phi1.data_ptr() % 16 == 4
    wd1, rep1 = torch.full_like(wd, float("nan")), torch.full_like(rep, float("nan"))
    _lib.check(lib.rrt_crmsa_combine_parts_f32(p(x1), p(part), p(gm1), p(bt1), p(phi1), p(wd1), p(rep1), L, D, k, C.byref(g8), stream()),
               "crmsa_combine_parts (unaligned parameters)")
    torch.cuda.synchronize()
    _cmp(rep1.cpu().numpy(), rep.cpu().numpy().astype(np.float64), 5e-6 if shift == 0.0 else 5e-5, "unaligned parameters: rep")
    _cmp(wd1.cpu().numpy(), wd.cpu().numpy().astype(np.float64), 5e-5 if shift == 0.0 else 5e-4, "unaligned parameters: wdisp")


@pytest.mark.parametrize("n_tokens,compute", [(5000, "bf16"), (9000, "bf16"), (9000, "f16"), (5000, "f32")])
def test_two_bags_in_flight_bit_identical_to_one(n_tokens, compute):
    """Two bags in flight through rrt_encoder_forward_f32 (two streams, two workspaces, forwards enqueued back to back so
    that the kernels of the two bags really overlap) == the same bag alone, bit for bit.  Round 5 found the mechanism of
    the round-2 'lanes 48..63' mis-sums with this loop: compiler-formed packed fp32 instructions (v_pk_fma_f32 with a
    cross-half op_sel) in a streaming kernel return run-to-run different values when the wave shares its SIMD with
    bf16-MFMA waves of the OTHER bag's kernels -- one (region, representative, 64 columns) chunk of CR-MSA's representatives
    in ~1 of 2 forwards, 1e-3 on the output.  The streaming kernels are therefore compiled without packed fp32
    (rrt-mil_amd/build.py: packed fp32 is off unless a file and a kernel are on PACKED_FP32_OK, checked by disassembly); this
    test is what failed before."""
    from hip_util import DEV
    lib = _lib.load()
    cfg = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
    from hip_util import encoder_from_state
    enc = encoder_from_state(synth.encoder_state(**cfg), cfg)
    enc._desc.compute = {"f32": _lib.COMPUTE_F32, "bf16": _lib.COMPUTE_BF16, "f16": _lib.COMPUTE_F16}[compute]
    enc._desc.solo = 0
    w = enc._weights()
    x = torch.from_numpy(synth.bag(n_tokens, 512, tag="inflight")).to(DEV)
    need = C.c_size_t()
    _lib.check(lib.rrt_encoder_workspace_size(C.byref(enc._desc), n_tokens, C.byref(need)), "workspace size")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    wss = [torch.zeros(need.value, dtype=torch.uint8, device=DEV) for _ in streams]

    def fwd(si, y, valid):
        enc._desc.weights16_valid = valid
        _lib.check(lib.rrt_encoder_forward_f32(C.byref(enc._desc), C.byref(w), x.data_ptr(), y.data_ptr(), n_tokens,
                                               wss[si].data_ptr(), wss[si].numel(), streams[si].cuda_stream), "forward")
    ref = torch.empty_like(x)
    fwd(0, ref, 0)
    torch.cuda.synchronize()
    other = torch.empty_like(x)
    fwd(1, other, 0)
    torch.cuda.synchronize()
    assert torch.equal(ref, other)
    for trial in range(3):
        ys = [torch.empty_like(x) for _ in range(12)]
        for i, y in enumerate(ys):
            fwd(i % 2, y, 1)
        torch.cuda.synchronize()
        bad = [i for i, y in enumerate(ys) if not torch.equal(y, ref)]
        assert not bad, f"trial {trial}: forwards {bad} of 12 differ from the bag alone (max {max(float((ys[i] - ref).abs().max()) for i in bad):.1e})"
    enc._desc.weights16_valid = 0


def test_bag_feeder_matches_direct_copy(tmp_path):
    """Row f3: pinned double-buffered H2D feed -- same bags, same order, same results as bag.to(device);
    accepts tensors and .pt paths (dataloader.py:181)."""
    from hip_util import encoder_from_state, DEV
    from rrt_mil_amd import BagFeeder
    cfg = dict(mlp_dim=64)
    enc = encoder_from_state(synth.encoder_state(mlp_dim=64), cfg)
    sizes = [300, 1000, 64, 777, 2000, 50, 1234]
    bags = [torch.from_numpy(synth.bag(n, 64, tag=f"feed{i}")) for i, n in enumerate(sizes)]
    path = str(tmp_path / "bag.pt")
    torch.save(bags[3].unsqueeze(0), path)          # (1, N, D) on disk, like the reference's feature files
    mixed = list(bags)
    mixed[3] = path
    want = [enc(b.to(DEV)).cpu() for b in bags]
    got = []
    for dev_bag in BagFeeder(mixed, device=DEV, depth=3):
        assert dev_bag.is_cuda and dev_bag.dtype == torch.float32
        got.append(enc(dev_bag).cpu())
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_bag_feeder_16bit_features_bit_identical_logits(dt):
    """Round 6, row f3 under --amp: BagFeeder(dtype=bf16 / fp16) ships the slide's features in 16 bits (half the PCIe bytes);
    RRTMIL under the same 16-bit arithmetic takes them as patch_to_emb's operand directly (rrt_mil_desc.input16) and returns
    logits BIT-IDENTICAL to the fp32-fed forward -- the reference's autocast rounds the fp32 features to the same values in its
    first op (modules/rrt.py:208-229 under main.py:439).  Bags whose dtype differs from the arithmetic are widened (fp32 route)."""
    from hip_util import DEV
    from rrt_mil_amd import RRTMIL, BagFeeder
    st = synth.mil_state(input_dim=1024, n_classes=2, epeg_k=15, crmsa_k=1)
    mil = RRTMIL(**load_golden("G8_rrtmil_n9000")["cfg"]).eval()
    mil.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    mil = mil.to(DEV)
    sizes = [9000, 777, 64, 3000]
    bags = [torch.from_numpy(synth.bag(n, 1024, tag=f"feed16/{i}", nonneg=True)) for i, n in enumerate(sizes)]
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        want = [mil(b.to(DEV).unsqueeze(0)).float().cpu() for b in bags]
        got = []
        for dev_bag in BagFeeder(bags, device=DEV, depth=3, dtype=dt):
            assert dev_bag.is_cuda and dev_bag.dtype == dt
            got.append(mil(dev_bag.unsqueeze(0)).float().cpu())
        stored = [b.to(dt) for b in bags]                       # feature files already stored in 16 bits, pinned
        got2 = [mil(d.unsqueeze(0)).float().cpu() for d in BagFeeder([s_.pin_memory() for s_ in stored], device=DEV, dtype=dt)]
        other = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
        wide = mil(bags[1].to(other).to(DEV).unsqueeze(0)).float().cpu()     # 16-bit bag of the OTHER type: widened, fp32 route
    for a, b, c in zip(got, want, got2):
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(c, b)
    assert torch.isfinite(wide).all() and (wide - want[1]).abs().max() <= 3e-2 * max(1.0, float(want[1].abs().max()))
    # the C ABI refuses 16-bit features that do not match the arithmetic
    lib = _lib.load()
    d = mil._mil_desc(1024)
    d.enc.compute, d.input16 = _lib.COMPUTE_F32, _lib.COMPUTE_BF16
    need = C.c_size_t()
    _lib.check(lib.rrt_mil_workspace_size(C.byref(d), 64, C.byref(need)), "ws")
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    x16 = torch.zeros(64, 1024, dtype=torch.bfloat16, device=DEV)
    out = torch.empty(2, device=DEV)
    w = mil._mil_weights()
    rc = lib.rrt_mil_forward_f32(C.byref(d), C.byref(w), x16.data_ptr(), out.data_ptr(), None, 0, None, 64, ws.data_ptr(),
                                 ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == -2


# ------------------------------------------------------------------ row f2 building blocks (backward stages)
@pytest.mark.parametrize("S,n,scatter", [(512, 1024, None), (512, 2560, (1024, 512, 3)), (64, 120, None), (1, 32, None),
                                         (3, 7, None), (2250, 1026, None), (16, 786432, None), (130, 4 + 5 * 96, (4, 96, 5)),
                                         (48, 33, None)])
def test_reduce_partials_immediate_and_deferred(S, n, scatter):
    """out[i] = sum_s part[s][i] in a fixed order: the stage's own launch and the backward's deferred job list (one launch,
    here with the job queued three times), against float64; ragged lengths, one partial, the transposed tail (CR-MSA's
    d phi), unaligned outputs; twice in a row bit for bit."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    part = synth.normal(f"rp/{S}x{n}", (S, n))
    want = part.astype(np.float64).sum(0)
    d_part = dev(part)
    tol = 2e-6 * np.sqrt(S) * 4
    split, trd, trk = scatter if scatter else (0, 0, 0)

    def check(out, out_tr, what):
        got = out.cpu().numpy().astype(np.float64)
        if scatter:
            np.testing.assert_allclose(got[:split], want[:split], rtol=0, atol=tol, err_msg=what)
            gt = out_tr.cpu().numpy().astype(np.float64)                    # [tr_dim, tr_k]
            np.testing.assert_allclose(gt, want[split:].reshape(trk, trd).T, rtol=0, atol=tol, err_msg=what + " (tail)")
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=tol, err_msg=what)

    for off in (0, 1):                                                      # off = 1: an output that takes no 16-byte stores
        if off and scatter:
            continue                                                        # (the scatter form needs an aligned head, api.hip)
        if not off:                                                         # immediate (the stage launch stores float4s: aligned outputs only)
            out = torch.full((n,), float("nan"), device=DEV)
            out_tr = torch.full((trd, trk), float("nan"), device=DEV) if scatter else None
            _lib.check(lib.rrt_reduce_partials_f32(p(d_part), out.data_ptr(), out_tr.data_ptr() if scatter else None, S, n,
                                                   split, trd, trk, 0, 1, stream()), "reduce_partials immediate")
            torch.cuda.synchronize()
            check(out, out_tr, "immediate")
        # deferred, three copies of the job in one launch
        runs = []
        for rep in range(2):
            buf3 = torch.full((3 * n + 4,), float("nan"), device=DEV)
            o3 = buf3[off:off + 3 * n]
            t3 = torch.full((3, trd, trk), float("nan"), device=DEV) if scatter else None
            _lib.check(lib.rrt_reduce_partials_f32(p(d_part), o3.data_ptr(), t3.data_ptr() if scatter else None, S, n, split,
                                                   trd, trk, 1, 3, stream()), "reduce_partials deferred")
            torch.cuda.synchronize()
            for c in range(3):
                check(o3[c * n:(c + 1) * n], t3[c] if scatter else None, f"deferred copy {c} (offset {off})")
            if scatter:
                assert torch.isnan(o3[split:n]).all()                       # the head buffer's tail is not written
            runs.append((o3.clone(), t3.clone() if scatter else None))
        assert torch.equal(runs[0][0].nan_to_num(7.0), runs[1][0].nan_to_num(7.0))
        if scatter:
            assert torch.equal(runs[0][1], runs[1][1])
    assert lib.rrt_reduce_partials_f32(p(d_part), None, None, S, n, 0, 0, 0, 1, 1, stream()) == -1
    assert lib.rrt_reduce_partials_f32(p(d_part), p(d_part), None, S, n, 0, 0, 0, 1, 17, stream()) == -1


@pytest.mark.parametrize("M,N,K", [(9216, 1536, 512), (9216, 512, 512), (192, 1536, 512), (192, 512, 512),
                                   (1000, 160, 96), (300, 192, 64), (3136, 512, 2048), (77, 32, 40)])
def test_linear_backward(M, N, K):
    """nn.Linear backward (dX = dY W, dW = dY^T X on the split-K TN kernel, db = colsum dY) against float64."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    dY = synth.normal(f"lb/dy{M}x{N}", (M, N))
    X = synth.normal(f"lb/x{M}x{K}", (M, K))
    W = synth.uniform(f"lb/w{N}x{K}", (N, K), -1, 1) / np.sqrt(K)
    d_dY, d_X, d_W = dev(dY), dev(X), dev(W)
    dX = torch.full((M, K), float("nan"), device=DEV)
    dW = torch.full((N, K), float("nan"), device=DEV)
    db = torch.full((N,), float("nan"), device=DEV)
    need = C.c_size_t()
    _lib.check(lib.rrt_linear_backward_workspace_size(M, N, K, C.byref(need)), "ws")
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rrt_linear_backward_f32(p(d_dY), p(d_X), p(d_W), p(dX), p(dW), p(db), M, N, K, 0, p(ws),
                                           ws.numel(), stream()), "linear_backward")
    torch.cuda.synchronize()
    dY64, X64, W64 = dY.astype(np.float64), X.astype(np.float64), W.astype(np.float64)
    _cmp(dX.cpu().numpy(), dY64 @ W64, 3e-5, "dX")
    scale = np.sqrt(M)                       # sums of M products of N(0,1) variables
    _cmp(dW.cpu().numpy() / scale, dY64.T @ X64 / scale, 3e-5, "dW")
    _cmp(db.cpu().numpy() / scale, dY64.sum(0) / scale, 3e-5, "db")
    # optional outputs
    _lib.check(lib.rrt_linear_backward_f32(p(d_dY), p(d_X), p(d_W), None, p(dW), None, M, N, K, 0, p(ws),
                                           ws.numel(), stream()), "linear_backward dW only")
    torch.cuda.synchronize()
    _cmp(dW.cpu().numpy() / scale, dY64.T @ X64 / scale, 3e-5, "dW only")


def _ln_bwd64(dy, x, gamma, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps)
    xh = (x - mu) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdims=True) - xh * (g * xh).mean(-1, keepdims=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


@pytest.mark.parametrize("L,D,rn", [(9000, 512, 8), (300, 64, 8), (1, 512, 8), (4096, 1024, 8), (30000, 512, 16)])
def test_layernorm_backward(L, D, rn):
    """LayerNorm backward, plain and with the upstream gradient in region-major padded order + residual."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    x = synth.normal(f"lnb/x{L}x{D}", (L, D)) * 1.7 + 0.3
    dy = synth.normal(f"lnb/dy{L}x{D}", (L, D))
    gamma = (1.0 + synth.uniform(f"lnb/g{D}", (D,), -0.25, 0.25)).astype(np.float32)
    add = synth.normal(f"lnb/add{L}x{D}", (L, D))
    dx64, dg64, db64 = _ln_bwd64(dy.astype(np.float64), x.astype(np.float64), gamma.astype(np.float64))
    d_x, d_dy, d_g, d_add = dev(x), dev(dy), dev(gamma), dev(add)
    ws = torch.full((512 * 2 * D * 4,), 0xFF, dtype=torch.uint8, device=DEV)
    dx = torch.full((L, D), float("nan"), device=DEV)
    dgb = torch.full((2, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_layernorm_backward_f32(p(d_dy), p(d_x), p(d_g), None, p(dx), p(dgb), L, D, None, p(ws),
                                              ws.numel(), stream()), "ln_backward")
    torch.cuda.synchronize()
    scale = max(1.0, np.sqrt(L))
    _cmp(dx.cpu().numpy(), dx64, 2e-5, "dx")
    _cmp(dgb[0].cpu().numpy() / scale, dg64 / scale, 2e-5, "dgamma")
    _cmp(dgb[1].cpu().numpy() / scale, db64 / scale, 2e-5, "dbeta")
    # region-major upstream gradient (adjoint of zero-pad + partition) + residual gradient
    g = _lib.region_grid(L, rn)
    Np = g.H * g.H
    dU = synth.normal(f"lnb/du{Np}x{D}", (Np, D))               # pad slots hold garbage that must be ignored
    perm = O.partition_index(g.H, g.s)                          # perm[slot] = token
    dy_tok = np.empty((Np, D), np.float32)
    dy_tok[perm] = dU
    dx64, dg64, db64 = _ln_bwd64(dy_tok[:L].astype(np.float64), x.astype(np.float64), gamma.astype(np.float64))
    d_dU = dev(dU)
    _lib.check(lib.rrt_layernorm_backward_f32(p(d_dU), p(d_x), p(d_g), p(d_add), p(dx), p(dgb), L, D, C.byref(g),
                                              p(ws), ws.numel(), stream()), "ln_backward mapped")
    torch.cuda.synchronize()
    _cmp(dx.cpu().numpy(), dx64 + add, 2e-5, "dx mapped + residual")
    _cmp(dgb[0].cpu().numpy() / scale, dg64 / scale, 2e-5, "dgamma mapped")
    _cmp(dgb[1].cpu().numpy() / scale, db64 / scale, 2e-5, "dbeta mapped")


@pytest.mark.parametrize("R,P,D,heads,ek", [(3, 144, 512, 8, 15), (2, 121, 512, 8, 21), (4, 64, 512, 8, 0),
                                            (5, 49, 512, 8, 15), (2, 100, 256, 4, 9), (3, 130, 512, 8, 0),
                                            (64, 144, 512, 8, 15), (2, 7, 128, 2, 15), (3, 81, 512, 8, 31),
                                            (3, 169, 512, 8, 15), (2, 196, 512, 8, 21), (2, 208, 512, 8, 0),
                                            (3, 177, 256, 4, 9),
                                            # streaming variant: regions beyond the resident kernel's 208 tokens
                                            (2, 256, 512, 8, 15), (2, 225, 512, 8, 21), (3, 240, 512, 8, 0), (1, 484, 512, 8, 21), (2, 324, 256, 4, 0),
                                            (3, 209, 512, 8, 9),
                                            # generic head dims (crmsa_heads = 1: head dim = dim), no EPEG
                                            (3, 64, 512, 1, 0), (5, 64, 512, 2, 0), (3, 64, 96, 1, 0), (1, 100, 64, 8, 0)])
def test_region_attention_backward(R, P, D, heads, ek):
    """Attention backward (recomputed probabilities, EPEG adjoint, tap gradients) against float64 autograd of the
    explicit formulation (scores [P,P], depth-wise conv along the query axis WITH a bias, softmax, A V)."""
    from hip_util import dev, p, stream, DEV, region_attention
    lib = _lib.load()
    hd = D // heads
    raw = synth.normal(f"ab/qkv{R}x{P}x{D}", (R * P, 3 * D)) * 0.6
    pe = synth.uniform("ab/pe", (heads, max(ek, 1)), -1, 1) / np.sqrt(max(ek, 1))
    pb = synth.uniform("ab/pb", (heads,), -0.3, 0.3)
    dO = synth.normal(f"ab/do{R}x{P}x{D}", (R * P, D))
    stash = raw.copy()
    stash[:, :D] *= hd ** -0.5                       # the forward stage stores q already scaled
    # float64 autograd oracle
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
    # HIP: forward output from the forward stage, then the backward stage
    d_stash, d_pe, d_dO = dev(stash), dev(pe), dev(dO)
    o = region_attention(d_stash, d_pe if ek else None, R, P, D, heads, ek)
    _cmp(o.cpu().numpy(), Oref.detach().numpy(), 5e-5, "forward O")
    dqkv = torch.full((R * P, 3 * D), float("nan"), device=DEV)
    dpe = torch.full((heads, max(ek, 1)), float("nan"), device=DEV)
    need = C.c_size_t()
    _lib.check(lib.rrt_region_attention_backward_workspace_size(R, P, D, heads, ek, C.byref(need)), "attn bwd ws")
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rrt_region_attention_backward_f32(p(d_stash), p(d_pe) if ek else None, p(o), p(d_dO), p(dqkv),
                                                     p(dpe) if ek else None, R, P, D, heads, ek, p(ws), ws.numel(),
                                                     stream()), "attention_backward")
    torch.cuda.synchronize()
    got, ref = dqkv.cpu().numpy(), tq.grad.numpy()
    _cmp(got[:, :D], ref[:, :D], 1e-4, "dq")
    _cmp(got[:, D:2 * D], ref[:, D:2 * D], 1e-4, "dk")
    _cmp(got[:, 2 * D:], ref[:, 2 * D:], 1e-4, "dv")
    if ek:
        scale = max(1.0, np.sqrt(R * P))
        _cmp(dpe.cpu().numpy() / scale, tw.grad.numpy() / scale, 1e-4, "d taps")
        assert np.abs(tb.grad.numpy()).max() < 1e-9 * R * P          # Identity 2: the bias gradient is zero


# ------------------------------------------------------------------ 16-bit operand path of the bf16 / fp16 modes
_DT16 = {1: torch.bfloat16, 2: torch.float16}


def _to16(a, compute):
    """fp32 numpy -> device int16 tensor holding the bf16 / fp16 bits (RNE), and the rounded values as float64"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_DT16[compute])
    return t.view(torch.int16).to("cuda:0"), t.double().numpy()


def _from16(bits, compute):
    return bits.view(_DT16[compute]).double().cpu().numpy()


@pytest.mark.parametrize("compute", [1, 2])
def test_cast16_and_ln_partition16(compute):
    """cast16 is torch's round-to-nearest-even cast bit for bit; ln_partition16 is the fp32 LayerNorm + pad + partition
    stage with its rows rounded once (a value that sits next to a rounding boundary may land on the other side of it
    than the float64 restatement: at most one 16-bit ulp, on a small fraction of the elements)."""
    from hip_util import dev, p, stream
    lib = _lib.load()
    w = synth.uniform("c16/w", (1536, 512), -1, 1) * np.exp(synth.uniform("c16/e", (1536, 512), -12, 4))
    out = torch.empty((1536, 512), dtype=torch.int16, device="cuda:0")
    wd = dev(w)                                   # (device buffers are kept alive across the asynchronous call)
    _lib.check(lib.rrt_cast16(p(wd), p(out), w.size, compute, stream()), "cast16")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(w).to(_DT16[compute]).view(torch.int16))
    # bag-sized jobs (round 5: the classifier's feature matrix goes through this kernel): one trip of four loads per thread
    # with a ragged last load, and a job larger than the grid's cap (several trips); the canary behind the end stays
    for n in (9000 * 1024, 4 * (4096 * 256 * 4 + 12345), 4 * 777):
        v = synth.uniform(f"c16/big{n}", (n,), -4, 4)
        vd = dev(v)
        o16 = torch.full((n + 8,), 0x7FC0, dtype=torch.int16, device="cuda:0")
        _lib.check(lib.rrt_cast16(p(vd), p(o16), n, compute, stream()), "cast16 (bag-sized)")
        torch.cuda.synchronize()
        assert torch.equal(o16[:n].cpu(), torch.from_numpy(v).to(_DT16[compute]).view(torch.int16))
        assert (o16[n:] == 0x7FC0).all()
    for L, rn, D in ((9000, 8, 512), (700, 8, 128), (30000, 16, 512)):
        x = synth.bag(L, D, tag="lnp16")
        gm, bt = 1.0 + synth.uniform("lnp16/g", (D,), -0.3, 0.3), synth.uniform("lnp16/b", (D,), -0.2, 0.2)
        g = _lib.region_grid(L, rn)
        u = torch.full((g.H * g.H, D), 0x7FC0, dtype=torch.int16, device="cuda:0")
        xd, gd_, bd_ = dev(x), dev(gm), dev(bt)
        _lib.check(lib.rrt_ln_partition16(p(xd), p(gd_), p(bd_), p(u), L, D, g, compute, stream()), "lnp16")
        torch.cuda.synchronize()
        got = _from16(u, compute)
        x64 = x.astype(np.float64)
        ln = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + 1e-5) * gm + bt
        ref = np.zeros((g.H * g.H, D))
        ref[:L] = ln
        ref = O.round_lowp(ref[O.partition_index(g.H, g.s)], "bf16" if compute == 1 else "f16")
        ulp = 2.0 ** (-7 if compute == 1 else -10)
        diff = np.abs(got - ref)
        assert (diff <= ulp * np.maximum(np.abs(ref), 1e-3)).all()
        assert (diff > 0).mean() < 0.01
        assert (got[np.abs(ref).sum(-1) == 0] == 0).all()          # pad slots: exact zeros


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("M,N,K", [(9216, 512, 512), (9216, 1536, 512), (3136, 512, 512), (1000, 192, 128), (9216, 512, 1024)])
def test_linear16(M, N, K, compute):
    """C = A16 . B16^T + bias on operands that ARE 16-bit in HBM: against the float64 product of exactly those values
    (only the fp32 accumulation differs)."""
    from hip_util import dev, p, stream
    lib = _lib.load()
    A16, A = _to16(synth.normal(f"l16/A{M}x{K}", (M, K)), compute)
    B16, B = _to16(synth.uniform(f"l16/B{N}x{K}", (N, K), -1, 1) / np.sqrt(K), compute)
    bias = synth.uniform("l16/b", (N,), -0.1, 0.1)
    C_ = torch.full((M, N), float("nan"), device="cuda:0")
    bd_ = dev(bias)
    _lib.check(lib.rrt_linear16_f32(p(A16), p(B16), p(bd_), None, p(C_), M, N, K, None, compute, stream()), "linear16")
    torch.cuda.synchronize()
    _cmp(C_.cpu().numpy(), A @ B.T + bias, 2e-5, f"linear16 {M}x{N}x{K}")


# (one size per rung of launch_linear16's row-count ladder: 64 / 96 / 144-row tiles, 128 x 128, 144 x 128, 128-row rounds)
@pytest.mark.parametrize("L,rn", [(9000, 8), (30000, 16), (3000, 8), (7000, 8), (10500, 8), (12000, 8), (15000, 8), (17000, 8), (20000, 16)])
def test_linear16_unpartition_residual(L, rn):
    from hip_util import dev, p, stream
    lib = _lib.load()
    D = 512
    g = _lib.region_grid(L, rn)
    Np = g.H * g.H
    A16, A = _to16(synth.normal("l16u/A", (Np, D)), 1)
    B16, B = _to16(synth.uniform("l16u/B", (D, D), -1, 1) / np.sqrt(D), 1)
    bias, resid = synth.uniform("l16u/b", (D,), -0.1, 0.1), synth.bag(L, D, tag="l16u/r")
    out = torch.full((L, D), float("nan"), device="cuda:0")
    bd_, rd_ = dev(bias), dev(resid)
    _lib.check(lib.rrt_linear16_f32(p(A16), p(B16), p(bd_), p(rd_), p(out), Np, D, D, g, 1, stream()), "linear16 unpart")
    torch.cuda.synchronize()
    z = np.empty((Np, D))
    z[O.partition_index(g.H, g.s)] = A @ B.T + bias
    _cmp(out.cpu().numpy(), resid + z[:L], 2e-5, "linear16 un-partition + residual")


@pytest.mark.parametrize("L,rn,ek,compute", [(30000, 16, 15, 1), (30000, 16, 15, 2), (29000, 16, 21, 1), (17000, 16, 15, 1),
                                             (20000, 16, 0, 1), (26000, 16, 15, 1)])
def test_rmsa_pair16_proj(L, rn, ek, compute):
    """Round 6: the 16-bit R-MSA core and its out-projection + un-partition + residual in ONE launch (rmsa_pair16_kernel<..,
    PROJ>: block b runs item b, then the projection slab of a region pair whose items finished a round earlier) against the
    two launches it replaces (rrt_rmsa_fused16, rrt_linear16_f32 with the residual): O and x1 bit for bit -- also on scratch
    full of NaN patterns, twice in a row (counters, stale lines), and with a ragged tail (L < Np)."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    D, heads = 512, 8
    g = _lib.region_grid(L, rn)
    Np, P, R = g.H * g.H, g.s * g.s, rn * rn
    u16, _ = _to16(synth.normal(f"p16p/u{L}", (Np, D)), compute)
    w16, _ = _to16(synth.uniform("p16p/w", (3 * D, D), -1, 1) / np.sqrt(D) * 1.5, compute)
    wp16, _ = _to16(synth.uniform("p16p/wp", (D, D), -1, 1) / np.sqrt(D), compute)
    b, bp = synth.uniform("p16p/b", (3 * D,), -0.2, 0.2), synth.uniform("p16p/bp", (D,), -0.1, 0.1)
    pe = synth.uniform("p16p/pe", (heads, ek), -0.3, 0.3) if ek else None
    resid = dev(synth.bag(L, D, tag="p16p/r"))
    bd_, bpd_, ped_ = dev(b), dev(bp), (dev(pe) if ek else None)
    o_ref = torch.full((Np, D), 0x7FC0, dtype=torch.int16, device=DEV)
    x_ref = torch.full((L, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_rmsa_fused16(p(u16), p(w16), p(bd_), p(ped_), p(o_ref), R, P, D, heads, ek, compute, stream()), "fused16")
    _lib.check(lib.rrt_linear16_f32(p(o_ref), p(wp16), p(bpd_), p(resid), p(x_ref), Np, D, D, g, compute, stream()), "linear16")
    torch.cuda.synchronize()
    assert torch.isfinite(x_ref).all()
    cnt = torch.full((R,), 12345, dtype=torch.int32, device=DEV)
    for rep in range(2):
        o = torch.full((Np, D), 0x7FC0, dtype=torch.int16, device=DEV)
        x1 = torch.full((L, D), float("nan"), device=DEV)
        rc = lib.rrt_rmsa_pair16_proj(p(u16), p(w16), p(bd_), p(ped_), p(wp16), p(bpd_), p(resid), p(x1), p(o), p(cnt), D, heads, ek,
                                      C.byref(g), compute, stream())
        _lib.check(rc, "rmsa_pair16_proj")
        torch.cuda.synchronize()
        assert lib.rrt_device_error(0) == 0
        assert torch.equal(o, o_ref), f"O differs (rep {rep})"
        assert torch.equal(x1, x_ref), f"x1 differs (rep {rep}): {float((x1 - x_ref).abs().nan_to_num(1e9).max())}"


def test_rmsa_pair16_proj_refuses_small_bags():
    """One round of items (N = 9000 at region_num = 8: 256 items) has no round behind which a slab could run: unsupported."""
    from hip_util import p, stream, DEV
    lib = _lib.load()
    g = _lib.region_grid(9000, 8)
    z = torch.zeros(16, device=DEV)
    rc = lib.rrt_rmsa_pair16_proj(p(z), p(z), None, None, p(z), None, p(z), p(z), p(z), p(z), 512, 8, 15, C.byref(g), 1, stream())
    assert rc == -2


@pytest.mark.parametrize("dtype,mix", [("bf16", "0"), ("bf16", "1"), ("f32", "0")])
def test_soak_bags_in_flight_short(dtype, mix):
    """Round 6 (review item 6): a SHORT soak in the suite -- tools/soak_merged.py in its own process (its own stream -> hardware
    queue map), four bags of different sizes in flight on four streams, 30 rounds x 16 forwards, every output bit for bit
    against the solo result of its (stream, size).  mix = 1: stream 0 runs exact-fp32 one-bag-in-flight forwards
    (crmsa_combine_parts_kernel) beside the 16-bit bags -- the setting in which compiler-formed packed fp32 instructions
    mis-summed: with the build's packed-fp32 census this is the run-time half of that guard."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SOAK_DTYPE=dtype, SOAK_MIX=mix, GPU_MAX_HW_QUEUES="16")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "soak_merged.py"), "30", "4"], capture_output=True, text=True,
                         env=env, timeout=300)
    assert out.returncode == 0 and " 0 differ" in out.stdout, (out.stdout[-400:], out.stderr[-400:])


def _fused16_ref(u, w, b, pe_w, R, P, D, heads, ek, dt, pair=False):
    """float64 restatement of rmsa_fused16's rounding points on the given (already 16-bit) u, w: -> O (unrounded).
    pair: the two-regions-per-block kernel (rmsa_pair16: Q rounded before the matrix-core stencil, taps as hi + lo)"""
    st = {"qkv.weight": w, "proj.weight": np.eye(D), "proj.bias": np.zeros(D)}
    if b is not None:
        st["qkv.bias"] = b
    if pe_w is not None:
        st["pe.weight"] = pe_w.reshape(heads, 1, ek, 1)

    class NoRound:                                 # u / w are exact already; O is compared before its rounding
        r = staticmethod(lambda a: a)
    return O._inner_attention64(u.reshape(R, P, D), st, "", heads, ek, None, NoRound, O.LowP(dt, True, stencil16=pair)).reshape(R * P, D)


@pytest.mark.parametrize("R,P,D,heads,ek,compute", [(64, 144, 512, 8, 15, 1), (64, 144, 512, 8, 15, 2), (9, 121, 512, 8, 15, 1),
                                                    (5, 196, 512, 8, 21, 1), (7, 169, 512, 8, 15, 1), (3, 100, 512, 8, 9, 1),
                                                    (12, 81, 512, 8, 15, 1), (20, 49, 512, 8, 15, 1), (6, 25, 512, 8, 15, 1),
                                                    (4, 64, 256, 4, 0, 1), (3, 208, 512, 8, 63, 1), (2, 130, 1024, 16, 15, 2),
                                                    (256, 121, 512, 8, 15, 1), (5, 225, 512, 8, 21, 1), (4, 256, 512, 8, 15, 1),
                                                    (3, 256, 512, 8, 15, 2), (2, 233, 512, 8, 9, 1),
                                                    # rmsa_pair16 (>= 8 regions of <= 176 tokens): odd region counts, every
                                                    # row-tile count, one / two / three stencil steps, no EPEG
                                                    (8, 169, 512, 8, 21, 1), (10, 176, 512, 8, 15, 2), (16, 100, 512, 8, 31, 1),
                                                    (9, 64, 512, 8, 63, 1), (8, 144, 512, 8, 0, 1), (11, 30, 512, 8, 15, 1),
                                                    (8, 130, 1024, 16, 15, 2), (13, 112, 512, 8, 17, 1), (64, 144, 512, 8, 21, 1)])
def test_rmsa_fused16(R, P, D, heads, ek, compute):
    """The 16-bit fused R-MSA kernel against a float64 restatement with the SAME rounding points (Q~ log2e, K, V and
    exp2(S - max) rounded to 16 bits; everything else exact), on inputs that are exactly representable: what is left
    is fp32 accumulation order and values that sit on a rounding boundary."""
    from hip_util import dev, p, stream
    lib = _lib.load()
    dt = "bf16" if compute == 1 else "f16"
    u16, u = _to16(synth.normal(f"f16/u{R}x{P}", (R * P, D)), compute)
    w16, w = _to16(synth.uniform("f16/w", (3 * D, D), -1, 1) / np.sqrt(D) * 1.5, compute)
    b = synth.uniform("f16/b", (3 * D,), -0.2, 0.2)
    pe = synth.uniform("f16/pe", (heads, ek), -0.3, 0.3) if ek else None
    o16 = torch.full((R * P, D), 0x7FC0, dtype=torch.int16, device="cuda:0")
    bd_, ped_ = dev(b), (dev(pe) if ek else None)
    _lib.check(lib.rrt_rmsa_fused16(p(u16), p(w16), p(bd_), p(ped_), p(o16), R, P, D, heads, ek, compute, stream()),
               "rmsa_fused16")
    torch.cuda.synchronize()
    got = _from16(o16, compute)
    Rr = min(R, 8)                                                # float64 restatement of the first regions
    pair = R >= 8 and 16 < P <= 176                               # the library's choice (rmsa_pair16_supported)
    ref = _fused16_ref(u[:Rr * P], w, b, pe, Rr, P, D, heads, ek, dt, pair)
    if pair and R > Rr:                                           # ... and the LAST regions (odd counts: the half-empty pair)
        ref = np.concatenate([ref, _fused16_ref(u[(R - 3) * P:], w, b, pe, 3, P, D, heads, ek, dt, pair)])
        got = np.concatenate([got[:Rr * P], got[(R - 3) * P:]])
    got = got[:ref.shape[0]]
    assert np.isfinite(_from16(o16, compute)).all()
    ulp = 2.0 ** (-8 if compute == 1 else -11)                    # half a 16-bit ulp, relative
    err = np.abs(got - ref)
    scale = np.abs(ref).max()
    # the final rounding of O accounts for <= ulp * |O|; rounding-boundary flips of individual probabilities / Q~
    # entries add a little on top
    assert (err <= 1.01 * ulp * np.abs(ref) + 4e-3 * ulp * 256 * scale).all(), (err.max(), scale)
    assert err.mean() <= 0.6 * ulp * np.abs(ref).mean() + 1e-6


@pytest.mark.parametrize("name,dt", [("G16_amp_bf16_d512_n9000", torch.bfloat16), ("G16_amp_bf16_d512_n1000", torch.bfloat16),
                                     ("G16_amp_f16_d512_n1000", torch.float16), ("G16_amp_bf16_d512_n9000_c1_sc", torch.bfloat16),
                                     ("G16_amp_bf16_d512_n3000_k21_c5", torch.bfloat16),
                                     ("G16_amp_bf16_d512_n15000_k21_c5", torch.bfloat16),
                                     ("G16_amp_bf16_d512_n30000_rn16", torch.bfloat16)])
def test_encoder_amp_against_restatement_and_reference_autocast(name, dt):
    """BASELINE configs[2..4] arithmetic.  (1) TIGHT: the HIP encoder under autocast against the float64 restatement of
    its own rounding points (oracle forward_f64(lowp=...)): a mis-rounded or skipped stage shows up here.
    (2) The reference's own autocast run (G16 fixtures: the real reference under torch.autocast('cpu', dtype)): the
    HIP result is at least as close to the fp32 reference as that run is, and within 1.25x that distance of it."""
    from hip_util import encoder_from_state, dev
    g = load_golden(name)
    x, st, cfg = synth_case(g)
    N = int(g["n"])
    enc = encoder_from_state(st, cfg)
    with torch.autocast("cuda", dtype=dt):
        y = enc(dev(x).unsqueeze(0)).squeeze(0)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32
    y = y.cpu().numpy().astype(np.float64)
    rows = g["rows"]
    H, s_, _ = O.grid(N, cfg.get("region_num", 8))
    fused16 = 16 < s_ * s_ <= 256
    if N <= 9000:
        ref = O.forward_f64(x, st, cfg, lowp=O.LowP("bf16" if dt == torch.bfloat16 else "f16", attn=fused16))
        d = np.abs(y - ref)
        # (round 3: 8e-4 instead of 6e-4 -- the pair kernel rounds Q before the stencil and the representatives' attention
        #  runs on 16-bit operands too: more places where an fp32-vs-float64 accumulation difference flips a rounding)
        tol = (8e-4, 3e-5) if dt == torch.bfloat16 else (1.2e-4, 5e-6)
        assert d.max() <= tol[0] and d.mean() <= tol[1], (d.max(), d.mean())
    to_fp32 = np.abs(y[rows] - g["y32_rows"])
    to_amp = np.abs(y[rows] - g["y_rows"])
    amp_to_fp32 = np.abs(g["y_rows"].astype(np.float64) - g["y32_rows"])
    assert to_fp32.mean() <= amp_to_fp32.mean() and to_fp32.max() <= 1.1 * amp_to_fp32.max(), (to_fp32.max(), amp_to_fp32.max())
    assert to_amp.max() <= 1.25 * amp_to_fp32.max() and to_amp.mean() <= 1.25 * amp_to_fp32.mean()
    assert to_fp32.max() > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [torch.bfloat16, "f32x3"])
def test_weight_image_cache_follows_the_parameters(mode):
    """The 16-bit weight images of the reduced-precision modes are kept in the workspace between forwards
    (rrt_encoder_desc.weights16_valid; rrt_mil_amd tracks parameter versions): a cached call is bit-identical to an
    uncached one, and a weight update -- an optimizer-style in-place op -- is picked up by the next forward."""
    from hip_util import encoder_from_state, dev
    g = load_golden("G3_d512_n9000")
    x, st, cfg = synth_case(g)
    xb = dev(x[:3000]).unsqueeze(0)
    enc = encoder_from_state(st, cfg)
    enc.compute_dtype = mode
    enc.solo = False                   # (the executor below runs two streams: same scheduling hint, same kernels, same bits)
    y1 = enc(xb).clone()
    assert enc._w16_key is not None
    y2 = enc(xb).clone()                                  # second call: conversion skipped
    assert torch.equal(y1, y2)
    with torch.no_grad():
        list(enc.layers.children())[0].attn.attn.qkv.weight.mul_(1.25)
    y3 = enc(xb).clone()
    fresh = encoder_from_state({k: (v * 1.25 if k == "layers.0.attn.attn.qkv.weight" else v) for k, v in st.items()}, cfg)
    fresh.compute_dtype = mode
    fresh.solo = False
    y4 = fresh(xb)
    torch.cuda.synchronize()
    assert torch.equal(y3, y4) and not torch.equal(y3, y1)
    # executor path (forward_bags): versions ride in rrt_encoder_weights.version
    a = enc.forward_bags([xb, xb], streams=2)
    b = enc.forward_bags([xb, xb], streams=2)
    torch.cuda.synchronize()
    assert torch.equal(a[0], y3) and torch.equal(b[1], y3)


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers", [2, 1])
def test_weight_image_cache_follows_the_crmsa_parameters(n_layers):
    """Round-3 advisor finding (high): CR-MSA's inner qkv / proj weights have cached 16-bit images too, but the validity
    fingerprint covered the R-MSA layers only -- an update of a cr_msa weight alone (frozen R-MSA layers), or ANY update
    at n_layers = 1 (no R-MSA layer: the fingerprint was the empty tuple), left the inner MSA on the first call's
    weights.  The fingerprint now covers every parameter of the encoder; module path and executor path."""
    from hip_util import encoder_from_state, dev
    cfg = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8, n_layers=n_layers)
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k != "region_num"})
    xb = dev(synth.bag(3000, 512, tag="w16/crmsa")).unsqueeze(0)

    def make(state):
        e = encoder_from_state(state, cfg)
        e.compute_dtype = torch.bfloat16
        e.solo = False
        return e
    enc = make(st)
    y1 = enc(xb).clone()
    assert torch.equal(enc(xb), y1) and enc._w16_key is not None          # cached images, same bits
    for name in ("cr_msa.attn.attn.qkv.weight", "cr_msa.attn.attn.proj.weight"):
        with torch.no_grad():
            dict(enc.named_parameters())[name].mul_(1.5)
        st = {k: (v * 1.5 if k == name else v) for k, v in st.items()}
        y2 = enc(xb).clone()
        want = make(st)(xb)
        torch.cuda.synchronize()
        assert torch.equal(y2, want) and not torch.equal(y2, y1), name
        outs = enc.forward_bags([xb, xb], streams=2)                      # executor: rrt_encoder_weights.version
        torch.cuda.synchronize()
        assert torch.equal(outs[0], want) and torch.equal(outs[1], want), name
        y1 = y2
    # a NEW Parameter object assigned to an existing submodule is seen as well (its data_ptr differs)
    enc.cr_msa.attn.attn.proj.weight = torch.nn.Parameter(enc.cr_msa.attn.attn.proj.weight.detach() * 0.5)
    st = {k: (v * 0.5 if k == "cr_msa.attn.attn.proj.weight" else v) for k, v in st.items()}
    y3 = enc(xb)
    want = make(st)(xb)
    torch.cuda.synchronize()
    assert torch.equal(y3, want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,big", [(torch.bfloat16, 20000), ("f32x3", 10500), ("f32x3", 20000)])
def test_weight_image_cache_survives_a_bag_that_skips_the_16bit_kernels(mode, big):
    """Round-2 advisor finding: the validity key of the cached weight images did not say whether the call had written
    them.  A bag whose regions the 16-bit / split kernels do not cover (N = 20000: P = 324; f32x3 also N = 10500:
    P = 169) used to cast nothing, mark the cache valid, and let the next small bag on the SAME workspace read
    uninitialised images.  Now every reduced-mode call writes them unless told they are valid."""
    from hip_util import DEV, encoder_from_state, dev
    g = load_golden("G3_d512_n9000")
    x, st, cfg = synth_case(g)
    fresh = encoder_from_state(st, cfg)
    fresh.compute_dtype = mode
    want = fresh(dev(x).unsqueeze(0)).clone()
    enc = encoder_from_state(st, cfg)
    enc.compute_dtype = mode
    enc._desc.compute = enc._compute_mode()
    enc._workspace(big, torch.device(DEV)).fill_(0xFF)                      # NaN-poisoned workspace: no image in it
    yb = enc(dev(synth.bag(big, 512, tag="w16/big")).unsqueeze(0))          # first call on this encoder: the big bag
    assert torch.isfinite(yb).all()
    y = enc(dev(x).unsqueeze(0))                                             # same (larger) workspace, supported P
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    # executor: one stream, big bag first
    ex = encoder_from_state(st, cfg)
    ex.compute_dtype = mode
    outs = ex.forward_bags([dev(synth.bag(big, 512, tag="w16/big")), dev(x)], streams=1)
    outs2 = ex.forward_bags([dev(x)], streams=1)
    torch.cuda.synchronize()
    assert torch.equal(outs[1], want[0]) and torch.equal(outs2[0], want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,dim", [("f32", 512), ("bf16", 512), ("f32x3", 512), ("f32", 384), ("bf16", 384), ("f32x3", 384)])
def test_concurrent_forwards_are_bit_reproducible(mode, dim):
    """Two forwards in flight on two streams (own workspaces) give, run after run, exactly the bits of a forward that
    had the chip to itself.  Round 2 found the LayerNorm-type kernels of the CR-MSA tail returning slightly different
    statistics (lanes 48..63 of a row, ~1e-4 relative) now and then when their waves shared a SIMD with the bf16-MFMA
    waves of the other bag's R-MSA kernel: lane-predicated code (column guards) around packed fp32 ops; the kernels
    now run guard-free when dim is a multiple of 256.  Round 3 (advisor): a width that keeps the guarded code (dim = 384:
    six heads of 64) runs the same check; there RRT_COMPUTE_F32X3 is answered with the exact fp32 kernels (the split
    kernels -- the co-runners that triggered the effect -- are used for dim % 256 == 0 only)."""
    import ctypes as C
    from hip_util import encoder_from_state, dev
    if dim == 512:
        g = load_golden("G3_d512_n9000")
        x, st, cfg = synth_case(g)
    else:
        cfg = dict(mlp_dim=dim, n_heads=dim // 64, crmsa_heads=dim // 64, epeg_k=15, crmsa_k=3, region_num=8)
        st = synth.encoder_state(**{k: v for k, v in cfg.items() if k != "region_num"})
        x = synth.bag(3000, dim, tag="conc/x")
    # Round 4: the two streams carry bags of DIFFERENT sizes (3000 and 2200 tokens, four and five forwards per round), so
    # that the kernels of one bag drift across those of the other -- two identical bags enqueued together run in lockstep and
    # every kernel only ever meets its own kind (tools/repro_guarded_ln.py is the long form of this test)
    lib = _lib.load()
    enc = encoder_from_state(st, cfg)
    enc._desc.compute = {"f32": _lib.COMPUTE_F32, "bf16": _lib.COMPUTE_BF16, "f32x3": _lib.COMPUTE_F32X3}[mode]
    w = enc._weights()
    ns, reps = [3000, 2200], [4, 5]
    xs = [dev(x[:m]).contiguous() for m in ns]
    streams = [torch.cuda.Stream() for _ in range(2)]
    ws = []
    for m in ns:
        need = C.c_size_t()
        _lib.check(lib.rrt_encoder_workspace_size(C.byref(enc._desc), m, C.byref(need)), "workspace size")
        ws.append(torch.zeros(need.value, dtype=torch.uint8, device="cuda:0"))
    ys = [[torch.zeros_like(xs[i]) for _ in range(reps[i])] for i in range(2)]

    def run(i, j):
        _lib.check(lib.rrt_encoder_forward_f32(C.byref(enc._desc), C.byref(w), xs[i].data_ptr(), ys[i][j].data_ptr(), ns[i],
                                               ws[i].data_ptr(), ws[i].numel(), streams[i].cuda_stream), "forward")
    torch.cuda.synchronize()
    refs = []
    for i in range(2):
        run(i, 0)
        torch.cuda.synchronize()
        refs.append(ys[i][0].clone())
    bad = total = 0
    for _ in range(12):
        for j in range(max(reps)):
            for i in range(2):
                if j < reps[i]:
                    run(i, j)
        torch.cuda.synchronize()
        for i in range(2):
            for j in range(reps[i]):
                total += 1
                bad += int(not torch.equal(ys[i][j], refs[i]))
    assert bad == 0, f"{bad} of {total} concurrent forwards differ from the solo run"


@pytest.mark.gpu
def test_concurrent_merged_launches_are_bit_reproducible():
    """The fp32 path of bags whose out-projection runs as a phase of the fused launch (regions of more than 64 tokens:
    rmsa_fused_kernel<.., PROJ>, blocks waiting for EARLIER blocks' attention output through workspace counters and reading
    it back through L2): four forwards in flight on four streams -- two bag sizes, so that the launches drift across
    each other and across the other bags' tails -- give, run after run, exactly the bits of a forward that had the chip to
    itself, and the plan says that these sizes take the merged launch."""
    import ctypes as C
    from hip_util import encoder_from_state, dev
    g = load_golden("G3_d512_n9000")
    x, st, cfg = synth_case(g)
    lib = _lib.load()
    enc = encoder_from_state(st, cfg)
    enc._desc.compute = _lib.COMPUTE_F32
    w = enc._weights()
    ns, reps = [9000, 6200, 9000, 7000], [3, 4, 3, 4]
    fl = C.c_int32(0)
    for m in set(ns):
        _lib.check(lib.rrt_encoder_plan(C.byref(enc._desc), m, C.byref(fl)), "plan")
        assert fl.value & _lib.PLAN_FUSED_PROJ, m
    xs = [dev(x[:m] * (1.0 + 0.01 * i)).contiguous() for i, m in enumerate(ns)]
    streams = [torch.cuda.Stream() for _ in ns]
    ws = []
    for m in ns:
        need = C.c_size_t()
        _lib.check(lib.rrt_encoder_workspace_size(C.byref(enc._desc), m, C.byref(need)), "workspace size")
        ws.append(torch.zeros(need.value, dtype=torch.uint8, device="cuda:0"))
    ys = [[torch.zeros_like(xs[i]) for _ in range(reps[i])] for i in range(len(ns))]

    def run(i, j):
        _lib.check(lib.rrt_encoder_forward_f32(C.byref(enc._desc), C.byref(w), xs[i].data_ptr(), ys[i][j].data_ptr(), ns[i],
                                               ws[i].data_ptr(), ws[i].numel(), streams[i].cuda_stream), "forward")
    torch.cuda.synchronize()
    refs = []
    for i in range(len(ns)):
        run(i, 0)
        torch.cuda.synchronize()
        refs.append(ys[i][0].clone())
        assert torch.isfinite(refs[i]).all()
    bad = total = 0
    for _ in range(10):
        for j in range(max(reps)):
            for i in range(len(ns)):
                if j < reps[i]:
                    run(i, j)
        torch.cuda.synchronize()
        for i in range(len(ns)):
            for j in range(reps[i]):
                total += 1
                bad += int(not torch.equal(ys[i][j], refs[i]))
                ys[i][j].fill_(float("nan"))
    assert bad == 0, f"{bad} of {total} concurrent forwards differ from the solo run"


# ------------------------------------------------------------------ RRT_COMPUTE_F32X3: fp32 emulated on the bf16 matrix cores
def _split_image(a):
    """numpy restatement of cast16.hip's split image: per 32 elements [32 bf16 hi | 32 bf16 lo] as uint16 bits"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    t = torch.from_numpy(a.reshape(-1, 32))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.cat([hi.view(torch.int16), lo.view(torch.int16)], dim=1).reshape(-1)


def _from_split(img, shape):
    g = img.cpu().view(torch.bfloat16).reshape(-1, 64)
    return (g[:, :32].double() + g[:, 32:].double()).reshape(shape).numpy()


def test_split_images():
    """cast_split / ln_partition_split: hi = bf16(x), lo = bf16(x - hi), 32-element groups -- bit for bit for the cast;
    hi + lo within 2^-16 of the float64 LayerNorm row for the fused producer."""
    from hip_util import dev, p, stream
    lib = _lib.load()
    w = synth.uniform("sp/w", (1536, 512), -1, 1) * np.exp(synth.uniform("sp/e", (1536, 512), -10, 3))
    wd = dev(w)
    out = torch.empty(w.size * 2, dtype=torch.int16, device="cuda:0")
    _lib.check(lib.rrt_cast_split(p(wd), p(out), w.size, stream()), "cast_split")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _split_image(w))
    assert np.abs(_from_split(out, w.shape) - w).max() <= 2.0 ** -16 * np.abs(w).max()
    L, rn, D = 9000, 8, 512
    x = synth.bag(L, D, tag="sp/x")
    gm, bt = 1.0 + synth.uniform("sp/g", (D,), -0.3, 0.3), synth.uniform("sp/b", (D,), -0.2, 0.2)
    g = _lib.region_grid(L, rn)
    xd, gd_, bd_ = dev(x), dev(gm), dev(bt)
    u = torch.full((g.H * g.H * D * 2,), 0x7FC0, dtype=torch.int16, device="cuda:0")
    _lib.check(lib.rrt_ln_partition_split(p(xd), p(gd_), p(bd_), p(u), L, D, g, stream()), "ln_partition_split")
    torch.cuda.synchronize()
    x64 = x.astype(np.float64)
    ln = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + 1e-5) * gm + bt
    ref = np.zeros((g.H * g.H, D))
    ref[:L] = ln
    ref = ref[O.partition_index(g.H, g.s)]
    got = _from_split(u, ref.shape)
    assert np.abs(got - ref).max() <= 3e-6 + 2.0 ** -15 * np.abs(ref).max() * 0 + 2.0 ** -16 * 8
    assert (got[np.abs(ref).sum(-1) == 0] == 0).all()


@pytest.mark.parametrize("M,N,K", [(9216, 512, 512), (9216, 1536, 512), (3136, 512, 512), (9216, 512, 1024)])
def test_linear_split(M, N, K):
    """C = A . B^T from split images: against hi.hi + hi.lo + lo.hi in float64 (tight: only the fp32 accumulation differs)
    and against the exact product (the emulation's own error: ~2^-16 of the products)."""
    from hip_util import dev, p, stream
    lib = _lib.load()
    A = synth.normal(f"ls/A{M}x{K}", (M, K))
    B = synth.uniform(f"ls/B{N}x{K}", (N, K), -1, 1) / np.sqrt(K)
    bias = synth.uniform("ls/b", (N,), -0.1, 0.1)
    Ai, Bi, bd_ = _split_image(A).to("cuda:0"), _split_image(B).to("cuda:0"), dev(bias)
    C_ = torch.full((M, N), float("nan"), device="cuda:0")
    _lib.check(lib.rrt_linear_split_f32(p(Ai), p(Bi), p(bd_), None, p(C_), M, N, K, None, stream()), "linear_split")
    torch.cuda.synchronize()
    got = C_.cpu().numpy()
    _cmp(got, O.split_matmul_t(A, B) + bias, 2e-5, f"linear_split {M}x{N}x{K} vs its restatement")
    exact = A.astype(np.float64) @ B.astype(np.float64).T + bias
    err = np.abs(got - exact)
    assert err.max() <= 3e-5 and err.mean() <= 3e-6, (err.max(), err.mean())


@pytest.mark.parametrize("R,P,D,heads,ek", [(64, 144, 512, 8, 15), (9, 121, 512, 8, 15), (5, 100, 512, 8, 21), (12, 81, 512, 8, 15),
                                            (20, 49, 512, 8, 9), (4, 64, 256, 4, 0), (3, 130, 1024, 16, 63), (256, 121, 512, 8, 15)])
def test_rmsa_fused_x3(R, P, D, heads, ek):
    """The F32X3 fused kernel against the float64 attention of the split-product projection (tight) and against the
    exact fp32 arithmetic (the emulation's error on the attention output)."""
    from hip_util import dev, p, stream
    lib = _lib.load()
    u = synth.normal(f"x3/u{R}x{P}", (R * P, D))
    w = synth.uniform("x3/w", (3 * D, D), -1, 1) / np.sqrt(D) * 1.5
    b = synth.uniform("x3/b", (3 * D,), -0.2, 0.2)
    pe = synth.uniform("x3/pe", (heads, max(ek, 1)), -0.3, 0.3)
    ui, wi, bd_, ped_ = _split_image(u).to("cuda:0"), _split_image(w).to("cuda:0"), dev(b), dev(pe)
    o = torch.full((R * P * D * 2,), 0x7FC0, dtype=torch.int16, device="cuda:0")
    _lib.check(lib.rrt_rmsa_fused_x3(p(ui), p(wi), p(bd_), p(ped_) if ek else None, p(o), R, P, D, heads, ek, stream()), "fused_x3")
    torch.cuda.synchronize()
    Rr = min(R, 8)
    got = _from_split(o, (R * P, D))[:Rr * P]
    assert np.isfinite(_from_split(o, (R * P, D))).all()
    st = {"qkv.weight": w, "qkv.bias": b, "proj.weight": np.eye(D), "proj.bias": np.zeros(D)}
    if ek:
        st["pe.weight"] = pe.reshape(heads, 1, ek, 1)
    taps = {}
    O._inner_attention64(u[:Rr * P].reshape(Rr, P, D), st, "", heads, ek, taps, O.SplitX3(), None)
    _cmp(got, taps["proj_in"].reshape(Rr * P, D), 4e-5, "fused_x3 vs its restatement")   # (O itself is stored as hi + lo)
    qkv_e = u[:Rr * P].astype(np.float64) @ w.astype(np.float64).T + b
    qkv_e[:, :D] *= (D // heads) ** -0.5
    err = np.abs(got - _attn_ref(qkv_e, pe, Rr, P, D, heads, ek))
    assert err.max() <= 1e-4 and err.mean() <= 5e-6, (err.max(), err.mean())


@pytest.mark.parametrize("name", ["G3_d512_n9000", "G2_d512_n512", "G5_d512_n4096", "G5_d512_n3000_k21_c5", "G4_d512_n30000_rn16",
                                  "G5_d512_n9000_c1_sc", "G10_d512_n8000_layers3", "G5_d512_n15000_k21_c5"])
def test_encoder_f32x3(name):
    """compute_dtype = "f32x3": the two big projections of the R-MSA layers emulated in fp32 on the bf16 matrix cores.
    Against the REAL reference's fp32 output: within 2e-5 (the north star asks for 1e-3; the exact path is at ~2e-6),
    and against the float64 restatement of its rounding points; bags the split kernels do not cover (regions beyond
    144 tokens or up to 48) silently take the exact path."""
    from hip_util import encoder_from_state, dev
    g = load_golden(name)
    x, st, cfg = synth_case(g)
    N = int(g["n"])
    enc = encoder_from_state(st, cfg)
    xd = dev(x)
    y_exact = enc(xd).cpu().numpy()
    enc.compute_dtype = "f32x3"
    y = enc(xd).cpu().numpy()
    enc.compute_dtype = None
    ref, got = (g["y"], y) if "y" in g else (g["y_rows"], y[g["rows"]])
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(y).all() and err.max() <= 2e-5 and err.mean() <= 2e-6, (err.max(), err.mean())
    H, s_, _ = O.grid(N, cfg.get("region_num", 8))
    covered = 48 < s_ * s_ <= 144
    assert (not np.array_equal(y, y_exact)) == covered
    if covered and N <= 9000:
        r3 = O.forward_f64(x, st, cfg, lowp=O.SplitX3())
        _cmp(y, r3, 1e-5, name + " f32x3 vs its restatement")
    assert np.array_equal(enc(xd).cpu().numpy(), y_exact)           # back on the exact path, bit for bit


# ------------------------------------------------------------------ row f2: training (forward + backward end to end)
TRAIN_CASES = {
    "crmsa_only_n700": (700, dict(mlp_dim=512, n_layers=1, crmsa_k=3)),
    "rmsa_only_n1000": (1000, dict(mlp_dim=512, cr_msa=False, epeg_k=15)),
    "default_n1500": (1500, dict(mlp_dim=512, epeg_k=15, crmsa_k=3)),
    "c16_n2600": (2600, dict(mlp_dim=512, epeg_k=15, crmsa_k=1, all_shortcut=True)),
    "nsclc_layers3_n900": (900, dict(mlp_dim=512, epeg_k=21, crmsa_k=5, n_layers=3)),
    "noepeg_nobias_n500": (500, dict(mlp_dim=512, epeg=False, qkv_bias=False)),
    "d256_n333": (333, dict(mlp_dim=256, n_heads=4, crmsa_heads=4, epeg_k=9)),
    # edge geometry: one-token regions, a single token, pads outnumbering tokens, region_num 4, the "give up region
    # attention" branch (one region = the whole bag), region_size override
    "edge_n50_p1": (50, dict(mlp_dim=512, epeg_k=15, crmsa_k=3)),
    "edge_n1": (1, dict(mlp_dim=512, epeg_k=15, crmsa_k=3)),
    "edge_n65": (65, dict(mlp_dim=512, epeg_k=15, crmsa_k=5)),
    "edge_rn4_n777": (777, dict(mlp_dim=512, epeg_k=9, crmsa_k=3, region_num=4)),
    "edge_minnum_n90": (90, dict(mlp_dim=512, epeg_k=15, crmsa_k=3, min_region_num=100)),
    "edge_rs5_n500": (500, dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_size=5)),
    "edge_k31_n130": (130, dict(mlp_dim=512, epeg_k=31, crmsa_k=1)),                 # taps far wider than the 4-token regions
    "edge_crk8_n400": (400, dict(mlp_dim=512, epeg_k=15, crmsa_k=8)),
    "edge_crmsa_only_sc_n300": (300, dict(mlp_dim=512, n_layers=1, crmsa_k=3, all_shortcut=True)),
    "edge_rn16_n2000": (2000, dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=16)),
    "edge_d1024_n300": (300, dict(mlp_dim=1024, n_heads=16, crmsa_heads=16, epeg_k=15, crmsa_k=3)),
    "pos_ppeg_first_n900": (900, dict(mlp_dim=512, epeg_k=15, crmsa_k=3, pos="ppeg", pos_pos=-1)),
    "pos_peg_mid_n700": (700, dict(mlp_dim=512, epeg_k=15, crmsa_k=3, pos="peg", pos_pos=0, n_layers=3)),
    "pos_peg1d_k5_nobias_n400": (400, dict(mlp_dim=512, crmsa_k=3, pos="peg", pos_pos=-1, peg_1d=True, peg_k=5,
                                           peg_bias=False)),
    "pos_ppeg_tiny_n30": (30, dict(mlp_dim=512, crmsa_k=3, pos="ppeg", pos_pos=-1)),
    "pos_ppeg_crmsa_only_n500": (500, dict(mlp_dim=512, n_layers=1, pos="ppeg", pos_pos=-1, peg_k=3)),
    "p169_n10000": (10000, dict(mlp_dim=512, epeg_k=15, crmsa_k=3)),          # regions of 169 tokens (MT = 11)
    "p256_n15000": (15000, dict(mlp_dim=512, epeg_k=15, crmsa_k=3)),          # regions of 256 tokens: streaming
    "brca_r50_heads1_n2000": (2000, dict(mlp_dim=512, epeg_k=17, crmsa_k=3, crmsa_heads=1)),   # README.md:98
    "ffn_gelu_n1200": (1200, dict(mlp_dim=512, epeg_k=15, crmsa_k=3, ffn=True, mlp_ratio=2.0)),
    "ffn_relu_sc_n700": (700, dict(mlp_dim=256, n_heads=4, crmsa_heads=4, ffn=True, ffn_act="relu", all_shortcut=True,
                                   n_layers=3, mlp_ratio=1.0)),
    "nsclc_plip_mlp_n1800": (1800, dict(mlp_dim=512, epeg_k=13, crmsa_k=3, crmsa_heads=1, all_shortcut=True,
                                        crmsa_mlp=True)),                                        # README.md:119
    "mlp_d192_n400": (400, dict(mlp_dim=192, n_heads=3, crmsa_heads=3, epeg_k=9, crmsa_k=3, crmsa_mlp=True)),   # hidden 48
    "attn2d_n1000_k5": (1000, dict(mlp_dim=512, epeg_k=5, crmsa_k=3, epeg_2d=True)),
    "valuebf_n700": (700, dict(mlp_dim=512, epeg_k=9, crmsa_k=3, epeg_type="value_bf")),
    "valueaf2d_n9000_k3": (9000, dict(mlp_dim=512, epeg_k=3, crmsa_k=3, epeg_type="value_af", epeg_2d=True)),
    # the other two value-EPEG type / shape combinations and the PEG / PPEG kernels' largest instantiations
    "valueaf1d_n700_k9": (700, dict(mlp_dim=512, epeg_k=9, crmsa_k=3, epeg_type="value_af")),
    "valuebf2d_n700_k3": (700, dict(mlp_dim=512, epeg_k=3, crmsa_k=3, epeg_type="value_bf", epeg_2d=True)),
    "pos_peg_k11_n500": (500, dict(mlp_dim=512, crmsa_k=3, pos="peg", pos_pos=-1, peg_k=11)),
    "pos_ppeg1d_k9_n500": (500, dict(mlp_dim=512, crmsa_k=3, pos="ppeg", pos_pos=-1, peg_k=9, peg_1d=True)),
}


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_encoder_backward_matches_autograd(case):
    """loss = <y, G>: every parameter gradient and dL/dx from rrt_encoder_backward_f32 (through the autograd
    Function of RRTEncoder in train() mode) against torch autograd of the reference's op sequence in float64."""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTEncoder
    N, cfg = TRAIN_CASES[case]
    D = cfg["mlp_dim"]
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k in _STATE_KEYS})
    x = synth.bag(N, D, tag="train/" + case)
    G = synth.normal("train/G/" + case, (N, D))
    # oracle
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    # HIP
    enc = RRTEncoder(drop_out=0., **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    assert y.grad_fn is not None
    _cmp(y.detach().cpu().numpy(), y64.detach().numpy(), 2e-4, case + " train forward")
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()

    # gradients that are mathematically zero (e.g. every score-path gradient when a region holds one token: the
    # softmax over a single key is constant) come out as fp32 rounding noise: the error floor is relative to the
    # largest gradient of the whole model, not to the (vanishing) tensor itself
    floor = 1e-3 * max([float(x_leaf.grad.abs().max())] + [float(v.grad.abs().max()) for v in params.values()
                                                           if v.grad is not None])

    def rel(got, ref, what):
        ref = ref.astype(np.float64)
        scale = max(np.abs(ref).max(), floor, 1e-6)
        err = np.abs(got.astype(np.float64) - ref).max() / scale
        assert np.isfinite(got).all(), what
        assert err <= 2e-3, f"{case} {what}: max error {err:.2e} of the largest gradient entry"
        return err

    rel(xd.grad.cpu().numpy(), x_leaf.grad.numpy(), "dx")
    for name, prm in enc.named_parameters():
        ref = params[name].grad
        assert prm.grad is not None, name
        if name.endswith("pe.bias") and cfg.get("epeg_type", "attn") == "attn":
            assert float(prm.grad.abs().max()) == 0.0 and float(ref.abs().max()) < 1e-6     # Identity 2
            continue
        rel(prm.grad.cpu().numpy(), ref.numpy().reshape(prm.shape), name)
    # eval() with gradients enabled records a graph too (the reference does: fine-tuning with dropout frozen,
    # attribution); under torch.no_grad() it is the inference path
    enc.eval()
    enc.zero_grad(set_to_none=True)
    ye = enc(xd.unsqueeze(0)).squeeze(0)
    assert ye.grad_fn is not None
    if case == "c16_n2600":
        (ye * dev(G)).sum().backward()
        rel(enc.cr_msa.attn.attn.qkv.weight.grad.cpu().numpy(), params["cr_msa.attn.attn.qkv.weight"].grad.numpy(), "eval-mode graph")
    with torch.no_grad():
        assert enc(xd.unsqueeze(0)).grad_fn is None
    if case == "default_n1500":
        # a second backward through a retained graph gives the same gradients again (accumulated: x2)
        enc.train()
        enc.zero_grad(set_to_none=True)
        y2 = enc(xd.unsqueeze(0)).squeeze(0)
        loss = (y2 * dev(G)).sum()
        loss.backward(retain_graph=True)
        g1 = enc.norm.weight.grad.clone()
        loss.backward()
        assert torch.allclose(enc.norm.weight.grad, 2 * g1, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", golden_names("G15"))
def test_encoder_gradients_match_reference(name):
    """Row f2 against the REAL reference's gradients (G15: the reference's own modules in .train() with drop_out = 0,
    cast to float64, loss = <y, G>; tools/make_golden_grad_amp.py): dL/dx and every parameter gradient of
    rrt_encoder_backward_f32, each within 1e-3 of THAT tensor's own largest entry (no model-wide scale); the only
    floors are for pe.bias (exactly zero, Identity 2).  Parameters the reference leaves without a gradient
    (a PEG / PPEG stage that is never applied) must come back None or exactly zero."""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTEncoder
    from test_oracle_golden import grad_fixture, grad_compare
    from conftest import STATE_KEYS
    g, fx, none = grad_fixture(name)
    cfg, N = g["cfg"], int(g["n"])
    D = cfg["mlp_dim"]
    tag = name[len("G15_grad_"):]
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k in STATE_KEYS})
    x = synth.bag(N, D, tag="train/" + tag)
    G = synth.normal("train/G/" + tag, (N, D))
    enc = RRTEncoder(drop_out=0., **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    y64 = y.detach().double().cpu().numpy()
    assert abs(y64.sum() - g["y_sums"][0]) <= 2e-4 * N * D and abs(np.abs(y64).max() - g["y_sums"][2]) <= 2e-4
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    grad_compare(xd.grad.cpu().numpy(), fx["dx"], 1e-3, "dx")
    for pname, prm in enc.named_parameters():
        if pname in none:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, pname
            continue
        assert prm.grad is not None, pname
        if pname.endswith("pe.bias") and cfg.get("epeg_type", "attn") == "attn":
            assert float(prm.grad.abs().max()) == 0.0            # Identity 2 (1-D and 2-D score-map EPEG alike)
            continue
        grad_compare(prm.grad.cpu().numpy(), fx["p_" + pname.replace(".", "_")], 1e-3, pname)


@pytest.mark.parametrize("case,p", [("default_n1500", 0.1), ("c16_n2600", 0.25), ("nsclc_layers3_n900", 0.1),
                                    ("ffn_gelu_n1200", 0.1), ("ffn_relu_sc_n700", 0.2)])
def test_encoder_backward_with_dropout(case, p):
    """Train-mode proj_drop (the reference's default drop_out=0.1): the kernels' stateless mask is rebuilt in
    numpy and handed to the float64 oracle, so forward and every gradient can be compared exactly; the masks
    themselves are checked for rate and for independence between layers."""
    from hip_util import DEV, dev, dropout_keep
    from rrt_mil_amd import RRTEncoder
    N, cfg = TRAIN_CASES[case]
    D = cfg["mlp_dim"]
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k in ("mlp_dim", "n_layers", "n_heads", "epeg", "epeg_k",
                                                                      "cr_msa", "crmsa_k", "qkv_bias", "ffn", "mlp_ratio")})
    x = synth.bag(N, D, tag="train/" + case)
    G = synth.normal("train/G/" + case, (N, D))
    seed = 0x1234_5678_9ABC_DEF
    H, s_, _ = O.grid(N, cfg.get("region_num", 8))
    n_layers = cfg.get("n_layers", 2) - 1
    masks = {li: dropout_keep(seed, li, H * H, D, p) for li in range(n_layers)}
    masks["cr_msa"] = dropout_keep(seed, 100, cfg.get("crmsa_k", 3) * 64, D, p)
    if cfg.get("ffn"):                            # the Mlp's two dropouts per TransLayer (api.hip: layers 200 + 2 i, + 1)
        hid = int(D * cfg.get("mlp_ratio", 4.0))
        for key, idx in [(li, li) for li in range(n_layers)] + [("cr_msa", 8)]:
            masks[("ffn1", key)] = dropout_keep(seed, 200 + 2 * idx, N, hid, p)
            masks[("ffn2", key)] = dropout_keep(seed, 201 + 2 * idx, N, D, p)
    for m in masks.values():
        assert abs(1.0 - m.mean() - p) < 0.01
    if n_layers > 1:
        assert abs((masks[0] == masks[1]).mean() - (p * p + (1 - p) ** 2)) < 0.02   # independent masks
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True, drop=(p, masks))
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = RRTEncoder(drop_out=p, **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    enc.drop_seed = seed
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    _cmp(y.detach().cpu().numpy(), y64.detach().numpy(), 2e-4, case + " train forward with dropout")
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    for name, got, ref in [("dx", xd.grad, x_leaf.grad)] + [(n_, p_.grad, params[n_].grad.reshape(p_.shape))
                                                            for n_, p_ in enc.named_parameters()
                                                            if not n_.endswith("pe.bias")]:
        ref = ref.numpy().astype(np.float64)
        err = np.abs(got.cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-6)
        assert err <= 2e-3, f"{case} {name}: {err:.2e}"
    # a fresh seed per call by default: two training forwards differ, eval does not
    enc.drop_seed = None
    y1, y2 = enc(xd.unsqueeze(0)), enc(xd.unsqueeze(0))
    assert not torch.equal(y1, y2)
    enc.eval()
    assert torch.equal(enc(xd.unsqueeze(0)), enc(xd.unsqueeze(0)))


@pytest.mark.parametrize("case,draws", [("default_n1500", [1 / 0.7, 0.0]), ("default_n1500", [0.0, 1 / 0.7]),
                                        ("ffn_gelu_n1200", [1 / 0.7, 0.0, 0.0, 1 / 0.7]),
                                        ("nsclc_layers3_n900", [0.0, 1 / 0.7, 1 / 0.7])])
def test_encoder_backward_with_drop_path(case, draws):
    """drop_path > 0 (TransLayer.drop_path, rrt.py:102,125,129: timm's DropPath keeps or drops a whole residual branch
    at batch size 1, kept branches scaled by 1 / keep_prob): with the draws pinned, forward and every gradient against
    the float64 oracle given the same multipliers (together with proj dropout); unpinned, the draws follow
    Bernoulli(keep_prob) and eval() ignores them."""
    from hip_util import DEV, dev, dropout_keep
    from rrt_mil_amd import RRTEncoder
    N, cfg = TRAIN_CASES[case]
    D, p = cfg["mlp_dim"], 0.1
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k in ("mlp_dim", "n_layers", "n_heads", "epeg", "epeg_k",
                                                                      "cr_msa", "crmsa_k", "qkv_bias", "ffn", "mlp_ratio")})
    x = synth.bag(N, D, tag="train/" + case)
    G = synth.normal("train/G/" + case, (N, D))
    seed = 0x0F1E_2D3C_4B5A
    H, _, _ = O.grid(N, cfg.get("region_num", 8))
    n_layers = cfg.get("n_layers", 2) - 1
    masks = {li: dropout_keep(seed, li, H * H, D, p) for li in range(n_layers)}
    masks["cr_msa"] = dropout_keep(seed, 100, cfg.get("crmsa_k", 3) * 64, D, p)
    keys = list(range(n_layers)) + ["cr_msa"]
    if cfg.get("ffn"):
        hid = int(D * cfg.get("mlp_ratio", 4.0))
        for key, idx in [(li, li) for li in range(n_layers)] + [("cr_msa", 8)]:
            masks[("ffn1", key)] = dropout_keep(seed, 200 + 2 * idx, N, hid, p)
            masks[("ffn2", key)] = dropout_keep(seed, 201 + 2 * idx, N, D, p)
    order = [(k, "attn") for k in keys] + ([(k, "ffn") for k in keys] if cfg.get("ffn") else [])
    assert len(order) == len(draws)
    branch = dict(zip(order, draws))
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True, drop=(p, masks), branch=branch)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = RRTEncoder(drop_out=p, drop_path=0.3, **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    enc.drop_seed, enc.drop_path_draws = seed, draws
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    _cmp(y.detach().cpu().numpy(), y64.detach().numpy(), 2e-4, case + " forward with drop_path")
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    top = max(float(v.grad.abs().max()) for v in params.values() if v.grad is not None)
    for name, got, ref in [("dx", xd.grad, x_leaf.grad)] + [(n_, p_.grad, params[n_].grad.reshape(p_.shape))
                                                            for n_, p_ in enc.named_parameters()
                                                            if not n_.endswith("pe.bias")]:
        ref = ref.numpy().astype(np.float64)
        # a dropped branch leaves its parameters with an exactly zero gradient
        err = np.abs(got.cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-6 * top)
        assert err <= 2e-3, f"{case} {name}: {err:.2e}"
    dropped = [k for k, m in branch.items() if m == 0.0 and k[1] == "attn" and k[0] != "cr_msa"]
    for li, _ in dropped:
        assert float(enc.layers[li].attn.attn.qkv.weight.grad.abs().max()) == 0.0
    # unpinned: draws are Bernoulli(keep) / keep from torch's CPU generator; eval() has none
    enc.drop_path_draws = None
    torch.manual_seed(7)
    seen = [tuple(enc._branch_scales()) for _ in range(200)]
    vals = np.array([s_[0] for s_ in seen])
    assert set(np.round(vals, 4)) == {0.0, round(1 / 0.7, 4)} and abs((vals > 0).mean() - 0.7) < 0.12
    enc.eval()
    assert enc._branch_scales() is None
    with torch.no_grad():
        assert torch.equal(enc(xd.unsqueeze(0)), enc(xd.unsqueeze(0)))


def test_train_mode_without_graph_and_stale_weights():
    """train() under torch.no_grad() (MC dropout, EMA / teacher forwards) applies proj dropout like the reference
    (rmsa.py:132) -- with the seed pinned it equals the oracle given the same masks -- and a parameter changed in
    place between a forward and its backward is refused (the backward kernels read the live weights)."""
    from hip_util import DEV, dev, dropout_keep
    from rrt_mil_amd import RRTEncoder
    N, cfg = TRAIN_CASES["default_n1500"]
    st = synth.encoder_state(mlp_dim=512, epeg_k=15, crmsa_k=3)
    x = synth.bag(N, 512, tag="train/default_n1500")
    p, seed = 0.1, 0x5EED
    H, _, _ = O.grid(N, 8)
    masks = {0: dropout_keep(seed, 0, H * H, 512, p), "cr_msa": dropout_keep(seed, 100, 3 * 64, 512, p)}
    ref = O.forward_eager(torch.from_numpy(x).double(), {k: torch.from_numpy(v).double() for k, v in st.items()}, cfg,
                          drop=(p, masks)).numpy()
    enc = RRTEncoder(drop_out=p, **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    xd = dev(x)
    with torch.no_grad():
        enc.drop_seed = seed
        y = enc(xd.unsqueeze(0)).squeeze(0)
        assert y.grad_fn is None
        _cmp(y.cpu().numpy(), ref, 2e-4, "train() forward under no_grad")
        enc.drop_seed = None
        assert not torch.equal(enc(xd.unsqueeze(0)), enc(xd.unsqueeze(0)))
        outs = enc.forward_bags([xd, xd[:700]])
        assert outs[0].shape == xd.shape and not torch.equal(outs[0], y)
    y = enc(xd.unsqueeze(0))
    with torch.no_grad():
        enc.norm.weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified in place"):
        y.sum().backward()


def test_rrtmil_learns_synthetic_task():
    """The reference's training loop in miniature (main.py:439-470): RRTMIL.train(), default dropouts, Adam, one bag
    per step, cross-entropy on the bag label.  Two classes of synthetic bags that differ in a handful of 'tumour'
    patches; the loss must fall and held-out bags must be classified (eval() under no_grad = the inference path)."""
    from rrt_mil_amd import RRTMIL
    torch.manual_seed(2021)
    dev_ = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    direction = rng.randn(256).astype(np.float32)

    def make_bag(label, n):
        x = np.maximum(rng.randn(n, 256), 0).astype(np.float32)
        if label:
            idx = rng.choice(n, size=max(4, n // 50), replace=False)
            x[idx] += 1.5 * np.maximum(direction, 0)
        return torch.from_numpy(x).unsqueeze(0)

    train = [(make_bag(i % 2, int(rng.randint(600, 1500))), i % 2) for i in range(24)]
    test = [(make_bag(i % 2, int(rng.randint(600, 1500))), i % 2) for i in range(10)]
    mil = RRTMIL(input_dim=256, n_classes=2, epeg_k=15, crmsa_k=3).to(dev_)
    opt = torch.optim.Adam(mil.parameters(), lr=2e-4)
    first, last = [], []
    for epoch in range(9):
        mil.train()
        for x, y in train:
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(mil(x.to(dev_)), torch.tensor([y], device=dev_))
            loss.backward()
            opt.step()
            (first if epoch == 0 else last if epoch == 8 else []).append(float(loss.detach()))
    assert np.mean(last) < 0.5 * np.mean(first), (np.mean(first), np.mean(last))
    mil.eval()
    with torch.no_grad():
        correct = sum(int(mil(x.to(dev_)).argmax(-1).item() == y) for x, y in test)
    assert correct >= 8, f"{correct}/10 held-out bags"


def test_training_limits_raise():
    """Outside the built training envelope the call raises (no silent fallback): R-MSA head dim != 64, dim > 1024,
    (PEG / PPEG train, see the pos_* cases above)."""
    from rrt_mil_amd import RRTEncoder
    x = torch.randn(1, 200, 64, device="cuda:0", requires_grad=True)
    with pytest.raises(NotImplementedError):
        RRTEncoder(mlp_dim=64, drop_out=0.).to("cuda:0").train()(x)                 # head dim 8
    x = torch.randn(1, 200, 512, device="cuda:0", requires_grad=True)
    with pytest.raises(NotImplementedError):
        RRTEncoder(mlp_dim=2048, n_heads=32, crmsa_heads=32).to("cuda:0").train()(torch.randn(1, 64, 2048, device="cuda:0"))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_training_under_autocast(dt):
    """The reference's --amp training (main.py:101-102,439): under torch.autocast the GEMMs of the training forward and
    the activation-gradient GEMMs round their operands; gradients stay close to the fp32 oracle's (and differ from
    the fp32 run, i.e. the mode really is on)."""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTEncoder
    N, cfg = TRAIN_CASES["default_n1500"]
    st = synth.encoder_state(mlp_dim=512, epeg_k=15, crmsa_k=3)
    x = synth.bag(N, 512, tag="train/default_n1500")
    G = synth.normal("train/G/default_n1500", (N, 512))
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = RRTEncoder(drop_out=0., **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    xd = dev(x).requires_grad_(True)
    with torch.autocast("cuda", dtype=dt):
        y = enc(xd.unsqueeze(0)).squeeze(0)
    (y.float() * dev(G)).sum().backward()
    torch.cuda.synchronize()
    tol = 3e-2 if dt == torch.bfloat16 else 5e-3
    worst = 0.0
    for name, got, ref in [("dx", xd.grad, x_leaf.grad)] + [(n_, p_.grad, params[n_].grad.reshape(p_.shape))
                                                            for n_, p_ in enc.named_parameters()
                                                            if not n_.endswith("pe.bias")]:
        ref = ref.numpy().astype(np.float64)
        err = np.abs(got.float().cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-6)
        worst = max(worst, err)
        assert err <= tol, f"{name}: {err:.2e}"
    assert worst > 1e-5          # reduced-precision operands leave a visible (small) difference

