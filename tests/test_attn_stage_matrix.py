"""GPU (-m gpu): every region-attention kernel variant, forward and backward, through the two public stage dispatchers
(rrt_region_attention_f32, rrt_region_attention_backward_f32).

A. the full instantiation grid: all 15 head dims of region_attn_hd_kernel<HD> / attn_bwd_*_hd_kernel<HD>, the region size
   drawn from each kernel's own edges (chunk, run, query group), the project's inputs and the project's bounds.
B. peaked softmax rows (largest |score| 40 .. 60) on every dispatch branch, head dim 64 included: unstructured, the row
   maximum in each key run in turn, ties, a dominant last key next to masked ones.  Bound: max(project bound, 8 x the error
   of a plain fp32 eager evaluation of the same formula on the CPU against float64).
C. the eight head dims no other test launches, inside the encoder: eval() and one training step against the float64 oracle.

Every stage call writes into NaN-filled outputs with canary rows behind them and a workspace of exactly the size the
library asks for with canary bytes behind it.  The case lists are plain module data (tests/test_attn_stage_grid_cpu.py
checks on the CPU that they cover what is claimed); importing this module needs no device."""
import os

import numpy as np
import pytest
import torch

from conftest import STATE_KEYS
from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth
from test_train_head_dims import _stage_inputs

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 5e-5, 1e-4     # the project's stage bounds (test_attn_fwd_head_dims.py / test_train_head_dims.py)
E32_FACTOR = 8.0                  # family B: a kernel may be 8 x the fp32 eager evaluation's own error off float64
RECORDS = []                      # (section, forward family, backward family, quantity, e32 or None, kernel error)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_STAGE_ERRORS_OUT")       # the table kept as profiles/attn_stage_errors.txt
    if out and RECORDS:
        with open(out, "w") as fh:
            fh.write(error_table(RECORDS))


def error_table(records):
    """per (section, kernel family, quantity): cases, worst e32, worst kernel error, worst kernel error / bound-free ratio
    to the same case's e32"""
    rows = {}
    for sec, ffam, bfam, what, e32, err in records:
        fam = ffam if what == "o" else bfam
        n, w32, werr, wr = rows.get((sec, fam, what), (0, 0.0, 0.0, 0.0))
        ratio = err / e32 if e32 else 0.0
        rows[(sec, fam, what)] = (n + 1, max(w32, e32 or 0.0), max(werr, err), max(wr, ratio))
    lines = [f"{'section':8s} {'kernel family':24s} {'quantity':8s} {'cases':>5s} {'worst e32':>10s} {'worst err':>10s} "
             f"{'worst err/e32':>13s}"]
    for (sec, fam, what), (n, w32, werr, wr) in sorted(rows.items()):
        e = f"{w32:10.2e}" if w32 else f"{'-':>10s}"
        r = f"{wr:13.2f}" if wr else f"{'-':>13s}"
        lines.append(f"{sec:8s} {fam:24s} {what:8s} {n:5d} {e} {werr:10.2e} {r}")
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------ the kernels' own constants and dispatch, restated
# Source: FwdCfg<HD> in csrc/region_attn_hd.hip and StreamCfg<HD> in csrc/attn_bwd.hip (CT = key tiles per chunk, CK = 16 CT
# keys per chunk, NWMAX / NW = 16-query tiles per block), launch_region_attention in csrc/region_attn.hip and
# launch_attention_backward in csrc/attn_bwd.hip (the branches).  tests/test_attn_stage_grid_cpu.py reads the head dims back
# out of the two dispatch switches.
HDS = [16, 32, 48, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256]
EKS = [9, 21, 31, 63]
P_MAX = 484


def fwd_cfg(hd):
    ct = min(9, max(2, 512 // hd))
    return dict(CT=ct, CK=16 * ct, G=16 * (8 if hd <= 128 else 4))


def bwd_cfg(hd):
    ct = min(8, max(2, 512 // hd))
    return dict(CT=ct, CK=16 * ct, G=16 * (4 if hd >= 192 else 6))


def fwd_runs(hd, P):
    """[(first key, key tiles)] of the forward's online-softmax runs over a region of P keys: per chunk, runs of three tiles,
    then what is left as a run of two or one (head dim 64: the general kernel's 48-key stages)"""
    ck = 48 if hd == 64 else fwd_cfg(hd)["CK"]
    runs = []
    for r0 in range(0, P, ck):
        nt = min(ck // 16, (P - r0 + 15) // 16)
        runs += [(r0 + 16 * t0, min(3, nt - t0)) for t0 in range(0, nt, 3)]
    return runs


def fwd_family(hd, P, ek):
    if hd != 64:
        return "region_attn_hd"
    if P == 64 and ek == 0:
        return "attn64"
    if 208 < P <= 256:
        return "resident16" if P > 240 else "resident15"
    nt = (P + 15) // 16
    nw = nt if nt < 4 else 3 if nt % 4 and nt % 3 == 0 else 4
    kc = 16 if P <= 16 else 32 if P <= 32 else 48
    while nw > 1 and min(P, 16 * nw + ek - 1) > 2 * kc:
        nw -= 1
    return "tile16" if P <= 16 else "tile32" if P <= 32 else f"tile48_nw{nw}" + ("_gt256" if P > 256 else "")


def bwd_family(hd, P, ek):
    if hd != 64:
        return "valu_generic" if ek == 0 and P <= 128 else "stream_hd"
    if P > 208:
        return "stream64_lds_adjoint" if P <= 256 else "stream64_global_adjoint"
    return "resident%d" % next(t for t in (64, 96, 112, 128, 144, 176, 208) if P <= t)


def stage_P_grid(hd):
    """the region sizes of section A for one head dim, from the constants above: the 16-key tile edge, every chunk edge
    (forward and backward CK), a last chunk of 1 .. CT tiles, the query-group edges, and the largest region"""
    f, b = fwd_cfg(hd), bwd_cfg(hd)
    ps = {1, 15, 16, 17, P_MAX}
    for c in (f, b):
        ck = c["CK"]
        ps |= {ck - 1, ck, ck + 1, ck + 17, ck + 33, 2 * ck + 1}
        ps |= {ck + 16 * t + 1 for t in range(c["CT"])}          # a last chunk of t + 1 tiles behind a full one
        ps |= {c["G"] - 1, c["G"], c["G"] + 1}
    return sorted(p for p in ps if 1 <= p <= P_MAX)


def _heads(hd):
    return 3 if hd <= 96 else 2


def stage_cases():
    """(hd, P, epeg_k): every (head dim, P) with epeg_k 0, 15 and one of 9 / 21 / 31 / 63 in turn; 63, wider than the region
    and across both its ends, at P = 15 and 17"""
    out = []
    for a, hd in enumerate(HDS):
        for b, P in enumerate(stage_P_grid(hd)):
            third = 63 if P in (15, 17) else EKS[(a + b) % len(EKS)]
            out += [(hd, P, ek) for ek in (0, 15, third)]
    return out


STAGE_CASES = stage_cases()

HD64_PS = [9, 25, 48, 64, 81, 100, 121, 144, 169, 196, 225, 256, 484]
HD64_MASKED_PS = [17, 49, 65, 97, 209, 241, 257]


def peaked_cases():
    """(variant, hd, P, epeg_k).  Per head dim of A: one chunk, CK + 1 and 484; head dim 64: a P in every branch of the two
    dispatchers."""
    out = []
    for a, hd in enumerate(HDS):
        ck = fwd_cfg(hd)["CK"]
        for b, P in enumerate((ck, ck + 1, P_MAX)):
            out.append(("plain", hd, P, (0, 15, EKS[(a + b) % len(EKS)])[(a + b) % 3]))
            out += [("runmax", hd, P, 0), ("runmax", hd, P, 15), ("ties_k", hd, P, 0)]
        out += [("ties_k", hd, ck + 1, 15), ("ties_q", hd, ck + 1, 15), ("ties_q", hd, P_MAX, 0)]
        out += [("masked", hd, P, ek) for P in (17, ck + 1) for ek in (0, 15)]
    for b, P in enumerate(HD64_PS):
        out += [("plain", 64, P, 0), ("plain", 64, P, 15), ("runmax", 64, P, (15, 0)[b % 2]), ("ties_k", 64, P, (0, 15)[b % 2])]
    out += [("runmax", 64, 64, 15), ("ties_q", 64, 144, 15), ("ties_q", 64, 64, 0)]
    out += [("masked", 64, P, ek) for P in HD64_MASKED_PS for ek in (0, 15)]
    return out


PEAKED_CASES = peaked_cases()


def case_id(hd, P, ek, variant=None):
    """names the kernel family each direction takes, so that a reader of the report sees both backward families hit"""
    head = f"{variant}-" if variant else ""
    return f"{head}hd{hd}-P{P}-k{ek}-fwd:{fwd_family(hd, P, ek)}-bwd:{bwd_family(hd, P, ek)}"


# ------------------------------------------------------------------ the reference: the explicit formulation, any dtype
def explicit(qkv, pe, pb, dO, R, P, D, heads, ek, dtype, prescaled):
    """scores [P, P], a depth-wise conv along the query axis WITH a bias, softmax, A V, and autograd of <O, dO> -- plain
    torch ops on the CPU in `dtype`.  prescaled: qkv holds q already times hd^-0.5 (the stash layout the stage reads), and
    the q gradient is brought back to the raw layout the stage writes.  -> O, d_qkv, d taps (or None), d bias, max |score|"""
    hd = D // heads
    tq = torch.tensor(qkv[:R * P], dtype=dtype, requires_grad=True)
    tw = torch.tensor(pe, dtype=dtype, requires_grad=True)
    tb = torch.tensor(pb, dtype=dtype, requires_grad=True)
    t = tq.reshape(R, P, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = (t[0] if prescaled else t[0] * hd ** -0.5), t[1], t[2]
    S = q @ k.transpose(-2, -1)
    if ek and dtype == torch.float64:
        S = S + torch.nn.functional.conv2d(S, tw.reshape(heads, 1, ek, 1), tb, padding=(ek // 2, 0), groups=heads)
    elif ek:
        # fp32: the same stencil as shifted slices.  torch's fp32 CPU conv2d returns a weight gradient that is off by far more
        # than rounding for a 63 x 1 filter on 484 x 484 maps (single taps wrong by 10 % and more, on random data too), which
        # would make e32, and with it the bound, meaningless for the taps.
        Sp = torch.nn.functional.pad(S, (0, 0, ek // 2, ek // 2))
        conv = tb.view(1, heads, 1, 1).expand_as(S)
        for tap in range(ek):
            conv = conv + tw[:, tap].view(1, heads, 1, 1) * Sp[:, :, tap:tap + P]
        S = S + conv
    Oref = (S.softmax(-1) @ v).transpose(1, 2).reshape(R * P, D)
    (Oref * torch.tensor(dO[:R * P], dtype=dtype)).sum().backward()
    g = tq.grad.double().numpy().copy()
    if prescaled:
        g[:, :D] *= hd ** -0.5
    return (Oref.detach().double().numpy(), g, tw.grad.double().numpy() if ek else None,
            tb.grad.double().numpy() if ek else None, float(S.detach().abs().max()))


def _maxerr(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())


def _run_and_check(section, variant, stash, pe, ref, ref32, dO, R, P, D, heads, ek):
    """both stage calls on `stash` (which may hold rows behind region R - 1), the memory checks, and every quantity against
    `ref` (float64): bound = the project's, or E32_FACTOR x the error of `ref32` where one is given.  Returns o (numpy)."""
    from hip_util import dev, region_attention_backward_guarded, region_attention_guarded
    hd = D // heads
    d_stash, d_pe = dev(stash), (dev(pe) if ek else None)
    o, ok = region_attention_guarded(d_stash, d_pe, R, P, D, heads, ek)
    assert ok, "forward: rows past n_regions * P of o were written"
    dqkv, dpe, intact = region_attention_backward_guarded(d_stash, d_pe, o, dev(dO[:R * P]), R, P, D, heads, ek)
    assert all(intact.values()), f"backward wrote past the end of: {[k for k, v in intact.items() if not v]}"
    o = o.cpu().numpy()
    scale = max(1.0, np.sqrt(R * P))
    got = {"o": o, "dq": dqkv[:, :D], "dk": dqkv[:, D:2 * D], "dv": dqkv[:, 2 * D:]}
    want = {"o": ref[0], "dq": ref[1][:, :D], "dk": ref[1][:, D:2 * D], "dv": ref[1][:, 2 * D:]}
    want32 = None if ref32 is None else {"o": ref32[0], "dq": ref32[1][:, :D], "dk": ref32[1][:, D:2 * D],
                                         "dv": ref32[1][:, 2 * D:]}
    if ek:
        got["taps"], want["taps"] = dpe / scale, ref[2] / scale
        if want32 is not None:
            want32["taps"] = ref32[2] / scale
    fam = (fwd_family(hd, P, ek), bwd_family(hd, P, ek))
    failures = []
    for what in got:
        assert np.isfinite(got[what]).all(), f"{what}: an element was left unwritten or is not finite"
        base = FWD_TOL if what == "o" else BWD_TOL
        e32 = None if want32 is None else _maxerr(want32[what], want[what])
        tol = base if e32 is None else max(base, E32_FACTOR * e32)
        err = _maxerr(got[what], want[what])
        RECORDS.append((section, fam[0], fam[1], what, e32, err))
        print(f"{variant or 'grid'} hd{hd} P{P} k{ek} {what}: max-abs {err:.3e}  e32 {e32 if e32 is None else f'{e32:.3e}'}  "
              f"bound {tol:.2e}  max|ref| {np.abs(want[what]).max():.3g}")
        if err > tol:
            failures.append(f"{what}: max-abs {err:.3e} > {tol:.2e}")
    assert not failures, "; ".join(failures)
    return o


# ------------------------------------------------------------------ A. the full instantiation grid
@pytest.mark.parametrize("hd,P,ek", STAGE_CASES, ids=[case_id(*c) for c in STAGE_CASES])
def test_stage_grid(hd, P, ek):
    """forward O against the float64 explicit formulation (with the conv bias, which must drop out): max-abs <= 5e-5; dq, dk,
    dv and the taps against float64 autograd: <= 1e-4; the bias gradient of the reference is zero; canaries and NaN fill"""
    R, heads = 2, _heads(hd)
    D = hd * heads
    raw, pe, pb, dO, stash = _stage_inputs(R, P, D, heads, ek)
    ref = explicit(raw, pe, pb, dO, R, P, D, heads, ek, torch.float64, prescaled=False)
    if ek:
        assert np.abs(ref[3]).max() < 1e-9 * R * P          # Identity 2: the bias gradient is zero
    _run_and_check("A", None, stash, pe, ref, None, dO, R, P, D, heads, ek)


# ------------------------------------------------------------------ B. peaked softmax on every dispatch branch
PEAK_TARGET, PEAK_WINDOW = 50.0, (40.0, 60.0)
BOOST = 6.0


def peaked_inputs(variant, hd, P, ek):
    """the streams of _stage_inputs, q and k (never v) scaled so that the largest |score| of the float64 reference is about
    50, with the variant's structure put in first.  -> (stash [rows, 3 D], taps, bias, dO, R); rows > R P for `masked`."""
    heads = _heads(hd) if hd != 64 else 2
    D = hd * heads
    runs = fwd_runs(hd, P)
    R = len(runs) if variant == "runmax" else 2
    behind = 1 if variant == "masked" else 0            # one more region's worth of rows behind the last region
    _, pe, pb, dO, stash = _stage_inputs(R + behind, P, D, heads, ek)
    t = stash.reshape(R + behind, P, 3, heads, hd)      # a view: [region, row, q|k|v, head, column]
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    if variant == "runmax":
        # region r: one key of run r carries the row maximum for the queries i = 0 (mod 3), is the smallest for i = 1 (mod 3)
        # and scores exactly 0 for the rest -- the running maximum arrives in run r, for every r in turn
        for r, (first, tiles) in enumerate(runs):
            j = first + (7 * r + 3) % min(16 * tiles, P - first)
            for h in range(heads):
                u = k[r, j, h] / np.linalg.norm(k[r, j, h])
                proj = q[r, :, h] @ u
                want = np.abs(proj) * np.array([1.0, -1.0, 0.0], dtype=np.float32)[np.arange(P) % 3]
                q[r, :, h] += np.outer(want - proj, u)
            k[r, j] *= BOOST
    elif variant == "ties_k":
        k[:] = k[:, :1]                                  # all keys of a region equal: uniform probabilities, O = mean of V
    elif variant == "ties_q":
        q[:] = 0.0                                       # distinct keys, all scores equal (0, or the conv bias)
    elif variant == "masked":
        # the single valid key of the last tile: the row maximum where q . k > 0, the smallest elsewhere; the rows directly
        # behind the last region (which the buffer holds, so nothing is read out of bounds) are very large
        k[:R, P - 1] *= BOOST
        t[R] *= 1.0e3
    hs = stash[:R * P].astype(np.float64).reshape(R, P, 3, heads, hd).transpose(2, 0, 3, 1, 4)
    S = torch.from_numpy(hs[0] @ hs[1].transpose(0, 1, 3, 2))
    if ek:
        S = S + torch.nn.functional.conv2d(S, torch.tensor(pe, dtype=torch.float64).reshape(heads, 1, ek, 1), None,
                                           padding=(ek // 2, 0), groups=heads)
    smax = float(S.abs().max())
    if smax > 0:
        stash[:R * P, :2 * D] *= np.float32(np.sqrt(PEAK_TARGET / smax))
    return stash, pe, pb, dO, R, heads


@pytest.mark.parametrize("variant,hd,P,ek", PEAKED_CASES, ids=[case_id(h, p_, k, v) for v, h, p_, k in PEAKED_CASES])
def test_stage_peaked(variant, hd, P, ek):
    """peaked softmax rows through both dispatchers.  Bound per quantity: max(project bound, 8 x e32), e32 = the error of the
    same formula in fp32 eager on the CPU against float64 (measured in this test, not read off the kernels)."""
    stash, pe, pb, dO, R, heads = peaked_inputs(variant, hd, P, ek)
    D = hd * heads
    ref = explicit(stash, pe, pb, dO, R, P, D, heads, ek, torch.float64, prescaled=True)
    ref32 = explicit(stash, pe, pb, dO, R, P, D, heads, ek, torch.float32, prescaled=True)
    if variant in ("plain", "runmax", "masked"):
        assert PEAK_WINDOW[0] <= ref[4] <= PEAK_WINDOW[1], f"largest |score| {ref[4]:.1f} outside {PEAK_WINDOW}"
    o = _run_and_check("B", variant, stash, pe, ref, ref32, dO, R, P, D, heads, ek)
    if variant == "ties_k" and ek == 0 and fwd_family(hd, P, ek) == "region_attn_hd":
        # every score of a query is one bit pattern: every exp2 argument is exactly 0, every alpha exactly 1, and each query
        # sums the same V rows in the same order -> all rows of O of one (region, head) are the same bits
        rows = o.reshape(R, P, D)
        assert np.array_equal(rows, np.broadcast_to(rows[:, :1], rows.shape)), "rows of O differ within a region"


# ------------------------------------------------------------------ C. the eight head dims inside the encoder
ENC_CFGS = {
    "d640_h8": dict(mlp_dim=640, n_heads=8, epeg_k=15, crmsa_k=3),         # head dim 80
    "d448_h4": dict(mlp_dim=448, n_heads=4, epeg_k=15, crmsa_k=3),         # 112
    "d320_h2": dict(mlp_dim=320, n_heads=2, epeg_k=15, crmsa_k=3),         # 160
    "d480_h2": dict(mlp_dim=480, n_heads=2, epeg_k=15, crmsa_k=3),         # 240
}
ENC_CASES = [(c, 3000) for c in ENC_CFGS] + [("d640_h8", 9000), ("d320_h2", 15000)]
ENC_TRAIN_CASES = [(c, 3000) for c in ENC_CFGS] + [("d448_h4", 9000)]


def _state(cfg):
    return synth.encoder_state(**{k: v for k, v in cfg.items() if k in STATE_KEYS})


@pytest.mark.parametrize("name,N", ENC_CASES)
def test_encoder_eval_untested_head_dims(name, N):
    """eval() under no_grad against the float64 oracle: max-abs <= 2e-4"""
    from hip_util import dev, encoder_from_state
    cfg = ENC_CFGS[name]
    st = _state(cfg)
    x = synth.bag(N, cfg["mlp_dim"], tag=f"asm/{name}/{N}")
    enc = encoder_from_state(st, cfg)
    with torch.no_grad():
        y = enc(dev(x).unsqueeze(0)).squeeze(0)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    err = _maxerr(y, O.forward_f64(x, st, cfg))
    print(f"{name} N={N}: max-abs {err:.3e} (bound 2.0e-04)")
    assert np.isfinite(y).all() and err <= 2e-4, f"{name} N={N}: max-abs {err:.3e}"


@pytest.mark.parametrize("name,N", ENC_TRAIN_CASES)
def test_encoder_training_step_untested_head_dims(name, N):
    """one training step, loss = <y, G>: y within 2e-4 of the float64 oracle, dL/dx and every parameter gradient within 2e-3
    of the largest gradient entry (the bounds of test_train_head_dims.py::test_encoder_backward_head_dims)"""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTEncoder
    cfg = ENC_CFGS[name]
    st = _state(cfg)
    x = synth.bag(N, cfg["mlp_dim"], tag=f"asm/train/{name}/{N}")
    G = synth.normal(f"asm/G/{name}/{N}", (N, cfg["mlp_dim"]))
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    enc = RRTEncoder(drop_out=0., **cfg)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    assert y.grad_fn is not None
    err = _maxerr(y.detach().cpu().numpy(), y64.detach().numpy())
    assert err <= 2e-4, f"{name} train forward: max-abs {err:.3e}"
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    floor = 1e-3 * max([float(x_leaf.grad.abs().max())] + [float(v.grad.abs().max()) for v in params.values()
                                                           if v.grad is not None])

    def rel(got, ref, what):
        ref = ref.astype(np.float64)
        e = np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), floor, 1e-6)
        assert np.isfinite(got).all(), what
        assert e <= 2e-3, f"{name} {what}: max error {e:.2e} of the largest gradient entry"

    rel(xd.grad.cpu().numpy(), x_leaf.grad.numpy(), "dx")
    for pname, prm in enc.named_parameters():
        ref = params[pname].grad
        assert prm.grad is not None, pname
        if pname.endswith("pe.bias"):
            assert float(prm.grad.abs().max()) == 0.0 and float(ref.abs().max()) < 1e-6     # Identity 2
            continue
        rel(prm.grad.cpu().numpy(), ref.numpy().reshape(prm.shape), pname)
