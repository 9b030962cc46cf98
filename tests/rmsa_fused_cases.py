"""Case lists, input builder, restatement and restated dispatch rules for tests/test_rmsa_fused_peaked.py (GPU) and
tests/test_rmsa_fused_peaked_cpu.py.  Plain module data and CPU code: importing it needs no device.

The fused R-MSA entries take (u, W, b, taps), not qkv, so a peaked score map has to be planted through the weights.  A
KEY-ONLY CHANNEL does it: column 0 of u is zero, the q and v rows of W have a zero in column 0, the k rows carry +-a there
(a = mean |k-row weight| x sqrt(D), signs from synth).  Writing beta into u[r, j, 0] then adds beta (+-a) to key j of region
r in every head and touches no query and no value: column j of the score map (EPEG included -- the stencil runs along the
query axis) is the row maximum for the queries with q . a_h > 0 and the row minimum for the others.  Afterwards the q and the
k rows of W and b (never v) are scaled by one factor so that the largest |score| of the float64 restatement is about 50."""
import collections
import functools

import numpy as np
import torch

from rrt_mil_amd import synth

HD = 64                               # the fused kernels' head dim
BETA = 16.0
PEAK_TARGET, PEAK_WINDOW = 50.0, (40.0, 60.0)
L2E = 1.4426950408889634
EKS = (0, 15, 21, 63)
VARIANTS = ("plain", "runmax", "masked", "ties_k", "ties_q")

# ------------------------------------------------------------------ the dispatch rules, restated
# Source: the RRT_FUSED / RRT_FUSED16 / RRT_PAIR16 / RRT_X3 ladders and the *_supported predicates in csrc/rmsa_fused.hip,
# rmsa_fused16.hip, rmsa_pair16.hip, rmsa_fused_x3.hip (tests/test_rmsa_fused_peaked_cpu.py reads the ladders back out of
# the source text).  A ladder is [(largest P, MT)] in ascending order.
LADDERS = {
    "fused_f32": [(64, 4), (96, 6), (112, 7), (128, 8), (144, 9), (176, 11), (208, 13)],
    "fused16": [(32, 2), (64, 4), (96, 6), (112, 7), (128, 8), (144, 9), (176, 11), (208, 13), (240, 15), (256, 16)],
    "pair16": [(32, 2), (64, 4), (96, 6), (112, 7), (128, 8), (144, 9), (176, 11)],
    "x3": [(64, 4), (96, 6), (112, 7), (128, 8), (144, 9)],
}
LADDERS["fused_proj"] = [(p_, m) for p_, m in LADDERS["fused_f32"] if m > 4]       # regions of <= 64 tokens keep two launches
P_MIN = {"fused_f32": 49, "fused_proj": 65, "fused16": 17, "pair16": 17, "x3": 49}
VT_PITCH = 512


def mt_of(kernel, P):
    """the row-tile count MT the kernel is instantiated with for a region of P tokens"""
    assert P >= P_MIN[kernel], (kernel, P)
    return next(m for top, m in LADDERS[kernel] if P <= top)


def mt_used(P):
    return (P + 15) // 16


def split_last(kernel, P):
    """rmsa_fused_kernel's SPLIT_LAST: nine row tiles on eight waves, the ninth merged from nine (max, sum, O) records"""
    return kernel in ("fused_f32", "fused_proj") and mt_of(kernel, P) == 9


def stencil_geo(BM, ek):
    """rmsa_pair16.hip::stencil_geo -> (H8, nstep, pitch)"""
    h8 = ((ek >> 1) + 7) & ~7
    nstep = (16 + 2 * h8 + 31) // 32
    return h8, nstep, (BM - 16 + 32 * nstep) * 2


def takes_pair(R, P, ek):
    """rmsa_pair16_supported at head dim 64: the library's choice inside rrt_rmsa_fused16"""
    if not (R >= 8 and 16 < P <= 176 and 0 <= ek <= 63):
        return False
    _, nstep, pitch = stencil_geo(16 * mt_of("pair16", P), ek)
    return pitch <= VT_PITCH and nstep <= 3


def pair_waves(P):
    """sixteen waves (two row halves per region) for 6 .. 9 row tiles, eight otherwise"""
    return 16 if 6 <= mt_of("pair16", P) <= 9 else 8


# ------------------------------------------------------------------ the cases
Case = collections.namedtuple("Case", "kernel variant P ek D heads R compute L")
Case.__new__.__defaults__ = (0, 0)


def _c(kernel, variant, P, ek, R=None, compute=0, D=128, L=0):
    if R is None:
        R = mt_used(P) if variant == "runmax" else 2
        if kernel == "pair16":
            R = (max(mt_used(P), 8) + 1) | 1       # at least one region per key tile and 9; odd: the half-empty last pair
    return Case(kernel, variant, P, ek, D, D // HD, R, compute, L)


def _cases():
    out = []
    # rrt_rmsa_fused_f32, exact fp32: a full and a ragged P per MT; masked; plain and ties at 144 and at a ragged P
    for P, ek in ((64, 15), (96, 21), (112, 63), (128, 0), (144, 15), (176, 21), (208, 63),
                  (49, 63), (81, 0), (100, 15), (113, 21), (137, 63), (169, 0), (196, 15)):
        out.append(_c("fused_f32", "runmax", P, ek))
    for P, ek in ((49, 63), (65, 0), (97, 15), (113, 21), (129, 15), (145, 63), (177, 0)):
        out.append(_c("fused_f32", "masked", P, ek))
    for v in ("plain", "ties_k", "ties_q"):
        out += [_c("fused_f32", v, 144, 15), _c("fused_f32", v, 137, 21)]
    out.append(_c("fused_f32", "plain", 144, 15, D=512))
    # ... with bf16 / fp16 matrix-core operands
    for compute in (1, 2):
        for v in ("plain", "runmax"):
            out += [_c("fused_f32", v, 144, 15, compute=compute), _c("fused_f32", v, 81, 21, compute=compute)]
    # the merged projection: two rounds of items (64 regions x 8 heads), MT = 9 and MT = 6
    out += [_c("fused_proj", "runmax", 144, 15, R=64, D=512, L=9000), _c("fused_proj", "runmax", 81, 15, R=64, D=512, L=5000)]
    # rrt_rmsa_fused16, the one-region kernel (fewer than 8 regions per call, or P > 176)
    for i, P in enumerate((32, 64, 96, 112, 128, 144, 176, 208, 240, 256)):
        out.append(_c("fused16", "runmax", P, EKS[(i + 1) % 4], compute=1))
    for i, P in enumerate((17, 33, 129, 209, 241)):
        out.append(_c("fused16", "masked", P, EKS[(i + 3) % 4], compute=1))
    out += [_c("fused16", "runmax", 144, 15, compute=2), _c("fused16", "runmax", 256, 0, compute=2)]
    out.append(_c("fused16", "plain", 144, 15, compute=1, D=512))
    # ... on >= 8 regions of <= 176 tokens: rmsa_pair16, eight and sixteen waves, the stencil in 1 / 2 / 3 steps and absent
    for P, ek in ((32, 15), (64, 63), (96, 21), (112, 0), (128, 15), (144, 21), (176, 63)):
        out.append(_c("pair16", "runmax", P, ek, compute=1))
    for P, ek in ((65, 21), (129, 15), (145, 0)):
        out.append(_c("pair16", "masked", P, ek, R=9, compute=1))
    out.append(_c("pair16", "runmax", 144, 15, compute=2))
    out.append(_c("pair16", "plain", 144, 15, R=9, compute=1, D=512))
    # rrt_rmsa_fused_x3
    for P, ek in ((64, 63), (96, 0), (112, 15), (128, 21), (144, 15)):
        out.append(_c("x3", "runmax", P, ek))
    out += [_c("x3", "masked", 129, 15), _c("x3", "plain", 137, 21), _c("x3", "plain", 144, 15, D=512)]
    return out


CASES = _cases()


def case_id(c):
    prec = {0: "", 1: "-bf16", 2: "-f16"}[c.compute]
    form = ""
    if c.kernel == "pair16":
        form = f"-w{pair_waves(c.P)}-s{stencil_geo(16 * mt_of('pair16', c.P), c.ek)[1] if c.ek else 0}"
    return f"{c.kernel}{prec}-{c.variant}-P{c.P}-k{c.ek}-D{c.D}-R{c.R}-MT{mt_of(c.kernel, c.P)}{form}"


def storage(c):
    """the format the kernel reads u and W in: the operands are rounded to it before anything is computed from them"""
    if c.kernel in ("fused16", "pair16"):
        return "bf16" if c.compute == 1 else "f16"
    return "f32"


def mode(c):
    """the restatement's rounding points for a case"""
    if c.kernel in ("fused16", "pair16"):
        return (c.kernel, "bf16" if c.compute == 1 else "f16")
    if c.kernel == "x3":
        return ("x3",)
    if c.compute:
        return ("ops", "bf16" if c.compute == 1 else "f16")
    return None


# ------------------------------------------------------------------ rounding, in torch, for any carrying dtype
_T16 = {"bf16": torch.bfloat16, "f16": torch.float16}


def r16(t, dt, flush=False):
    """round to bf16 / fp16 (nearest even, through float32 like a kernel that holds the value in a 32-bit register), kept in
    t's dtype.  flush: fp16 results below the smallest normal (2^-14) become zero."""
    out = t.float().to(_T16[dt]).to(t.dtype)
    if flush and dt == "f16":
        out = torch.where(out.abs() < 2.0 ** -14, torch.zeros_like(out), out)
    return out


def split_hi_lo(t):
    """(hi, lo) bf16 pair of an fp32 value: hi = bf16(x), lo = bf16(x - hi)"""
    a = t.float().to(t.dtype)
    hi = r16(a, "bf16")
    return hi, r16(a - hi, "bf16")


def _np16(a, dt):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(_T16[dt]).float().numpy()


# ------------------------------------------------------------------ the restatement
def _stencil(x, taps, ek, P, start):
    """start + sum_t taps[h, t] x[.., i + t - ek / 2, ..] along axis 2 of x [R, heads, P, *], zero padded"""
    half = ek // 2
    xp = torch.nn.functional.pad(x, (0, 0, half, half))
    acc = start
    for t in range(ek):
        acc = acc + taps[None, :, t, None, None] * xp[:, :, t:t + P]
    return acc


def restate(u, W, b, taps, R, P, D, heads, ek, dtype, mode=None, flush=False):
    """projection and bias, q hd^-0.5, scores, the EPEG stencil, softmax, A V -- plain torch ops on the CPU, carried in
    `dtype` (float64: the reference; float32: what e32 is measured with).  mode: None -- exact, the stencil explicit on the
    [P, P] score map with an arbitrary constant bias that must drop out; ("ops", dt) -- u and W rounded, the rest exact (the
    fp32 kernel with 16-bit matrix-core operands); ("fused16", dt) / ("pair16", dt) -- the rounding points the headers of
    rmsa_fused16.hip / rmsa_pair16.hip list; ("x3",) -- the hi + lo split of rmsa_fused_x3.  -> (O [R P, D], scores or None)"""
    tt = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)
    x, W, b = tt(u)[:R * P], tt(W), tt(b)
    w = tt(taps) if ek else None
    hd = D // heads
    kind = mode[0] if mode else None
    if kind == "x3":
        xh, xl = split_hi_lo(x)
        wh, wl = split_hi_lo(W)
        qkv = xh @ wh.T + xh @ wl.T + xl @ wh.T
    else:
        if kind is not None:
            x, W = r16(x, mode[1]), r16(W, mode[1])
        qkv = x @ W.T
    qkv = (qkv + b).reshape(R, P, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * hd ** -0.5, qkv[1], qkv[2]
    kT = lambda a: a.transpose(-2, -1)
    if kind in (None, "ops"):
        S = q @ kT(k)
        scores = S
        if ek:
            scores = S + _stencil(S, w, ek, P, torch.zeros_like(S))
            S = scores + 0.37
        e = torch.exp(S - S.max(-1, keepdim=True).values)
        o = (e / e.sum(-1, keepdim=True)) @ v
        return o.transpose(1, 2).reshape(R * P, D), scores
    # the kernels' form: Q~ = Q + T Q, scores from Q~ log2(e), exp2
    if kind == "pair16":
        dt = mode[1]
        qt = r16(q * L2E, dt)
        if ek:
            wt = w.clone()
            wt[:, ek // 2] += 1.0                       # the identity tap rides in the band
            wt = wt.float().to(dtype)                   # (the table holds fp32 values)
            whi = r16(wt, dt)
            qt = _stencil(qt, whi + r16(wt - whi, dt), ek, P, torch.zeros_like(qt))
        S = r16(qt, dt) @ kT(r16(k, dt))
    else:
        qt = _stencil(q, w, ek, P, q) if ek else q
        if kind == "x3":
            qh, ql = split_hi_lo(qt * L2E)
            kh, kl = split_hi_lo(k)
            S = qh @ kT(kh) + qh @ kT(kl) + ql @ kT(kh)
        else:
            dt = mode[1]
            S = r16(qt * L2E, dt) @ kT(r16(k, dt))
    e = torch.exp2(S - S.max(-1, keepdim=True).values)
    if kind == "x3":
        eh, el = split_hi_lo(e)
        vh, vl = split_hi_lo(v)
        o = (eh @ vh + eh @ vl + el @ vh) / e.sum(-1, keepdim=True)
    else:
        o = (r16(e, dt, flush) @ r16(v, dt)) / e.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(R * P, D), None


# ------------------------------------------------------------------ the inputs
def _clamped(a, floor=2.0 ** -6):
    """magnitudes >= 2^-6 of the scale, signs kept: no rounded operand is an fp16 subnormal"""
    return np.where(a < 0, np.minimum(a, -floor), np.maximum(a, floor)).astype(np.float32)


def planted(c):
    """[(region, key, key tile)] of the planted keys"""
    if c.variant == "runmax":
        n = mt_used(c.P)
        out = []
        for r in range(c.R):
            t = r % n
            out.append((r, 16 * t + (7 * r + 3) % min(16, c.P - 16 * t), t))
        return out
    if c.variant == "masked":
        return [(r, c.P - 1, (c.P - 1) // 16) for r in range(c.R)]
    return []


Inputs = collections.namedtuple("Inputs", "u W b taps")


@functools.lru_cache(maxsize=4)
def inputs(c):
    """-> Inputs(u [(R + behind) P, D], W [3 D, D], b [3 D], taps [heads, max(ek, 1)]) as float32, representable in the
    case's storage format.  `masked` holds one more region's worth of rows, x 1e3, behind region R - 1."""
    R, P, D, heads, ek = c.R, c.P, c.D, c.heads, c.ek
    tag = f"rfp/{c.kernel}/{c.variant}/{P}/{ek}/{D}/{R}"
    behind = 1 if c.variant == "masked" else 0
    u = _clamped(synth.normal(tag + "/u", ((R + behind) * P, D)))
    W = (_clamped(synth.uniform(tag + "/w", (3 * D, D), -1, 1)) / np.float32(np.sqrt(D))).astype(np.float32)
    b = synth.uniform(tag + "/b", (3 * D,), -0.3, 0.3).astype(np.float32)
    taps = (synth.uniform(tag + "/pe", (heads, max(ek, 1)), -1, 1) / np.sqrt(max(ek, 1))).astype(np.float32)
    a = np.abs(W[D:2 * D]).mean() * np.sqrt(D)
    sign = np.where(synth.uniform(tag + "/s", (D,), -1, 1) < 0, -1.0, 1.0)
    u[:, 0] = 0.0
    W[:, 0] = 0.0
    W[D:2 * D, 0] = sign * a
    ur = u.reshape(R + behind, P, D)
    for r, j, _ in planted(c):
        ur[r, j, 0] = BETA
    if c.variant == "ties_k":
        ur[:R] = ur[:R, :1]
    if c.variant == "ties_q":
        W[:D] = 0.0
        b[:D] = 0.0
    if behind:
        ur[R] *= 1.0e3
    _, S = restate(u, W, b, taps, R, P, D, heads, ek, torch.float64)
    smax = float(S.abs().max())
    if smax > 0:
        g = np.float32(np.sqrt(PEAK_TARGET / smax))
        W[:2 * D] *= g
        b[:2 * D] *= g
    st = storage(c)
    if st != "f32":
        u, W = _np16(u, st), _np16(W, st)
    for a_ in (u, W, b, taps):
        a_.setflags(write=False)
    return Inputs(u, W, b, taps)


def reference(c, dtype=torch.float64, flush=False, exact=False):
    """the restatement of the case's own rounding points (exact: of none) on its inputs -> (O as float64 numpy, scores)"""
    i = inputs(c)
    o, S = restate(i.u, i.W, i.b, i.taps, c.R, c.P, c.D, c.heads, c.ek, dtype, None if exact else mode(c), flush)
    return o.double().numpy(), (None if S is None else S.double().numpy())


# ------------------------------------------------------------------ the projection bags
def proj_inputs(c):
    """out-projection weights, bias and residual of a fused_proj case, and the bag's geometry (H, s)"""
    from oracle import rrt_oracle as O
    H, s, _ = O.grid(c.L, 8)
    assert s * s == c.P and (H // s) ** 2 == c.R
    tag = f"rfp/proj/{c.L}"
    Wp = (synth.uniform(tag + "/wp", (c.D, c.D), -1, 1) / np.sqrt(c.D)).astype(np.float32)
    bp = synth.uniform(tag + "/bp", (c.D,), -0.5, 0.5).astype(np.float32)
    res = synth.normal(tag + "/r", (c.L, c.D))
    return Wp, bp, res, H, s


def proj_reference(c, dtype):
    """x1 = residual + un-partition(O Wp^T + bp), the projection carried in `dtype` too -> float64 numpy [L, D]"""
    from oracle import rrt_oracle as O
    i = inputs(c)
    Wp, bp, res, H, s = proj_inputs(c)
    o, _ = restate(i.u, i.W, i.b, i.taps, c.R, c.P, c.D, c.heads, c.ek, dtype)
    tt = lambda a: torch.from_numpy(a.astype(np.float64)).to(dtype)
    Z = o @ tt(Wp).T + tt(bp)
    z = torch.empty_like(Z)
    z[torch.from_numpy(O.partition_index(H, s))] = Z
    return (tt(res) + z[:c.L]).double().numpy()
