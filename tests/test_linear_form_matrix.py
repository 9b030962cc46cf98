"""GPU (-m gpu): every kernel form of csrc/linear_f32.hip -- linear_kernel, linear_ws_kernel (fp32 operands, 16-bit images,
split images; once / deferred epilogue), linear_splitk_kernel -- against the float64 product of the operands as the mode sees
them, at the smallest shape that still selects the form.

Reach.  Every case names the form it is there for (`ws<9,1>/unpart/f32/defer/cap512`); the test first asks rrt_linear_plan --
the function the launchers dispatch from -- and fails if the shape no longer selects that form.  The cases go through
rrt_debug_linear_f32, which sets the whole epilogue (solo, dropout, zero64: what rrt_linear*_f32 cannot pass).

Two input families per case:
  integer  operands, bias, residual in -3..3 from element indices modulo 251 / 241, q_scale 0.5, ReLU, dropout scale 2: every
           sum is an integer below 2^24, so every precision is exact and the comparison is np.array_equal -- a misplaced row,
           column or K tile moves a value by at least 1.
  synth    synth.normal x synth.uniform(-1, 1) / sqrt(K), magnitudes clamped to >= 2^-6 (no rounded operand is an fp16
           subnormal), against float64.  Tolerance: 4 x the error of an fp32 fma chain over K in index order (+ the fp32
           epilogue) on 64 sample rows, floored at 8 x 2^-24 x max |ref|; activations add L_act x that + 4 x the error of
           torch's CPU fp32 activation on the case's own pre-activation values.  Measured on the reference side only.

Outputs go into NaN-filled buffers with canary rows behind them (un-partition: the buffer holds the pad tokens' rows too,
which must stay NaN), the residual into a guarded buffer of its own; inputs must come back unmodified.  The case list is
plain module data: tests/test_linear_form_grid_cpu.py checks on the CPU that it covers what is claimed.  Importing this
module needs no device."""
import collections
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth

pytestmark = pytest.mark.gpu

RECORDS = []                      # (form, shape, family, chain error, tolerance, measured error)
from hip_util import CANARY, CANARY_ROWS      # noqa: E402  (rows behind every guarded buffer, their fill value)
DROP_P, DROP_SEED, DROP_LAYER = 0.5, 0x1234567887654321, 1
ACT_LIPSCHITZ = {"relu": 1.0, "gelu": 1.13, "tanh": 1.0, "sigmoid": 0.25}
ACT_CODE = {"relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU, "tanh": _lib.ACT_TANH, "sigmoid": _lib.ACT_SIGMOID}
OPS_CODE = {"f32": _lib.LINEAR_OPS_F32, "16": _lib.LINEAR_OPS_16, "x3": _lib.LINEAR_OPS_SPLIT}
PREC_NAME = {0: "f32", 1: "bf16", 2: "f16", 3: "x3"}
MODE_NAME = {0: "plain", 1: "unpart", 2: "act", 3: "unpart+drop", 4: "drop"}
# epilogue of a case -> RRT_LINEAR_EPI_* of its plan query
EPI_KIND = {"bias+q": 0, "nobias": 0, "relu": 2, "gelu": 2, "tanh": 2, "sigmoid": 2, "unpart": 1, "unpart+q": 1, "drop": 4,
            "unpart+drop": 3}

Case = collections.namedtuple("Case", "ops compute M N K epi solo zero64 H rn form")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_LINEAR_FORM_ERRORS_OUT")      # the table kept as profiles/linear_form_errors.txt
    if out and RECORDS:
        with open(out, "w") as fh:
            fh.write(error_table(RECORDS))


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """a device error is sticky: nothing more is started on a device that reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is run on it: {e}", returncode=3)


def error_table(records):
    lines = [f"{'form':44s} {'M x N x K':>18s} {'epilogue':12s} {'family':8s} {'chain err':>10s} {'tolerance':>10s} {'error':>10s}"]
    for form, shape, epi, fam, chain, tol, err in records:
        lines.append(f"{form:44s} {shape:>18s} {epi:12s} {fam:8s} {chain:10.2e} {tol:10.2e} {err:10.2e}")
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------ forms
def form_of(ops, plan):
    """the name of the kernel form a plan (dict of _lib.LINEAR_PLAN_FIELDS) stands for"""
    mode = MODE_NAME[plan["mode"]]
    if plan["kernel"] == _lib.LINEAR_KERNEL_SPLITK:
        return f"splitk<{plan['mt']},{plan['kg']}{',drop' if plan['drop'] else ''}>/{mode}/f32"
    prec = PREC_NAME[plan["prec"]]
    tile = f"<{plan['mt']},{plan['nt']}>"
    if plan["kernel"] == _lib.LINEAR_KERNEL_PLAIN:
        return f"plain{tile}/{mode}/{prec}/{'rounds' if plan['ntiles'] > plan['grid'] else 'once'}/cap{plan['cap']}"
    return f"{'ws16' if ops == '16' else 'ws'}{tile}/{mode}/{prec}/{'defer' if plan['defer'] else 'once'}/cap{plan['cap']}"


def instantiation(ops, plan):
    """(kernel, MT, NT, mode, precision, defer): what tests/test_linear_form_grid_cpu.py reads out of linear_f32.hip"""
    if plan["kernel"] == _lib.LINEAR_KERNEL_SPLITK:
        return ("splitk", plan["mt"], plan["kg"], MODE_NAME[plan["mode"]], "f32", 0)
    kern = "plain" if plan["kernel"] == _lib.LINEAR_KERNEL_PLAIN else "ws16" if ops == "16" else "ws"
    return (kern, plan["mt"], plan["nt"], MODE_NAME[plan["mode"]], PREC_NAME[plan["prec"]], plan["defer"])


def plan_of(c):
    return _lib.linear_plan(c.M, c.N, c.K, c.compute, OPS_CODE[c.ops], EPI_KIND[c.epi], c.solo, c.zero64)


def straight_unpart(c, nt):
    """the kernel's own choice (not in the plan): the straight-line un-partition store"""
    return c.epi == "unpart" and c.N % (64 * nt) == 0


# ------------------------------------------------------------------ the case list
# One row per (operand kind, tile form): the smallest shape that selects it (rrt_linear_plan on every case says so).
# (ops, precision class, tile form, M, N, K, solo, un-partition geometry (H, rn, N, K) with Np = H * H in the same band of
#  the rule, K depths or None where the rule pins K)
F32, LOW, I16, X3 = "f32", "low", "16", "x3"
ROWS = [
    (F32, F32, "plain<2,1>/once/cap512", 16, 64, 32, 0, (12, 4, 130, 32), None),
    (F32, F32, "plain<2,1>/rounds/cap512", 12500, 130, 32, 0, (116, 4, 130, 32), None),
    (F32, F32, "plain<4,1>/once/cap512", 2761, 130, 64, 0, (60, 4, 130, 64), None),
    (F32, F32, "plain<4,1>/rounds/cap512", 27500, 130, 64, 0, (172, 4, 130, 64), None),
    (F32, F32, "plain<4,1>/once/cap1024", 2090, 512, 512, 0, (52, 4, 512, 512), None),
    (F32, F32, "plain<4,1>/rounds/cap1024", 14000, 512, 512, 0, (118, 2, 512, 512), None),
    (F32, F32, "ws<6,1>/once/cap768", 8000, 512, 256, 0, (90, 9, 512, 256), None),
    (F32, F32, "ws<8,1>/once/cap512", 5500, 130, 64, 0, (76, 4, 130, 64), None),
    (F32, F32, "ws<8,1>/defer/cap512", 38500, 130, 64, 0, (196, 7, 130, 64), None),
    (F32, F32, "ws<8,1>/once/cap768", 9500, 512, 512, 0, (100, 10, 512, 512), None),
    (F32, F32, "ws<9,1>/once/cap768", 4500, 512, 512, 0, (66, 6, 512, 512), None),
    (F32, F32, "ws<9,1>/once/cap512", 11000, 130, 64, 0, (105, 5, 130, 64), None),
    (F32, F32, "ws<9,1>/defer/cap512", 5500, 1536, 64, 0, (74, 2, 1536, 64), "f32"),
    (F32, F32, "ws<8,1>/defer/cap512", 4901, 1536, 64, 0, (70, 7, 1536, 64), "f32"),
    # fp32 operands rounded to bf16 / fp16 behind LDS
    (F32, LOW, "plain<2,1>/once/cap512", 16, 64, 32, 0, (12, 4, 130, 32), None),
    (F32, LOW, "plain<4,1>/once/cap512", 2761, 130, 64, 0, (60, 4, 130, 64), None),
    (F32, LOW, "ws<8,1>/once/cap512", 5500, 130, 64, 0, (76, 4, 130, 64), None),
    (F32, LOW, "ws<9,1>/once/cap512", 11000, 130, 64, 0, (105, 5, 130, 64), None),
    (F32, LOW, "ws<6,1>/once/cap768", 16500, 130, 64, 0, (130, 10, 130, 64), None),
    (F32, LOW, "ws<6,1>/defer/cap768", 25000, 130, 64, 0, (160, 8, 130, 64), None),
    (F32, LOW, "ws<6,1>/defer/cap768", 3101, 1536, 64, 0, (56, 8, 1536, 64), "f32"),
    (F32, LOW, "ws<9,2>/once/cap256", 4500, 256, 1024, 0, (66, 6, 256, 1024), None),
    # 16-bit images
    (I16, LOW, "ws16<2,1>/once/cap512", 16, 64, 64, 0, (12, 4, 1536, 64), None),
    (I16, LOW, "ws16<4,1>/once/cap512", 321, 1536, 64, 0, (20, 4, 1536, 64), None),
    (I16, LOW, "ws16<6,1>/once/cap768", 1053, 64, 64, 0, (28, 4, 1536, 64), None),
    (I16, LOW, "ws16<6,1>/defer/cap768", 5500, 1536, 64, 0, (74, 2, 1536, 64), "16"),
    (I16, LOW, "ws16<8,1>/once/cap512", 992, 1536, 64, 0, (33, 3, 1536, 64), None),
    (I16, LOW, "ws16<8,1>/defer/cap512", 9500, 512, 64, 0, (100, 10, 512, 64), None),
    (I16, LOW, "ws16<8,1>/defer/cap512", 3501, 1536, 64, 0, (60, 6, 1536, 64), "16"),
    (I16, LOW, "ws16<9,1>/once/cap512", 1297, 1536, 64, 0, (66, 6, 512, 64), None),
    (I16, LOW, "ws16<4,1>/once/cap1024", 2090, 512, 512, 0, (52, 4, 512, 512), None),
    (I16, LOW, "ws16<6,2>/once/cap512", 7000, 512, 512, 0, (90, 9, 512, 512), None),
    (I16, LOW, "ws16<8,2>/defer/cap256", 12000, 512, 512, 0, (110, 10, 512, 512), None),
    (I16, LOW, "ws16<6,1>/once/cap1024", 9500, 512, 512, 1, (100, 10, 512, 512), None),
    (I16, LOW, "ws16<9,1>/once/cap768", 12500, 512, 512, 1, (114, 6, 512, 512), None),
    (I16, LOW, "ws16<8,2>/once/cap512", 14000, 512, 512, 1, (120, 8, 512, 512), None),
    (I16, LOW, "ws16<9,2>/once/cap512", 16500, 512, 512, 1, (129, 3, 512, 512), None),
    # split images
    (X3, X3, "ws<8,1>/once/cap512", 16, 64, 64, 0, (12, 4, 64, 64), None),
    (X3, X3, "ws<8,1>/defer/cap512", 24500, 192, 64, 0, (158, 2, 192, 64), "f32"),
    (X3, X3, "ws<9,1>/once/cap512", 1297, 1536, 64, 0, (105, 5, 192, 64), None),
    (X3, X3, "ws<9,1>/defer/cap512", 33000, 256, 64, 0, (74, 2, 1536, 64), "f32"),
]
# rows that also run all four activations (one per kernel and operand kind); every other row that has the mode runs ReLU
ALL_ACTS = {(F32, F32, "plain<2,1>/once/cap512"), (F32, F32, "ws<8,1>/once/cap512"), (F32, F32, "ws<9,1>/defer/cap512"),
            (F32, LOW, "ws<6,1>/once/cap768"), (I16, LOW, "ws16<6,1>/once/cap768"), (I16, LOW, "ws16<6,1>/defer/cap768")}
# K tiles per deferred form: the flush loop behind the K loop (nk < MT), the kt <= MT branch, the odd-nk copy
K_DEPTHS_16 = (1, 2, 3, 8)


def k_depths(kind, mt):
    return K_DEPTHS_16 if kind == "16" else tuple(sorted({1, 2, 3, mt - 1, mt, mt + 1, 16}))


def _named(base, mode, prec):
    """tile form of a row + epilogue + precision -> the full form name (form_of's layout)"""
    kern, rest = base.split("/", 1)
    return f"{kern}/{mode}/{prec}/{rest}"


def _cases():
    out = []
    for ops, pc, base, M, N, K, solo, (H, rn, Nu, Ku), depths in ROWS:
        computes = {F32: (0,), LOW: (1, 2), X3: (3,)}[pc]
        mt = int(base.split("<")[1].split(",")[0])
        for compute in computes:
            prec = PREC_NAME[compute]
            acts = ("relu", "gelu", "tanh", "sigmoid") if (ops, pc, base) in ALL_ACTS else ("relu",)
            epis = ["bias+q", "nobias"] + ([] if ops == X3 else list(acts)) + ["unpart", "unpart+q"]
            if ops == F32 and pc == F32:
                epis += ["drop", "unpart+drop"]
            for epi in epis:
                mode = MODE_NAME[EPI_KIND[epi]]
                p = "f32" if "drop" in epi else prec
                if epi.startswith("unpart"):
                    out.append(Case(ops, compute, H * H, Nu, Ku, epi, solo, 0, H, rn, _named(base, mode, p)))
                else:
                    out.append(Case(ops, compute, M, N, K, epi, solo, 0, 0, 0, _named(base, mode, p)))
            if depths:
                for nk in k_depths(depths, mt):
                    Kd = nk * (64 if depths == "16" else 32)
                    if Kd != K:
                        out.append(Case(ops, compute, M, N, Kd, "bias+q", solo, 0, 0, 0, _named(base, "plain", prec)))
                    if Kd != Ku:
                        out.append(Case(ops, compute, H * H, Nu, Kd, "unpart", solo, 0, H, rn, _named(base, "unpart", prec)))
    # split-K (the GEMMs of CR-MSA's representatives with one bag in flight): solo = 1, plain / dropout epilogues only
    for M in (17, 192, 512):
        out.append(Case(F32, 0, M, 1536, 256, "bias+q", 1, 0, 0, 0, "splitk<2,4>/plain/f32"))
    for M, N, K in ((17, 130, 256), (192, 130, 512), (17, 512, 512), (192, 512, 256)):
        out.append(Case(F32, 0, M, N, K, "bias+q" if N == 130 else "nobias", 1, 0, 0, 0, "splitk<1,4>/plain/f32"))
    out.append(Case(F32, 0, 192, 512, 512, "drop", 1, 0, 0, 0, "splitk<1,4,drop>/drop/f32"))
    out.append(Case(F32, 0, 17, 130, 256, "drop", 1, 0, 0, 0, "splitk<1,4,drop>/drop/f32"))
    # the zero64 side job: one plain-kernel and one warp-specialised case (with it set the split-K form is not taken)
    out.append(Case(F32, 0, 16, 64, 32, "bias+q", 1, 1, 0, 0, "plain<2,1>/plain/f32/once/cap512"))
    out.append(Case(F32, 0, 5500, 130, 64, "bias+q", 0, 1, 0, 0, "ws<8,1>/plain/f32/once/cap512"))
    out.append(Case(I16, 1, 1053, 64, 64, "nobias", 0, 1, 0, 0, "ws16<6,1>/plain/bf16/once/cap768"))
    # ragged N (no multiple of 64, scalar store tail) on 16-bit and split images: the rows above give those kernels whole columns
    out.append(Case(I16, 1, 1053, 130, 64, "bias+q", 0, 0, 0, 0, "ws16<6,1>/plain/bf16/once/cap768"))
    out.append(Case(I16, 2, 1053, 130, 64, "relu", 0, 0, 0, 0, "ws16<6,1>/act/f16/once/cap768"))
    out.append(Case(I16, 1, 33 * 33, 130, 64, "unpart", 0, 0, 33, 3, "ws16<6,1>/unpart/bf16/once/cap768"))
    out.append(Case(X3, 3, 1297, 130, 64, "bias+q", 0, 0, 0, 0, "ws<8,1>/plain/x3/once/cap512"))
    out.append(Case(X3, 3, 33 * 33, 130, 64, "unpart", 0, 0, 33, 3, "ws<8,1>/unpart/x3/once/cap512"))
    return out


CASES = _cases()


def case_id(c):
    geo = f"H{c.H}rn{c.rn}" if c.H else f"M{c.M}"
    return f"{c.ops}-{PREC_NAME[c.compute]}-{geo}x{c.N}x{c.K}-{c.epi}-s{c.solo}{'-z' if c.zero64 else ''}"


def families(c):
    return ("integer", "synth") if c.epi not in ("gelu", "tanh", "sigmoid") else ("synth",)


# ------------------------------------------------------------------ inputs
def _ints(shape, prime, shift=0):
    """integers in -3 .. 3 from the element index modulo two primes above the largest tile dimension"""
    x = np.arange(int(np.prod(shape)), dtype=np.int64) + shift
    other = 241 if prime == 251 else 251
    a, b = x % prime, x % other                        # (a, b) repeats after 251 * 241 elements only
    ta, tb = (a * a * a * 5 + a * 11) % prime, (b * b * b * 3 + b * 7) % other      # cubics: no short period modulo 7
    return (((ta + tb) % 7) - 3).astype(np.float32).reshape(shape)


def _clamped(a):
    """magnitudes >= 2^-6, signs kept"""
    return np.where(a < 0, np.minimum(a, -2.0 ** -6), np.maximum(a, 2.0 ** -6)).astype(np.float32)


@functools.lru_cache(maxsize=6)
def matrices(family, M, N, K):
    if family == "integer":
        return _ints((M, K), 251), _ints((N, K), 241)
    A = _clamped(synth.normal(f"lfm/A{M}x{K}", (M, K)))
    B = (_clamped(synth.uniform(f"lfm/B{N}x{K}", (N, K), -1, 1)) / np.float32(np.sqrt(K))).astype(np.float32)
    return A, B


def grid_of(c):
    return _lib.region_grid(c.H * c.H - c.H - 3, c.rn) if c.H else None


@functools.lru_cache(maxsize=3)
def _synth_resid(L, N):
    return synth.normal(f"lfm/r{L}x{N}", (L, N))


def inputs(c, family):
    """A [M, K], B [N, K], bias [N] or None, resid [L, N] or None, q_cols, q_scale"""
    A, B = matrices(family, c.M, c.N, c.K)
    L = c.H * c.H - c.H - 3
    if family == "integer":
        bias = ((np.arange(c.N) * 5) % 7 - 3).astype(np.float32)
        resid = _ints((L, c.N), 251, shift=17) if c.H else None
        q_scale = 0.5
    else:
        bias = synth.uniform(f"lfm/b{c.N}", (c.N,), -0.5, 0.5)
        resid = _synth_resid(L, c.N) if c.H else None
        q_scale = 0.125
    if c.epi == "nobias":
        bias = None
    q_cols = c.N // 3 if c.epi in ("bias+q", "unpart+q") else 0
    return A, B, bias, resid, q_cols, q_scale


def seen(a, c, f32=False):
    """an operand as the mode's MFMA sees it (float64); split images: (hi, lo)"""
    if c.ops == X3:
        return O.split_hi_lo(a)
    if c.compute in (1, 2) and "drop" not in c.epi:
        return O.round_lowp(a, "bf16" if c.compute == 1 else "f16")
    return a.astype(np.float64)


@functools.lru_cache(maxsize=3)
def _product(family, ops, compute, M, N, K):
    c = Case(ops, compute, M, N, K, "nobias", 0, 0, 0, 0, "")
    A, B = matrices(family, M, N, K)
    if ops == X3:
        return O.split_matmul_t(A, B)
    return seen(A, c) @ seen(B, c).T


def product64(c, family):
    return _product(family, c.ops, c.compute, c.M, c.N, c.K)


def keep_mask(c):
    from hip_util import dropout_keep
    return dropout_keep(DROP_SEED, DROP_LAYER, c.M, c.N, DROP_P) if "drop" in c.epi else None


def _act(z, name):
    t = torch.from_numpy(np.ascontiguousarray(z))
    fn = {"relu": torch.relu, "gelu": torch.nn.functional.gelu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[name]
    return fn(t).numpy()


def epilogue(P, c, bias, q_cols, q_scale, keep, dt, rows=None, act=True):
    """the kernel's epilogue in `dt` on the product rows P (`rows`: their A-row indices, all when None), before the
    un-partition: (acc + bias) * q-scale, activation, dropout"""
    Z = P.astype(dt)
    if bias is not None:
        Z = Z + bias.astype(dt)
    if q_cols:
        Z[:, :q_cols] = Z[:, :q_cols] * dt(q_scale)
    if act and c.epi in ACT_CODE:
        Z = _act(Z, c.epi)
    if keep is not None:
        k = keep if rows is None else keep[rows]
        Z = np.where(k, Z * dt(1.0 / (1.0 - DROP_P)), dt(0))
    return Z


def unpartition(Z, resid, g, dt):
    """[Np, N] slot rows -> [L, N] token rows + residual"""
    z = np.empty_like(Z)
    z[O.partition_index(g.H, g.s)] = Z
    return resid.astype(dt) + z[:g.L]


def sample_rows(c, mt):
    """64 A rows: first, last, one per row tile (evenly spaced tiles, a different row of each)"""
    bm = 16 * mt
    tiles = (c.M + bm - 1) // bm
    picks = {0, c.M - 1}
    for t in np.unique(np.linspace(0, tiles - 1, 62).astype(int)):
        picks.add(min(c.M - 1, int(t) * bm + (7 * int(t) + 3) % bm))
    return np.array(sorted(picks))


def chain32(c, family, rows):
    """fp32 fma chain over K in index order on the operands as the mode sees them: acc = float32(float64(acc) + a * b)"""
    A, B = matrices(family, c.M, c.N, c.K)
    a, b = seen(A[rows], c), seen(B, c)
    acc = np.zeros((len(rows), c.N), np.float32)
    for k in range(c.K):
        if c.ops == X3:
            (ah, al), (bh, bl) = a, b
            for x, y in ((ah, bl), (al, bh), (ah, bh)):
                acc = (acc.astype(np.float64) + x[:, k, None] * y[None, :, k]).astype(np.float32)
        else:
            acc = (acc.astype(np.float64) + a[:, k, None] * b[None, :, k]).astype(np.float32)
    return acc


def reference(c, family, mt):
    """float64 result [rows_out, N] and, for synth, the tolerance with the figures it comes from"""
    A, B, bias, resid, q_cols, q_scale = inputs(c, family)
    P, keep, g = product64(c, family), keep_mask(c), grid_of(c)
    ref = epilogue(P, c, bias, q_cols, q_scale, keep, np.float64)
    out = unpartition(ref, resid, g, np.float64) if c.H else ref
    if family == "integer":
        return dict(ref=out)
    rows = sample_rows(c, mt)
    pre64 = epilogue(P, c, bias, q_cols, q_scale, keep, np.float64, act=False)
    pre32 = epilogue(chain32(c, family, rows), c, bias, q_cols, q_scale, keep, np.float32, rows=rows, act=False)
    if c.H:                                   # compare at the token rows of the sampled slots (pad slots write nothing)
        tok = O.partition_index(g.H, g.s)[rows]
        real = tok < g.L
        want = resid.astype(np.float64)[tok[real]] + pre64[rows[real]]
        got = resid[tok[real]] + pre32[real]
        scale = np.abs(out).max()
    else:
        want, got, scale = pre64[rows], pre32, np.abs(pre64).max()
    chain = float(np.abs(got.astype(np.float64) - want).max())
    tol = max(4.0 * chain, 8.0 * 2.0 ** -24 * float(scale))
    e_act = 0.0
    if c.epi in ACT_CODE:
        e_act = float(np.abs(_act(pre64.astype(np.float32), c.epi).astype(np.float64) - _act(pre64, c.epi)).max())
        tol = ACT_LIPSCHITZ[c.epi] * tol + 4.0 * e_act
    return dict(ref=out, tol=tol, chain=chain, e_act=e_act, pre64=pre64)


def reference32(c, family):
    """numpy's fp32 matmul of the operands as the mode sees them + the fp32 epilogue (the CPU module holds it to the tolerance)"""
    A, B, bias, resid, q_cols, q_scale = inputs(c, family)
    if c.ops == X3:
        (ah, al), (bh, bl) = (tuple(x.astype(np.float32) for x in seen(m, c)) for m in (A, B))
        P = ah @ bl.T + al @ bh.T + ah @ bh.T
    else:
        P = seen(A, c).astype(np.float32) @ seen(B, c).astype(np.float32).T
    Z = epilogue(P, c, bias, q_cols, q_scale, keep_mask(c), np.float32)
    return unpartition(Z, resid, grid_of(c), np.float32) if c.H else Z


# ------------------------------------------------------------------ the device side
def _image(a, c):
    """the operand as the entry point takes it: fp32, 16-bit image, split image (device tensors)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if c.ops == I16:
        return torch.from_numpy(a).to(torch.bfloat16 if c.compute == 1 else torch.float16).view(torch.int16).to("cuda:0")
    if c.ops == X3:
        t = torch.from_numpy(a.reshape(-1, 32))
        hi = t.to(torch.bfloat16)
        lo = (t - hi.float()).to(torch.bfloat16)
        return torch.cat([hi.view(torch.int16), lo.view(torch.int16)], dim=1).reshape(-1).to("cuda:0")
    return torch.from_numpy(a).to("cuda:0")


def _guarded(rows, cols, fill):
    buf = torch.full((rows + CANARY_ROWS, cols), float("nan"), device="cuda:0")
    if fill is not None:
        buf[:rows] = torch.from_numpy(fill).to("cuda:0")
    buf[rows:] = CANARY
    return buf


def run(c, family, solo=None):
    """rrt_debug_linear_f32 on the case -> (out [rows_out, N] numpy, list of violated guards)"""
    lib = _lib.load()
    A, B, bias, resid, q_cols, q_scale = inputs(c, family)
    g = grid_of(c)
    dA, dB = _image(A, c), _image(B, c)
    db = None if bias is None else torch.from_numpy(bias).to("cuda:0")
    rows_out = c.M                                                   # un-partition: Np rows, the pad tokens' included
    out = _guarded(rows_out, c.N, None)
    dr = _guarded(g.L, c.N, resid) if c.H else None
    z = torch.full((65,), -1, dtype=torch.int32, device="cuda:0")
    z[64] = 0x5A5A5A5A
    keepA, keepB, keepb, keepr = dA.clone(), dB.clone(), None if db is None else db.clone(), None if dr is None else dr.clone()
    ptr = lambda t: None if t is None else t.data_ptr()
    act = ACT_CODE.get(c.epi, 0)
    _lib.check(lib.rrt_debug_linear_f32(ptr(dA), ptr(dB), ptr(db), ptr(dr), ptr(out), c.M, c.N, c.K,
                                        C.byref(g) if c.H else None, OPS_CODE[c.ops], c.compute, q_cols, q_scale, act,
                                        c.solo if solo is None else solo, DROP_P if "drop" in c.epi else 0.0, DROP_SEED,
                                        DROP_LAYER, ptr(z) if c.zero64 else None, torch.cuda.current_stream().cuda_stream),
               "rrt_debug_linear_f32")
    torch.cuda.synchronize()
    bad = []
    written = g.L if c.H else c.M
    if torch.isnan(out[:written]).any():
        bad.append("NaN left in a written row")
    if c.H and not torch.isnan(out[written:rows_out]).all():
        bad.append("a pad token's row was written")
    if not (out[rows_out:] == CANARY).all():
        bad.append("canary rows behind the output")
    if dr is not None and not torch.equal(dr, keepr):
        bad.append("residual (or the canary behind it) modified")
    if not (torch.equal(dA, keepA) and torch.equal(dB, keepB) and (db is None or torch.equal(db, keepb))):
        bad.append("an input was modified")
    zc = z.cpu().numpy()
    if c.zero64 and not ((zc[:64] == 0).all() and zc[64] == 0x5A5A5A5A):
        bad.append("zero64: 64 ints zero, the one behind untouched")
    if not c.zero64 and not (zc[:64] == -1).all():
        bad.append("zero64 buffer touched without being passed")
    return out[:written].cpu().numpy(), bad


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_form_against_float64(c):
    plan = plan_of(c)
    assert form_of(c.ops, plan) == c.form, f"the shape no longer selects the form this case is for: {plan}"
    for family in families(c):
        r = reference(c, family, plan["mt"])
        got, bad = run(c, family)
        assert not bad, (family, bad)
        shape = f"{c.M}x{c.N}x{c.K}"
        if family == "integer":
            assert np.abs(r["ref"]).max() < 2 ** 24
            wrong = int((got != r["ref"]).sum())
            RECORDS.append((c.form, shape, c.epi, family, 0.0, 0.0, float(np.abs(got - r["ref"]).max())))
            assert wrong == 0, f"integer: {wrong} of {got.size} values differ, first at {np.argwhere(got != r['ref'])[:3].tolist()}"
            continue
        err = float(np.abs(got.astype(np.float64) - r["ref"]).max())
        RECORDS.append((c.form, shape, c.epi, family, r["chain"], r["tol"], err))
        print(f"{case_id(c)} {c.form}: chain {r['chain']:.3e} tol {r['tol']:.3e} err {err:.3e}")
        assert err <= r["tol"], f"synth: max-abs {err:.3e} > {r['tol']:.3e} (chain {r['chain']:.3e})"
        if c.compute in (1, 2) and "drop" not in c.epi:              # the mode really ran: off the exact product
            A, B, bias, resid, q_cols, q_scale = inputs(c, family)
            exact = epilogue(A.astype(np.float64) @ B.astype(np.float64).T, c, bias, q_cols, q_scale, None, np.float64)
            if c.H:
                exact = unpartition(exact, resid, grid_of(c), np.float64)
            assert np.abs(got - exact).max() > r["tol"], "reduced precision: the result is the exact product's"


# ------------------------------------------------------------------ bit claims of the comments
def _plain16(M, N, K, solo):
    return Case(I16, 1, M, N, K, "bias+q", solo, 0, 0, 0, "")


def test_bits_do_not_depend_on_the_tile_shape():
    """choose16: "The bits do not depend on the tile shape" -- 16-bit images, the solo = 0 and solo = 1 forms of one product;
    a once and a deferred form of equal N, K on their common rows (the small product's A is the head of the large one's)"""
    a, b = _plain16(7000, 512, 512, 0), _plain16(7000, 512, 512, 1)
    pa, pb = plan_of(a), plan_of(b)
    assert (pa["mt"], pa["nt"]) == (6, 2) and (pb["mt"], pb["nt"]) == (4, 1)
    ga, bad_a = run(a, "synth")
    gb, bad_b = run(b, "synth")
    assert not bad_a and not bad_b and np.array_equal(ga, gb)
    small, big = _plain16(992, 1536, 64, 0), _plain16(5500, 1536, 64, 0)
    ps, pbig = plan_of(small), plan_of(big)
    assert (ps["mt"], ps["defer"]) == (8, 0) and (pbig["mt"], pbig["defer"]) == (6, 1)
    A, B = matrices("synth", big.M, big.N, big.K)
    lib = _lib.load()
    outs = []
    db = torch.from_numpy(synth.uniform("lfm/bits/b", (1536,), -0.5, 0.5)).to("cuda:0")
    dB = _image(B, big)
    for c in (small, big):
        dA = _image(A[:c.M], c)
        out = _guarded(c.M, c.N, None)
        _lib.check(lib.rrt_debug_linear_f32(dA.data_ptr(), dB.data_ptr(), db.data_ptr(), None, out.data_ptr(), c.M, c.N, c.K,
                                            None, OPS_CODE[I16], 1, 512, 0.125, 0, 0, 0.0, 0, 0, None,
                                            torch.cuda.current_stream().cuda_stream), "rrt_debug_linear_f32")
        torch.cuda.synchronize()
        assert (out[c.M:] == CANARY).all()
        outs.append(out[:c.M])
    assert torch.equal(outs[0], outs[1][:small.M])


def test_split_k_against_the_plain_kernel():
    """solo = 1 (K split inside the block) against solo = 0 (linear_kernel): the K order differs, so the tolerance, not bits"""
    c = Case(F32, 0, 192, 512, 512, "bias+q", 1, 0, 0, 0, "")
    assert plan_of(c)["kernel"] == _lib.LINEAR_KERNEL_SPLITK and plan_of(c._replace(solo=0))["kernel"] == _lib.LINEAR_KERNEL_PLAIN
    r = reference(c, "synth", 1)
    g1, bad1 = run(c, "synth")
    g0, bad0 = run(c, "synth", solo=0)
    assert not bad1 and not bad0
    assert np.abs(g1.astype(np.float64) - g0).max() <= r["tol"]
    assert np.abs(g1 - r["ref"]).max() <= r["tol"] and np.abs(g0 - r["ref"]).max() <= r["tol"]


def test_refusals_launch_nothing():
    """what the launchers refuse comes back as RRT_E_UNSUPPORTED / RRT_E_INVALID and the output stays NaN"""
    lib = _lib.load()
    A, B = matrices("integer", 16, 64, 64)
    dA, dB = torch.from_numpy(A).to("cuda:0"), torch.from_numpy(B).to("cuda:0")
    out = torch.full((16, 64), float("nan"), device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def call(ops=0, compute=0, act=0, p=0.0, K=64, M=16):
        return lib.rrt_debug_linear_f32(dA.data_ptr(), dB.data_ptr(), None, None, out.data_ptr(), M, 64, K, None, ops, compute, 0,
                                        1.0, act, 0, p, 1, 0, None, st)
    assert call(compute=1, p=0.5) == -2 and call(act=1, p=0.5) == -2          # dropout: exact fp32, no activation
    assert call(ops=1, compute=1, p=0.5) == -2 and call(ops=2, compute=3, act=1) == -2
    assert call(ops=1, compute=0) == -2 and call(ops=0, compute=3) == -2 and call(ops=2, compute=0) == -2
    assert call(K=48) == -2 and call(ops=1, compute=1, K=32) == -2
    assert call(M=0) == -1 and call(act=5) == -1 and call(p=1.0) == -1 and call(ops=3) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
