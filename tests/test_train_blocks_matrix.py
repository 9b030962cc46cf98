"""GPU (-m gpu): the building blocks of the training backward -- csrc/linear_bwd.hip (transpose, the split-K TN product with its
bias column sums, colsum, the partial reduce) and csrc/ln_bwd.hip (LayerNorm backward, the activation passes, partition_rows,
the drop-mask pass) -- form by form against float64, each form at the smallest shape that selects it.

Reach.  Every case names the form it is there for (`tn/general/3d/S9/last5`, `ln<4>/partial/reduce<16>/once`); the test first
derives the form from the Python restatement of linear_bwd_chunks, tn_grid and the LayerNorm / reduce dispatch below and fails
if the shape no longer selects it.  tests/test_train_blocks_grid_cpu.py ties the restatement to the compiled rule (through
rrt_linear_backward_workspace_size) and the case lists to the instantiations the two files compile.

A. rrt_linear_backward_f32.  Three input families per case:
  integer  operands in -3..3 from element indices modulo 251 / 241: every dX, dW, db entry is an integer below 2^24, so
           the comparison is np.array_equal at compute 0, 1 and 2 -- a dropped row or a misplaced chunk moves a value by >= 1.
  synth    dY, X from synth.normal, W from synth.uniform / sqrt(K) (dY, W magnitudes >= 2^-6: no rounded operand is an fp16
           subnormal) against the float64 product, for dX at compute 1 / 2 on the operands rounded as the mode sees them.
  cancel   synth, but in every row chunk of the split-K rule the second half of the rows of dY is the negated first half plus
           2^-10 noise (and X's second half repeats its first): dW and db are small sums of large terms.
  Tolerance: 4 x the error against float64 of an fp32 fma chain over the reduction in index order on 64 sample rows of the
  output (every column of each; db is one row), floored at 8 x 2^-24 x max |ref| (the rule and the sample of
  tests/test_linear_form_matrix.py).  Measured on the reference side only.
B. rrt_layernorm_backward_f32: plain, with `add`, and with dy in region-major padded order (pad slots hold 1e30 and must
  never be read); input families mild / offset (row mean 100) / flat (constant rows, rows with deviations of 2^-12: eps
  dominates rstd) / outlier (one entry 1e4).  dx per row relative to the row's largest reference entry and per tensor, dgamma,
  dbeta per tensor.
C. the activation passes, partition_rows, the drop mask and the batched transpose through the rrt_debug_* stage entries; the
  mask reference is hip_util.dropout_keep.  Whatever is one IEEE operation per element is compared bit for bit.
  Tolerance of B and the GELU passes: max(2e-5 x max(1, max |ref|), 8 x e32), e32 the error of the same restatement in plain
  fp32 on the CPU on the same inputs (the rule of tests/test_crmsa_stage_matrix.py).

Outputs go into NaN-filled buffers with hip_util canary rows behind them, the workspace is exactly the size the library asks for
with canary bytes behind it (first run filled with 0xFF, second with another byte), inputs must come back unmodified, and
every case runs twice and must give the same bits.  The case lists are plain module data; importing this module needs no
device.  RRT_TRAIN_BLOCK_ERRORS_OUT=<file>: the per-form error table kept as profiles/train_block_errors.txt."""
import collections
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth
from hip_util import CANARY, CANARY_ROWS, CANARY_BYTES, CANARY_BYTE, dropout_keep

pytestmark = pytest.mark.gpu

RECORDS = []                      # (form group, e32 / chain error, measured error, tolerance)
DROP_SEED, DROP_LAYER = 0x1234567887654321, 3
DEV = "cuda:0"
STAGE_BOUND = 2e-5                # the project's per-stage bound (test_layernorm_backward), x max(1, max |ref|)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_TRAIN_BLOCK_ERRORS_OUT")      # the table kept as profiles/train_block_errors.txt
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
    """per form: cases, worst e32 (linear: chain error), worst error, worst error / tolerance (bit-exact forms: zeros)"""
    rows = collections.OrderedDict()
    for form, e32, err, tol in records:
        n, a, b, r = rows.get(form, (0, 0.0, 0.0, 0.0))
        rows[form] = (n + 1, max(a, e32), max(b, err), max(r, err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))))
    lines = [f"{'form':52s} {'cases':>6s} {'worst e32':>10s} {'worst err':>10s} {'worst ratio':>12s}"]
    for form, (n, a, b, r) in rows.items():
        lines.append(f"{form:52s} {n:6d} {a:10.2e} {b:10.2e} {r:12.3f}")
    return "\n".join(lines) + "\n"


def record(form, e32, err, tol):
    RECORDS.append((form, float(e32), float(err), float(tol)))
    print(f"{form}: e32 {e32:.3e} err {err:.3e} tol {tol:.3e}")


# ------------------------------------------------------------------ the dispatch rules, restated
TN_BN = TN_BK = 128
TN_BM = 32
TN_TARGET = 768                   # blocks the split-K rule aims at (csrc/linear_bwd.hip linear_bwd_chunks)
LNB_BLOCKS = 512
PARTITION_BLOCKS = 4096


def align256(v):
    return (v + 255) // 256 * 256


def linear_bwd_chunks(M, N, K):
    """(S, rows_per_chunk) of csrc/linear_bwd.hip::linear_bwd_chunks"""
    tiles = -(-N // TN_BN) * -(-K // TN_BK)
    S = -(-TN_TARGET // tiles)
    S = max(1, min(S, -(-M // (4 * TN_BM))))
    rpc = -(-M // S)
    rpc = -(-rpc // TN_BM) * TN_BM
    return -(-M // rpc), rpc


def linear_bwd_workspace(M, N, K):
    S, _ = linear_bwd_chunks(M, N, K)
    return align256(4 * N * K) + align256(4 * S * N * K) + align256(4 * (-(-M // 128)) * N)


def tn_cell(M, N, K):
    """(FAST, grid) with grid = direct (S == 1: dW / db written by the product itself), 3d, xcd (tn_grid: S % 8 == 0)"""
    S, _ = linear_bwd_chunks(M, N, K)
    return N % TN_BN == 0 and K % TN_BK == 0, "direct" if S == 1 else "xcd" if S % 8 == 0 else "3d"


def last_chunk(M, N, K):
    S, rpc = linear_bwd_chunks(M, N, K)
    return M - (S - 1) * rpc


def reduce_waves(S, n):
    """NWV of launch_reduce_partials"""
    return 16 if S >= 64 and -(-n // 256) <= 64 else 4


def tn_form(M, N, K):
    fast, grid = tn_cell(M, N, K)
    S, _ = linear_bwd_chunks(M, N, K)
    return f"tn/{'fast' if fast else 'general'}/{grid}/S{S}/last{last_chunk(M, N, K)}"


def colsum_form(M, N):
    SB = -(-M // 128)
    tail = (M - 128 * (SB - 1)) % 4
    return f"colsum/{'direct' if SB == 1 else 'reduce'}/SB{SB}/tail{tail}"


def lin_form(M, N, K, outs):
    if "W" in outs:
        return tn_form(M, N, K)
    if "b" in outs:
        return colsum_form(M, N)
    return f"dx/transpose{'-ragged' if N % 32 or K % 32 else ''}"


def ln_nv(dim):
    return 1 if dim <= 256 else 2 if dim <= 512 else 4 if dim <= 1024 else 8


def ln_blocks(L):
    return min((L + 3) // 4, LNB_BLOCKS)


def ln_form(L, dim):
    nv, blocks = ln_nv(dim), ln_blocks(L)
    lanes = "full" if dim == nv * 256 else "partial"
    rows = "short" if L < 4 else "stride" if L > 4 * blocks else "once"
    return f"ln<{nv}>/{lanes}/reduce<{reduce_waves(blocks, 2 * dim)}>/{rows}"


# ------------------------------------------------------------------ A. the case list of rrt_linear_backward_f32
LinCase = collections.namedtuple("LinCase", "M N K outs form")        # outs: subset of "XWb" (dX, dW, db)

# (M, N, K) -> the form the shape is there for; lin_cases() re-derives every figure from the restatement
TN_SHAPES = [
    ((127, 128, 128), "tn/fast/direct/S1/last127"),
    ((128, 128, 128), "tn/fast/direct/S1/last128"),
    ((77, 32, 40), "tn/general/direct/S1/last77"),
    ((129, 128, 128), "tn/fast/3d/S2/last33"),
    ((1025, 128, 128), "tn/fast/3d/S9/last1"),
    ((1056, 128, 128), "tn/fast/3d/S9/last32"),
    ((2052, 128, 128), "tn/fast/3d/S17/last4"),
    ((1024, 128, 128), "tn/fast/xcd/S8/last128"),
    ((1000, 128, 256), "tn/fast/xcd/S8/last104"),             # tiles_k = 2
    ((2048, 384, 256), "tn/fast/xcd/S16/last128"),            # tiles_n = 3, two rounds of XCDs
    ((900, 8, 128), "tn/general/xcd/S8/last4"),               # N < 128
    ((1029, 129, 258), "tn/general/3d/S9/last5"),             # N, K one / two past a tile, neither a multiple of 4
    ((1030, 126, 66), "tn/general/3d/S9/last6"),              # N, K no multiples of 4, one tile each way
]
ALL_COMBOS = ("X", "W", "b", "XW", "Xb", "Wb", "XWb")
COMBO_SHAPES = ((77, 32, 40), (129, 128, 128))                # S == 1 and S > 1: every non-empty (dX, dW, db)


def lin_cases():
    out = []
    for (M, N, K), form in TN_SHAPES:
        assert tn_form(M, N, K) == form, (M, N, K, tn_form(M, N, K))
        combos = ALL_COMBOS if (M, N, K) in COMBO_SHAPES else ("XWb" if N % 32 == 0 else "Wb",)
        for outs in combos:
            out.append(LinCase(M, N, K, outs, lin_form(M, N, K, outs)))
    # dW alone at N = crmsa_k <= 8: how api.hip computes the phi-MLP gradients (launch_gemm_tn, the reduce of its own)
    out.append(LinCase(2049, 5, 128, "W", "tn/general/3d/S17/last1"))
    # db alone: colsum_kernel, SB == 1 direct / SB == 2 through the reduce, the 4-row loop's tail of 0 .. 3 rows
    for M in (1, 127, 128, 129, 130, 131):
        for N in (32, 257):
            out.append(LinCase(M, N, 64, "b", colsum_form(M, N)))
    # dX alone with K no multiple of 4: the transpose's ragged tiles, the GEMM's scalar store tail
    out.append(LinCase(77, 32, 30, "X", "dx/transpose-ragged"))
    out.append(LinCase(131, 96, 130, "X", "dx/transpose-ragged"))
    for c in out:
        assert lin_form(c.M, c.N, c.K, c.outs) == c.form, c
    return out


LIN_CASES = lin_cases()


def lin_id(c):
    return f"{c.M}x{c.N}x{c.K}-{c.outs}"


def lin_runs(c):
    """(family, compute) pairs of a case: compute only matters to dX"""
    modes = (0, 1, 2) if "X" in c.outs else (0,)
    return [("integer", m) for m in modes] + [("synth", m) for m in modes] + [("cancel", 0)]


def _ints(shape, prime, shift=0):
    """integers in -3 .. 3 from the element index modulo two primes above the largest tile dimension"""
    x = np.arange(int(np.prod(shape)), dtype=np.int64) + shift
    other = 241 if prime == 251 else 251
    a, b = x % prime, x % other
    ta, tb = (a * a * a * 5 + a * 11) % prime, (b * b * b * 3 + b * 7) % other
    return (((ta + tb) % 7) - 3).astype(np.float32).reshape(shape)


def _clamped(a):
    """magnitudes >= 2^-6, signs kept"""
    return np.where(a < 0, np.minimum(a, -2.0 ** -6), np.maximum(a, 2.0 ** -6)).astype(np.float32)


@functools.lru_cache(maxsize=6)
def lin_inputs(family, M, N, K):
    """dY [M, N], X [M, K], W [N, K]"""
    if family == "integer":
        return _ints((M, N), 251), _ints((M, K), 241), _ints((N, K), 251, shift=17)
    dY = _clamped(synth.normal(f"tbm/dy{M}x{N}", (M, N)))
    X = synth.normal(f"tbm/x{M}x{K}", (M, K))
    W = (_clamped(synth.uniform(f"tbm/w{N}x{K}", (N, K), -1, 1)) / np.float32(np.sqrt(K))).astype(np.float32)
    if family == "cancel":
        noise = synth.normal(f"tbm/nz{M}x{N}", (M, N)) * np.float32(2.0 ** -10)
        S, rpc = linear_bwd_chunks(M, N, K)
        for s in range(S):
            b, e = s * rpc, min(M, (s + 1) * rpc)
            h = (e - b) // 2
            dY[b + h:b + 2 * h] = -dY[b:b + h] + noise[b:b + h]
            X[b + h:b + 2 * h] = X[b:b + h]
            if (e - b) % 2:                   # a chunk of odd length: its last row has no partner and is noise alone
                dY[e - 1] = noise[e - 1]
    return dY, X, W


def seen(a, compute):
    """an operand of the dX product as the mode's MFMA sees it (float64)"""
    return O.round_lowp(a, "bf16" if compute == 1 else "f16") if compute in (1, 2) else a.astype(np.float64)


def _samples(size):
    """64 rows of an output (first, last, evenly spaced), every column of each: the sample of tests/test_linear_form_matrix.py"""
    return np.unique(np.linspace(0, size - 1, 64).astype(np.int64))


def _chain32(a, b):
    """fp32 fma chain over R in index order, a [R, p] x b [R, q] -> [p, q]: acc = float32(float64(acc) + a * b)"""
    acc = np.zeros((a.shape[1], b.shape[1]), np.float32)
    for r in range(a.shape[0]):
        acc = (acc.astype(np.float64) + a[r][:, None] * b[r][None, :]).astype(np.float32)
    return acc


def lin_reference(c, family, compute):
    """float64 outputs {name: array} and, for the synth families, {name: (chain error, tolerance)}"""
    dY, X, W = lin_inputs(family, c.M, c.N, c.K)
    dY64 = dY.astype(np.float64)
    ref, tol = {}, {}
    if "X" in c.outs:
        ref["dX"] = seen(dY, compute) @ seen(W, compute)
    if "W" in c.outs:
        ref["dW"] = dY64.T @ X.astype(np.float64)
    if "b" in c.outs:
        ref["db"] = dY64.sum(0)
    if family == "integer":
        return ref, None
    for name, r in ref.items():
        if name == "dX":                      # reduction over N, 64 rows m
            rows = _samples(c.M)
            got, want = _chain32(seen(dY, compute)[rows].T, seen(W, compute)), r[rows]
        elif name == "dW":                    # reduction over the M rows, 64 rows n
            rows = _samples(c.N)
            got, want = _chain32(dY64[:, rows], X.astype(np.float64)), r[rows]
        else:                                 # db is one row
            got, want = _chain32(np.ones((c.M, 1)), dY64), r[None, :]
        chain = float(np.abs(got.astype(np.float64) - want).max())
        tol[name] = (chain, max(4.0 * chain, 8.0 * 2.0 ** -24 * float(np.abs(r).max())))
    return ref, tol


def lin_reference32(c, family, compute):
    """numpy's fp32 evaluation of the same products (the CPU module holds it to the tolerance)"""
    dY, X, W = lin_inputs(family, c.M, c.N, c.K)
    out = {}
    if "X" in c.outs:
        out["dX"] = seen(dY, compute).astype(np.float32) @ seen(W, compute).astype(np.float32)
    if "W" in c.outs:
        out["dW"] = dY.T @ X
    if "b" in c.outs:
        out["db"] = dY.sum(0, dtype=np.float32)
    return out


# ------------------------------------------------------------------ the device side
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(rows, cols, fill=None):
    """a NaN-filled (or `fill`ed) [rows, cols] head of a buffer whose last CANARY_ROWS rows hold CANARY"""
    buf = torch.full((rows + CANARY_ROWS, cols), float("nan"), device=DEV)
    if fill is not None:
        buf[:rows] = dev(fill).reshape(rows, cols)
    buf[rows:] = CANARY
    return buf


def intact(buf, rows):
    return bool((buf[rows:] == CANARY).all())


def workspace(need, fill):
    ws = torch.full((need + CANARY_BYTES,), fill, dtype=torch.uint8, device=DEV)
    ws[need:] = CANARY_BYTE
    return ws


def run_linear(c, family, compute, fill=0xFF):
    """rrt_linear_backward_f32 on the case -> ({name: numpy}, list of violated guards)"""
    lib = _lib.load()
    dY, X, W = lin_inputs(family, c.M, c.N, c.K)
    ins = {"dY": dev(dY), "X": dev(X) if "W" in c.outs else None, "W": dev(W) if "X" in c.outs else None}
    keep = {k: None if v is None else v.clone() for k, v in ins.items()}
    outs = {"dX": guarded(c.M, c.K) if "X" in c.outs else None, "dW": guarded(c.N, c.K) if "W" in c.outs else None,
            "db": guarded(c.N, 1) if "b" in c.outs else None}
    rows = {"dX": c.M, "dW": c.N, "db": c.N}
    need = C.c_size_t()
    _lib.check(lib.rrt_linear_backward_workspace_size(c.M, c.N, c.K, C.byref(need)), "linear backward ws")
    ws = workspace(need.value, fill)
    _lib.check(lib.rrt_linear_backward_f32(ptr(ins["dY"]), ptr(ins["X"]), ptr(ins["W"]), ptr(outs["dX"]), ptr(outs["dW"]),
                                           ptr(outs["db"]), c.M, c.N, c.K, compute, ptr(ws), need.value, stream()),
               "rrt_linear_backward_f32")
    torch.cuda.synchronize()
    bad, got = [], {}
    for name, buf in outs.items():
        if buf is None:
            continue
        if torch.isnan(buf[:rows[name]]).any():
            bad.append(f"NaN left in {name}")
        if not intact(buf, rows[name]):
            bad.append(f"canary rows behind {name}")
        got[name] = buf[:rows[name]].cpu().numpy().reshape((c.N,) if name == "db" else (rows[name], c.K))
    if not bool((ws[need.value:] == CANARY_BYTE).all()):
        bad.append("canary bytes behind the workspace")
    for k, v in ins.items():
        if v is not None and not torch.equal(v, keep[k]):
            bad.append(f"input {k} modified")
    return got, bad


@pytest.mark.parametrize("c", LIN_CASES, ids=lin_id)
def test_linear_backward_form(c):
    assert lin_form(c.M, c.N, c.K, c.outs) == c.form, "the shape no longer selects the form this case is for"
    group = c.form.rsplit("/last", 1)[0] if c.form.startswith("tn/") else c.form.rsplit("/tail", 1)[0]
    for family, compute in lin_runs(c):
        ref, tol = lin_reference(c, family, compute)
        got, bad = run_linear(c, family, compute, 0xFF)
        again, bad2 = run_linear(c, family, compute, 0x3C)
        assert not bad and not bad2, (family, compute, bad, bad2)
        for name, r in ref.items():
            g = got[name]
            assert np.array_equal(g, again[name]), f"{family} c{compute} {name}: two runs differ"
            if family == "integer":
                assert np.abs(r).max() < 2 ** 24
                wrong = int((g != r).sum())
                record(f"{group} {name} integer", 0.0, float(np.abs(g - r).max()), 0.0)
                assert wrong == 0, f"integer c{compute} {name}: {wrong} of {g.size} differ, first at {np.argwhere(g != r)[:3].tolist()}"
                continue
            chain, t = tol[name]
            err = float(np.abs(g.astype(np.float64) - r).max())
            record(f"{group} {name} {family}{' c%d' % compute if name == 'dX' and compute else ''}", chain, err, t)
            assert err <= t, f"{family} c{compute} {name}: max-abs {err:.3e} > {t:.3e} (chain {chain:.3e})"
            if name == "dX" and compute:                    # the mode really ran: off the exact product
                dY, X, W = lin_inputs(family, c.M, c.N, c.K)
                assert np.abs(g - dY.astype(np.float64) @ W.astype(np.float64)).max() > t, "reduced precision: the exact product"


# ------------------------------------------------------------------ B. rrt_layernorm_backward_f32
LN_SHAPES = {                       # dim -> three L: every L of the list below with two dims or more
    4: (1, 5, 2049), 64: (3, 256, 2047), 256: (4, 255, 2049), 260: (1, 257, 2047), 512: (3, 252, 256),
    516: (5, 255, 257), 768: (4, 252, 2047), 1024: (1, 5, 256), 1028: (3, 257, 2049), 2048: (4, 255, 252),
}
LN_LS = (1, 3, 4, 5, 252, 255, 256, 257, 2047, 2049)          # 252 / 255: 63 / 64 partials, either side of reduce<16>
LN_FAMILIES = ("mild", "offset", "flat", "outlier")
LN_MODES = ("plain", "add", "map4", "map8+add")
LnCase = collections.namedtuple("LnCase", "L dim family form")
LN_CASES = [LnCase(L, dim, fam, ln_form(L, dim)) for dim, Ls in LN_SHAPES.items() for L in Ls for fam in LN_FAMILIES]


def ln_id(c):
    return f"L{c.L}xD{c.dim}-{c.family}"


@functools.lru_cache(maxsize=2)
def ln_inputs(family, L, D):
    """x, dy, add [L, D], gamma [D]"""
    dy = synth.normal(f"tbm/ln/dy{L}x{D}", (L, D))
    add = synth.normal(f"tbm/ln/add{L}x{D}", (L, D))
    gamma = (1.0 + synth.uniform(f"tbm/ln/g{D}", (D,), -0.25, 0.25)).astype(np.float32)
    z = synth.normal(f"tbm/ln/x{L}x{D}", (L, D))
    if family == "mild":
        x = z * np.float32(1.7) + np.float32(0.3)
    elif family == "offset":
        x = z + np.float32(100.0)
    elif family == "flat":                  # even rows constant, odd rows constant +- 2^-12
        x = np.repeat(synth.normal(f"tbm/ln/c{L}", (L, 1)), D, axis=1)
        sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0).astype(np.float32)
        x[1::2] += sign * np.float32(2.0 ** -12)
    else:
        x = z.copy()
        x[np.arange(L), (7 * np.arange(L) + 3) % D] = 1e4
    return x.astype(np.float32), dy, add, gamma


def _ln_bwd(dy, x, gamma, dt):
    """_ln_bwd64 of tests/test_hip_parity.py in the precision `dt`"""
    dy, x, gamma, eps = dy.astype(dt), x.astype(dt), gamma.astype(dt), dt(1e-5)
    mu = x.mean(-1, keepdims=True, dtype=dt)
    rstd = dt(1.0) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True, dtype=dt) + eps)
    xh = (x - mu) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdims=True, dtype=dt) - xh * (g * xh).mean(-1, keepdims=True, dtype=dt))
    return dx, (dy * xh).sum(0, dtype=dt), dy.sum(0, dtype=dt)


def _ln_bwd64(dy, x, gamma):
    return _ln_bwd(dy, x, gamma, np.float64)


@functools.lru_cache(maxsize=2)
def ln_reference(family, L, D):
    """float64 (dx, dgamma, dbeta) and the fp32 evaluation of the same lines"""
    x, dy, add, gamma = ln_inputs(family, L, D)
    return _ln_bwd64(dy, x, gamma), _ln_bwd(dy, x, gamma, np.float32)


def row_rel(err, ref):
    """per row: max |err| relative to max(1, the row's largest reference entry)"""
    return np.abs(err).max(-1) / np.maximum(1.0, np.abs(ref).max(-1))


def ln_bounds(family, L, D, with_add):
    """reference outputs and {quantity: (e32, tolerance)}; dx also per row (relative)"""
    (dx64, dg64, db64), (dx32, dg32, db32) = ln_reference(family, L, D)
    x, dy, add, gamma = ln_inputs(family, L, D)
    if with_add:
        dx64, dx32 = dx64 + add, dx32 + add
    ref = {"dx": dx64, "dgamma": dg64, "dbeta": db64}
    b = {}
    for name, r, r32 in (("dx", dx64, dx32), ("dgamma", dg64, dg32), ("dbeta", db64, db32)):
        e32 = float(np.abs(r32.astype(np.float64) - r).max())
        b[name] = (e32, max(STAGE_BOUND * max(1.0, float(np.abs(r).max())), 8.0 * e32))
    e32row = float(row_rel(dx32.astype(np.float64) - dx64, dx64).max())
    b["dx/row"] = (e32row, max(STAGE_BOUND, 8.0 * e32row))
    return ref, b


def run_ln(c, mode, fill=0xFF):
    lib = _lib.load()
    x, dy, add, gamma = ln_inputs(c.family, c.L, c.dim)
    L, D = c.L, c.dim
    g = None
    if mode.startswith("map"):
        g = _lib.region_grid(L, int(mode[3]))
        perm = O.partition_index(g.H, g.s)                  # perm[slot] = token
        dU = np.full((g.H * g.H, D), 1e30, np.float32)      # pad slots: never read
        real = perm < L
        dU[real] = dy[perm[real]]
        dy = dU
    ins = {"dy": dev(dy), "x": dev(x), "gamma": dev(gamma), "add": dev(add) if "add" in mode else None}
    keep = {k: None if v is None else v.clone() for k, v in ins.items()}
    dx, dgb = guarded(L, D), guarded(2, D)
    need = LNB_BLOCKS * 2 * D * 4                            # include/rrt_hip.h: 512 * 2 * dim floats
    ws = workspace(need, fill)
    _lib.check(lib.rrt_layernorm_backward_f32(ptr(ins["dy"]), ptr(ins["x"]), ptr(ins["gamma"]), ptr(ins["add"]), ptr(dx),
                                              ptr(dgb), L, D, C.byref(g) if g is not None else None, ptr(ws), need, stream()),
               "rrt_layernorm_backward_f32")
    torch.cuda.synchronize()
    bad = []
    if torch.isnan(dx[:L]).any() or torch.isnan(dgb[:2]).any():
        bad.append("NaN left in an output")
    if not intact(dx, L) or not intact(dgb, 2):
        bad.append("canary rows behind an output")
    if not bool((ws[need:] == CANARY_BYTE).all()):
        bad.append("canary bytes behind the workspace")
    for k, v in ins.items():
        if v is not None and not torch.equal(v, keep[k]):
            bad.append(f"input {k} modified")
    o = dgb[:2].cpu().numpy()
    return {"dx": dx[:L].cpu().numpy(), "dgamma": o[0], "dbeta": o[1]}, bad


@pytest.mark.parametrize("c", LN_CASES, ids=ln_id)
def test_layernorm_backward_form(c):
    assert ln_form(c.L, c.dim) == c.form
    assert lib_refuses_short_ln_workspace(c.dim)
    for mode in LN_MODES:
        ref, bounds = ln_bounds(c.family, c.L, c.dim, "add" in mode)
        got, bad = run_ln(c, mode, 0xFF)
        again, bad2 = run_ln(c, mode, 0x3C)
        assert not bad and not bad2, (mode, bad, bad2)
        fails = []
        for name in ("dx", "dgamma", "dbeta"):
            assert np.array_equal(got[name], again[name]), f"{mode} {name}: two runs differ"
            e32, tol = bounds[name]
            err = float(np.abs(got[name].astype(np.float64) - ref[name]).max())
            record(f"{c.form} {c.family} {name}", e32, err, tol)
            if not err <= tol:
                fails.append(f"{mode} {name}: max-abs {err:.3e} > {tol:.3e} (e32 {e32:.3e})")
        e32, tol = bounds["dx/row"]
        err = float(row_rel(got["dx"].astype(np.float64) - ref["dx"], ref["dx"]).max())
        record(f"{c.form} {c.family} dx/row", e32, err, tol)
        if not err <= tol:
            fails.append(f"{mode} dx per row: {err:.3e} > {tol:.3e} (e32 {e32:.3e})")
        assert not fails, fails


def lib_refuses_short_ln_workspace(dim):
    """one byte short is RRT_E_WORKSPACE before any launch (dummy non-null pointers, never followed)"""
    P = 0x1000
    return _lib.load().rrt_layernorm_backward_f32(P, P, P, None, P, P, 4, dim, None, P, LNB_BLOCKS * 2 * dim * 4 - 1, None) == -3


# ------------------------------------------------------------------ C. activation passes
ACT_NS = (4, 1020, 1024, 1028, 262148)
ACT_DROPS = (0.0, 0.5, 0.1)
ACT_CODE = {"gelu": _lib.ACT_GELU, "relu": _lib.ACT_RELU}
ActCase = collections.namedtuple("ActCase", "which act n p form")
ACT_CASES = [ActCase(w, a, n, p, f"act_{w}/{a}/{'drop' if p else 'plain'}")
             for w in ("forward", "backward") for a in ("gelu", "relu") for n in ACT_NS for p in ACT_DROPS]


def act_id(c):
    return f"{c.which}-{c.act}-n{c.n}-p{c.p}"


def act_grid():
    """+-0, +-2^-130, every multiple of 1/8 in [-12, 12], +-20, +-88, +-100"""
    sp = [0.0, -0.0, 2.0 ** -130, -2.0 ** -130] + [k / 8.0 for k in range(-96, 97)] + [20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
    return np.array(sp, dtype=np.float32)


@functools.lru_cache(maxsize=8)
def act_inputs(n, integer=False):
    """hpre, dh [n]: the grid first, the rest synth.normal * 3 (integer: whole numbers in -3 .. 3, zeros included)"""
    if integer:
        return _ints((n,), 251), _ints((n,), 241, shift=5)
    x = np.concatenate([act_grid(), synth.normal(f"tbm/act/x{n}", (n,)) * np.float32(3.0)])[:n].astype(np.float32)
    return x, synth.normal(f"tbm/act/dh{n}", (n,))


def _phi_terms(x, dt):
    """Phi(x) and x phi(x) in the precision dt; float64 through erfc (no cancellation in the tail)"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(torch.float64 if dt is np.float64 else torch.float32)
    if dt is np.float64:
        Phi = 0.5 * torch.erfc(-t * 0.7071067811865476)
    else:
        Phi = 0.5 * (1.0 + torch.erf(t * 0.70710678118654752))
    return Phi.numpy(), (t * 0.3989422804014327 * torch.exp(-0.5 * t * t)).numpy()


def act_value(x, act, dt):
    """act(x): x Phi(x) / max(x, 0)"""
    if act == "relu":
        return np.maximum(x.astype(dt), dt(0))
    return x.astype(dt) * _phi_terms(x, dt)[0]


def act_slope(x, act, dt):
    """act'(x): Phi(x) + x phi(x) / [x > 0] (0 at +-0)"""
    if act == "relu":
        return (x > 0).astype(dt)
    Phi, xphi = _phi_terms(x, dt)
    return (Phi + xphi).astype(dt)


def drop_scale(p):
    """make_drop's 1 / (1 - p) in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_of(n, p, rows=None):
    if not p:
        return np.ones(n if rows is None else (rows, n // rows), bool)
    k = dropout_keep(DROP_SEED, DROP_LAYER, n, 1, float(np.float32(p))).reshape(-1)      # p as the entry's float sees it
    return k if rows is None else k.reshape(rows, -1)


def act_reference(c, dt, integer=False):
    x, dh = act_inputs(c.n, integer)
    keep, sc = keep_of(c.n, c.p), dt(drop_scale(c.p) if c.p else 1.0)
    if c.which == "forward":
        v = act_value(x, c.act, dt)
        return np.where(keep, v * sc, dt(0)) if c.p else v
    g = np.where(keep, dh.astype(dt) * sc, dt(0)) if c.p else dh.astype(dt)
    return g * act_slope(x, c.act, dt)


def run_act(c, integer=False):
    lib = _lib.load()
    x, dh = act_inputs(c.n, integer)
    d_x = dev(x)
    keep = d_x.clone()
    if c.which == "forward":
        out = guarded(c.n, 1)
        _lib.check(lib.rrt_debug_act_forward_f32(ptr(d_x), ptr(out), c.n, ACT_CODE[c.act], c.p, DROP_SEED, DROP_LAYER, stream()),
                   "rrt_debug_act_forward_f32")
    else:
        out = guarded(c.n, 1, dh)                            # in place
        _lib.check(lib.rrt_debug_act_backward_f32(ptr(out), ptr(d_x), c.n, ACT_CODE[c.act], c.p, DROP_SEED, DROP_LAYER, stream()),
                   "rrt_debug_act_backward_f32")
    torch.cuda.synchronize()
    bad = []
    if torch.isnan(out[:c.n]).any():
        bad.append("NaN left in the output")
    if not intact(out, c.n):
        bad.append("canary rows behind the output")
    if not torch.equal(d_x, keep):
        bad.append("hpre modified")
    return out[:c.n].cpu().numpy().reshape(-1), bad


@pytest.mark.parametrize("c", ACT_CASES, ids=act_id)
def test_activation_pass(c):
    ref, r32 = act_reference(c, np.float64), act_reference(c, np.float32)
    got, bad = run_act(c)
    again, bad2 = run_act(c)
    assert not bad and not bad2, (bad, bad2)
    assert np.array_equal(got, again), "two runs differ"
    keep = keep_of(c.n, c.p)
    assert (got[~keep] == 0).all(), "an element the mask reference drops is not zero"
    if c.act == "relu":                                      # one IEEE operation per element: bit for bit
        record(c.form, 0.0, float(np.abs(got - r32).max()), 0.0)
        assert np.array_equal(got, r32), np.argwhere(got != r32)[:3].tolist()
        if c.which == "backward":
            assert (got[act_inputs(c.n)[0] == 0] == 0).all(), "ReLU's derivative at +-0 is 0"
    else:
        e32 = float(np.abs(r32.astype(np.float64) - ref).max())
        tol = max(STAGE_BOUND * max(1.0, float(np.abs(ref).max())), 8.0 * e32)
        err = float(np.abs(got.astype(np.float64) - ref).max())
        record(c.form, e32, err, tol)
        assert err <= tol, f"max-abs {err:.3e} > {tol:.3e} (e32 {e32:.3e})"
    if c.p == 0.5:
        # integer inputs, scale 2 (exact): the masked output is the unmasked one doubled where the mask reference keeps,
        # zero elsewhere, bit for bit; ReLU's is the reference itself
        got_i, bad = run_act(c, integer=True)
        plain_i, bad2 = run_act(c._replace(p=0.0), integer=True)
        assert not bad and not bad2, (bad, bad2)
        want = np.where(keep, plain_i * np.float32(2), np.float32(0))
        assert np.array_equal(got_i, want), np.argwhere(got_i != want)[:3].tolist()
        if c.act == "relu":
            assert np.array_equal(got_i, act_reference(c, np.float32, integer=True))


# ------------------------------------------------------------------ C. partition_rows
PART_VARIANTS = (("plain", 0.0, 1.0), ("scale0.5", 0.0, 0.5), ("scale0", 0.0, 0.0), ("drop0.5", 0.5, 1.0), ("drop0.1+scale0.5", 0.1, 0.5))
PartCase = collections.namedtuple("PartCase", "L rn dim form")


def part_form(L, rn, dim):
    g_np = _grid_np(L, rn)
    return f"partition_rows/{'stride' if (g_np + 3) // 4 > PARTITION_BLOCKS else 'once'}/{'cols-loop' if dim > 256 else 'cols-once'}"


@functools.lru_cache(maxsize=None)
def _grid_np(L, rn):
    """H * H of the default region grid (rrt_region_grid: host only)"""
    g = _lib.region_grid(L, rn)
    return g.H * g.H


PART_SHAPES = [(L, rn, dim) for L in (1, 50, 777, 4097) for rn in (4, 8) for dim in (4, 260, 512)] + [(16500, 8, 4)]


def part_cases():
    return [PartCase(L, rn, dim, part_form(L, rn, dim)) for L, rn, dim in PART_SHAPES]


def part_reference(L, rn, dim, p, scale):
    """fp32, one multiplication per element: dst [Np, dim]; the mask is indexed by padded slot * dim + column"""
    g = _lib.region_grid(L, rn)
    Np = g.H * g.H
    src = synth.normal(f"tbm/part/{L}x{dim}", (L, dim))
    perm = O.partition_index(g.H, g.s)
    dst = np.zeros((Np, dim), np.float32)
    real = perm < L
    dst[real] = src[perm[real]]
    if p or scale != 1.0:
        sc = np.float32((drop_scale(p) if p else np.float32(1.0)) * np.float32(scale))
        dst = np.where(keep_of(Np * dim, p, rows=Np), dst * sc, np.float32(0)).astype(np.float32)
    return g, src, dst


@pytest.mark.parametrize("L,rn,dim", PART_SHAPES, ids=lambda v: str(v))
def test_partition_rows(L, rn, dim):
    lib = _lib.load()
    form = part_form(L, rn, dim)
    for name, p, scale in PART_VARIANTS:
        g, src, want = part_reference(L, rn, dim, p, scale)
        Np = g.H * g.H
        outs = []
        for _ in range(2):
            d_src = guarded(L, dim, src)
            keep = d_src.clone()
            dst = guarded(Np, dim)
            _lib.check(lib.rrt_debug_partition_rows_f32(ptr(d_src), ptr(dst), dim, C.byref(g), p, DROP_SEED, DROP_LAYER, scale,
                                                        stream()), "rrt_debug_partition_rows_f32")
            torch.cuda.synchronize()
            assert not torch.isnan(dst[:Np]).any() and intact(dst, Np) and torch.equal(d_src, keep), name
            outs.append(dst[:Np].cpu().numpy())
        assert np.array_equal(outs[0], outs[1])
        record(f"{form} {'drop' if p else 'scale' if scale != 1.0 else 'plain'}", 0.0, float(np.abs(outs[0] - want).max()), 0.0)
        assert np.array_equal(outs[0], want), (name, np.argwhere(outs[0] != want)[:3].tolist())
        if p:
            assert (want == 0).sum() > (want.size - L * dim), "the mask drops something"


# ------------------------------------------------------------------ C. the drop-mask pass
MASK_NS = (1, 255, 256, 257, 100003)
MASK_VARIANTS = ((0.5, 1.0), (0.1, 1.0), (0.1, 0.5), (0.0, 0.5))


@pytest.mark.parametrize("n", MASK_NS)
@pytest.mark.parametrize("in_place", (True, False), ids=("inplace", "copy"))
def test_drop_mask(n, in_place):
    lib = _lib.load()
    src = synth.normal(f"tbm/mask/{n}", (n,))
    for p, scale in MASK_VARIANTS:
        sc = np.float32((drop_scale(p) if p else np.float32(1.0)) * np.float32(scale))
        want = np.where(keep_of(n, p), src * sc, np.float32(0)).astype(np.float32)
        outs = []
        for _ in range(2):
            d_src = guarded(n, 1, src)
            keep = d_src.clone()
            dst = d_src if in_place else guarded(n, 1)
            _lib.check(lib.rrt_debug_drop_mask_f32(ptr(d_src), ptr(dst), n, p, DROP_SEED, DROP_LAYER, scale, stream()),
                       "rrt_debug_drop_mask_f32")
            torch.cuda.synchronize()
            assert not torch.isnan(dst[:n]).any() and intact(dst, n) and (in_place or torch.equal(d_src, keep))
            outs.append(dst[:n].cpu().numpy().reshape(-1))
        assert np.array_equal(outs[0], outs[1])
        record(f"drop_mask/{'inplace' if in_place else 'copy'}", 0.0, float(np.abs(outs[0] - want).max()), 0.0)
        assert np.array_equal(outs[0], want), (p, scale, np.argwhere(outs[0] != want)[:3].tolist())
    # no dropout, scale 1: the in-place form launches nothing, the copying form copies
    d_src = guarded(n, 1, src)
    dst = d_src if in_place else guarded(n, 1)
    _lib.check(lib.rrt_debug_drop_mask_f32(ptr(d_src), ptr(dst), n, 0.0, DROP_SEED, DROP_LAYER, 1.0, stream()), "drop mask identity")
    torch.cuda.synchronize()
    assert np.array_equal(dst[:n].cpu().numpy().reshape(-1), src) and intact(dst, n)


# ------------------------------------------------------------------ C. the batched transpose
TR_SHAPES = ((1, 1), (31, 33), (32, 32), (33, 31), (1, 300), (300, 1), (96, 512))
TR_JOBS = (1, 2, _lib.TRANSPOSE_MAX_JOBS)


def tr_shapes(n_jobs):
    """the job list of a case: the shapes in turn, starting at a different one per job count"""
    return [TR_SHAPES[(j + n_jobs) % len(TR_SHAPES)] for j in range(n_jobs)]


@pytest.mark.parametrize("n_jobs", TR_JOBS)
def test_transpose_batch(n_jobs):
    lib = _lib.load()
    shapes = tr_shapes(n_jobs)
    mats = [synth.normal(f"tbm/tr/{j}/{R}x{Cc}", (R, Cc)) for j, (R, Cc) in enumerate(shapes)]
    results = []
    for _ in range(2):
        ins = [dev(m) for m in mats]
        keep = [t.clone() for t in ins]
        outs = [guarded(Cc, R) for R, Cc in shapes]          # every job's output guarded separately
        a_in = (C.c_void_p * n_jobs)(*[t.data_ptr() for t in ins])
        a_out = (C.c_void_p * n_jobs)(*[t.data_ptr() for t in outs])
        a_R = (C.c_int32 * n_jobs)(*[s[0] for s in shapes])
        a_C = (C.c_int32 * n_jobs)(*[s[1] for s in shapes])
        _lib.check(lib.rrt_debug_transpose_batch_f32(a_in, a_out, a_R, a_C, n_jobs, stream()), "rrt_debug_transpose_batch_f32")
        torch.cuda.synchronize()
        got = []
        for j, (R, Cc) in enumerate(shapes):
            assert not torch.isnan(outs[j][:Cc]).any() and intact(outs[j], Cc), f"job {j}"
            assert torch.equal(ins[j], keep[j]), f"job {j}: input modified"
            got.append(outs[j][:Cc].cpu().numpy())
        results.append(got)
    for j, m in enumerate(mats):
        assert np.array_equal(results[0][j], results[1][j])
        record(f"transpose_batch/jobs{n_jobs}", 0.0, float(np.abs(results[0][j] - m.T).max()), 0.0)
        assert np.array_equal(results[0][j], m.T), f"job {j} {shapes[j]}"
