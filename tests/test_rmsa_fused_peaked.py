"""GPU (-m gpu): the fused R-MSA kernels -- rmsa_fused_kernel (fp32, and bf16 / fp16 matrix-core operands), its merged-
projection form, rmsa_fused16, rmsa_pair16, rmsa_fused_x3 -- on softmax rows that are not nearly flat, through their C-ABI
entries, against the float64 restatement of tests/rmsa_fused_cases.py.

The inputs (rmsa_fused_cases.inputs) carry a largest |score| of about 50 and, per variant: nothing else (plain), the row
maximum in each key tile in turn (runmax: a record that is dropped, stale or mis-indexed in the nine-way merge of
rmsa_fused_kernel<9, ..> or in a row-max reduction moves O by whole units; a maximum that is merely too small does not show
in fp32 or bf16, where exp2(72) is representable, and turns the fp16 probabilities into infinities), a dominant single valid key of the last tile next to
15 masked ones with very large rows behind the region (masked), equal keys (ties_k) and equal scores (ties_q: a wrong
divisor shows at once).  The cases are the smallest shapes that still select each kernel form;
tests/test_rmsa_fused_peaked_cpu.py checks on the CPU that they cover every form and are as peaked as claimed.

Bounds.  e32 = the max-abs difference between the restatement carried in fp32 and in float64 on the same inputs, measured
here on the reference side only.
  fp32 kernel            max-abs <= max(5e-5, 8 e32); fp16 operands: max(5e-4, 8 e32) (the floors of test_rmsa_fused)
  16-bit kernels         element-wise |err| <= 1.01 ulp |ref| + max(4e-3 ulp 256 max|ref|, 8 e32), ulp = half a 16-bit ulp (the
                         final rounding of O, and test_rmsa_fused16's slack for rounding-boundary flips, which may grow with
                         what fp32-against-float64 carrying does to the same rounding points on these inputs);
                         mean |err| <= 0.6 ulp mean|ref| + max(1e-6, 8 mean e32).  fp16: + e_flush, the distance between
                         the restatement with fp16-subnormal probabilities kept and with them flushed to zero.
  split kernel           against its own restatement max(4e-5, 8 e32); against exact arithmetic max(1e-4, 8 x the float64
                         split restatement's own distance from the exact float64 result)
  projection bags        O and x1 bit for bit against the two launches; x1 against float64 max(1e-4, 8 e32)
Every call writes into a NaN-filled (0x7FC0-filled) output with canary rows behind it, runs twice to the same bits, leaves
its inputs unmodified and leaves rrt_device_error at 0.  Importing this module needs no device."""
import collections
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rmsa_fused_cases as F
from rrt_mil_amd import _lib
from test_hip_parity import _from16, _from_split, _split_image, _to16

pytestmark = pytest.mark.gpu

E32_FACTOR = 8.0
CANARY_ROWS, CANARY, CANARY16 = 64, -777.25, 0x5A5A
Record = collections.namedtuple("Record", "form variant quantity e32 err bound e_flush nearer")
RECORDS = []


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_FUSED_PEAKED_ERRORS_OUT")     # the table kept as profiles/rmsa_fused_peaked_errors.txt
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
    """one line per (kernel form, variant, quantity): cases, worst e32, worst error, worst error / bound; fp16: the worst
    e_flush and which restatement the kernel is nearer to"""
    rows = collections.OrderedDict()
    for r in records:
        n, w32, werr, wr, wfl, near = rows.get(r[:3], (0, 0.0, 0.0, 0.0, None, set()))
        wfl = wfl if r.e_flush is None else max(wfl or 0.0, r.e_flush)
        rows[r[:3]] = (n + 1, max(w32, r.e32), max(werr, r.err), max(wr, r.err / r.bound), wfl, near | ({r.nearer} - {None}))
    lines = [f"{'kernel form':34s} {'variant':8s} {'quantity':18s} {'cases':>5s} {'worst e32':>10s} {'worst err':>10s} "
             f"{'err/bound':>9s} {'e_flush':>10s} nearer to"]
    for (form, variant, what), (n, w32, werr, wr, wfl, near) in sorted(rows.items()):
        fl = f"{'-':>10s}" if wfl is None else f"{wfl:10.2e}"
        lines.append(f"{form:34s} {variant:8s} {what:18s} {n:5d} {w32:10.2e} {werr:10.2e} {wr:9.3f} {fl} "
                     f"{'/'.join(sorted(near)) or '-'}")
    return "\n".join(lines) + "\n"


def form_of(c):
    prec = {0: "", 1: " bf16", 2: " f16"}[c.compute]
    mt = F.mt_of(c.kernel, c.P)
    if c.kernel == "pair16":
        return f"pair16{prec} MT{mt} w{F.pair_waves(c.P)} s{F.stencil_geo(16 * mt, c.ek)[1] if c.ek else 0}"
    return f"{c.kernel}{prec} MT{mt}" + (" split-last" if F.split_last(c.kernel, c.P) else "")


# ------------------------------------------------------------------ guarded launches
def _out32(rows, cols):
    buf = torch.full((rows + CANARY_ROWS, cols), float("nan"), device="cuda:0")
    buf[rows:] = CANARY
    return buf


def _out16(rows, cols):
    buf = torch.full((rows + CANARY_ROWS, cols), 0x7FC0, dtype=torch.int16, device="cuda:0")
    buf[rows:] = CANARY16
    return buf


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _twice(launch, make_outs, rows, operands):
    """launch(*outs) twice into fresh guarded outputs: the same bits, canaries intact, operands unmodified, no device error
    -> the outputs of the second run (without the canary rows)"""
    lib = _lib.load()
    before = [t.clone() for t in operands]
    runs = []
    for _ in range(2):
        outs = make_outs()
        launch(*outs)
        torch.cuda.synchronize()
        assert lib.rrt_device_error(0) == 0
        for o, n in zip(outs, rows):
            tail = o[n:]
            assert bool((tail == (CANARY if o.dtype == torch.float32 else CANARY16)).all()), "rows behind the output were written"
        runs.append(outs)
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), "two runs of the same call differ"
    for t, t0 in zip(operands, before):
        assert torch.equal(_bits(t), _bits(t0)), "an operand was modified"
    return [o[:n] for o, n in zip(runs[1], rows)]


def _copies(i):
    """the cached inputs are read-only: torch gets writable copies"""
    return F.Inputs(*(np.array(a) for a in i))


def run_kernel(c, i):
    """the case's C-ABI entry on its inputs -> O [R P, D] as float64 numpy"""
    from hip_util import dev, p, stream
    i = _copies(i)
    lib = _lib.load()
    R, P, D, heads, ek = c.R, c.P, c.D, c.heads, c.ek
    d_b, d_pe = dev(i.b), dev(i.taps)
    pe = lambda: p(d_pe) if ek else None
    if c.kernel == "fused_f32":
        d_u, d_W = dev(i.u), dev(i.W)
        o, = _twice(lambda o: _lib.check(lib.rrt_rmsa_fused_f32(p(d_u), p(d_W), p(d_b), pe(), p(o), R, P, D, heads, ek,
                                                                c.compute, stream()), "rmsa_fused"),
                    lambda: [_out32(R * P, D)], [R * P], [d_u, d_W, d_b, d_pe])
        return o.double().cpu().numpy()
    if c.kernel in ("fused16", "pair16"):
        u16, w16 = _to16(i.u, c.compute)[0], _to16(i.W, c.compute)[0]
        # the one-region kernel: P > 176, or the call cut into pieces of fewer than 8 regions
        step = R if (c.kernel == "pair16" or P > 176) else 7
        assert F.takes_pair(min(R, step), P, ek) == (c.kernel == "pair16")

        def launch(o):
            for r0 in range(0, R, step):
                n = min(step, R - r0)
                _lib.check(lib.rrt_rmsa_fused16(p(u16[r0 * P:]), p(w16), p(d_b), pe(), p(o[r0 * P:]), n, P, D, heads, ek,
                                                c.compute, stream()), "rmsa_fused16")
        o, = _twice(launch, lambda: [_out16(R * P, D)], [R * P], [u16, w16, d_b, d_pe])
        return _from16(o, c.compute)
    assert c.kernel == "x3"
    ui, wi = _split_image(i.u).to("cuda:0"), _split_image(i.W).to("cuda:0")
    o, = _twice(lambda o: _lib.check(lib.rrt_rmsa_fused_x3(p(ui), p(wi), p(d_b), pe(), p(o), R, P, D, heads, ek, stream()),
                                     "fused_x3"),
                lambda: [_out16(R * P, 2 * D)], [R * P], [ui, wi, d_b, d_pe])
    return _from_split(o.reshape(-1), (R * P, D))


# ------------------------------------------------------------------ the checks
def _maxerr(a, b):
    return float(np.abs(a - b).max())


def _record(c, what, e32, err, bound, e_flush=None, nearer=None):
    RECORDS.append(Record(form_of(c), c.variant, what, e32, err, bound, e_flush, nearer))
    extra = "" if e_flush is None else f"  e_flush {e_flush:.3e} nearer to {nearer}"
    print(f"{F.case_id(c)} {what}: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}{extra}")
    return None if err <= bound else f"{what}: {err:.3e} > {bound:.3e}"


def _same_rows_per_tile(c, o):
    """ties_k: every probability is exp2(0) and every value row the same bits, so the rows of O of one (region, head)
    within one 16-row tile are the same bits (the ninth tile of rmsa_fused_kernel<9, ..> is merged in another order)"""
    rows = o.reshape(c.R, c.P, c.D)
    for t0 in range(0, c.P, 16):
        tile = rows[:, t0:t0 + 16]
        assert np.array_equal(tile, np.broadcast_to(tile[:, :1], tile.shape)), f"rows of O differ within row tile {t0 // 16}"


CORE_CASES = [c for c in F.CASES if c.kernel != "fused_proj"]
PROJ_CASES = [c for c in F.CASES if c.kernel == "fused_proj"]


@pytest.mark.parametrize("c", CORE_CASES, ids=[F.case_id(c) for c in CORE_CASES])
def test_fused_peaked(c):
    i = F.inputs(c)
    ref, _ = F.reference(c)
    ref32, _ = F.reference(c, torch.float32)
    e32 = _maxerr(ref32, ref)
    got = run_kernel(c, i)
    assert np.isfinite(got).all(), "an element of O was left unwritten or is not finite"
    err = np.abs(got - ref)
    failures = []
    if c.kernel == "fused_f32":
        floor = 5e-4 if c.compute == 2 else 5e-5
        failures.append(_record(c, "O", e32, float(err.max()), max(floor, E32_FACTOR * e32)))
    elif c.kernel == "x3":
        failures.append(_record(c, "O vs restatement", e32, float(err.max()), max(4e-5, E32_FACTOR * e32)))
        exact, _ = F.reference(c, exact=True)
        failures.append(_record(c, "O vs exact", e32, _maxerr(got, exact), max(1e-4, E32_FACTOR * _maxerr(ref, exact))))
    else:
        ulp = 2.0 ** (-8 if c.compute == 1 else -11)               # half a 16-bit ulp, relative
        e_flush = mean_flush = nearer = None
        if c.compute == 2:
            flushed, _ = F.reference(c, flush=True)
            e_flush, mean_flush = _maxerr(flushed, ref), float(np.abs(flushed - ref).mean())
            ef = _maxerr(got, flushed)
            nearer = "same" if e_flush == 0 else "kept" if float(err.max()) <= ef else "flushed"
            print(f"{F.case_id(c)}: max-abs against the restatement with fp16-subnormal probabilities kept {err.max():.3e}, "
                  f"flushed {ef:.3e}")
        bound = 1.01 * ulp * np.abs(ref) + max(4e-3 * ulp * 256 * np.abs(ref).max(), E32_FACTOR * e32) + (e_flush or 0.0)
        worst = int(np.argmax(err / bound))
        failures.append(_record(c, "O", e32, float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]), e_flush, nearer))
        mean32 = float(np.abs(ref32 - ref).mean())
        failures.append(_record(c, "mean |err| of O", mean32, float(err.mean()),
                                0.6 * ulp * float(np.abs(ref).mean()) + max(1e-6, E32_FACTOR * mean32) + (mean_flush or 0.0)))
    failures = [f for f in failures if f]
    assert not failures, "; ".join(failures)
    if c.variant == "ties_k":
        _same_rows_per_tile(c, got)


@pytest.mark.parametrize("c", PROJ_CASES, ids=[F.case_id(c) for c in PROJ_CASES])
def test_fused_proj_peaked(c):
    """the merged launch on a bag whose regions carry the planted maxima: O and x1 bit for bit against the two launches it
    replaces, x1 against float64"""
    from hip_util import dev, p, stream
    lib = _lib.load()
    i = _copies(F.inputs(c))
    Wp, bp, res, H, s = F.proj_inputs(c)
    g = _lib.region_grid(c.L, 8)
    Np, R, P, D, heads, ek, L = g.H * g.H, c.R, c.P, c.D, c.heads, c.ek, c.L
    assert (g.H, g.s) == (H, s) and Np == R * P
    d_u, d_W, d_b, d_pe, d_Wp, d_bp, d_res = dev(i.u), dev(i.W), dev(i.b), dev(i.taps), dev(Wp), dev(bp), dev(res)
    ops = [d_u, d_W, d_b, d_pe, d_Wp, d_bp, d_res]

    def two(o, x1):
        _lib.check(lib.rrt_rmsa_fused_f32(p(d_u), p(d_W), p(d_b), p(d_pe), p(o), R, P, D, heads, ek, 0, stream()), "rmsa_fused")
        _lib.check(lib.rrt_linear_unpartition_residual_f32(p(o), p(d_Wp), p(d_bp), p(d_res), p(x1), D, D, C.byref(g), 0,
                                                           stream()), "unpart")
    cnt = torch.full((R,), 12345, device="cuda:0", dtype=torch.int32)

    def merged(o, x1):
        _lib.check(lib.rrt_rmsa_fused_proj_f32(p(d_u), p(d_W), p(d_b), p(d_pe), p(d_Wp), p(d_bp), p(d_res), p(x1), p(o),
                                               p(cnt), D, heads, ek, C.byref(g), stream()), "rmsa_fused_proj")
    outs = lambda: [_out32(Np, D), _out32(L, D)]
    o1, x1 = _twice(two, outs, [Np, L], ops)
    o2, x2 = _twice(merged, outs, [Np, L], ops)
    assert torch.equal(_bits(o1), _bits(o2)), "attention output differs from the two-launch path"
    assert torch.equal(_bits(x1), _bits(x2)), "projection differs from the two-launch path"
    ref, ref32 = F.proj_reference(c, torch.float64), F.proj_reference(c, torch.float32)
    e32 = _maxerr(ref32, ref)
    got = x2.double().cpu().numpy()
    assert np.isfinite(got).all()
    fail = _record(c, "x1", e32, _maxerr(got, ref), max(1e-4, E32_FACTOR * e32))
    assert not fail, fail
