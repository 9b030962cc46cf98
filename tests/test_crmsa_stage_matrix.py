"""GPU (-m gpu): every CR-MSA kernel against a float64 restatement of rmsa.py:303-335, never against another kernel.

A. the front -- LayerNorm-2 statistics, logits, combine (softmax over the tokens of a region, pads in the sum but not in the
   contraction), dispatch weights (softmax over the representatives x the min/max normaliser), dispatch + residual + LN --
   in every form the library has: `two` (rrt_crmsa_logits_f32 + rrt_crmsa_combine_f32), `one` (rrt_crmsa_region_f32),
   `four` (rrt_crmsa_region4_f32), `stream` (rrt_crmsa_stream4_f32) and `parts` (rrt_crmsa_combine_parts_f32, fed row
   records synthesised here in float64), each wherever its *_supported predicate, restated below, admits the shape.
   Input families: mild (|logit| <= ~7), peaked (largest |logit| 50, the region maximum of representative 0 moved into every
   block's share of the rows in turn, one region per position) and pad-bound (every real logit of one representative above /
   below the pads' exact 0, at both scales).
   Bound per quantity: max(project bound, 8 x e32), e32 = the error against float64 of the same restatement evaluated in
   plain fp32 on the CPU on the same inputs -- measured here, never read off the kernels.
B. the backward (crmsa_bwd.hip has no stage entry point): RRTEncoder(n_layers=1).train() against float64 autograd, per
   tensor and, sharper, per row of dx at the arg-min / arg-max token of every (region, representative); with pads at a
   representative's minimum / maximum, against the term the normaliser's gradient would add to a real row (it must vanish).

Every stage output is NaN-filled with canary rows behind it; the one-pass forms' scratch has exactly the size the library
asks for with canary bytes behind it, and they run twice on it (same bits: the merge order is fixed, no stale record is read).  The case lists are plain module data (tests/test_crmsa_stage_grid_cpu.py checks on
the CPU that they cover what is claimed); importing this module needs no device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth

pytestmark = pytest.mark.gpu

TOL = 2e-5                        # the project's stage bound (test_hip_parity.py::test_crmsa_stages); logits: x max(1, max |Lg|)
TOL_STATS = 2e-6                  # mean / rstd, x max(1, largest reference entry): 512-term fp32 sums, |x| <= ~6
E32_FACTOR = 8.0                  # a kernel may be 8 x the fp32 eager evaluation's own error off float64
PEAK_TARGET, PEAK_WINDOW = 50.0, (40.0, 60.0)
RECORDS = []                      # (section, kernel form / instantiation, quantity, e32 or None, kernel error)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_CRMSA_STAGE_ERRORS_OUT")      # the table kept as profiles/crmsa_stage_errors.txt
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
    """per (section, kernel form or instantiation, quantity): cases, worst e32, worst kernel error, worst ratio of a kernel
    error to the same case's e32"""
    rows = {}
    for sec, inst, what, e32, err in records:
        n, w32, werr, wr = rows.get((sec, inst, what), (0, 0.0, 0.0, 0.0))
        rows[(sec, inst, what)] = (n + 1, max(w32, e32 or 0.0), max(werr, err), max(wr, err / e32 if e32 else 0.0))
    lines = [f"{'section':8s} {'kernel form / instantiation':44s} {'quantity':10s} {'cases':>5s} {'worst e32':>10s} "
             f"{'worst err':>10s} {'worst err/e32':>13s}"]
    for (sec, inst, what), (n, w32, werr, wr) in sorted(rows.items()):
        e = f"{w32:10.2e}" if w32 else f"{'-':>10s}"
        r = f"{wr:13.2f}" if wr else f"{'-':>13s}"
        lines.append(f"{sec:8s} {inst:44s} {what:10s} {n:5d} {e} {werr:10.2e} {r}")
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------ the launchers' predicates and dispatch, restated
# Source: the launchers at the end of csrc/crmsa.hip.  tests/test_crmsa_stage_grid_cpu.py reads the instantiations back
# out of that file and checks that the cases below reach every one of them.
FORMS = ("two", "one", "one_u", "four", "four_u", "stream", "parts")      # _u: phi one float off a 16-byte boundary


def r4_blocks(P):
    return 16 if P > 288 else 8 if P > 144 else 4


def supported(form, D, k, P):
    """crmsa_region_supported / crmsa_region4_supported / crmsa_stream4_supported / crmsa_combine_parts_supported; the _u
    forms where the issue asks for them (region4 at k = 4, 5 and P <= 144; crmsa_region's GK = 0 fallback)"""
    if not 1 <= k <= 8:
        return False
    if form == "two":
        return D % 4 == 0
    if form == "parts":
        lds = P * (4 if k <= 4 else 8) * 4 * 2 + ((P + 1) & ~1) * 8 + 16 * ((4 if k <= 4 else 8) + 1) * 16 * 16
        return D % 64 == 0 and 64 <= D <= 512 and lds <= 150 * 1024
    if D != 512:
        return False
    if form in ("one", "one_u"):
        return k <= 3 and P <= 144
    if form == "four":
        return 4 <= P <= 576
    if form == "four_u":
        return 4 <= P <= 144 and k in (4, 5)
    return 16 <= P <= 576                                   # stream (rrt_crmsa_stream4_f32 asks for both predicates)


def instantiation(form, D, k, P):
    """the kernel instantiation(s) a form launches at this shape, as the label the CPU module reads out of crmsa.hip"""
    if form == "two":
        return f"logits512<{k}>+combine512<{k}>" if D == 512 else "logits+combine(generic)"
    if form in ("one", "one_u"):
        return f"region<GK={k if form == 'one' else 0}>"
    if form == "parts":
        return f"combine_parts<KM={4 if k <= 4 else 8}{',COAL' if 3 <= k <= 4 and D == 512 and P <= 144 else ''}>"
    if form == "stream":
        return "stream4<%d,%d,%d>" % ((12, 3, k) if k <= 3 else (8, 3, k) if k <= 6 else (8, 2, k))
    nb, al = r4_blocks(P), form == "four"
    if nb > 4:
        km, gpr = (3 if k <= 3 else 8), False
    elif k == 4:                                            # registers for five representatives; k = 5 has the GPR form instead
        km, gpr = 5, False
    elif al and k in (1, 3, 5):
        km, gpr = k, True
    else:
        km, gpr = (3 if k <= 3 else 8), False
    return f"region4<{nb},12,3,{km}{',GPR' if gpr else ''}>"


def scratch_bytes(P, k):
    """256 bytes of arrival counters + crmsa_region4_scratch_floats"""
    return 256 + 64 * (16 if P > 288 else 8) * (3 if k <= 3 else 8) * (512 + 8) * 4


def share(form, P, k, p):
    """(block of the region, wave or row group inside it) that reads slot p of a region: region4 / stream4 split the region
    into NB runs of ceil(P / NB) slots and deal a run's rows to the block's waves round-robin; the other forms keep a whole
    region in one block (sixteen waves / row groups)"""
    if form in ("four", "four_u", "stream"):
        nb = r4_blocks(P) if form != "stream" else 4
        nw = 12 if form != "stream" or k <= 3 else 8
        pq = (P + nb - 1) // nb
        return p // pq, (p % pq) % nw
    return 0, p % 16


def peak_slots(P, k):
    """the slots the arg-max of representative 0 is moved to, one region each: slot 0, one slot in every block's share of
    every split the forms use at this P (4 blocks: region4 at P <= 144 and stream4; 8 / 16: region4 above), at a wave that
    moves with the block, and the region's last real slot (appended by the builder: it depends on the region)"""
    slots = [0]
    for nb in sorted({4, r4_blocks(P)}):
        pq = (P + nb - 1) // nb
        for b in range(nb):
            rows = min(pq, P - b * pq)
            if rows > 0:
                slots.append(b * pq + (5 * b + 2) % rows)
    return sorted(set(slots))


# ------------------------------------------------------------------ the cases
FRONT_SHAPES = [(50, 1), (300, 9), (1100, 25), (2305, 49), (9000, 144), (9217, 169), (16385, 289), (36864, 576)]   # (L, P8), dim 512
SMALL_DIM_SHAPES = [(64, 300), (64, 1100), (192, 300), (192, 1100)]                                               # (dim, L)
FAMILIES = [("mild", None), ("peaked", None), ("mild", "min"), ("mild", "max"), ("peaked", "min"), ("peaked", "max")]


def region_P(L):
    H, s, add = O.grid(L, 8, 0, 0, 0.0)
    return s * s


def front_ks(P):
    return tuple(range(1, 9)) if P in (144, 169) else (3, 8) if P > 169 else (1, 3, 4, 5, 8)


def mixed_regions(L):
    """regions of the 8 x 8 grid that hold both tokens and pads"""
    H, s, add = O.grid(L, 8, 0, 0, 0.0)
    real = (O.partition_index(H, s) < L).reshape(64, s * s)
    return [r for r in range(64) if real[r].any() and not real[r].all()]


def front_cases():
    """(dim, L, k, scale, pad).  The pad-bound families need a region that holds tokens AND pads: L = 36864 fills its grid,
    and the one-token regions of L = 50 are a token or a pad, never both."""
    out = []
    for L, P in FRONT_SHAPES:
        out += [(512, L, k, sc, pad) for k in front_ks(P) for sc, pad in FAMILIES if not pad or mixed_regions(L)]
    for D, L in SMALL_DIM_SHAPES:
        out += [(D, L, k, sc, pad) for k in (3, 5) for sc, pad in FAMILIES]
    return out


FRONT_CASES = front_cases()


def front_id(D, L, k, scale, pad):
    return f"d{D}-L{L}-P{region_P(L)}-k{k}-{scale}" + (f"-pads_{pad}" if pad else "")


def case_forms(D, k, P):
    return [f for f in FORMS if supported(f, D, k, P)]


# ------------------------------------------------------------------ inputs and the restatement, any dtype
class Base:
    """what depends on (L, dim) only: x1, x0, the 8 x 8 grid, and LayerNorm's statistics / normalised rows in both dtypes"""

    def __init__(self, L, D):
        self.L, self.D = L, D
        self.H, self.s, self.add = O.grid(L, 8, 0, 0, 0.0)
        self.P, self.R, self.Np = self.s * self.s, 64, self.H * self.H
        self.perm = O.partition_index(self.H, self.s)
        self.real = (self.perm < L).reshape(self.R, self.P)
        self.x1 = synth.normal("crm/x1", (L, D)) * np.float32(1.3) + np.float32(0.2)
        self.x0 = synth.normal("crm/x0", (L, D))
        self.stats = {}
        for dt in (np.float64, np.float32):
            x = self.x1.astype(dt)
            mean = x.mean(-1, keepdims=True, dtype=dt)
            xc = x - mean
            rstd = 1 / np.sqrt((xc * xc).mean(-1, keepdims=True, dtype=dt) + dt(1e-5))
            self.stats[dt] = (mean, rstd, xc * rstd)


@functools.lru_cache(maxsize=2)
def base(L, D):
    return Base(L, D)


def _rows(a, rowsrc):
    return a if rowsrc is None else a[rowsrc]


def logits64(b, rowsrc, gm, bt, phi):
    """[R, k, P] float64 logits; pads exactly 0"""
    v = _rows(b.stats[np.float64][2], rowsrc) * gm.astype(np.float64) + bt.astype(np.float64)
    lg = np.concatenate([v @ phi.astype(np.float64), np.zeros((b.add, phi.shape[1]))], 0)[b.perm]
    return lg.reshape(b.R, b.P, -1).transpose(0, 2, 1)


def restate(b, c, dt):
    """rmsa.py:303-335 in dtype dt (the arithmetic of test_crmsa_stages): LN-2, pad, partition, logits, softmax over the
    tokens, softmax over the representatives, min/max normaliser, combine, dispatch + residual + LN.
    -> dict(mr [L, 2], lg / wd [R, k, P], rep [k, R, D], y [L, D])"""
    mean, rstd, xhat = (_rows(a, c["rowsrc"]) for a in b.stats[dt])
    gm, bt, phi = (c[n].astype(dt) for n in ("gm", "bt", "phi"))
    v = xhat * gm + bt
    V = np.concatenate([v, np.zeros((b.add, b.D), dt)], 0)[b.perm].reshape(b.R, b.P, b.D)
    Lg = (V @ phi).transpose(0, 2, 1)
    Cw = np.exp(Lg - Lg.max(-1, keepdims=True))
    Cw /= Cw.sum(-1, keepdims=True, dtype=dt)
    rep = (Cw @ V).transpose(1, 0, 2)
    Dw = np.exp(Lg - Lg.max(1, keepdims=True))
    Dw /= Dw.sum(1, keepdims=True, dtype=dt)
    mn, mx = Lg.min(-1, keepdims=True), Lg.max(-1, keepdims=True)
    wd = (Lg - mn) / (mx - mn + dt(1e-8)) * Dw
    out = np.einsum("rnp,nrd->rpd", wd, c["rep2"].astype(dt))
    z = np.empty((b.Np, b.D), dt)
    z[b.perm] = out.reshape(-1, b.D)
    x2 = _rows(b.x1, c["rowsrc"]).astype(dt) + z[:b.L] + b.x0.astype(dt)
    mu = x2.mean(-1, keepdims=True, dtype=dt)
    xc = x2 - mu
    y = xc / np.sqrt((xc * xc).mean(-1, keepdims=True, dtype=dt) + dt(1e-5)) * c["gm3"].astype(dt) + c["bt3"].astype(dt)
    res = dict(mr=np.concatenate([mean, rstd], 1), lg=Lg, wd=wd, rep=rep, y=y)
    assert all(a.dtype == dt for a in res.values())
    return res


def make_case(D, L, k, scale, pad):
    """the inputs of one case and the float64 facts the family promises (asserted here, so on the CPU and on the GPU box
    alike).  -> dict(gm, bt, phi, rep2, gm3, bt3, rowsrc (None, or the row of the base x1 each token takes), peaks
    [(region, slot)], pad_rep, maxlg)"""
    b = base(L, D)
    c = dict(gm=1.0 + synth.uniform("crm/g", (D,), -0.3, 0.3), bt=synth.uniform("crm/b", (D,), -0.2, 0.2),
             phi=synth.uniform("crm/phi", (D, k), -1, 1) * np.float32(3.0 / np.sqrt(D)),
             rep2=synth.normal("crm/rep2", (k, b.R, D)), gm3=1.0 + synth.uniform("crm/g3", (D,), -0.3, 0.3),
             bt3=synth.uniform("crm/b3", (D,), -0.2, 0.2), rowsrc=None, peaks=[], pad_rep=None)
    if pad:
        # +- c phi_n / |phi_n|^2 on LN's bias moves every real logit of representative n by +- c and leaves the pads at 0
        n = c["pad_rep"] = k // 2
        ph = c["phi"][:, n].astype(np.float64)
        cc = 1.5 * np.abs(logits64(b, None, c["gm"], c["bt"], c["phi"])[:, n][b.real]).max()
        c["bt"] = (c["bt"].astype(np.float64) + (cc if pad == "min" else -cc) * ph / (ph @ ph)).astype(np.float32)
    if scale == "peaked":
        c["phi"] = (c["phi"] * (PEAK_TARGET / np.abs(logits64(b, None, c["gm"], c["bt"], c["phi"])).max())).astype(np.float32)
    Lg = logits64(b, None, c["gm"], c["bt"], c["phi"])
    if scale == "peaked" and not pad:
        # region by region: the token that holds representative 0's maximum changes rows with the token at the target slot
        rowsrc = np.arange(L)
        tok = b.perm.reshape(b.R, b.P)
        full = [r for r in range(b.R) if b.real[r].all()]
        part = [r for r in range(b.R) if b.real[r].any() and not b.real[r].all()]
        targets = [(r, p) for r, p in zip(full, peak_slots(b.P, k))]
        assert len(targets) == len(peak_slots(b.P, k)), "fewer all-real regions than target slots"
        last = (part or full)[-1]                              # the last real slot, of a partly padded region where there is one
        targets.append((last, int(np.nonzero(b.real[last])[0].max())))
        for r, p in targets:
            a = int(Lg[r, 0].argmax())
            assert b.real[r, a] and b.real[r, p]
            rowsrc[[tok[r, a], tok[r, p]]] = rowsrc[[tok[r, p], tok[r, a]]]
        c["rowsrc"], c["peaks"] = rowsrc, targets
        Lg = logits64(b, rowsrc, c["gm"], c["bt"], c["phi"])
        for r, p in targets:
            assert int(Lg[r, 0].argmax()) == p, f"region {r}: the arg-max of representative 0 is not at slot {p}"
    c["maxlg"] = float(np.abs(Lg).max())
    if scale == "peaked":
        assert PEAK_WINDOW[0] <= c["maxlg"] <= PEAK_WINDOW[1], f"largest |logit| {c['maxlg']:.1f} outside {PEAK_WINDOW}"
    if pad:
        padded = [r for r in range(b.R) if b.real[r].any() and not b.real[r].all()]
        assert padded, "no region holds both tokens and pads"
        lr = Lg[:, c["pad_rep"]]
        assert (lr[b.real] > 0).all() if pad == "min" else (lr[b.real] < 0).all(), "the real logits are not of one sign"
        assert (lr[~b.real] == 0).all()
        for r in padded:                                       # the pads' exact 0 is the representative's min / max there
            assert (lr[r].min() if pad == "min" else lr[r].max()) == 0.0
    return c


def parts_records(b, c):
    """the row records the merged R-MSA launch leaves for rrt_crmsa_combine_parts_f32, computed in float64 and rounded to
    fp32: per (token, 64-column slab) the mean and the centred sum of squares of x1 there and d_n = sum_c x1[c] gamma[c]
    phi[c, n]; record stride 2 + k floats rounded up to whole float4s (the tail floats stay NaN, as the launch leaves them)"""
    k, NS = c["phi"].shape[1], b.D // 64
    K2 = (2 + k + 3) // 4 * 4
    xs = _rows(b.x1, c["rowsrc"]).astype(np.float64).reshape(b.L, NS, 64)
    m = xs.mean(-1)
    part = np.full((b.L, NS, K2), np.nan, dtype=np.float32)
    part[..., 0] = m
    part[..., 1] = ((xs - m[..., None]) ** 2).sum(-1)
    gphi = (c["gm"].astype(np.float64)[:, None] * c["phi"].astype(np.float64)).reshape(NS, 64, k)
    part[..., 2:2 + k] = np.einsum("tsc,sck->tsk", xs, gphi)
    return part


def bounds(c, ref, ref32):
    """{quantity: (e32, bound)}: max(project bound, 8 x e32)"""
    proj = dict(mr=TOL_STATS * max(1.0, float(np.abs(ref["mr"]).max())), lg=TOL * max(1.0, c["maxlg"]), wd=TOL, rep=TOL, y=TOL)
    out = {}
    for what, p in proj.items():
        e32 = float(np.abs(ref32[what].astype(np.float64) - ref[what]).max())
        out[what] = (e32, max(p, E32_FACTOR * e32))
    return out


# ------------------------------------------------------------------ A. every front form against float64
def _run_form(form, b, c, d, k):
    """one form into fresh NaN-filled, canary-guarded outputs -> {quantity: device tensor}, [buffers whose canary broke]"""
    from hip_util import CANARY_BYTE, CANARY_BYTES, DEV, _guard_intact, _guarded, p, stream
    lib = _lib.load()
    L, D, g8 = b.L, b.D, d["g8"]
    phi = d["phi_u"] if form.endswith("_u") else d["phi"]
    if form.endswith("_u"):
        assert phi.data_ptr() % 16 == 4 and d["gm"].data_ptr() % 16 == 0 and d["bt"].data_ptr() % 16 == 0
    else:
        assert all(d[n].data_ptr() % 16 == 0 for n in ("gm", "bt", "phi"))
    bufs = dict(mr=(_guarded(L, 2), L), lg=(_guarded(b.Np, k), b.Np), wd=(_guarded(b.Np, k), b.Np), rep=(_guarded(k * b.R, D), k * b.R))
    mr, lg, wd, rep = (bufs[n][0] for n in ("mr", "lg", "wd", "rep"))
    a = (p(d["x1"]), p(d["gm"]), p(d["bt"]), p(phi), p(mr), p(lg), p(wd), p(rep), L, D, k, C.byref(g8))
    runs = 1
    if form == "two":
        _lib.check(lib.rrt_crmsa_logits_f32(p(d["x1"]), p(d["gm"]), p(d["bt"]), p(phi), p(mr), p(lg), L, D, k, C.byref(g8), stream()), "logits")
        _lib.check(lib.rrt_crmsa_combine_f32(p(d["x1"]), p(d["gm"]), p(d["bt"]), p(mr), p(lg), p(wd), p(rep), L, D, k, C.byref(g8), stream()),
                   "combine")
    elif form in ("one", "one_u"):
        _lib.check(lib.rrt_crmsa_region_f32(*a, stream()), "region")
    elif form == "parts":
        _lib.check(lib.rrt_crmsa_combine_parts_f32(p(d["x1"]), p(d["part"]), p(d["gm"]), p(d["bt"]), p(phi), p(wd), p(rep), L, D, k,
                                                   C.byref(g8), stream()), "combine_parts")
        del bufs["mr"], bufs["lg"]
    else:
        # twice on the same scratch (the entry point zeroes the arrival counters itself on every call): the second call finds
        # the first one's records in the scratch and must give the same bits -- run-to-run determinism of the merge order,
        # and no stale record read
        need = scratch_bytes(b.P, k)
        scratch = torch.full((need + CANARY_BYTES,), 0x5A, dtype=torch.uint8, device=DEV)
        scratch[need:] = CANARY_BYTE
        entry = lib.rrt_crmsa_stream4_f32 if form == "stream" else lib.rrt_crmsa_region4_f32
        _lib.check(entry(*a, p(scratch), need, stream()), form)
        again = {n: _guarded(rows, t.shape[1]) for n, (t, rows) in bufs.items()}
        a2 = a[:4] + tuple(p(again[n]) for n in ("mr", "lg", "wd", "rep")) + a[8:]
        _lib.check(entry(*a2, p(scratch), need, stream()), form + " again")
        runs = 2
    torch.cuda.synchronize()
    broken = [n for n, (t, rows) in bufs.items() if not _guard_intact(t, rows)]
    if runs == 2:
        broken += [n + " (second call)" for n, (t, rows) in bufs.items() if not _guard_intact(again[n], rows)]
        broken += [] if bool((scratch[need:] == CANARY_BYTE).all()) else ["scratch"]
        broken += [n + ": the second call on the same scratch gives other bits" for n, (t, rows) in bufs.items()
                   if not torch.equal(t[:rows].view(torch.int32), again[n][:rows].view(torch.int32))]
    return {n: t[:rows] for n, (t, rows) in bufs.items()}, broken


@pytest.mark.parametrize("D,L,k,scale,pad", FRONT_CASES, ids=[front_id(*c) for c in FRONT_CASES])
def test_front_forms_against_float64(D, L, k, scale, pad):
    """mean_rstd and the logits (where the form writes them), the dispatch weights and the representatives of every form the
    shape admits, then rrt_crmsa_dispatch_ln_f32 on the form's own dispatch weights, all against float64"""
    from hip_util import _guard_intact, _guarded, dev, p, stream, DEV
    lib = _lib.load()
    b = base(L, D)
    c = make_case(D, L, k, scale, pad)
    ref, ref32 = restate(b, c, np.float64), restate(b, c, np.float32)
    bnd = bounds(c, ref, ref32)
    forms = case_forms(D, k, b.P)
    d = {n: dev(c[n]) for n in ("gm", "bt", "phi", "rep2", "gm3", "bt3")}
    d["x1"], d["x0"], d["g8"] = dev(_rows(b.x1, c["rowsrc"])), dev(b.x0), _lib.region_grid(L, 8)
    assert (d["g8"].H, d["g8"].s, d["g8"].add) == (b.H, b.s, b.add)
    d["phi_keep"] = torch.empty((D * k + 1,), device=DEV)
    d["phi_keep"][1:] = d["phi"].reshape(-1)
    d["phi_u"] = d["phi_keep"][1:]
    if "parts" in forms:
        d["part"] = torch.from_numpy(parts_records(b, c)).to(DEV)
    failures = []
    for form in forms:
        out, broken = _run_form(form, b, c, d, k)
        failures += [f"{form}: {m}" if ":" in m else f"{form}: wrote past the end of {m}" for m in broken]
        y = _guarded(L, D)
        _lib.check(lib.rrt_crmsa_dispatch_ln_f32(p(d["x1"]), p(d["x0"]), p(out["wd"]), p(d["rep2"]), p(d["gm3"]), p(d["bt3"]), p(y),
                                                 L, D, k, C.byref(d["g8"]), stream()), "dispatch")
        torch.cuda.synchronize()
        if not _guard_intact(y, L):
            failures.append(f"{form}: dispatch wrote past the end of y")
        got = {n: t.cpu().numpy() for n, t in out.items()}
        got["y"] = y[:L].cpu().numpy()
        for n in ("lg", "wd"):
            if n in got:
                got[n] = got[n].reshape(b.R, b.P, k).transpose(0, 2, 1)
        got["rep"] = got["rep"].reshape(k, b.R, D)
        inst = instantiation(form, D, k, b.P)
        for what, g in got.items():
            e32, tol = bnd[what]
            err = float(np.abs(g.astype(np.float64) - ref[what]).max()) if np.isfinite(g).all() else float("inf")
            RECORDS.append(("A " + scale + ("+pads" if pad else ""), inst, what, e32, err))
            print(f"{front_id(D, L, k, scale, pad)} {form:7s} {inst:36s} {what:3s}: max-abs {err:.3e}  e32 {e32:.3e}  bound {tol:.2e}")
            if not err <= tol:
                failures.append(f"{form} [{inst}] {what}: max-abs {err:.3e} > {tol:.2e}")
    assert not failures, "; ".join(failures)


# ------------------------------------------------------------------ B. the backward, through the encoder
BWD_SHAPES = [(50, 3), (300, 1), (1100, 8), (2305, 5), (9217, 3)]         # (N, crmsa_k), regions of 1, 9, 25, 49, 169 tokens
BWD_VARIANTS = ("synth", "peaked", "synth+pads_min", "synth+pads_max", "peaked+pads_min", "peaked+pads_max")
PAD_MARGIN = 1.05


def bwd_cases():
    """(N, k, crmsa_mlp, variant): the synth state, phi rescaled to max |logit| 50, and the two pad-bound bias shifts at either
    scale.  The shifts need a region with tokens and pads (not N = 50)."""
    out = [(N, k, False, v) for N, k in BWD_SHAPES for v in BWD_VARIANTS if "pads" not in v or mixed_regions(N)]
    return out + [(1100, 3, True, "synth"), (1100, 3, True, "peaked")]


BWD_CASES = bwd_cases()


def bwd_logits64(x, st, cfg):
    """float64 logits [64, k, P] of a CR-MSA-only encoder (its input is x itself), pads exactly 0; real [64, P]"""
    N, D = x.shape
    H, s, add = O.grid(N, 8, 0, 0, 0.0)
    perm = O.partition_index(H, s)
    x64 = x.astype(np.float64)
    mu = x64.mean(-1, keepdims=True)
    v = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-5)
    v = v * st["cr_msa.norm.weight"].astype(np.float64) + st["cr_msa.norm.bias"].astype(np.float64)
    if cfg.get("crmsa_mlp"):
        lg = np.tanh(v @ st["cr_msa.attn.phi.0.weight"].astype(np.float64).T) @ st["cr_msa.attn.phi.2.weight"].astype(np.float64).T
    else:
        lg = v @ st["cr_msa.attn.phi"].astype(np.float64)
    lg = np.concatenate([lg, np.zeros((add, lg.shape[1]))], 0)[perm]
    return lg.reshape(64, s * s, -1).transpose(0, 2, 1), (perm < N).reshape(64, s * s), perm.reshape(64, s * s)


def bwd_state(N, k, mlp, variant):
    """-> cfg, state, x, G, pad representative (or None)"""
    cfg = dict(mlp_dim=512, n_layers=1, crmsa_k=k, crmsa_mlp=mlp)
    st = synth.encoder_state(**cfg)
    x = synth.bag(N, 512, tag=f"crm/bwd/{N}")
    G = synth.normal(f"crm/bwd/G/{N}", (N, 512))
    key = "cr_msa.attn.phi.2.weight" if mlp else "cr_msa.attn.phi"
    n = None
    if "pads" in variant:
        # pads hold the minimum: + c phi_n / |phi_n|^2 on the bias lifts every real logit of representative n above the pads'
        # 0 (section A's shift).  Pads hold the maximum: pushing n alone below 0 starves its share of the softmax over the
        # representatives, and the normaliser's gradient with it -- such a state cannot tell a misrouted arg-max gradient
        # from a right one -- so the bias moves by Phi (Phi^T Phi)^-1 c instead, which lowers EVERY representative m by c_m
        # and leaves their shares as they were.  c = PAD_MARGIN x the representative's largest |real logit|.
        n = k // 2
        lg, real, _ = bwd_logits64(x, st, cfg)
        ph = st[key].astype(np.float64)
        cc = PAD_MARGIN * np.abs(lg.transpose(0, 2, 1)[real]).max(0)
        if variant.endswith("min"):
            cc = cc * (np.arange(k) == n)
        else:
            cc = -cc
        st["cr_msa.norm.bias"] = (st["cr_msa.norm.bias"].astype(np.float64) + ph @ np.linalg.solve(ph.T @ ph, cc)).astype(np.float32)
    if "peaked" in variant:
        st[key] = (st[key] * (PEAK_TARGET / np.abs(bwd_logits64(x, st, cfg)[0]).max())).astype(np.float32)
    return cfg, st, x, G, n


def normaliser_terms64(x, st, cfg, G, n, sign):
    """float64 autograd of the same encoder with the region minimum and maximum cut out of the graph: dx without the min/max
    normaliser's own gradient, and per mixed region the dx row that gradient WOULD add if it were sent to the real token with
    the smallest (sign > 0) / largest real logit of representative n instead of the pad that holds the minimum / maximum.
    -> dx_cut [N, D], {region: (token, row [D])}"""
    import torch.nn.functional as F
    N, D = x.shape
    k, heads = cfg["crmsa_k"], cfg.get("crmsa_heads", 8)
    t = {m: torch.from_numpy(np.ascontiguousarray(v)).double() for m, v in st.items()}
    xl = torch.from_numpy(x).double().requires_grad_(True)
    H, s, add = O.grid(N, 8, 0, 0, 0.0)
    P = s * s
    perm = torch.from_numpy(O.partition_index(H, s).astype(np.int64))
    v = F.layer_norm(xl, (D,), t["cr_msa.norm.weight"], t["cr_msa.norm.bias"], 1e-5)
    xr = torch.cat([v, torch.zeros((add, D), dtype=torch.float64)])[perm].reshape(64, P, D)
    lg = (xr @ t["cr_msa.attn.phi"]).transpose(1, 2)
    mn = lg.min(-1, keepdim=True)[0].detach().requires_grad_(True)
    mx = lg.max(-1, keepdim=True)[0].detach().requires_grad_(True)
    rep = (lg.softmax(-1) @ xr).transpose(0, 1)                                      # [k, R, D]: k sequences of 64 regions
    qkv = F.linear(rep, t["cr_msa.attn.attn.qkv.weight"], t["cr_msa.attn.attn.qkv.bias"])
    q, kk, vv = qkv.reshape(k, 64, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    o = ((q * (D // heads) ** -0.5) @ kk.transpose(-2, -1)).softmax(-1) @ vv
    rep2 = F.linear(o.transpose(1, 2).reshape(k, 64, D), t["cr_msa.attn.attn.proj.weight"], t["cr_msa.attn.attn.proj.bias"])
    rep2 = rep2.transpose(0, 1)                                                      # [R, k, D]
    wd = (lg - mn) / (mx - mn + 1e-8) * lg.softmax(1)
    z = torch.zeros((H * H, D), dtype=torch.float64).index_put((perm,), (wd.transpose(1, 2) @ rep2).reshape(-1, D))
    y = F.layer_norm(xl + z[:N], (D,), t["norm.weight"], t["norm.bias"], 1e-5)
    (y * torch.from_numpy(G).double()).sum().backward(retain_graph=True)
    dx_cut = xl.grad.numpy().copy()
    g = (mn if sign > 0 else mx).grad.numpy()[:, n, 0]
    lgn, real = lg.detach().numpy()[:, n], (perm.numpy() < N).reshape(64, P)
    rows = {}
    for r in mixed_regions(N):
        cand = np.where(real[r], sign * lgn[r], np.inf)
        p = int(cand.argmin())
        (row,) = torch.autograd.grad(lg[r, n, p], xl, retain_graph=True)
        tok = int(perm.numpy().reshape(64, P)[r, p])
        rows[r] = (tok, g[r] * row.numpy()[tok])
    return dx_cut, rows


def check_backward(tag, dx, grads, dx_ref, grads_ref, lg, real, tok, cut=None):
    """the criteria of section B on numpy arrays.  grads / grads_ref: {parameter name: array}; cut: None or (pad
    representative, dx_cut, {region: (token, row)}) from normaliser_terms64.  -> [failure messages]"""
    fails = []
    floor = 1e-3 * max([np.abs(dx_ref).max()] + [np.abs(v).max() for v in grads_ref.values()])
    for name, ref in [("dx", dx_ref)] + sorted(grads_ref.items()):
        got = dx if name == "dx" else grads[name]
        scale = np.abs(ref).max() if np.abs(ref).max() > 0 else floor        # the floor: identically-zero references only
        err = np.abs(got.astype(np.float64) - ref).max() / scale if np.isfinite(got).all() else np.inf
        RECORDS.append(("B", tag, name.replace("cr_msa.", ""), None, float(err)))
        if not err <= 1e-3:
            fails.append(f"{name}: {err:.2e} of the tensor's largest entry")
    # sharper: the rows of dx at the arg-min and arg-max token of every (region, representative) that is a real token
    R, k, P = lg.shape
    hit = {int(tok[r, a]) for r in range(R) for n in range(k) for a in (lg[r, n].argmin(), lg[r, n].argmax()) if real[r, a]}
    rows = np.array(sorted(hit))
    rel = np.abs(dx[rows].astype(np.float64) - dx_ref[rows]).max(-1) / np.maximum(np.abs(dx_ref[rows]).max(-1), 1e-300)
    RECORDS.append(("B", tag, "dx min/max rows", None, float(rel.max())))
    print(f"{tag}: {len(rows)} arg-min / arg-max rows, worst {rel.max():.2e} of the row's largest entry")
    if not rel.max() <= 1e-3:
        fails.append(f"dx row of token {rows[rel.argmax()]} (an arg-min / arg-max): {rel.max():.2e} of the row's largest entry")
    if cut is not None:
        n, dx_cut, terms = cut
        # the float64 runs agree: the normaliser's gradient is all that separates them, and it sits on the hit rows only
        rest = np.setdiff1d(np.arange(len(dx_ref)), rows)
        assert np.abs(dx_ref[rest] - dx_cut[rest]).max() <= 1e-9 * np.abs(dx_ref).max()
        sized = 0
        for r, (t, row) in terms.items():
            assert not real[r, (lg[r, n].argmin() if lg[r, n].min() == 0 else lg[r, n].argmax())], "the bound is not a pad"
            size = np.abs(row).max()
            if size < 4e-3 * np.abs(dx_ref[t]).max():
                continue                 # below the row's own 1e-3 bound (checked above for the whole of dx): nothing to tell apart
            sized += 1
            mine = tok[r][real[r]]
            err = np.abs(dx[mine].astype(np.float64) - dx_ref[mine]).max()
            if not err < 0.5 * size:
                fails.append(f"region {r}: a real row of dx is off by {err:.2e}, the normaliser's term is {size:.2e}")
        print(f"{tag}: the normaliser's term is visible in {sized} of {len(terms)} regions with pads")
        assert sized >= 1, f"{tag}: in no region with pads is the normaliser's term large enough to be told from rounding"
    return fails


@pytest.mark.parametrize("N,k,mlp,variant", BWD_CASES, ids=[f"N{N}-k{k}{'-mlp' if m else ''}-{v}" for N, k, m, v in BWD_CASES])
def test_backward_against_float64(N, k, mlp, variant):
    """RRTEncoder(n_layers=1).train(), loss <y, G>: every parameter gradient and dx within 1e-3 of the tensor's own largest
    reference entry (float64 autograd of O.forward_eager); each dx row at an arg-min / arg-max token within 1e-3 of the row's
    own largest entry; pad-bound: the normaliser's gradient must fall on a pad and vanish -- in every region with pads where
    the term it would add to a real row is at least 4 x that row's own bound (at least one region per case, asserted), no
    real row may be off by half the term"""
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTEncoder
    cfg, st, x, G, n = bwd_state(N, k, mlp, variant)
    lg, real, tok = bwd_logits64(x, st, cfg)
    if "peaked" in variant:
        assert PEAK_WINDOW[0] <= np.abs(lg).max() <= PEAK_WINDOW[1]
    y64, x_leaf, params = O.forward_eager(x, st, cfg, grad=True)
    (y64 * torch.from_numpy(G).double()).sum().backward()
    cut = None
    if n is not None:
        sign = 1 if variant.endswith("min") else -1
        assert (sign * lg[:, n][real] > 0).all() and mixed_regions(N)
        cut = (n,) + normaliser_terms64(x, st, cfg, G, n, sign)
    enc = RRTEncoder(drop_out=0., **cfg)
    enc.load_state_dict({m: torch.from_numpy(v.copy()) for m, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    assert y.grad_fn is not None
    assert np.abs(y.detach().cpu().numpy() - y64.detach().numpy()).max() <= 2e-4
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    grads = {m: prm.grad.cpu().numpy() for m, prm in enc.named_parameters()}
    grads_ref = {m: params[m].grad.numpy().reshape(grads[m].shape) for m in grads}
    fails = check_backward(f"N{N} k{k}{' mlp' if mlp else ''} {variant}", xd.grad.cpu().numpy(), grads, x_leaf.grad.numpy(),
                           grads_ref, lg, real, tok, cut)
    assert not fails, "; ".join(fails)
