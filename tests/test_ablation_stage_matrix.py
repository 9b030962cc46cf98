"""GPU (-m gpu): the ablation kernels of csrc/peg.hip and csrc/epeg_variants.hip, one stage at a time, against float64
restatements of the reference's lines -- never against another kernel.

A. PEG / PPEG (emb_position.py:24-82) through rrt_peg_f32 / rrt_peg_backward_f32: y, dx, every dW, every db, for every kernel
   side the file instantiates, 2-D and (k, 1), with and without biases, a full and a half-filled 64-channel slab, and the bags
   at which the wrapped square, PPEG's 7 x 7 zero padding and the 8 x 8 tiling change shape.  dx is also held row by row at
   the tokens that were wrapped into the tail of the square (two contributions each).
B. the 2-D score-map EPEG (rmsa.py:78-79,106-108) through rrt_attn_scoremap_f32 / rrt_attn_scoremap_backward_f32: o, dq, dk,
   dv, dW at the region sizes where the kernels change from LDS to > 64 KiB of LDS to global maps, head dims 16, 64, 80,
   stencils up to 63 x 63 (wider than the map), on mild and on peaked (max |S~| = 50) scores.
C. the value EPEG (rmsa.py:80-85,114-129) through rrt_value_pe_f32 / rrt_value_pe_backward_f32: pe, the dv added into a
   pre-filled d_qkv, dW, db; all four type / shape combinations reduce to (k, 1) and k x k here.  The channel permutation is
   asserted on an input whose every v column holds its own index.
D. the composition around them in the encoder (add_cols / copy_cols / sub, the stash of v + pe): RRTEncoder(n_layers=2,
   cr_msa=False).train() against float64 autograd of O.forward_eager, regions that hold pads; and PEG k = 11 / PPEG k = 9
   (k, 1) through train().

Bound per quantity: max(TOL, 8 x e32) relative to max(1, max |reference|) (gradients: to the largest entry of that gradient
tensor of this stage alone), e32 = the error against float64 of the same restatement evaluated in plain fp32 on the CPU on the
same inputs -- measured here, never read off a kernel.

Every output is NaN-filled with canary rows behind it, scratch and workspaces have exactly the size the library asks for with
canary bytes behind them, and every backward runs twice on the same workspace and must give the same bits (fixed summation
orders, no atomics).  The case lists are plain module data (tests/test_ablation_stage_grid_cpu.py checks on the CPU that they
cover what is claimed); importing this module needs no device."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rrt_oracle as O
from rrt_mil_amd import _lib, synth

pytestmark = pytest.mark.gpu

TOL = 2e-5                        # the project's stage bound, as in tests/test_crmsa_stage_matrix.py
E32_FACTOR = 8.0                  # a kernel may be 8 x the fp32 eager evaluation's own error off float64
PEAK_TARGET, PEAK_WINDOW = 50.0, (40.0, 60.0)
LDS_MAX, LDS_OPT_IN = 160 * 1024, 64 * 1024
RECORDS = []                      # (section, case group, quantity, e32 (relative), kernel error (relative))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()
    yield
    out = os.environ.get("RRT_ABLATION_STAGE_ERRORS_OUT")   # the table kept as profiles/ablation_stage_errors.txt
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
    """per (section, case group, quantity): cases, worst e32, worst kernel error (both relative to the quantity's scale), worst
    ratio of a kernel error to the same case's e32"""
    rows = {}
    for sec, grp, what, e32, err in records:
        n, w32, werr, wr = rows.get((sec, grp, what), (0, 0.0, 0.0, 0.0))
        rows[(sec, grp, what)] = (n + 1, max(w32, e32), max(werr, err), max(wr, err / e32 if e32 else 0.0))
    lines = [f"{'section':8s} {'case group':44s} {'quantity':22s} {'cases':>5s} {'worst e32':>10s} {'worst err':>10s} "
             f"{'worst err/e32':>13s}"]
    for (sec, grp, what), (n, w32, werr, wr) in sorted(rows.items()):
        r = f"{wr:13.2f}" if wr else f"{'-':>13s}"
        lines.append(f"{sec:8s} {grp:44s} {what:22s} {n:5d} {w32:10.2e} {werr:10.2e} {r}")
    return "\n".join(lines) + "\n"


def judge(sec, grp, case, what, got, ref, ref32, grad, fails):
    """one quantity of one case against float64: relative to max(1, max |ref|) (a gradient: to max |ref| of this tensor), bound
    max(TOL, 8 x e32).  Appends to RECORDS and, on a miss, to fails."""
    ref = np.asarray(ref, dtype=np.float64)
    top = float(np.abs(ref).max()) if ref.size else 0.0
    scale = (top if top > 0 else 1.0) if grad else max(1.0, top)
    e32 = float(np.abs(np.asarray(ref32, dtype=np.float64) - ref).max()) / scale if ref.size else 0.0
    got = np.asarray(got)
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref).max()) / scale if np.isfinite(got).all() and ref.size else \
        (0.0 if not ref.size else float("inf"))
    bound = max(TOL, E32_FACTOR * e32)
    RECORDS.append((sec, grp, what, e32, err))
    if not err <= bound:
        fails.append(f"{case} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")
    return err, e32, bound


def _t(a, dt, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).requires_grad_(grad)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ================================================================== A. PEG / PPEG
PEG_KINDS = ("peg", "ppeg")
PEG_KS = (1, 3, 5, 7, 9, 11)
PEG_CS = (64, 96)                                   # 96: a half-filled second 64-channel slab
PEG_NS = (1, 2, 3, 5, 36, 37, 49, 50, 64, 65, 290)
PEG_CASES = [(kind, k, one_d, bias, Cc, N) for kind in PEG_KINDS for k in PEG_KS for one_d in (False, True)
             for bias in (True, False) for Cc in PEG_CS for N in PEG_NS]
PEG_GROUPS = [(kind, k) for kind in PEG_KINDS for k in PEG_KS]


def peg_sides(N, kind):
    """(H0, H): the wrapped square's side ceil(sqrt(N)) and the grid's (PPEG zero-pads a smaller square to 7 x 7)"""
    H0 = math.isqrt(N - 1) + 1 if N > 1 else 1
    return H0, (7 if kind == "ppeg" and H0 < 7 else H0)


def peg_kk(kind, k):
    """the template side the launchers pick: PPEG's largest conv is at least its 5 x 5, PEG k = 1 runs in the 3 x 3 form"""
    return max(k, 5) if kind == "ppeg" else max(k, 3)


def peg_fwd_lds(KK):
    return (8 + 2 * (KK // 2)) ** 2 * 64 * 4


def peg_dw_lds(KK):
    """peg_bwd_dw_kernel: the three waves' partial sums take the patch's place"""
    return max((8 + 2 * (KK // 2)) ** 2 * 64, 3 * KK * KK * 64) * 4


def peg_workspace_bytes(N, Cc, k, kind):
    """peg_bwd_workspace restated: the adjoint stencil's output on the wrapped square, per-tile tap partials and their sum,
    the column sums' partials, 1 KiB of slack"""
    H0, H = peg_sides(N, kind)
    KK, tiles = peg_kk(kind, k), ((H + 7) // 8) ** 2
    return (H0 * H0 * Cc + (tiles + 1) * KK * KK * Cc + ((N + 127) // 128 + 1) * Cc) * 4 + 1024


def peg_names(kind):
    return ("proj", "proj1", "proj2") if kind == "ppeg" else ("proj",)


@functools.lru_cache(maxsize=None)
def peg_bag(N, Cc):
    return synth.normal(f"abl/peg/x/{N}x{Cc}", (N, Cc)), synth.normal(f"abl/peg/dy/{N}x{Cc}", (N, Cc))


@functools.lru_cache(maxsize=8)
def peg_params(kind, k, one_d, bias, Cc):
    """{state_dict key: array} of the position encoder, in the reference's names"""
    st = {}
    for name, kk in zip(peg_names(kind), (k, 5, 3)):
        kw = 1 if one_d else kk
        tag = f"abl/peg/{kind}/{name}/{kk}x{kw}/{Cc}"
        st[f"pos_embedding.{name}.weight"] = synth.uniform(tag + "/w", (Cc, 1, kk, kw), -1, 1) * np.float32(1 / np.sqrt(kk * kw))
        if bias:
            st[f"pos_embedding.{name}.bias"] = synth.uniform(tag + "/b", (Cc,), -0.25, 0.25)
    return st


def pos_restate(x, ws, bs, kind):
    """emb_position.py:24-82 in x's dtype: wrap-pad to the square, PPEG zero-pads to 7 x 7, depth-wise convs + identity, keep
    the first N tokens"""
    N, D = x.shape
    H0, H = peg_sides(N, kind)
    t = torch.cat([x, x[:H0 * H0 - N]], 0)
    if H > H0:
        t = torch.cat([t, torch.zeros((H * H - H0 * H0, D), dtype=x.dtype)], 0)
    feat = t.t().reshape(1, D, H, H)
    out = feat
    for w, b in zip(ws, bs):
        out = out + F.conv2d(feat, w, b, padding=(w.shape[2] // 2, w.shape[3] // 2), groups=D)
    return out.flatten(2)[0].t()[:N]


def peg_reference(kind, k, one_d, bias, Cc, N, dt):
    """-> dict(y, dx, dw0.., db0..) as numpy arrays of dtype dt"""
    x, dy = peg_bag(N, Cc)
    st = peg_params(kind, k, one_d, bias, Cc)
    xl = _t(x, dt, True)
    ws = [_t(st[f"pos_embedding.{n}.weight"], dt, True) for n in peg_names(kind)]
    bs = [_t(st[f"pos_embedding.{n}.bias"], dt, True) if bias else None for n in peg_names(kind)]
    y = pos_restate(xl, ws, bs, kind)
    (y * _t(dy, dt)).sum().backward()
    out = dict(y=y.detach().numpy(), dx=xl.grad.numpy())
    for i, w in enumerate(ws):
        out[f"dw{i}"] = w.grad.numpy()
        if bias:
            out[f"db{i}"] = bs[i].grad.numpy()
    return out


def _ptr3(ts):
    from hip_util import p
    ts = list(ts) + [None] * (3 - len(ts))
    return (C.c_void_p * 3)(*[p(t) for t in ts])


def _peg_backward_once(lib, d, kind, k, one_d, bias, Cc, N, ws_buf, need):
    from hip_util import _guarded, p, stream
    n = len(peg_names(kind))
    dx = _guarded(N, Cc)
    dws = [_guarded(Cc, w.shape[2] * w.shape[3]) for w in d["w"]]
    dbs = [_guarded(1, Cc) if bias else None for _ in range(n)]
    _lib.check(lib.rrt_peg_backward_f32(p(d["x"]), p(d["dy"]), _ptr3(d["w"]), p(dx), _ptr3(dws), _ptr3(dbs) if bias else None,
                                        N, Cc, k, int(one_d), int(kind == "ppeg"), p(ws_buf), need, stream()), "peg backward")
    return dx, dws, dbs


@pytest.mark.parametrize("kind,k", PEG_GROUPS, ids=[f"{kind}-k{k}" for kind, k in PEG_GROUPS])
def test_peg_stage_against_float64(kind, k):
    """y, dx (whole and row by row at the wrapped tokens), every dW and db of every case of this (kind, k); rows behind N
    untouched; the workspace's size is the restated formula and nothing is written behind it; two backward runs, same bits"""
    from hip_util import CANARY_BYTE, CANARY_BYTES, DEV, _guard_intact, _guarded, dev, p, stream
    lib = _lib.load()
    fails = []
    for case in [c for c in PEG_CASES if c[:2] == (kind, k)]:
        _, _, one_d, bias, Cc, N = case
        cid = f"{kind}-k{k}{'x1' if one_d else ''}-{'bias' if bias else 'nobias'}-C{Cc}-N{N}"
        grp = f"{kind} K={peg_kk(kind, k)}"
        x, dy = peg_bag(N, Cc)
        st = peg_params(kind, k, one_d, bias, Cc)
        ref, ref32 = peg_reference(*case, torch.float64), peg_reference(*case, torch.float32)
        y64 = O._pos64(x.astype(np.float64), st, kind, one_d)
        assert np.abs(ref["y"] - y64).max() <= 1e-12 * max(1.0, np.abs(y64).max()), cid      # the graph is the oracle's forward
        names = peg_names(kind)
        d = dict(x=dev(x), dy=dev(dy), w=[dev(st[f"pos_embedding.{n}.weight"]) for n in names],
                 b=[dev(st[f"pos_embedding.{n}.bias"]) if bias else None for n in names])
        y = _guarded(N, Cc)
        _lib.check(lib.rrt_peg_f32(p(d["x"]), _ptr3(d["w"]), _ptr3(d["b"]) if (bias or kind == "ppeg") else None, p(y), N, Cc, k,
                                   int(one_d), int(kind == "ppeg"), stream()), "peg")
        need = C.c_size_t()
        _lib.check(lib.rrt_peg_backward_workspace_size(N, Cc, k, int(kind == "ppeg"), C.byref(need)), "peg ws")
        assert need.value == peg_workspace_bytes(N, Cc, k, kind), cid
        ws_buf = torch.full((need.value + CANARY_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)
        ws_buf[need.value:] = CANARY_BYTE
        runs = [_peg_backward_once(lib, d, kind, k, one_d, bias, Cc, N, ws_buf, need.value) for _ in range(2)]
        torch.cuda.synchronize()
        if not _guard_intact(y, N):
            fails.append(f"{cid}: rows behind N of y were written")
        if not bool((ws_buf[need.value:] == CANARY_BYTE).all()):
            fails.append(f"{cid}: the backward wrote behind its workspace")
        for r, (dx, dws, dbs) in enumerate(runs):
            broken = [n for n, t, rows in [("dx", dx, N)] + [(f"dw{i}", t, Cc) for i, t in enumerate(dws)] +
                      [(f"db{i}", t, 1) for i, t in enumerate(dbs) if t is not None] if not _guard_intact(t, rows)]
            fails += [f"{cid}: run {r} wrote past the end of {n}" for n in broken]
        (dx, dws, dbs), (dx2, dws2, dbs2) = runs
        pairs = [("dx", dx[:N], dx2[:N])] + [(f"dw{i}", a[:Cc], b[:Cc]) for i, (a, b) in enumerate(zip(dws, dws2))]
        pairs += [(f"db{i}", a[:1], b[:1]) for i, (a, b) in enumerate(zip(dbs, dbs2)) if a is not None]
        fails += [f"{cid}: the second backward on the same workspace gives other bits in {n}" for n, a, b in pairs if not _same_bits(a, b)]
        got = dict(y=y[:N].cpu().numpy(), dx=dx[:N].cpu().numpy())
        for i, w in enumerate(d["w"]):
            got[f"dw{i}"] = dws[i][:Cc].cpu().numpy().reshape(w.shape)
            if bias:
                got[f"db{i}"] = dbs[i][0].cpu().numpy()
        for what in ref:
            err, e32, bound = judge("A", grp, cid, what, got[what], ref[what], ref32[what], what != "y", fails)
        # the wrapped tokens: dx[t] = g[t] + g[N + t], each row against its own largest entry
        H0, _ = peg_sides(N, kind)
        for t in range(H0 * H0 - N):
            judge("A", grp, cid, "dx wrapped rows", got["dx"][t], ref["dx"][t], ref32["dx"][t], True, fails)
    print(error_table([r for r in RECORDS if r[0] == "A" and r[1] == f"{kind} K={peg_kk(kind, k)}"]))
    assert not fails, f"{len(fails)} failures: " + "; ".join(fails[:12])


# ================================================================== B. the 2-D score-map EPEG
SM_PS = (1, 4, 16, 64, 81, 100, 121, 144, 196, 225)
SM_HEADS = ((2, 64), (3, 16), (2, 80))              # (heads, head dim): one round of the lane loops, a quarter, two rounds
SM_FAMILIES = ("mild", "peaked")
SM_FWD_PATH = {1: "lds", 4: "lds", 16: "lds", 64: "lds", 81: "lds", 100: "lds", 121: "lds", 144: "lds>64K", 196: "lds>64K",
               225: "global"}
SM_BWD_PATH = {1: "lds", 4: "lds", 16: "lds", 64: "lds", 81: "lds>64K", 100: "lds>64K", 121: "global", 144: "global",
               196: "global", 225: "global"}


def sm_ks(P):
    return (3, 5, 15) + ((63,) if P in (4, 16) else ())          # 63: wider than the map on every side


def sm_regions(P):
    return 3 if P <= 64 else 2


SM_CASES = [(P, heads, hd, k, fam) for P in SM_PS for heads, hd in SM_HEADS for k in sm_ks(P) for fam in SM_FAMILIES]


def sm_path(P, k, maps):
    """the launchers' choice restated: maps [P, P] maps + the taps + four probability rows in LDS while they fit the CU, with
    the opt-in above 64 KiB; else the maps in global scratch"""
    lds = (maps * P * P + k * k + 4 * P) * 4
    return "global" if lds > LDS_MAX else "lds>64K" if lds > LDS_OPT_IN else "lds"


def sm_scratch_bytes(R, P, heads, k, backward):
    maps = 3 if backward else 1
    floats = maps * R * heads * P * P if sm_path(P, k, maps) == "global" else 0
    return (floats + (R * heads * k * k if backward else 0)) * 4


def scoremap_restate(qkv, pw, R, P, heads, hd):
    """rmsa.py:98-110 with the k x k conv over the score map, in qkv's dtype; q arrives scaled -> (o [R*P, dim], S~)"""
    q, k, v = qkv.reshape(R, P, 3, heads, hd).permute(2, 0, 3, 1, 4)
    S = q @ k.transpose(-2, -1)
    S = S + F.conv2d(S, pw, None, padding=pw.shape[2] // 2, groups=heads)
    return (S.softmax(-1) @ v).transpose(1, 2).reshape(R * P, heads * hd), S


def scoremap64(qkv, pw, R, P, heads, hd):
    """the same lines as O._inner_attention64 writes them, numpy float64 -> (o, S~)"""
    t = qkv.astype(np.float64).reshape(R, P, 3, heads, hd).transpose(2, 0, 3, 1, 4)
    S = t[0] @ t[1].transpose(0, 1, 3, 2)
    S = S + O._conv_dw64(S, pw.astype(np.float64), None, True)
    return (O._softmax64(S, -1) @ t[2]).transpose(0, 2, 1, 3).reshape(R * P, heads * hd), S


@functools.lru_cache(maxsize=4)
def sm_inputs(P, heads, hd, k, fam):
    """qkv [R*P, 3*dim] with q scaled by hd^-0.5 as the qkv linear leaves it, the taps, dO; peaked: q rescaled so that the
    largest |S~| is PEAK_TARGET (S~ is linear in q) -> qkv, pw, dO, max |S~|"""
    R, dim = sm_regions(P), heads * hd
    qkv = synth.normal(f"abl/sm/qkv/{P}/{heads}x{hd}", (R * P, 3 * dim))
    qkv[:, :dim] *= np.float32(hd ** -0.5)
    pw = synth.uniform(f"abl/sm/w/{heads}/{k}", (heads, 1, k, k), -1, 1) * np.float32(1.0 / k)
    dO = synth.normal(f"abl/sm/dO/{P}/{heads}x{hd}", (R * P, dim))
    if fam == "peaked":
        top = np.abs(scoremap64(qkv, pw, R, P, heads, hd)[1]).max()
        qkv[:, :dim] *= np.float32(PEAK_TARGET / top)
    top = float(np.abs(scoremap64(qkv, pw, R, P, heads, hd)[1]).max())
    if fam == "peaked":
        assert PEAK_WINDOW[0] <= top <= PEAK_WINDOW[1], f"largest |S~| {top:.1f} outside {PEAK_WINDOW}"
    return qkv, pw, dO, top


def sm_reference(P, heads, hd, k, fam, dt):
    """-> dict(o, dq, dk, dv, dw); dq is the gradient w.r.t. the UNSCALED projection (x hd^-0.5), as the kernel writes it"""
    R, dim = sm_regions(P), heads * hd
    qkv, pw, dO, _ = sm_inputs(P, heads, hd, k, fam)
    ql, wl = _t(qkv, dt, True), _t(pw, dt, True)
    o, _ = scoremap_restate(ql, wl, R, P, heads, hd)
    (o * _t(dO, dt)).sum().backward()
    g = ql.grad.numpy()
    scale = np.asarray(hd ** -0.5, dtype=g.dtype)
    return dict(o=o.detach().numpy(), dq=g[:, :dim] * scale, dk=g[:, dim:2 * dim], dv=g[:, 2 * dim:], dw=wl.grad.numpy())


def _scratch(lib, R, P, heads, k, backward):
    from hip_util import CANARY_BYTE, CANARY_BYTES, DEV
    need = C.c_size_t()
    _lib.check(lib.rrt_attn_scoremap_scratch_size(R, P, heads, k, int(backward), C.byref(need)), "scoremap scratch")
    buf = torch.full((need.value + CANARY_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)
    buf[need.value:] = CANARY_BYTE
    return buf, need.value


SM_GROUPS = [(P, heads, hd) for P in SM_PS for heads, hd in SM_HEADS]


@pytest.mark.parametrize("P,heads,hd", SM_GROUPS, ids=[f"P{P}-fwd_{SM_FWD_PATH[P]}-bwd_{SM_BWD_PATH[P]}-h{h}x{d}" for P, h, d in SM_GROUPS])
def test_scoremap_stage_against_float64(P, heads, hd):
    """o, dq, dk, dv, dW of every case at this region size; the forward and the backward took the branch the size is listed
    for (by the scratch the library asks for and the restated formula); nothing written behind o, d_qkv, dW or the scratch; two
    backward runs on the same scratch, same bits"""
    from hip_util import CANARY, CANARY_BYTE, CANARY_ROWS, DEV, _guard_intact, _guarded, dev, p, stream
    lib = _lib.load()
    fails = []
    for case in [c for c in SM_CASES if c[:3] == (P, heads, hd)]:
        _, _, _, k, fam = case
        R, dim = sm_regions(P), heads * hd
        cid = f"P{P}-h{heads}x{hd}-k{k}-{fam}"
        grp = f"fwd {SM_FWD_PATH[P]} / bwd {SM_BWD_PATH[P]} {fam}"
        qkv, pw, dO, top = sm_inputs(*case)
        ref, ref32 = sm_reference(*case, torch.float64), sm_reference(*case, torch.float32)
        o64, _ = scoremap64(qkv, pw, R, P, heads, hd)
        assert np.abs(ref["o"] - o64).max() <= 1e-12, cid
        # --- the branches
        assert sm_path(P, k, 1) == SM_FWD_PATH[P] and sm_path(P, k, 3) == SM_BWD_PATH[P], cid
        fbuf, fneed = _scratch(lib, R, P, heads, k, False)
        bbuf, bneed = _scratch(lib, R, P, heads, k, True)
        assert fneed == sm_scratch_bytes(R, P, heads, k, False) and bneed == sm_scratch_bytes(R, P, heads, k, True), cid
        assert (fneed > 0) == (SM_FWD_PATH[P] == "global") and (bneed > R * heads * k * k * 4) == (SM_BWD_PATH[P] == "global"), cid
        d = dict(qkv=dev(qkv), pw=dev(pw), dO=dev(dO))
        o = _guarded(R * P, dim)
        _lib.check(lib.rrt_attn_scoremap_f32(p(d["qkv"]), p(d["pw"]), p(o), R, P, dim, heads, k, p(fbuf) if fneed else None, fneed,
                                             stream()), "scoremap")
        runs = []
        for _ in range(2):
            dqkv = _guarded(R * P, 3 * dim)
            dw = torch.full((heads * k * k + CANARY_ROWS,), float("nan"), device=DEV)
            dw[heads * k * k:] = CANARY
            _lib.check(lib.rrt_attn_scoremap_backward_f32(p(d["qkv"]), p(d["pw"]), p(d["dO"]), p(dqkv), p(dw), R, P, dim, heads, k,
                                                          p(bbuf), bneed, stream()), "scoremap backward")
            runs.append((dqkv, dw))
        torch.cuda.synchronize()
        if not _guard_intact(o, R * P):
            fails.append(f"{cid}: wrote past the end of o")
        for name, buf, need in (("forward", fbuf, fneed), ("backward", bbuf, bneed)):
            if not bool((buf[need:] == CANARY_BYTE).all()):
                fails.append(f"{cid}: the {name} wrote behind its scratch")
        for r, (dqkv, dw) in enumerate(runs):
            if not _guard_intact(dqkv, R * P):
                fails.append(f"{cid}: run {r} wrote past the end of d_qkv")
            if not bool((dw[heads * k * k:] == CANARY).all()):
                fails.append(f"{cid}: run {r} wrote past the end of dW")
        if not (_same_bits(runs[0][0][:R * P], runs[1][0][:R * P]) and _same_bits(runs[0][1][:heads * k * k], runs[1][1][:heads * k * k])):
            fails.append(f"{cid}: the second backward on the same scratch gives other bits")
        g = runs[0][0][:R * P].cpu().numpy()
        got = dict(o=o[:R * P].cpu().numpy(), dq=g[:, :dim], dk=g[:, dim:2 * dim], dv=g[:, 2 * dim:],
                   dw=runs[0][1][:heads * k * k].cpu().numpy().reshape(heads, 1, k, k))
        for what in ("o", "dq", "dk", "dv", "dw"):
            err, e32, bound = judge("B", grp, cid, what, got[what], ref[what], ref32[what], what != "o", fails)
            print(f"{cid:28s} max|S~| {top:5.1f} {what:2s}: {err:.3e}  e32 {e32:.3e}  bound {bound:.2e}")
    assert not fails, f"{len(fails)} failures: " + "; ".join(fails[:12])


# ================================================================== C. the value EPEG
VP_HEADS = ((8, 64), (3, 16), (2, 160), (4, 4))     # dim 512 (two rounds of the c += 256 loops), 48, 320 (not a multiple of 64), 16
VP_SS = (1, 2, 3, 7, 11, 16)
VP_RS = (1, 3)


def vp_kernels(s):
    """(k, two_d); 63 x 63 at s = 2: 3969 taps, the bias slot is thread 129's last of its sixteen"""
    return [(3, False), (9, False), (15, False), (3, True), (5, True)] + ([(63, True)] if s == 2 else [])


VP_CASES = [(heads, hd, s, k, two_d, R, vsub, bias) for heads, hd in VP_HEADS for s in VP_SS for k, two_d in vp_kernels(s)
            for R in VP_RS for vsub in (False, True) for bias in (True, False)]
VP_QMAX, VP_THREADS = 16, 256                      # value_pe_wgrad_kernel: taps t, t + 256, ... per thread, the bias is tap k * kw


def vp_src_col(c, heads, hd):
    """the v column image channel c reads: v.permute(0, 3, 1, 2).reshape(B_, C, s, s) makes c = d * heads + head"""
    return (c % heads) * hd + c // heads


@functools.lru_cache(maxsize=4)
def vp_inputs(heads, hd, s, k, two_d, R):
    dim, P = heads * hd, s * s
    kw = k if two_d else 1
    tag = f"abl/vp/{heads}x{hd}/s{s}/R{R}"
    return dict(qkv=synth.normal(tag + "/qkv", (R * P, 3 * dim)), vsub=synth.normal(tag + "/vsub", (R * P, dim)) * np.float32(0.5),
                dpe=synth.normal(tag + "/dpe", (R * P, dim)), pre=synth.normal(tag + "/pre", (R * P, 3 * dim)),
                w=synth.uniform(f"abl/vp/w/{dim}/{k}x{kw}", (dim, 1, k, kw), -1, 1) * np.float32(1 / np.sqrt(k * kw)),
                b=synth.uniform(f"abl/vp/b/{dim}", (dim,), -0.25, 0.25))


def value_pe_restate(qkv, vsub, w, b, R, s, heads, hd, two_d):
    """rmsa.py:114-118 / :124-129 in qkv's dtype: the v columns (minus vsub) as R images [dim, s, s], depth-wise conv,
    back to rows [R*P, dim] (column c of the result is image channel c for value_bf and value_af alike)"""
    dim, P, k = heads * hd, s * s, w.shape[2]
    v = qkv[:, 2 * dim:]
    if vsub is not None:
        v = v - vsub
    img = v.reshape(R, P, heads, hd).permute(0, 3, 2, 1).reshape(R, dim, s, s)
    pe = F.conv2d(img, w, b, padding=(k // 2, k // 2 if two_d else 0), groups=dim)
    return pe.reshape(R, dim, P).transpose(1, 2).reshape(R * P, dim)


def vp_reference(heads, hd, s, k, two_d, R, vsub, bias, dt):
    """-> dict(pe (without vsub: the forward has none), dv = pre-fill + conv^T(dpe) on the v columns, dw, db)"""
    dim = heads * hd
    a = vp_inputs(heads, hd, s, k, two_d, R)
    ql, wl = _t(a["qkv"], dt, True), _t(a["w"], dt, True)
    bl = _t(a["b"], dt, True) if bias else None
    pe = value_pe_restate(ql, _t(a["vsub"], dt) if vsub else None, wl, bl, R, s, heads, hd, two_d)
    (pe * _t(a["dpe"], dt)).sum().backward()
    g = ql.grad.numpy()
    assert not g[:, :2 * dim].any()
    out = dict(dv=g[:, 2 * dim:], dvsum=_t(a["pre"], dt).numpy()[:, 2 * dim:] + g[:, 2 * dim:], dw=wl.grad.numpy())
    if bias:
        out["db"] = bl.grad.numpy()
    if not vsub:
        out["pe"] = pe.detach().numpy()
    return out


VP_GROUPS = [(heads, hd, s) for heads, hd in VP_HEADS for s in VP_SS]


@pytest.mark.parametrize("heads,hd,s", VP_GROUPS, ids=[f"h{h}x{d}-s{s}" for h, d, s in VP_GROUPS])
def test_value_pe_stage_against_float64(heads, hd, s):
    """pe, the dv added into a pre-filled d_qkv (its q and k columns keep their bits), dW, db of every case at this channel
    layout; two backward runs, same bits"""
    from hip_util import _guard_intact, _guarded, dev, p, stream
    lib = _lib.load()
    fails = []
    dim = heads * hd
    for case in [c for c in VP_CASES if c[:3] == (heads, hd, s)]:
        _, _, _, k, two_d, R, vsub, bias = case
        P, kw = s * s, (k if two_d else 1)
        cid = f"h{heads}x{hd}-s{s}-k{k}{'x' + str(k) if two_d else 'x1'}-R{R}{'-vsub' if vsub else ''}{'-bias' if bias else ''}"
        grp = f"h{heads}x{hd} {'2-D' if two_d else '1-D'}"
        a = vp_inputs(heads, hd, s, k, two_d, R)
        ref, ref32 = vp_reference(*case, torch.float64), vp_reference(*case, torch.float32)
        d = {n: dev(v) for n, v in a.items()}
        bufs = {}
        if not vsub:
            img = a["qkv"][:, 2 * dim:].astype(np.float64).reshape(R, P, heads, hd).transpose(0, 3, 2, 1).reshape(R, dim, s, s)
            pe64 = O._conv_dw64(img, a["w"].astype(np.float64), a["b"].astype(np.float64) if bias else None, two_d)
            assert np.abs(ref["pe"] - pe64.reshape(R, dim, P).transpose(0, 2, 1).reshape(R * P, dim)).max() <= 1e-12, cid
            pe = bufs["pe"] = _guarded(R * P, dim)
            _lib.check(lib.rrt_value_pe_f32(p(d["qkv"]), p(d["w"]), p(d["b"]) if bias else None, p(pe), R, P, s, dim, heads, k,
                                            int(two_d), stream()), "value_pe")
        runs = []
        for _ in range(2):
            dqkv = _guarded(R * P, 3 * dim)
            dqkv[:R * P] = d["pre"]
            dw, db = _guarded(dim, k * kw), (_guarded(1, dim) if bias else None)
            _lib.check(lib.rrt_value_pe_backward_f32(p(d["dpe"]), p(d["qkv"]), p(d["vsub"]) if vsub else None, p(d["w"]), p(dqkv),
                                                     p(dw), p(db), R, P, s, dim, heads, k, int(two_d), stream()), "value_pe backward")
            runs.append((dqkv, dw, db))
        torch.cuda.synchronize()
        if "pe" in bufs and not _guard_intact(bufs["pe"], R * P):
            fails.append(f"{cid}: wrote past the end of pe")
        for r, (dqkv, dw, db) in enumerate(runs):
            broken = [n for n, t, rows in (("d_qkv", dqkv, R * P), ("dW", dw, dim), ("db", db, 1)) if t is not None and not _guard_intact(t, rows)]
            fails += [f"{cid}: run {r} wrote past the end of {n}" for n in broken]
            if not _same_bits(dqkv[:R * P, :2 * dim], d["pre"][:, :2 * dim]):
                fails.append(f"{cid}: run {r} changed the q / k columns of d_qkv")
        same = _same_bits(runs[0][0][:R * P], runs[1][0][:R * P]) and _same_bits(runs[0][1][:dim], runs[1][1][:dim])
        if bias:
            same = same and _same_bits(runs[0][2][:1], runs[1][2][:1])
        if not same:
            fails.append(f"{cid}: the second backward gives other bits")
        dqkv, dw, db = runs[0]
        if "pe" in bufs:
            judge("C", grp, cid, "pe", bufs["pe"][:R * P].cpu().numpy(), ref["pe"], ref32["pe"], False, fails)
        # the sum pre-fill + dv, in units of the largest dv entry (the gradient this stage adds)
        top = float(np.abs(ref["dv"]).max()) or 1.0
        got = dqkv[:R * P, 2 * dim:].cpu().numpy().astype(np.float64)
        e32 = float(np.abs(ref32["dvsum"].astype(np.float64) - ref["dvsum"]).max()) / top
        err = float(np.abs(got - ref["dvsum"]).max()) / top if np.isfinite(got).all() else float("inf")
        RECORDS.append(("C", grp, "dv (added)", e32, err))
        if not err <= max(TOL, E32_FACTOR * e32):
            fails.append(f"{cid} dv: {err:.3e} > {max(TOL, E32_FACTOR * e32):.2e} (e32 {e32:.2e})")
        judge("C", grp, cid, "dw", dw[:dim].cpu().numpy().reshape(dim, 1, k, kw), ref["dw"], ref32["dw"], True, fails)
        if bias:
            judge("C", grp, cid, "db", db[0].cpu().numpy(), ref["db"], ref32["db"], True, fails)
    assert not fails, f"{len(fails)} failures: " + "; ".join(fails[:12])


@pytest.mark.parametrize("heads,hd", VP_HEADS, ids=[f"h{h}x{d}" for h, d in VP_HEADS])
@pytest.mark.parametrize("two_d", (False, True))
def test_value_pe_channel_map(heads, hd, two_d):
    """every v column holds its own index and the conv is the identity tap: pe[:, c] must be (c % heads) * hd + c // heads
    exactly; backwards, d_pe[:, c] = c must land on v column (c % heads) * hd + c // heads of a zero-filled d_qkv"""
    from hip_util import _guard_intact, _guarded, dev, p, stream
    lib = _lib.load()
    dim, s, k, R = heads * hd, 3, 3, 2
    P, kw = s * s, (3 if two_d else 1)
    qkv = np.full((R * P, 3 * dim), -1.0, dtype=np.float32)
    qkv[:, 2 * dim:] = np.arange(dim, dtype=np.float32)
    w = np.zeros((dim, 1, k, kw), dtype=np.float32)
    w[:, 0, k // 2, kw // 2] = 1.0
    src = np.array([vp_src_col(c, heads, hd) for c in range(dim)])
    assert sorted(src) == list(range(dim))
    if heads != hd and heads > 1 and hd > 1:
        assert (src != (np.arange(dim) % hd) * heads + np.arange(dim) // hd).any()      # the pair tells the map from its inverse
    dq, dw_ = dev(qkv), dev(w)
    pe = _guarded(R * P, dim)
    _lib.check(lib.rrt_value_pe_f32(p(dq), p(dw_), None, p(pe), R, P, s, dim, heads, k, int(two_d), stream()), "value_pe")
    dpe = dev(np.tile(np.arange(dim, dtype=np.float32), (R * P, 1)))
    dqkv = _guarded(R * P, 3 * dim)
    dqkv[:R * P] = 0.0
    dwg = _guarded(dim, k * kw)
    _lib.check(lib.rrt_value_pe_backward_f32(p(dpe), p(dq), None, p(dw_), p(dqkv), p(dwg), None, R, P, s, dim, heads, k, int(two_d),
                                             stream()), "value_pe backward")
    torch.cuda.synchronize()
    assert _guard_intact(pe, R * P) and _guard_intact(dqkv, R * P) and _guard_intact(dwg, dim)
    assert np.array_equal(pe[:R * P].cpu().numpy(), np.tile(src.astype(np.float32), (R * P, 1)))
    want = np.zeros((R * P, 3 * dim), dtype=np.float32)
    want[:, 2 * dim + src] = np.arange(dim, dtype=np.float32)
    assert np.array_equal(dqkv[:R * P].cpu().numpy(), want)


# ================================================================== D. the composition in the encoder
ENC_SHAPES = [(200, 7, 128, 4), (500, 11, 128, 4), (200, 7, 512, 8), (500, 11, 512, 8)]      # (N, region_size, dim, heads)
ENC_VARIANTS = {
    "epeg_2d": dict(epeg_k=5, epeg_2d=True),
    "value_bf_1d": dict(epeg_k=9, epeg_type="value_bf"),
    "value_bf_2d": dict(epeg_k=3, epeg_type="value_bf", epeg_2d=True),
    "value_af_1d": dict(epeg_k=9, epeg_type="value_af"),
    "value_af_2d": dict(epeg_k=3, epeg_type="value_af", epeg_2d=True),
}
ENC_CASES = [(v, *s) for v in ENC_VARIANTS for s in ENC_SHAPES]
POS_CASES = {"peg_k11": dict(pos="peg", pos_pos=-1, peg_k=11), "ppeg_k9_1d": dict(pos="ppeg", pos_pos=-1, peg_k=9, peg_1d=True)}
POS_N = 65


def enc_cfg(variant, N, rs, dim, heads):
    return dict(mlp_dim=dim, n_heads=heads, n_layers=2, cr_msa=False, region_size=rs, **ENC_VARIANTS[variant])


def _train_against_eager(grp, tag, N, cfg):
    """one training step of RRTEncoder(**cfg), loss <y, G>, against float64 autograd of O.forward_eager; per tensor the bound
    max(TOL, 8 x e32) of the tensor's own largest entry, e32 from the same eager graph on float32 leaves -> failures"""
    from conftest import STATE_KEYS
    from hip_util import DEV, dev
    from rrt_mil_amd import RRTEncoder
    D = cfg["mlp_dim"]
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k in STATE_KEYS})
    x = synth.bag(N, D, tag="abl/enc/" + tag)
    G = synth.normal("abl/enc/G/" + tag, (N, D))
    refs = []
    for dt in (torch.float64, torch.float32):
        y, xl, params = O.forward_eager(x, st, cfg, grad=True, grad_dtype=dt)
        (y * torch.from_numpy(G).to(dt)).sum().backward()
        refs.append((y.detach().numpy(), xl.grad.numpy(), {m: v.grad.numpy() for m, v in params.items() if v.grad is not None}))
    (y64, dx64, g64), (y32, dx32, g32) = refs
    enc = RRTEncoder(drop_out=0., **cfg)
    enc.load_state_dict({m: torch.from_numpy(v.copy()) for m, v in st.items()}, strict=True)
    enc = enc.to(DEV).train()
    xd = dev(x).requires_grad_(True)
    y = enc(xd.unsqueeze(0)).squeeze(0)
    assert y.grad_fn is not None
    (y * dev(G)).sum().backward()
    torch.cuda.synchronize()
    fails, first = [], len(RECORDS)
    judge("D", grp, tag, "y", y.detach().cpu().numpy(), y64, y32, False, fails)
    judge("D", grp, tag, "dx", xd.grad.cpu().numpy(), dx64, dx32, True, fails)
    for name, prm in enc.named_parameters():
        assert prm.grad is not None, name
        if name.endswith("pe.bias") and cfg.get("epeg_type", "attn") == "attn":
            # the conv bias is a per-head constant on every score: it cancels in the softmax
            assert float(prm.grad.abs().max()) == 0.0 and np.abs(g64[name]).max() < 1e-9, name
            continue
        short = name.replace("layers.0.attn.attn.", "").replace("pos_embedding.", "pos.").replace("cr_msa.attn.attn.", "cr.").replace("cr_msa.", "cr.")
        judge("D", grp, tag, short, prm.grad.cpu().numpy(), g64[name].reshape(prm.shape), g32[name].reshape(prm.shape), True, fails)
    print("\n".join(f"{tag} {what}: {err:.3e} (e32 {e32:.2e})" for _, g, what, e32, err in RECORDS[first:]))
    return fails


@pytest.mark.parametrize("variant,N,rs,dim,heads", ENC_CASES, ids=[f"{c[0]}-N{c[1]}-rs{c[2]}-d{c[3]}h{c[4]}" for c in ENC_CASES])
def test_epeg_variants_in_the_encoder(variant, N, rs, dim, heads):
    """one R-MSA layer + the final LayerNorm; regions of rs x rs tokens that hold pads"""
    H, s, add = O.grid(N, 8, rs, 0, 0.0)
    assert s == rs and add > 0
    fails = _train_against_eager(variant, f"{variant} N{N} rs{rs} d{dim}", N, enc_cfg(variant, N, rs, dim, heads))
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("case", list(POS_CASES))
def test_peg_largest_kernels_in_the_encoder(case):
    """pos='peg' peg_k=11 (the backward's largest LDS request) and pos='ppeg' peg_k=9 (k, 1) in front of CR-MSA, N = 65"""
    fails = _train_against_eager(f"{case} N{POS_N}", f"{case} N{POS_N}", POS_N, dict(mlp_dim=512, n_layers=1, crmsa_k=3, **POS_CASES[case]))
    assert not fails, "; ".join(fails)
