"""GPU (-m gpu): the stage entries of DTFD-MIL's first tier (csrc/segment_pool.hip: rrt_gate_scores_f32,
rrt_segment_pool_f32, rrt_segment_pool_backward_f32) against the float64 restatement tests/dtfd_ref.py -- never against another
kernel, except the scores, which must equal rrt_attn_pool_f32's a_raw bit for bit.

pooled, attn, p and the backward's d_a: the project's value rule, err <= max(2e-5, 8 x e32) relative to
max(1, max |float64 reference|), e32 = the error of the same restatement evaluated in fp32 numpy.  d_mid: the gradient rule,
within 1e-3 of the tensor's own largest entry.  sel: EXACT -- the argmax / argmin, lowest position first, of the kernel's OWN
p output, for every group.  Group sizes on both sides of the chunk of 32 positions (1, 2, 31, 32, 33, 64, 65, mixed q / q + 1),
every dim / class count / permutation / score pattern of tests/dtfd_cases.py, exact ties, NaN rows and an all-NaN group.

Every output is NaN / -1 filled with canaries behind it, the workspace has exactly the queried size with canary bytes behind
it, every call runs twice on differently dirtied workspaces and must give the same bits; nothing more runs after a device
error.  Importing this module needs no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import dtfd_cases as DC
import dtfd_ref as R
from rrt_mil_amd import _lib, synth

pytestmark = pytest.mark.gpu
TOL, E32_FACTOR, GRAD_TOL = 2e-5, 8.0, 1e-3
CANARY = 1234.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """a device error is sticky: nothing more is started on a device that reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is run on it: {e}", returncode=3)


class Out:
    """an output of `shape`, filled with NaN / -1, with 64 canary entries behind it"""

    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.n = shape, int(np.prod(shape))
        self.canary = CANARY if dtype.is_floating_point else 77
        self.fill = float("nan") if dtype.is_floating_point else -1
        self.buf = torch.full((self.n + 64,), self.fill, dtype=dtype, device="cuda")
        self.buf[self.n:] = self.canary

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.n:] == self.canary).all()), f"{what}: wrote behind its output"

    def np(self):
        return self.buf[:self.n].reshape(self.shape).cpu().numpy()

    def untouched(self):
        t = self.buf[:self.n]
        return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == -1).all())


class Ws:
    """a workspace of exactly `nbytes` bytes, dirtied, with 256 canary bytes behind it"""

    def __init__(self, nbytes, fill):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 256,), fill, dtype=torch.uint8, device="cuda")
        self.buf[self.n:] = 0x5C

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.n:] == 0x5C).all()), f"{what}: wrote behind its workspace"


def dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def run_pool(mid, a, perm, cls_w, g, d_pooled=None, fill=0xA5):
    """one forward (and, with d_pooled, one backward on the workspace the forward left) -> dict of numpy arrays"""
    lib = _lib.load()
    (n, dim), c = mid.shape, cls_w.shape[0]
    t_mid, t_a, t_perm, t_w = dev(mid), dev(a), dev(perm, torch.int64), dev(cls_w)
    need = C.c_size_t()
    _lib.check(lib.rrt_segment_pool_workspace_size(n, dim, c, g, C.byref(need)), "rrt_segment_pool_workspace_size")
    ws = Ws(need.value, fill)
    pooled, sel, attn, p = Out((g, dim)), Out((g, 2), torch.int64), Out((n,)), Out((n,))
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.rrt_segment_pool_f32(ptr(t_mid), ptr(t_a), ptr(t_perm), ptr(t_w), pooled.ptr(), sel.ptr(), attn.ptr(), p.ptr(),
                                        n, dim, c, g, ws.ptr(), ws.n, st), "rrt_segment_pool_f32")
    torch.cuda.synchronize()
    for o in (pooled, sel, attn, p, ws):
        o.check("rrt_segment_pool_f32")
    out = dict(pooled=pooled.np(), sel=sel.np(), attn=attn.np(), p=p.np())
    if d_pooled is not None:
        t_dp, t_pooled = dev(d_pooled), dev(out["pooled"])
        d_mid, d_a = Out((n, dim)), Out((n,))
        _lib.check(lib.rrt_segment_pool_backward_f32(ptr(t_mid), ptr(t_a), ptr(t_perm), ptr(t_pooled), ptr(t_dp), d_mid.ptr(),
                                                     d_a.ptr(), n, dim, g, ws.ptr(), ws.n, st), "rrt_segment_pool_backward_f32")
        torch.cuda.synchronize()
        for o in (d_mid, d_a, ws):
            o.check("rrt_segment_pool_backward_f32")
        out.update(d_mid=d_mid.np(), d_a=d_a.np())
    return out


def same_bits(x, y):
    return all(np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)) for k in x)


def judge(tag, what, got, ref64, ref32, fails):
    e32 = R.rel_err(ref32, ref64)
    err = R.rel_err(got, ref64)
    bound = max(TOL, E32_FACTOR * e32)
    print(f"{tag} {what}: err {err:.3e} e32 {e32:.2e} bound {bound:.2e}")
    if not err <= bound:
        fails.append(f"{tag} {what}: {err:.3e} > {bound:.2e} (e32 {e32:.2e})")


def check_case(tag, mid, a, perm, cls_w, g, backward=True):
    n, dim = mid.shape
    d_pooled = synth.normal(f"dtfd/stage/dp/{g}x{dim}", (g, dim)) if backward else None
    got = run_pool(mid, a, perm, cls_w, g, d_pooled, fill=0xA5)
    again = run_pool(mid, a, perm, cls_w, g, d_pooled, fill=0x3C)      # another workspace content: nothing is read before written
    assert same_bits(got, again), f"{tag}: two runs differ"
    r64, r32 = R.segment_pool(mid, a, perm, cls_w, g), R.segment_pool(mid, a, perm, cls_w, g, dtype=np.float32)
    fails = []
    for q in ("pooled", "attn", "p"):
        judge(tag, q, got[q], r64[q], r32[q], fails)
    # the selection: exact, from the kernel's own p, every group
    want = R.select_from_p(got["p"], perm, g)
    assert np.array_equal(got["sel"], want), (tag, got["sel"].tolist(), want.tolist())
    if backward:
        dm64, da64 = R.segment_pool_backward(mid, a, perm, d_pooled, g)
        _, da32 = R.segment_pool_backward(mid, a, perm, d_pooled, g, dtype=np.float32)
        judge(tag, "d_a", got["d_a"], da64, da32, fails)
        top = float(np.abs(dm64).max())
        err = float(np.abs(got["d_mid"].astype(np.float64) - dm64).max()) / top
        print(f"{tag} d_mid: err {err:.3e} of max {top:.3e}")
        if not (np.isfinite(got["d_mid"]).all() and err <= GRAD_TOL):
            fails.append(f"{tag} d_mid: {err:.3e} > {GRAD_TOL}")
    assert not fails, "\n".join(fails)
    return got


@pytest.mark.parametrize("n,g", DC.STAGE_SHAPES)
def test_group_sizes_around_the_chunk(n, g):
    sizes = R.split_sizes(n, g)
    assert sum(sizes) == n and min(sizes) >= 1
    for j, kind in enumerate(DC.PERMS):                  # every permutation kind at the small shapes, one of them at 4099
        if n > 1000 and j != (g % 3):
            continue
        check_case(f"n{n}_g{g}_{kind}", DC.stage_mid(n, 512), DC.stage_scores("mild", n), DC.stage_perm(kind, n),
                   DC.stage_cls_w(2, 512), g)


def test_the_shapes_cover_the_chunk_edges():
    seen = {s for n, g in DC.STAGE_SHAPES for s in R.split_sizes(n, g)}
    assert {1, 2, 31, 32, 33, 64, 65} <= seen
    assert any(n % g and n > g for n, g in DC.STAGE_SHAPES) and (4099, 64) in DC.STAGE_SHAPES


@pytest.mark.parametrize("dim", DC.STAGE_DIMS)
@pytest.mark.parametrize("c", DC.STAGE_CLASSES)
def test_dims_and_class_counts(dim, c):
    n, g = 259, 8
    got = check_case(f"d{dim}_c{c}", DC.stage_mid(n, dim), DC.stage_scores("mild", n), DC.stage_perm("shuffle", n),
                     DC.stage_cls_w(c, dim), g)
    if c == 1:          # one class: every p is exactly 1, every group selects its first position at both ends
        perm = DC.stage_perm("shuffle", n)
        assert np.all(got["p"] == 1.0)
        firsts = np.array([perm[s] for s, _ in R.group_positions(n, g)])
        assert np.array_equal(got["sel"], np.stack([firsts, firsts], 1))


def test_widest_row_most_classes_most_groups():
    n, g, dim, c = 4099, 64, 2048, 8
    check_case("wide", DC.stage_mid(n, dim), DC.stage_scores("peaked", n), DC.stage_perm("shuffle", n), DC.stage_cls_w(c, dim), g)


@pytest.mark.parametrize("pattern", DC.SCORE_PATTERNS)
@pytest.mark.parametrize("kind", DC.PERMS)
def test_score_patterns_and_permutations(pattern, kind):
    n, g = 259, 8
    check_case(f"{pattern}_{kind}", DC.stage_mid(n, 512), DC.stage_scores(pattern, n), DC.stage_perm(kind, n), DC.stage_cls_w(4, 512), g)


@pytest.mark.parametrize("kind", DC.PERMS)
def test_exactly_tied_rows_select_the_lower_position(kind):
    """duplicated rows with equal scores inside one group: their p are the same bits, the lower position must win"""
    n, g = 130, 2
    mid, a = DC.stage_mid(n, 512).copy(), DC.stage_scores("mild", n).copy()
    perm = DC.stage_perm(kind, n)
    order = np.arange(n) if perm is None else perm
    for s, sz in R.group_positions(n, g):
        rows = order[s:s + sz]
        mid[rows] = mid[rows[0]]                      # the whole group is one row, one score
        a[rows] = a[rows[0]]
    got = check_case(f"tied_{kind}", mid, a, perm, DC.stage_cls_w(2, 512), g)
    for k, (s, sz) in enumerate(R.group_positions(n, g)):
        assert np.unique(got["p"][order[s:s + sz]]).size == 1
        assert got["sel"][k].tolist() == [order[s], order[s]]
    # two pairs of twins in a group of distinct rows: whichever pair holds an extreme, its lower position is selected
    mid, a = DC.stage_mid(n, 512).copy(), DC.stage_scores("flat", n)
    p0 = run_pool(mid, a, perm, DC.stage_cls_w(2, 512), g)["p"]
    for s, sz in R.group_positions(n, g):
        rows = order[s:s + sz]
        head = rows[:-2]                                  # (flat scores: a row's p depends on that row alone)
        hi, lo = head[np.argmax(p0[head])], head[np.argmin(p0[head])]
        mid[rows[-1]], mid[rows[-2]] = mid[hi], mid[lo]          # twins of both extremes at the group's end
    got = check_case(f"twins_{kind}", mid, a, perm, DC.stage_cls_w(2, 512), g)
    for k, (s, sz) in enumerate(R.group_positions(n, g)):
        rows = order[s:s + sz]
        assert got["sel"][k, 0] not in (rows[-1], rows[-2]) and got["sel"][k, 1] not in (rows[-1], rows[-2])


def test_nan_rows_are_never_selected_and_an_all_nan_group_selects_its_first_member():
    n, g = 259, 8
    perm = DC.stage_perm("shuffle", n)
    groups = R.group_positions(n, g)
    mid, a = DC.stage_mid(n, 512).copy(), DC.stage_scores("mild", n).copy()
    bad = perm[groups[2][0] + 5]
    mid[bad] = np.nan                                 # one NaN row with a finite score: its p is NaN, its group's pooled row too
    rows5 = perm[groups[5][0]:groups[5][0] + groups[5][1]]
    a[rows5] = np.nan                                 # a group whose every score is NaN
    got = check_case("nan", mid, a, perm, DC.stage_cls_w(4, 512), g, backward=False)
    assert np.isnan(got["p"][bad]) and bad not in got["sel"][2] and np.isnan(got["pooled"][2]).all()
    assert np.isnan(got["p"][rows5]).all() and got["sel"][5].tolist() == [rows5[0], rows5[0]] and np.isnan(got["pooled"][5]).all()
    others = [k for k in range(g) if k not in (2, 5)]
    assert np.isfinite(got["pooled"][others]).all()


@pytest.mark.parametrize("n", [1, 33, 4099])
@pytest.mark.parametrize("hidden,gated,bias", [(4, False, False), (128, True, True), (384, True, False), (260, False, True)])
def test_gate_scores_are_the_attention_pools_raw_scores_bit_for_bit(n, hidden, gated, bias):
    lib = _lib.load()
    dim = 64
    hid_a = dev(np.tanh(synth.normal(f"dtfd/gs/a/{n}x{hidden}", (n, hidden))))
    hid_b = dev(synth.uniform(f"dtfd/gs/b/{n}x{hidden}", (n, hidden), 0.0, 1.0)) if gated else None
    c_w, c_b = dev(synth.normal(f"dtfd/gs/w/{hidden}", (hidden,))), (dev(np.array([0.37], np.float32)) if bias else None)
    y = dev(synth.normal(f"dtfd/gs/y/{n}", (n, dim)))
    st = torch.cuda.current_stream().cuda_stream
    a = Out((n,))
    _lib.check(lib.rrt_gate_scores_f32(ptr(hid_a), ptr(hid_b), ptr(c_w), ptr(c_b), a.ptr(), n, hidden, st), "rrt_gate_scores_f32")
    need = C.c_size_t()
    _lib.check(lib.rrt_attn_pool_workspace_size(n, dim, hidden, C.byref(need)), "rrt_attn_pool_workspace_size")
    ws = Ws(need.value, 0xA5)
    pooled, attn, a_raw = Out((dim,)), Out((n,)), Out((n,))
    _lib.check(lib.rrt_attn_pool_f32(ptr(y), ptr(hid_a), ptr(hid_b), ptr(c_w), ptr(c_b), pooled.ptr(), attn.ptr(), a_raw.ptr(), n,
                                     dim, hidden, ws.ptr(), ws.n, st), "rrt_attn_pool_f32")
    torch.cuda.synchronize()
    a.check("rrt_gate_scores_f32")
    assert np.array_equal(a.np().view(np.uint32), a_raw.np().view(np.uint32))
    ref = R.gate_scores(hid_a.cpu().numpy(), None if hid_b is None else hid_b.cpu().numpy(), c_w.cpu().numpy(), 0.37 if bias else None)
    ref32 = R.gate_scores(hid_a.cpu().numpy(), None if hid_b is None else hid_b.cpu().numpy(), c_w.cpu().numpy(),
                          0.37 if bias else None, dtype=np.float32)
    fails = []
    judge(f"scores n{n} h{hidden}", "a", a.np(), ref, ref32, fails)
    assert not fails, fails


def test_refusals_launch_nothing():
    lib = _lib.load()
    n, dim, c, g = 100, 512, 2, 8
    t_mid, t_a, t_w = dev(DC.stage_mid(n, dim)), dev(DC.stage_scores("mild", n)), dev(DC.stage_cls_w(c, dim))
    need = C.c_size_t()
    _lib.check(lib.rrt_segment_pool_workspace_size(n, dim, c, g, C.byref(need)), "rrt_segment_pool_workspace_size")
    ws = Ws(need.value, 0xA5)
    st = torch.cuda.current_stream().cuda_stream
    outs = pooled, sel, attn, p = Out((g, dim)), Out((g, 2), torch.int64), Out((n,)), Out((n,))
    call = lambda n_=n, dim_=dim, c_=c, g_=g, bytes_=ws.n, mid_=t_mid: lib.rrt_segment_pool_f32(   # noqa: E731
        ptr(mid_), ptr(t_a), None, ptr(t_w), pooled.ptr(), sel.ptr(), attn.ptr(), p.ptr(), n_, dim_, c_, g_, ws.ptr(), bytes_, st)
    assert call(n_=7) == -2 and b"n_tokens < n_groups" in lib.rrt_strerror(-2)
    assert call(dim_=48) == -2 and call(dim_=2080) == -2 and call(c_=9) == -2 and call(c_=0) == -1 and call(g_=65) == -2
    assert call(g_=0) == -1 and call(n_=0) == -1 and call(n_=1000001) == -2 and call(bytes_=ws.n - 1) == -3
    assert call(mid_=None) == -1
    d_mid, d_a = Out((n, dim)), Out((n,))
    back = lambda n_=n, dim_=dim, g_=g, bytes_=ws.n: lib.rrt_segment_pool_backward_f32(   # noqa: E731
        ptr(t_mid), ptr(t_a), None, ptr(t_mid), ptr(t_mid), d_mid.ptr(), d_a.ptr(), n_, dim_, g_, ws.ptr(), bytes_, st)
    assert back(n_=7) == -2 and back(dim_=48) == -2 and back(g_=65) == -2 and back(bytes_=16) == -3 and back(n_=0) == -1
    a = Out((n,))
    assert lib.rrt_gate_scores_f32(ptr(t_mid), None, ptr(t_w), None, a.ptr(), n, 126, st) == -2
    assert lib.rrt_gate_scores_f32(None, None, ptr(t_w), None, a.ptr(), n, 128, st) == -1
    torch.cuda.synchronize()
    for o in outs + (d_mid, d_a, a):
        assert o.untouched(), "a refused call wrote an output"
        o.check("refusal")
    assert bool((ws.buf[:ws.n] == 0xA5).all()), "a refused call wrote its workspace"
