"""GPU (-m gpu): the mask selection kernels of csrc/mask_select.hip (rrt_mask_select_f32) and the row gather / scatter
(rrt_gather_rows_f32, rrt_scatter_rows_f32) against the restatement tests/mhim_ref.py -- EXACT integer equality of ids, count
and mask; bit equality of moved rows.  Sizes on both sides of every boundary of the kernels (the wave, the 256-token block,
the 1024-key LDS fill, several chunks of the j range), value patterns with ties, +-0, +-inf and NaN (tests/mhim_cases.py).

Every output is -1 / 0xEE / NaN filled with canaries behind it, the workspace has exactly the queried size with canary bytes
behind it, every call runs twice and must give the same bits, one case runs on a non-default stream; nothing more runs after a
device error.  Importing this module needs no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import mhim_cases as MC
import mhim_ref as R
from rrt_mil_amd import _lib

pytestmark = pytest.mark.gpu
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
    """an output of n entries of `dtype`, filled with `fill`, with 64 canary entries behind it"""

    def __init__(self, n, dtype, fill, row=1):
        self.n, canary = n, (CANARY if dtype.is_floating_point else 77)
        self.buf = torch.full((n + 64, row), fill, dtype=dtype, device="cuda")
        self.buf[n:] = canary
        self.canary = canary

    @property
    def t(self):
        return self.buf[:self.n]

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.n:] == self.canary).all()), f"{what}: wrote behind its output"


class Ws:
    """a workspace of exactly `nbytes` bytes, dirtied, with 256 canary bytes behind it"""

    def __init__(self, nbytes, fill=0xA5):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 256,), fill, dtype=torch.uint8, device="cuda")
        self.buf[self.n:] = 0x5C

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.n:] == 0x5C).all()), f"{what}: wrote behind its workspace"


def run_select(a_dev, n, stages, invert, want_mask=True, fill=0xA5):
    """one rrt_mask_select_f32 call on the current stream -> (ids, count, mask) as numpy; stages = [(largest, k, pick array|None)]"""
    lib = _lib.load()
    arr = (_lib.MaskStage * len(stages))()
    picks = []
    for s, (largest, k, pick) in zip(arr, stages):
        s.largest, s.k = int(largest), int(k)
        if pick is not None:
            # the pick array has exactly k bytes; a canary row behind it would be read only by an out-of-range rank
            picks.append(torch.from_numpy(np.asarray(pick, np.uint8)).cuda())
            s.pick = picks[-1].data_ptr()
    need = C.c_size_t()
    _lib.check(lib.rrt_mask_select_workspace_size(n, len(stages), C.byref(need)), "rrt_mask_select_workspace_size")
    ws = Ws(need.value, fill)
    ids, count, mask = Out(n, torch.int64, -1), Out(1, torch.int64, -1), Out(n, torch.uint8, 0xEE)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.rrt_mask_select_f32(a_dev.data_ptr(), n, arr, len(stages), int(invert), ids.ptr(), count.ptr(),
                                       mask.ptr() if want_mask else None, ws.ptr(), ws.n, st), "rrt_mask_select_f32")
    torch.cuda.current_stream().synchronize()
    for o in (ids, count, mask, ws):
        o.check("rrt_mask_select_f32")
    if not want_mask:
        assert bool((mask.t == 0xEE).all()), "wrote a mask nobody asked for"
    return ids.t[:, 0].cpu().numpy(), int(count.t[0, 0]), mask.t[:, 0].cpu().numpy()


def check_setting(a, a_dev, n, setting, tag):
    spec, invert = setting
    stages = [(largest, k, MC.pick(kind, k, f"{tag}/{j}")) for j, (largest, k, kind) in enumerate(spec)]
    ref_ids, ref_count, ref_mask = R.select(a, stages, invert)
    first = run_select(a_dev, n, stages, invert, fill=0xA5)
    again = run_select(a_dev, n, stages, invert, fill=0x3C)        # another workspace content: nothing is read before written
    for got in (first, again):
        assert got[1] == ref_count, (tag, spec, invert, got[1], ref_count)
        assert np.array_equal(got[0], ref_ids), (tag, spec, invert)
        assert np.array_equal(got[2], ref_mask), (tag, spec, invert)
    return stages, invert


@pytest.mark.parametrize("pattern", MC.PATTERNS)
@pytest.mark.parametrize("n", MC.SELECT_NS)
def test_mask_select_is_the_stable_sort(n, pattern):
    a = MC.scores(pattern, n)
    a_dev = torch.from_numpy(a).cuda()
    for j, setting in enumerate(MC.select_settings(n)):
        check_setting(a, a_dev, n, setting, f"{pattern}/{n}/{j}")


def test_mask_select_without_a_mask_and_on_another_stream():
    n = 4099
    a = MC.scores("levels5", n)
    a_dev = torch.from_numpy(a).cuda()
    spec, invert = MC.select_settings(n)[5]
    stages = [(largest, k, MC.pick(kind, k, f"stream/{j}")) for j, (largest, k, kind) in enumerate(spec)]
    ref_ids, ref_count, _ = R.select(a, stages, invert)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ids, count, _ = run_select(a_dev, n, stages, invert, want_mask=False)
    assert count == ref_count and np.array_equal(ids, ref_ids)


def test_mask_select_the_largest_bag():
    """n = 262144, the entry's limit: one chunk, 1024 blocks, every block count through the one-block scan"""
    n = _lib.MASK_SELECT_MAX_N
    a = MC.scores("levels5", n)
    a_dev = torch.from_numpy(a).cuda()
    stages = [(False, n // 3, None), (True, n // 5, MC.pick("sparse", n // 5, "largest"))]
    ref_ids, ref_count, ref_mask = R.select(a, stages, False)
    ids, count, mask = run_select(a_dev, n, stages, False)
    assert count == ref_count and np.array_equal(ids, ref_ids) and np.array_equal(mask, ref_mask)


# ---------------------------------------------------------------------- rows by index
def rows_case(n_rows, dim):
    n_src = n_rows + 37
    src = torch.from_numpy(np.arange(n_src * dim, dtype=np.float32).reshape(n_src, dim) % 8191 + 1).cuda()
    g = torch.Generator().manual_seed(n_rows * 131 + dim)
    ids = torch.randperm(n_src, generator=g)[:n_rows].to(torch.int64)
    return src, ids, n_src


@pytest.mark.parametrize("dim", MC.ROW_DIMS)
@pytest.mark.parametrize("n_rows", MC.ROW_NS)
def test_gather_scatter_rows(n_rows, dim):
    lib = _lib.load()
    src, ids, n_src = rows_case(n_rows, dim)
    bad = ids.clone()
    where = [0, n_rows // 2, n_rows - 1]
    for w, v in zip(sorted(set(where)), (-1, n_src, 1 << 40)):       # three kinds of out-of-range id (n_rows = 1: the first)
        bad[w] = v
    st = torch.cuda.current_stream().cuda_stream
    for id_host in (ids, bad):
        id_dev = id_host.cuda()
        ok = ((id_host >= 0) & (id_host < n_src))
        outs = []
        for _ in range(2):
            dst = Out(n_rows, torch.float32, CANARY * 2, row=dim)
            _lib.check(lib.rrt_gather_rows_f32(src.data_ptr(), id_dev.data_ptr(), dst.ptr(), n_rows, n_src, dim, st), "rrt_gather_rows_f32")
            torch.cuda.synchronize()
            dst.check("rrt_gather_rows_f32")
            outs.append(dst.t.clone())
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        got = outs[0].cpu()
        assert torch.equal(got[ok], src.cpu()[id_host[ok]]), "a gathered row differs"
        assert bool(torch.isnan(got[~ok]).all()), "an out-of-range id did not give a NaN row"
        # the adjoint: the rows go back where they came from, zeros elsewhere, out-of-range ids skipped
        rows = torch.where(torch.isnan(outs[0]), torch.full_like(outs[0], 5.0), outs[0])
        back = Out(n_src, torch.float32, float("nan"), row=dim)
        _lib.check(lib.rrt_scatter_rows_f32(rows.data_ptr(), id_dev.data_ptr(), back.ptr(), n_rows, n_src, dim, st), "rrt_scatter_rows_f32")
        torch.cuda.synchronize()
        back.check("rrt_scatter_rows_f32")
        want = torch.zeros(n_src, dim)
        want[id_host[ok]] = src.cpu()[id_host[ok]]
        assert torch.equal(back.t.cpu(), want), "scatter of gather is not the identity on the kept rows and zero elsewhere"


def test_gather_rows_of_a_selection():
    """ids straight from rrt_mask_select_f32, count rows of them: what the masked student does"""
    n, dim = 1025, 64
    a = MC.scores("distinct", n)
    stages = [(False, n, MC.pick("sparse", n, "gather")), (True, n // 3, None)]
    ids, count, _ = run_select(torch.from_numpy(a).cuda(), n, stages, False)
    ref_ids, ref_count, _ = R.select(a, stages, False)
    assert count == ref_count and 0 < count < n
    from rrt_mil_amd import mhim
    x = torch.from_numpy(np.arange(n * dim, dtype=np.float32).reshape(n, dim)).cuda()
    got = mhim.gather_rows(x, torch.from_numpy(ids).cuda(), count)
    assert torch.equal(got.cpu(), x.cpu()[torch.from_numpy(ref_ids[:count])])
