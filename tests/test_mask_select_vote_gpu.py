"""GPU (-m gpu): multi-head vote fusion on the device (rrt_mask_select_vote_f32, csrc/mask_select.hip) against the restatement
tests/mhim_sattn_ref.py -- EXACT integer equality of ids, count and mask.  Sizes on both sides of every boundary of the kernels
(the wave, the 256-token block, the 1024-key LDS fill, several chunks of the j range), 1 to 16 heads, per-head rows with ties,
+-0, +-inf and NaN (tests/mhim_cases.py patterns, one row per head) and three arrangements of heads: all the same row (votes in
{0, heads}), alternating negated rows, all values equal (the first k indices win in every head).

Every output is -1 / 0xEE filled with canaries behind it, the workspace has exactly the queried size with canary bytes behind
it, every call runs twice on differently dirtied workspaces and must give the same bits; nothing more runs after a device error.
Importing this module needs no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import mhim_cases as MC
import mhim_ref as MR
import mhim_sattn_cases as SC
import mhim_sattn_ref as R
from rrt_mil_amd import _lib
from test_mask_select_gpu import Out, Ws, run_select

pytestmark = pytest.mark.gpu
# (arrangement, pattern): every pattern with one row per head, then the three arrangements of heads
ROW_SETS = [("tagged", p) for p in MC.PATTERNS] + [("same", "levels5"), ("negated", "distinct"), ("all_equal", "equal")]


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


def run_vote(a_dev, n, heads, stages, invert, want_mask=True, fill=0xA5):
    """one rrt_mask_select_vote_f32 call on the current stream -> (ids, count, mask) as numpy; stages = [(largest, k, pick|None)]"""
    lib = _lib.load()
    arr = (_lib.MaskStage * len(stages))()
    picks = []
    for s, (largest, k, pick) in zip(arr, stages):
        s.largest, s.k = int(largest), int(k)
        if pick is not None:
            picks.append(torch.from_numpy(np.asarray(pick, np.uint8)).cuda())      # exactly k bytes
            s.pick = picks[-1].data_ptr()
    need = C.c_size_t()
    _lib.check(lib.rrt_mask_select_vote_workspace_size(n, heads, len(stages), C.byref(need)), "rrt_mask_select_vote_workspace_size")
    ws = Ws(need.value, fill)
    ids, count, mask = Out(n, torch.int64, -1), Out(1, torch.int64, -1), Out(n, torch.uint8, 0xEE)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.rrt_mask_select_vote_f32(a_dev.data_ptr(), n, heads, arr, len(stages), int(invert), ids.ptr(), count.ptr(),
                                            mask.ptr() if want_mask else None, ws.ptr(), ws.n, st), "rrt_mask_select_vote_f32")
    torch.cuda.current_stream().synchronize()
    for o in (ids, count, mask, ws):
        o.check("rrt_mask_select_vote_f32")
    if not want_mask:
        assert bool((mask.t == 0xEE).all()), "wrote a mask nobody asked for"
    return ids.t[:, 0].cpu().numpy(), int(count.t[0, 0]), mask.t[:, 0].cpu().numpy()


@pytest.mark.parametrize("heads", SC.VOTE_HEADS)
@pytest.mark.parametrize("n", MC.SELECT_NS)
def test_vote_fusion_is_the_restatement(n, heads):
    for arrangement, pattern in ROW_SETS:
        a = SC.head_rows(arrangement, pattern, n, heads)
        assert a.shape == (heads, n) and a.dtype == np.float32
        a_dev = torch.from_numpy(a).cuda()
        cache = R.orders(a)                                     # the per-head orders do not depend on the stage
        for j, (spec, invert) in enumerate(MC.select_settings(n)):
            tag = f"{arrangement}/{pattern}/{n}/{heads}/{j}"
            stages = [(largest, k, MC.pick(kind, k, f"vote/{tag}/{s}")) for s, (largest, k, kind) in enumerate(spec)]
            ref_ids, ref_count, ref_mask = R.select_vote(a, stages, invert, cache)
            for fill in (0xA5, 0x3C):                           # two workspace contents: nothing is read before it is written
                ids, count, mask = run_vote(a_dev, n, heads, stages, invert, fill=fill)
                assert count == ref_count, (tag, spec, invert, count, ref_count)
                assert np.array_equal(ids, ref_ids) and np.array_equal(mask, ref_mask), (tag, spec, invert)


@pytest.mark.parametrize("n", MC.SELECT_NS)
def test_one_head_without_pick_is_the_single_head_entry(n):
    """heads = 1, pick = NULL: a vote of 1 for the head's first k, so the fused set is the head's own -- rrt_mask_select_f32's
    ids, count and mask bit for bit"""
    for pattern in MC.PATTERNS:
        a = MC.scores(pattern, n)
        a_dev = torch.from_numpy(a).cuda()
        k3 = max(1, n // 3)
        for stages, invert in (([(False, k3, None)], False), ([(True, k3, None), (False, 1, None)], True),
                               ([(False, n, None)], False), ([(True, 1, None), (False, k3, None), (True, k3, None)], False)):
            one = run_select(a_dev, n, stages, invert)
            vote = run_vote(a_dev.reshape(1, n), n, 1, stages, invert)
            assert one[1] == vote[1] and np.array_equal(one[0], vote[0]) and np.array_equal(one[2], vote[2]), (pattern, n, stages)


def test_all_equal_rows_take_the_first_k():
    n, heads, k = 1025, 3, 300
    a = SC.head_rows("all_equal", "equal", n, heads)
    ids, count, mask = run_vote(torch.from_numpy(a).cuda(), n, heads, [(True, k, None)], True)
    assert count == k and np.array_equal(ids, np.arange(n)) and np.array_equal(mask, (np.arange(n) >= k).astype(np.uint8))


def test_vote_without_a_mask_and_on_another_stream():
    n, heads = 4099, 8
    a = SC.head_rows("tagged", "levels5", n, heads)
    a_dev = torch.from_numpy(a).cuda()
    spec, invert = MC.select_settings(n)[5]
    stages = [(largest, k, MC.pick(kind, k, f"vote/stream/{j}")) for j, (largest, k, kind) in enumerate(spec)]
    ref_ids, ref_count, _ = R.select_vote(a, stages, invert)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ids, count, _ = run_vote(a_dev, n, heads, stages, invert, want_mask=False)
    assert count == ref_count and np.array_equal(ids, ref_ids)


def test_vote_the_largest_bag():
    """n = 262144, the entry's limit, two heads: one chunk per head, 1024 blocks, every histogram through the one-block scans"""
    n, heads = _lib.MASK_SELECT_MAX_N, 2
    a = SC.head_rows("tagged", "levels5", n, heads)
    stages = [(False, n // 3, None), (True, n // 5, MC.pick("sparse", n // 5, "vote/largest"))]
    ref_ids, ref_count, ref_mask = R.select_vote(a, stages, False)
    ids, count, mask = run_vote(torch.from_numpy(a).cuda(), n, heads, stages, False)
    assert count == ref_count and np.array_equal(ids, ref_ids) and np.array_equal(mask, ref_mask)


def test_python_wrapper():
    from rrt_mil_amd import mhim_sattn
    n, heads = 257, 2
    a = SC.head_rows("tagged", "distinct", n, heads)
    pick = MC.pick("sparse", 100, "vote/wrapper")
    ids, count, mask = mhim_sattn.mask_select_vote(torch.from_numpy(a).cuda(), [(True, 100, torch.from_numpy(pick).cuda()), (False, 20, None)],
                                                   invert=False, return_mask=True)
    ref_ids, ref_count, ref_mask = R.select_vote(a, [(True, 100, pick), (False, 20, None)], False)
    assert int(count.item()) == ref_count and np.array_equal(ids.cpu().numpy(), ref_ids) and np.array_equal(mask.cpu().numpy(), ref_mask)
    ids2, count2 = mhim_sattn.mask_select_vote(torch.from_numpy(a[:1]).cuda(), [(True, 100, None)], invert=True)
    ref = MR.select(a[0], [(True, 100, None)], True)
    assert int(count2.item()) == ref[1] == 100 and np.array_equal(ids2.cpu().numpy(), ref[0])
