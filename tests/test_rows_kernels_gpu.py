"""GPU (-m gpu): the row-looping forms of LayerNorm + partition and of dispatch + residual + final LayerNorm
(ln_partition_rows_kernel, crmsa_dispatch_ln_rows_kernel) against the one-wave-per-row kernels of the same build, bit for bit
(torch.equal on the raw float32 / 16-bit words), stage by stage and through a whole forward.

Shapes: D = 512, region_num = 8.  N = 1 and 50 leave most waves without a row, 300 has pad rows inside and behind the last
regions, 1000 is the general case, 2600 gives every wave several rows at every width the kernels take (w = 3 on 256 CUs is
3072 waves for 2704 padded rows; the row loop itself runs at w = 1 and 2)."""
import ctypes as C

import pytest
import torch

from rrt_mil_amd import _lib, synth

pytestmark = pytest.mark.gpu

D = 512
SIZES = (1, 50, 300, 1000, 2600)
WIDTHS = (1, 2, 3)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    _lib.load()


@pytest.fixture(scope="module")
def params():
    from hip_util import dev
    return dict(gm=dev(1.0 + synth.uniform("rows/g", (D,), -0.3, 0.3)), bt=dev(synth.uniform("rows/b", (D,), -0.2, 0.2)))


@pytest.mark.parametrize("L", SIZES)
def test_ln_partition_rows(L, params):
    """u of rrt_ln_partition_rows_f32 at w = 1, 2, 3 (and its own w = 0) == rrt_ln_partition_f32's, bit for bit, into a
    NaN-filled buffer (pad rows must come out as exact zeros); the counters handed over for zeroing are zero afterwards."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    g = _lib.region_grid(L, 8)
    Np = g.H * g.H
    x = dev(synth.bag(L, D, tag="rows/lnp"))
    ref = torch.full((Np, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_ln_partition_f32(p(x), p(params["gm"]), p(params["bt"]), p(ref), L, D, C.byref(g), stream()), "lnp")
    torch.cuda.synchronize()
    assert not torch.isnan(ref).any()
    for w in (0,) + WIDTHS:
        u = torch.full((Np, D), float("nan"), device=DEV)
        cnt = torch.full((300,), 7, dtype=torch.int32, device=DEV)        # more than one pass of block 0's 256 threads
        _lib.check(lib.rrt_ln_partition_rows_f32(p(x), p(params["gm"]), p(params["bt"]), p(u), L, D, C.byref(g), w, p(cnt), 290,
                                                 stream()), "lnp rows")
        torch.cuda.synchronize()
        assert torch.equal(u, ref), f"L={L} w={w}: {int((u != ref).sum())} words differ"
        assert int(cnt[:290].abs().sum()) == 0 and bool((cnt[290:] == 7).all()), f"L={L} w={w}: counters"
    # no counters: nothing is touched
    u = torch.full((Np, D), float("nan"), device=DEV)
    _lib.check(lib.rrt_ln_partition_rows_f32(p(x), p(params["gm"]), p(params["bt"]), p(u), L, D, C.byref(g), 2, None, 0, stream()),
               "lnp rows")
    torch.cuda.synchronize()
    assert torch.equal(u, ref)


@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("k", (1, 3, 5))
def test_crmsa_dispatch_ln_rows(L, k, params):
    """y (and the bf16 side output y16) of rrt_crmsa_dispatch_ln_rows_f32 at w = 1, 2, 3 == the one-wave-per-row kernel's, with
    and without the shortcut x0: y against rrt_crmsa_dispatch_ln_f32, y16 against the same entry point at w = 0 (the only one
    that exposes the side output)."""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    g8 = _lib.region_grid(L, 8)
    Np8 = g8.H * g8.H
    x1 = dev(synth.normal("rows/x1", (L, D)) * 1.3 + 0.2)
    x0 = dev(synth.normal("rows/x0", (L, D)))
    wd = dev(synth.uniform("rows/wd", (Np8, k), 0.0, 1.0))
    rep2 = dev(synth.normal("rows/rep2", (k, 64, D)))
    gm, bt = params["gm"], params["bt"]
    for shortcut in (None, x0):
        ref = torch.full((L, D), float("nan"), device=DEV)
        _lib.check(lib.rrt_crmsa_dispatch_ln_f32(p(x1), p(shortcut), p(wd), p(rep2), p(gm), p(bt), p(ref), L, D, k, C.byref(g8),
                                                 stream()), "dispatch")
        ref0 = torch.full((L, D), float("nan"), device=DEV)
        ref16 = torch.full((L, D), -1, dtype=torch.int16, device=DEV)
        _lib.check(lib.rrt_crmsa_dispatch_ln_rows_f32(p(x1), p(shortcut), p(wd), p(rep2), p(gm), p(bt), p(ref0), L, D, k, C.byref(g8),
                                                      0, p(ref16), _lib.COMPUTE_BF16, stream()), "dispatch w=0")
        torch.cuda.synchronize()
        assert not torch.isnan(ref).any() and torch.equal(ref0, ref)
        # the side output is the bf16 rounding of y (round to nearest even), so the reference itself is pinned
        assert torch.equal(ref16.view(torch.bfloat16), ref.to(torch.bfloat16))
        for w in WIDTHS:
            for with16 in (False, True):
                y = torch.full((L, D), float("nan"), device=DEV)
                y16 = torch.full((L, D), -1, dtype=torch.int16, device=DEV)
                _lib.check(lib.rrt_crmsa_dispatch_ln_rows_f32(p(x1), p(shortcut), p(wd), p(rep2), p(gm), p(bt), p(y), L, D, k,
                                                              C.byref(g8), w, p(y16) if with16 else None,
                                                              _lib.COMPUTE_BF16 if with16 else 0, stream()), "dispatch rows")
                torch.cuda.synchronize()
                what = f"L={L} k={k} w={w} shortcut={shortcut is not None} y16={with16}"
                assert torch.equal(y, ref), f"{what}: {int((y != ref).sum())} words of y differ"
                if with16:
                    assert torch.equal(y16, ref16), f"{what}: {int((y16 != ref16).sum())} words of y16 differ"
                else:
                    assert bool((y16 == -1).all()), f"{what}: y16 written without being asked for"


@pytest.mark.parametrize("L", (1, 130))
def test_layernorm_rows(L, params):
    """the plain LayerNorm use of the dispatch kernel (launch_layernorm: k = 0, no dispatch) in its row-looping form ==
    rrt_layernorm_f32's output, with and without the shortcut"""
    from hip_util import dev, p, stream, DEV
    lib = _lib.load()
    x1 = dev(synth.normal("rows/ln/x1", (L, D)) * 0.7 - 0.1)
    x0 = dev(synth.normal("rows/ln/x0", (L, D)))
    gm, bt = params["gm"], params["bt"]
    for shortcut in (None, x0):
        ref = torch.full((L, D), float("nan"), device=DEV)
        _lib.check(lib.rrt_layernorm_f32(p(x1), p(shortcut), p(gm), p(bt), p(ref), L, D, stream()), "layernorm")
        torch.cuda.synchronize()
        assert not torch.isnan(ref).any()
        for w in (0,) + WIDTHS:
            y = torch.full((L, D), float("nan"), device=DEV)
            _lib.check(lib.rrt_crmsa_dispatch_ln_rows_f32(p(x1), p(shortcut), None, None, p(gm), p(bt), p(y), L, D, 0, None, w, None, 0,
                                                          stream()), "layernorm rows")
            torch.cuda.synchronize()
            assert torch.equal(y, ref), f"L={L} w={w} shortcut={shortcut is not None}: {int((y != ref).sum())} words differ"


def test_stage_entry_refusals():
    """widths outside 0 .. 3 and inconsistent side-output arguments are refused before anything is launched"""
    lib = _lib.load()
    g = _lib.region_grid(50, 8)
    one = 8       # a non-null pointer value that is never dereferenced: the checks come first
    assert lib.rrt_ln_partition_rows_f32(one, one, one, one, 50, D, C.byref(g), 4, None, 0, None) == -1
    assert lib.rrt_ln_partition_rows_f32(one, one, one, one, 50, D, C.byref(g), -1, None, 0, None) == -1
    assert lib.rrt_ln_partition_rows_f32(one, one, one, one, 50, D, C.byref(g), 2, None, 5, None) == -1
    assert lib.rrt_crmsa_dispatch_ln_rows_f32(one, None, one, one, one, one, one, 50, D, 3, C.byref(g), 4, None, 0, None) == -1
    assert lib.rrt_crmsa_dispatch_ln_rows_f32(one, None, one, one, one, one, one, 50, D, 3, C.byref(g), 2, one, 0, None) == -1
    assert lib.rrt_crmsa_dispatch_ln_rows_f32(one, None, one, None, one, one, one, 50, D, 0, None, 2, None, 0, None) == -1


def test_encoder_forward_rows_bit_identical():
    """rrt_encoder_forward_f32 at N = 1000 with solo = 0 == the same forward with its two streaming stages forced to the
    one-wave-per-row kernels (rrt_debug_encoder_forward_rows_f32, rows_w = 0) and to every row-looping width, bit for bit;
    rrt_encoder_plan_rows reports the form the plan takes for solo = 0 and a wave per row for solo = 1."""
    from hip_util import encoder_from_state, DEV
    lib = _lib.load()
    n = 1000
    cfg = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
    enc = encoder_from_state(synth.encoder_state(**cfg), cfg)
    enc._desc.compute, enc._desc.solo = _lib.COMPUTE_F32, 0
    w = enc._weights()
    x = torch.from_numpy(synth.bag(n, 512, tag="rows/e2e")).to(DEV)
    need = C.c_size_t()
    _lib.check(lib.rrt_encoder_workspace_size(C.byref(enc._desc), n, C.byref(need)), "workspace size")
    ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def forced(rows_w):
        y = torch.full((n, 512), float("nan"), device=DEV)
        _lib.check(lib.rrt_debug_encoder_forward_rows_f32(C.byref(enc._desc), C.byref(w), x.data_ptr(), y.data_ptr(), n, ws.data_ptr(),
                                                          ws.numel(), st, rows_w), f"forward rows_w={rows_w}")
        torch.cuda.synchronize()
        return y
    ref = forced(0)
    assert not torch.isnan(ref).any()
    y = torch.full((n, 512), float("nan"), device=DEV)
    _lib.check(lib.rrt_encoder_forward_f32(C.byref(enc._desc), C.byref(w), x.data_ptr(), y.data_ptr(), n, ws.data_ptr(), ws.numel(),
                                           st), "forward")
    torch.cuda.synchronize()
    assert torch.equal(y, ref), f"the plan's forward: {int((y != ref).sum())} words differ from the one-wave-per-row forward"
    for rows_w in WIDTHS:
        got = forced(rows_w)
        assert torch.equal(got, ref), f"rows_w={rows_w}: {int((got != ref).sum())} words differ"
    # the plan: what this build's rule says for bags in flight, and never the row-looping forms for one bag in flight
    from test_rows_plan_cpu import EXPECT_ROWS_W
    pw = C.c_int32(-1)
    assert lib.rrt_encoder_plan_rows(C.byref(enc._desc), n, C.byref(pw)) == 0 and pw.value == EXPECT_ROWS_W
    enc._desc.solo = 1
    assert lib.rrt_encoder_plan_rows(C.byref(enc._desc), n, C.byref(pw)) == 0 and pw.value == 0
    enc._desc.solo = 0
    assert lib.rrt_debug_encoder_forward_rows_f32(C.byref(enc._desc), C.byref(w), x.data_ptr(), y.data_ptr(), n, ws.data_ptr(),
                                                  ws.numel(), st, 4) == -1
