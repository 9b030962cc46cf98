"""CPU: the plan rule for the row-looping LayerNorm + partition / dispatch + LayerNorm kernels, through rrt_encoder_plan_rows
(host-only, as rrt_encoder_plan), and the refusals of the test-hook forward before its first launch."""
import ctypes as C

from rrt_mil_amd import RRTEncoder, _lib

# What api.hip::plan_encoder takes for exact fp32 with bags in flight (solo = 0), dim <= 512, crmsa_k <= 3: waves per SIMD of
# the row-looping forms, 0 = one wave per row.  The A/B behind the value: profiles/rows_in_flight_ab.txt, DESIGN.md section 9.
EXPECT_ROWS_W = 1


def _rows(lib, enc, n, solo, compute=_lib.COMPUTE_F32):
    enc._desc.compute, enc._desc.solo = compute, solo
    w = C.c_int32(-1)
    assert lib.rrt_encoder_plan_rows(C.byref(enc._desc), n, C.byref(w)) == 0
    enc._desc.compute = _lib.COMPUTE_F32
    return w.value


def test_plan_rows_rule():
    lib = _lib.load()
    enc = RRTEncoder()
    for n in (50, 1000, 9000, 30000):
        assert _rows(lib, enc, n, solo=0) == EXPECT_ROWS_W, n
        assert _rows(lib, enc, n, solo=1) == 0, n                          # one bag in flight: a wave per row
        for compute in (_lib.COMPUTE_BF16, _lib.COMPUTE_F16, _lib.COMPUTE_F32X3):
            assert _rows(lib, enc, n, solo=0, compute=compute) == 0, (n, compute)     # exact fp32 only
    assert _rows(lib, RRTEncoder(cr_msa=False), 9000, solo=0) == EXPECT_ROWS_W          # the final LayerNorm alone
    assert _rows(lib, RRTEncoder(crmsa_k=1), 9000, solo=0) == EXPECT_ROWS_W
    # forms that do not fit two waves beside two fused R-MSA waves of a SIMD stay with a wave per row
    assert _rows(lib, RRTEncoder(crmsa_k=5), 9000, solo=0) == 0
    assert _rows(lib, RRTEncoder(mlp_dim=1024), 9000, solo=0) == 0
    assert lib.rrt_encoder_plan_rows(C.byref(enc._desc), 9000, None) == -1
    assert lib.rrt_encoder_plan_rows(C.byref(enc._desc), 0, C.byref(C.c_int32())) == -1


def test_plan_flags_do_not_carry_the_rows_choice():
    """rrt_encoder_plan's flag word is compared for equality by its users: the rows choice has its own entry point"""
    lib = _lib.load()
    enc = RRTEncoder()
    fl = C.c_int32(-1)
    for solo in (0, 1):
        enc._desc.solo = solo
        assert lib.rrt_encoder_plan(C.byref(enc._desc), 9000, C.byref(fl)) == 0
        assert fl.value & ~(_lib.PLAN_FUSED | _lib.PLAN_FUSED_PROJ | _lib.PLAN_CRMSA_PARTS) == 0


def test_forced_rows_forward_refuses_on_the_host():
    lib = _lib.load()
    enc = RRTEncoder()
    for bad in (-1, 4):
        assert lib.rrt_debug_encoder_forward_rows_f32(C.byref(enc._desc), None, None, None, 10, None, 0, None, bad) == -1
    assert lib.rrt_debug_encoder_forward_rows_f32(C.byref(enc._desc), None, None, None, 10, None, 0, None, 2) == -1   # null pointers
