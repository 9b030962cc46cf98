"""CPU: the host side of the matrix-core attention forward at head dims other than 64 -- the support predicate, the plan
flag rrt_encoder_plan reports for encoders whose R-MSA attention takes that kernel, the stage entry's refusal outside the
predicate, and the kernel's register metadata (no scratch in any instantiation).  Nothing is launched."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from rrt_mil_amd import RRTEncoder, _lib
from rrt_mil_amd import build as build_mod

HEAD_DIMS = [hd for hd in range(16, 257, 16) if hd != 64]


@pytest.fixture(scope="module")
def lib():
    build_mod.build()
    return _lib.load()


def test_hd_supported_table(lib):
    for ek in (0, 15, 63):
        for P in (1, 144, 484):
            for hd in HEAD_DIMS:
                for heads in (1, 2, 3):
                    assert lib.rrt_region_attention_hd_supported(P, hd * heads, heads, ek) == 1, (P, hd, heads, ek)
            for hd in (64, 8, 24, 272, 512):
                assert lib.rrt_region_attention_hd_supported(P, hd * 2, 2, ek) == 0, (P, hd, ek)
    for hd in HEAD_DIMS:
        assert lib.rrt_region_attention_hd_supported(144, hd * 2, 2, 65) == 0
    assert lib.rrt_region_attention_hd_supported(144, 512, 3, 15) == 0          # heads does not divide dim
    assert lib.rrt_region_attention_hd_supported(0, 512, 4, 15) == 0


def test_plan_reports_the_head_dim_kernel(lib):
    fl = C.c_int32(-1)

    def plan(enc, n=9000, compute=_lib.COMPUTE_F32):
        enc._desc.compute, enc._desc.solo = compute, 1
        assert lib.rrt_encoder_plan(C.byref(enc._desc), n, C.byref(fl)) == 0
        enc._desc.compute = _lib.COMPUTE_F32
        return fl.value
    for kw in (dict(n_heads=4), dict(n_heads=2), dict(n_heads=16), dict(mlp_dim=1024), dict(mlp_dim=256)):
        assert plan(RRTEncoder(**kw)) == _lib.PLAN_ATTN_HD, kw
    assert plan(RRTEncoder(n_heads=4), 15000) == _lib.PLAN_ATTN_HD               # any region size
    assert plan(RRTEncoder(n_heads=4), compute=_lib.COMPUTE_BF16) == _lib.PLAN_ATTN_HD   # autocast: fp32 attention, this kernel
    assert plan(RRTEncoder(n_heads=4, epeg=False)) == _lib.PLAN_ATTN_HD
    # head dim 64: what tests/test_abi_cpu.py::test_encoder_plan_flags expects, unchanged
    parts = _lib.PLAN_FUSED | _lib.PLAN_FUSED_PROJ | _lib.PLAN_CRMSA_PARTS
    assert plan(RRTEncoder()) == parts and plan(RRTEncoder(), 3000) == _lib.PLAN_FUSED
    assert plan(RRTEncoder(), 15000) == 0 and plan(RRTEncoder(), 600) == 0
    assert plan(RRTEncoder(), compute=_lib.COMPUTE_BF16) == _lib.PLAN_FUSED16
    # outside the predicate: head dim 8, head dim 512; the EPEG ablations keep reporting nothing
    assert plan(RRTEncoder(n_heads=64)) == 0 and plan(RRTEncoder(n_heads=1)) == 0
    assert plan(RRTEncoder(n_heads=4, epeg_type="value_bf")) == 0


def test_stage_entry_refuses_outside_the_predicate(lib):
    """The unsupported check comes before the pointer checks and nothing is dereferenced or launched on that path, so the
    calls are made in-process with NULL pointers: RRT_E_UNSUPPORTED (-2) for head dims 64 and 512, RRT_E_INVALID (-1) for
    NULL qkv / o at a head dim inside the predicate."""
    for dim, heads in ((512, 8), (512, 1), (128, 2), (1024, 2)):
        rc = lib.rrt_region_attention_hd_f32(None, None, None, 2, 144, dim, heads, 0, None)
        assert rc == -2, (dim, heads, rc)
        assert b"region_attention_hd" in lib.rrt_strerror(rc)
    assert lib.rrt_region_attention_hd_f32(None, None, None, 2, 144, 512, 4, 0, None) == -1
    assert lib.rrt_region_attention_hd_f32(None, None, None, 0, 144, 512, 4, 0, None) == -1


def test_no_scratch_in_any_instantiation(lib):
    """every region_attn_hd_kernel<HD> in the built library: private segment 0, no spilled register (a lane holds HD / 16
    accumulator fragments; a spill would put them in scratch memory)"""
    readelf = os.path.join(os.path.dirname(build_mod.OBJDUMP), "llvm-readelf")
    if not (os.path.exists(build_mod.OBJDUMP) and os.path.exists(readelf)):
        pytest.fail("llvm-objdump / llvm-readelf not found next to the compiler that built the library")
    tmp = tempfile.mkdtemp(prefix="rrt_meta_")
    try:
        local = os.path.join(tmp, "librrt_hip.so")
        shutil.copy(_lib.LIB_PATH, local)
        subprocess.run([build_mod.OBJDUMP, "--offloading", local], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        notes = "".join(subprocess.run([readelf, "--notes", os.path.join(tmp, f)], check=True, capture_output=True,
                                       text=True).stdout for f in sorted(os.listdir(tmp)) if "amdgcn" in f)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    seen = {}
    for entry in re.split(r"\n\s*- \.agpr_count:", notes):
        name = re.search(r"\.name:\s+(\S*region_attn_hd_kernel\S*)", entry)
        if not name:
            continue
        hd = int(re.search(r"region_attn_hd_kernelILi(\d+)E", name.group(1)).group(1))
        seen[hd] = tuple(int(re.search(rf"\.{key}:\s+(\d+)", entry).group(1))
                         for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
    assert sorted(seen) == HEAD_DIMS, sorted(seen)
    assert all(v == (0, 0, 0) for v in seen.values()), seen
