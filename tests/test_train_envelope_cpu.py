"""CPU: the training envelope of the R-MSA attention backward at head dims other than 64 (multiples of 16 up to 256, any
region size, epeg_k <= 63), checked through the host-only entry points -- rrt_encoder_train_sizes, the stage's workspace
size and the stage's own argument check (a supported configuration gets as far as the missing workspace, an unsupported
one is refused before it) -- and, in the library, the matrix-core kernels that serve it."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

from rrt_mil_amd import RRTEncoder, _lib
from rrt_mil_amd import build as B

OK, E_UNSUPPORTED, E_WORKSPACE = 0, -2, -3


@pytest.fixture(scope="module")
def lib():
    B.build()
    return _lib.load()


def _train_sizes(lib, n, **cfg):
    enc = RRTEncoder(**cfg)
    stash, ws = C.c_size_t(), C.c_size_t()
    rc = lib.rrt_encoder_train_sizes(C.byref(enc._desc), n, C.byref(stash), C.byref(ws))
    return rc, ws.value


def _stage_check(lib, R, P, D, heads, ek):
    """the backward stage's return code with placeholder (never dereferenced) device pointers and no workspace"""
    fake = C.c_void_p(4096)
    return lib.rrt_region_attention_backward_f32(fake, fake if ek else None, fake, fake, fake, None, R, P, D, heads, ek,
                                                 None, 0, None)


@pytest.mark.parametrize("n,cfg", [
    (9000, dict(mlp_dim=512, n_heads=2, epeg_k=15, crmsa_k=3)),          # head dim 256
    (9000, dict(mlp_dim=512, n_heads=4, epeg_k=15, crmsa_k=3)),          # 128
    (9000, dict(mlp_dim=512, n_heads=16, epeg_k=15, crmsa_k=3)),         # 32
    (9000, dict(mlp_dim=512, n_heads=32, epeg_k=15, crmsa_k=3)),         # 16
    (3000, dict(mlp_dim=1024, n_heads=8)),                               # 128
    (15000, dict(mlp_dim=768, n_heads=8)),                               # 96, P = 256
    (3000, dict(mlp_dim=384, n_heads=8)),                                # 48
    (3000, dict(mlp_dim=256, n_heads=8, region_num=16)),                 # 32
    (9000, dict(mlp_dim=512, n_heads=4, epeg=False)),
    (9000, dict(mlp_dim=512, n_heads=4, epeg_type="value_bf")),
    (9000, dict(mlp_dim=512, n_heads=4, epeg_k=63)),
    (30000, dict(mlp_dim=512, n_heads=4, epeg_k=15)),                    # P = 484
    (1, dict(mlp_dim=512, n_heads=4)),
    (50, dict(mlp_dim=512, n_heads=4)),
])
def test_new_head_dims_train(lib, n, cfg):
    rc, ws = _train_sizes(lib, n, **cfg)
    assert rc == OK, lib.rrt_strerror(rc)
    assert ws > 0


@pytest.mark.parametrize("n,cfg,what", [
    (9000, dict(mlp_dim=64), b"multiple of 16"),                              # head dim 8 with EPEG, P = 144
    (9000, dict(mlp_dim=512, n_heads=1), b"multiple of 16"),                  # head dim 512 with EPEG
    (9000, dict(mlp_dim=160, n_heads=8, epeg=False), b"multiple of 16"),      # head dim 20, P > 128
    (64, dict(mlp_dim=2048, n_heads=32, crmsa_heads=32), b"dim > 1024"),
])
def test_outside_envelope_still_raises(lib, n, cfg, what):
    rc, _ = _train_sizes(lib, n, **cfg)
    assert rc == E_UNSUPPORTED
    assert what in lib.rrt_strerror(rc)
    with pytest.raises(NotImplementedError):
        _lib.check(rc, "train sizes")


@pytest.mark.parametrize("hd", [16, 32, 48, 80, 96, 128, 144, 192, 240, 256])
@pytest.mark.parametrize("P,ek", [(1, 0), (4, 31), (7, 9), (49, 15), (129, 0), (144, 21), (256, 63), (484, 15)])
def test_stage_envelope_and_workspace(lib, hd, P, ek):
    heads = 4
    D, R = hd * heads, 3
    assert _stage_check(lib, R, P, D, heads, ek) == E_WORKSPACE          # accepted: stops at the missing workspace
    need = C.c_size_t()
    assert lib.rrt_region_attention_backward_workspace_size(R, P, D, heads, ek, C.byref(need)) == OK
    part = R * heads * max(ek, 1) * 4
    generic = ek == 0 and P <= 128                                        # the VALU kernel's cases: no streaming buffers
    rows = R * P
    stream = 0 if generic else (2 * rows * D + 2 * rows * heads) * 4      # q~, tmp, lse, D
    assert need.value >= part + stream


@pytest.mark.parametrize("hd,P,ek", [(8, 144, 15), (8, 200, 0), (512, 100, 15), (272, 300, 0), (40, 49, 9),
                                     (64, 100, 65), (128, 100, 65)])
def test_stage_outside_envelope(lib, hd, P, ek):
    assert _stage_check(lib, 2, P, hd * 2, 2, ek) == E_UNSUPPORTED


def test_unchanged_workspace_of_existing_cases(lib):
    """the VALU kernel's and head dim 64's cases keep their workspace sizes (no streaming buffers where none were)"""
    need = C.c_size_t()
    for R, P, D, heads in [(64, 64, 512, 1), (3, 128, 512, 4), (8, 100, 96, 3)]:
        assert lib.rrt_region_attention_backward_workspace_size(R, P, D, heads, 0, C.byref(need)) == OK
        assert need.value == (R * heads * 4 + 255) // 256 * 256
    assert lib.rrt_region_attention_backward_workspace_size(64, 144, 512, 8, 15, C.byref(need)) == OK
    assert need.value == (64 * 8 * 15 * 4 + 255) // 256 * 256 + (2 * 64 * 144 * 512 + 2 * 64 * 144 * 8) * 4 + 1024


def test_new_kernels_use_fp32_matrix_cores(lib):
    """the streaming backward at the other head dims runs on v_mfma_f32_16x16x4_f32 (exact fp32): its q and kv passes
    carry the instruction at every head dim of the envelope (the code objects of the library, read as build.py reads them)"""
    if not os.path.exists(B.OBJDUMP):
        pytest.skip("llvm-objdump not on this machine")
    tmp = tempfile.mkdtemp(prefix="rrt_mfma_")
    outs = []
    try:
        local = os.path.join(tmp, os.path.basename(B.LIB))
        shutil.copy(B.LIB, local)
        subprocess.run([B.OBJDUMP, "--offloading", local], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" in f:
                outs.append(subprocess.run([B.OBJDUMP, "-d", "-C", os.path.join(tmp, f)], check=True, capture_output=True,
                                           text=True).stdout)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    mfma, name = {}, None
    for out in outs:
        for line in out.splitlines():
            m = B._SYM_RE.match(line)
            if m:
                name = m.group(1)
            elif name is not None and "v_mfma_f32_16x16x4_f32" in line:
                mfma[name] = mfma.get(name, 0) + 1
    for hd in (16, 32, 48, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256):
        for kern in (f"attn_bwd_q_hd_kernel<{hd}>", f"attn_bwd_kv_hd_kernel<{hd}>"):
            assert any(kern in k for k in mfma), kern
