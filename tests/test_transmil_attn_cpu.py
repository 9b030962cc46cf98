"""CPU: the attention-map surface of Nystrom attention / TransMIL -- the float64 restatement tests/transmil_attn_ref.py against
the reference's own ``return_attn=True`` goldens and against tests/nystrom_ref.py, the new C-ABI exports and their argument
checks, what must raise without a device, and the case lists of tests/test_transmil_attn_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import nystrom_ref as R
import transmil_attn_cases as AC
import transmil_attn_ref as AR
import transmil_cases as TC
from conftest import load_golden
from rrt_mil_amd import _lib
from test_transmil_cpu import nystrom_desc, nystrom_weights, transmil_desc, transmil_weights, why

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rrt_nystrom_attn_row_f32", "rrt_nystrom_attention_row_workspace_size", "rrt_nystrom_attention_row_f32",
       "rrt_transmil_attn_workspace_size", "rrt_transmil_forward_attn_f32")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x1000            # a non-NULL pointer no call may touch: every check happens before the first launch


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------ the restatement against the reference and against nystrom_ref
@pytest.mark.parametrize("dim,heads,n,gain", AC.GOLDEN_CASES, ids=lambda v: str(v))
def test_restatement_reproduces_the_reference_row(dim, heads, n, gain):
    gold = load_golden("transmil_attn_row")
    key = AC.golden_key(dim, heads, n, gain)
    state, x = TC.attn_inputs(dim, heads, n, gain)
    st = R.nystrom(x, state, heads, dtype=torch.float64)
    row = AR.attn_row(st, heads, 0, n)
    ref = torch.from_numpy(gold[key + "/attn"])
    assert ref.shape == (heads, n - 1) and ref.dtype == torch.float64
    assert AR.rel_err_max(row["attn"][:, 1:], ref) <= 1e-12, key
    assert float(gold[key + "/e32"]) <= 1e-5, key              # the reference itself stays well inside the stage rule
    if gain > 1:
        assert TC.PEAK_RANGE[0] <= st["peak"] <= TC.PEAK_RANGE[1], (key, st["peak"])


def test_the_row_is_what_the_issue_says_it_is():
    """against the materialised matrix softmax(q kl^T) z softmax(ql k^T); the pad keys keep their share; the full row sums to
    sum r; the exponent is never above 0 up to rounding"""
    dim, heads, n = 128, 2, 257
    state, x = TC.attn_inputs(dim, heads, n, 6.0)
    st = R.nystrom(x, state, heads, dtype=torch.float64)
    q, k, _ = R.split_heads(st["qkv"], heads)
    full = (q @ st["kl"].transpose(-1, -2)).softmax(-1) @ st["z"] @ (st["ql"] @ k.transpose(-1, -2)).softmax(-1)
    pad = TC.pad_of(n)
    for row in AC.rows_of(n):
        got = AR.attn_row(st, heads, row, n)
        assert AR.rel_err_max(got["full"], full[:, pad + row]) <= 1e-12
        assert torch.equal(got["attn"], got["full"][:, pad:])
        assert AR.rel_err_max(got["full"].sum(-1), got["r"].sum(-1), scale=float(got["r"].abs().sum(-1).max())) <= 1e-12
        assert float(got["full"][:, :pad].abs().sum(-1).min()) > 0.0     # the 255 pad keys keep a share
        assert float(got["attn"].min()) < 0.0                            # and entries can be negative
    s3 = st["ql"] @ k.transpose(-1, -2) - AR.lse3_of(st["qkv"], st["ql"], heads)[..., None]
    assert float(s3.max()) <= 1e-12


@pytest.mark.parametrize("input_dim,act,N", AC.MODEL_CASES, ids=lambda v: str(v))
def test_model_restatement_matches_nystrom_ref(input_dim, act, N):
    state, x = TC.model_inputs(input_dim, N)
    a, b = AR.transmil_attn(x, state, act, dtype=torch.float64), R.transmil(x, state, act, dtype=torch.float64)
    assert R.rel_err(a["logits"], b["logits"]) <= 1e-12 and R.rel_err(a["feat"], b["feat"]) <= 1e-12
    H = math.isqrt(N - 1) + 1 if N > 1 else 1
    assert a["rows"].shape == (2, 8, 1 + H * H) and a["attn"].shape == (2, 8, N)
    # the fold: every column but the cls token's lands on exactly one patch
    assert AR.rel_err_max(a["attn"].sum(-1), a["rows"][..., 1:].sum(-1)) <= 1e-12
    wrap = H * H - N
    if wrap:
        assert torch.equal(a["attn"][..., :wrap], a["rows"][..., 1:1 + wrap] + a["rows"][..., 1 + N:])
    assert torch.equal(a["attn"][..., wrap:], a["rows"][..., 1 + wrap:1 + N])


# ------------------------------------------------------------------ exports and argument checks (nothing is launched)
def test_exports(lib):
    hdr = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert "#define RRT_ABI_VERSION 29" in hdr and lib.rrt_abi_version() == 29
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rrt_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    build = __import__("rrt_mil_amd.build", fromlist=["SOURCES"])
    assert "nystrom_row.hip" in build.SOURCES and not build.PACKED_FP32_OK


def test_null_sizes_and_rows(lib):
    need = C.c_size_t()
    d, w, t, tw = nystrom_desc(), nystrom_weights(), transmil_desc(), transmil_weights()
    # the stage entry: seven pointers, row_padded, n_padded, heads
    for i in range(7):
        ptrs = [P] * 7
        ptrs[i] = None
        assert lib.rrt_nystrom_attn_row_f32(*ptrs, 0, 256, 8, None) == INVALID, i
    assert lib.rrt_nystrom_attn_row_f32(*[P] * 7, 0, 0, 8, None) == INVALID
    assert lib.rrt_nystrom_attn_row_f32(*[P] * 7, 0, -256, 8, None) == INVALID
    assert lib.rrt_nystrom_attn_row_f32(*[P] * 7, 0, 100, 8, None) == UNSUPPORTED and "n_padded" in why(lib)
    for heads in (0, 17):
        assert lib.rrt_nystrom_attn_row_f32(*[P] * 7, 0, 256, heads, None) == UNSUPPORTED and "heads" in why(lib)
    for row in (-1, 256, 1 << 40):
        assert lib.rrt_nystrom_attn_row_f32(*[P] * 7, row, 256, 8, None) == UNSUPPORTED and "row" in why(lib), row
    # the whole attention
    assert lib.rrt_nystrom_attention_row_workspace_size(None, 10, C.byref(need)) == INVALID
    assert lib.rrt_nystrom_attention_row_workspace_size(C.byref(d), 10, None) == INVALID
    assert lib.rrt_nystrom_attention_row_workspace_size(C.byref(d), 0, C.byref(need)) == INVALID
    big = 1 << 40
    for args in ((None, C.byref(w), P, P, 0, P, 10), (C.byref(d), None, P, P, 0, P, 10), (C.byref(d), C.byref(w), None, P, 0, P, 10),
                 (C.byref(d), C.byref(w), P, None, 0, P, 10), (C.byref(d), C.byref(w), P, P, 0, None, 10),
                 (C.byref(d), C.byref(w), P, P, 0, P, 0), (C.byref(d), C.byref(w), P, P, 0, P, -3),
                 (C.byref(d), C.byref(nystrom_weights(None)), P, P, 0, P, 10)):
        assert lib.rrt_nystrom_attention_row_f32(*args, P, big, None) == INVALID, args
    for row in (-1, 10, 11, 1 << 40):
        assert lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), P, P, row, P, 10, P, big, None) == UNSUPPORTED
        assert "row" in why(lib)
    bad = nystrom_desc(dim_head=32)
    assert lib.rrt_nystrom_attention_row_workspace_size(C.byref(bad), 10, C.byref(need)) == UNSUPPORTED and "dim_head" in why(lib)
    assert lib.rrt_nystrom_attention_row_f32(C.byref(bad), C.byref(w), P, P, 0, P, 10, P, big, None) == UNSUPPORTED
    assert lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), P, P, 0, P, 1000001, P, big, None) == UNSUPPORTED
    # the whole model
    assert lib.rrt_transmil_attn_workspace_size(None, 10, C.byref(need)) == INVALID
    assert lib.rrt_transmil_attn_workspace_size(C.byref(t), 10, None) == INVALID
    assert lib.rrt_transmil_attn_workspace_size(C.byref(t), 0, C.byref(need)) == INVALID
    for args in ((None, C.byref(tw), P, P), (C.byref(t), None, P, P), (C.byref(t), C.byref(tw), None, P),
                 (C.byref(t), C.byref(tw), P, None), (C.byref(t), C.byref(transmil_weights(None)), P, P)):
        assert lib.rrt_transmil_forward_attn_f32(*args, None, P, P, 10, P, big, None) == INVALID, args
    assert lib.rrt_transmil_forward_attn_f32(C.byref(t), C.byref(tw), P, P, None, P, P, 0, P, big, None) == INVALID
    badt = transmil_desc(n_classes=0)
    assert lib.rrt_transmil_attn_workspace_size(C.byref(badt), 10, C.byref(need)) == UNSUPPORTED and "n_classes" in why(lib)
    assert lib.rrt_transmil_forward_attn_f32(C.byref(badt), C.byref(tw), P, P, None, P, P, 10, P, big, None) == UNSUPPORTED
    assert lib.rrt_transmil_forward_attn_f32(C.byref(t), C.byref(tw), P, P, None, P, P, 1000001, P, big, None) == UNSUPPORTED


def test_short_workspaces(lib):
    need, plain = C.c_size_t(), C.c_size_t()
    d, w, t, tw = nystrom_desc(), nystrom_weights(), transmil_desc(), transmil_weights()
    for n in (1, 256, 2600):
        assert lib.rrt_nystrom_attention_row_workspace_size(C.byref(d), n, C.byref(need)) == 0
        assert lib.rrt_nystrom_workspace_size(C.byref(d), n, C.byref(plain)) == 0
        assert need.value >= plain.value + 2 * 8 * 256 * 4                   # lse and r behind the forward's workspace
        assert lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), P, P, 0, P, n, P, need.value - 1, None) == WORKSPACE
        assert lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), P, P, 0, P, n, P, plain.value, None) == WORKSPACE
        assert lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), P, P, 0, P, n, None, need.value, None) == WORKSPACE
        assert lib.rrt_transmil_attn_workspace_size(C.byref(t), n, C.byref(need)) == 0
        assert lib.rrt_transmil_workspace_size(C.byref(t), n, C.byref(plain)) == 0
        assert need.value >= plain.value + 2 * 8 * 256 * 4
        for a1, a2 in ((P, P), (None, None)):                                 # one size, whichever maps are asked for
            assert lib.rrt_transmil_forward_attn_f32(C.byref(t), C.byref(tw), P, P, None, a1, a2, n, P, need.value - 1,
                                                     None) == WORKSPACE
        assert lib.rrt_transmil_forward_attn_f32(C.byref(t), C.byref(tw), P, P, None, P, P, n, None, need.value, None) == WORKSPACE


_WORKSPACE_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from rrt_mil_amd import _lib
import test_transmil_cpu as T
lib = _lib.load()
n_dev = C.c_int(-1)
C.CDLL(_lib.LIB_PATH).hipGetDeviceCount(C.byref(n_dev))
if n_dev.value != 0 or torch.cuda.device_count() != 0:
    sys.exit(f"a GPU is visible ({n_dev.value} devices): the host-pointer forward calls must not run")
keep = torch.zeros(4096)
for kw in (dict(), dict(dim=128, heads=2), dict(heads=16, dim=1024), dict(residual=0)):
    for n in (1, 17, 256, 257, 2600):
        d, w = T.nystrom_desc(**kw), T.nystrom_weights(keep.data_ptr())
        need = C.c_size_t()
        assert lib.rrt_nystrom_attention_row_workspace_size(C.byref(d), n, C.byref(need)) == 0
        buf = (C.c_char * need.value)()
        x, y, a = torch.zeros(n, d.dim), torch.zeros(n, d.dim), torch.zeros(d.heads, n)
        for row in (0, n - 1):
            rc = lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), x.data_ptr(), y.data_ptr(), row, a.data_ptr(), n,
                                                   C.addressof(buf), need.value, None)
            assert rc > 0, (kw, n, rc)
        assert lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), x.data_ptr(), y.data_ptr(), 0, a.data_ptr(), n,
                                                 C.addressof(buf), need.value - 1, None) == -3
for kw in (dict(input_dim=64), dict(input_dim=1024)):
    for n in (1, 10, 250, 2500):
        t, tw = T.transmil_desc(**kw), T.transmil_weights(keep.data_ptr())
        need = C.c_size_t()
        assert lib.rrt_transmil_attn_workspace_size(C.byref(t), n, C.byref(need)) == 0
        buf = (C.c_char * need.value)()
        x, lg, a = torch.zeros(n, t.input_dim), torch.zeros(2), torch.zeros(2, 8, 2 + n + 2 * int(n ** 0.5) + 2)
        rc = lib.rrt_transmil_forward_attn_f32(C.byref(t), C.byref(tw), x.data_ptr(), lg.data_ptr(), None, a[0].data_ptr(),
                                               a[1].data_ptr(), n, C.addressof(buf), need.value, None)
        assert rc > 0, (kw, n, rc)
        assert lib.rrt_transmil_forward_attn_f32(C.byref(t), C.byref(tw), x.data_ptr(), lg.data_ptr(), None, a[0].data_ptr(),
                                                 a[1].data_ptr(), n, C.addressof(buf), need.value - 1, None) == -3
print("workspace checks ok")
"""


def test_workspace_queries_cover_what_the_calls_check():
    """The size a query returns is the size the call checks against.  No GPU in the child that makes the host-pointer calls:
    a call that passes validation fails at its first launch with a HIP error (> 0); a sizing bug shows up as RRT_E_WORKSPACE
    (-3) before anything is launched."""
    out = subprocess.run([sys.executable, "-c", _WORKSPACE_CHILD, ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0 and "workspace checks ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ------------------------------------------------------------------ the Python surface without a device
def test_what_must_raise_on_the_cpu():
    from rrt_mil_amd import NystromAttention, TransMIL
    model, attn = TransMIL(64, 2, False, "relu").eval(), NystromAttention(128, heads=2).eval()
    with torch.no_grad():
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            attn.attention_row(torch.zeros(1, 10, 128))
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            attn.attention_row(torch.zeros(1, 10, 128), row=3)
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            model(torch.zeros(1, 10, 64), return_attn=True)
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            model.forward_bag(torch.zeros(10, 64), return_attn=True)
        with pytest.raises(_lib.RRTHipError, match="no CPU fallback"):
            model.forward_bags([torch.zeros(10, 64)], return_attn=True)
        with pytest.raises(NotImplementedError, match="return_attn"):       # the existing refusal stays
            attn(torch.zeros(1, 10, 128), return_attn=True)


# ------------------------------------------------------------------ the GPU file's case lists cover what they claim
def test_case_lists_cover_what_the_gpu_file_claims():
    assert set(AC.LENGTHS) == {(128, 2), (512, 8)}
    assert sorted(AC.LENGTHS[(128, 2)]) == [1, 2, 17, 255, 256, 257, 513, 1030] and sorted(AC.LENGTHS[(512, 8)]) == [257, 2600]
    assert AC.GAINS == (1.0, 6.0) and len(AC.ATTN_CASES) == len(set(AC.ATTN_CASES)) == 20
    assert AC.rows_of(1) == [0] and AC.rows_of(2) == [0, 1] and AC.rows_of(257) == [0, 128, 256]
    assert (2600 + TC.pad_of(2600)) // 64 > 32                                # several key tiles per head
    assert AC.GOLDEN_CASES == [(128, 2, 256, 1.0), (128, 2, 512, 6.0), (512, 8, 256, 6.0)]
    gold = load_golden("transmil_attn_row")
    for c in AC.GOLDEN_CASES:
        assert c[2] % 256 == 0 and AC.golden_key(*c) + "/attn" in gold
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "transmil_attn_row.npz")) < 100_000
    assert AC.MODEL_CASES == [(64, "gelu", n) for n in (1, 3, 10, 37, 250, 1000)] + [(1024, "relu", 1000)]
    sides = {N: (math.isqrt(N - 1) + 1 if N > 1 else 1) for _, _, N in AC.MODEL_CASES}
    assert sides[3] ** 2 - 3 == 1 and sides[10] == 4 and sides[10] ** 2 - 10 == 6 and 1 + sides[250] ** 2 == 257
    src = open(os.path.join(ROOT, "tests", "test_transmil_attn_gpu.py")).read()
    for name in ("rrt_nystrom_attn_row_f32", "rrt_nystrom_attention_row_f32"):
        assert "lib.%s(" % name in src, name
