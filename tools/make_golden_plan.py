"""What the host side of librrt_hip.so answers before anything is launched, recorded from the library that is built in the tree:

    python tools/make_golden_plan.py          # writes tests/golden/plan_flags_grid.json

- flags: rrt_encoder_plan over a grid of bag sizes, region counts, compute modes, head counts, the solo hint, CR-MSA forms and
  EPEG forms (AXES below, itertools.product order);
- sizes: rrt_encoder_workspace_size, rrt_encoder_batch_workspace_size (B = 2) and rrt_encoder_train_sizes on a subset of it
  (return codes included: training refuses F32X3 and some head dims);
- null_codes: the return code of rrt_encoder_forward_f32 for argument sets that are refused before the first launch (a null
  weight, a workspace one byte short), made by a child process that sees no GPU.

Host calls only: no reference import, no GPU.  tests/test_abi_cpu.py imports the table builders from here and compares the
library it built with the recorded values -- regenerate the file only from a library whose choices are known to be right.
"""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from rrt_mil_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "plan_flags_grid.json")

AXES = dict(
    n=[600, 2000, 3000, 4096, 5000, 9000, 15000, 30000, 36000],
    region_num=[4, 8, 16],
    compute=[_lib.COMPUTE_F32, _lib.COMPUTE_BF16, _lib.COMPUTE_F16, _lib.COMPUTE_F32X3],
    n_heads=[8, 4, 1],
    solo=[0, 1],
    crmsa=[(1, 3, 0, 0), (1, 5, 0, 0), (1, 3, 1, 0), (1, 3, 0, 1), (0, 3, 0, 0)],      # (cr_msa, crmsa_k, ffn, crmsa_mlp)
    epeg=["attn", "off", "value_bf"],
)
SIZE_AXES = dict(AXES, n=[600, 9000], solo=[1])         # (no size depends on the solo hint)


def desc_for(region_num, compute, n_heads, solo, crmsa, epeg, dim=512, n_rmsa_layers=1):
    cr_msa, crmsa_k, ffn, crmsa_mlp = crmsa
    return _lib.EncoderDesc(
        dim=dim, n_heads=n_heads, n_rmsa_layers=n_rmsa_layers, region_num=region_num, epeg=int(epeg != "off"), epeg_k=15,
        cr_msa=cr_msa, crmsa_k=crmsa_k, crmsa_heads=8, crmsa_mlp=crmsa_mlp, compute=compute, ffn=ffn, ffn_act=_lib.ACT_GELU,
        ffn_hidden=4 * dim, epeg_type=_lib.EPEG_VALUE_BF if epeg == "value_bf" else _lib.EPEG_ATTN, solo=solo)


def cases(axes):
    """(n_tokens, descriptor) in the order of the recorded lists"""
    for n, *rest in itertools.product(*axes.values()):
        yield n, desc_for(*rest)


def plan_table(lib, axes=AXES):
    out, fl = [], C.c_int32()
    for n, d in cases(axes):
        rc = lib.rrt_encoder_plan(C.byref(d), n, C.byref(fl))
        assert rc == 0, (n, rc)
        out.append(fl.value)
    return out


def size_table(lib, axes=SIZE_AXES):
    """per case [rc, workspace bytes, rc, batch workspace bytes (B = 2), rc, stash bytes, backward workspace bytes]"""
    out = []
    for n, d in cases(axes):
        a, b, s, w = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        rc_a = lib.rrt_encoder_workspace_size(C.byref(d), n, C.byref(a))
        rc_b = lib.rrt_encoder_batch_workspace_size(C.byref(d), 2, n, C.byref(b))
        rc_t = lib.rrt_encoder_train_sizes(C.byref(d), n, C.byref(s), C.byref(w))
        out.append([rc_a, a.value, rc_b, b.value, rc_t, s.value, w.value])
    return out


# The forward calls run in a child that sees no GPU (HIP drops every HIP_VISIBLE_DEVICES index from the first invalid one on):
# each argument set is refused on the host, but a library that let one through must fail at its first launch with a HIP error
# instead of running kernels on these pointers.
_NULL_CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, sys.argv[1])
import torch
from rrt_mil_amd import RRTEncoder, _lib
lib = _lib.load()
n_dev = C.c_int(-1)
C.CDLL(os.environ.get("RRT_HIP_LIB") or _lib.LIB_PATH).hipGetDeviceCount(C.byref(n_dev))
if n_dev.value != 0 or torch.cuda.device_count() != 0:
    sys.exit(f"a GPU is visible ({n_dev.value} devices): the host-pointer forward calls must not run")
x, y = torch.zeros(9000, 512), torch.zeros(9000, 512)
codes = {}

def run(name, enc, n, null=None, compute=_lib.COMPUTE_F32, short=0):
    d = _lib.EncoderDesc.from_buffer_copy(enc._desc)
    d.compute, d.solo = compute, 1
    w = _lib.EncoderWeights.from_buffer_copy(enc._weights())
    if null:
        obj = w
        for part in null[:-1]:
            obj = getattr(obj, part) if isinstance(part, str) else obj[part]
        setattr(obj, null[-1], None)
    need = C.c_size_t()
    assert lib.rrt_encoder_workspace_size(C.byref(d), n, C.byref(need)) == 0
    # (the workspace is never touched on the host: any non-null address will do)
    codes[name] = lib.rrt_encoder_forward_f32(C.byref(d), C.byref(w), x.data_ptr(), y.data_ptr(), n, 4096, need.value - short, None)

two, one = RRTEncoder(), RRTEncoder(n_layers=1)           # one R-MSA layer + CR-MSA; CR-MSA alone
run("rmsa0_norm_w", two, 700, ("rmsa", 0, "norm_w"))
run("rmsa0_qkv_w_bf16", two, 700, ("rmsa", 0, "qkv_w"), _lib.COMPUTE_BF16)       # the weight images' job list
run("rmsa0_proj_w_x3", two, 9000, ("rmsa", 0, "proj_w"), _lib.COMPUTE_F32X3)
run("crmsa_qkv_w", one, 700, ("crmsa", "qkv_w"))
run("crmsa_qkv_w_bf16", two, 700, ("crmsa", "qkv_w"), _lib.COMPUTE_BF16)         # inner MSA on the 16-bit kernels
run("phi", one, 700, ("phi",))
run("phi_parts", two, 9000, ("phi",))                                            # the merged launch that leaves CR-MSA's row records
run("norm_w", one, 700, ("norm_w",))
run("workspace_short", two, 700, None, short=1)
run("workspace_short_crmsa_only", one, 700, None, short=1)
print("NULL_CODES " + json.dumps(codes))
"""


def null_codes():
    out = subprocess.run([sys.executable, "-c", _NULL_CHILD, ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    lines = [l for l in out.stdout.splitlines() if l.startswith("NULL_CODES ")]
    assert out.returncode == 0 and lines, out.stderr[-3000:]
    return json.loads(lines[-1][len("NULL_CODES "):])


def main():
    from rrt_mil_amd.build import build
    build()
    lib = _lib.load()
    rec = dict(axes={k: v for k, v in AXES.items()}, size_axes={k: v for k, v in SIZE_AXES.items()},
               flags=plan_table(lib), sizes=size_table(lib), null_codes=null_codes())
    with open(OUT, "w") as fh:
        json.dump(rec, fh, separators=(",", ":"))
        fh.write("\n")
    vals = sorted(set(rec["flags"]))
    print(f"wrote {OUT}: {len(rec['flags'])} flags (values {vals}), {len(rec['sizes'])} size records, null codes {rec['null_codes']}")


if __name__ == "__main__":
    main()
