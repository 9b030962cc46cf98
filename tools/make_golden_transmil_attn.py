"""Attention-map fixtures from the REAL reference (modules/nystrom_attention.py, forward(return_attn=True), on the CPU; run
where the reference is checked out):

    python tools/make_golden_transmil_attn.py

transmil_attn_row : for every golden case of tests/transmil_attn_cases.py (lengths with n % 256 == 0, where the reference's
                    row 0 is a real row): <key>/attn [heads, n - 1] = the reference's float64 return_attn output (row 0
                    of the approximated attention matrix without column 0), and <key>/e32 = the reference's own fp32 run
                    against its own float64 run, relative to the float64 tensor's largest |entry|.
Every input and parameter regenerates from rrt-mil_amd/synth.py (nystrom_state, nystrom_input).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from rrt_mil_amd import synth  # noqa: E402
from _ref import load_reference  # noqa: E402
from transmil_attn_cases import GOLDEN_CASES, golden_key  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def main():
    load_reference()
    from modules import nystrom_attention as na
    out = {}
    for dim, heads, n, gain in GOLDEN_CASES:
        assert n % 256 == 0
        state = synth.nystrom_state(dim, heads, gain=gain)
        x = torch.from_numpy(synth.nystrom_input(n, dim))[None]
        mod = na.NystromAttention(dim, heads=heads).eval()
        mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
        with torch.no_grad():
            _, a32 = mod(x, return_attn=True)
            _, a64 = mod.double()(x.double(), return_attn=True)
        assert a64.dtype == torch.float64 and a64.shape == (1, heads, n - 1)
        key = golden_key(dim, heads, n, gain)
        out[key + "/attn"] = a64[0].numpy()
        out[key + "/e32"] = np.float64(float((a32.double() - a64).abs().max() / a64.abs().max()))
        print(key, "max |attn| %.3e" % float(a64.abs().max()), "min %.3e" % float(a64.min()), "e32 %.2e" % out[key + "/e32"],
              flush=True)
    np.savez(os.path.join(OUT, "transmil_attn_row.npz"), **out)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("transmil_"))
    print("transmil_* fixtures:", total, "bytes")
    assert total < 1_000_000


if __name__ == "__main__":
    main()
