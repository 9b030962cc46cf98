"""Gradient fixtures of Nystrom attention and TransMIL from the REAL reference (modules/nystrom_attention.py,
modules/transmil.py, on the CPU; run where the reference is checked out, with einops installed):

    python tools/make_golden_transmil_grad.py

transmil_grad : for the attention cases GOLDEN_ATTN_CASES and the model cases GOLDEN_MODEL_CASES of
                tests/nystrom_grad_cases.py, the reference's float64 gradients in eval() with grad enabled -- the first and the
                last row of dx, the rows nystrom_grad_cases.golden_rows keeps of every parameter gradient -- and e32 = the
                reference's own fp32 gradients against its float64 ones, relative to the largest float64 entry.
                Attention: loss = sum(y . dy) with the seeded dy of nystrom_grad_cases.cotangent; model: cross-entropy of the
                logits against LABEL.  Every input and parameter regenerates from rrt-mil_amd/synth.py.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from rrt_mil_amd import synth  # noqa: E402
from _ref import load_reference  # noqa: E402
import nystrom_grad_cases as GC  # noqa: E402
from transmil_cases import model_inputs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def record(out, key, grads64, grads32):
    """grads: {name: tensor}; 'dx' keeps its first and last row, the others golden_rows"""
    for name, g64 in grads64.items():
        rows = torch.stack([g64[0], g64[-1]]) if name == "dx" else GC.golden_rows(g64)
        out[f"{key}/{name}"] = rows.numpy()
        out[f"{key}/e32/{name}"] = np.float64(GC.rel_grad(grads32[name].numpy(), g64.numpy()))


def attention_grads(na, dim, heads, n, gain, dtype):
    state = synth.nystrom_state(dim, heads, gain=gain)
    mod = na.NystromAttention(dim, heads=heads).eval()
    mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    mod = mod.to(dtype)
    x = torch.from_numpy(synth.nystrom_input(n, dim))[None].to(dtype).requires_grad_(True)
    dy = torch.from_numpy(GC.cotangent(f"dy/{GC.case_key(dim, heads, n, gain)}", (n, dim))).to(dtype)
    (mod(x)[0] * dy).sum().backward()
    g = {k: p.grad.detach() for k, p in mod.named_parameters()}
    g["dx"] = x.grad[0].detach()
    return g


def model_grads(tm, input_dim, act, N, dtype):
    state, x = model_inputs(input_dim, N)
    ref = tm.TransMIL(input_dim, 2, False, act).eval()
    ref.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    ref = ref.to(dtype)
    xd = torch.from_numpy(x)[None].to(dtype).requires_grad_(True)
    if dtype == torch.float64:
        xd.float = lambda: xd          # forward() casts to fp32 in front of _fc1: neutralised for the float64 run
    logits = ref(xd)
    logits = logits[0] if isinstance(logits, (tuple, list)) else logits
    F.cross_entropy(logits.reshape(1, -1), torch.tensor([GC.LABEL])).backward()
    g = {k: p.grad.detach() for k, p in ref.named_parameters()}
    g["dx"] = xd.grad[0].detach()
    return g


def main():
    load_reference()
    from modules import nystrom_attention as na
    from modules import transmil as tm
    out = {}
    for case in GC.GOLDEN_ATTN_CASES:
        g64, g32 = (attention_grads(na, *case, dt) for dt in (torch.float64, torch.float32))
        assert all(v.dtype == torch.float64 for v in g64.values())
        record(out, "attn/" + GC.case_key(*case), g64, g32)
        print(case, {k: "%.1e" % out[f"attn/{GC.case_key(*case)}/e32/{k}"] for k in g64}, flush=True)
    for case in GC.GOLDEN_MODEL_CASES:
        g64, g32 = (model_grads(tm, *case, dt) for dt in (torch.float64, torch.float32))
        assert all(v.dtype == torch.float64 for v in g64.values()) and len(g64) == 26
        record(out, "model/" + GC.model_key(*case), g64, g32)
        print(case, "worst e32 %.1e" % max(out[f"model/{GC.model_key(*case)}/e32/{k}"] for k in g64), flush=True)
    path = os.path.join(OUT, "transmil_grad.npz")
    np.savez(path, **out)
    print("transmil_grad.npz:", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 450_000


if __name__ == "__main__":
    main()
