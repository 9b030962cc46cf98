"""Fixtures of the Nystrom ablations of RRTEncoder from the REAL reference (modules/rrt.py, modules/rmsa.py,
modules/nystrom_attention.py, on the CPU; run where the reference is checked out):

    python tools/make_golden_ntrans.py

Only what a test compares is stored; every input and parameter regenerates from rrt-mil_amd/synth.py through
tests/ntrans_cases.py.

ntrans_keys    : the reference's state_dict key / shape lists of RRTEncoder(attn='ntrans') and RRTEncoder(region_attn='ntrans')
                 at the tests' configuration.
ntrans_attn    : for every batched attention case: rows 0 and n - 1 of every item of the reference NystromAttention's float64
                 output on the (b, n, dim) batch, and e32 = its own fp32 run against its own float64 run.
ntrans_encoder : for every encoder case: rows 0, 1, N // 2, N - 1 of the reference RRTEncoder's float64 output and e32; for
                 the two RRTMIL cases the float64 logits and e32.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from _ref import load_reference  # noqa: E402
import ntrans_cases as NC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def load(module, state, dtype):
    module.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    return module.to(dtype).eval()


def main():
    RRTEncoder, RRTMIL = load_reference()
    from modules.nystrom_attention import NystromAttention
    keys, attn, enc = {}, {}, {}
    with torch.no_grad():
        for mode, kw in (("bag", dict(attn="ntrans")), ("regions", dict(region_attn="ntrans"))):
            sd = RRTEncoder(**NC.ENC_BASE, **kw).state_dict()
            keys[mode] = np.frombuffer(json.dumps([[k, list(v.shape)] for k, v in sd.items()]).encode(), dtype=np.uint8)
        for name, (b, n, peaked) in NC.ATTN_CASES.items():
            state, x = NC.batch_inputs(b, n, peaked)
            ys = [load(NystromAttention(dim=NC.DIM, dim_head=64, heads=NC.HEADS), state, dt)(torch.from_numpy(x).to(dt))
                  for dt in (torch.float64, torch.float32)]
            attn[name + "/y"] = ys[0][:, [0, n - 1]].numpy()
            attn[name + "/e32"] = np.float64(rel(ys[1], ys[0]))
            print(name, "e32", attn[name + "/e32"])
        for name in NC.ENCODER_CASES:
            cfg, state, x = NC.encoder_inputs(name)
            ys = [load(RRTEncoder(**cfg), state, dt)(torch.from_numpy(x).to(dt)) for dt in (torch.float64, torch.float32)]
            enc[name + "/y"] = ys[0][NC.golden_rows(x.shape[0])].numpy()
            enc[name + "/e32"] = np.float64(rel(ys[1], ys[0]))
            print(name, "e32", enc[name + "/e32"])
        for name in NC.MIL_CASES:
            cfg, state, x = NC.mil_inputs(name)
            ys = [load(RRTMIL(input_dim=NC.MIL_INPUT_DIM, **cfg), state, dt)(torch.from_numpy(x).to(dt)[None])
                  for dt in (torch.float64, torch.float32)]
            enc[name + "/logits"] = ys[0][0].numpy()
            enc[name + "/e32"] = np.float64(rel(ys[1], ys[0]))
            print(name, "e32", enc[name + "/e32"])
    np.savez_compressed(os.path.join(OUT, "ntrans_keys.npz"), **keys)
    np.savez_compressed(os.path.join(OUT, "ntrans_attn.npz"), **attn)
    np.savez_compressed(os.path.join(OUT, "ntrans_encoder.npz"), **enc)


if __name__ == "__main__":
    main()
