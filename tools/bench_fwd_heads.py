#!/usr/bin/env python3
"""Inference latency of the encoder at several R-MSA head dims (one bag of N tokens through enc.eval() under no_grad, fp32
and bf16 autocast), and what its forward attention kernel costs.

    python tools/bench_fwd_heads.py [--n 9000] [--calls 30] [--warmup 5]         latencies (device events), one table
    python tools/bench_fwd_heads.py --run CONFIG [--n 9000] [--calls 30]         fp32 calls of one config only: run this
                                                                                 under rocprofv3 --kernel-trace --stats
    python tools/bench_fwd_heads.py --report CONFIG DB [--n 9000]                the forward attention kernel's times
                                                                                 from that run's rocpd database

Configs as tools/bench_train_heads.py: mlp_dim 512 with n_heads 2 / 4 / 8 / 16 (head dims 256 / 128 / 64 / 32) and mlp_dim
1024 with 8 heads (128), epeg_k 15, crmsa_k 3, region_num 8.  The attention's work per R-MSA layer is two [P, P] x [P, D/heads]
products per (region, head): 2 x 2 P^2 D R FLOP; shares are of the fp32 matrix peak, 157.3 TFLOP/s.  Uses the public module
only, so it runs unchanged on older commits."""
import argparse
import os
import sqlite3
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rrt_mil_amd import RRTEncoder, synth          # noqa: E402
from oracle import rrt_oracle as O                  # noqa: E402

PEAK = 157.3e12
CONFIGS = {"d512_h8": (512, 8), "d512_h2": (512, 2), "d512_h4": (512, 4), "d512_h16": (512, 16), "d1024_h8": (1024, 8)}
# forward attention kernels of the non-fused path (head dim 64 at P = 144 runs the fused R-MSA kernel instead)
FWD_ATTN = ("region_attn_generic_kernel", "region_attn_hd_kernel", "region_attn_kernel", "region_attn_resident_kernel")


def make_call(name, n):
    D, heads = CONFIGS[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = RRTEncoder(mlp_dim=D, n_heads=heads, epeg_k=15, crmsa_k=3, region_num=8).to(dev).eval()
    x = torch.from_numpy(synth.bag(n, D, tag="bfh")).to(dev).unsqueeze(0)

    def call():
        with torch.no_grad():
            return enc(x)
    return call


def time_calls(call, calls, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def report(name, db_path, n):
    D, heads = CONFIGS[name]
    H, s, _ = O.grid(n, 8)
    R, P = (H // s) ** 2, s * s
    flop = 2 * 2.0 * P * P * D * R
    db = sqlite3.connect(db_path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    namecol = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    gridcols = [c for c in ("grid_x", "grid_y", "grid_z") if c in cols] or [c for c in cols if c.startswith("grid")][:3]
    fwd, total, launches = {}, 0.0, 0
    for row in db.execute(f"select {', '.join([namecol, 'start', 'end'] + gridcols)} from kernels"):
        kname = row[0].replace("(anonymous namespace)::", "").replace("void ", "")
        total += (row[2] - row[1]) / 1e3
        launches += 1
        if kname.startswith(FWD_ATTN):
            fwd.setdefault((kname.split("(")[0], tuple(row[3:])), []).append((row[2] - row[1]) / 1e3)
    print(f"## {name}: mlp_dim {D}, {heads} heads (head dim {D // heads}), N {n}: {R} regions of P = {P}; "
          f"{flop / 1e9:.2f} GFLOP of attention per R-MSA layer")
    if not fwd:
        print("no stand-alone forward attention kernel in this trace (fused R-MSA kernel)")
    rmsa_grid = max((int(np.prod(g)) for _, g in fwd), default=0)
    for (k, g), v in sorted(fwd.items(), key=lambda kv: -sum(kv[1])):
        is_rmsa = int(np.prod(g)) == rmsa_grid
        share = f", {flop / (np.mean(v) * 1e-6) / PEAK:.3f} of the fp32 matrix peak" if is_rmsa else ""
        print(f"{k} grid {'x'.join(map(str, g))} ({'R-MSA' if is_rmsa else 'CR-MSA inner'}): {len(v)} calls, avg "
              f"{np.mean(v):.1f} us [min {np.min(v):.1f}, max {np.max(v):.1f}]{share}")
    print(f"all kernels: {total:.1f} us over {launches} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--run")
    ap.add_argument("--report", nargs=2, metavar=("CONFIG", "DB"))
    a = ap.parse_args()
    if a.report:
        report(a.report[0], a.report[1], a.n)
        return
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.run:
        call = make_call(a.run, a.n)
        for _ in range(a.calls + a.warmup):
            call()
        torch.cuda.synchronize()
        return
    print(f"# one bag of N = {a.n} through enc.eval() under no_grad; device events, {a.calls} calls after {a.warmup} "
          f"warm-up: median [min, max] ms")
    for name in CONFIGS:
        call = make_call(name, a.n)
        D, heads = CONFIGS[name]
        f32 = time_calls(call, a.calls, a.warmup)

        def amp():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return call()
        b16 = time_calls(amp, a.calls, a.warmup)
        print(f"{name:10s} head dim {D // heads:4d}: fp32 {f32[0]:.3f} [{f32[1]:.3f}, {f32[2]:.3f}] ms   "
              f"bf16 autocast {b16[0]:.3f} [{b16[1]:.3f}, {b16[2]:.3f}] ms")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
