#!/usr/bin/env python3
"""Training step of the encoder at several R-MSA head dims (fp32, drop_out = 0, one bag of N tokens, loss = <y, G>), and
what its attention backward and its forward attention kernel cost.

    python tools/bench_train_heads.py [--n 9000] [--steps 30] [--warmup 5]        step times (device events), one table
    python tools/bench_train_heads.py --run CONFIG [--n 9000] [--steps 20]        steps of one config only: run this under
                                                                                  rocprofv3 --kernel-trace --stats
    python tools/bench_train_heads.py --report CONFIG DB [--n 9000] [--steps 20]  per-step kernel times from that run's
                                                                                  rocpd database (<name>_results.db)

Configs: mlp_dim 512 with n_heads 2 / 4 / 8 / 16 (head dims 256 / 128 / 64 / 32) and mlp_dim 1024 with 8 heads (128), all
with epeg_k 15, crmsa_k 3, region_num 8.  At N = 9000 a region holds P = 144 tokens and there are 64 regions.

The attention backward's work per R-MSA layer: one [P, P] x [P, D/heads] product per (region, head) is 2 P^2 D R FLOP
whatever the head count.  The algorithm needs five (S, dA, dV, dK, dQ~); the head-dim-64 resident kernel issues seven (S and
dA twice), the streaming kernels eight (S three times, dA twice).  Shares are of the fp32 matrix peak, 157.3 TFLOP/s."""
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
FWD_ATTN = ("region_attn_generic_kernel", "region_attn_hd_kernel")
CONFIGS = {"d512_h8": (512, 8), "d512_h2": (512, 2), "d512_h4": (512, 4), "d512_h16": (512, 16), "d1024_h8": (1024, 8)}


def geometry(n, D):
    H, s, _ = O.grid(n, 8)
    R, P = (H // s) ** 2, s * s
    return R, P, 2.0 * P * P * D * R


def make_step(name, n):
    D, heads = CONFIGS[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = RRTEncoder(mlp_dim=D, n_heads=heads, epeg_k=15, crmsa_k=3, region_num=8, drop_out=0.).to(dev).train()
    x = torch.from_numpy(synth.bag(n, D, tag="bth")).to(dev).unsqueeze(0)
    G = torch.randn(1, n, D, device=dev)

    def step():
        enc.zero_grad(set_to_none=True)
        (enc(x) * G).sum().backward()
    return step


def time_steps(name, n, steps, warmup):
    step = make_step(name, n)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def report(name, db_path, n, steps):
    """kernel times per step of an `--run` trace: the attention backward's kernels, the forward attention kernel"""
    D, heads = CONFIGS[name]
    R, P, prod = geometry(n, D)
    db = sqlite3.connect(db_path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    namecol = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    gridcols = [c for c in ("grid_x", "grid_y", "grid_z") if c in cols] or [c for c in cols if c.startswith("grid")][:3]
    per, fwd = {}, {}
    for row in db.execute(f"select {', '.join([namecol, 'start', 'end'] + gridcols)} from kernels"):
        kname = row[0].replace("(anonymous namespace)::", "").replace("void ", "")
        per.setdefault(kname, []).append((row[2] - row[1]) / 1e3)
        if kname.startswith(FWD_ATTN):                 # forward attention kernel: calls told apart by grid size
            fwd.setdefault((kname.split("(")[0], tuple(row[3:])), []).append((row[2] - row[1]) / 1e3)
    calls = steps + 2                               # --run: two warm-up steps, then the timed ones
    attn = {k: v for k, v in per.items() if k.split("(")[0].startswith(("attn_bwd", "attn_stencil", "attn_adjoint"))}
    # CR-MSA's inner attention (k x 64 representatives, no EPEG) runs its own backward: the resident <4, .> instance or
    # the VALU kernel; everything else here is the R-MSA layer's
    inner = lambda k: k.startswith("attn_bwd_kernel<4,") or k.startswith("attn_bwd_generic_kernel")
    rmsa_us = sum(sum(v) for k, v in attn.items() if not inner(k)) / calls
    issued = 7 if (D // heads == 64 and P <= 208) else 8
    print(f"## {name}: mlp_dim {D}, {heads} heads (head dim {D // heads}), N {n}: {R} regions of P = {P}")
    print(f"{'kernel':64s} {'calls/step':>10s} {'avg_us':>9s} {'us/step':>9s}")
    for k, v in sorted(attn.items(), key=lambda kv: -sum(kv[1])):
        print(f"{k.split('(')[0][:64]:64s} {len(v) / calls:10.2f} {np.mean(v):9.2f} {sum(v) / calls:9.2f}"
              f"{'   (CR-MSA inner)' if inner(k) else ''}")
    print(f"R-MSA attention backward: {rmsa_us:.1f} us per layer; {5 * prod / 1e9:.2f} GFLOP algorithmic -> "
          f"{5 * prod / (rmsa_us * 1e-6) / PEAK:.3f} of the fp32 matrix peak; {issued} products issued ({issued * prod / 1e9:.2f} "
          f"GFLOP) -> {issued * prod / (rmsa_us * 1e-6) / PEAK:.3f}")
    # whichever forward attention kernel ran at this head dim (the VALU one, or the MFMA one of region_attn_hd.hip); the
    # call with the largest grid is the R-MSA layer's, a smaller one CR-MSA's inner attention under the same name
    rmsa_grid = max((int(np.prod(g)) for _, g in fwd), default=0)
    for (k, g), v in sorted(fwd.items(), key=lambda kv: -sum(kv[1])):
        is_rmsa = int(np.prod(g)) == rmsa_grid
        share = f", {2 * prod / (np.mean(v) * 1e-6) / PEAK:.3f} of the fp32 matrix peak for 2 products" if is_rmsa else ""
        print(f"forward attention kernel {k} grid {'x'.join(map(str, g))} ({'R-MSA' if is_rmsa else 'CR-MSA inner'}): "
              f"{len(v) / calls:.2f} calls/step, avg {np.mean(v):.1f} us, {sum(v) / calls:.1f} us/step{share}")
    tot = sum(sum(v) for v in per.values()) / calls
    print(f"all kernels: {tot:.1f} us per step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--run")
    ap.add_argument("--report", nargs=2, metavar=("CONFIG", "DB"))
    a = ap.parse_args()
    if a.report:
        report(a.report[0], a.report[1], a.n, a.steps)
        return
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.run:
        step = make_step(a.run, a.n)
        for _ in range(a.steps + 2):
            step()
        torch.cuda.synchronize()
        return
    print(f"# training step (forward with stash + backward), fp32, N = {a.n}; device events, {a.steps} steps after "
          f"{a.warmup} warm-up: median [min, max] ms")
    base = None
    for name in CONFIGS:
        med, lo, hi = time_steps(name, a.n, a.steps, a.warmup)
        if name == "d512_h8":
            base = med
        D, heads = CONFIGS[name]
        print(f"{name:10s} head dim {D // heads:4d}: {med:.3f} [{lo:.3f}, {hi:.3f}] ms" +
              (f"   ({med / base:.2f} x the 8-head step)" if base and D == 512 and name != "d512_h8" else ""))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
