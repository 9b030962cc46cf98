"""CLAM head on the MI355X: the one-call forward against the eager head behind the same encoder, and the branch-pool kernel
alone against rrt_attn_pool_f32.

    python tools/bench_clam.py [--out profiles/clam_head.txt] [--n 9000] [--input-dim 1024]

(a) CLAM_*.forward_bag: ONE rrt_clam_forward_f32 call.  (b) the same module with the head (gate Linears, softmax over N,
mm(A, h), classifiers) as eager torch ops behind the HIP embedding + encoder: what a user of RRTEncoder alone can run.
Timing: HIP events around batches of calls on one stream after warm-up; the variants ALTERNATE batch by batch and the median
batch of each is reported, so clock drift hits them alike.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rrt_mil_amd  # noqa: E402,F401
from rrt_mil_amd import CLAM_MB, CLAM_SB, RRTEncoder, _lib, synth  # noqa: E402

DEV = "cuda:0"


def alternate(fns, batches=9, per_batch=20, warmup=10):
    """{name: median us per call} over `batches` alternating batches of `per_batch` calls"""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(batches):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_batch):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / per_batch)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--input-dim", type=int, default=1024)
    a = ap.parse_args()
    lines = [f"CLAM head, N = {a.n}, input_dim = {a.input_dim}, {torch.cuda.get_device_name(0)}; us per bag, median (min-max) of 9 "
             "alternating batches of 20"]
    x = torch.from_numpy(synth.bag(a.n, a.input_dim, tag="bench/clam", nonneg=True)).to(DEV)
    torch.manual_seed(0)
    for kind, cls, nc in (("CLAM_SB", CLAM_SB, 2), ("CLAM_MB n_classes=2", CLAM_MB, 2), ("CLAM_MB n_classes=8", CLAM_MB, 8)):
        m = cls(a.input_dim, n_classes=nc, rrt=RRTEncoder()).to(DEV).eval()
        for mode, dt in (("fp32", None), ("bf16 autocast", torch.bfloat16)):
            def one_call():
                with torch.no_grad(), torch.autocast("cuda", dtype=dt or torch.bfloat16, enabled=dt is not None):
                    return m.forward_bag(x)

            def eager():
                with torch.no_grad(), torch.autocast("cuda", dtype=dt or torch.bfloat16, enabled=dt is not None):
                    return m._eager_head(m._embed_encode(x))[0]
            r = alternate({"a": one_call, "b": eager})
            lines.append(f"{kind:22s} {mode:14s} (a) forward_bag {r['a'][0]:8.1f} ({r['a'][1]:.1f}-{r['a'][2]:.1f})   "
                         f"(b) eager head {r['b'][0]:8.1f} ({r['b'][1]:.1f}-{r['b'][2]:.1f})   b/a {r['b'][0] / r['a'][0]:.2f}x")
    # the pooling kernels alone
    lib = _lib.load()
    N, D, H = a.n, 512, 256
    y = torch.randn(N, D, device=DEV)
    ha, hb = torch.tanh(torch.randn(N, H, device=DEV)), torch.sigmoid(torch.randn(N, H, device=DEV))
    st = torch.cuda.current_stream().cuda_stream
    fns = {}
    keep = []
    for K in (1, 2, 4, 8):
        cw, cb = torch.randn(K, H, device=DEV) / 16, torch.zeros(K, device=DEV)
        need = C.c_size_t()
        _lib.check(lib.rrt_branch_pool_workspace_size(N, D, H, K, C.byref(need)), "ws")
        ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
        po, at, ra = torch.empty(K, D, device=DEV), torch.empty(K, N, device=DEV), torch.empty(K, N, device=DEV)
        keep.append((cw, cb, ws, po, at, ra))
        fns[f"branch_pool K={K}"] = (lambda cw=cw, cb=cb, ws=ws, po=po, at=at, ra=ra, K=K: _lib.check(lib.rrt_branch_pool_f32(
            y.data_ptr(), ha.data_ptr(), hb.data_ptr(), cw.data_ptr(), cb.data_ptr(), po.data_ptr(), at.data_ptr(), ra.data_ptr(),
            N, D, H, K, ws.data_ptr(), ws.numel(), st), "branch_pool"))
    cw1, cb1, _, po1, at1, ra1 = keep[0]
    need = C.c_size_t()
    _lib.check(lib.rrt_attn_pool_workspace_size(N, D, H, C.byref(need)), "ws")
    ws1 = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    fns["rrt_attn_pool_f32 (K=1)"] = lambda: _lib.check(lib.rrt_attn_pool_f32(
        y.data_ptr(), ha.data_ptr(), hb.data_ptr(), cw1.data_ptr(), cb1.data_ptr(), po1.data_ptr(), at1.data_ptr(), ra1.data_ptr(),
        N, D, H, ws1.data_ptr(), ws1.numel(), st), "attn_pool")
    r = alternate(fns, per_batch=50)
    lines.append(f"pooling alone (two launches each), N = {N}, dim = {D}, hidden = {H}, gated:")
    base = r["branch_pool K=1"][0]
    for k, v in r.items():
        lines.append(f"  {k:26s} {v[0]:7.1f} ({v[1]:.1f}-{v[2]:.1f})   {v[0] / base:.2f}x of K=1")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
