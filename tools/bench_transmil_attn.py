"""TransMIL attention maps on the MI355X: what ``return_attn=True`` adds to TransMIL.forward_bag, against eager PyTorch computing
the same two rows by materialising softmax(ql k^T), and the two kernels of csrc/nystrom_row.hip alone.

    python tools/bench_transmil_attn.py [--out profiles/transmil_attn.txt] [--n 9000] [--input-dim 1024] [--reps 30]

Timing as tools/bench_transmil.py: HIP events on the stream around each repetition after warm-up, four distinct bags cycled,
the variants alternating repetition by repetition; medians (min-max) are reported.  The kernel rows time the stage entry point
rrt_nystrom_attn_row_f32 (events around batches of 10 calls, launches included) at the layer's padded length -- both kernels --
and at 256 keys, where the key kernel is 4 tiles per head and the call is all but nys_row_r_kernel; the key kernel's time is
the difference (the 256-key call pays the key kernel's launch too, so the difference is a lower bound of its time and the
share an upper bound; the time of both kernels is the upper bound).  FLOPs of the key kernel: 2 * np * 256 * 64 per head; the share is of the 157.3 TFLOP/s fp32 matrix peak.
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rrt_mil_amd  # noqa: E402,F401
from rrt_mil_amd import TransMIL, _lib, synth  # noqa: E402
import nystrom_ref as R  # noqa: E402
import transmil_attn_ref as AR  # noqa: E402
from bench_transmil import DEV, PEAK_TF, med, timed  # noqa: E402

ESTIMATE_US = 50.0           # the issue's untested estimate for the key kernel, per layer, at N = 9000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--input-dim", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_transmil_attn.py needs the MI355X: no HIP device visible")
    N, reps = a.n, max(20, a.reps)
    state = synth.transmil_state(a.input_dim, 2)
    model = TransMIL(a.input_dim, 2, False, "relu")
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    model = model.to(DEV).eval()
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    bags = [torch.from_numpy(synth.bag(N, a.input_dim, tag=f"bench/transmil{i}", nonneg=True)).to(DEV) for i in range(4)]
    it = [0]

    def bag():
        it[0] += 1
        return bags[it[0] % 4]

    def hip():
        with torch.no_grad():
            return model.forward_bag(bag())

    def hip_attn():
        with torch.no_grad():
            return model.forward_bag(bag(), return_attn=True)

    def eager():
        with torch.no_grad():
            return R.transmil(bag(), sd, "relu", dtype=torch.float32, device=DEV)["logits"]

    def eager_attn():
        with torch.no_grad():
            return AR.transmil_attn(bag(), sd, "relu", dtype=torch.float32, device=DEV)["attn"]

    variants = (hip, hip_attn, eager, eager_attn)
    for _ in range(5):
        for fn in variants:
            fn()
    torch.cuda.synchronize()
    got, ref = hip_attn()[1], AR.transmil_attn(bags[it[0] % 4], sd, "relu", dtype=torch.float32, device=DEV)["attn"]
    diff = [float((got[i] - ref[i]).abs().max() / ref[i].abs().max()) for i in range(2)]
    t = {fn.__name__: [] for fn in variants}
    for _ in range(reps):                                   # alternate: clock drift hits all alike
        for fn in variants:
            t[fn.__name__] += timed(fn, 1)
    m = {k: statistics.median(v) for k, v in t.items()}
    side = math.isqrt(N - 1) + 1
    rows = 1 + side * side
    npad = (rows + 255) // 256 * 256
    add_hip, add_eager = m["hip_attn"] - m["hip"], m["eager_attn"] - m["eager"]
    lines = [f"TransMIL(input_dim={a.input_dim}, n_classes=2, act='relu'), N = {N} ({rows} rows, {npad} padded), "
             f"{torch.cuda.get_device_name(0)}; ms per slide, median (min-max) of {reps} alternating repetitions, 4 bags cycled",
             f"forward_bag                                   {med(t['hip'])}",
             f"forward_bag(return_attn=True)                 {med(t['hip_attn'])}   adds {add_hip:.3f} ms per slide "
             "(two layers' rows and the fold)",
             f"eager PyTorch fp32 (nystrom_ref)              {med(t['eager'])}",
             f"eager PyTorch fp32 + the two rows, A3 built   {med(t['eager_attn'])}   adds {add_eager:.3f} ms per slide",
             f"with the maps, eager / HIP: {m['eager_attn'] / m['hip_attn']:.2f}x per slide; the maps alone (added ms), eager / HIP: "
             f"{add_eager / add_hip:.2f}x" if add_hip > 0 else "the added time is below the run-to-run spread",
             f"max |difference| between the two maps on one bag, relative to the layer's largest entry: "
             f"{diff[0]:.2e} (layer 1), {diff[1]:.2e} (layer 2)", ""]

    # ---- the two kernels, through the stage entry point
    lib, h, d, mm = _lib.load(), 8, 64, 256
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s, sc=1.0: torch.randn(*s, device=DEV, generator=g) * sc   # noqa: E731
    qkv = rnd(npad, 3 * h * d, sc=0.5)
    ql, kl, z = rnd(h, mm, d, sc=0.5), rnd(h, mm, d, sc=0.5), rnd(h, mm, mm, sc=1.0 / 16)
    lse3 = AR.lse3_of(qkv, ql, h).contiguous()
    r, out = torch.empty(h, mm, device=DEV), torch.empty(h, npad, device=DEV)
    st = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    p = lambda x: x.data_ptr()   # noqa: E731

    def stage(n_keys):
        def call():
            _lib.check(lib.rrt_nystrom_attn_row_f32(p(qkv), p(ql), p(kl), p(z), p(lse3), p(r), p(out), 0, n_keys, h, st()),
                       "rrt_nystrom_attn_row_f32")
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        return statistics.median(timed(call, reps, per=10))

    t_all, t_small = stage(npad), stage(256)
    t_keys = max(t_all - t_small, 1e-6)
    flops = 2.0 * npad * mm * d * h
    lines += [f"rrt_nystrom_attn_row_f32 at {npad} keys, 8 heads x 64, 256 landmarks, ms per call (median of {reps} batches of 10, "
              "launches included)",
              f"  both kernels (nys_row_r + nys_row_keys)            {t_all * 1e3:8.1f} us",
              f"  at 256 keys (nys_row_r + 4 key tiles per head)     {t_small * 1e3:8.1f} us",
              f"  nys_row_keys alone, by difference                  {t_keys * 1e3:8.1f} us   {flops / 1e9:.2f} GFLOP   "
              f"{flops / t_keys / 1e9:.1f} TFLOP/s   {100 * flops / t_keys / 1e9 / PEAK_TF:.1f} % of the {PEAK_TF} TFLOP/s fp32 matrix peak",
              f"  the issue's estimate for the key kernel: {ESTIMATE_US:.0f} us per layer (30 % of the peak)"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
