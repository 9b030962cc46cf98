"""TransMIL on the MI355X: ms per slide and slides/s of TransMIL.forward_bag (one rrt_transmil_forward_f32 call) against the
same model evaluated with eager PyTorch ops in fp32 on the same GPU (tests/nystrom_ref.py, the restatement the tests use),
and the per-kernel table of one Nystrom layer at that size.

    python tools/bench_transmil.py [--out profiles/transmil.txt] [--n 9000] [--input-dim 1024] [--reps 30]

Timing: HIP events on the stream around each repetition after warm-up, four distinct bags cycled, the two variants
alternating repetition by repetition; medians (min-max) are reported.  The per-kernel rows time each stage entry point alone
(events around batches of 10 calls, launch included) on tensors of the layer's shapes; FLOPs are counted from the shapes of this
decomposition and the share is of the 157.3 TFLOP/s fp32 matrix peak.
"""
import argparse
import math
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401
from rrt_mil_amd import TransMIL, _lib, synth  # noqa: E402
import nystrom_ref as R  # noqa: E402

DEV = "cuda:0"
PEAK_TF = 157.3


def timed(fn, reps, per=1):
    """ms per call: `reps` event-timed batches of `per` calls on the current stream"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / per)
    return out


def med(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f}-{max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--input-dim", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_transmil.py needs the MI355X: no HIP device visible")
    N, reps = a.n, max(20, a.reps)
    state = synth.transmil_state(a.input_dim, 2)
    model = TransMIL(a.input_dim, 2, False, "relu")
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    model = model.to(DEV).eval()
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    bags = [torch.from_numpy(synth.bag(N, a.input_dim, tag=f"bench/transmil{i}", nonneg=True)).to(DEV) for i in range(4)]
    it = [0]

    def hip():
        it[0] += 1
        with torch.no_grad():
            return model.forward_bag(bags[it[0] % 4])

    def eager():
        it[0] += 1
        with torch.no_grad():
            return R.transmil(bags[it[0] % 4], sd, "relu", dtype=torch.float32, device=DEV)["logits"]

    for _ in range(5):
        hip()
        eager()
    torch.cuda.synchronize()
    diff = float((hip()[0] - R.transmil(bags[it[0] % 4], sd, "relu", dtype=torch.float32, device=DEV)["logits"]).abs().max())
    t_hip, t_eager = [], []
    for _ in range(reps):                                   # alternate: clock drift hits both alike
        t_hip += timed(hip, 1)
        t_eager += timed(eager, 1)
    side = math.isqrt(N - 1) + 1
    rows = 1 + side * side
    npad = (rows + 255) // 256 * 256
    lines = [f"TransMIL(input_dim={a.input_dim}, n_classes=2, act='relu'), N = {N} ({rows} rows, {npad} padded), "
             f"{torch.cuda.get_device_name(0)}; ms per slide, median (min-max) of {reps} alternating repetitions, 4 bags cycled",
             f"forward_bag (one rrt_transmil_forward_f32 call)   {med(t_hip)}   {1e3 / statistics.median(t_hip):8.1f} slides/s",
             f"eager PyTorch fp32 on the same GPU (nystrom_ref)   {med(t_eager)}   {1e3 / statistics.median(t_eager):8.1f} slides/s"
             f"   ratio {statistics.median(t_eager) / statistics.median(t_hip):.2f}x",
             f"max |logit difference| between the two on one bag: {diff:.2e}", ""]

    # ---- one Nystrom layer, stage by stage
    lib, h, d, m, dim = _lib.load(), 8, 64, 256, 512
    hd = h * d
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s, sc=1.0: torch.randn(*s, device=DEV, generator=g) * sc   # noqa: E731
    x, wq, wo, bo = rnd(rows, dim), rnd(3 * hd, dim, sc=dim ** -0.5), rnd(dim, hd, sc=hd ** -0.5), rnd(dim, sc=0.05)
    conv = rnd(h, 33, sc=33 ** -0.5)
    qkv = torch.zeros(npad, 3 * hd, device=DEV)
    ql, kl, av, wz = (torch.empty(h, m, d, device=DEV) for _ in range(4))
    a2, z = (torch.empty(h, m, m, device=DEV) for _ in range(2))
    o, y = torch.empty(npad, hd, device=DEV), torch.empty(rows, dim, device=DEV)
    need = C.c_size_t()
    _lib.check(lib.rrt_nystrom_landmark_attn_workspace_size(npad, h, C.byref(need)), "ws")
    ws_l = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rrt_nystrom_pinv_workspace_size(h, C.byref(need)), "ws")
    ws_p = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    st = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    p = lambda t: t.data_ptr()   # noqa: E731
    pad = npad - rows
    stages = [
        ("qkv linear (rrt_linear_f32)", 2.0 * rows * dim * 3 * hd,
         lambda: lib.rrt_linear_f32(p(x), p(wq), None, p(qkv) + pad * 3 * hd * 4, rows, 3 * hd, dim, hd, 0.125, 0, st())),
        ("landmarks", 2.0 * npad * hd, lambda: lib.rrt_nystrom_landmarks_f32(p(qkv), p(ql), p(kl), npad, h, st())),
        ("landmark_sim (a2)", 2.0 * h * m * m * d, lambda: lib.rrt_nystrom_landmark_sim_f32(p(ql), p(kl), p(a2), h, st())),
        ("landmark_attn (a3 v)", 4.0 * h * m * npad * d,
         lambda: lib.rrt_nystrom_landmark_attn_f32(p(qkv), p(ql), p(av), npad, h, p(ws_l), ws_l.numel(), st())),
        ("pinv, 6 iterations", 6 * 4 * 2.0 * h * m ** 3,
         lambda: lib.rrt_nystrom_pinv_f32(p(a2), p(z), h, 6, p(ws_p), ws_p.numel(), st())),
        ("zav", 2.0 * h * m * m * d, lambda: lib.rrt_nystrom_zav_f32(p(z), p(av), p(wz), h, st())),
        ("output (+ 33-tap stencil)", 4.0 * h * npad * m * d + 2.0 * 33 * npad * hd,
         lambda: lib.rrt_nystrom_output_f32(p(qkv), p(kl), p(wz), p(conv), p(o), npad, h, 33, st())),
        ("to_out linear (rrt_linear_f32)", 2.0 * rows * hd * dim,
         lambda: lib.rrt_linear_f32(p(o) + pad * hd * 4, p(wo), p(bo), p(y), rows, dim, hd, 0, 1.0, 0, st())),
    ]
    lines.append(f"one Nystrom layer at {rows} rows ({npad} padded), 8 heads x 64, 256 landmarks: each stage entry point alone, "
                 f"ms per call (median of {reps} batches of 10), FLOPs of this decomposition, share of the {PEAK_TF} TFLOP/s fp32 "
                 "matrix peak")
    total_ms, total_fl = 0.0, 0.0
    for name, flops, fn in stages:
        def call(fn=fn, name=name):
            _lib.check(fn(), name)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        t = statistics.median(timed(call, reps, per=10))
        total_ms, total_fl = total_ms + t, total_fl + flops
        lines.append(f"  {name:32s} {t:8.3f} ms  {flops / 1e9:7.2f} GFLOP  {flops / t / 1e9:7.1f} TFLOP/s  "
                     f"{100 * flops / t / 1e9 / PEAK_TF:5.1f} %")
    lines.append(f"  {'sum of the stages':32s} {total_ms:8.3f} ms  {total_fl / 1e9:7.2f} GFLOP  {total_fl / total_ms / 1e9:7.1f} TFLOP/s  "
                 f"{100 * total_fl / total_ms / 1e9 / PEAK_TF:5.1f} %")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
