"""Training the Nystrom ablations of RRTEncoder on the MI355X: ms per training step (forward with a graph + backward, every
parameter gradient and dx) of RRTEncoder(attn='ntrans').enable_training() and RRTEncoder(region_attn='ntrans').enable_training()
against

  * the same step on the eager fp32 restatement under torch.autograd on the same GPU (tests/ntrans_ref.py), and
  * for the region mode, one attention layer's backward: the one batched call (rrt_nystrom_attention_batched_backward_f32,
    b = region_num^2) next to a HOST LOOP of region_num^2 single-sequence calls (rrt_nystrom_attention_backward_f32).  The
    loop is a speed yardstick only: its values are WRONG (a pseudo-inverse scale, and its gradient, per region).

It also reports the bytes of the batched stash and backward workspace.

    python tools/bench_ntrans_train.py [--out profiles/ntrans_train.txt] [--n 9000] [--region-num 8] [--reps 20]

Timing: HIP events on the stream around each repetition after warm-up, the variants alternating repetition by repetition;
medians (min-max) are reported."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401
from rrt_mil_amd import RRTEncoder, _lib, synth  # noqa: E402
import ntrans_cases as NC  # noqa: E402
import ntrans_ref as NR  # noqa: E402

DEV = "cuda:0"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f}-{max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--region-num", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ntrans_train.py needs the MI355X: no HIP device visible")
    N, D, rn, reps = a.n, a.dim, a.region_num, max(5, a.reps)
    heads = D // 64
    bag = torch.from_numpy(synth.bag(N, D, tag="bench/ntrans_train")).to(DEV)
    dy = torch.from_numpy(synth.normal("bench/ntrans_train/dy", (N, D))).to(DEV)
    lines = [f"RRTEncoder(mlp_dim={D}, n_heads={heads}, region_num={rn}).enable_training(), N = {N}, {torch.cuda.get_device_name(0)}; "
             f"ms per training step (forward with a graph + backward), median (min-max) of {reps} alternating repetitions, "
             f"eval() with gradients on (no dropout), exact fp32"]
    for label, extra in (("attn='ntrans' (whole bag, b = 1)", dict(attn="ntrans")),
                         (f"region_attn='ntrans' ({rn * rn} regions as the batch)", dict(region_attn="ntrans", region_num=rn))):
        cfg = dict(mlp_dim=D, n_heads=heads, crmsa_heads=heads, **extra)
        state = NC.ntrans_state(cfg)
        enc = RRTEncoder(**cfg)
        enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
        enc = enc.to(DEV).eval().enable_training()
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}

        def hip():
            enc.zero_grad(set_to_none=True)
            x = bag.clone().requires_grad_(True)
            (enc(x) * dy).sum().backward()
            return x.grad

        def eager():
            for v in sd.values():
                v.grad = None
            x = bag.clone().requires_grad_(True)
            (NR.encoder(x, sd, cfg, dtype=torch.float32) * dy).sum().backward()
            return x.grad

        for _ in range(2):
            gh, ge = hip(), eager()
        torch.cuda.synchronize()
        diff = float((gh - ge).abs().max() / ge.abs().max())
        t_hip, t_eager = [], []
        for _ in range(reps):                                   # alternate: clock drift hits both alike
            t_hip.append(timed(hip))
            t_eager.append(timed(eager))
        lines += [f"{label}",
                  f"  the layer path (HIP attention + tail, torch glue)    {med(t_hip)}",
                  f"  eager PyTorch fp32 autograd on the same GPU          {med(t_eager)}   ratio "
                  f"{statistics.median(t_eager) / statistics.median(t_hip):.2f}x",
                  f"  max |dx difference| / max |dx| between the two: {diff:.2e}"]
        del enc, sd
        torch.cuda.empty_cache()

    # ---- one region-mode attention layer's backward: the batched call against a host loop over the regions
    lib = _lib.load()
    g = _lib.region_grid(N, rn)
    R, P = g.regions_side ** 2, g.s * g.s
    st8 = synth.nystrom_state(D, heads, tag="bench/ntrans")
    d, w = _lib.NystromDesc(), _lib.NystromWeights()
    d.dim, d.heads, d.dim_head, d.num_landmarks, d.pinv_iterations, d.residual, d.residual_conv_kernel = D, heads, 64, 256, 6, 1, 33
    keep = [torch.from_numpy(st8[k]).to(DEV).contiguous() for k in NR.NYS_KEYS]
    w.qkv_w, w.out_w, w.out_b, w.conv_w = (t.data_ptr() for t in keep)
    x = torch.from_numpy(synth.nystrom_input(R * P, D, tag="bench/ntrans")).to(DEV).reshape(R, P, D).contiguous()
    dyr = torch.from_numpy(synth.normal("bench/ntrans_train/dyr", (R, P, D))).to(DEV)
    y, dx_b, dx_l = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    gb = [torch.empty_like(t) for t in keep]
    gl = [torch.empty_like(t) for t in keep]
    gsb, gsl = _lib.NystromGrads(), _lib.NystromGrads()
    gsb.qkv_w, gsb.out_w, gsb.out_b, gsb.conv_w = (t.data_ptr() for t in gb)
    gsl.qkv_w, gsl.out_w, gsl.out_b, gsl.conv_w = (t.data_ptr() for t in gl)
    sb, wb, s1, w1 = (C.c_size_t() for _ in range(4))
    _lib.check(lib.rrt_nystrom_batched_train_sizes(C.byref(d), R, P, C.byref(sb), C.byref(wb)), "sizes")
    _lib.check(lib.rrt_nystrom_train_sizes(C.byref(d), P, C.byref(s1), C.byref(w1)), "sizes")
    stash_b = torch.empty(sb.value, dtype=torch.uint8, device=DEV)
    ws_b = torch.empty(wb.value, dtype=torch.uint8, device=DEV)
    stash_l = torch.empty((R, s1.value), dtype=torch.uint8, device=DEV)
    ws_1 = torch.empty(w1.value, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.rrt_nystrom_attention_batched_forward_train_f32(C.byref(d), C.byref(w), x.data_ptr(), y.data_ptr(), R, P,
                                                                   stash_b.data_ptr(), stash_b.numel(), stream), "forward")
    for r in range(R):
        _lib.check(lib.rrt_nystrom_attention_forward_train_f32(C.byref(d), C.byref(w), x[r].data_ptr(), y[r].data_ptr(), P,
                                                               stash_l[r].data_ptr(), s1.value, stream), "forward")

    def batched():
        _lib.check(lib.rrt_nystrom_attention_batched_backward_f32(C.byref(d), C.byref(w), x.data_ptr(), dyr.data_ptr(),
                                                                  stash_b.data_ptr(), stash_b.numel(), C.byref(gsb), dx_b.data_ptr(),
                                                                  R, P, ws_b.data_ptr(), ws_b.numel(), stream), "batched")

    def loop():
        for r in range(R):        # (each call WRITES its parameter gradients: a real loop would also have to add them up)
            _lib.check(lib.rrt_nystrom_attention_backward_f32(C.byref(d), C.byref(w), x[r].data_ptr(), dyr[r].data_ptr(),
                                                              stash_l[r].data_ptr(), s1.value, C.byref(gsl), dx_l[r].data_ptr(), P,
                                                              ws_1.data_ptr(), ws_1.numel(), stream), "single")

    for _ in range(2):
        batched()
        loop()
    torch.cuda.synchronize()
    t_b, t_l = [], []
    for _ in range(reps):
        t_b.append(timed(batched))
        t_l.append(timed(loop))
    rel = float((dx_l - dx_b).abs().max() / dx_b.abs().max())
    lines += [f"one attention layer's backward on the {R} regions of {P} tokens ({(P + 255) // 256 * 256} padded), {heads} heads x 64:",
              f"  rrt_nystrom_attention_batched_backward_f32, b = {R}      {med(t_b)}",
              f"  host loop of {R} rrt_nystrom_attention_backward_f32 calls {med(t_l)}   ratio "
              f"{statistics.median(t_l) / statistics.median(t_b):.2f}x",
              f"  (the loop's values are wrong -- a scale per region: max |dx loop - dx batched| / max |dx batched| = {rel:.2e})",
              f"  batched stash {sb.value} bytes ({sb.value / 2 ** 20:.1f} MiB), backward workspace {wb.value} bytes "
              f"({wb.value / 2 ** 20:.1f} MiB); one region: stash {s1.value}, workspace {w1.value} bytes"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
