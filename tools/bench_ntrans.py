"""The Nystrom ablations of RRTEncoder on the MI355X: ms per bag of RRTEncoder(attn='ntrans') and RRTEncoder(region_attn='ntrans')
(one rrt_encoder_nystrom_forward_f32 call each) against

  * the same encoder evaluated with eager PyTorch ops in fp32 on the same GPU (tests/ntrans_ref.py, the restatement the tests
    use), and
  * for the region mode, one attention layer as a HOST LOOP of region_num^2 calls of the single-sequence export
    (rrt_nystrom_attention_f32) next to the one batched call (rrt_nystrom_attention_batched_f32) on the same regions.  The loop
    is a speed yardstick only: its values are WRONG (a pseudo-inverse scale per region instead of one for all regions).

    python tools/bench_ntrans.py [--out profiles/ntrans.txt] [--n 9000] [--region-num 8] [--reps 30]

Timing: HIP events on the stream around each repetition after warm-up, four distinct bags cycled, the variants alternating
repetition by repetition; medians (min-max) are reported."""
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
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ntrans.py needs the MI355X: no HIP device visible")
    torch.set_grad_enabled(False)                               # inference: the ablations have no backward
    N, D, rn, reps = a.n, a.dim, a.region_num, max(10, a.reps)
    heads = D // 64
    bags = [torch.from_numpy(synth.bag(N, D, tag=f"bench/ntrans{i}")).to(DEV) for i in range(4)]
    lines = [f"RRTEncoder(mlp_dim={D}, n_heads={heads}, region_num={rn}), N = {N}, {torch.cuda.get_device_name(0)}; ms per bag, median "
             f"(min-max) of {reps} alternating repetitions, 4 bags cycled, exact fp32"]
    for label, extra in (("attn='ntrans' (whole bag, b = 1)", dict(attn="ntrans")),
                         (f"region_attn='ntrans' ({rn * rn} regions as the batch)", dict(region_attn="ntrans", region_num=rn))):
        cfg = dict(mlp_dim=D, n_heads=heads, crmsa_heads=heads, **extra)
        state = NC.ntrans_state(cfg)
        enc = RRTEncoder(**cfg)
        enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
        enc = enc.to(DEV).eval()
        sd = {k: v.detach() for k, v in enc.state_dict().items()}
        it = [0]

        def hip():
            it[0] += 1
            with torch.no_grad():
                return enc(bags[it[0] % 4])

        def eager():
            it[0] += 1
            with torch.no_grad():
                return NR.encoder(bags[it[0] % 4], sd, cfg, dtype=torch.float32)

        for _ in range(3):
            hip()
            eager()
        torch.cuda.synchronize()
        diff = float((enc(bags[0]) - NR.encoder(bags[0], sd, cfg, dtype=torch.float32)).abs().max())
        t_hip, t_eager = [], []
        for _ in range(reps):                                   # alternate: clock drift hits both alike
            t_hip.append(timed(hip))
            t_eager.append(timed(eager))
        lines += [f"{label}",
                  f"  one rrt_encoder_nystrom_forward_f32 call          {med(t_hip)}",
                  f"  eager PyTorch fp32 on the same GPU (ntrans_ref)   {med(t_eager)}   ratio "
                  f"{statistics.median(t_eager) / statistics.median(t_hip):.2f}x",
                  f"  max |difference| between the two on one bag: {diff:.2e}"]

    # ---- one region-mode attention layer: the batched call against a host loop over the regions
    lib = _lib.load()
    g = _lib.region_grid(N, rn)
    R, P = g.regions_side ** 2, g.s * g.s
    st8 = synth.nystrom_state(D, heads, tag="bench/ntrans")
    d, w = _lib.NystromDesc(), _lib.NystromWeights()
    d.dim, d.heads, d.dim_head, d.num_landmarks, d.pinv_iterations, d.residual, d.residual_conv_kernel = D, heads, 64, 256, 6, 1, 33
    keep = [torch.from_numpy(st8[k]).to(DEV).contiguous() for k in NR.NYS_KEYS]
    w.qkv_w, w.out_w, w.out_b, w.conv_w = (t.data_ptr() for t in keep)
    x = torch.from_numpy(synth.nystrom_input(R * P, D, tag="bench/ntrans")).to(DEV).reshape(R, P, D).contiguous()
    y_b, y_l = torch.empty_like(x), torch.empty_like(x)
    need = C.c_size_t()
    _lib.check(lib.rrt_nystrom_batched_workspace_size(C.byref(d), R, P, C.byref(need)), "size")
    ws_b = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rrt_nystrom_workspace_size(C.byref(d), P, C.byref(need)), "size")
    ws_1 = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def batched():
        _lib.check(lib.rrt_nystrom_attention_batched_f32(C.byref(d), C.byref(w), x.data_ptr(), y_b.data_ptr(), R, P, ws_b.data_ptr(),
                                                         ws_b.numel(), stream), "batched")

    def loop():
        for r in range(R):
            _lib.check(lib.rrt_nystrom_attention_f32(C.byref(d), C.byref(w), x[r].data_ptr(), y_l[r].data_ptr(), P, ws_1.data_ptr(),
                                                     ws_1.numel(), stream), "single")

    for _ in range(3):
        batched()
        loop()
    torch.cuda.synchronize()
    t_b, t_l = [], []
    for _ in range(reps):
        t_b.append(timed(batched))
        t_l.append(timed(loop))
    rel = float((y_l - y_b).abs().max() / y_b.abs().max())
    lines += [f"one attention layer on the {R} regions of {P} tokens ({(P + 255) // 256 * 256} padded), {heads} heads x 64:",
              f"  rrt_nystrom_attention_batched_f32, b = {R}            {med(t_b)}",
              f"  host loop of {R} rrt_nystrom_attention_f32 calls      {med(t_l)}   ratio "
              f"{statistics.median(t_l) / statistics.median(t_b):.2f}x",
              f"  (the loop's values are wrong -- a scale per region: max |loop - batched| / max |batched| = {rel:.2e})"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
