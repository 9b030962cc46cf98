"""One TransMIL training step on the MI355X: forward + backward with all parameter gradients of the ``enable_training()`` model
(the layer path: torch ops around the HIP Nystrom attention, csrc/nystrom.hip + csrc/nystrom_bwd.hip), of the
``enable_training(one_call=True)`` model (ONE rrt_transmil_forward_train_f32 and ONE rrt_transmil_backward_f32 call) and of the
eager restatement (tests/nystrom_ref.py in fp32 on the same GPU under
autograd), and the per-stage table of one Nystrom layer's backward at that size.

    python tools/bench_transmil_train.py [--out profiles/transmil_train.txt] [--n 9000] [--input-dim 1024] [--reps 20]
                                         [--layer2 row|full|both]

The cls-row tail's A/B drives the two export families directly, with preallocated stash, workspace and gradients and the loss
as a torch op in between: --layer2 row is the tail (rrt_debug_transmil_*_row: layer 2's output stage and to_out for the cls row
alone), --layer2 full the full-row stages instead (rrt_transmil_*, what the step uses); --layer2 both (the default) times both
in the same alternation and reports the difference.

Timing as tools/bench_transmil.py: HIP events on the stream around each repetition after warm-up, four distinct bags cycled,
the variants alternating repetition by repetition; medians (min-max) are reported.  The per-stage rows time each backward
stage entry point alone (events around batches of 5 calls, launch included) on tensors of the layer's shapes; FLOPs are counted
from the shapes of this decomposition and the share is of the 157.3 TFLOP/s fp32 matrix peak.
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layer2", choices=("row", "full", "both"), default="both")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_transmil_train.py needs the MI355X: no HIP device visible")
    N, reps = a.n, max(10, a.reps)
    state = synth.transmil_state(a.input_dim, 2)
    model = TransMIL(a.input_dim, 2, False, "relu")
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    model = model.to(DEV).eval().enable_training()
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    import copy
    step_model = copy.deepcopy(model).enable_training(one_call=True)      # the same parameters in a model of its own
    kinds = ("row", "full") if a.layer2 == "both" else (a.layer2,)
    bags = [torch.from_numpy(synth.bag(N, a.input_dim, tag=f"bench/transmil{i}", nonneg=True)).to(DEV) for i in range(4)]
    label = torch.tensor([1], device=DEV)
    it = [0]

    def hip():
        it[0] += 1
        model.zero_grad(set_to_none=True)
        F.cross_entropy(model(bags[it[0] % 4]), label).backward()

    def module_step():
        it[0] += 1
        step_model.zero_grad(set_to_none=True)
        F.cross_entropy(step_model(bags[it[0] % 4]), label).backward()

    def module_fwd():
        it[0] += 1
        return step_model(bags[it[0] % 4])

    def driver(kind):
        """the step through one export family, called directly: (run, forward only, gradients, stash bytes, workspace bytes)"""
        lib = _lib.load()
        sizes, fwd_fn, bwd_fn = ((lib.rrt_debug_transmil_train_sizes_row, lib.rrt_debug_transmil_forward_train_row_f32,
                                  lib.rrt_debug_transmil_backward_row_f32) if kind == "row" else
                                 (lib.rrt_transmil_train_sizes, lib.rrt_transmil_forward_train_f32, lib.rrt_transmil_backward_f32))
        keep = []
        d, w = step_model._desc_weights(keep)
        params = step_model._step_params()
        sb, wb = C.c_size_t(), C.c_size_t()
        _lib.check(sizes(C.byref(d), N, C.byref(sb), C.byref(wb)), "train_sizes")
        stash = torch.empty(sb.value, dtype=torch.uint8, device=DEV)
        wsp = torch.empty(wb.value, dtype=torch.uint8, device=DEV)
        grads = [torch.empty_like(p_) for p_ in params]
        gs = _lib.TransmilGrads()
        slots = (C.c_void_p * len(grads)).from_buffer(gs)
        for i_, g_ in enumerate(grads):
            slots[i_] = g_.data_ptr()
        logits = torch.empty((1, 2), device=DEV)
        stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

        def fwd():
            it[0] += 1
            x = bags[it[0] % 4]
            _lib.check(fwd_fn(C.byref(d), C.byref(w), x.data_ptr(), logits.data_ptr(), N, stash.data_ptr(), stash.numel(), 0.0, 0.0,
                              0, stream()), "forward_train")
            return x

        def run():
            x = fwd()
            lg = logits.detach().clone().requires_grad_(True)
            F.cross_entropy(lg, label).backward()
            _lib.check(bwd_fn(C.byref(d), C.byref(w), x.data_ptr(), lg.grad.data_ptr(), stash.data_ptr(), stash.numel(),
                              C.byref(gs), None, N, wsp.data_ptr(), wsp.numel(), 0.0, 0.0, 0, stream()), "backward")
        return run, fwd, grads, sb.value, wb.value, keep      # (keep: the weight tensors the struct points to)

    drivers = {k: driver(k) for k in kinds}
    step_fns = {k: (v[0], v[1]) for k, v in drivers.items()}

    def eager():
        it[0] += 1
        for v in sd.values():
            v.grad = None
        F.cross_entropy(R.transmil(bags[it[0] % 4], sd, "relu", dtype=torch.float32, device=DEV)["logits"][None], label).backward()

    def fwd_hip():
        it[0] += 1
        return model(bags[it[0] % 4])

    def fwd_eager():
        it[0] += 1
        return R.transmil(bags[it[0] % 4], sd, "relu", dtype=torch.float32, device=DEV)["logits"]

    for _ in range(3):
        hip()
        eager()
        module_step()
        for run, _ in step_fns.values():
            run()
    torch.cuda.synchronize()
    it[0] = 0
    hip()
    it[0] = 0
    eager()
    worst = max(float((p.grad - sd[k].grad).abs().max() / sd[k].grad.abs().max()) for k, p in model.named_parameters())
    it[0] = 0
    module_step()
    worst_module = max(float((p.grad - sd[k].grad).abs().max() / sd[k].grad.abs().max()) for k, p in step_model.named_parameters())
    worst_step = {}
    by_id = {id(p_): k for k, p_ in step_model.named_parameters()}
    for kind, (run, _) in step_fns.items():
        it[0] = 0
        run()
        torch.cuda.synchronize()
        worst_step[kind] = max(float((g_ - sd[by_id[id(p_)]].grad).abs().max() / sd[by_id[id(p_)]].grad.abs().max())
                               for p_, g_ in zip(step_model._step_params(), drivers[kind][2]))
    t_hip, t_eager, f_hip, f_eager = [], [], [], []
    t_step, f_step = {k: [] for k in step_fns}, {k: [] for k in step_fns}
    t_mod, f_mod = [], []
    for _ in range(reps):                                   # alternate: clock drift hits all alike
        t_hip += timed(hip, 1)
        t_eager += timed(eager, 1)
        t_mod += timed(module_step, 1)
        for kind, (run, fwd) in step_fns.items():
            t_step[kind] += timed(run, 1)
        f_hip += timed(fwd_hip, 1)
        f_eager += timed(fwd_eager, 1)
        f_mod += timed(module_fwd, 1)
        for kind, (run, fwd) in step_fns.items():
            f_step[kind] += timed(fwd, 1)
    side = math.isqrt(N - 1) + 1
    rows = 1 + side * side
    npad = (rows + 255) // 256 * 256
    mh, me = statistics.median(t_hip), statistics.median(t_eager)
    lines = [f"TransMIL(input_dim={a.input_dim}, n_classes=2, act='relu').enable_training(), eval(), N = {N} ({rows} rows, {npad} "
             f"padded), fp32, {torch.cuda.get_device_name(0)}; one training step = forward + cross-entropy + backward with all 25 "
             f"parameter gradients; ms per step, median (min-max) of {reps} alternating repetitions, 4 bags cycled",
             f"layer path with the HIP Nystrom attention (forward-with-stash + backward)   {med(t_hip)}   {1e3 / mh:7.1f} steps/s",
             f"eager PyTorch fp32 under autograd on the same GPU (nystrom_ref)             {med(t_eager)}   {1e3 / me:7.1f} steps/s"
             f"   ratio {me / mh:.2f}x",
             f"  of which the forward with the graph recorded: HIP path {med(f_hip)}, eager {med(f_eager)}",
             f"worst parameter-gradient difference between the two on one bag, relative to the gradient's largest entry: {worst:.2e}"]
    def overlap(u, v):
        return "ranges overlap" if min(u) <= max(v) and min(v) <= max(u) else "ranges do not overlap"

    mm = statistics.median(t_mod)
    sb, wb = C.c_size_t(), C.c_size_t()
    d_t, _w = step_model._desc_weights([])
    _lib.check(_lib.load().rrt_transmil_train_sizes(C.byref(d_t), N, C.byref(sb), C.byref(wb)), "rrt_transmil_train_sizes")
    lines += [f"one-call step, enable_training(one_call=True) (rrt_transmil_forward_train_f32 + rrt_transmil_backward_f32)   "
              f"{med(t_mod)}   {1e3 / mm:7.1f} steps/s   layer path / this = {mh / mm:.3f}x ({overlap(t_mod, t_hip)})",
              f"  of which the forward with the graph recorded: {med(f_mod)}; stash {sb.value / 1e6:.1f} MB, backward workspace "
              f"{wb.value / 1e6:.1f} MB; worst parameter-gradient difference to eager {worst_module:.2e}",
              "the two export families called directly (preallocated stash, workspace and gradients; no dx; the loss a torch op):"]
    names = {"row": "  layer 2 on the cls-row tail (rrt_debug_transmil_*_row)   ",
             "full": "  layer 2 on the full-row stages (rrt_transmil_*, the step)"}
    for kind in step_fns:
        ms = statistics.median(t_step[kind])
        lines += [f"{names[kind]}   {med(t_step[kind])}   {1e3 / ms:7.1f} steps/s; forward only {med(f_step[kind])}; stash "
                  f"{drivers[kind][3] / 1e6:.1f} MB; worst parameter-gradient difference to eager {worst_step[kind]:.2e}"]
    if len(step_fns) == 2:
        dr, df = statistics.median(t_step["row"]), statistics.median(t_step["full"])
        lines.append(f"cls-row tail against the full-row stages: {df - dr:+.3f} ms per step in the tail's favour "
                     f"({overlap(t_step['row'], t_step['full'])}); the stage table's to_out linear backward + output_backward below "
                     f"are what the tail replaces in the backward")
    lines.append("")

    # ---- one Nystrom layer's backward, stage by stage
    lib, h, d, m, dim = _lib.load(), 8, 64, 256, 512
    hd = h * d
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s, sc=1.0: torch.randn(*s, device=DEV, generator=g) * sc   # noqa: E731
    desc = _lib.NystromDesc()
    desc.dim, desc.heads, desc.dim_head, desc.num_landmarks, desc.pinv_iterations, desc.residual = dim, h, d, m, 6, 1
    desc.residual_conv_kernel = 33
    x, wq, wo, bo = rnd(rows, dim), rnd(3 * hd, dim, sc=dim ** -0.5), rnd(dim, hd, sc=hd ** -0.5), rnd(dim, sc=0.05)
    conv = rnd(h, 33, sc=33 ** -0.5)
    w = _lib.NystromWeights()
    w.qkv_w, w.out_w, w.out_b, w.conv_w = wq.data_ptr(), wo.data_ptr(), bo.data_ptr(), conv.data_ptr()
    sb, wb, need = C.c_size_t(), C.c_size_t(), C.c_size_t()
    _lib.check(lib.rrt_nystrom_train_sizes(C.byref(desc), rows, C.byref(sb), C.byref(wb)), "rrt_nystrom_train_sizes")
    stash = torch.empty(sb.value, dtype=torch.uint8, device=DEV)
    wsb = torch.empty(wb.value, dtype=torch.uint8, device=DEV)
    y, dy, dx = torch.empty(rows, dim, device=DEV), rnd(rows, dim), torch.empty(rows, dim, device=DEV)
    gq, go, gb, gc = torch.empty_like(wq), torch.empty_like(wo), torch.empty_like(bo), torch.empty_like(conv)
    gr = _lib.NystromGrads()
    gr.qkv_w, gr.out_w, gr.out_b, gr.conv_w = gq.data_ptr(), go.data_ptr(), gb.data_ptr(), gc.data_ptr()
    st = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    p = lambda t: t.data_ptr()   # noqa: E731
    # stage tensors of a real forward (the stash is opaque: run the stage entry points once)
    qkv = torch.zeros(npad, 3 * hd, device=DEV)
    pad = npad - rows
    _lib.check(lib.rrt_linear_f32(p(x), p(wq), None, p(qkv) + pad * 3 * hd * 4, rows, 3 * hd, dim, hd, 0.125, 0, st()), "qkv")
    ql, kl, av, wz = (torch.empty(h, m, d, device=DEV) for _ in range(4))
    a2, z = (torch.empty(h, m, m, device=DEV) for _ in range(2))
    o = torch.empty(npad, hd, device=DEV)
    _lib.check(lib.rrt_nystrom_landmark_attn_workspace_size(npad, h, C.byref(need)), "ws")
    ws_l = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rrt_nystrom_pinv_workspace_size(h, C.byref(need)), "ws")
    ws_p = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rrt_nystrom_landmarks_f32(p(qkv), p(ql), p(kl), npad, h, st()), "landmarks")
    _lib.check(lib.rrt_nystrom_landmark_sim_f32(p(ql), p(kl), p(a2), h, st()), "sim")
    _lib.check(lib.rrt_nystrom_landmark_attn_f32(p(qkv), p(ql), p(av), npad, h, p(ws_l), ws_l.numel(), st()), "lattn")
    _lib.check(lib.rrt_nystrom_pinv_f32(p(a2), p(z), h, 6, p(ws_p), ws_p.numel(), st()), "pinv")
    _lib.check(lib.rrt_nystrom_zav_f32(p(z), p(av), p(wz), h, st()), "zav")
    _lib.check(lib.rrt_nystrom_output_f32(p(qkv), p(kl), p(wz), p(conv), p(o), npad, h, 33, st()), "output")
    d_o, d_qkv = rnd(npad, hd), torch.zeros(npad, 3 * hd, device=DEV)
    d_kl, d_wz, d_av, d_ql = (torch.empty(h, m, d, device=DEV) for _ in range(4))
    d_z, d_conv = rnd(h, m, m, sc=0.01), torch.empty(h, 33, device=DEV)

    def ws_of(fn, *args):
        _lib.check(fn(*args, C.byref(need)), fn.__name__)
        return torch.empty(need.value, dtype=torch.uint8, device=DEV)

    ws_o = ws_of(lib.rrt_nystrom_output_backward_workspace_size, npad, h)
    ws_a = ws_of(lib.rrt_nystrom_landmark_attn_backward_workspace_size, npad, h)
    ws_i = ws_of(lib.rrt_nystrom_pinv_sim_backward_workspace_size, h, 6)
    ws_lin = max(ws_of(lib.rrt_linear_backward_workspace_size, rows, 3 * hd, dim),
                 ws_of(lib.rrt_linear_backward_workspace_size, rows, dim, hd), key=lambda t: t.numel())
    d_rows = p(d_qkv) + pad * 3 * hd * 4
    stages = [
        ("to_out linear backward (dX, dW, db)", 2 * 2.0 * rows * hd * dim,
         lambda: lib.rrt_linear_backward_f32(p(dy), p(o) + pad * hd * 4, p(wo), p(d_o) + pad * hd * 4, p(go), p(gb), rows, dim, hd,
                                             0, p(ws_lin), ws_lin.numel(), st())),
        ("output_backward (+ stencil adjoint)", 10.0 * h * npad * m * d + 4.0 * 33 * npad * hd,
         lambda: lib.rrt_nystrom_output_backward_f32(p(qkv), p(kl), p(wz), p(conv), p(d_o), p(d_qkv), p(d_kl), p(d_wz),
                                                     p(d_conv), npad, h, 33, p(ws_o), ws_o.numel(), st())),
        ("zav_backward", 4.0 * h * m * m * d, lambda: lib.rrt_nystrom_zav_backward_f32(p(z), p(av), p(d_wz), p(d_z), p(d_av), h, st())),
        ("landmark_attn_backward (+ a3 v again)", (4.0 + 10.0) * h * m * npad * d,
         lambda: lib.rrt_nystrom_landmark_attn_backward_f32(p(qkv), p(ql), p(d_av), p(d_qkv), p(d_ql), npad, h, p(ws_a),
                                                            ws_a.numel(), st())),
        # a2 again; 65 products of the forward sweep (terms, iterates, tangent), 69 of the reverse one; d_ql, d_kl
        ("pinv_sim_backward, 6 iterations", h * (2.0 * m * m * d + 134 * 2.0 * m ** 3 + 4.0 * m * m * d),
         lambda: lib.rrt_nystrom_pinv_sim_backward_f32(p(ql), p(kl), p(d_z), p(d_ql), p(d_kl), h, 6, p(ws_i), ws_i.numel(), st())),
        ("landmarks_backward", 2.0 * npad * 2 * hd,
         lambda: lib.rrt_nystrom_landmarks_backward_f32(p(d_ql), p(d_kl), p(d_qkv), npad, h, st())),
        ("to_qkv linear backward (dX, dW)", 2 * 2.0 * rows * dim * 3 * hd,
         lambda: lib.rrt_linear_backward_f32(d_rows, p(x), p(wq), p(dx), p(gq), None, rows, 3 * hd, dim, 0, p(ws_lin),
                                             ws_lin.numel(), st())),
    ]
    lines.append(f"one Nystrom layer's backward at {rows} rows ({npad} padded), 8 heads x 64, 256 landmarks: each stage entry point "
                 f"alone, ms per call (median of {reps} batches of 5), FLOPs of this decomposition (2 x multiply-adds of its matrix "
                 f"products, recomputation included), share of the {PEAK_TF} TFLOP/s fp32 matrix peak")
    total_ms, total_fl = 0.0, 0.0
    for name, flops, fn in stages:
        def call(fn=fn, name=name):
            _lib.check(fn(), name)
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        t = statistics.median(timed(call, reps, per=5))
        total_ms, total_fl = total_ms + t, total_fl + flops
        lines.append(f"  {name:40s} {t:8.3f} ms  {flops / 1e9:7.2f} GFLOP  {flops / t / 1e9:7.1f} TFLOP/s  "
                     f"{100 * flops / t / 1e9 / PEAK_TF:5.1f} %")
    lines.append(f"  {'sum of the stages':40s} {total_ms:8.3f} ms  {total_fl / 1e9:7.2f} GFLOP  {total_fl / total_ms / 1e9:7.1f} TFLOP/s  "
                 f"{100 * total_fl / total_ms / 1e9 / PEAK_TF:5.1f} %")

    def whole_fwd():
        _lib.check(lib.rrt_nystrom_attention_forward_train_f32(C.byref(desc), C.byref(w), p(x), p(y), rows, p(stash), stash.numel(),
                                                               st()), "forward_train")

    def whole_bwd():
        _lib.check(lib.rrt_nystrom_attention_backward_f32(C.byref(desc), C.byref(w), p(x), p(dy), p(stash), stash.numel(),
                                                          C.byref(gr), p(dx), rows, p(wsb), wsb.numel(), st()), "backward")

    whole_fwd()
    whole_bwd()
    torch.cuda.synchronize()
    lines.append(f"  {'rrt_nystrom_attention_forward_train_f32':40s} {statistics.median(timed(whole_fwd, reps, per=5)):8.3f} ms   "
                 f"(stash {sb.value / 1e6:.1f} MB)")
    lines.append(f"  {'rrt_nystrom_attention_backward_f32':40s} {statistics.median(timed(whole_bwd, reps, per=5)):8.3f} ms   "
                 f"(workspace {wb.value / 1e6:.1f} MB)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
