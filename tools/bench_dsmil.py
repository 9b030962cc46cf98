"""DSMIL head on the MI355X: the one-call forward against (b) the eager head behind the same embedding + encoder and (c) the
composition the layer path runs (rrt_instance_max_f32 + rrt_branch_pool_f32 with y = hid_a = feats + torch's fcc); and the
bag stream alone, one-pass rrt_dsmil_pool_f32 against that composition, on the same feats and critical ids.

    python tools/bench_dsmil.py [--out profiles/dsmil_head.txt] [--n 9000] [--input-dim 1024] [--classes 2]

One bag on one stream, and four bags in flight (forward_bags / four streams).  Timing: HIP events around batches of calls
after warm-up; the variants ALTERNATE batch by batch and the median batch of each is reported, so clock drift hits them alike.
"""
import argparse
import ctypes as C
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rrt_mil_amd  # noqa: E402,F401
from rrt_mil_amd import MILNet, RRTEncoder, _lib, synth  # noqa: E402
from bench_clam import alternate  # noqa: E402

DEV = "cuda:0"


def on_streams(fn, streams):
    """fn once per stream, all in flight; the caller's stream waits for them (what forward_bags does around its bags)"""
    def run():
        cur = torch.cuda.current_stream()
        for s in streams:
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                fn()
        for s in streams:
            cur.wait_stream(s)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--input-dim", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=2)
    a = ap.parse_args()
    N, nc = a.n, a.classes
    lines = [f"DSMIL head, N = {N}, input_dim = {a.input_dim}, C = {nc}, {torch.cuda.get_device_name(0)}; us per call, median "
             "(min-max) of 9 alternating batches of 20"]
    x = torch.from_numpy(synth.bag(N, a.input_dim, tag="bench/dsmil", nonneg=True)).to(DEV)
    torch.manual_seed(0)
    m = MILNet(nc, 0., "relu", input_dim=a.input_dim, rrt=RRTEncoder()).to(DEV).eval()
    streams = [torch.cuda.Stream(DEV) for _ in range(4)]

    def fmt(r, names):
        base = r["a"][0]
        return "   ".join(f"({k}) {names[k]} {v[0]:8.1f} ({v[1]:.1f}-{v[2]:.1f})" + ("" if k == "a" else f" {v[0] / base:.2f}x")
                          for k, v in r.items())
    for mode, dt in (("fp32", None), ("bf16 autocast", torch.bfloat16)):
        ctx = lambda: torch.autocast("cuda", dtype=dt or torch.bfloat16, enabled=dt is not None)   # noqa: E731

        def one_call():
            with torch.no_grad(), ctx():
                return m.forward_bag(x)

        def eager():
            with torch.no_grad(), ctx():
                feats = m._embed(x)
                y = m.rrt(feats).float()
                with torch.autocast("cuda", enabled=False):
                    classes = m.i_classifier(y)
                    return m.b_classifier._eager(feats, classes)[0], classes.max(0)[0]

        def composed():
            with torch.no_grad(), ctx():
                return m._streams(m._embed(x))[0]

        def four_one_call():
            with ctx():
                return m.forward_bags([x, x, x, x], streams=4)
        names = {"a": "one call", "b": "eager head", "c": "composition"}
        lines.append(f"whole forward, one bag       {mode:14s} " + fmt(alternate({"a": one_call, "b": eager, "c": composed}), names))
        r4 = alternate({"a": four_one_call, "b": on_streams(eager, streams), "c": on_streams(composed, streams)})
        lines.append(f"whole forward, four in flight {mode:13s} " + fmt(r4, names) + "   (per FOUR bags)")

    # the bag stream alone on the same feats and critical ids
    lib = _lib.load()
    D, Q = 512, 128
    feats = torch.relu(torch.randn(N, D, device=DEV))
    idx = torch.randint(0, N, (nc,), device=DEV)
    q, fcc = m.b_classifier.q, m.b_classifier.fcc
    qw, qb, fw, fb = q.weight.detach(), q.bias.detach(), fcc.weight.detach(), fcc.bias.detach()
    need, need_b = C.c_size_t(), C.c_size_t()
    _lib.check(lib.rrt_dsmil_pool_workspace_size(N, D, Q, nc, C.byref(need)), "ws")
    _lib.check(lib.rrt_branch_pool_workspace_size(N, D, D, nc, C.byref(need_b)), "ws")

    def slot():
        return dict(ws=torch.empty(need.value, dtype=torch.uint8, device=DEV), wsb=torch.empty(need_b.value, dtype=torch.uint8, device=DEV),
                    logits=torch.empty(nc, device=DEV), A=torch.empty(N, nc, device=DEV), B=torch.empty(nc, D, device=DEV),
                    At=torch.empty(nc, N, device=DEV), raw=torch.empty(nc, N, device=DEV))
    slots = [slot() for _ in range(5)]

    def one_pass(s, with_a):
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.rrt_dsmil_pool_f32(feats.data_ptr(), idx.data_ptr(), qw.data_ptr(), qb.data_ptr(), fw.data_ptr(), fb.data_ptr(),
                                          s["logits"].data_ptr(), s["A"].data_ptr() if with_a else None, s["B"].data_ptr(), None, N, D,
                                          Q, nc, s["ws"].data_ptr(), need.value, st), "rrt_dsmil_pool_f32")

    def composition(s, with_a):
        st = torch.cuda.current_stream().cuda_stream
        q_max = F.linear(feats.index_select(0, idx), qw, qb)
        c_w = torch.mm(q_max, qw) * (1.0 / math.sqrt(Q))
        c_b = torch.mv(q_max, qb) * (1.0 / math.sqrt(Q))
        _lib.check(lib.rrt_branch_pool_f32(feats.data_ptr(), feats.data_ptr(), None, c_w.data_ptr(), c_b.data_ptr(), s["B"].data_ptr(),
                                           s["At"].data_ptr() if with_a else None, s["raw"].data_ptr(), N, D, D, nc,
                                           s["wsb"].data_ptr(), need_b.value, st), "rrt_branch_pool_f32")
        return F.conv1d(s["B"].unsqueeze(0), fw, fb)
    it = [0]

    def rot(fn, with_a):            # four in flight: a workspace set of its own per stream
        def f():
            it[0] = (it[0] + 1) % 4
            fn(slots[it[0]], with_a)
        return f
    for with_a in (False, True):
        tag = "with A" if with_a else "logits + B only"
        names = {"a": "one-pass pool", "b": "composition"}
        r1 = alternate({"a": lambda: one_pass(slots[4], with_a), "b": lambda: composition(slots[4], with_a)}, per_batch=50)
        lines.append(f"bag stream alone, one in flight  ({tag:15s}) " + fmt(r1, names))
        r4 = alternate({"a": on_streams(rot(one_pass, with_a), streams), "b": on_streams(rot(composition, with_a), streams)}, per_batch=50)
        lines.append(f"bag stream alone, four in flight ({tag:15s}) " + fmt(r4, names) + "   (per FOUR)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
