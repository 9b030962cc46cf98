"""ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL heads on the MI355X, ms per slide at N = 9000 x 1024 for three paths:
(a) the one-call path (rrt_bagmil_forward_f32 through forward_bag), (b) the eager torch head behind the same embedding +
encoder (the reference's op sequence for the tail), (c) the composition of the exports the library had before these heads
-- the library GEMM for the embedding, the encoder, then rrt_pool_predict_f32 / rrt_instance_max_f32 / torch ops for the tail.

    python tools/bench_bagmil.py [--out profiles/bagmil.txt] [--n 9000] [--input-dim 1024] [--repeats 3]

Timing: HIP events around batches of calls after warm-up; the paths ALTERNATE batch by batch and the median batch of each is
reported; the whole measurement is repeated ``--repeats`` times so that the run-to-run spread stands next to the medians.
"""
import argparse
import ctypes as C
import math
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rrt_mil_amd  # noqa: E402,F401
from rrt_mil_amd import ABMIL, GatedABMIL, IBMIL, MaxMIL, MeanMIL, RRTEncoder, _lib, synth  # noqa: E402
from rrt_mil_amd._head import instance_max  # noqa: E402
from bench_clam import alternate  # noqa: E402

DEV = "cuda:0"


def pool_predict(y, a, b, c, cls, act, pooled=None):
    """rrt_pool_predict_f32 on y (N, 512): the attention pool + predictor as one library call (an export older than the heads)"""
    lib = _lib.load()
    n, d = y.shape
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    need = C.c_size_t()
    _lib.check(lib.rrt_pool_workspace_size(n, d, a.out_features, int(b is not None), C.byref(need)), "rrt_pool_workspace_size")
    ws = torch.empty(need.value, dtype=torch.uint8, device=y.device)
    logits = torch.empty(cls.out_features, device=y.device)
    _lib.check(lib.rrt_pool_predict_f32(y.data_ptr(), p(a.weight), p(a.bias), p(b.weight) if b is not None else None,
                                        p(b.bias) if b is not None else None, p(c.weight), p(c.bias), p(cls.weight), p(cls.bias),
                                        p(pooled), logits.data_ptr(), None, 0, n, d, a.out_features, act, cls.out_features, 0,
                                        ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "rrt_pool_predict_f32")
    return logits


def deconf(m, M):
    q, k = m.W_q(M), m.W_k(m.confounder_feat)
    a = F.softmax(torch.mm(k, q.t()) / math.sqrt(k.shape[1]), 0)
    return m.head(torch.cat((M, torch.mm(a.t(), m.confounder_feat)), 1))


def tails(kind, m):
    """(eager tail, composed tail): y (N, 512) -> logits"""
    if kind == "attmil":
        att, cls = m.attention, m.classifier[0]
        return (lambda y: m.classifier(torch.mm(F.softmax(att(y).t(), 1), y)),
                lambda y: pool_predict(y, att[0], None, att[2], cls, _lib.ACT_TANH))
    if kind == "gattmil":
        cls = m.classifier[0]
        return (lambda y: m.classifier(torch.mm(F.softmax(m.attention_c(m.attention_a(y) * m.attention_b(y)).t(), 1), y)),
                lambda y: pool_predict(y, m.attention_a[0], m.attention_b[0], m.attention_c, cls, m._pool_act))
    if kind == "ibmil":
        att = m.attention
        pooled = torch.empty(512, device=DEV)
        # the composition: the pool as one call with its pooled row out (the predictor's rows are W_q's: they are not used)
        return (lambda y: deconf(m, torch.mm(F.softmax(att(y).t(), 1), y)),
                lambda y: (pool_predict(y, att[0], None, att[2], m.W_q, _lib.ACT_TANH, pooled=pooled), deconf(m, pooled[None]))[1])
    cls = m._classifier()
    if kind == "meanmil":
        return (lambda y: cls(y).mean(0, keepdim=True), lambda y: F.linear(y.mean(0, keepdim=True), cls.weight, cls.bias))
    return (lambda y: cls(y).max(0)[0][None], lambda y: instance_max(y, cls.weight, cls.bias)[0][None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--input-dim", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    N, ind = a.n, a.input_dim
    lines = [f"plain MIL heads around RRTEncoder(), N = {N}, input_dim = {ind}, fp32, {torch.cuda.get_device_name(0)}; ms per slide, "
             f"median (min-max) of 9 alternating batches of 20, {a.repeats} repeats"]
    x = torch.from_numpy(synth.bag(N, ind, tag="bench/bagmil", nonneg=True)).to(DEV)
    tmp = tempfile.TemporaryDirectory()
    conf = os.path.join(tmp.name, "conf.npy")
    np.save(conf, (synth.normal("bench/bagmil/conf", (8, 512)) * 0.7).astype(np.float32))
    torch.manual_seed(0)
    heads = {"attmil": lambda: ABMIL(ind, 2, 0., "relu", rrt=RRTEncoder()), "gattmil": lambda: GatedABMIL(512, rrt=RRTEncoder()),
             "ibmil": lambda: IBMIL(2, ind, 0., conf, rrt=RRTEncoder()), "meanmil": lambda: MeanMIL(ind, 2, False, rrt=RRTEncoder()),
             "maxmil": lambda: MaxMIL(ind, 2, False, rrt=RRTEncoder())}
    names = {"a": "one call", "b": "eager head", "c": "composition"}
    for kind, make in heads.items():
        if kind in ("gattmil", "maxmil") and ind != 1024:
            lines.append(f"{kind:8s} skipped: its embedding is Linear(1024, 512)")
            continue
        m = make().to(DEV).eval()
        eager_tail, composed_tail = tails(kind, m)

        def one_call():
            with torch.no_grad():
                return m.forward_bag(x)

        def eager():
            with torch.no_grad():
                return eager_tail(m._embed_encode(x))

        def composed():
            with torch.no_grad():
                return composed_tail(m._embed_encode(x))
        ref = one_call()
        for name, fn in (("eager", eager), ("composition", composed)):
            err = float((fn().reshape(-1) - ref.reshape(-1)).abs().max())
            assert err < 1e-3, (kind, name, err)
        for rep in range(a.repeats):
            r = alternate({"a": one_call, "b": eager, "c": composed})
            base = r["a"][0]
            lines.append(f"{kind:8s} repeat {rep}   " + "   ".join(
                f"({k}) {names[k]} {v[0] / 1e3:7.4f} ({v[1] / 1e3:.4f}-{v[2] / 1e3:.4f})" + ("" if k == "a" else f" {v[0] / base:.2f}x")
                for k, v in r.items()))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
