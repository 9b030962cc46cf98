"""DTFD-MIL on the MI355X, per slide at N = 9000 x 1024 with group = 8:
(a) the one-call path (rrt_dtfd_forward_f32 through forward_bag) against (b) an eager torch restatement of the reference's
``test_forward`` on the same GPU (the Python loop over pseudo-bags: index_select / einsum / softmax / sort per group), both
behind the same permutation; and the segmented pool alone (rrt_segment_pool_f32 on a ready embedding and ready scores) against
that eager per-group loop alone.

    python tools/bench_dtfd.py [--out profiles/dtfd.txt] [--n 9000] [--input-dim 1024] [--group 8] [--repeats 3]

Timing: HIP events around batches of calls after warm-up; the paths ALTERNATE batch by batch and the median batch of each is
reported; the whole measurement is repeated ``--repeats`` times so that the run-to-run spread stands next to the medians.
No speed figure here is a pass criterion of any test.
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rrt_mil_amd  # noqa: E402,F401
from rrt_mil_amd import DTFD, synth  # noqa: E402
from rrt_mil_amd.dtfd import _SegmentPool, get_cam_1d, split_sizes  # noqa: E402
from bench_clam import alternate  # noqa: E402

DEV = "cuda:0"


def eager_scores(att, x):
    """Attention.forward(isNorm=False) as plain torch ops"""
    F = torch.nn.functional
    v = torch.tanh(F.linear(x, att.attention_V[0].weight, att.attention_V[0].bias))
    u = torch.sigmoid(F.linear(x, att.attention_U[0].weight, att.attention_U[0].bias))
    return att.attention_weights(v * u).transpose(1, 0)


def eager_tier2(u, rows):
    return u.classifier.fc(torch.mm(torch.softmax(eager_scores(u.attention, rows), 1), rows))


def eager_groups(m, mid, AA, chunks):
    """the loop of test_forward over the pseudo-bags -> the distilled rows"""
    rows = []
    for idx in chunks:
        tmid = mid.index_select(0, idx)
        tAA = torch.softmax(AA.index_select(0, idx), 0)
        tatt = torch.einsum("ns,n->ns", tmid, tAA)
        pooled = torch.sum(tatt, 0).unsqueeze(0)
        cam = torch.transpose(get_cam_1d(m.classifier, tatt.unsqueeze(0)).squeeze(0), 0, 1)
        _, order = torch.sort(torch.softmax(cam, 1)[:, -1], descending=True)
        if m.distill == "MaxMinS":
            rows.append(tmid.index_select(0, torch.cat([order[:1], order[-1:]])))
        elif m.distill == "MaxS":
            rows.append(tmid.index_select(0, order[:1]))
        else:
            rows.append(pooled)
    return torch.cat(rows, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--input-dim", type=int, default=1024)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    N, ind, G = a.n, a.input_dim, a.group
    lines = [f"DTFD-MIL (no encoder), N = {N}, input_dim = {ind}, group = {G}, fp32, {torch.cuda.get_device_name(0)}; us per slide, "
             f"median (min-max) of 9 alternating batches of 20, {a.repeats} repeats"]
    x = torch.from_numpy(synth.bag(N, ind, tag="bench/dtfd", nonneg=True)).to(DEV)
    random.seed(0)
    perm = list(range(N))
    random.shuffle(perm)
    perm = torch.from_numpy(np.array(perm, np.int64)).to(DEV)
    chunks = list(torch.split(perm, split_sizes(N, G)))
    for distill in ("MaxMinS", "MaxS", "AFS"):
        torch.manual_seed(0)
        m = DTFD(1e-4, 1e-5, 10, None, input_dim=ind, group=G, distill=distill).to(DEV).eval()

        def one_call():
            with torch.no_grad():
                return m.forward_bag(x, perm=perm)

        def eager():
            with torch.no_grad():
                mid = torch.relu(torch.nn.functional.linear(x, m.dimReduction.fc1.weight))
                AA = eager_scores(m.attention, mid).squeeze(0)
                return eager_tier2(m.UClassifier, eager_groups(m, mid, AA, chunks))
        err = float((eager() - one_call()).abs().max())
        assert err < 1e-3, (distill, err)
        with torch.no_grad():
            mid = m.dimReduction(x).float().contiguous()
            AA = m.attention(mid, isNorm=False).squeeze(0).contiguous()
        w = m.classifier.fc.weight.detach()

        def pool():
            with torch.no_grad():
                return _SegmentPool.apply(mid, AA, w, G, perm)

        def pool_eager():
            with torch.no_grad():
                return eager_groups(m, mid, AA, chunks)
        for rep in range(a.repeats):
            r = alternate({"a": one_call, "b": eager, "c": pool, "d": pool_eager})
            lines.append(f"{distill:8s} repeat {rep}   (a) one call {r['a'][0]:8.1f} ({r['a'][1]:.1f}-{r['a'][2]:.1f})   (b) eager test_forward "
                         f"{r['b'][0]:8.1f} ({r['b'][1]:.1f}-{r['b'][2]:.1f}) {r['b'][0] / r['a'][0]:.2f}x   (c) segmented pool alone "
                         f"{r['c'][0]:7.1f} ({r['c'][1]:.1f}-{r['c'][2]:.1f})   (d) eager per-group loop {r['d'][0]:7.1f} "
                         f"({r['d'][1]:.1f}-{r['d'][2]:.1f}) {r['d'][0] / r['c'][0]:.2f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
