"""MHIM-MIL with the TransMIL baseline on the MI355X: one training step of ``mhim_sattn.MHIM_MIL`` (teacher forward with both
attention rows + vote-fused mask selection + student forward / backward) with ratios 0.6 / 0.2 / 0.02, head = 2 and every
dropout on, at N = 9 000 x 1024 and N = 30 000 x 1024, against an eager fp32 restatement on the same GPU
(SAttention and Nystrom attention in torch ops in the reference's own order of operations, the cls token's own row) in two forms:
  (a) eager, host round trip: per-head topk, scatter_, sum, topk on the device, then the reference's index lists pulled to the
      host, Python set arithmetic, the result uploaded; the student embeds all N rows and gathers;
  (b) eager, device only: the same topk / scatter_ / sum / topk, a boolean mask, boolean indexing
      -- so that the gain is not credited to the round trip alone.
Also, alone: rrt_mask_select_vote_f32 against the eager device-side selection of (b), and the teacher pass with and without the
two attention rows.

    python tools/bench_mhim_sattn.py [--out profiles/mhim_sattn.txt] [--repeats 3] [--ns 9000 30000]

Timing: HIP events around batches of calls after warm-up; the paths ALTERNATE batch by batch, the median batch of each is
reported with its range, the whole measurement is repeated ``--repeats`` times.  Per N the first line checks the device's
selection against the restatement on the rows of that very teacher call (mismatches, exact).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401
from rrt_mil_amd import _lib, mhim_sattn, synth  # noqa: E402
from bench_clam import alternate  # noqa: E402
from bench_mhim import fmt  # noqa: E402
import mhim_ref as MR  # noqa: E402
import mhim_sattn_ref as R  # noqa: E402
import nystrom_ref as NR  # noqa: E402

DEV = "cuda:0"
PARAMS = dict(num_epoch=200, niter_per_ep=100, input_dim=1024, mlp_dim=512, mask_ratio=0.6, mask_ratio_l=0.2, mask_ratio_h=0.02,
              baseline="selfattn", head=2, teacher_init=None)
STEP, HEADS, P_EMB, P_ATTN = 100, 2, 0.25, 0.1


def stage_list(m, ps):
    return MR.stage_plan(ps, m.mask_ratio, m.mask_ratio_l, float(m.mrh_sche[STEP]), m.mask_ratio_hr)


def vote_candidates(attn, largest, k):
    """network.py:497-508 on the device: attn (heads, n) -> the k indices of the most votes (ties as torch.topk leaves them)"""
    idx = torch.topk(attn, k, largest=largest, sorted=False)[1]
    vote = torch.zeros_like(attn).scatter_(1, idx, 1.).sum(0)
    return torch.topk(vote, k, sorted=False)[1]


def kept_host(m, attn):
    """(a): the selected set through host lists and Python sets, as the reference forms it"""
    ps = attn.shape[1]
    sel = set()
    for largest, k, cnt in stage_list(m, ps):
        idx = vote_candidates(attn, largest, k)
        if cnt is not None:
            idx = idx[torch.randperm(k, device=attn.device)[:cnt]]
        sel |= set(idx.tolist())
    return torch.tensor(sorted(set(range(ps)) - sel), device=attn.device)


def kept_device(m, attn):
    """(b): a boolean mask; nothing but the final size visits the host"""
    ps = attn.shape[1]
    sel = torch.zeros(ps, dtype=torch.bool, device=attn.device)
    for largest, k, cnt in stage_list(m, ps):
        idx = vote_candidates(attn, largest, k)
        if cnt is not None:
            idx = idx[torch.randperm(k, device=attn.device)[:cnt]]
        sel[idx] = True
    return torch.nonzero(~sel)[:, 0]


def state_of(m):
    return {k: v for k, v in m.named_parameters()}


def eager_nystrom(x, st, pre, heads, want_row):
    """network.py:184-256 on x (n, 512) in torch ops, in the reference's own order of operations -> (y (n, 512) before the
    dropout, the cls token's own row without its column (heads, n - 1) or None)"""
    n = x.shape[0]
    pad = (256 - n % 256) % 256
    qkv = F.pad(x, (0, 0, pad, 0)) @ st[pre + "to_qkv.weight"].t()
    q, k, v = (t.reshape(n + pad, heads, 64).transpose(0, 1) for t in qkv.chunk(3, dim=-1))
    q = q * 0.125
    l = (n + pad) // 256
    ql, kl = q.reshape(heads, 256, l, 64).sum(2) / l, k.reshape(heads, 256, l, 64).sum(2) / l
    a1, a2, a3 = ((a @ b.transpose(-1, -2)).softmax(-1) for a, b in ((q, kl), (ql, kl), (ql, k)))
    z = NR.pinv_iter(a2, 6)
    out = (a1 @ z) @ (a3 @ v) + F.conv2d(v[None], st[pre + "res_conv.weight"], padding=(16, 0), groups=heads)[0]
    y = (out.transpose(0, 1).reshape(n + pad, -1) @ st[pre + "to_out.0.weight"].t() + st[pre + "to_out.0.bias"])[pad:]
    row = ((a1[:, pad:pad + 1] @ z) @ a3)[:, 0, pad + 1:] if want_row else None
    return y, row


def eager_sattention(y, st, heads, want_rows=False):
    """SAttention.forward (network.py:362-408) in torch ops with the layers' output dropout on -> (cls row (1, 512), [a1, a2])"""
    pre = R.PRE
    h = torch.cat([st[pre + "cls_token"].reshape(1, -1), y])
    rows = []
    for name in ("layer1", "layer2"):
        ln = F.layer_norm(h, (512,), st[f"{pre}{name}.norm.weight"], st[f"{pre}{name}.norm.bias"])
        o, row = eager_nystrom(ln, st, f"{pre}{name}.attn.", heads, want_rows)
        rows.append(row)
        h = h + F.dropout(o, P_ATTN)
        if name == "layer1":
            h = torch.cat([h[:1], R.ppeg(h[1:], st, h.dtype)])
    return F.layer_norm(h[:1], (512,), st[pre + "norm.weight"], st[pre + "norm.bias"]), rows


def eager_embed(m, st, x, train=True):
    return F.dropout(R.embed(x, st, "relu"), P_EMB, training=train)


def eager_step(model, x, kept_fn):
    s, t = model.student, model.teacher
    with torch.no_grad():
        ts = state_of(t)
        tea, rows = eager_sattention(eager_embed(t, ts, x), ts, HEADS, True)
    kept = kept_fn(s, rows[0])
    ss = state_of(s)
    feat, _ = eager_sattention(eager_embed(s, ss, x)[kept], ss, HEADS)
    logits = s.predictor(feat)
    loss = F.cross_entropy(logits, torch.zeros(1, dtype=torch.long, device=x.device)) + 0.5 * s.cl_loss(feat, tea.detach())
    for p in s.parameters():
        p.grad = None
    loss.backward()
    return logits


def hip_step(model, x):
    logits, cls_loss = model(x[None], i=STEP)
    loss = F.cross_entropy(logits, torch.zeros(1, dtype=torch.long, device=x.device)) + 0.5 * cls_loss
    for p in model.student.parameters():
        p.grad = None
    loss.backward()
    return logits


def check_selection(model, x, lines):
    """the device's selection against the restatement on the device's own rows (exact)"""
    n, s = x.shape[0], model.student
    with torch.no_grad():
        _, rows = model.teacher.forward_teacher(x[None], return_attn=True)
    perms = []
    real = s._randperm
    s._randperm = lambda k, device: perms.append(real(k, device)) or perms[-1]
    try:
        lk, ids = s.get_mask(n, STEP, rows)
    finally:
        del s._randperm
    ref_keep, ref_ids = R.get_mask(n, rows[0][0].cpu().numpy(), [p.cpu().numpy() for p in perms], select_inv=False,
                                   mask_ratio=s.mask_ratio, mask_ratio_l=s.mask_ratio_l, mask_ratio_h=float(s.mrh_sche[STEP]),
                                   mask_ratio_hr=s.mask_ratio_hr)
    lines.append(f"N = {n}: len_keep {lk} (restatement {ref_keep}), ids that differ from the restatement: "
                 f"{int((ids[0].cpu().numpy() != ref_ids).sum())} of {n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ns", type=int, nargs="+", default=[9000, 30000])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mhim_sattn.py measures on an MI355X; no HIP device is visible")
    _lib.load()
    name = torch.cuda.get_device_name(0)
    lines = [f"mhim_sattn.MHIM_MIL training step (teacher forward with both rows + vote selection + student forward / backward), "
             f"input_dim 1024, head 2, ratios 0.6 / 0.2 / 0.02, dropout 0.25 / 0.1, fp32, {name}; us per call, median (min-max) of 9 "
             f"alternating batches of 20, {a.repeats} repeats",
             "hip = rrt_mil_amd.mhim_sattn.MHIM_MIL; (a) = eager torch, host list / set round trip; (b) = eager torch, device-side "
             "topk / scatter_ / sum / topk and a boolean mask"]
    torch.manual_seed(0)
    model = mhim_sattn.MHIM_MIL(**PARAMS).to(DEV).train()
    s, t = model.student, model.teacher
    for n in a.ns:
        x = torch.from_numpy(synth.bag(n, 1024, tag="bench/mhim_sattn", nonneg=True)).to(DEV)
        check_selection(model, x, lines)
        with torch.no_grad():
            rows = t.forward_teacher(x[None], return_attn=True)[1][0][0].contiguous()
        plan = stage_list(s, n)
        picks = [(lg, k, None if cnt is None else torch.from_numpy(MR.pick_of(np.random.default_rng(k).permutation(k), k, cnt)).to(DEV))
                 for lg, k, cnt in plan]
        keep_n = int(mhim_sattn.mask_select_vote(rows, picks)[1].item())
        lines.append(f"N = {n}: stages (largest, k, drawn) {plan}, kept {keep_n}")
        for rep in range(a.repeats):
            r = alternate({"hip": lambda: hip_step(model, x), "(a)": lambda: eager_step(model, x, kept_host),
                           "(b)": lambda: eager_step(model, x, kept_device)})
            lines.append(f"  step      repeat {rep}   " + fmt(r, "hip"))
        for rep in range(a.repeats):
            with torch.no_grad():
                r = alternate({"rrt_mask_select_vote_f32": lambda: mhim_sattn.mask_select_vote(rows, picks),
                               "eager device selection": lambda: kept_device(s, rows)})
            lines.append(f"  selection repeat {rep}   " + fmt(r, "rrt_mask_select_vote_f32"))
        for rep in range(a.repeats):
            r = alternate({"teacher with rows": lambda: t.forward_teacher(x[None], return_attn=True),
                           "teacher without": lambda: t.forward_teacher(x[None])})
            lines.append(f"  teacher   repeat {rep}   " + fmt(r, "teacher with rows"))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
