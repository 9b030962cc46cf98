"""MHIM-MIL on the MI355X: one training step of ``MHIM_MIL`` (teacher forward + mask selection + student forward / backward)
with the ratios of Survival/main.py (0.7 / 0.2 / 0.02, dropout 0.25), at N = 9 000 x 1024 and N = 30 000 x 1024, against two
eager torch baselines on the same GPU, both written from tests/mhim_ref.py's algorithm:
  (a) eager, host round trip: topk per stage on the device, the index lists pulled to the host, Python set arithmetic, the
      result uploaded; the student embeds all N rows and gathers;
  (b) eager, device only: stable argsort per order, a boolean mask, boolean indexing; the student embeds all N rows and gathers
      -- so that the gain is not credited to the round trip alone.
Also: rrt_mask_select_f32 alone against the argsorts of (b) alone, and the student's embedding GEMM on the kept rows against
all rows.

    python tools/bench_mhim.py [--out profiles/mhim.txt] [--errors profiles/mhim_errors.txt] [--repeats 3]

Timing: HIP events around batches of calls after warm-up; the paths ALTERNATE batch by batch, the median batch of each is
reported with its range, the whole measurement is repeated ``--repeats`` times.  The error file: the device's selection against
the stable-sort restatement on the device's own attention row (mismatches, exact) and the student against float64 at dropout 0.
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
from rrt_mil_amd import MHIM_MIL, _lib, mhim, synth  # noqa: E402
from rrt_mil_amd.mil import lib_linear  # noqa: E402
from bench_clam import alternate  # noqa: E402
import mhim_ref as R  # noqa: E402

DEV = "cuda:0"
PARAMS = dict(num_epoch=200, niter_per_ep=100, input_dim=1024, mlp_dim=512, mask_ratio=0.7, mask_ratio_l=0.2, mask_ratio_h=0.02,
              baseline="attn", teacher_init=None)
STEP = 100


def pool(m, y):
    """the gated pool of MHIM `m` in eager torch ops: y (n, 512) -> (pooled (1, 512), attn (n,))"""
    att = m.online_encoder.attention
    raw = att.attention_c(att.attention_a(y) * att.attention_b(y))[:, 0]
    attn = F.softmax(raw, dim=0)
    return attn[None] @ y, attn


def stage_list(m, ps):
    return R.stage_plan(ps, m.mask_ratio, m.mask_ratio_l, float(m.mrh_sche[STEP]), m.mask_ratio_hr)


def kept_host(m, attn):
    """(a): the selected set through host lists and Python sets"""
    ps = attn.numel()
    sel = set()
    for largest, k, cnt in stage_list(m, ps):
        idx = torch.topk(attn, k, largest=largest)[1]
        if cnt is not None:
            idx = idx[torch.randperm(k, device=attn.device)[:cnt]]
        sel |= set(idx.tolist())
    return torch.tensor(sorted(set(range(ps)) - sel), device=attn.device)


def kept_device(m, attn):
    """(b): ranks from stable argsorts, a boolean mask, nothing but the final size visits the host"""
    ps = attn.numel()
    sel = torch.zeros(ps, dtype=torch.bool, device=attn.device)
    order = {}
    for largest, k, cnt in stage_list(m, ps):
        if largest not in order:
            order[largest] = torch.argsort(attn, descending=largest, stable=True)
        idx = order[largest][:k]
        if cnt is not None:
            idx = idx[torch.randperm(k, device=attn.device)[:cnt]]
        sel[idx] = True
    return torch.nonzero(~sel)[:, 0]


def eager_step(model, x, kept_fn):
    s, t = model.student, model.teacher
    with torch.no_grad():
        tea, attn = pool(t, t.dp(t.patch_to_emb(x)))
    kept = kept_fn(s, attn)
    feat, _ = pool(s, s.dp(s.patch_to_emb(x))[kept])
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


def fmt(r, base=None):
    return "   ".join(f"{k} {v[0]:8.1f} ({v[1]:.1f}-{v[2]:.1f})" + ("" if base is None or k == base else f" {v[0] / r[base][0]:.2f}x")
                      for k, v in r.items())


def errors(model, x, lines):
    """selection against the restatement on the device's own scores (exact), the student against float64 at dropout 0"""
    n = x.shape[0]
    s, t = model.student, model.teacher
    model.eval()                                                  # dropout off on both sides; the masking path is called directly
    with torch.no_grad():
        tea, attn = t.forward_teacher(x[None], return_attn=True)
    perms = []
    real = s._randperm
    s._randperm = lambda k, device: perms.append(real(k, device)) or perms[-1]
    try:
        logits, cls_loss, _, len_keep = s(x[None], attn, tea, STEP)
    finally:
        s._randperm = real
    it = iter([p.clone() for p in perms])
    s._randperm = lambda k, device: next(it)
    try:
        lk, ids = s.get_mask(n, STEP, attn)
    finally:
        s._randperm = real
    ref_keep, ref_ids = R.get_mask(n, attn[0].cpu().numpy(), [p.cpu().numpy() for p in perms], select_inv=False,
                                   mask_ratio=s.mask_ratio, mask_ratio_l=s.mask_ratio_l, mask_ratio_h=float(s.mrh_sche[STEP]),
                                   mask_ratio_hr=s.mask_ratio_hr)
    wrong = int((ids[0].cpu().numpy() != ref_ids).sum())
    st = {k: v.detach().cpu().numpy() for k, v in s.state_dict().items()}
    o64 = R.student(x.cpu().numpy(), st, ref_ids[:ref_keep], teacher_feat=tea.cpu().numpy())
    o32 = R.student(x.cpu().numpy(), st, ref_ids[:ref_keep], teacher_feat=tea.cpu().numpy(), dtype=torch.float32)
    lines.append(f"N = {n}: len_keep {lk} (restatement {ref_keep}), ids that differ from the stable-sort restatement: {wrong} of {n}; "
                 f"student at dropout 0 against float64: logits {R.rel_err(logits, o64['logits']):.2e} (fp32 restatement on the CPU "
                 f"{R.rel_err(o32['logits'], o64['logits']):.2e}), cls_loss {R.rel_err(cls_loss.reshape(1), o64['cls_loss'].reshape(1)):.2e} "
                 f"({R.rel_err(o32['cls_loss'].reshape(1), o64['cls_loss'].reshape(1)):.2e})")
    model.train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--errors", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ns", type=int, nargs="+", default=[9000, 30000])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mhim.py measures on an MI355X; no HIP device is visible")
    _lib.load()
    name = torch.cuda.get_device_name(0)
    lines = [f"MHIM_MIL training step (teacher forward + selection + student forward / backward), input_dim 1024, ratios 0.7 / 0.2 / "
             f"0.02, dropout 0.25, fp32, {name}; us per call, median (min-max) of 9 alternating batches of 20, {a.repeats} repeats",
             "hip = rrt_mil_amd.MHIM_MIL; (a) = eager torch, host list / set round trip; (b) = eager torch, device argsort / boolean mask"]
    err_lines = [f"MHIM_MIL selection and student errors, {name}"]
    torch.manual_seed(0)
    model = MHIM_MIL(**PARAMS).to(DEV).train()
    s = model.student
    for n in a.ns:
        x = torch.from_numpy(synth.bag(n, 1024, tag="bench/mhim", nonneg=True)).to(DEV)
        errors(model, x, err_lines)
        with torch.no_grad():
            attn = model.teacher.forward_teacher(x[None], return_attn=True)[1][0].contiguous()
        plan = stage_list(s, n)
        picks = [(lg, k, None if cnt is None else torch.from_numpy(R.pick_of(np.random.default_rng(k).permutation(k), k, cnt)).to(DEV))
                 for lg, k, cnt in plan]
        kept = mhim.mask_select(attn, picks)
        keep_n = int(kept[1].item())
        xk = mhim.gather_rows(x, kept[0], keep_n)
        lin = s.patch_to_emb[0]
        lines.append(f"N = {n}: stages (largest, k, drawn) {plan}, kept {keep_n}")
        for rep in range(a.repeats):
            r = alternate({"hip": lambda: hip_step(model, x), "(a)": lambda: eager_step(model, x, kept_host),
                           "(b)": lambda: eager_step(model, x, kept_device)})
            lines.append(f"  step      repeat {rep}   " + fmt(r, "hip"))
        for rep in range(a.repeats):
            with torch.no_grad():
                r = alternate({"rrt_mask_select_f32": lambda: mhim.mask_select(attn, picks),
                               "argsort asc+desc (stable)": lambda: (torch.argsort(attn, stable=True),
                                                                     torch.argsort(attn, descending=True, stable=True)),
                               "topk(k=N) asc+desc": lambda: (torch.topk(attn, n, largest=False), torch.topk(attn, n))})
            lines.append(f"  selection repeat {rep}   " + fmt(r, "rrt_mask_select_f32"))
        for rep in range(a.repeats):
            with torch.no_grad():
                r = alternate({"embedding GEMM, kept rows": lambda: lib_linear(lin, xk, _lib.COMPUTE_F32),
                               "all rows": lambda: lib_linear(lin, x, _lib.COMPUTE_F32),
                               "gather kept rows": lambda: mhim.gather_rows(x, kept[0], keep_n)})
            lines.append(f"  embedding repeat {rep}   " + fmt(r, "embedding GEMM, kept rows"))
    for path, text in ((a.out, lines), (a.errors, err_lines)):
        print("\n".join(text))
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
