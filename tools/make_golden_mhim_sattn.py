"""MHIM-MIL fixtures with the TransMIL baseline from the REAL reference (Survival/models/MHIM/network.py, baseline='selfattn',
on the CPU; run where the reference is checked out, einops installed):

    python tools/make_golden_mhim_sattn.py

tests/golden/mhim_sattn.npz, for every case of tests/mhim_sattn_cases.py::CASES (input_dim 64, p = 0 on every nn.Dropout,
including the 0.1 TransLayer hard-codes): the teacher's rows of both layers in fp32 (the scores the masks are selected on) and
float64, the teacher's feature, ``forward_test``'s logits, every permutation a stage draws, the kept ids, the student's logits,
feature and ``cls_loss`` in float64, and the reference's OWN fp32-against-float64 error of each quantity (relative to
max(1, max |float64|)).  For the gradient cases, per parameter (and for the bag): the float64 gradient's largest entry, its
2-norm, its first 32 values and the reference's own fp32 gradient error relative to the largest entry.  Arrays and a JSON cfg
only: the weights regenerate from mhim_sattn_cases.state, the bags from their tags; a float64 checksum of each pins them.

torch.topk leaves the order of equal votes unspecified, so the reference's masks are not reproducible as sets.  Two steps:
  1. for every stage the reference's ``select_mask_fn`` runs alone (no random draw) on the recorded rows, and its set and the
     restatement's are both held to what every valid answer shares: k tokens, every token above the threshold vote, none below
     (mhim_sattn_ref.threshold_property); the size of the tie class goes into the cfg.  Also for PROPERTY_NS x PROPERTY_HEADS.
  2. the reference student runs with ``get_mask`` replaced by a spy that returns the restatement's mask, both parts ascending:
     everything downstream of the mask is the reference's own code on the library's documented order.
Every recorded row is asserted NaN-free with pairwise distinct fp32 values per head.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from make_golden import cfg_array  # noqa: E402
from make_golden_mhim import keys_of, load_reference  # noqa: E402
import mhim_ref as MR  # noqa: E402
import mhim_sattn_cases as SC  # noqa: E402
import mhim_sattn_ref as SR  # noqa: E402
from mhim_ref import rel_err  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def build(ref, case, who, dtype):
    m = ref.MHIM(**SC.model_kwargs(case))
    st = SC.state(SC.CASES[case]["head"], who)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()}, strict=True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.
    return m.to(dtype).train(), float(sum(np.asarray(v, np.float64).sum() for v in st.values()))


def drop_no_norm(encoder):
    """the reference's forward_test(return_attn=True) hands ``no_norm`` to an SAttention that has no such argument: drop it"""
    real = encoder.forward
    encoder.forward = lambda x, no_norm=False, **kw: real(x, **kw)


def stage_check(ref_model, rows32, ps, largest, k):
    """step 1 for one stage -> the tie class's size"""
    ratio = (k - 0.5) / ps                                   # ceil(ps * ratio / (1 + 1e-8)) == k
    with torch.no_grad():
        len_keep, ids = ref_model.select_mask_fn(ps, torch.from_numpy(rows32)[None], largest, ratio, random_ratio=1.)
    theirs = ids[0, len_keep:].numpy()
    ours = SR.fused_order(SR.votes(rows32, largest, k))[:k]
    ok_t, ties = SR.threshold_property(rows32, largest, k, theirs)
    ok_o, _ = SR.threshold_property(rows32, largest, k, ours)
    assert ok_t and ok_o, (ps, largest, k, ok_t, ok_o)
    return ties, bool(set(theirs.tolist()) == set(ours.tolist()))


def main():
    ref = load_reference()
    out, cfg = {}, {"cases": {}, "property": []}
    for case, c in SC.CASES.items():
        n, head = c["n"], c["head"]
        x = SC.bag(case)
        rec = {"x_sum": float(np.asarray(x, np.float64).sum())}
        tea = {}
        for dtype in (torch.float64, torch.float32):
            t, rec["teacher_sum"] = build(ref, case, "teacher", dtype)
            xt = torch.from_numpy(x).to(dtype)[None]
            feat, rows = t.forward_teacher(xt, return_attn=True)
            drop_no_norm(t.online_encoder)
            logits, _ = t.forward_test(xt, return_attn=True)
            tea[dtype] = dict(feat=feat, a1=rows[0][0], a2=rows[1][0], test_logits=logits)
        for q in ("feat", "a1", "a2", "test_logits"):
            out[f"{case}/teacher_{q}"] = tea[torch.float64][q].numpy()
            rec[f"e32_teacher_{q}"] = rel_err(tea[torch.float32][q], tea[torch.float64][q])
        rows32 = [tea[torch.float32]["a1"].numpy(), tea[torch.float32]["a2"].numpy()]
        for r in rows32:
            assert np.isfinite(r).all() and all(np.unique(h).size == n for h in r), case
        out[f"{case}/rows32"] = np.stack(rows32)
        sel_rows = rows32[1 if c.get("attn_layer", 0) == -1 else c.get("attn_layer", 0)]
        # the stages, their permutations, the restatement's mask
        plan = MR.stage_plan(n, **SC.ratios(case))
        g = torch.Generator().manual_seed(1000 + n + head)
        perms = [torch.randperm(k, generator=g).numpy() for _, k, m in plan if m is not None]
        for j, p in enumerate(perms):
            out[f"{case}/perm{j}"] = p.astype(np.int64)
        len_keep, ids = SR.get_mask(n, sel_rows, perms, select_inv=c["select_inv"], **SC.ratios(case))
        out[f"{case}/ids"] = ids
        rec.update(len_keep=len_keep, n_perms=len(perms), ties=[], same_set=[])
        probe, _ = build(ref, case, "student", torch.float32)
        for largest, k, _ in plan:
            ties, same = stage_check(probe, sel_rows, n, largest, k)
            rec["ties"].append(ties)
            rec["same_set"].append(same)
        # step 2: the reference student on the restatement's mask
        stu, grads = {}, {}
        for dtype in (torch.float64, torch.float32):
            s, rec["student_sum"] = build(ref, case, "student", dtype)
            s.get_mask = lambda ps, i, attn, mrh=None: (len_keep, torch.from_numpy(ids)[None])
            xt = torch.from_numpy(x).to(dtype)[None].requires_grad_(case in SC.GRAD_CASES)
            logits, cls_loss, ps, lk = s(xt, attn=[tea[dtype]["a1"][None], tea[dtype]["a2"][None]], teacher_cls_feat=tea[dtype]["feat"], i=0)
            assert ps == n and lk == len_keep
            stu[dtype] = dict(logits=logits.detach(), cls_loss=cls_loss.detach().reshape(1))
            if case in SC.GRAD_CASES:
                (logits.sum() + cls_loss).backward()
                grads[dtype] = dict({k: p.grad for k, p in s.named_parameters()}, x=xt.grad[0])
        for q in ("logits", "cls_loss"):
            out[f"{case}/student_{q}"] = stu[torch.float64][q].numpy()
            rec[f"e32_student_{q}"] = rel_err(stu[torch.float32][q], stu[torch.float64][q])
        if grads:
            rec["grad"] = {}
            for k, g64 in grads[torch.float64].items():
                peak = float(g64.abs().max())
                rec["grad"][k] = dict(peak=peak, norm=float(g64.norm()),
                                      e32=float((grads[torch.float32][k].double() - g64).abs().max() / max(peak, 1e-300)))
                out[f"{case}/grad/{k}"] = g64.reshape(-1)[:32].numpy()
        cfg["cases"][case] = rec
        print(case, {k: v for k, v in rec.items() if k != "grad"}, flush=True)
    # step 1 at every N x heads of the property list, on teacher rows of those shapes, all three stage kinds
    for n in SC.PROPERTY_NS:
        for head in SC.PROPERTY_HEADS:
            t = ref.MHIM(**dict(SC.model_kwargs("n37_std"), head=head))
            t.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in SC.state(head, "teacher").items()}, strict=True)
            for mod in t.modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = 0.
            for seed in range(16):
                _, rows = t.forward_teacher(torch.from_numpy(SC.property_bag(n, seed))[None], return_attn=True)
                r = rows[0][0].numpy()
                if np.isfinite(r).all() and all(np.unique(h).size == n for h in r):
                    break
            else:
                raise AssertionError(f"no bag with pairwise distinct rows at n={n}, head={head}")
            out[f"property/n{n}_h{head}"] = r
            for largest, k, _ in MR.stage_plan(n, **SC.STD):
                ties, same = stage_check(t, r, n, largest, k)
                cfg["property"].append(dict(n=n, head=head, seed=seed, largest=bool(largest), k=k, ties=ties, same_set=same))
    print(cfg["property"], flush=True)
    models = {"MHIM": ref.MHIM(input_dim=SC.INPUT_DIM), "PURE_MHIM": ref.PURE_MHIM(input_dim=SC.INPUT_DIM, baseline="selfattn"),
              "MHIM_MIL": ref.MHIM_MIL(num_epoch=2, niter_per_ep=3, input_dim=SC.INPUT_DIM, mask_ratio_h=0.02)}
    cfg["keys"] = {k: keys_of(m) for k, m in models.items()}
    out["cfg"] = cfg_array(cfg)
    np.savez_compressed(os.path.join(OUT, "mhim_sattn.npz"), **out)
    print("wrote", os.path.join(OUT, "mhim_sattn.npz"), os.path.getsize(os.path.join(OUT, "mhim_sattn.npz")))


if __name__ == "__main__":
    main()
