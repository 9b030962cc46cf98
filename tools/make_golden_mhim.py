"""MHIM-MIL fixtures from the REAL reference (Survival/models/MHIM/network.py, baseline='attn', on the CPU; run where the
reference is checked out):

    python tools/make_golden_mhim.py

tests/golden/mhim.npz, for every case of tests/mhim_cases.py::CASES (N = 37 / 300, input_dim 64, dropout 0): the teacher's fp32
attention row (the scores the masks are selected on), every ``torch.randperm`` result of the training step in call order, the
reference's ``len_keep`` and the sorted kept ids, the student's logits and ``cls_loss`` and the teacher's and
``forward_test``'s outputs in float64, and the reference's OWN fp32-against-float64 error of each quantity (relative to
max(1, max |float64|)).  Arrays and a JSON cfg only: the weights regenerate from mhim_cases.state (rrt-mil_amd/synth.py), the
bags from their tags; a float64 checksum of each pins them.  Also the state_dict key lists of MHIM_MIL / PURE_MHIM / MHIM and
the reference's cosine schedules for mhim_cases.SCHEDULES.

Every recorded attention row is asserted NaN-free with pairwise distinct fp32 values: then the k smallest / largest of it are
ONE set, whatever order torch.topk gives ties in, and the reference's masks are comparable with the library's tie rule.
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from _ref import load_reference as _encoder_reference  # noqa: E402
from make_golden import cfg_array  # noqa: E402
import mhim_cases as MC  # noqa: E402
from mhim_ref import rel_err  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# the checkout tools/_ref.py imports the encoder from
REFERENCE = os.path.join(_encoder_reference.__defaults__[0], "Survival", "models", "MHIM", "network.py")
torch.set_num_threads(8)


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_mhim_network", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Perms:
    """torch.randperm wrapped: records every result, or replays recorded ones"""

    def __init__(self, replay=None):
        self.rec, self.replay, self.real = [], (list(replay) if replay is not None else None), torch.randperm

    def __call__(self, n, **kw):
        if self.replay is not None:
            p = torch.as_tensor(self.replay.pop(0))
            assert p.numel() == n
            return p
        p = self.real(n, **kw)
        self.rec.append(p.clone())
        return p

    def __enter__(self):
        torch.randperm = self
        return self

    def __exit__(self, *a):
        torch.randperm = self.real


def keys_of(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def load(model, who):
    st = MC.state({k: tuple(v.shape) for k, v in model.state_dict().items()}, who)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()}, strict=True)
    return float(sum(np.asarray(v, np.float64).sum() for v in st.values()))


def step(student, x, attn, tea):
    """the reference's MHIM.forward with get_mask's result recorded"""
    got = {}
    real = student.get_mask

    def spy(*a, **kw):
        got["len_keep"], got["mask_ids"] = real(*a, **kw)
        return got["len_keep"], got["mask_ids"]
    student.get_mask = spy
    try:
        logits, cls_loss, ps, len_keep = student(x, attn, tea, None)
    finally:
        del student.get_mask
    return dict(logits=logits.detach(), cls_loss=cls_loss.detach().reshape(1), len_keep=int(len_keep),
                kept=np.sort(got["mask_ids"][0, :len_keep].numpy()).astype(np.int64), ps=int(ps))


def main():
    ref = load_reference()
    out, cases = {}, {}
    torch.manual_seed(20240521)
    for cid, c in MC.CASES.items():
        kw = MC.model_kwargs(cid)
        student, teacher = ref.MHIM(**kw).train(), ref.MHIM(**kw).train()           # dropout 0: train() draws nothing
        sums = [load(student, "student"), load(teacher, "teacher")]
        x = torch.from_numpy(MC.bag(cid)).unsqueeze(0)
        s64, t64 = copy.deepcopy(student).double(), copy.deepcopy(teacher).double()
        tea32, attn32 = teacher.forward_teacher(x.float(), return_attn=True)
        tea64, attn64 = t64.forward_teacher(x.double(), return_attn=True)
        a = attn32[0].numpy()
        assert a.dtype == np.float32 and not np.isnan(a).any() and np.unique(a).size == a.size, f"{cid}: attention row with ties"
        with Perms() as rec:
            r32 = step(student, x.float(), attn32, tea32)
        with Perms(replay=[p.numpy() for p in rec.rec]) as rep:
            r64 = step(s64, x.double(), attn32.double(), tea64)                     # the same scores: the same mask
        assert not rep.replay and r64["len_keep"] == r32["len_keep"] and np.array_equal(r64["kept"], r32["kept"]), cid
        pooled = {}
        for tag, m, xx in (("32", student, x.float()), ("64", s64, x.double())):
            test_logits, test_attn = m.forward_test(xx, return_attn=True)
            _, test_raw = m.forward_test(xx, return_attn=True, no_norm=True)
            pooled["test_logits" + tag], pooled["test_attn" + tag], pooled["test_raw" + tag] = test_logits, test_attn, test_raw
        for q, v32, v64 in (("logits", r32["logits"], r64["logits"]), ("cls_loss", r32["cls_loss"], r64["cls_loss"]),
                            ("tea_feat", tea32, tea64), ("tea_attn", attn32, attn64),
                            ("test_logits", pooled["test_logits32"], pooled["test_logits64"]),
                            ("test_attn", pooled["test_attn32"], pooled["test_attn64"]),
                            ("test_raw", pooled["test_raw32"], pooled["test_raw64"])):
            out[f"{cid}/{q}"] = v64.detach().numpy()
            out[f"{cid}/e32_{q}"] = np.array(rel_err(v32, v64))
        out[f"{cid}/attn32"] = a
        out[f"{cid}/kept"] = r32["kept"]
        for j, p in enumerate(rec.rec):
            out[f"{cid}/perm{j}"] = p.numpy().astype(np.int64)
        cases[cid] = dict(c, len_keep=r32["len_keep"], n_perms=len(rec.rec), state_sum=sums, bag_sum=float(x.double().sum()),
                          keys=keys_of(student))
        print(f"{cid}: len_keep {r32['len_keep']} / {c['n']}  perms {[p.numel() for p in rec.rec]}  logits "
              f"{r64['logits'].numpy().round(4).tolist()} e32 {float(out[cid + '/e32_logits']):.2e}  cls_loss "
              f"{float(r64['cls_loss']):.6f} e32 {float(out[cid + '/e32_cls_loss']):.2e}")
    keys = dict(MHIM_MIL=keys_of(ref.MHIM_MIL(**MC.MAIN_PARAMS)), PURE_MHIM=keys_of(ref.PURE_MHIM()),
                MHIM=keys_of(ref.MHIM(baseline="attn")), MHIM_gelu_nodrop=keys_of(ref.MHIM(baseline="attn", act="gelu", dropout=0.)),
                MHIM_noact=keys_of(ref.MHIM(baseline="attn", act="none", da_act="none")))
    for j, s in enumerate(MC.SCHEDULES):
        out[f"schedule{j}"] = ref.cosine_scheduler(s[0], s[1], epochs=s[2], niter_per_ep=s[3], warmup_epochs=s[4],
                                                   start_warmup_value=s[5])
    path = os.path.join(OUT, "mhim.npz")
    np.savez_compressed(path, cfg=cfg_array(dict(cases=cases, keys=keys)), **out)
    print(f"mhim: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
