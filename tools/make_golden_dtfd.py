"""DTFD-MIL fixtures from the REAL reference (Survival/models/DTFD/network.py, rrt=False, on the CPU; run where the reference
is checked out):

    python tools/make_golden_dtfd.py            # records tests/golden/dtfd.npz, asserting what is said below
    python tools/make_golden_dtfd.py --search   # prints, per case, the first seed under which the assertions hold

The reference file cannot be imported as it stands: it does ``from .rrt import RRTEncoder`` (a file that does not exist) and
imports torchvision.  It is loaded with importlib under a made-up package name after stub modules of our own are registered
for that package, its ``.rrt`` (a placeholder RRTEncoder class) and, where it is not installed, torchvision /
torchvision.models; ``rrt=False`` throughout.  Every nn.Dropout of the reference model has p = 0.

tests/golden/dtfd.npz, for every case of tests/dtfd_cases.py::CASES (input_dim 64, inner_dim 512): the ``random.shuffle``
permutation under the case's seed, the reference's fp32 CAM probability of every row and the rows it selected, logits /
hazards / S in fp32 and float64; for dtfd_cases.TRAIN_CASES one training step: (hazards, S), loss0, the outer loss, the rows
selected, and of every parameter's .grad after the forward alone (the inner backward) and after the outer
``criterion(...).backward()``, and of the bag's gradient, the float64 summary dtfd_cases.grad_summary keeps (sums, the largest
entry and evenly spread samples: whole gradients would not fit a fixture; the tests compare whole tensors against
tests/dtfd_ref.py, which tests/test_dtfd_cpu.py pins to these summaries).  With every quantity the reference's OWN
fp32-against-float64 error, relative to max(1, max |float64|).  Arrays and a JSON cfg only: weights and bags regenerate from
dtfd_cases (rrt-mil_amd/synth.py), float64 checksums pin them.

Asserted for EVERY group of EVERY case, in eval and in the training step: p is NaN-free, has a unique maximum and a unique
minimum, and the float64 gap to the runner-up at both ends is at least 64 x the case's max |p32 - p64| -- so the reference's
selection is one well-defined set whatever order torch.sort gives ties in, and comparable with the library's tie rule.
"""
import copy
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from _ref import load_reference as _encoder_reference  # noqa: E402
from make_golden import cfg_array  # noqa: E402
import dtfd_cases as DC  # noqa: E402
import dtfd_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.path.join(_encoder_reference.__defaults__[0], "Survival", "models", "DTFD", "network.py")
PKG = "reference_dtfd_pkg"
GAP_FACTOR = 64.0
torch.set_num_threads(8)


def load_reference():
    pkg = types.ModuleType(PKG)
    pkg.__path__ = []
    rrt = types.ModuleType(PKG + ".rrt")

    class RRTEncoder(torch.nn.Module):
        """placeholder: never built (rrt=False)"""

    rrt.RRTEncoder = RRTEncoder
    sys.modules.update({PKG: pkg, PKG + ".rrt": rrt})
    if importlib.util.find_spec("torchvision") is None:
        tv, tvm = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
        tv.models = tvm
        sys.modules.update({"torchvision": tv, "torchvision.models": tvm})
    spec = importlib.util.spec_from_file_location(PKG + ".network", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[PKG + ".network"] = mod
    spec.loader.exec_module(mod)
    return mod


class Spy:
    """torch.sort and the criterion recorded while the reference runs; the tier-2 logits through a forward hook"""

    def __init__(self, model):
        self.model, self.sorts, self.losses, self.logits, self.real = model, [], [], [], torch.sort

    def sort(self, t, *a, **kw):
        out = self.real(t, *a, **kw)
        self.sorts.append((t.detach().clone(), out[1].detach().clone()))
        return out

    def criterion(self, **kw):
        loss = R.nll_surv(**kw)
        self.losses.append(loss.detach().clone())
        return loss

    def __enter__(self):
        torch.sort = self.sort
        self.hook = self.model.UClassifier.register_forward_hook(lambda m, i, o: self.logits.append(o.detach().clone()))
        return self

    def __exit__(self, *a):
        torch.sort = self.real
        self.hook.remove()


def build(ref, cid, dtype):
    c = DC.CASES[cid]
    m = ref.DTFD(1e-4, 1e-5, 10, None, rrt=False, **DC.model_kwargs(cid))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    st = DC.state(c["n_classes"])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()}, strict=True)
    return m.to(dtype), st


def per_row(sorts, perm, n, group):
    """the recorded per-group p (group order) and sort results -> p [n] in original row order, sel [group, 2] original rows"""
    perm = np.arange(n) if perm is None else np.asarray(perm)
    assert len(sorts) == group
    p = np.zeros(n, sorts[0][0].numpy().dtype)
    sel = np.zeros((group, 2), np.int64)
    for k, ((s, sz), (pg, order)) in enumerate(zip(R.group_positions(n, group), sorts)):
        rows = perm[s:s + sz]
        assert pg.numel() == sz
        p[rows] = pg.numpy()
        sel[k] = rows[int(order[0])], rows[int(order[-1])]
    return p, sel


def check_gaps(cid, what, p32, p64, perm, n, group):
    """the module docstring's assertion; -> None, or why it fails"""
    perm = np.arange(n) if perm is None else np.asarray(perm)
    err = float(np.abs(p32.astype(np.float64) - p64).max())
    if np.isnan(p32).any() or np.isnan(p64).any():
        return f"{cid} {what}: NaN in p"
    for k, (s, sz) in enumerate(R.group_positions(n, group)):
        for p in (p32[perm[s:s + sz]], p64[perm[s:s + sz]]):
            if (p == p.max()).sum() != 1 or ((p == p.min()).sum() != 1 and sz > 1):
                return f"{cid} {what} group {k}: a tied extreme"
        if sz > 1:
            srt = np.sort(p64[perm[s:s + sz]])
            gap = min(srt[-1] - srt[-2], srt[1] - srt[0])
            if not gap >= GAP_FACTOR * err:
                return f"{cid} {what} group {k}: gap {gap:.3e} < {GAP_FACTOR:.0f} x {err:.3e}"
    return None


def run_eval(m, x, seed):
    random.seed(seed)
    with Spy(m) as spy, torch.no_grad():
        hazards, S = m.eval()(x[None])
    return dict(hazards=hazards, S=S, logits=spy.logits[0], sorts=spy.sorts)


def run_train(m, x, n_classes):
    x = x.clone().requires_grad_()
    grads = lambda: {k: (np.zeros(tuple(p.shape)) if p.grad is None else p.grad.detach().double().numpy().copy())   # noqa: E731
                     for k, p in m.named_parameters()}
    with Spy(m) as spy:
        m.criterion = spy.criterion
        hazards, S = m.train()(x[None], label=DC.LABEL)
        inner = grads()
        loss = spy.criterion(hazards=hazards, S=S, Y=torch.tensor([DC.LABEL["label"]]), c=torch.tensor([DC.LABEL["censorship"]]))
        loss.backward()
    return dict(hazards=hazards.detach(), S=S.detach(), loss0=spy.losses[0].reshape(1), loss=spy.losses[1].reshape(1),
                sorts=spy.sorts, inner=inner, outer=grads(), dx=x.grad.detach().double().numpy().copy())


def record(ref, cid, out, cases):
    """one case -> None (recorded into out / cases), or the reason its assertions fail"""
    c = DC.CASES[cid]
    n, g = c["n"], c["group"]
    m32, st = build(ref, cid, torch.float32)
    m64, _ = build(ref, cid, torch.float64)
    x = torch.from_numpy(DC.bag(cid))
    random.seed(c["seed"])
    perm = list(range(n))
    random.shuffle(perm)
    perm = np.array(perm, np.int64)
    e32, e64 = run_eval(m32, x.float(), c["seed"]), run_eval(m64, x.double(), c["seed"])
    p32, sel32 = per_row(e32["sorts"], perm, n, g)
    p64, sel64 = per_row(e64["sorts"], perm, n, g)
    why = check_gaps(cid, "eval", p32, p64, perm, n, g)
    if why:
        return why
    assert np.array_equal(sel32, sel64) and np.array_equal(sel32, R.select_from_p(p32, perm, g)), cid
    out[f"{cid}/perm"], out[f"{cid}/p32"], out[f"{cid}/sel"] = perm, p32, sel32
    out[f"{cid}/e32_p"] = np.array(R.rel_err(p32, p64))
    for q in ("logits", "hazards", "S"):
        out[f"{cid}/{q}32"], out[f"{cid}/{q}64"] = e32[q].numpy(), e64[q].numpy()
        out[f"{cid}/e32_{q}"] = np.array(R.rel_err(e32[q], e64[q]))
    info = dict(c, state_sum=DC.state_sum(st), bag_sum=float(x.double().sum()), keys=[[k, list(v.shape)] for k, v in m32.state_dict().items()])
    if cid in DC.TRAIN_CASES:
        t32, t64 = run_train(m32, x.float(), c["n_classes"]), run_train(m64, x.double(), c["n_classes"])
        tp32, tsel32 = per_row(t32["sorts"], None, n, g)
        tp64, tsel64 = per_row(t64["sorts"], None, n, g)
        why = check_gaps(cid, "train", tp32, tp64, None, n, g)
        if why:
            return why
        assert np.array_equal(tsel32, tsel64) and np.array_equal(tsel32, R.select_from_p(tp32, None, g)), cid
        out[f"{cid}/train_sel"] = tsel32
        for q in ("hazards", "S", "loss0", "loss"):
            out[f"{cid}/train_{q}"] = t64[q].numpy()
            out[f"{cid}/e32_train_{q}"] = np.array(R.rel_err(t32[q], t64[q]))
        for which in ("inner", "outer"):
            for k, v in t64[which].items():
                out[f"{cid}/{which}/{k}"] = DC.grad_summary(v)
        out[f"{cid}/dx"] = DC.grad_summary(t64["dx"])
        # (both attention_weights.bias gradients are sums that cancel to zero in exact arithmetic -- a softmax does not see a
        #  shift of its scores --: roundoff in either precision, no yardstick of their own)
        worst = max(float(np.abs(t32[w][k] - t64[w][k]).max() / np.abs(t64[w][k]).max()) for w in ("inner", "outer")
                    for k in t64[w] if np.abs(t64[w][k]).max() > 0 and not k.endswith("attention_weights.bias"))
        info["e32_grad_worst"] = worst
    cases[cid] = info
    print(f"{cid}: logits {e64['logits'].numpy().round(4).tolist()} e32 {float(out[cid + '/e32_logits']):.2e}  p e32 "
          f"{float(out[cid + '/e32_p']):.2e}  sel {sel32.tolist()[:3]}{' ...' if g > 3 else ''}"
          + (f"  train loss0 {float(out[cid + '/train_loss0'][0]):.6f} grads' worst e32 {info['e32_grad_worst']:.2e}" if cid in DC.TRAIN_CASES else ""))
    return None


def main():
    ref = load_reference()
    if "--search" in sys.argv:
        for cid, c in DC.CASES.items():
            for seed in range(64):
                c["seed"] = seed
                if record(ref, cid, {}, {}) is None:
                    print(f"    {cid}: seed {seed}")
                    break
            else:
                raise SystemExit(f"{cid}: no seed below 64 satisfies the assertions")
        return
    out, cases = {}, {}
    for cid in DC.CASES:
        why = record(ref, cid, out, cases)
        assert why is None, why
    path = os.path.join(OUT, "dtfd.npz")
    np.savez_compressed(path, cfg=cfg_array(dict(cases=cases, label=DC.LABEL, gap_factor=GAP_FACTOR)), **out)
    size = os.path.getsize(path)
    print(f"dtfd: {size / 1024:.0f} KiB")
    assert size < 200 * 1024, size


if __name__ == "__main__":
    main()
