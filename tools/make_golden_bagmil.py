"""ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL fixtures from the REAL reference (modules/attmil.py, attmil_ibmil.py,
mean_max.py, on the CPU in float64; run where the reference is checked out):

    python tools/make_golden_bagmil.py [--keys-only]

bagmil_keys: the reference's state_dict key / shape lists for every dropout x rrt x act combination of the five heads
(IBMIL also with and without a confounder file).
bagmil_<head>: for every whole-head case of tests/bagmil_cases.py (rrt=None: N = 1, 2, 300; rrt=RRTEncoder: N = 30, 300, 1000)
the logits, the pooled row, the attention at a few indices, MaxMIL's arg-maxima and margin, and the reference's OWN
fp32-against-float64 error of each quantity (relative to max(1, max |float64|)); for one case per head (with rrt, N = 300)
the float64 gradients of a cross-entropy loss w.r.t. every parameter and the bag (small tensors whole, large ones as sampled
rows, the largest entry of every tensor for the relative criterion).  Arrays and a JSON cfg only: the state values
regenerate from rrt-mil_amd/synth.py (encoder_state + bagmil_head_state) and the bags from their tags.

modules/attmil.py imports torchvision.models at the top of the module (for a ResNet class no head uses); torchvision is
not installed here, so it is stubbed in sys.modules, as tools/_ref.py stubs timm.
"""
import copy
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from _ref import load_reference  # noqa: E402
from make_golden import cfg_array  # noqa: E402
from make_golden_clam import pack  # noqa: E402
import bagmil_cases as BC  # noqa: E402
from bagmil_ref import rel_err  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def load_heads():
    """(reference RRTEncoder, {kind: reference class})"""
    RRTEncoder, _ = load_reference()
    if "torchvision" not in sys.modules:
        tv, tvm = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
        tv.models = tvm
        sys.modules.update({"torchvision": tv, "torchvision.models": tvm})
    import importlib
    return RRTEncoder, {k: getattr(importlib.import_module("modules." + mod), name) for k, (mod, name) in BC.CLASS_OF.items()}


def key_lists(tmp):
    RRTEncoder, classes = load_heads()
    conf = BC.conf_file(tmp)
    combos = []
    for kind in BC.HEADS:
        acts = ("relu", "gelu", "tanh", "none") if kind == "gattmil" else (("relu", "gelu", "none") if kind in ("meanmil", "maxmil")
                                                                            else ("relu", "gelu"))
        for dropout in (0., 0.25):
            for with_rrt in (False, True):
                for act in acts:
                    for cp in ((False, True) if kind == "ibmil" else (False,)):
                        m = BC.construct(classes, kind, rrt=RRTEncoder(**BC.ENC_CFG) if with_rrt else None, dropout=dropout,
                                         act=act, conf_path=conf if cp else False, bias=with_rrt)
                        combos.append(dict(kind=kind, dropout=dropout, rrt=with_rrt, act=act, conf=cp, bias=with_rrt,
                                           keys=[[k, list(v.shape)] for k, v in m.state_dict().items()]))
    np.savez_compressed(os.path.join(OUT, "bagmil_keys.npz"), cfg=cfg_array(dict(combos=combos, enc=BC.ENC_CFG)))
    print(f"bagmil_keys: {len(combos)} combinations")


def run(model, kind, x):
    """the reference's forward with the pieces it computes and drops recorded through hooks on its own modules"""
    rec, hooks = {}, []
    if kind in ("attmil", "gattmil"):
        hooks.append(model.classifier.register_forward_hook(lambda m, i, o: rec.update(pooled=i[0][0])))
    if kind == "gattmil":
        hooks.append(model.attention_c.register_forward_hook(lambda m, i, o: rec.update(attn=F.softmax(o[:, 0], 0))))
    if kind == "ibmil":
        hooks.append(model.attention.register_forward_hook(lambda m, i, o: rec.update(attn=F.softmax(o[:, 0], 0))))
        hooks.append(model.head.register_forward_hook(lambda m, i, o: rec.update(pooled=i[0][0, :512], deconf_cf=i[0][0, 512:])))
    if kind in ("meanmil", "maxmil"):
        hooks.append(model.head.register_forward_hook(lambda m, i, o: rec.update(scores=o[0])))
    if kind == "attmil":
        logits, A = model(x, return_attn=True)
        rec["attn"] = A[0]
    else:
        logits = model(x)
    for h in hooks:
        h.remove()
    rec["logits"] = logits
    return rec


def head_file(kind, tmp):
    RRTEncoder, classes = load_heads()
    conf = BC.conf_file(tmp)
    out, cases = {}, {}
    for (k, with_rrt, N) in BC.WHOLE_CASES:
        if k != kind:
            continue
        cid = BC.case_id(kind, with_rrt, N)
        model = BC.construct(classes, kind, rrt=RRTEncoder(drop_out=0., **BC.ENC_CFG) if with_rrt else None,
                             conf_path=conf if kind == "ibmil" else False, bias=with_rrt)
        ref_sd = model.state_dict()
        state = BC.head_state(ref_sd, kind)
        model.load_state_dict({k_: torch.from_numpy(np.array(v)) for k_, v in state.items()}, strict=True)
        model = model.eval()
        m64, m32 = copy.deepcopy(model).double(), copy.deepcopy(model).float()
        x = torch.from_numpy(BC.bag(kind, with_rrt, N)).unsqueeze(0)
        want_grad = (kind, with_rrt, N) in BC.GRAD_CASES
        x64 = x.double().requires_grad_(want_grad)
        with torch.set_grad_enabled(want_grad):
            r64 = run(m64, kind, x64)
        with torch.no_grad():
            r32 = run(m32, kind, x.float())
        info = dict(n=N, rrt=with_rrt, act=BC.ACT[kind], ref_keys=[[k_, list(v.shape)] for k_, v in ref_sd.items()])
        idx = sorted({0, N // 2, N - 1})
        for q in ("logits", "pooled", "attn", "deconf_cf"):
            if q not in r64:
                continue
            a64, a32 = r64[q].detach(), r32[q].detach()
            out[f"{cid}/e32_{q}"] = np.array(rel_err(a32, a64))
            if q == "attn":
                out[f"{cid}/attn_idx"], a64 = np.array(idx), a64[idx]
                info["attn_peak"] = float(r64[q].detach().max() * N)
            out[f"{cid}/{q}"] = a64.numpy()
        if kind == "maxmil":
            s = r64["scores"].detach()
            top = torch.sort(s, 0, descending=True)[0]
            out[f"{cid}/argmax"] = s.argmax(0).numpy().astype(np.int64)
            info["margin"] = float(((top[0] - top[1]) if N > 1 else top[0].abs()).min() / s.abs().max())
        if want_grad:
            label = torch.tensor([1])
            loss = F.cross_entropy(r64["logits"], label)
            loss.backward()
            out[f"{cid}/loss"] = np.array(float(loss.detach()))
            g = {}
            pack("x", x64.grad[0].numpy(), g)
            none = []
            for pname, p in m64.named_parameters():
                if p.grad is None:
                    none.append(pname)
                else:
                    pack(pname.replace(".", "__"), p.grad.numpy(), g)
            out.update({f"{cid}/g__{k_}": v for k_, v in g.items()})
            info["none"] = none
            info["label"] = 1
        cases[cid] = info
        print(f"{cid}: logits {r64['logits'].detach().numpy().round(4).tolist()} e32 {float(out[cid + '/e32_logits']):.2e} "
              + " ".join(f"{k_}={v:.3g}" for k_, v in info.items() if k_ in ("attn_peak", "margin")))
    path = os.path.join(OUT, f"bagmil_{kind}.npz")
    np.savez_compressed(path, cfg=cfg_array(dict(kind=kind, cases=cases, enc=BC.ENC_CFG, n_conf=BC.N_CONF)), **out)
    print(f"bagmil_{kind}: {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        key_lists(tmp)
        if "--keys-only" in sys.argv:
            return
        for kind in BC.HEADS:
            head_file(kind, tmp)


if __name__ == "__main__":
    main()
