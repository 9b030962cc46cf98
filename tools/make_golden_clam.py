"""CLAM fixtures from the REAL reference (modules/clam.py, on the CPU in float64; run where the reference is checked out):

    python tools/make_golden_clam.py

clam_keys: the reference's state_dict key / shape lists for every kind x dropout x rrt x gate combination.
clam_{sb,mb}_n{2,3}[_sub]: CLAM_SB / CLAM_MB with n_classes 2 and 3, with and without ``subtyping``, around an ``rrt=`` built
from the reference RRTEncoder.  Each file holds arrays and a JSON cfg only: the reference's state_dict key list with shapes
(the values regenerate from rrt-mil_amd/synth.py: encoder_state + clam_head_state), the label, logits, A_raw, M, the instance
logits / targets / loss, the top-k instance ids of every evaluated branch, and the float64 gradients of every parameter and
of the bag for loss = CE(logits, label) + instance_loss (small tensors whole, large ones as sampled rows; the largest entry
of every tensor is stored for the relative criterion of the tests).

The reference does not import as it stands where `future` is not installed and there is no GPU; two shims of this tool's own:
a stub ``future.builtins`` exposing ``range`` (modules/topk/polynomial imports it) and ``SmoothTop1SVM.cuda = identity``
(clam.py:116 calls .cuda() in the constructor).

A case is REFUSED while the k_sample-th and (k_sample+1)-th attention values at an evaluated end of an evaluated branch are
closer than 100x the forward bounds of tests/test_clam_gpu.py (1e-6 on the attention, 1e-4 on the raw scores): the seed
(part of the bag's tag) is stepped until the gap holds, so that the top-k ids are well defined by the reference alone.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from rrt_mil_amd import synth  # noqa: E402
from _ref import load_reference  # noqa: E402
from make_golden import cfg_array  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ENC_CFG = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
INPUT_DIM, K_SAMPLE = 128, 8
GAP_ATTN, GAP_RAW = 100 * 1e-6, 100 * 1e-4
FULL_LIMIT, ROWS = 4096, 16
torch.set_num_threads(8)


def load_clam():
    RRTEncoder, _ = load_reference()
    if "future" not in sys.modules:
        fut, fb = types.ModuleType("future"), types.ModuleType("future.builtins")
        fb.range = range
        fut.builtins = fb
        sys.modules.update({"future": fut, "future.builtins": fb})
    from modules import clam
    from modules.topk.svm import SmoothTop1SVM
    SmoothTop1SVM.cuda = lambda self, device=None: self
    return RRTEncoder, clam


def pack(key, g, out):
    g = np.asarray(g, dtype=np.float64)
    out[key + "__max"] = np.array(np.abs(g).max())
    if g.size <= FULL_LIMIT:
        out[key + "__full"] = g.astype(np.float32)
    else:
        g2 = g.reshape(g.shape[0], -1)
        rows = np.arange(0, g2.shape[0], max(1, g2.shape[0] // ROWS))
        out[key + "__rows"] = rows
        out[key + "__vals"] = g2[rows].astype(np.float32)


def smallest_gaps(A, A_raw, branches, k):
    """branches: [(row, both_ends)] -> the smallest (attention gap, raw gap) over the evaluated ends"""
    g = [np.inf, np.inf]
    for r, both in branches:
        for j, arr in enumerate((A[r], A_raw[r])):
            s = np.sort(arr)[::-1]
            g[j] = min(g[j], s[k - 1] - s[k])
            if both:
                g[j] = min(g[j], s[-k - 1] - s[-k])
    ga, gr = g
    return ga, gr


def run_case(kind, n_classes, subtyping, N, label):
    RRTEncoder, clam = load_clam()
    enc_state = synth.encoder_state(**{k: v for k, v in ENC_CFG.items() if k != "region_num"})
    name = f"clam_{kind}_n{n_classes}" + ("_sub" if subtyping else "")
    for seed in range(400):
        rrt = RRTEncoder(drop_out=0., **ENC_CFG)
        cls = clam.CLAM_SB if kind == "sb" else clam.CLAM_MB
        model = cls(INPUT_DIM, gate=True, size_arg="small", dropout=0., k_sample=K_SAMPLE, n_classes=n_classes,
                    subtyping=subtyping, rrt=rrt)
        ref_sd = model.state_dict()
        ridx = next(i for i, m in enumerate(model.attention_net) if m is rrt)
        pre = f"attention_net.{ridx}."
        head_shapes = {k: tuple(v.shape) for k, v in ref_sd.items() if not k.startswith(pre)}
        state = synth.clam_head_state(head_shapes, name)
        state.update({pre + k: v for k, v in enc_state.items()})
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
        model = model.double().eval()
        tag = f"clam/{name}/s{seed}"
        x = torch.from_numpy(synth.bag(N, INPUT_DIM, tag=tag, nonneg=True)).double().unsqueeze(0).requires_grad_(True)
        lab = torch.tensor([label])
        # the pieces the reference computes inside forward() and drops: recorded through hooks on its own modules
        rec = {"inst": []}
        hooks = [model.attention_net.register_forward_hook(lambda m, i, o: rec.update(A_raw=o[0].transpose(1, 0), h=o[1]))]
        for ic in model.instance_classifiers:
            hooks.append(ic.register_forward_hook(lambda m, i, o: rec["inst"].append(o)))
        logits, inst_loss, ps = model(x, label=lab, instance_eval=True)
        for h_ in hooks:
            h_.remove()
        A_raw = rec["A_raw"]
        A = F.softmax(A_raw, dim=1)
        M = torch.mm(A, rec["h"])
        onehot = F.one_hot(lab, n_classes).squeeze().tolist()
        branches = []              # (attention row, both ends used, instance classifier)
        for i in range(n_classes):
            row = i if kind == "mb" else 0
            if onehot[i] == 1:
                branches.append((row, True, i))
            elif subtyping:
                branches.append((row, False, i))
        ga, gr = smallest_gaps(A.detach().numpy(), A_raw.detach().numpy(), [(r, b) for r, b, _ in branches], K_SAMPLE)
        if ga < GAP_ATTN or gr < GAP_RAW:
            print(f"{name}: seed {seed} refused (attention gap {ga:.2e}, raw gap {gr:.2e})")
            continue
        loss = F.cross_entropy(logits, lab) + inst_loss
        loss.backward()
        K = A.shape[0]
        ids = np.stack([np.stack([torch.topk(A[r], K_SAMPLE)[1].numpy(), torch.topk(-A[r], K_SAMPLE)[1].numpy()]) for r in range(K)])
        inst_logits = torch.cat(rec["inst"], 0).detach().numpy()
        inst_targets = np.concatenate([np.r_[np.ones(K_SAMPLE), np.zeros(K_SAMPLE)] if b else np.zeros(K_SAMPLE)
                                       for _, b, _ in branches]).astype(np.int64)
        cfg = dict(kind=kind, n_classes=n_classes, subtyping=subtyping, input_dim=INPUT_DIM, k_sample=K_SAMPLE, gate=True,
                   size_arg="small", enc=ENC_CFG, rrt_prefix=pre, tag=tag, name=name, ps=int(ps),
                   ref_keys=[[k, list(v.shape)] for k, v in ref_sd.items()],
                   branches=[[r, int(b), i] for r, b, i in branches], gap_attn=float(ga), gap_raw=float(gr))
        out = dict(cfg=cfg_array(cfg), n=np.array(N), label=np.array(label), logits=logits.detach().numpy(),
                   a_raw=A_raw.detach().numpy(), features=M.detach().numpy(), inst_loss=np.array(float(inst_loss)),
                   loss=np.array(float(loss)), topk=ids, inst_logits=inst_logits, inst_targets=inst_targets)
        pack("g__x", x.grad[0].numpy(), out)
        none = []
        for pname, p in model.named_parameters():
            if p.grad is None:
                none.append(pname)
            else:
                pack("g__" + pname.replace(".", "__"), p.grad.numpy(), out)
        out["none"] = np.frombuffer("\n".join(none).encode(), dtype=np.uint8) if none else np.zeros(0, np.uint8)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KiB, inst_loss {float(inst_loss):.4f}, gaps {ga:.2e} / {gr:.2e}")
        return
    raise SystemExit(f"{name}: no seed gave the required top-k gap")


def key_lists():
    """clam_keys: the reference's state_dict key / shape list for every kind x dropout x rrt x gate (x size) combination"""
    RRTEncoder, clam = load_clam()
    combos = []
    for kind in ("sb", "mb"):
        for dropout in (0., 0.25):
            for with_rrt in (False, True):
                for gate in (False, True):
                    size = "big" if (gate and dropout) else "small"
                    cls = clam.CLAM_SB if kind == "sb" else clam.CLAM_MB
                    m = cls(INPUT_DIM, gate=gate, size_arg=size, dropout=dropout, n_classes=3,
                            rrt=RRTEncoder(**ENC_CFG) if with_rrt else None)
                    combos.append(dict(kind=kind, dropout=dropout, rrt=with_rrt, gate=gate, size_arg=size, n_classes=3,
                                       input_dim=INPUT_DIM, enc=ENC_CFG,
                                       keys=[[k, list(v.shape)] for k, v in m.state_dict().items()]))
    np.savez_compressed(os.path.join(OUT, "clam_keys.npz"), cfg=cfg_array(dict(combos=combos)))
    print(f"clam_keys: {len(combos)} combinations")


def main():
    key_lists()
    if "--keys-only" in sys.argv:
        return
    n = 120
    for kind in ("sb", "mb"):
        for n_classes in (2, 3):
            for subtyping in (False, True):
                run_case(kind, n_classes, subtyping, n, label=n_classes - 1)
                n += 13


if __name__ == "__main__":
    main()
