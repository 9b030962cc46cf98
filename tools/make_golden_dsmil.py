"""DSMIL fixtures from the REAL reference (modules/dsmil.py, on the CPU in float64; run where the reference is checked out):

    python tools/make_golden_dsmil.py

dsmil_keys: the reference's state_dict key / shape lists for every dropout x rrt x act combination.
dsmil_n2, dsmil_n3, dsmil_n2_norrt, dsmil_n2_bce, dsmil_n2_wide: MILNet with 2 / 3 classes around an ``rrt=`` built from the
reference RRTEncoder (``_norrt``: rrt=None; ``_bce``: nn.BCEWithLogitsLoss instead of nn.CrossEntropyLoss).  Each file holds
arrays and a JSON cfg only: the reference's state_dict key list with shapes (the values regenerate from
rrt-mil_amd/synth.py: encoder_state + dsmil_head_state), the label, the bag logits, the class maxima, the critical instance
ids, A, B, the loss, and the float64 gradients of every parameter and of the bag for
loss = criterion(bag logits) + max_loss (small tensors whole, large ones as sampled rows; the largest entry of every tensor
is stored for the relative criterion of the tests).

A case is REFUSED while the largest and the second-largest instance score of any class column are closer than 1e-2 (100x
the 1e-4 forward bound of tests/test_dsmil_gpu.py; ``dsmil_n2_wide``, which the bf16 test uses: 0.2, 10x its 2e-2 bound):
the seed (part of the bag's tag) is stepped until the gap holds, so that the critical instances are well defined by the
reference alone.
"""
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from rrt_mil_amd import synth  # noqa: E402
from _ref import load_reference  # noqa: E402
from make_golden import cfg_array  # noqa: E402
from make_golden_clam import pack  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ENC_CFG = dict(mlp_dim=512, epeg_k=15, crmsa_k=3, region_num=8)
INPUT_DIM = 128
GAP, GAP_WIDE = 1e-2, 0.2
torch.set_num_threads(8)


def load_dsmil():
    RRTEncoder, _ = load_reference()
    from modules import dsmil
    return RRTEncoder, dsmil


def run_case(name, n_classes, N, label, act="relu", with_rrt=True, bce=False, gap=GAP):
    RRTEncoder, dsmil = load_dsmil()
    enc_state = synth.encoder_state(**{k: v for k, v in ENC_CFG.items() if k != "region_num"})
    for seed in range(400):
        rrt = RRTEncoder(drop_out=0., **ENC_CFG) if with_rrt else None
        model = dsmil.MILNet(n_classes, 0., act, input_dim=INPUT_DIM, rrt=rrt)
        ref_sd = model.state_dict()
        head_shapes = {k: tuple(v.shape) for k, v in ref_sd.items() if not k.startswith("rrt.")}
        state = synth.dsmil_head_state(head_shapes, name)
        if with_rrt:
            state.update({"rrt." + k: v for k, v in enc_state.items()})
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
        model = model.double().train()               # train(): the branch that computes max_loss; nothing stochastic (p = 0)
        tag = f"dsmil/{name}/s{seed}"
        x = torch.from_numpy(synth.bag(N, INPUT_DIM, tag=tag, nonneg=True)).double().unsqueeze(0).requires_grad_(True)
        # the pieces the reference computes inside forward() and drops: recorded through hooks on its own modules
        rec = {}
        hooks = [model.i_classifier.register_forward_hook(lambda m, i, o: rec.update(classes=o)),
                 model.b_classifier.register_forward_hook(lambda m, i, o: rec.update(A=o[1], B=o[2]))]
        if bce:
            crit, lab = nn.BCEWithLogitsLoss(), torch.tensor(label)
            bag_target = lab.view(1, -1).double()
        else:
            crit, lab = nn.CrossEntropyLoss(), torch.tensor([label])
            bag_target = lab
        pred, max_loss, ps = model(x, label=lab, loss=crit)
        for h_ in hooks:
            h_.remove()
        classes = rec["classes"].detach()
        top2 = torch.sort(classes, 0, descending=True)[0][:2]
        g = float((top2[0] - top2[1]).min())
        if g < gap:
            print(f"{name}: seed {seed} refused (instance score gap {g:.2e} < {gap})")
            continue
        loss = crit(pred, bag_target) + max_loss
        loss.backward()
        A = rec["A"].detach().numpy()
        cfg = dict(n_classes=n_classes, input_dim=INPUT_DIM, act=act, rrt=with_rrt, bce=bce, enc=ENC_CFG, tag=tag, name=name,
                   ps=int(ps), ref_keys=[[k, list(v.shape)] for k, v in ref_sd.items()], gap=g,
                   attn_peak=float(A.max() * N))
        out = dict(cfg=cfg_array(cfg), n=np.array(N), label=np.array(label), logits=pred.detach().numpy(),
                   classes_max=classes.max(0)[0].numpy(), critical=classes.argmax(0).numpy().astype(np.int64), attn=A,
                   features=rec["B"].detach().numpy(), max_loss=np.array(float(max_loss.detach())), loss=np.array(float(loss.detach())))
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
        print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KiB, loss {float(loss):.4f}, gap {g:.2e}, "
              f"largest attention {A.max() * N:.1f} / N, critical {out['critical'].tolist()}")
        return
    raise SystemExit(f"{name}: no seed gave the required instance score gap")


def key_lists():
    """dsmil_keys: the reference's state_dict key / shape list for every dropout x rrt x act combination"""
    RRTEncoder, dsmil = load_dsmil()
    combos = []
    for dropout in (0., 0.25):
        for with_rrt in (False, True):
            for act in ("relu", "gelu"):
                m = dsmil.MILNet(3, dropout, act, input_dim=INPUT_DIM, rrt=RRTEncoder(**ENC_CFG) if with_rrt else None)
                combos.append(dict(dropout=dropout, rrt=with_rrt, act=act, n_classes=3, input_dim=INPUT_DIM, enc=ENC_CFG,
                                   keys=[[k, list(v.shape)] for k, v in m.state_dict().items()]))
    np.savez_compressed(os.path.join(OUT, "dsmil_keys.npz"), cfg=cfg_array(dict(combos=combos)))
    print(f"dsmil_keys: {len(combos)} combinations")


def main():
    key_lists()
    if "--keys-only" in sys.argv:
        return
    run_case("dsmil_n2", 2, 700, label=1)
    run_case("dsmil_n3", 3, 1500, label=2, act="gelu")
    run_case("dsmil_n2_norrt", 2, 300, label=0, with_rrt=False)
    run_case("dsmil_n2_bce", 2, 433, label=[1, 0], bce=True)
    run_case("dsmil_n2_wide", 2, 520, label=1, gap=GAP_WIDE)


if __name__ == "__main__":
    main()
