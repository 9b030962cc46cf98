"""TransMIL / Nystrom-attention fixtures from the REAL reference (modules/transmil.py, modules/nystrom_attention.py, on the
CPU; run where the reference is checked out):

    python tools/make_golden_transmil.py

Only what a test compares is stored; every input and parameter regenerates from rrt-mil_amd/synth.py (nystrom_state,
nystrom_input, transmil_state, bag).

transmil_keys   : the reference's state_dict key / shape lists of TransMIL(1024, 2, ...) and NystromAttention(512), and the
                  two constructor signatures (names and defaults).
transmil_attn   : for every (dim, heads, n, gain) attention case of tests/test_transmil_gpu.py: the first and the last row of
                  the reference's float64 output, its peak |logit|, and e32 = the reference's own fp32 run against its own
                  float64 run.
transmil_stages : the stage tensors of the small cases (float64, every 32nd landmark row): landmarks, a2, a3 v, z, z (a3 v)
                  and the last rows of the merged heads.  They are read off the reference's own run: the landmark tensors
                  einops' reduce returned (divided in place by the reference afterwards), the operands of its three einsum
                  calls, the argument and the result of its moore_penrose_iter_pinv, the input of to_out; a3 v and z (a3 v)
                  are products of those.
transmil_model  : for every whole-model case: the reference's float64 logits, rows 0, 1 and the last of the rows before the
                  final LayerNorm, and e32 of both.  TransMIL.forward casts its input to fp32, so the float64 run feeds the
                  fp32-representable bag to the reference's submodules in double (forward itself is the reference's).
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrt_mil_amd  # noqa: E402,F401  (the shim)
from rrt_mil_amd import synth  # noqa: E402
from _ref import load_reference  # noqa: E402
from transmil_cases import ATTN_CASES, MODEL_CASES, STAGE_GOLDEN_CASES, STAGE_ROWS, model_inputs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def cfg_bytes(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def signature(cls):
    out = []
    for name, p in list(inspect.signature(cls.__init__).parameters.items())[1:]:
        out.append([name, None if p.default is inspect.Parameter.empty else p.default])
    return out


class Recorder:
    """what the reference's NystromAttention.forward computed on the way, captured without touching its text"""

    def __init__(self, mod, attn):
        self.mod, self.attn, self.rec = mod, attn, {}

    def __enter__(self):
        m, rec = self.mod, self.rec
        self.saved = (m.reduce, m.einsum, m.moore_penrose_iter_pinv)

        def reduce(t, *a, **k):
            r = self.saved[0](t, *a, **k)
            rec.setdefault("landmarks", []).append(r)          # divided in place by the caller afterwards
            return r

        def einsum(eq, a, b):
            rec.setdefault("einsum", []).append((a, b))
            return self.saved[1](eq, a, b)

        def pinv(x, iters):
            rec["a2"] = x
            rec["z"] = self.saved[2](x, iters)
            return rec["z"]

        m.reduce, m.einsum, m.moore_penrose_iter_pinv = reduce, einsum, pinv
        self.h1 = self.attn.to_out.register_forward_pre_hook(lambda _m, inp: rec.__setitem__("o", inp[0]))
        self.h2 = self.attn.res_conv.register_forward_pre_hook(lambda _m, inp: rec.__setitem__("v", inp[0]))
        return rec

    def __exit__(self, *exc):
        self.mod.reduce, self.mod.einsum, self.mod.moore_penrose_iter_pinv = self.saved
        self.h1.remove()
        self.h2.remove()


def main():
    load_reference()
    from modules import nystrom_attention as na
    from modules import transmil as tm

    # ---- keys and signatures
    model = tm.TransMIL(1024, 2, False, "relu")
    attn = na.NystromAttention(512)
    np.savez(os.path.join(OUT, "transmil_keys.npz"), cfg=cfg_bytes({
        "transmil": [[k, list(v.shape)] for k, v in model.state_dict().items()],
        "nystrom": [[k, list(v.shape)] for k, v in attn.state_dict().items()],
        "transmil_signature": signature(tm.TransMIL),
        "nystrom_signature": signature(na.NystromAttention)}))

    # ---- attention cases
    attn_out, stage_out = {}, {}
    for dim, heads, n, gain in ATTN_CASES:
        state = synth.nystrom_state(dim, heads, gain=gain)
        x = torch.from_numpy(synth.nystrom_input(n, dim))[None]
        mod = na.NystromAttention(dim, heads=heads).eval()
        mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
        with torch.no_grad():
            y32 = mod(x)[0]
            mod = mod.double()
            with Recorder(na, mod) as rec:
                y64 = mod(x.double())[0]
        (q, kl), (ql, _), (_, k) = rec["einsum"]
        peak = max(float((a @ b.transpose(-1, -2)).abs().max()) for a, b in rec["einsum"])
        key = f"d{dim}_h{heads}_n{n}_g{int(gain)}"
        attn_out[key + "/y"] = torch.stack([y64[0], y64[-1]]).numpy()
        attn_out[key + "/e32"] = np.float64(rel(y32, y64))
        attn_out[key + "/peak"] = np.float64(peak)
        print(key, "peak %.1f" % peak, "e32 %.2e" % attn_out[key + "/e32"], flush=True)
        if (dim, heads, n, gain) in STAGE_GOLDEN_CASES:
            assert torch.equal(rec["landmarks"][0][0], ql[0]) and torch.equal(rec["landmarks"][1][0], kl[0])
            a3 = (ql @ k.transpose(-1, -2)).softmax(-1)
            av = a3 @ rec["v"]
            wz = rec["z"] @ av
            rows = slice(None, None, STAGE_ROWS)
            for name, t in (("ql", ql), ("kl", kl), ("a2", rec["a2"]), ("av", av), ("z", rec["z"]), ("wz", wz)):
                stage_out[f"{key}/{name}"] = t[0][:, rows].numpy()
            stage_out[f"{key}/o"] = rec["o"][0][-4:].numpy()
    np.savez(os.path.join(OUT, "transmil_attn.npz"), **attn_out)
    np.savez(os.path.join(OUT, "transmil_stages.npz"), **stage_out)

    # ---- whole-model cases
    model_out = {}
    for input_dim, act, N in MODEL_CASES:
        state, x = model_inputs(input_dim, N)
        ref = tm.TransMIL(input_dim, 2, False, act).eval()
        ref.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
        feats = {}
        hook = ref.norm.register_forward_pre_hook(lambda _m, inp: feats.__setitem__("feat", inp[0][0]))
        with torch.no_grad():
            l32 = ref(torch.from_numpy(x)[None])[0]
            f32 = feats["feat"]
            ref = ref.double()
            # forward() casts to fp32 in front of _fc1; the bag IS fp32 data, so feeding it to the double submodules in
            # double is the same bag: run forward with the cast neutralised
            xd = torch.from_numpy(x)[None].double()
            xd.float = lambda: xd
            l64 = ref(xd)[0]
            f64 = feats["feat"]
        hook.remove()
        assert l64.dtype == torch.float64 and f64.dtype == torch.float64
        key = f"i{input_dim}_{act}_n{N}"
        model_out[key + "/logits"] = l64.numpy()
        model_out[key + "/feat"] = torch.stack([f64[0], f64[1], f64[-1]]).numpy()
        model_out[key + "/e32_logits"] = np.float64(rel(l32, l64))
        model_out[key + "/e32_feat"] = np.float64(rel(f32, f64))
        print(key, l64.numpy(), "e32 %.2e %.2e" % (model_out[key + "/e32_logits"], model_out[key + "/e32_feat"]), flush=True)
    np.savez(os.path.join(OUT, "transmil_model.npz"), **model_out)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("transmil_"))
    print("transmil_* fixtures:", total, "bytes")
    assert total < 1_000_000


if __name__ == "__main__":
    main()
