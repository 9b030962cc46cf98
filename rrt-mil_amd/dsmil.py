"""MILNet / DSMIL -- the reference's dual-stream MIL head (modules/dsmil.py:96-135) around the MI355X encoder.

``--only_rrt_enc --model dsmil`` in the reference builds an RRTEncoder and hands it to ``MILNet(..., rrt=)``.  Same constructor,
module tree and parameter names (``patch_to_emb.0``, ``rrt``, ``i_classifier``, ``b_classifier.q``, ``b_classifier.fcc``):
reference checkpoints load with ``strict=True``.

Two streams (csrc/dsmil_pool.hip):
  * instance stream: ``classes = i_classifier(rrt(feats))`` [N, C]; its column maxima are the eval-mode second output and the
    ``max_loss`` input, its column arg-maxima the C critical instances (rrt_instance_max_f32; ties: the lowest index);
  * bag stream: on ``feats``, the embedding BEFORE the encoder (dsmil.py:124) -- the encoder influences it only through the
    choice of the critical instances, so the bag loss does not reach the encoder at all, and ``max_loss`` reaches it through
    exactly C rows.

In ``eval()`` without a graph a bag is ONE C-ABI call (rrt_dsmil_forward_f32: forward_bag / forward_bags).  With a graph the
encoder is its HIP autograd Function, the instance stream is `_InstanceMax` (sparse backward) and the bag stream the CLAM
heads' `_BranchPool` with y = hid_a = feats and the folded score rows c_w = q_w^T q_max / sqrt(Q); the [C, .] pieces are torch
ops.  The head's own arithmetic is fp32 in every compute mode.
"""
import ctypes as C
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._head import HeadState, _InstanceMax, copy_encoder_desc, head_compute, instance_max  # noqa: F401  (both live in _head.py: MaxMIL shares them)
from .clam import _BranchPool
from .encoder import RRTEncoder
from .mil import lib_linear


def initialize_weights(module):
    """modules/dsmil.py:5-19"""
    for m in module.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.xavier_normal_(m.weight)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)


class BClassifier(nn.Module):
    """modules/dsmil.py:59-94, the form MILNet builds (nonlinear=False, passing_v=False): the parameter holder of the bag
    stream.  Its forward is MILNet's (the HIP kernels); `_eager` restates the reference's op sequence in torch ops."""

    def __init__(self, input_size, output_class, dropout_v=0.0, nonlinear=False, passing_v=False):
        super().__init__()
        if nonlinear or passing_v:
            raise NotImplementedError("BClassifier(nonlinear=True / passing_v=True): MILNet never builds them")
        self.q = nn.Linear(input_size, 128)
        self.v = nn.Identity()
        self.fcc = nn.Conv1d(output_class, output_class, kernel_size=input_size)

    def _eager(self, feats, c):
        """dsmil.py:78-94 on torch ops (the benchmark's and the tests' comparison base, not used by forward)"""
        Q = self.q(feats)
        m_feats = torch.index_select(feats, 0, torch.sort(c, 0, descending=True)[1][0])
        A = F.softmax(torch.mm(Q, self.q(m_feats).transpose(0, 1)) / math.sqrt(Q.shape[1]), 0)
        B = torch.mm(A.transpose(0, 1), feats)
        return self.fcc(B.unsqueeze(0)).view(1, -1), A, B


class MILNet(HeadState, nn.Module):
    """modules/dsmil.py:96-135.  ``rrt``: an rrt_mil_amd.RRTEncoder of width 512, or None.

    ``forward(x, label=None, loss=None)`` returns what the reference returns: ``(prediction_bag [1, C], classes_max [C])`` in
    eval(), ``(prediction_bag, max_loss, ps)`` in train() for ``nn.CrossEntropyLoss`` / ``nn.BCEWithLogitsLoss``.  A bag of
    one instance works (A = 1, B = feats[0]; the reference's squeeze() breaks there).  Critical instances: among equal
    instance scores the lowest index."""

    def __init__(self, n_classes, dropout, act, input_dim=1024, rrt=None, **kwargs):
        super().__init__()
        if rrt is not None:
            if not isinstance(rrt, RRTEncoder):
                raise TypeError("rrt must be an rrt_mil_amd.RRTEncoder or None")
            if rrt.final_dim != 512:
                raise ValueError(f"rrt.final_dim must be 512 (the DSMIL embedding width), got {rrt.final_dim}")
        emb = [nn.Linear(input_dim, 512)]
        if act.lower() == 'relu':
            emb += [nn.ReLU()]
        elif act.lower() == 'gelu':
            emb += [nn.GELU()]
        self.patch_to_emb = nn.Sequential(*emb)
        self.dp = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.rrt = rrt if rrt is not None else nn.Identity()
        self.i_classifier = nn.Linear(512, n_classes)
        self.b_classifier = BClassifier(512, n_classes)
        self.apply(initialize_weights)
        self.n_classes = n_classes
        self._emb_act = {"relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU}.get(act.lower(), _lib.ACT_NONE)
        self._has_dropout = dropout > 0.
        self._ws = None

    # ------------------------------------------------------------------ pieces
    def _enc(self):
        return self.rrt if isinstance(self.rrt, RRTEncoder) else None

    def _compute(self):
        return head_compute(self._enc())

    def _stochastic(self):
        enc = self._enc()
        return self.training and (self._has_dropout or (enc is not None and enc._stochastic()))

    # ------------------------------------------------------------------ the one-call HIP path
    def _desc_weights(self, in_dim, solo):
        enc, p = self._enc(), RRTEncoder._ptr
        d, w = _lib.DsmilDesc(), _lib.DsmilWeights()
        if enc is not None:
            copy_encoder_desc(d.enc, enc, "DSMIL")
            w.enc = enc._weights()
        d.enc.dim = 512
        d.enc.compute = self._compute()
        d.enc.solo = int(bool(solo))       # per-call scheduling hint, never inherited (see RRTMIL._mil_desc)
        d.input_dim, d.emb_act, d.has_rrt = in_dim, self._emb_act, int(enc is not None)
        d.n_classes, d.q_dim = self.n_classes, self.b_classifier.q.out_features
        lin, ic, q, fcc = self.patch_to_emb[0], self.i_classifier, self.b_classifier.q, self.b_classifier.fcc
        w.emb_w, w.emb_b = p(lin.weight), p(lin.bias)
        w.icls_w, w.icls_b = p(ic.weight), p(ic.bias)
        w.q_w, w.q_b = p(q.weight), p(q.bias)
        w.fcc_w, w.fcc_b = p(fcc.weight), p(fcc.bias)
        return d, w

    def forward_bag(self, x2d, return_attn=False, return_features=False, return_critical=False, solo=True):
        """One bag, eval, no graph: x2d (N, input_dim) fp32 device tensor -> {logits (1, C), classes_max (C,)} through ONE
        rrt_dsmil_forward_f32 call, plus what was asked for: attn (N, C) (the reference's A), features (C, 512) (its B),
        critical (C,) int64 (the critical instances).  ``solo``: the slide has the GPU to itself (forward_bags passes False
        with several slides in flight)."""
        if not x2d.is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.MILNet runs on MI355X only: move the bag to a 'cuda' (HIP) device; there is "
                                   "no CPU fallback")
        if self._stochastic():
            raise NotImplementedError("forward_bag is the one-call inference entry (no dropout inside); in train() call the "
                                      "module itself")
        n, in_dim = x2d.shape
        if in_dim != self.patch_to_emb[0].in_features:
            raise ValueError(f"expected feature dim {self.patch_to_emb[0].in_features}, got {in_dim}")
        x2d = x2d.float().contiguous()
        d, w = self._desc_weights(in_dim, solo)
        dev = x2d.device
        nc = self.n_classes
        new = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)   # noqa: E731
        logits, cmax = new(1, nc), new(nc)
        attn = new(n, nc) if return_attn else None
        feat = new(nc, 512) if return_features else None
        crit = new(nc, dt=torch.int64) if return_critical else None
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        self._head_forward("dsmil", d, w, x2d, (logits.data_ptr(), cmax.data_ptr(), p(attn), p(feat), p(crit)),
                           d.enc.compute != _lib.COMPUTE_F32 and d.has_rrt)
        return {k: v for k, v in (("logits", logits), ("classes_max", cmax), ("attn", attn), ("features", feat),
                                  ("critical", crit)) if v is not None}

    def forward_bags(self, bags, streams=4, **kw):
        """A batch of independent slides (each (N_i, input_dim) or (1, N_i, input_dim)) -> list of forward_bag results, with
        ``streams`` slides in flight on the heads' bag scheduler (HeadState._schedule_bags: one rrt_dsmil_forward_f32 call
        per slide with its own workspace), bit for bit forward_bag(..., solo=False) per bag."""
        if not bags:
            return []
        if not bags[0].is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.MILNet runs on MI355X only; there is no CPU fallback")
        if self._stochastic():
            raise NotImplementedError("forward_bags is an inference entry; in train() call the module itself")
        return self._schedule_bags(bags, streams, lambda x2, solo: self.forward_bag(x2, solo=solo, **kw), lambda o: o.values())

    # ------------------------------------------------------------------ the layer path (graph, dropout, eager comparison)
    def _embed(self, x2d):
        """patch_to_emb (+ Dropout) -> feats (N, 512)"""
        compute = self._compute()
        compute = _lib.COMPUTE_F32 if compute == _lib.COMPUTE_F32X3 else compute
        x = lib_linear(self.patch_to_emb[0], x2d, compute).float()
        for m in list(self.patch_to_emb)[1:]:
            x = m(x)
        return self.dp(x)

    def _streams(self, feats):
        """feats (N, 512) -> (prediction_bag (1, C), classes_max (C,), critical (C,), A (N, C) no grad, B (C, 512))"""
        y = self.rrt(feats)
        with torch.autocast("cuda", enabled=False):
            feats, y = feats.float(), y.float()
            ic, q, fcc = self.i_classifier, self.b_classifier.q, self.b_classifier.fcc
            cmax, idx = _InstanceMax.apply(y, ic.weight, ic.bias)
            q_max = F.linear(feats.index_select(0, idx), q.weight, q.bias)          # (C, Q)
            scale = 1.0 / math.sqrt(q.out_features)
            c_w = torch.mm(q_max, q.weight) * scale                                  # (C, 512): s[c, n] = c_w[c] . feats_n + c_b[c]
            c_b = (torch.mv(q_max, q.bias) * scale) if q.bias is not None else None
            B, A, _raw = _BranchPool.apply(feats, feats, None, c_w, c_b)
            pred = F.conv1d(B.unsqueeze(0), fcc.weight, fcc.bias).view(1, -1)
        return pred, cmax, idx, A.transpose(0, 1), B

    def forward(self, x, label=None, loss=None):
        if not x.is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.MILNet runs on MI355X only: move the bag to a 'cuda' (HIP) device; there is "
                                   "no CPU fallback")
        ps = x.size(1) if x.dim() == 3 else x.size(0)
        x2d = x.reshape(-1, x.shape[-1])
        graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if not self.training and not graph:
            out = self.forward_bag(x2d)
            return out["logits"], out["classes_max"]
        if x2d.shape[1] != self.patch_to_emb[0].in_features:
            raise ValueError(f"expected feature dim {self.patch_to_emb[0].in_features}, got {x2d.shape[1]}")
        with torch.set_grad_enabled(graph):
            pred, cmax, _idx, _A, _B = self._streams(self._embed(x2d))
            if not self.training:
                return pred, cmax
            if isinstance(loss, nn.CrossEntropyLoss):
                max_loss = loss(cmax.view(1, -1), label)
            elif isinstance(loss, nn.BCEWithLogitsLoss):
                max_loss = loss(cmax.view(1, -1), label.view(1, -1).float())
            else:
                raise TypeError("train(): loss must be an nn.CrossEntropyLoss or an nn.BCEWithLogitsLoss (dsmil.py:128-133)")
        return pred, max_loss, ps


DSMIL = MILNet
