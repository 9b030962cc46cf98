"""DTFD-MIL -- the reference's ``--model dtfd`` (Survival/models/DTFD/network.py; the same blocks sit in DTFD/Model/) around the
MI355X encoder: the double-tier head whose first tier splits the bag into ``group`` pseudo-bags, pools each with its own
softmax attention and distils, per pseudo-bag, the instances with the highest and the lowest class-activation probability
(``MaxMinS``), the highest alone (``MaxS``) or the pooled row (``AFS``); the second tier is a gated attention pool and a
classifier over the distilled rows.

Same class names, constructor signatures and parameter keys as the reference: its checkpoints load with ``strict=True``, both
ways.  ``rrt=`` takes an ``rrt_mil_amd.RRTEncoder`` of width 512 or ``None`` (the reference builds its own from a flag).

In ``eval()`` under ``torch.no_grad()`` a bag is ONE C-ABI call (rrt_dtfd_forward_f32: the heads' shared front, the gate
Linears, csrc/segment_pool.hip, a row gather and the ABMIL tail); ``model(bag)`` draws the permutation with ``random.shuffle``
exactly as the reference does, so the same ``random.seed`` gives the same pseudo-bags.  In ``train()``, or with a graph, the
layer path runs: the front on the library GEMM (per chunk when there is an encoder, once over the bag otherwise -- the same
function, with one dropout draw in place of ``group``), the scores as torch modules, and ``_SegmentPool`` -- an autograd
Function over rrt_segment_pool_f32 / rrt_segment_pool_backward_f32 -- for every pseudo-bag's pooling, CAM and selection.

Kept from the reference: ``train_forward`` computes the pseudo-bag loss with the ``criterion`` it was built with, calls
``optimizer0.zero_grad()`` and ``loss0.backward(retain_graph=True)`` INSIDE the forward, and returns ``(hazards, S)`` of the
second tier; the CAM uses the classifier's weight without its bias; scores are not normalised before the split in eval.
Fixed here: among equal CAM probabilities the lower position in group order is selected at both ends (``torch.sort`` leaves it
open), a NaN is never selected; a bag with fewer instances than ``group`` is refused (the reference lets its empty chunks add
no rows).
"""
import ctypes as C
import random

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._head import BagHead, HeadState, copy_encoder_desc, head_compute
from .mil import lib_linear

DISTILL = {"MaxMinS": _lib.DTFD_MAXMINS, "MaxS": _lib.DTFD_MAXS, "AFS": _lib.DTFD_AFS}


def initialize_weights(module):
    """network.py:13-27"""
    for m in module.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.xavier_normal_(m.weight)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)


def _robust_init(module, n_robust):
    """the reference's ``n_robust`` re-initialisation: a second init under its own seed, then n_robust draws to move the
    global generator on"""
    if n_robust > 0:
        rng = torch.random.get_rng_state()
        torch.random.manual_seed(n_robust)
        module.apply(initialize_weights)
        torch.random.set_rng_state(rng)
        [torch.rand((1024, 512)) for _ in range(n_robust)]


def get_cam_1d(classifier, features):
    """network.py:30-33: features (b, g, f) against the classifier's weight (c, f), no bias -> (b, c, g)"""
    tweight = list(classifier.parameters())[-2]
    return torch.einsum("bgf,cf->bcg", [features, tweight])


def split_sizes(n, group):
    """np.array_split's chunk sizes in closed form: the first n % group chunks hold n // group + 1 rows"""
    q, r = divmod(int(n), int(group))
    return [q + 1] * r + [q] * (group - r)


def _compute_of(enc):
    compute = head_compute(enc)
    return _lib.COMPUTE_F32 if compute == _lib.COMPUTE_F32X3 else compute


class _SegmentPool(torch.autograd.Function):
    """(mid (N, dim), a (N,), cls_w (C, dim), group, perm (N,) int64 or None) -> pooled (group, dim), sel (group, 2) int64,
    attn (N,), p (N,) through rrt_segment_pool_f32; the gradient reaches mid and a through pooled alone
    (rrt_segment_pool_backward_f32).  sel, attn and p carry no gradient: what reaches mid through the selected rows is
    index_select's."""

    @staticmethod
    def forward(ctx, mid, a, cls_w, group, perm):
        lib = _lib.load()
        if not mid.is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.dtfd runs on MI355X only; there is no CPU fallback")
        mid, a = mid.detach().float().contiguous(), a.detach().float().contiguous()
        cls_w = cls_w.detach().float().contiguous()
        perm = perm.to(device=mid.device, dtype=torch.int64).contiguous() if perm is not None else None
        (n, d), c, dev = mid.shape, cls_w.shape[0], mid.device
        pooled = torch.empty((group, d), dtype=torch.float32, device=dev)
        sel = torch.empty((group, 2), dtype=torch.int64, device=dev)
        attn = torch.empty(n, dtype=torch.float32, device=dev)
        p = torch.empty(n, dtype=torch.float32, device=dev)
        need = C.c_size_t()
        _lib.check(lib.rrt_segment_pool_workspace_size(n, d, c, group, C.byref(need)), "rrt_segment_pool_workspace_size")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_segment_pool_f32(mid.data_ptr(), a.data_ptr(), perm.data_ptr() if perm is not None else None,
                                                cls_w.data_ptr(), pooled.data_ptr(), sel.data_ptr(), attn.data_ptr(), p.data_ptr(),
                                                n, d, c, group, ws.data_ptr(), ws.numel(), st), "rrt_segment_pool_f32")
        ctx.save_for_backward(mid, a, pooled, ws)      # (the workspace keeps every group's (m_g, l_g) for the backward)
        ctx.perm, ctx.group = perm, group
        ctx.mark_non_differentiable(sel, attn, p)
        return pooled, sel, attn, p

    @staticmethod
    def backward(ctx, d_pooled, _d_sel, _d_attn, _d_p):
        lib = _lib.load()
        mid, a, pooled, ws = ctx.saved_tensors
        d_pooled = d_pooled.float().contiguous()
        (n, d), dev, perm = mid.shape, mid.device, ctx.perm
        d_mid, d_a = torch.empty_like(mid), torch.empty_like(a)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_segment_pool_backward_f32(mid.data_ptr(), a.data_ptr(), perm.data_ptr() if perm is not None else None,
                                                         pooled.data_ptr(), d_pooled.data_ptr(), d_mid.data_ptr(), d_a.data_ptr(),
                                                         n, d, ctx.group, ws.data_ptr(), ws.numel(), st),
                       "rrt_segment_pool_backward_f32")
        return d_mid, d_a, None, None, None


class Classifier_1fc(nn.Module):
    """network.py:36-59"""

    def __init__(self, n_channels, n_classes, droprate=0.0, n_robust=0):
        super().__init__()
        self.fc = nn.Linear(n_channels, n_classes)
        self.droprate = droprate
        if self.droprate != 0.0:
            self.dropout = torch.nn.Dropout(p=self.droprate)
        self.apply(initialize_weights)
        _robust_init(self, n_robust)

    def forward(self, x):
        if self.droprate != 0.0:
            x = self.dropout(x)
        return self.fc(x)


class DimReduction(nn.Module):
    """network.py:62-92: Linear(n_channels, m_dim, bias=False) + ReLU / GELU (+ Dropout(0.25) in train()) (+ the encoder).
    ``rrt``: an rrt_mil_amd.RRTEncoder of width m_dim, or None / False."""

    def __init__(self, n_channels, m_dim=512, dropout=False, act="relu", n_robust=0, rrt=None):
        super().__init__()
        rrt = None if rrt is False else rrt
        BagHead._check_rrt(rrt)
        self.fc1 = nn.Linear(n_channels, m_dim, bias=False)
        self.rrt = rrt if rrt is not None else nn.Identity()
        self.relu1 = nn.ReLU() if act.lower() == "relu" else nn.GELU()
        self.drop = nn.Dropout(0.25)
        self.dropout = dropout
        if rrt is None:                 # (an encoder handed in keeps the parameters it came with)
            self.apply(initialize_weights)
            _robust_init(self, n_robust)
        else:
            initialize_weights(self.fc1)

    def _enc(self):
        return None if isinstance(self.rrt, nn.Identity) else self.rrt

    def forward(self, x):
        x = lib_linear(self.fc1, x, _compute_of(self._enc())).float()
        x = self.relu1(x)
        if self.dropout:
            x = self.drop(x)
        return self.rrt(x)


class Attention(nn.Module):
    """network.py:108-143: gated attention scores, K x N (softmax over N unless ``isNorm=False``)"""

    def __init__(self, L=512, D=128, K=1, n_robust=0):
        super().__init__()
        self.L, self.D, self.K = L, D, K
        self.attention_V = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh())
        self.attention_U = nn.Sequential(nn.Linear(self.L, self.D), nn.Sigmoid())
        self.attention_weights = nn.Linear(self.D, self.K)
        self.apply(initialize_weights)
        _robust_init(self, n_robust)

    def forward(self, x, isNorm=True):
        A_V = self.attention_V[1](lib_linear(self.attention_V[0], x, _lib.COMPUTE_F32).float())
        A_U = self.attention_U[1](lib_linear(self.attention_U[0], x, _lib.COMPUTE_F32).float())
        A = self.attention_weights(A_V * A_U)
        A = torch.transpose(A, 1, 0)
        if isNorm:
            A = F.softmax(A, dim=1)
        return A


class Attention_with_Classifier(nn.Module):
    """network.py:95-105"""

    def __init__(self, L=512, D=128, K=1, num_cls=2, droprate=0, n_robust=0):
        super().__init__()
        self.attention = Attention(L, D, K, n_robust=n_robust)
        self.classifier = Classifier_1fc(L, num_cls, droprate, n_robust=n_robust)

    def forward(self, x):
        AA = self.attention(x)
        afeat = torch.mm(AA, x)
        return self.classifier(afeat)


class DTFD(HeadState, nn.Module):
    """network.py:146-280.  ``forward(x, label=None)``: x (1, N, input_dim) or (N, input_dim) -> ``(hazards, S)``, both
    (1, n_classes); in ``train()`` ``label`` is the reference's dict with ``label`` and ``censorship`` and the pseudo-bag loss
    is back-propagated inside the call (its value stays in ``self.loss0``)."""

    def __init__(self, lr, weight_decay, steps, criterion, rrt=None, epeg_k=15, crmsa_k=3, input_dim=1024, inner_dim=512,
                 n_classes=2, group=8, distill="MaxMinS"):
        super().__init__()
        if inner_dim != 512:
            raise ValueError(f"DTFD(inner_dim={inner_dim}): the blocks behind the embedding are built 512 wide "
                             "(Attention(inner_dim) beside Attention_with_Classifier's default D), only inner_dim=512 can run")
        if distill not in DISTILL:
            raise ValueError(f"distill must be one of {sorted(DISTILL)}, got {distill!r}")
        if not 1 <= int(group) <= _lib.SEGMENT_POOL_MAX_GROUPS:
            raise ValueError(f"group must be in 1..{_lib.SEGMENT_POOL_MAX_GROUPS}, got {group}")
        if not 1 <= int(n_classes) <= 8:
            raise ValueError(f"n_classes must be in 1..8 (the CAM selection holds a row's class scores in registers), got {n_classes}")
        self.classifier = Classifier_1fc(inner_dim, n_classes, 0.25)
        self.attention = Attention(inner_dim)
        self.dimReduction = DimReduction(input_dim, inner_dim, rrt=rrt, dropout=0.25)
        self.UClassifier = Attention_with_Classifier(L=inner_dim, num_cls=n_classes, droprate=0.25)
        self.group = group
        self.distill = distill
        self.criterion = criterion
        trainable_parameters = []
        trainable_parameters += list(self.classifier.parameters())
        trainable_parameters += list(self.attention.parameters())
        trainable_parameters += list(self.dimReduction.parameters())
        self.optimizer0 = torch.optim.Adam(trainable_parameters, lr=lr, weight_decay=weight_decay)
        self.scheduler0 = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer0, steps, 0)
        self.loss0 = None
        self._ws = None

    # ------------------------------------------------------------------ checks
    def _check_bag(self, x2d):
        k = self.dimReduction.fc1.in_features
        if x2d.dim() != 2 or x2d.shape[0] == 0 or x2d.shape[1] != k:
            raise ValueError(f"expected a bag of shape (N, {k}), got {tuple(x2d.shape)}")
        if x2d.shape[0] < self.group:
            raise ValueError(f"DTFD(group={self.group}): a bag of {x2d.shape[0]} instances leaves pseudo-bags empty; the reference "
                             "lets the empty chunks add no rows, this library refuses the bag")
        if not x2d.is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.DTFD runs on MI355X only: move the bag to a 'cuda' (HIP) device; there is no CPU "
                                   "fallback")

    # ------------------------------------------------------------------ the one-call HIP path
    def _desc_weights(self):
        from .encoder import RRTEncoder
        enc, p = self.dimReduction._enc(), RRTEncoder._ptr
        d, w = _lib.DtfdDesc(), _lib.DtfdWeights()
        if enc is not None:
            copy_encoder_desc(d.enc, enc, "DTFD")
            w.enc = enc._weights()
        d.enc.dim = 512
        d.enc.compute = head_compute(enc)
        d.enc.solo = 1                     # one bag in flight (forward_bags is a plain loop)
        fc1, act = self.dimReduction.fc1, self.dimReduction.relu1
        d.input_dim, d.emb_act = fc1.in_features, (_lib.ACT_RELU if isinstance(act, nn.ReLU) else _lib.ACT_GELU)
        d.has_rrt, d.n_classes, d.hidden = int(enc is not None), self.classifier.fc.out_features, self.attention.D
        d.group, d.distill = int(self.group), DISTILL[self.distill]
        t1, t2, ucls = self.attention, self.UClassifier.attention, self.UClassifier.classifier.fc
        w.emb_w, w.cls_w = p(fc1.weight), p(self.classifier.fc.weight)
        w.att_v_w, w.att_v_b = p(t1.attention_V[0].weight), p(t1.attention_V[0].bias)
        w.att_u_w, w.att_u_b = p(t1.attention_U[0].weight), p(t1.attention_U[0].bias)
        w.att_w_w, w.att_w_b = p(t1.attention_weights.weight), p(t1.attention_weights.bias)
        w.u_v_w, w.u_v_b = p(t2.attention_V[0].weight), p(t2.attention_V[0].bias)
        w.u_u_w, w.u_u_b = p(t2.attention_U[0].weight), p(t2.attention_U[0].bias)
        w.u_w_w, w.u_w_b = p(t2.attention_weights.weight), p(t2.attention_weights.bias)
        w.u_fc_w, w.u_fc_b = p(ucls.weight), p(ucls.bias)
        return d, w

    def forward_bag(self, x2d, perm=None, return_sel=False, return_cam=False):
        """One bag, inference, no graph: x2d (N, input_dim) fp32 device tensor -> logits (1, n_classes) through ONE
        rrt_dtfd_forward_f32 call.  ``perm``: the order in which the N rows are dealt to the pseudo-bags (a sequence or
        tensor holding a permutation of range(N); None: the identity -- contiguous chunks).  With ``return_sel`` /
        ``return_cam`` a tuple (logits[, sel (group, 2) int64: each pseudo-bag's rows of highest and lowest CAM probability]
        [, p (N,): every row's CAM probability -- the heat map])."""
        self._check_bag(x2d)
        x2d = x2d.float().contiguous()
        n, dev = x2d.shape[0], x2d.device
        if perm is not None:
            perm = torch.as_tensor(perm, dtype=torch.int64).to(dev).contiguous()
            if perm.shape != (n,):
                raise ValueError(f"perm must hold a permutation of range({n}), got shape {tuple(perm.shape)}")
        d, w = self._desc_weights()
        logits = torch.empty((1, d.n_classes), dtype=torch.float32, device=dev)
        sel = torch.empty((d.group, 2), dtype=torch.int64, device=dev) if return_sel else None
        cam = torch.empty(n, dtype=torch.float32, device=dev) if return_cam else None
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        self._head_forward("dtfd", d, w, x2d, (p(perm), logits.data_ptr(), p(sel), p(cam)),
                           d.enc.compute != _lib.COMPUTE_F32 and d.has_rrt)
        out = (logits,) + ((sel,) if return_sel else ()) + ((cam,) if return_cam else ())
        return out[0] if len(out) == 1 else out

    def forward_bags(self, bags, **kw):
        """a plain loop of forward_bag over slides (each (N_i, input_dim) or (1, N_i, input_dim))"""
        return [self.forward_bag(b[0] if b.dim() == 3 else b, **kw) for b in bags]

    # ------------------------------------------------------------------ the layer path
    def _front_chunks(self, x, sizes):
        """the front: once over the bag without an encoder, per pseudo-bag with one (the encoder sees one chunk at a time)"""
        if self.dimReduction._enc() is None:
            return self.dimReduction(x)
        return torch.cat([self.dimReduction(c) for c in torch.split(x, sizes, dim=0)], dim=0)

    def _distilled(self, mid, pooled, sel):
        if self.distill == "MaxMinS":
            return mid.index_select(0, sel.reshape(-1))
        if self.distill == "MaxS":
            return mid.index_select(0, sel[:, 0].contiguous())
        return pooled

    def _tier2(self, rows):
        logits = self.UClassifier(rows)
        hazards = torch.sigmoid(logits)
        return hazards, torch.cumprod(1 - hazards, dim=1)

    def train_forward(self, x, label):
        self._check_bag(x)
        sizes = split_sizes(x.shape[0], self.group)
        mid = self._front_chunks(x.float(), sizes).float()
        a = self.attention(mid, isNorm=False).squeeze(0)
        pooled, sel, _attn, _p = _SegmentPool.apply(mid, a, self.classifier.fc.weight, int(self.group), None)
        tPredict = self.classifier(pooled)
        tHazards = torch.sigmoid(tPredict)
        tS = torch.cumprod(1 - tHazards, dim=1)
        labels, censorship = [label["label"]] * self.group, [label["censorship"]] * self.group
        loss0 = self.criterion(hazards=tHazards, S=tS, Y=torch.tensor(labels).to(x.device), c=torch.tensor(censorship).to(x.device))
        self.optimizer0.zero_grad()
        loss0.backward(retain_graph=True)
        self.loss0 = loss0.detach()
        return self._tier2(self._distilled(mid, pooled, sel))

    def _test_forward_layers(self, x, perm):
        """test_forward with a graph: the front over the whole bag, every pseudo-bag through _SegmentPool"""
        mid = self.dimReduction(x.float()).float()
        a = self.attention(mid, isNorm=False).squeeze(0)
        pooled, sel, _attn, _p = _SegmentPool.apply(mid, a, self.classifier.fc.weight, int(self.group), perm)
        return self._tier2(self._distilled(mid, pooled, sel))

    def test_forward(self, x):
        self._check_bag(x)
        feat_index = list(range(x.shape[0]))
        random.shuffle(feat_index)
        perm = torch.from_numpy(np.array(feat_index, dtype=np.int64))
        graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if graph:
            return self._test_forward_layers(x, perm.to(x.device))
        logits = self.forward_bag(x, perm=perm)
        hazards = torch.sigmoid(logits)
        return hazards, torch.cumprod(1 - hazards, dim=1)

    def forward(self, x, label=None):
        if x.dim() == 3:
            if x.shape[0] != 1:
                raise ValueError(f"DTFD takes one bag per call, got a batch of {x.shape[0]}")
            x = x.squeeze(0)
        if self.training:
            return self.train_forward(x, label)
        return self.test_forward(x)
