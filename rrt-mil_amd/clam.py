"""CLAM_SB / CLAM_MB -- the reference's CLAM heads (modules/clam.py) around the MI355X encoder.

The reference re-embeds features for any MIL head: ``--only_rrt_enc --model clam_sb|clam_mb`` builds an RRTEncoder and hands it
to the head as ``rrt=`` (main.py:138-153, modules/clam.py:104-105, :237-238).  Same constructor, the same ``attention_net``
``nn.Sequential`` layout (its indices shift with ``dropout`` / ``rrt``), the same parameter and buffer names: reference
checkpoints load with ``strict=True``.

Hot path: csrc/clam_pool.hip.  The K attention branches (1 for CLAM_SB, n_classes for CLAM_MB) are pooled from ONE pass over
the encoder output, and the k_sample highest- / lowest-attention instances of a branch come from rrt_topk_rows_f32.  In
``eval()`` without a graph a bag is ONE C-ABI call (rrt_clam_forward_f32: forward_bag / forward_bags); with a graph the
encoder is the HIP autograd Function, the gate Linears run on the library GEMMs and the pooling is `_BranchPool`.
"""
import ctypes as C
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._head import HeadState, copy_encoder_desc, head_compute
from .encoder import RRTEncoder
from .mil import lib_linear


def initialize_weights(module):
    """modules/clam.py:7-15"""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_normal_(m.weight)
            m.bias.data.zero_()
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)


class SmoothTop1SVM(nn.Module):
    """The smooth top-1 SVM loss CLAM supervises its instance classifiers with (Berrada et al., "Smooth Loss Functions for
    Deep Top-k Classification", ICLR 2018, eq. 5 at k = 1), as a few torch ops:

        row loss = tau * logsumexp_j((x_j + alpha * [j != y] - x_y) / tau)                      (smooth)
                 = max_j(x_j + alpha * [j != y]) - x_y      where top1 - top2 >= tau * ln(1000)   (hard: the smooth form's limit)

    averaged over the rows.  ``labels`` is a buffer (arange(n_classes)) so that ``instance_loss_fn.labels`` is part of the
    state dict as in the reference."""

    def __init__(self, n_classes=2, alpha=None, tau=1.0):
        super().__init__()
        self.alpha = 1.0 if alpha is None else float(alpha)
        self.tau = float(tau)
        self.thresh = 1e3
        self.n_classes = n_classes
        self.register_buffer("labels", torch.arange(n_classes, dtype=torch.int64))

    def forward(self, x, y):
        margin = x + self.alpha * (y[:, None] != self.labels.to(y.device)[None, :]).to(x.dtype)
        gt = x.gather(1, y[:, None])
        top = x.topk(2, dim=1)[0]
        hard = ((top[:, 0] - top[:, 1]) >= self.tau * math.log(self.thresh)).detach()
        smooth_loss = self.tau * torch.logsumexp((margin - gt) / self.tau, dim=1)
        hard_loss = margin.max(1)[0] - gt.squeeze(1)
        return torch.where(hard, hard_loss, smooth_loss).sum() / x.size(0)


class Attn_Net(nn.Module):
    """modules/clam.py:25-41 (attention network without gating)."""

    def __init__(self, L=1024, D=256, dropout=False, n_classes=1):
        super().__init__()
        mods = [nn.Linear(L, D), nn.Tanh()]
        if dropout:
            mods.append(nn.Dropout(0.25))
        mods.append(nn.Linear(D, n_classes))
        self.module = nn.Sequential(*mods)

    def forward(self, x):
        return self.module(x), x


class Attn_Net_Gated(nn.Module):
    """modules/clam.py:51-74 (attention network with sigmoid gating)."""

    def __init__(self, L=1024, D=256, dropout=False, n_classes=1):
        super().__init__()
        a = [nn.Linear(L, D), nn.Tanh()]
        b = [nn.Linear(L, D), nn.Sigmoid()]
        if dropout:
            a.append(nn.Dropout(0.25))
            b.append(nn.Dropout(0.25))
        self.attention_a = nn.Sequential(*a)
        self.attention_b = nn.Sequential(*b)
        self.attention_c = nn.Linear(D, n_classes)

    def forward(self, x):
        return self.attention_c(self.attention_a(x).mul(self.attention_b(x))), x


def topk_rows(a, k):
    """a (K, N) fp32 device tensor -> ids (K, 2, k) int64: [:, 0] the k largest of each row in descending order, [:, 1] the k
    smallest in ascending order (rrt_topk_rows_f32).  Equal values: the lower index first.  NaN entries are never selected; a
    row with fewer than k non-NaN values has its unused slots set to -1."""
    lib = _lib.load()
    if not a.is_cuda:
        raise _lib.RRTHipError("rrt_mil_amd.clam runs on MI355X only; there is no CPU fallback")
    a = a.detach().float().contiguous()
    rows, n = a.shape
    ids = torch.empty((rows, 2, k), dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        st = torch.cuda.current_stream(a.device).cuda_stream
        _lib.check(lib.rrt_topk_rows_f32(a.data_ptr(), ids.data_ptr(), rows, n, k, st), "rrt_topk_rows_f32")
    return ids


class _BranchPool(torch.autograd.Function):
    """K attention branches over one bag as ONE library call each way (rrt_branch_pool_f32 / rrt_branch_pool_backward_f32):
    s[c, n] = c_w[c] . h_n + c_b[c] (h = hid_a, or hid_a * hid_b when gated), attn = softmax over the bag per branch,
    pooled[c] = sum_n attn[c, n] y_n.  Returns (pooled [K, dim], attn [K, N], a_raw [K, N]); the gradient flowing into the
    raw scores is honoured, the returned attention is not differentiable (CLAM only takes instance ids from it)."""

    @staticmethod
    def forward(ctx, y2d, hid_a, hid_b, c_w, c_b):
        lib = _lib.load()
        y2d, hid_a = y2d.float().contiguous(), hid_a.float().contiguous()
        hid_b = hid_b.float().contiguous() if hid_b is not None else None
        n, d = y2d.shape
        hdim, k = hid_a.shape[1], c_w.shape[0]
        dev = y2d.device
        pooled = torch.empty((k, d), dtype=torch.float32, device=dev)
        attn = torch.empty((k, n), dtype=torch.float32, device=dev)
        a_raw = torch.empty((k, n), dtype=torch.float32, device=dev)
        need = C.c_size_t()
        _lib.check(lib.rrt_branch_pool_workspace_size(n, d, hdim, k, C.byref(need)), "rrt_branch_pool_workspace_size")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        cw = c_w.float().contiguous()
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_branch_pool_f32(y2d.data_ptr(), hid_a.data_ptr(), hid_b.data_ptr() if hid_b is not None else None,
                                               cw.data_ptr(), c_b.data_ptr() if c_b is not None else None, pooled.data_ptr(),
                                               attn.data_ptr(), a_raw.data_ptr(), n, d, hdim, k, ws.data_ptr(), ws.numel(), st),
                       "rrt_branch_pool_f32")
        ctx.save_for_backward(y2d, hid_a, hid_b, cw, attn, pooled)
        ctx.has_bias = c_b is not None
        ctx.mark_non_differentiable(attn)
        ctx.set_materialize_grads(False)
        return pooled, attn, a_raw

    @staticmethod
    def backward(ctx, d_pooled, _d_attn, d_raw):
        lib = _lib.load()
        y2d, hid_a, hid_b, cw, attn, pooled = ctx.saved_tensors
        n, d = y2d.shape
        hdim, k = hid_a.shape[1], cw.shape[0]
        dev = y2d.device
        d_pooled = torch.zeros((k, d), dtype=torch.float32, device=dev) if d_pooled is None else d_pooled.float().contiguous()
        d_raw = d_raw.float().contiguous() if d_raw is not None else None
        dy = torch.empty_like(y2d)
        dha = torch.empty_like(hid_a)
        dhb = torch.empty_like(hid_b) if hid_b is not None else None
        dwcb = torch.empty(k * hdim + 8, dtype=torch.float32, device=dev)
        need = C.c_size_t()
        _lib.check(lib.rrt_branch_pool_workspace_size(n, d, hdim, k, C.byref(need)), "rrt_branch_pool_workspace_size")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_branch_pool_backward_f32(y2d.data_ptr(), hid_a.data_ptr(), p(hid_b), cw.data_ptr(), attn.data_ptr(),
                                                        pooled.data_ptr(), d_pooled.data_ptr(), p(d_raw), dy.data_ptr(),
                                                        dha.data_ptr(), p(dhb), dwcb.data_ptr(), n, d, hdim, k, ws.data_ptr(),
                                                        ws.numel(), st), "rrt_branch_pool_backward_f32")
        dcw = dwcb[:k * hdim].reshape(k, hdim)
        dcb = dwcb[k * hdim:k * hdim + k].clone() if ctx.has_bias else None
        return dy, dha, dhb, dcw, dcb


class CLAM_SB(HeadState, nn.Module):
    """modules/clam.py:88-218.  ``rrt``: an rrt_mil_amd.RRTEncoder of width 512, or None.

    ``forward(h, label=None, instance_eval=True, return_features=False, attention_only=False)`` returns what the reference
    returns: ``(logits, total_inst_loss, ps)`` with instance evaluation, ``logits`` without, ``A_raw`` (K, N) for
    ``attention_only``.  With ``label=None`` the reference dies in ``F.one_hot`` (TypeError); here the instance branch is
    skipped and ``logits`` is returned, as with ``instance_eval=False``.  ``return_features`` only fills the reference's
    local results dict (it never reaches the caller there); here the last bag embedding M (K, 512) is also kept as
    ``self.last_features``.  Top-k instance ids: among equal attention values the lower index comes first."""
    _per_branch = False

    def __init__(self, input_dim, gate=True, size_arg="small", dropout=0., k_sample=8, n_classes=2,
                 instance_loss_fn=None, subtyping=False, test=False, act='relu', rrt=None):
        super().__init__()
        self._build(input_dim, gate, size_arg, dropout, k_sample, n_classes, subtyping, act, rrt,
                    {"small": [input_dim, 512, 256], "big": [input_dim, 512, 384], "hipt": [192, 512, 256]})

    def _build(self, input_dim, gate, size_arg, dropout, k_sample, n_classes, subtyping, act, rrt, size_dict):
        if rrt is not None:
            if not isinstance(rrt, RRTEncoder):
                raise TypeError("rrt must be an rrt_mil_amd.RRTEncoder or None")
            if rrt.final_dim != 512:
                raise ValueError(f"rrt.final_dim must be 512 (the CLAM embedding width), got {rrt.final_dim}")
        self.size_dict = size_dict
        size = size_dict[size_arg]
        fc = [nn.Linear(size[0], size[1]), nn.GELU() if act.lower() == 'gelu' else nn.ReLU()]
        if dropout != 0.:
            fc.append(nn.Dropout(dropout))
        if rrt is not None:
            fc.append(rrt)
        n_br = n_classes if self._per_branch else 1
        net = (Attn_Net_Gated if gate else Attn_Net)(L=size[1], D=size[2], dropout=dropout, n_classes=n_br)
        fc.append(net)
        self.attention_net = nn.Sequential(*fc)
        if self._per_branch:   # an independent linear layer predicts each class
            self.classifiers = nn.ModuleList([nn.Linear(size[1], 1) for _ in range(n_classes)])
        else:
            self.classifiers = nn.Linear(size[1], n_classes)
        self.instance_classifiers = nn.ModuleList([nn.Linear(size[1], 2) for _ in range(n_classes)])
        self.k_sample = k_sample
        self.instance_loss_fn = SmoothTop1SVM(2)       # (the reference ignores its instance_loss_fn argument too)
        self.n_classes = n_classes
        self.subtyping = subtyping
        initialize_weights(self)
        self._emb_act = _lib.ACT_GELU if act.lower() == 'gelu' else _lib.ACT_RELU
        self._gate, self._hidden, self._has_dropout = bool(gate), size[2], dropout != 0.
        self._ws = None
        self.last_features = None

    _TRANSIENT = HeadState._TRANSIENT + ("last_features", "_cls_pack")
    _RESET = HeadState._RESET + ("last_features",)

    def relocate(self):
        return self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    # ------------------------------------------------------------------ pieces
    @property
    def rrt(self):
        return next((m for m in self.attention_net if isinstance(m, RRTEncoder)), None)

    def _net(self):
        return self.attention_net[-1]

    def _gate_linears(self):
        net = self._net()
        if self._gate:
            return net.attention_a, net.attention_b, net.attention_c
        mods = list(net.module)
        return mods[:-1], None, mods[-1]

    def _compute(self):
        return head_compute(self.rrt)

    def _cls_packed(self):
        """bag classifier rows as [n_classes, 512] + [n_classes] (CLAM_MB: its n_classes Linear(512, 1) packed)"""
        if not self._per_branch:
            return self.classifiers.weight, self.classifiers.bias
        key = tuple((m.weight.data_ptr(), m.weight._version, m.bias.data_ptr(), m.bias._version) for m in self.classifiers)
        hit = self.__dict__.get("_cls_pack")
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, torch.cat([m.weight for m in self.classifiers], 0).contiguous(),
                       torch.cat([m.bias for m in self.classifiers], 0).contiguous())
            self.__dict__["_cls_pack"] = hit
        return hit[1], hit[2]

    def _bag_logits(self, M):
        if not self._per_branch:
            return self.classifiers(M)
        return torch.cat([self.classifiers[c](M[c]) for c in range(self.n_classes)]).unsqueeze(0)

    def _stochastic(self):
        return self.training and (self._has_dropout or (self.rrt is not None and self.rrt._stochastic()))

    # ------------------------------------------------------------------ the one-call HIP path
    def _desc_weights(self, in_dim, solo):
        enc, p = self.rrt, RRTEncoder._ptr
        d, w = _lib.ClamDesc(), _lib.ClamWeights()
        if enc is not None:
            copy_encoder_desc(d.enc, enc, "CLAM")
            w.enc = enc._weights()
        d.enc.dim = 512
        d.enc.compute = self._compute()
        d.enc.solo = int(bool(solo))       # per-call scheduling hint, never inherited (see RRTMIL._mil_desc)
        d.input_dim, d.emb_act, d.has_rrt = in_dim, self._emb_act, int(enc is not None)
        d.n_classes, d.per_branch, d.gated, d.hidden, d.k_sample = (self.n_classes, int(self._per_branch), int(self._gate),
                                                                    self._hidden, self.k_sample)
        lin = self.attention_net[0]
        w.emb_w, w.emb_b = p(lin.weight), p(lin.bias)
        a, b, c = self._gate_linears()
        w.a_w, w.a_b = p(a[0].weight), p(a[0].bias)
        if b is not None:
            w.b_w, w.b_b = p(b[0].weight), p(b[0].bias)
        w.c_w, w.c_b = p(c.weight), p(c.bias)
        cw, cb = self._cls_packed()
        w.cls_w, w.cls_b = p(cw), p(cb)
        return d, w, (cw, cb)

    def forward_bag(self, x2d, attention_only=False, return_features=False, return_attn=False, return_topk=False, solo=True):
        """One bag, eval, no graph: x2d (N, input_dim) fp32 device tensor -> logits (1, n_classes) through ONE
        rrt_clam_forward_f32 call.  ``attention_only``: A_raw (K, N) instead.  With any of ``return_features`` /
        ``return_attn`` / ``return_topk`` a dict {logits, features (K, 512), attn (K, N), topk (K, 2, k_sample)} of what was
        asked for.  ``solo``: the slide has the GPU to itself (forward_bags passes False with several slides in flight)."""
        if not x2d.is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.CLAM runs on MI355X only: move the bag to a 'cuda' (HIP) device; there is "
                                   "no CPU fallback")
        if self._stochastic():
            raise NotImplementedError("forward_bag is the one-call inference entry (no dropout inside); in train() call the "
                                      "module itself")
        n, in_dim = x2d.shape
        if in_dim != self.attention_net[0].in_features:
            raise ValueError(f"expected feature dim {self.attention_net[0].in_features}, got {in_dim}")
        x2d = x2d.float().contiguous()
        d, w, _keep = self._desc_weights(in_dim, solo)
        dev = x2d.device
        K = self.n_classes if self._per_branch else 1
        new = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)   # noqa: E731
        logits = new(1, self.n_classes)
        a_raw = new(K, n) if attention_only else None
        attn = new(K, n) if return_attn else None
        feat = new(K, 512) if return_features else None
        topk = new(K, 2, self.k_sample, dt=torch.int64) if return_topk else None
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        self._head_forward("clam", d, w, x2d, (logits.data_ptr(), p(a_raw), p(attn), p(feat), p(topk)),
                           d.enc.compute != _lib.COMPUTE_F32 and d.has_rrt)
        if feat is not None:
            self.last_features = feat
        if attention_only:
            return a_raw
        if return_features or return_attn or return_topk:
            return {k: v for k, v in (("logits", logits), ("features", feat), ("attn", attn), ("topk", topk)) if v is not None}
        return logits

    @torch.no_grad()
    def forward_bags(self, bags, streams=4, **kw):
        """A batch of independent slides (each (N_i, input_dim) or (1, N_i, input_dim)) -> list of forward_bag results, with
        ``streams`` slides in flight on the heads' bag scheduler (HeadState._schedule_bags: one rrt_clam_forward_f32 call
        per slide with its own workspace; the call blocks the host; one call at a time per module)."""
        if not bags:
            return []
        if not bags[0].is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.CLAM runs on MI355X only; there is no CPU fallback")
        if self._stochastic():
            raise NotImplementedError("forward_bags is an inference entry; in train() call the module itself")
        return self._schedule_bags(bags, streams, lambda x2, solo: self.forward_bag(x2, solo=solo, **kw),
                                   lambda o: o.values() if isinstance(o, dict) else (o,))

    # ------------------------------------------------------------------ the layer path (graph, dropout, eager comparison)
    def _embed_encode(self, h2d):
        """attention_net up to the attention network: Linear + act (+ Dropout) (+ encoder) -> (N, 512)"""
        compute = self._compute()
        compute = _lib.COMPUTE_F32 if compute == _lib.COMPUTE_F32X3 else compute
        mods = list(self.attention_net)[:-1]
        x = lib_linear(mods[0], h2d, compute).float()
        for m in mods[1:]:
            x = m(x)
        return x

    def _attend(self, y):
        """y (N, 512) -> (M (K, 512), A (K, N) no grad, A_raw (K, N)): gate Linears on the library GEMMs, pooling in HIP"""
        compute = self._compute()
        compute = _lib.COMPUTE_F32 if compute == _lib.COMPUTE_F32X3 else compute
        a, b, c = self._gate_linears()

        def seq(mods, t):
            t = lib_linear(mods[0], t, compute).float()
            for m in list(mods)[1:]:
                t = m(t)
            return t
        ha = seq(a, y)
        hb = seq(b, y) if b is not None else None
        return _BranchPool.apply(y, ha, hb, c.weight, c.bias)

    def _eager_head(self, y):
        """The reference's op sequence for the head on torch ops (what a user of the encoder alone runs behind it; the
        benchmark's and the tests' comparison base, not used by forward): y (N, 512) -> (logits, M, A, A_raw)"""
        A, _ = self._net()(y)
        A_raw = A.transpose(1, 0)
        A = F.softmax(A_raw, dim=1)
        M = torch.mm(A, y)
        return self._bag_logits(M), M, A, A_raw

    def inst_eval(self, ids, h, classifier):
        """in-the-class branch (clam.py:137-154): ids (2, k_sample) = the top and bottom instances of the branch"""
        k = self.k_sample
        inst = torch.index_select(h, 0, ids.reshape(-1))
        targets = torch.cat([torch.ones(k, dtype=torch.int64, device=h.device), torch.zeros(k, dtype=torch.int64, device=h.device)])
        logits = classifier(inst)
        return self.instance_loss_fn(logits, targets), logits.argmax(1), targets

    def inst_eval_out(self, ids, h, classifier):
        """out-of-the-class branch (clam.py:157-167): the top instances are negatives"""
        inst = torch.index_select(h, 0, ids[0])
        targets = torch.zeros(self.k_sample, dtype=torch.int64, device=h.device)
        logits = classifier(inst)
        return self.instance_loss_fn(logits, targets), logits.argmax(1), targets

    def forward(self, h, label=None, instance_eval=True, return_features=False, attention_only=False):
        if not h.is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.CLAM runs on MI355X only: move the bag to a 'cuda' (HIP) device; there is "
                                   "no CPU fallback")
        ps = h.size(1) if h.dim() == 3 else h.size(0)
        h2d = h.reshape(-1, h.shape[-1])
        inst = instance_eval and label is not None
        graph = torch.is_grad_enabled() and (h.requires_grad or any(p.requires_grad for p in self.parameters()))
        if not graph and not self._stochastic() and not inst:
            out = self.forward_bag(h2d, attention_only=attention_only, return_features=return_features)
            return out["logits"] if isinstance(out, dict) else out
        with torch.set_grad_enabled(graph):
            y = self._embed_encode(h2d)
            M, A, A_raw = self._attend(y)
            if attention_only:
                return A_raw
            total_inst_loss = 0.0
            self.inst_preds, self.inst_targets = [], []
            if inst:
                ids = topk_rows(A, self.k_sample)
                onehot = F.one_hot(label.reshape(-1)[:1], num_classes=self.n_classes).reshape(-1).tolist()
                for i, classifier in enumerate(self.instance_classifiers):
                    br = ids[i if self._per_branch else 0]
                    if onehot[i] == 1:
                        loss, preds, targets = self.inst_eval(br, y, classifier)
                    elif self.subtyping:
                        loss, preds, targets = self.inst_eval_out(br, y, classifier)
                    else:
                        continue
                    self.inst_preds.append(preds)
                    self.inst_targets.append(targets)
                    total_inst_loss = total_inst_loss + loss
                if self.subtyping:
                    total_inst_loss = total_inst_loss / len(self.instance_classifiers)
            logits = self._bag_logits(M)
            if return_features:
                self.last_features = M
        return (logits, total_inst_loss, ps) if inst else logits


class CLAM_MB(CLAM_SB):
    """modules/clam.py:220-311: one attention branch and one bag classifier per class."""
    _per_branch = True

    def __init__(self, input_dim, gate=True, size_arg="small", dropout=0., k_sample=8, n_classes=2,
                 instance_loss_fn=None, subtyping=False, act='relu', rrt=None):
        nn.Module.__init__(self)
        self._build(input_dim, gate, size_arg, dropout, k_sample, n_classes, subtyping, act, rrt,
                    {"small": [input_dim, 512, 256], "big": [input_dim, 512, 384]})
