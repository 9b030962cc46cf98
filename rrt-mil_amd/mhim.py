"""MHIM-MIL -- the reference's ``Survival/main.py --model MHIM-MIL`` (Survival/models/MHIM/network.py) with its ABMIL baseline:
a gated-ABMIL student, its momentum teacher, and attention-driven masking of instances.

Same class names, constructor signatures and parameter names as the reference, so its checkpoints load with ``strict=True``
and ours load there.  ``MHIM`` is a ``BagHead`` (front = ``patch_to_emb[0]`` + activation + ``dp``, pool = gated attention,
classifier = ``predictor``): in ``eval()`` without a graph a bag is ONE C-ABI call (rrt_bagmil_forward_f32: ``forward_test``,
``pure``, ``forward_bag`` / ``forward_bags``); in ``train()`` or with a graph the Linears run on the library GEMMs and the
pooling is ``_AttnPool``.

The masking (``get_mask``) is ONE rrt_mask_select_f32 call (csrc/mask_select.hip): where the reference ranks all N scores with
``torch.topk(k=N)``, pulls the index lists to the host, does ``set`` arithmetic on them and uploads the result, the sizes of
the stages are computed here on the host in the reference's float arithmetic and the sets are formed on the device.  The
student then gathers the kept rows of the INPUT features (rrt_gather_rows_f32) and embeds only those.

What differs from the reference, on purpose:
  * ``mask_ids[:, :len_keep]`` are ascending, and so is the rest; the reference's order inside each part is that of a Python
    set.  The pooled row is a softmax-weighted sum over the kept rows: their order does not enter it.
  * equal scores go to the lower index; ``torch.topk`` leaves the order of ties unspecified.
  * dropout is drawn on the kept rows only (the reference draws it on all N rows, then gathers): the same distribution, other
    random numbers.
Out of scope here (NotImplementedError at construction): ``mlp_dim != 512``, and ``baseline='selfattn'``, which is the
sibling module ``rrt_mil_amd.mhim_sattn``.
"""
import ctypes as C
import warnings
from copy import deepcopy

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._head import BagHead
from .attmil import attn_tail, initialize_weights
from .mil import lib_attn_pool, lib_linear

_NO_SELFATTN = ("rrt_mil_amd.mhim.MHIM covers baseline='attn' (the gated-ABMIL baseline of Survival/main.py); baseline='selfattn' "
                "-- the TransMIL-style baseline, whose per-head attention rows (a 3-D attn) are fused by vote -- is not "
                "implemented in this module: it is rrt_mil_amd.mhim_sattn (the same class names)")


def cosine_scheduler(base_value, final_value, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0):
    """One value per iteration: a linear warm-up from ``start_warmup_value`` to ``base_value`` over ``warmup_epochs``, then half
    a cosine from ``base_value`` down (or up) to ``final_value`` -- numpy float64, value for value the reference's schedule."""
    total, warm = epochs * niter_per_ep, warmup_epochs * niter_per_ep
    ramp = np.linspace(start_warmup_value, base_value, warm) if warmup_epochs > 0 else np.array([])
    t = np.arange(total - warm)
    wave = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * t / len(t)))
    out = np.concatenate((ramp, wave))
    assert len(out) == total
    return out


@torch.no_grad()
def ema_update(model, targ_model, mm=0.9999):
    """targ <- mm * targ + (1 - mm) * model over the two modules' parameters, in place (two fused multi-tensor ops)"""
    if not 0.0 <= mm <= 1.0:
        raise AssertionError("Momentum needs to be between 0.0 and 1.0, got %.5f" % mm)
    q, k = [p.data for p in model.parameters()], [p.data for p in targ_model.parameters()]
    if k:
        torch._foreach_mul_(k, float(mm))
        torch._foreach_add_(k, q, alpha=1. - float(mm))


class SoftTargetCrossEntropy_v2(nn.Module):
    """cross-entropy of softmax(x / temp_s) against the soft target softmax(target / temp_t), over the last axis"""

    def __init__(self, temp_t=1., temp_s=1.):
        super().__init__()
        self.temp_t, self.temp_s = temp_t, temp_s

    def forward(self, x, target, mean=True):
        loss = -(F.softmax(target / self.temp_t, dim=-1) * F.log_softmax(x / self.temp_s, dim=-1)).sum(dim=-1)
        return loss.mean() if mean else loss


def _need_hip(t, who):
    if not t.is_cuda:
        raise _lib.RRTHipError(f"rrt_mil_amd.{who} runs on MI355X only: move the tensors to a 'cuda' (HIP) device; there is no "
                               "CPU fallback")


def gather_rows(x2d, ids, n_rows):
    """x2d (N, dim) fp32, ids (>= n_rows,) int64 device -> (n_rows, dim) = x2d[ids[:n_rows]] through rrt_gather_rows_f32 (an id
    outside [0, N) gives a NaN row); no graph -- `_GatherRows` is the autograd form"""
    _need_hip(x2d, "mhim.gather_rows")
    x2d, ids = x2d.detach().float().contiguous(), ids.contiguous()
    out = torch.empty((n_rows, x2d.shape[1]), dtype=torch.float32, device=x2d.device)
    with torch.cuda.device(x2d.device):
        st = torch.cuda.current_stream(x2d.device).cuda_stream
        _lib.check(_lib.load().rrt_gather_rows_f32(x2d.data_ptr(), ids.data_ptr(), out.data_ptr(), n_rows, x2d.shape[0],
                                                   x2d.shape[1], st), "rrt_gather_rows_f32")
    return out


def scatter_rows(rows, ids, n_dst):
    """the adjoint: (n_dst, dim) zeros with rows[r] at ids[r] (distinct ids) through rrt_scatter_rows_f32"""
    _need_hip(rows, "mhim.scatter_rows")
    rows, ids = rows.detach().float().contiguous(), ids.contiguous()
    out = torch.empty((n_dst, rows.shape[1]), dtype=torch.float32, device=rows.device)
    with torch.cuda.device(rows.device):
        st = torch.cuda.current_stream(rows.device).cuda_stream
        _lib.check(_lib.load().rrt_scatter_rows_f32(rows.data_ptr(), ids.data_ptr(), out.data_ptr(), rows.shape[0], n_dst,
                                                    rows.shape[1], st), "rrt_scatter_rows_f32")
    return out


class _GatherRows(torch.autograd.Function):
    """x2d[ids[:n_rows]] with rrt_scatter_rows_f32 as its backward (used only when the bag itself requires a gradient)"""

    @staticmethod
    def forward(ctx, x2d, ids, n_rows):
        ctx.save_for_backward(ids)
        ctx.n_src = x2d.shape[0]
        return gather_rows(x2d, ids, n_rows)

    @staticmethod
    def backward(ctx, d_rows):
        (ids,) = ctx.saved_tensors
        return scatter_rows(d_rows, ids, ctx.n_src), None, None


def mask_select(a, stages, invert=False, return_mask=False):
    """rrt_mask_select_f32 on the scores ``a`` (n,) fp32 device tensor: ``stages`` = [(largest, k, pick)] with pick a uint8 device
    tensor [k] or None -> (ids (n,) int64, count (1,) int64[, mask (n,) uint8]), all on the device (nothing visits the host)."""
    _need_hip(a, "mhim.mask_select")
    a = a.detach().float().contiguous()
    n, dev = a.numel(), a.device
    arr = (_lib.MaskStage * len(stages))()
    keep = []
    for s, (largest, k, pick) in zip(arr, stages):
        s.largest, s.k = int(bool(largest)), int(k)
        if pick is not None:
            pick = pick.to(torch.uint8).contiguous()
            keep.append(pick)
            s.pick = pick.data_ptr()
    lib = _lib.load()
    need = C.c_size_t()
    _lib.check(lib.rrt_mask_select_workspace_size(n, len(stages), C.byref(need)), "rrt_mask_select_workspace_size")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev) if return_mask else None
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.rrt_mask_select_f32(a.data_ptr(), n, arr, len(stages), int(bool(invert)), ids.data_ptr(), count.data_ptr(),
                                           mask.data_ptr() if return_mask else None, ws.data_ptr(), ws.numel(), st),
                   "rrt_mask_select_f32")
    return (ids, count, mask) if return_mask else (ids, count)


class AttentionGated(nn.Module):
    """The MHIM file's gated attention pool (network.py:35-78): Linear(L, 128) + act, Linear(L, 128) + sigmoid, their product
    through Linear(128, 1), softmax over the bag, weighted sum.  ``forward(x (1, N, L))`` -> (pooled (1, 1, L), A (1, 1, N));
    with ``no_norm`` A holds the raw scores."""

    def __init__(self, input_dim=512, act='relu', bias=False, dropout=False):
        super().__init__()
        self.L, self.D, self.K = input_dim, 128, 1
        a = [nn.Linear(self.L, self.D, bias=bias)]
        if act in ('gelu', 'relu', 'tanh'):
            a += [{'gelu': nn.GELU, 'relu': nn.ReLU, 'tanh': nn.Tanh}[act]()]
        b = [nn.Linear(self.L, self.D, bias=bias), nn.Sigmoid()]
        if dropout:
            a += [nn.Dropout(0.25)]
            b += [nn.Dropout(0.25)]
        self.attention_a = nn.Sequential(*a)
        self.attention_b = nn.Sequential(*b)
        self.attention_c = nn.Linear(self.D, self.K, bias=bias)

    def forward(self, x, no_norm=False):
        _need_hip(x, "mhim.AttentionGated")
        if x.dim() == 2:
            x = x.unsqueeze(0)

        def seq(mods):
            t = lib_linear(mods[0], x, _lib.COMPUTE_F32).float()
            for m in list(mods)[1:]:
                t = m(t)
            return t
        out = lib_attn_pool(x.float(), seq(self.attention_a), seq(self.attention_b), self.attention_c)
        if out is None:
            raise NotImplementedError("mhim.AttentionGated: one fp32 bag (1, N, L) with L % 32 == 0")
        pooled, a, a_raw = out
        return pooled.unsqueeze(1), (a_raw if no_norm else a).unsqueeze(1)


class DAttention(nn.Module):
    """network.py:81-122: the (always gated) pool with the student's masking in front of it."""

    def __init__(self, input_dim=512, act='relu', gated=True, bias=False, dropout=False):
        super().__init__()
        self.gated = gated
        if gated:
            self.attention = AttentionGated(input_dim, act, bias, dropout)

    def masking(self, x, ids_shuffle=None, len_keep=None):
        """x (1, N, D), ids_shuffle (1, N) a permutation whose first len_keep entries are kept -> (the kept rows (1, len_keep, D),
        mask (1, N) = 1 where removed, ids_restore (1, N))"""
        assert ids_shuffle is not None
        _need_hip(x, "mhim.DAttention")
        if x.shape[0] != 1:
            raise NotImplementedError("mhim.DAttention.masking: one bag per call")
        ids = ids_shuffle[0].contiguous()
        rows = _GatherRows.apply(x[0], ids, len_keep) if x.requires_grad else gather_rows(x[0], ids, len_keep)
        ids_restore = torch.empty_like(ids)
        ids_restore[ids] = torch.arange(ids.numel(), device=ids.device)
        return rows.unsqueeze(0), (ids_restore >= len_keep).to(torch.float32).unsqueeze(0), ids_restore.unsqueeze(0)

    def forward(self, x, mask_ids=None, len_keep=None, return_attn=False, no_norm=False, mask_enable=False):
        if mask_enable and mask_ids is not None:
            x, _, _ = self.masking(x, mask_ids, len_keep)
        x, attn = self.attention(x, no_norm)
        return (x.squeeze(1), attn.squeeze(1)) if return_attn else x.squeeze(1)


def _stage_sizes(ps, ratio, random_ratio):
    """One stage's sizes in the reference's float arithmetic (network.py:480-518) -> (k candidates, m of them drawn at random, or
    None = all of them).  The candidates' share of the bag is ratio / (random_ratio + 1e-8); when that exceeds 1 the whole bag is
    the candidate list and ``ratio`` itself becomes the share drawn from it."""
    share = ratio / (random_ratio + 1e-8)
    draw = random_ratio
    if share > 1:
        share, draw = 1., ratio
    k = int(np.ceil(ps * share))
    return k, (int(np.ceil(k * draw)) if draw < 1. else None)


class MHIM(BagHead, nn.Module):
    """network.py:438-659 with ``baseline='attn'``.

    ``forward(x, attn=None, teacher_cls_feat=None, i=None)`` -> (student_logit (1, C), cls_loss, ps, len_keep): the training
    step of the student on the instances that ``get_mask`` keeps."""
    _POOL = _lib.BAGPOOL_ATTN_GATED
    _NAME = "MHIM"

    def __init__(self, input_dim=1024, mlp_dim=512, mask_ratio=0, n_classes=2, temp_t=1., temp_s=1., dropout=0.25, act='relu',
                 select_mask=True, select_inv=False, msa_fusion='vote', mask_ratio_h=0., mrh_sche=None, mask_ratio_hr=0.,
                 mask_ratio_l=0., da_act='relu', baseline='selfattn', head=2, attn_layer=0):
        super().__init__()
        if baseline != 'attn':
            raise NotImplementedError(_NO_SELFATTN)
        if mlp_dim != 512:
            raise NotImplementedError(f"rrt_mil_amd.MHIM: mlp_dim must be 512, the heads' embedding width (got {mlp_dim})")
        self.mask_ratio, self.mask_ratio_h, self.mask_ratio_hr, self.mask_ratio_l = mask_ratio, mask_ratio_h, mask_ratio_hr, mask_ratio_l
        self.select_mask, self.select_inv, self.msa_fusion = select_mask, select_inv, msa_fusion
        self.mrh_sche, self.attn_layer = mrh_sche, attn_layer
        emb = [nn.Linear(input_dim, mlp_dim)]
        if act.lower() in ('relu', 'gelu'):
            emb += [nn.ReLU() if act.lower() == 'relu' else nn.GELU()]
        self.dp = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.patch_to_emb = nn.Sequential(*emb)
        self.online_encoder = DAttention(mlp_dim, da_act)
        self.predictor = nn.Linear(mlp_dim, n_classes)
        self.temp_t, self.temp_s = temp_t, temp_s
        self.cl_loss = SoftTargetCrossEntropy_v2(self.temp_t, self.temp_s)
        self.predictor_cl = nn.Identity()
        self.target_predictor = nn.Identity()
        self.apply(initialize_weights)
        self._emb_act = _lib.ACT_BY_NAME.get(act.lower(), _lib.ACT_NONE) if act.lower() in ('relu', 'gelu') else _lib.ACT_NONE
        self._pool_act = _lib.ACT_BY_NAME.get(da_act, _lib.ACT_NONE)
        self._ws = None

    # ------------------------------------------------------------------ BagHead
    def _front(self):
        return list(self.patch_to_emb) + [self.dp]

    def _classifier(self):
        return self.predictor

    def _fill(self, d, w, p):
        att = self.online_encoder.attention
        a, b, c = att.attention_a[0], att.attention_b[0], att.attention_c
        d.pool_hidden, d.pool_act = att.D, self._pool_act
        w.a_w, w.a_b, w.b_w, w.b_b, w.c_w, w.c_b = p(a.weight), p(a.bias), p(b.weight), p(b.bias), p(c.weight), p(c.bias)

    def _pool(self, y, compute):
        """y (n, 512) -> (pooled (512,), attn (n,), raw (n,)) on the layer path"""
        att = self.online_encoder.attention
        return attn_tail(self, y, att.attention_a, att.attention_b, att.attention_c, compute)

    def _tail(self, y, no_norm, compute):
        pooled, attn, a_raw = self._pool(y, compute)
        return self.predictor(pooled.unsqueeze(0)), (a_raw if no_norm else attn)

    def _bag2d(self, x):
        if x.dim() == 3 and x.shape[0] != 1:
            raise ValueError(f"{self._NAME} takes one bag per call, got a batch of {x.shape[0]}")
        x2d = x.reshape(-1, x.shape[-1])
        self._check_bag(x2d)
        return x2d

    # ------------------------------------------------------------------ masking
    def _randperm(self, k, device):
        """the permutation a stage draws its share of the k candidates with (tests override it with recorded ones)"""
        return torch.randperm(k, device=device)

    def _stage(self, ps, largest, mask_ratio, random_ratio, device):
        k, m = _stage_sizes(ps, mask_ratio, random_ratio)
        if m is None:
            return (largest, k, None)
        perm = self._randperm(k, device)
        pick = torch.zeros(k, dtype=torch.uint8, device=device)
        pick.index_fill_(0, perm[:m], 1)                        # pick[perm[:m]] = 1 without the host-to-device copy of the 1
        return (largest, k, pick)

    def _scores(self, ps, attn):
        if attn.dim() > 2:
            raise NotImplementedError(_NO_SELFATTN)
        if attn.numel() != ps:
            raise ValueError(f"attn holds {attn.numel()} scores for a bag of {ps} instances")
        _need_hip(attn, self._NAME)
        return attn.reshape(-1)

    def _select(self, ps, attn, stages, select_inv):
        """ONE rrt_mask_select_f32 call; reading the kept count back is the step's only host visit"""
        ids, count = mask_select(attn, stages, invert=select_inv)
        return int(count.item()), ids.unsqueeze(0)

    def select_mask_fn(self, ps, attn, largest, mask_ratio, mask_ids_other=None, len_keep_other=None,
                       cls_attn_topk_idx_other=None, random_ratio=1., select_inv=False):
        """One stage on its own -> (len_keep, mask_ids (1, N) int64).  ``get_mask`` does not chain calls of this method as the
        reference does: it hands all its stages to one device call, so an earlier stage's result (``mask_ids_other`` /
        ``cls_attn_topk_idx_other``) is not accepted here."""
        if mask_ids_other is not None or cls_attn_topk_idx_other is not None:
            raise NotImplementedError("rrt_mil_amd.MHIM.select_mask_fn selects one stage; the union over stages is formed inside "
                                      "get_mask's single rrt_mask_select_f32 call")
        if attn is None:
            raise ValueError("select_mask_fn needs the teacher's attention scores (attn is None)")
        a = self._scores(ps, attn)
        return self._select(ps, a, [self._stage(ps, largest, mask_ratio, random_ratio, a.device)], select_inv)

    def get_mask(self, ps, i, attn, mrh=None):
        """-> (len_keep, mask_ids (1, N) int64) like the reference (network.py:537-575): ``mask_ids[:, :len_keep]`` are the
        instances the student keeps (ascending), the rest follow (ascending); (ps, None) when no stage is active.

        The stages -- random (``mask_ratio``, drawn with random_ratio 0.001), low attention (``mask_ratio_l``), high attention
        (``mrh_sche[i]`` / ``mask_ratio_h`` / ``mrh``, drawn with ``mask_ratio_hr``) -- get their sizes here, on the host, in
        the reference's float arithmetic; their sets, the union and the complement come from ONE rrt_mask_select_f32 call.  The
        read-back of the kept count (``len_keep``, which sizes the student's tensors) is the only host visit of a training
        step."""
        if attn is not None and isinstance(attn, (list, tuple)):
            attn = attn[1] if self.attn_layer == -1 else attn[self.attn_layer]
        mask_ratio_h = self.mask_ratio_h
        if self.mrh_sche is not None:
            mask_ratio_h = self.mrh_sche[i]
        if mrh is not None:
            mask_ratio_h = mrh
        want = []                                               # (largest, ratio, random_ratio) in the reference's order
        if attn is not None and self.mask_ratio > 0.:
            want.append((False, self.mask_ratio, 0.001))
        if attn is not None and self.mask_ratio_l > 0.:
            want.append((False, self.mask_ratio_l, 1.))
        if mask_ratio_h > 0.:
            if attn is None:
                raise ValueError("the high-attention stage (mask_ratio_h > 0) needs the teacher's attention scores, attn is None")
            want.append((True, mask_ratio_h, self.mask_ratio_hr))
        if not want:
            return ps, None
        a = self._scores(ps, attn)
        stages = [self._stage(ps, largest, ratio, rr, a.device) for largest, ratio, rr in want]
        return self._select(ps, a, stages, self.select_inv)

    # ------------------------------------------------------------------ forwards
    @torch.no_grad()
    def forward_teacher(self, x, return_attn=False):
        """-> (pooled (1, 512), attn (1, N) or None); in train() the teacher's dropout is on, as in the reference"""
        x2d = self._bag2d(x)
        compute = self._gemm_compute()
        y = self._embed_encode(x2d)
        with torch.autocast("cuda", enabled=False):
            pooled, attn, _ = self._pool(y.float(), compute)
        return pooled.unsqueeze(0), (attn.unsqueeze(0) if return_attn else None)

    @torch.no_grad()
    def forward_test(self, x, return_attn=False, no_norm=False):
        """-> logits (1, C) [, attention (1, N): the raw scores with ``no_norm``]; in eval() one rrt_bagmil_forward_f32 call"""
        logits, a = self._run(x, return_attn=return_attn, no_norm=no_norm)
        return (logits, a.reshape(1, -1)) if return_attn else logits

    def pure(self, x, return_attn=False):
        """the unmasked baseline: eval -> logits [, attn]; train -> (logits, 0, ps, ps[, attn])"""
        ps = self._bag2d(x).shape[0]
        logits, a = self._run(x, return_attn=return_attn)
        a = a.reshape(1, -1) if return_attn else None
        if self.training:
            return (logits, 0, ps, ps, a) if return_attn else (logits, 0, ps, ps)
        return (logits, a) if return_attn else logits

    def forward_loss(self, student_cls_feat, teacher_cls_feat):
        return self.cl_loss(student_cls_feat, teacher_cls_feat.detach()) if teacher_cls_feat is not None else 0.

    def forward(self, x, attn=None, teacher_cls_feat=None, i=None):
        x2d = self._bag2d(x)
        ps = x2d.shape[0]
        len_keep, mask_ids = self.get_mask(ps, i, attn) if self.select_mask else (ps, None)
        if mask_ids is not None:
            # the kept rows of the INPUT features: the embedding GEMM runs on len_keep rows, not on ps
            ids = mask_ids[0]
            x2d = _GatherRows.apply(x2d, ids, len_keep) if x2d.requires_grad else gather_rows(x2d, ids, len_keep)
        compute = self._gemm_compute()
        y = self._embed_encode(x2d)
        with torch.autocast("cuda", enabled=False):
            pooled, _, _ = self._pool(y.float(), compute)
            student_cls_feat = pooled.unsqueeze(0)
            student_logit = self.predictor(student_cls_feat)
            cls_loss = self.forward_loss(student_cls_feat=student_cls_feat, teacher_cls_feat=teacher_cls_feat)
        return student_logit, cls_loss, ps, len_keep


class PURE_MHIM(nn.Module):
    """network.py:662-668: the unmasked baseline whose checkpoint initialises a teacher"""

    _MHIM = None     # the MHIM class to build (mhim_sattn's subclass names its own)

    def __init__(self, input_dim=1024, mlp_dim=512, n_classes=2, baseline='attn'):
        super().__init__()
        self.model = (self._MHIM or MHIM)(select_mask=False, input_dim=input_dim, mlp_dim=mlp_dim, n_classes=n_classes, baseline=baseline)

    def forward(self, x):
        return self.model.pure(x)


class MHIM_MIL(nn.Module):
    """network.py:671-722: student + momentum teacher.  ``model(x, i=step)`` in train() -> (logits (1, C), cls_loss);
    ``model(x)`` in eval() -> logits; ``update_teacher(step)`` after the optimiser step."""

    _MHIM = None     # as PURE_MHIM._MHIM

    def __init__(self, num_epoch, niter_per_ep, teacher_init=None, mm=0.9999, mm_sche=True, **kwargs):
        super().__init__()
        self.mm = mm
        kwargs['mrh_sche'] = cosine_scheduler(kwargs['mask_ratio_h'], 0., epochs=num_epoch, niter_per_ep=niter_per_ep)
        self.mm_sche = cosine_scheduler(self.mm, 1., epochs=num_epoch, niter_per_ep=niter_per_ep,
                                        start_warmup_value=1.) if mm_sche else None
        self.student = (self._MHIM or MHIM)(**kwargs)
        self.teacher = deepcopy(self.student)
        if teacher_init is not None:
            # a baseline checkpoint: the whole teacher, and the student's embedding (what loads, loads: strict=False, and a
            # checkpoint the teacher cannot take is reported, not fatal -- the reference's behaviour)
            try:
                self.teacher.load_state_dict(torch.load(teacher_init), strict=False)
            except Exception as e:      # noqa: BLE001
                warnings.warn(f"MHIM_MIL: teacher_init {teacher_init!r} did not load into the teacher: {e}")
            emb = {(k.replace('patch_to_emb.', '') if 'patch_to_emb' in k else k): v for k, v in torch.load(teacher_init).items()}
            self.student.patch_to_emb.load_state_dict(emb, strict=False)

    def update_teacher(self, index):
        """index = epoch * len(loader) + i"""
        ema_update(self.student, self.teacher, self.mm_sche[index] if self.mm_sche is not None else self.mm)

    def train_forward(self, x, i):
        cls_tea, attn = self.teacher.forward_teacher(x, return_attn=True)
        train_logits, cls_loss, _, _ = self.student(x, attn, cls_tea, i)
        return train_logits, cls_loss

    def forward(self, x, i=None):
        if self.training:
            return self.train_forward(x, i)
        return self.student.forward_test(x)
