"""MHIM-MIL with the TransMIL baseline -- the reference's Survival/models/MHIM/network.py with ``baseline='selfattn'`` (its own
default): a student and a momentum teacher that are both ``SAttention`` (a cls token, two Nystrom layers, PPEG between them),
and masking of instances driven by the teacher's per-head attention rows, fused by vote.

The sibling of ``rrt_mil_amd.mhim`` (``baseline='attn'``), with the reference's class names inside this module: ``SAttention``,
``TransLayer``, ``PPEG``, ``MHIM``, ``PURE_MHIM``, ``MHIM_MIL``.  Constructor signatures, defaults and parameter names are the
reference's, so its ``state_dict`` loads with ``strict=True`` and ours loads there.  ``baseline='attn'`` raises here and names
``rrt_mil_amd.mhim``.  The schedule, the EMA, the loss, the row gather and the stage arithmetic are ``mhim.py``'s, imported.

Where the work runs:
  * ``get_mask`` is ONE rrt_mask_select_vote_f32 call (csrc/mask_select.hip): every head's rank, the votes, the fused order, the
    union over the stages and the complement on the device; reading the kept count back is the training step's only host visit.
  * the attention is ``rrt_mil_amd.NystromAttention``: with a graph (the student) forward-with-stash and the HIP backward under
    autograd -- the layers' training path is enabled here, MHIM is a training model; under ``torch.no_grad()`` (the teacher,
    ``forward_test``) the inference call, with ``to_out``'s Dropout applied to its result in ``train()``.
  * the teacher's rows a1, a2 (1, heads, N) are the cls token's own row of each layer's Nystrom-approximated attention, without
    its own column (rrt_nystrom_attention_row_f32, row 0); they need ``torch.no_grad()``, not ``eval()``.
  * PPEG is rrt_peg_f32 / rrt_peg_backward_f32 (``_PPEGFn``); the kept rows move with rrt_gather_rows_f32 / rrt_scatter_rows_f32.
  * fp32 in every context: autocast is disabled inside, as in TransMIL.

What differs from the reference, on purpose:
  * kept-row order: the kept rows enter the sequence ascending; the reference's order is that of a Python ``set`` difference.
    Unlike with the ABMIL baseline the order changes the values here (Nystrom landmarks, PPEG's image); ascending keeps the
    bag's own order and is deterministic.
  * vote ties go to the lower index; ``torch.topk`` on the integer votes leaves them unspecified.
  * the attention row is the cls token's own; the reference reads row 0 of the front-padded sequence, a zero pad row whenever
    ``(N + 1) % 256 != 0`` (the two agree where ``(N + 1) % 256 == 0``).
  * dropout is drawn on the kept rows only (the student embeds only those).
  * ``forward_test(x, return_attn=True)`` returns ``(logits, [a1, a2])`` where the reference raises a TypeError.
Out of scope (NotImplementedError at construction): ``msa_fusion='mean'`` (its candidate set is a ``unique`` whose size is only
known on the device, a second host visit), ``pos_pos != 0``, ``pos != 'ppeg'``, ``mlp_dim != 512``, ``head`` outside 1..16.
The attention rows with a graph (``pure(x, return_attn=True)`` with gradients enabled) raise at the call.
"""
import ctypes as C

import torch
from torch import nn

from . import _lib
from . import mhim as _mhim
from .mhim import (SoftTargetCrossEntropy_v2, _GatherRows, _need_hip, _stage_sizes, cosine_scheduler, ema_update,  # noqa: F401
                   gather_rows)
from .mil import lib_linear
from .transmil import NystromAttention, _needs_graph

_NO_ATTN = ("rrt_mil_amd.mhim_sattn covers baseline='selfattn' (the TransMIL-style baseline, the reference's default); "
            "baseline='attn', the gated-ABMIL baseline, is rrt_mil_amd.mhim (the same class names)")


def initialize_weights(module):
    """network.py:10-18: xavier-normal Linear weights, zero biases, LayerNorm (1, 0); the convolutions keep torch's default"""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_normal_(m.weight)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)


def mask_select_vote(a, stages, invert=False, return_mask=False):
    """rrt_mask_select_vote_f32 on the per-head rows ``a`` (heads, n) fp32 device tensor: ``stages`` = [(largest, k, pick)] with
    pick a uint8 device tensor [k] or None -> (ids (n,) int64, count (1,) int64[, mask (n,) uint8]), all on the device
    (nothing visits the host).  Each head ranks its own row, a token's vote is the number of heads that hold it among their first
    k, and the stage's candidates are the first k by vote, equal votes to the lower index."""
    if a.dim() != 2:
        raise ValueError(f"mask_select_vote takes the rows as (heads, n), got {tuple(a.shape)}")
    _need_hip(a, "mhim_sattn.mask_select_vote")
    a = a.detach().float().contiguous()
    (heads, n), dev = a.shape, a.device
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
    _lib.check(lib.rrt_mask_select_vote_workspace_size(n, heads, len(stages), C.byref(need)), "rrt_mask_select_vote_workspace_size")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev) if return_mask else None
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.rrt_mask_select_vote_f32(a.data_ptr(), n, heads, arr, len(stages), int(bool(invert)), ids.data_ptr(),
                                                count.data_ptr(), mask.data_ptr() if return_mask else None, ws.data_ptr(),
                                                ws.numel(), st), "rrt_mask_select_vote_f32")
    return (ids, count, mask) if return_mask else (ids, count)


def _ptr3(ts):
    return (C.c_void_p * 3)(*[t.data_ptr() if t is not None else None for t in ts])


class _PPEGFn(torch.autograd.Function):
    """y [n, dim] = PPEG(x) -- x on its ceil(sqrt(n)) square (wrapped; a side below 7 lifted to 7 with zero rows), plus the three
    depth-wise convolutions: rrt_peg_f32 with ppeg = 1, and rrt_peg_backward_f32 (dx, the three dW, the three db)."""

    @staticmethod
    def forward(ctx, x, k, w0, w1, w2, b0, b1, b2):
        lib = _lib.load()
        ts = [t.detach().float().contiguous() for t in (x, w0, w1, w2, b0, b1, b2)]
        x, dev = ts[0], ts[0].device
        n, dim = x.shape
        y = torch.empty_like(x)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_peg_f32(x.data_ptr(), _ptr3(ts[1:4]), _ptr3(ts[4:7]), y.data_ptr(), n, dim, k, 0, 1, st), "rrt_peg_f32")
        ctx.save_for_backward(*ts)
        ctx.k = k
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, ws3 = ctx.saved_tensors[0], ctx.saved_tensors[1:4]
        (n, dim), dev, k = x.shape, x.device, ctx.k
        dy = dy.float().contiguous()
        dx = torch.empty_like(x)
        dws = [torch.empty_like(w) for w in ws3]
        dbs = [torch.empty(dim, dtype=torch.float32, device=dev) for _ in range(3)]
        need = C.c_size_t()
        _lib.check(lib.rrt_peg_backward_workspace_size(n, dim, k, 1, C.byref(need)), "rrt_peg_backward_workspace_size")
        ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_peg_backward_f32(x.data_ptr(), dy.data_ptr(), _ptr3(ws3), dx.data_ptr(), _ptr3(dws), _ptr3(dbs), n, dim, k,
                                                0, 1, ws.data_ptr(), need.value, st), "rrt_peg_backward_f32")
        grads = [dx, None] + dws + dbs
        return tuple(g if need_g else None for g, need_g in zip(grads, ctx.needs_input_grad))


class PPEG(nn.Module):
    """network.py:259-293.  ``forward(x (1, n, dim))`` -> (1, n, dim) through rrt_peg_f32.  The 2-D form with biases, which is
    what SAttention builds; k odd, at most 11."""

    def __init__(self, dim=512, k=7, conv_1d=False, bias=True):
        super().__init__()
        if conv_1d or not bias:
            raise NotImplementedError("rrt_mil_amd.mhim_sattn.PPEG: the 2-D convolutions with biases (conv_1d=False, bias=True), "
                                      "what SAttention builds")
        if k % 2 == 0 or not 1 <= k <= 11:
            raise NotImplementedError(f"rrt_mil_amd.mhim_sattn.PPEG: k must be odd and at most 11 (got {k})")
        self.proj = nn.Conv2d(dim, dim, k, 1, k // 2, groups=dim, bias=bias)
        self.proj1 = nn.Conv2d(dim, dim, 5, 1, 5 // 2, groups=dim, bias=bias)
        self.proj2 = nn.Conv2d(dim, dim, 3, 1, 3 // 2, groups=dim, bias=bias)
        self.k = k

    def forward(self, x):
        _need_hip(x, "mhim_sattn.PPEG")
        if x.dim() != 3 or x.shape[0] != 1:
            raise ValueError(f"PPEG expects one sequence (1, n, dim), got {tuple(x.shape)}")
        with torch.autocast("cuda", enabled=False):
            return self._rows(x[0].float()).unsqueeze(0)

    def _rows(self, x2d):
        return _PPEGFn.apply(x2d, self.k, self.proj.weight, self.proj1.weight, self.proj2.weight, self.proj.bias, self.proj1.bias,
                             self.proj2.bias)


class TransLayer(nn.Module):
    """network.py:296-317: x + attn(norm(x)), attn = NystromAttention(dim, dim // 8, heads=head, num_landmarks=dim // 2,
    pinv_iterations=6, residual=True, dropout=0.1) with its training path enabled.  ``forward(x (1, n, dim), need_attn=False)``
    -> x' [, attn (1, heads, n - 1): row 0 of the approximated attention matrix without column 0]."""

    def __init__(self, norm_layer=nn.LayerNorm, dim=512, head=8):
        super().__init__()
        self.norm = norm_layer(dim)
        self.attn = NystromAttention(dim=dim, dim_head=dim // 8, heads=head, num_landmarks=dim // 2, pinv_iterations=6,
                                     residual=True, dropout=0.1).enable_training()

    def forward(self, x, need_attn=False):
        _need_hip(x, "mhim_sattn.TransLayer")
        with torch.autocast("cuda", enabled=False):
            h, a = self._rows(x[0].float(), need_attn)
        return (h.unsqueeze(0), a) if need_attn else h.unsqueeze(0)

    def _rows(self, h, need_attn):
        """h (n, dim) fp32 -> (h + attn(norm(h)), the row (1, heads, n - 1) or None)"""
        z = self.norm(h).unsqueeze(0)
        attn, a = self.attn, None
        if need_attn:
            if _needs_graph(self, h):
                raise NotImplementedError("rrt_mil_amd.mhim_sattn: the attention rows are an inference output (no gradient flows "
                                          "through them): ask for them under torch.no_grad(), as forward_teacher and forward_test do")
            y, a = attn.attention_row(z, 0, in_train=True)
            y, a = attn.to_out[1](y), a[:, :, 1:]
        elif _needs_graph(self, h):
            y = attn(z)                                          # forward-with-stash + HIP backward; its Dropout inside
        else:
            y = attn.to_out[1](attn._forward_batched(z))         # the inference call; the Dropout is the identity in eval()
        return h + y[0], a


class SAttention(nn.Module):
    """network.py:320-408.  ``forward(x (1, N, 512), mask_ids=None, len_keep=None, return_attn=False, mask_enable=False)`` -> the
    cls row (1, 512) after the final LayerNorm [, [a1, a2], each (1, heads, N)]: the kept rows (``mask_ids[:, :len_keep]``, with
    ``mask_enable``), the cls token in front, layer 1, PPEG on rows 1.., layer 2, LayerNorm, row 0."""

    def __init__(self, mlp_dim=512, pos_pos=0, pos='ppeg', peg_k=7, head=8):
        super().__init__()
        if pos_pos != 0 or pos != 'ppeg':
            raise NotImplementedError(f"rrt_mil_amd.mhim_sattn.SAttention: pos_pos=0 and pos='ppeg', what MHIM builds "
                                      f"(got pos_pos={pos_pos!r}, pos={pos!r})")
        self.norm = nn.LayerNorm(mlp_dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, mlp_dim))
        self.layer1 = TransLayer(dim=mlp_dim, head=head)
        self.layer2 = TransLayer(dim=mlp_dim, head=head)
        self.pos_embedding = PPEG(dim=mlp_dim, k=peg_k)
        self.pos_pos = pos_pos

    def forward(self, x, mask_ids=None, len_keep=None, return_attn=False, mask_enable=False):
        _need_hip(x, "mhim_sattn.SAttention")
        if x.dim() == 3:
            if x.shape[0] != 1:
                raise ValueError(f"SAttention takes one bag per call, got a batch of {x.shape[0]}")
            x = x[0]
        if x.dim() != 2 or x.shape[1] != self.norm.normalized_shape[0] or x.shape[0] < 1:
            raise ValueError(f"SAttention expects (1, N, {self.norm.normalized_shape[0]}), got {tuple(x.shape)}")
        with torch.autocast("cuda", enabled=False):
            h = x.float()
            if mask_enable and mask_ids is not None:
                ids = mask_ids.reshape(-1).contiguous()
                h = _GatherRows.apply(h, ids, len_keep) if h.requires_grad else gather_rows(h, ids, len_keep)
            h = torch.cat([self.cls_token.reshape(1, -1).float(), h])
            h, a1 = self.layer1._rows(h, return_attn)
            h = torch.cat([h[:1], self.pos_embedding._rows(h[1:])])
            h, a2 = self.layer2._rows(h, return_attn)
            out = self.norm(h[:1])
        return (out, [a1, a2]) if return_attn else out


class MHIM(nn.Module):
    """network.py:438-659 with ``baseline='selfattn'``.

    ``forward(x, attn=None, teacher_cls_feat=None, i=None)`` -> (student_logit (1, C), cls_loss, ps, len_keep): the training
    step of the student on the instances that ``get_mask`` keeps; ``attn`` is the teacher's ``[a1, a2]`` (or one (1, heads, N)
    tensor)."""
    _NAME = "mhim_sattn.MHIM"

    def __init__(self, input_dim=1024, mlp_dim=512, mask_ratio=0, n_classes=2, temp_t=1., temp_s=1., dropout=0.25, act='relu',
                 select_mask=True, select_inv=False, msa_fusion='vote', mask_ratio_h=0., mrh_sche=None, mask_ratio_hr=0.,
                 mask_ratio_l=0., da_act='relu', baseline='selfattn', head=2, attn_layer=0):
        super().__init__()
        if baseline != 'selfattn':
            raise NotImplementedError(_NO_ATTN)
        if mlp_dim != 512:
            raise NotImplementedError(f"rrt_mil_amd.mhim_sattn.MHIM: mlp_dim must be 512 -- head dim 64 and 256 landmarks, what the "
                                      f"Nystrom kernels take (got {mlp_dim})")
        if not 1 <= head <= _lib.MASK_VOTE_MAX_HEADS:
            raise NotImplementedError(f"rrt_mil_amd.mhim_sattn.MHIM: head must be in 1..{_lib.MASK_VOTE_MAX_HEADS} (got {head})")
        if msa_fusion != 'vote':
            raise NotImplementedError(f"rrt_mil_amd.mhim_sattn.MHIM: msa_fusion='vote' only (got {msa_fusion!r}); 'mean' draws its "
                                      "random share from a unique() whose size is only known on the device, a second host visit")
        if attn_layer not in (-1, 0, 1):
            raise ValueError(f"attn_layer must be 0, 1 or -1 (got {attn_layer})")
        self.mask_ratio, self.mask_ratio_h, self.mask_ratio_hr, self.mask_ratio_l = mask_ratio, mask_ratio_h, mask_ratio_hr, mask_ratio_l
        self.select_mask, self.select_inv, self.msa_fusion = select_mask, select_inv, msa_fusion
        self.mrh_sche, self.attn_layer = mrh_sche, attn_layer
        emb = [nn.Linear(input_dim, mlp_dim)]
        if act.lower() in ('relu', 'gelu'):
            emb += [nn.ReLU() if act.lower() == 'relu' else nn.GELU()]
        self.dp = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.patch_to_emb = nn.Sequential(*emb)
        self.online_encoder = SAttention(mlp_dim=mlp_dim, head=head)
        self.predictor = nn.Linear(mlp_dim, n_classes)
        self.temp_t, self.temp_s = temp_t, temp_s
        self.cl_loss = SoftTargetCrossEntropy_v2(self.temp_t, self.temp_s)
        self.predictor_cl = nn.Identity()
        self.target_predictor = nn.Identity()
        self.apply(initialize_weights)
        self.head = head

    # ------------------------------------------------------------------ masking: mhim.MHIM's stage logic on the vote entry
    _randperm = _mhim.MHIM._randperm
    _stage = _mhim.MHIM._stage
    select_mask_fn = _mhim.MHIM.select_mask_fn
    get_mask = _mhim.MHIM.get_mask
    forward_loss = _mhim.MHIM.forward_loss

    def _scores(self, ps, attn):
        """the teacher's rows of one layer, (1, heads, ps) -> (heads, ps)"""
        if attn.dim() == 2:
            raise ValueError(f"rrt_mil_amd.mhim_sattn.MHIM takes the per-head attention rows, (1, heads, N); a 2-D attn "
                             f"{tuple(attn.shape)} is the ABMIL baseline's: rrt_mil_amd.mhim")
        if attn.dim() != 3 or attn.shape[0] != 1:
            raise ValueError(f"attn must be (1, heads, N), got {tuple(attn.shape)}")
        attn = attn[0]
        if attn.shape[0] != self.head or attn.shape[1] != ps:
            raise ValueError(f"attn holds {tuple(attn.shape)} scores for {self.head} heads and a bag of {ps} instances")
        _need_hip(attn, self._NAME)
        return attn

    def _select(self, ps, attn, stages, select_inv):
        """ONE rrt_mask_select_vote_f32 call; reading the kept count back is the step's only host visit"""
        ids, count = mask_select_vote(attn, stages, invert=select_inv)
        return int(count.item()), ids.unsqueeze(0)

    # ------------------------------------------------------------------ forwards
    def _bag2d(self, x):
        _need_hip(x, self._NAME)
        if x.dim() == 3 and x.shape[0] != 1:
            raise ValueError(f"{self._NAME} takes one bag per call, got a batch of {x.shape[0]}")
        x2d = x.reshape(-1, x.shape[-1])
        if x.dim() not in (2, 3) or x2d.shape[0] < 1 or x2d.shape[1] != self.patch_to_emb[0].in_features:
            raise ValueError(f"{self._NAME} expects (1, N, {self.patch_to_emb[0].in_features}), got {tuple(x.shape)}")
        return x2d

    def _embed(self, x2d):
        """patch_to_emb (the Linear on the library GEMM, fp32) and dp -> (n, 512)"""
        y = lib_linear(self.patch_to_emb[0], x2d.float(), _lib.COMPUTE_F32).float()
        for m in list(self.patch_to_emb)[1:]:
            y = m(y)
        return self.dp(y)

    @torch.no_grad()
    def forward_teacher(self, x, return_attn=False):
        """-> (the cls row (1, 512), [a1, a2] each (1, heads, N), or None); in train() the teacher's dropout is on, as in the
        reference -- the rows do not depend on their own layer's output dropout"""
        x2d = self._bag2d(x)
        with torch.autocast("cuda", enabled=False):
            out = self.online_encoder(self._embed(x2d), return_attn=return_attn)
        return out if return_attn else (out, None)

    @torch.no_grad()
    def forward_test(self, x, return_attn=False, no_norm=False):
        """-> logits (1, C) [, [a1, a2]]"""
        if no_norm:
            raise ValueError("rrt_mil_amd.mhim_sattn.MHIM.forward_test: no_norm belongs to the ABMIL baseline (rrt_mil_amd.mhim); "
                             "SAttention's rows have no softmax of their own to leave out")
        x2d = self._bag2d(x)
        with torch.autocast("cuda", enabled=False):
            out = self.online_encoder(self._embed(x2d), return_attn=return_attn)
            feat, a = out if return_attn else (out, None)
            logits = self.predictor(feat)
        return (logits, a) if return_attn else logits

    def forward_bag(self, x, return_attn=False):
        """one bag (N, input_dim) or (1, N, input_dim) -> forward_test's result"""
        return self.forward_test(x, return_attn=return_attn)

    def forward_bags(self, bags, return_attn=False):
        """a list of independent bags -> a list of forward_test's results: a plain loop on the caller's stream"""
        return [self.forward_test(b, return_attn=return_attn) for b in bags]

    def pure(self, x, return_attn=False):
        """the unmasked baseline: eval -> logits [, attn]; train -> (logits, 0, ps, ps[, attn])"""
        x2d = self._bag2d(x)
        ps = x2d.shape[0]
        with torch.autocast("cuda", enabled=False):
            out = self.online_encoder(self._embed(x2d), return_attn=return_attn)
            feat, a = out if return_attn else (out, None)
            logits = self.predictor(feat)
        if self.training:
            return (logits, 0, ps, ps, a) if return_attn else (logits, 0, ps, ps)
        return (logits, a) if return_attn else logits

    def forward(self, x, attn=None, teacher_cls_feat=None, i=None):
        x2d = self._bag2d(x)
        ps = x2d.shape[0]
        len_keep, mask_ids = self.get_mask(ps, i, attn) if self.select_mask else (ps, None)
        if mask_ids is not None:
            # the kept rows of the INPUT features, ascending: the embedding GEMM runs on len_keep rows, not on ps
            ids = mask_ids[0]
            x2d = _GatherRows.apply(x2d.float(), ids, len_keep) if x2d.requires_grad else gather_rows(x2d, ids, len_keep)
        with torch.autocast("cuda", enabled=False):
            student_cls_feat = self.online_encoder(self._embed(x2d))
            student_logit = self.predictor(student_cls_feat)
            cls_loss = self.forward_loss(student_cls_feat=student_cls_feat, teacher_cls_feat=teacher_cls_feat)
        return student_logit, cls_loss, ps, len_keep


class PURE_MHIM(_mhim.PURE_MHIM):
    """network.py:662-668: the unmasked baseline whose checkpoint initialises a teacher.  The reference's default here is
    ``baseline='attn'``, which this module refuses: pass ``baseline='selfattn'``."""
    _MHIM = MHIM


class MHIM_MIL(_mhim.MHIM_MIL):
    """network.py:671-722: student + momentum teacher.  ``model(x, i=step)`` in train() -> (logits (1, C), cls_loss);
    ``model(x)`` in eval() -> logits; ``update_teacher(step)`` after the optimiser step."""
    _MHIM = MHIM
