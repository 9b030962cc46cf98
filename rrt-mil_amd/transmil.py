"""TransMIL -- the transformer baseline of the reference (modules/transmil.py:26-125) and its hot path, Nystrom attention
(modules/nystrom_attention.py:32-149), on the MI355X kernels of csrc/nystrom.hip.

Same constructor signatures, module tree and parameter names as the reference (``_fc1.0``, ``cls_token``,
``layer{1,2}.norm``, ``layer{1,2}.attn.{to_qkv, to_out.0, res_conv}``, ``pos_layer.{proj, proj1, proj2}``, ``norm``,
``_fc2``): reference checkpoints load with ``strict=True``.

Inference is the default: a bag is ONE C-ABI call (rrt_transmil_forward_f32: ``forward_bag``), and a call that needs a graph,
or ``train()`` with dropout, raises ``NotImplementedError`` -- use ``eval()`` under ``torch.no_grad()``.

Training is opt-in: after ``model.enable_training()`` a call that needs a graph (or ``train()`` with dropout) takes the layer
path -- torch ops around ``NystromAttention``, whose forward-with-stash and backward are the HIP kernels of csrc/nystrom.hip and
csrc/nystrom_bwd.hip under a ``torch.autograd.Function``; a call that needs no graph still takes the one-call path, bit for bit.
``model.enable_training(one_call=True)`` takes the whole step into the library instead: ONE rrt_transmil_forward_train_f32 call
and ONE rrt_transmil_backward_f32 call (csrc/transmil_bwd.hip).
Attention maps are an inference output: ``TransMIL.forward_bag(x, return_attn=True)`` adds the class token's row of the
Nystrom-approximated attention matrix of both layers (rrt_transmil_forward_attn_f32, csrc/nystrom_row.hip), and
``NystromAttention.attention_row(x, row)`` any one row; with either, a call that needs a graph raises, opt-in or not.
The arithmetic is exact fp32 on the fp32 matrix cores in every context: under ``torch.autocast`` the modules STILL compute
in fp32 (there is no 16-bit path for the pseudo-inverse iteration, whose conditioning does not survive 8 mantissa bits).
"""
import ctypes as C

import torch
from torch import nn

from . import _lib
from ._head import HeadState


def initialize_weights(module):
    """modules/transmil.py:6-24"""
    for m in module.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.xavier_normal_(m.weight)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _param(t):
    """the parameter's own fp32 storage (no copy when it is already contiguous fp32)"""
    return t.detach().float().contiguous()


def _no_cpu(t, who):
    if not t.is_cuda:
        raise _lib.RRTHipError(f"rrt_mil_amd.{who} runs on MI355X only: move the input to a 'cuda' (HIP) device; there is no "
                               "CPU fallback")


def _needs_graph(module, x):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


def _no_graph(module, x, who):
    if _needs_graph(module, x):
        raise NotImplementedError(f"rrt_mil_amd.{who} has no backward by default: call it in eval() under torch.no_grad(), "
                                  "or opt in to the training path with enable_training()")


class _NystromFn(torch.autograd.Function):
    """y [n, dim] = NystromAttention without its Dropout, fp32: rrt_nystrom_attention_forward_train_f32 (the bits of
    rrt_nystrom_attention_f32; what the backward reads stays in a stash the graph owns) and
    rrt_nystrom_attention_backward_f32 (d x and the gradients of to_qkv.weight, to_out.0.weight, to_out.0.bias,
    res_conv.weight)."""

    @staticmethod
    def forward(ctx, desc, x2d, wq, wo, bo, wc):
        lib = _lib.load()
        ts = [t.detach().float().contiguous() if t is not None else None for t in (x2d, wq, wo, bo, wc)]
        x, dev = ts[0], ts[0].device
        n = x.shape[0]
        w = _lib.NystromWeights()
        w.qkv_w, w.out_w, w.out_b, w.conv_w = (_ptr(t) for t in ts[1:])
        stash_bytes, bwd_bytes = C.c_size_t(), C.c_size_t()
        _lib.check(lib.rrt_nystrom_train_sizes(C.byref(desc), n, C.byref(stash_bytes), C.byref(bwd_bytes)),
                   "rrt_nystrom_train_sizes")
        stash = torch.empty(stash_bytes.value, dtype=torch.uint8, device=dev)
        y = torch.empty((n, desc.dim), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_nystrom_attention_forward_train_f32(C.byref(desc), C.byref(w), x.data_ptr(), y.data_ptr(), n,
                                                                   stash.data_ptr(), stash.numel(), st),
                       "rrt_nystrom_attention_forward_train_f32")
        ctx.save_for_backward(stash, *[t for t in ts if t is not None])
        ctx.desc, ctx.bwd_bytes, ctx.has_conv = desc, bwd_bytes.value, ts[4] is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        stash, x, wq, wo, bo = ctx.saved_tensors[:5]
        wc = ctx.saved_tensors[5] if ctx.has_conv else None
        desc, dev, n = ctx.desc, x.device, x.shape[0]
        dy = dy.float().contiguous()
        w, g = _lib.NystromWeights(), _lib.NystromGrads()
        w.qkv_w, w.out_w, w.out_b, w.conv_w = (_ptr(t) for t in (wq, wo, bo, wc))
        grads = [torch.empty_like(t) if t is not None else None for t in (wq, wo, bo, wc)]
        g.qkv_w, g.out_w, g.out_b, g.conv_w = (_ptr(t) for t in grads)
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        ws = torch.empty(ctx.bwd_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_nystrom_attention_backward_f32(C.byref(desc), C.byref(w), x.data_ptr(), dy.data_ptr(),
                                                              stash.data_ptr(), stash.numel(), C.byref(g), _ptr(dx), n,
                                                              ws.data_ptr(), ws.numel(), st),
                       "rrt_nystrom_attention_backward_f32")
        return (None, dx) + tuple(gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[2:]))


class _NystromBatchedFn(torch.autograd.Function):
    """y [b, n, dim] = NystromAttention on a batch without its Dropout, fp32 -- ONE pseudo-inverse scale over all b * heads
    matrices, in the forward and in the gradient through it: rrt_nystrom_attention_batched_forward_train_f32 (the bits of
    rrt_nystrom_attention_batched_f32; the stash is owned by the graph node) and rrt_nystrom_attention_batched_backward_f32.
    As _NystromFn, the parameters are saved tensors: an in-place update between forward and backward raises."""

    @staticmethod
    def forward(ctx, desc, x3d, wq, wo, bo, wc):
        lib = _lib.load()
        ts = [t.detach().float().contiguous() if t is not None else None for t in (x3d, wq, wo, bo, wc)]
        x, dev = ts[0], ts[0].device
        b, n = x.shape[0], x.shape[1]
        w = _lib.NystromWeights()
        w.qkv_w, w.out_w, w.out_b, w.conv_w = (_ptr(t) for t in ts[1:])
        stash_bytes, bwd_bytes = C.c_size_t(), C.c_size_t()
        _lib.check(lib.rrt_nystrom_batched_train_sizes(C.byref(desc), b, n, C.byref(stash_bytes), C.byref(bwd_bytes)),
                   "rrt_nystrom_batched_train_sizes")
        stash = torch.empty(stash_bytes.value, dtype=torch.uint8, device=dev)
        y = torch.empty((b, n, desc.dim), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_nystrom_attention_batched_forward_train_f32(C.byref(desc), C.byref(w), x.data_ptr(), y.data_ptr(),
                                                                           b, n, stash.data_ptr(), stash.numel(), st),
                       "rrt_nystrom_attention_batched_forward_train_f32")
        ctx.save_for_backward(stash, *[t for t in ts if t is not None])
        ctx.desc, ctx.bwd_bytes, ctx.has_conv = desc, bwd_bytes.value, ts[4] is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        stash, x, wq, wo, bo = ctx.saved_tensors[:5]
        wc = ctx.saved_tensors[5] if ctx.has_conv else None
        desc, dev, b, n = ctx.desc, x.device, x.shape[0], x.shape[1]
        dy = dy.float().contiguous()
        w, g = _lib.NystromWeights(), _lib.NystromGrads()
        w.qkv_w, w.out_w, w.out_b, w.conv_w = (_ptr(t) for t in (wq, wo, bo, wc))
        grads = [torch.empty_like(t) if t is not None else None for t in (wq, wo, bo, wc)]
        g.qkv_w, g.out_w, g.out_b, g.conv_w = (_ptr(t) for t in grads)
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        ws = torch.empty(ctx.bwd_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_nystrom_attention_batched_backward_f32(C.byref(desc), C.byref(w), x.data_ptr(), dy.data_ptr(),
                                                                      stash.data_ptr(), stash.numel(), C.byref(g), _ptr(dx), b, n,
                                                                      ws.data_ptr(), ws.numel(), st),
                       "rrt_nystrom_attention_batched_backward_f32")
        return (None, dx) + tuple(gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[2:]))


class _TransmilStepFn(torch.autograd.Function):
    """logits (1, n_classes) = the whole of TransMIL for one bag through rrt_transmil_forward_train_f32, and every parameter
    gradient (and d x, when x needs one) through ONE rrt_transmil_backward_f32.  The parameters are passed as inputs so that
    autograd routes their gradients; the stash lives in a tensor owned by the graph node (retain_graph works); the dropout
    masks are regenerated in the backward from (p, seed)."""

    @staticmethod
    def forward(ctx, model, x2d, fc1_p, attn_p, seed, *params):
        lib = _lib.load()
        x = x2d.detach().float().contiguous()
        n, dev = x.shape[0], x.device
        keep = []
        d, w = model._desc_weights(keep)
        stash_b, ws_b = C.c_size_t(), C.c_size_t()
        _lib.check(lib.rrt_transmil_train_sizes(C.byref(d), n, C.byref(stash_b), C.byref(ws_b)), "rrt_transmil_train_sizes")
        stash = torch.empty(stash_b.value, dtype=torch.uint8, device=dev)
        logits = torch.empty((1, model.n_classes), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_transmil_forward_train_f32(C.byref(d), C.byref(w), x.data_ptr(), logits.data_ptr(), n,
                                                          stash.data_ptr(), stash.numel(), fc1_p, attn_p, seed, st),
                       "rrt_transmil_forward_train_f32")
        ctx.model, ctx.stash, ctx.ws_bytes, ctx.drop = model, stash, ws_b.value, (fc1_p, attn_p, seed)
        # the backward reads the parameters through their live pointers: an in-place update between forward and backward
        # (optimizer.step() before a second backward through a retained graph) must not go unnoticed
        ctx.versions = [(p_.data_ptr(), p_._version) for p_ in params]
        ctx.save_for_backward(x)
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        lib = _lib.load()
        model = ctx.model
        (x,) = ctx.saved_tensors
        params = model._step_params()
        if ctx.versions != [(p_.data_ptr(), p_._version) for p_ in params]:
            raise RuntimeError("TransMIL: a parameter was modified in place (or replaced) between this forward and its "
                               "backward; the backward kernels read the live weights, so the gradients would be wrong -- "
                               "run the forward again")
        n, dev = x.shape[0], x.device
        d_logits = d_logits.contiguous().float()
        keep = []
        d, w = model._desc_weights(keep)
        # fresh tensors on every call: autograd (and torch.autograd.grad's caller) may keep what is returned here
        grads = [torch.empty(p_.shape, dtype=torch.float32, device=dev) for p_ in params]
        gstruct = _lib.TransmilGrads()
        slots = (C.c_void_p * len(grads)).from_buffer(gstruct)      # one float* per parameter, in _step_params' order
        for i, g in enumerate(grads):
            slots[i] = g.data_ptr()
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        ws = model._backward_workspace(ctx.ws_bytes, dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_transmil_backward_f32(C.byref(d), C.byref(w), x.data_ptr(), d_logits.data_ptr(),
                                                     ctx.stash.data_ptr(), ctx.stash.numel(), C.byref(gstruct), _ptr(dx), n,
                                                     ws.data_ptr(), ws.numel(), ctx.drop[0], ctx.drop[1], ctx.drop[2], st),
                       "rrt_transmil_backward_f32")
        return (None, dx, None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[5:]))


class NystromAttention(HeadState, nn.Module):
    """modules/nystrom_attention.py:32-149.  ``forward(x)`` with x (1, n, dim) -> (1, n, dim); ``forward_batch(x)`` with x
    (b, n, dim), 1 <= b <= 4096 -> (b, n, dim): one launch per stage for all b sequences and ONE pseudo-inverse scale over the
    whole batch, as the reference's forward on a batch (rrt_nystrom_attention_batched_f32; inference by default, and after
    ``enable_training()`` with a graph through the batched backward, b <= 2048 -- ``forward`` and ``attention_row`` keep b = 1);
    ``mask=`` and
    ``return_attn=True`` are not implemented (the reference's mask branch names undefined variables, and TransMIL passes
    neither); ``attention_row(x, row)`` gives one row of the approximated attention matrix.  The HIP path supports dim_head = 64, num_landmarks = 256, heads <= 16, pinv_iterations <= 16, an odd
    residual_conv_kernel <= 63 and dim a multiple of 32 up to 1024; anything else raises NotImplementedError at the call."""

    def __init__(self, dim, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6, residual=True,
                 residual_conv_kernel=33, eps=1e-8, dropout=0.):
        super().__init__()
        self.eps = eps
        inner_dim = heads * dim_head
        self.num_landmarks = num_landmarks
        self.pinv_iterations = pinv_iterations
        self.heads = heads
        self.dim, self.dim_head = dim, dim_head
        self.scale = dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))
        self.residual = residual
        self.residual_conv_kernel = residual_conv_kernel
        if residual:
            self.res_conv = nn.Conv2d(heads, heads, (residual_conv_kernel, 1), padding=(residual_conv_kernel // 2, 0),
                                      groups=heads, bias=False)
        self._dropout = dropout
        self._ws = None
        self._train_enabled = False

    def enable_training(self, mode=True):
        """Opt in to (or out of) the training path: with it on, a call that needs a graph -- or ``train()`` with dropout --
        runs the HIP forward-with-stash and backward under autograd instead of raising.  A plain attribute: not part of
        ``state_dict``, kept by pickle and deepcopy.  Returns self."""
        self._train_enabled = bool(mode)
        return self

    def _desc(self):
        d = _lib.NystromDesc()
        d.dim, d.heads, d.dim_head, d.num_landmarks = self.dim, self.heads, self.dim_head, self.num_landmarks
        d.pinv_iterations, d.residual, d.residual_conv_kernel = self.pinv_iterations, int(bool(self.residual)), \
            self.residual_conv_kernel
        return d

    def _weights(self, keep):
        """(NystromWeights, ...); the fp32 tensors the pointers refer to are appended to ``keep``"""
        w = _lib.NystromWeights()
        ts = [_param(self.to_qkv.weight), _param(self.to_out[0].weight), _param(self.to_out[0].bias),
              _param(self.res_conv.weight) if self.residual else None]
        keep.extend(ts)
        w.qkv_w, w.out_w, w.out_b, w.conv_w = (_ptr(t) for t in ts)
        return w

    def forward(self, x, mask=None, return_attn=False):
        if mask is not None:
            raise NotImplementedError("rrt_mil_amd.NystromAttention: mask= is not implemented (the reference's mask branch "
                                      "names undefined variables)")
        if return_attn:
            raise NotImplementedError("rrt_mil_amd.NystromAttention: return_attn=True is not implemented")
        _no_cpu(x, "NystromAttention")
        stochastic = self.training and self._dropout > 0.
        layer_path = getattr(self, "_train_enabled", False) and (stochastic or _needs_graph(self, x))
        if not layer_path:
            if stochastic:
                raise NotImplementedError("rrt_mil_amd.NystromAttention in train() with dropout: inference only by default, "
                                          "call eval() under torch.no_grad(), or opt in with enable_training()")
            _no_graph(self, x, "NystromAttention")
        if x.dim() != 3 or x.shape[0] != 1:
            raise ValueError(f"NystromAttention expects (1, n, dim) -- batch > 1 is not supported by forward(): "
                             f"forward_batch() takes (b, n, dim) for inference -- got {tuple(x.shape)}")
        if x.shape[2] != self.dim:
            raise ValueError(f"expected feature dim {self.dim}, got {x.shape[2]}")
        if layer_path:
            with torch.autocast("cuda", enabled=False):      # fp32 in every context, as the one-call path
                y = _NystromFn.apply(self._desc(), x[0].float(), self.to_qkv.weight, self.to_out[0].weight, self.to_out[0].bias,
                                     self.res_conv.weight if self.residual else None)
                return self.to_out[1](y.unsqueeze(0))
        return self._forward_batched(x)

    def forward_batch(self, x):
        """x (b, n, dim), 1 <= b <= 4096 -> (b, n, dim): what the reference's forward computes on a batch -- every sequence
        padded in front on its own, ONE pseudo-inverse scale over all b * heads matrices -- in one launch per stage
        (rrt_nystrom_attention_batched_f32).  With b = 1 the bits of ``forward``.  Inference by default: ``eval()`` under
        ``torch.no_grad()``.  After ``enable_training()`` a call that needs a graph (or ``train()`` with dropout) runs the
        batched forward-with-stash and backward under autograd (b <= 2048; fp32 under autocast; ``to_out``'s Dropout is
        torch's own, on the result); ``forward`` and ``attention_row`` keep b = 1."""
        _no_cpu(x, "NystromAttention")
        if x.dim() != 3 or x.shape[0] < 1:
            raise ValueError(f"NystromAttention.forward_batch expects (b, n, dim), got {tuple(x.shape)}")
        if x.shape[2] != self.dim:
            raise ValueError(f"expected feature dim {self.dim}, got {x.shape[2]}")
        if (self.training and self._dropout > 0.) or _needs_graph(self, x):
            if not getattr(self, "_train_enabled", False):
                raise NotImplementedError("rrt_mil_amd.NystromAttention.forward_batch is an inference entry (the training path keeps "
                                          "b = 1: the backward kernels take one sequence): call it in eval() under torch.no_grad()")
            with torch.autocast("cuda", enabled=False):      # fp32 in every context, as the one-call path
                y = _NystromBatchedFn.apply(self._desc(), x.float(), self.to_qkv.weight, self.to_out[0].weight,
                                            self.to_out[0].bias, self.res_conv.weight if self.residual else None)
                return self.to_out[1](y)
        return self._forward_batched(x)

    def _forward_batched(self, x):
        lib = _lib.load()
        x3d = x.float().contiguous()
        (b, n, _), dev = x3d.shape, x3d.device
        d, keep = self._desc(), []
        w = self._weights(keep)
        need = C.c_size_t()
        _lib.check(lib.rrt_nystrom_batched_workspace_size(C.byref(d), b, n, C.byref(need)), "rrt_nystrom_batched_workspace_size")
        ws = self._workspace(need.value, dev)
        y = torch.empty((b, n, self.dim), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            # (b = 1: the bits of rrt_nystrom_attention_f32)
            _lib.check(lib.rrt_nystrom_attention_batched_f32(C.byref(d), C.byref(w), x3d.data_ptr(), y.data_ptr(), b, n,
                                                             ws.data_ptr(), ws.numel(), st), "rrt_nystrom_attention_batched_f32")
        return y

    def attention_row(self, x, row=0, in_train=False):
        """x (1, n, dim), ``row`` in [0, n) -> (y (1, n, dim), attn (1, heads, n)): ``forward(x)``, bit for bit, and row
        ``row`` of the Nystrom-approximated attention matrix over the n tokens (the reference's ``return_attn=True`` is row 0
        without column 0 when n % 256 == 0; at other n it reads a zero pad row, here the row is always the token's own).
        One rrt_nystrom_attention_row_f32 call; softmax(ql k^T) is never materialised.  Inference only: ``eval()`` under
        ``torch.no_grad()``.  Not a probability vector: the front pad keys keep their share, so the row does not sum to 1,
        and entries can be negative (the pseudo-inverse is an approximation).

        ``in_train=True`` lifts the ``eval()`` condition (not the ``torch.no_grad()`` one): the row does not depend on the
        output dropout, so a momentum teacher that runs in ``train()`` may read it.  ``y`` is then the result BEFORE
        ``to_out``'s Dropout, which the caller applies (mhim_sattn.SAttention does)."""
        _no_cpu(x, "NystromAttention")
        _no_map_with_graph(self, x, self.training and self._dropout > 0. and not in_train, "NystromAttention.attention_row")
        if x.dim() != 3 or x.shape[0] != 1:
            raise ValueError(f"NystromAttention.attention_row expects (1, n, dim) -- it keeps b = 1, batch > 1 is "
                             f"forward_batch() only -- got {tuple(x.shape)}")
        if x.shape[2] != self.dim:
            raise ValueError(f"expected feature dim {self.dim}, got {x.shape[2]}")
        lib = _lib.load()
        x2d = x[0].float().contiguous()
        n, dev = x2d.shape[0], x2d.device
        if not 0 <= int(row) < n:
            raise ValueError(f"row must be in [0, {n}), got {row}")
        d, keep = self._desc(), []
        w = self._weights(keep)
        need = C.c_size_t()
        _lib.check(lib.rrt_nystrom_attention_row_workspace_size(C.byref(d), n, C.byref(need)),
                   "rrt_nystrom_attention_row_workspace_size")
        ws = self._workspace(need.value, dev)
        y = torch.empty((n, self.dim), dtype=torch.float32, device=dev)
        attn = torch.empty((self.heads, n), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_nystrom_attention_row_f32(C.byref(d), C.byref(w), x2d.data_ptr(), y.data_ptr(), int(row),
                                                         attn.data_ptr(), n, ws.data_ptr(), ws.numel(), st),
                       "rrt_nystrom_attention_row_f32")
        return y.unsqueeze(0), attn.unsqueeze(0)


def _no_map_with_graph(module, x, stochastic, who):
    """the attention map is an inference output, with or without enable_training()"""
    if stochastic or _needs_graph(module, x):
        raise NotImplementedError(f"rrt_mil_amd.{who}: the attention map is an inference output (no gradient flows through "
                                  "it, and the training path does not compute it): call it in eval() under torch.no_grad()")


class _NystromLayer(nn.Module):
    """modules/transmil.py:26-44 (its TransLayer): x + attn(norm(x)).  Parameter holder; TransMIL's forward is one call."""

    def __init__(self, norm_layer=nn.LayerNorm, dim=512):
        super().__init__()
        self.norm = norm_layer(dim)
        self.attn = NystromAttention(dim=dim, dim_head=dim // 8, heads=8, num_landmarks=dim // 2, pinv_iterations=6,
                                     residual=True, dropout=0.1)


class PPEG(nn.Module):
    """modules/transmil.py:47-61.  Parameter holder (three depth-wise convs); TransMIL's forward is one call."""

    def __init__(self, dim=512):
        super().__init__()
        self.proj = nn.Conv2d(dim, dim, 7, 1, 7 // 2, groups=dim)
        self.proj1 = nn.Conv2d(dim, dim, 5, 1, 5 // 2, groups=dim)
        self.proj2 = nn.Conv2d(dim, dim, 3, 1, 3 // 2, groups=dim)


class TransMIL(HeadState, nn.Module):
    """modules/transmil.py:64-125.  ``model(x)`` with x (1, N, input_dim) or (N, input_dim) -> logits (1, n_classes)."""
    _TRANSIENT = HeadState._TRANSIENT + ("_bwd_ws",)     # the step's backward workspaces stay with the process too

    def __init__(self, input_dim, n_classes, dropout, act):
        super().__init__()
        self.pos_layer = PPEG(dim=512)
        fc1 = [nn.Linear(input_dim, 512)]
        if act.lower() == 'relu':
            fc1 += [nn.ReLU()]
        elif act.lower() == 'gelu':
            fc1 += [nn.GELU()]
        if dropout:
            fc1 += [nn.Dropout(0.25)]
        self._fc1 = nn.Sequential(*fc1)
        self.cls_token = nn.Parameter(torch.randn(1, 1, 512))
        nn.init.normal_(self.cls_token, std=1e-6)
        self.n_classes = n_classes
        self.layer1 = _NystromLayer(dim=512)
        self.layer2 = _NystromLayer(dim=512)
        self.norm = nn.LayerNorm(512)
        self._fc2 = nn.Linear(512, self.n_classes)
        self.apply(initialize_weights)
        self._act = {"relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU}.get(act.lower(), _lib.ACT_NONE)
        self._ws = None
        self._train_enabled = False
        self._one_call = False

    def enable_training(self, mode=True, one_call=False):
        """Opt in to (or out of) the training path, here and in both attention modules (see
        NystromAttention.enable_training).  With ``one_call=True`` a call that needs a graph (or ``train()`` with dropout)
        is ONE rrt_transmil_forward_train_f32 call and its backward ONE rrt_transmil_backward_f32 call instead of torch
        ops around the two attentions; ``return_features=True`` with a
        graph keeps taking the layer path (the step has no feat).  Dropout then uses the library's stateless mask, seeded
        from torch's CPU generator (``torch.manual_seed`` reproduces a run; a ``drop_seed`` attribute pins it): the
        distribution of torch's dropout, not its bits.  Returns self."""
        self._train_enabled = bool(mode)
        self._one_call = bool(mode) and bool(one_call)
        self.layer1.attn.enable_training(mode)
        self.layer2.attn.enable_training(mode)
        return self

    def _backward_workspace(self, need, dev):
        """the one-call step's backward workspace, kept per device and grown on demand: nothing in it outlives the call (the
        gradients are fresh tensors, the stash belongs to the graph node), and backward calls of one model on one device are
        ordered on the stream"""
        cache = self.__dict__.setdefault("_bwd_ws", {})
        ws = cache.get(dev)
        if ws is None or ws.numel() < need:
            ws = cache[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    def _step_params(self):
        """the 25 parameters in the order of rrt_transmil_grads' pointers"""
        ps = [self._fc1[0].weight, self._fc1[0].bias, self.cls_token]
        for layer in (self.layer1, self.layer2):
            ps += [layer.norm.weight, layer.norm.bias, layer.attn.to_qkv.weight, layer.attn.to_out[0].weight,
                   layer.attn.to_out[0].bias, layer.attn.res_conv.weight]
        convs = (self.pos_layer.proj, self.pos_layer.proj1, self.pos_layer.proj2)
        ps += [c.weight for c in convs] + [c.bias for c in convs]
        return ps + [self.norm.weight, self.norm.bias, self._fc2.weight, self._fc2.bias]

    def _forward_step(self, x2d):
        """The one-call step under autograd -> logits (1, n_classes).  fp32 in every context."""
        fc1_p = attn_p = 0.0
        if self.training:
            fc1_p = float(self._fc1[-1].p) if isinstance(self._fc1[-1], nn.Dropout) else 0.0
            attn_p = float(self.layer1.attn.to_out[1].p)
            if float(self.layer2.attn.to_out[1].p) != attn_p:
                raise NotImplementedError("rrt_mil_amd.TransMIL one-call step: both attention layers must share one dropout p")
        seed = 0
        if fc1_p > 0. or attn_p > 0.:
            fixed = getattr(self, "drop_seed", None)
            seed = int(fixed) if fixed is not None else int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        with torch.autocast("cuda", enabled=False):
            return _TransmilStepFn.apply(self, x2d, fc1_p, attn_p, seed, *self._step_params())

    def _forward_layers(self, x2d):
        """The layer path under autograd: torch ops around the two HIP attentions -> (logits (1, n_classes), the
        (1 + H*H, 512) rows before the last LayerNorm).  fp32 in every context."""
        import torch.nn.functional as F
        with torch.autocast("cuda", enabled=False):
            h = self._fc1(x2d.float())
            N, D = h.shape
            H = _ceil_sqrt(N)
            h = torch.cat([self.cls_token.reshape(1, D).float(), h, h[:H * H - N]])     # the wrap, then the cls token in front
            h = h + self.layer1.attn(self.layer1.norm(h).unsqueeze(0))[0]
            img = h[1:].t().reshape(1, D, H, H)
            pe = img
            for conv in (self.pos_layer.proj, self.pos_layer.proj1, self.pos_layer.proj2):
                pe = pe + F.conv2d(img, conv.weight, conv.bias, padding=conv.kernel_size[0] // 2, groups=D)
            h = torch.cat([h[:1], pe.reshape(D, H * H).t()])
            h = h + self.layer2.attn(self.layer2.norm(h).unsqueeze(0))[0]
            return self._fc2(self.norm(h[:1])), h

    def _desc_weights(self, keep):
        d, w = _lib.TransmilDesc(), _lib.TransmilWeights()
        d.input_dim, d.n_classes, d.act = self._fc1[0].in_features, self.n_classes, self._act
        d.attn = self.layer1.attn._desc()

        def p(t):
            t = _param(t)
            keep.append(t)
            return t.data_ptr()

        w.fc1_w, w.fc1_b, w.cls_token = p(self._fc1[0].weight), p(self._fc1[0].bias), p(self.cls_token)
        for i, layer in enumerate((self.layer1, self.layer2)):
            w.layer[i].norm_w, w.layer[i].norm_b = p(layer.norm.weight), p(layer.norm.bias)
            w.layer[i].attn = layer.attn._weights(keep)
        for i, conv in enumerate((self.pos_layer.proj, self.pos_layer.proj1, self.pos_layer.proj2)):
            w.pos_w[i], w.pos_b[i] = p(conv.weight), p(conv.bias)
        w.norm_w, w.norm_b = p(self.norm.weight), p(self.norm.bias)
        w.fc2_w, w.fc2_b = p(self._fc2.weight), p(self._fc2.bias)
        return d, w

    def forward_bag(self, x2d, return_features=False, return_attn=False):
        """One bag: x2d (N, input_dim) device tensor -> logits (1, n_classes) through ONE rrt_transmil_forward_f32 call
        (with ``return_features`` also the (1 + H*H, 512) rows before the last LayerNorm).

        With ``return_attn`` the result gains, last, ``attn`` (2, heads, N), indexed [layer, head, patch]: the class token's
        row of the Nystrom-approximated attention matrix in layer 1 and in layer 2, without its own column, the wrap folded
        back (the sequence is [cls, h_0 .. h_{N-1}, h_0 .. h_{H*H-N-1}], so patch i < H*H - N gets the sum of its two
        columns).  One rrt_transmil_forward_attn_f32 call plus two torch ops for the fold; the logits (and features) have
        the bits of the call without it.  Inference only.  Not a probability vector: the cls column and the front pad keys
        keep their share, so a row does not sum to 1, and entries can be negative."""
        _no_cpu(x2d, "TransMIL")
        stochastic = self.training and any(isinstance(m, nn.Dropout) and m.p > 0. for m in self.modules())
        if return_attn:
            _no_map_with_graph(self, x2d, stochastic, "TransMIL(return_attn=True)")
        layer_path = getattr(self, "_train_enabled", False) and (stochastic or _needs_graph(self, x2d))
        if not layer_path:
            if stochastic:
                raise NotImplementedError("rrt_mil_amd.TransMIL in train() with dropout: inference only by default, call eval() "
                                          "under torch.no_grad(), or opt in with enable_training()")
            _no_graph(self, x2d, "TransMIL")
        if x2d.dim() != 2:
            raise ValueError(f"forward_bag expects (N, input_dim), got {tuple(x2d.shape)}")
        n, in_dim = x2d.shape
        if in_dim != self._fc1[0].in_features:
            raise ValueError(f"expected feature dim {self._fc1[0].in_features}, got {in_dim}")
        if layer_path and getattr(self, "_one_call", False) and not return_features:
            return self._forward_step(x2d)
        if layer_path:
            logits, feat = self._forward_layers(x2d)
            return (logits, feat) if return_features else logits
        lib = _lib.load()
        x2d = x2d.float().contiguous()
        keep = []
        d, w = self._desc_weights(keep)
        need = C.c_size_t()
        size_fn = lib.rrt_transmil_attn_workspace_size if return_attn else lib.rrt_transmil_workspace_size
        _lib.check(size_fn(C.byref(d), n, C.byref(need)), size_fn.__name__)
        dev = x2d.device
        ws = self._workspace(need.value, dev)
        logits = torch.empty((1, self.n_classes), dtype=torch.float32, device=dev)
        feat = None
        side = _ceil_sqrt(n)
        if return_features:
            feat = torch.empty((1 + side * side, 512), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            if not return_attn:
                _lib.check(lib.rrt_transmil_forward_f32(C.byref(d), C.byref(w), x2d.data_ptr(), logits.data_ptr(), _ptr(feat), n,
                                                        ws.data_ptr(), ws.numel(), st), "rrt_transmil_forward_f32")
                return (logits, feat) if return_features else logits
            rows = torch.empty((2, d.attn.heads, 1 + side * side), dtype=torch.float32, device=dev)
            _lib.check(lib.rrt_transmil_forward_attn_f32(C.byref(d), C.byref(w), x2d.data_ptr(), logits.data_ptr(), _ptr(feat),
                                                         rows[0].data_ptr(), rows[1].data_ptr(), n, ws.data_ptr(), ws.numel(),
                                                         st), "rrt_transmil_forward_attn_f32")
        # without the cls column; the wrapped rows' columns go back to their patches
        attn = rows[:, :, 1:1 + n].clone()
        attn[:, :, :side * side - n] += rows[:, :, 1 + n:]
        return (logits, feat, attn) if return_features else (logits, attn)

    def forward_bags(self, bags, return_attn=False):
        """A list of independent slides (each (N_i, input_dim) or (1, N_i, input_dim)) -> list of logits (with
        ``return_attn``: of (logits, attn) pairs): a plain loop of forward_bag on the caller's stream."""
        return [self.forward(b, return_attn=return_attn) for b in bags]

    def forward(self, x, return_attn=False):
        """x (1, N, input_dim) or (N, input_dim) -> logits (1, n_classes); with ``return_attn`` -> (logits, attn (2, heads, N)),
        see forward_bag."""
        _no_cpu(x, "TransMIL")
        if x.dim() == 3:
            if x.shape[0] != 1:
                raise ValueError(f"TransMIL expects one bag, (1, N, input_dim) or (N, input_dim) -- batch > 1 is not "
                                 f"supported -- got {tuple(x.shape)}")
            x = x[0]
        return self.forward_bag(x, return_attn=return_attn)


def _ceil_sqrt(n):
    h = int(n ** 0.5)
    while h * h < n:
        h += 1
    while h > 1 and (h - 1) * (h - 1) >= n:
        h -= 1
    return h
