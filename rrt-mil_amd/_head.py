"""What the classifier heads share on the host side: the per-process device state of a module (grow-on-demand workspace,
left out of pickles), the one-call C-ABI forward with its 16-bit weight-image key, and the bag scheduler of ``forward_bags``.

``HeadState`` is a mixin in front of ``nn.Module``: RRTMIL, CLAM_SB / CLAM_MB and MILNet use all of it, TransMIL and
NystromAttention the workspace cache and the pickling pair.
"""
import ctypes as C

import torch

from . import _lib


def head_compute(enc):
    """RRT_COMPUTE_* of a head whose encoder is optional: the encoder's own mode, else what autocast asks for"""
    if enc is not None:
        return enc._compute_mode()
    if torch.is_autocast_enabled("cuda"):
        return {torch.bfloat16: _lib.COMPUTE_BF16, torch.float16: _lib.COMPUTE_F16}.get(torch.get_autocast_dtype("cuda"),
                                                                                         _lib.COMPUTE_F32)
    return _lib.COMPUTE_F32


class HeadState:
    # device workspaces and their validity keys stay with the process (deepcopy / pickle); a class lists its own extra keys
    _TRANSIENT = ("_ws", "_slots", "_w16_key")
    _RESET = ("_ws",)                  # ... and the attributes that come back as None

    def __getstate__(self):
        st = dict(self.__dict__)
        for k in self._TRANSIENT:
            st.pop(k, None)
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        for k in self._RESET:
            self.__dict__.setdefault(k, None)

    def _workspace(self, need, dev):
        """the module's cached workspace tensor, grown on demand (per device)"""
        if self._ws is None or self._ws.device != dev or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    def _head_forward(self, head, d, w, x2d, args, lowp):
        """One bag through ``rrt_<head>_forward_f32(d, w, x2d, *args, n, workspace, bytes, stream)`` on the bag's device
        and its current stream, out of the module's workspace.  ``lowp``: the call keeps 16-bit images of the encoder's
        weights inside that workspace (their place depends on n).  Are they still those of these weights?  The key of the
        last successful call says so (rrt_encoder_desc.weights16_valid, see RRTEncoder.forward_bag)."""
        lib = _lib.load()
        n, dev = x2d.shape[0], x2d.device
        need = C.c_size_t()
        _lib.check(getattr(lib, f"rrt_{head}_workspace_size")(C.byref(d), n, C.byref(need)), f"rrt_{head}_workspace_size")
        ws = self._workspace(need.value, dev)
        with torch.cuda.device(dev):             # kernels launch on the bag's device, whatever the current one is
            stream = torch.cuda.current_stream(dev).cuda_stream
            key = (ws.data_ptr(), d.enc.compute, w.enc.version, stream, n)
            d.enc.weights16_valid = int(bool(lowp) and key == self.__dict__.get("_w16_key"))
            rc = getattr(lib, f"rrt_{head}_forward_f32")(C.byref(d), C.byref(w), x2d.data_ptr(), *args, n, ws.data_ptr(),
                                                         ws.numel(), stream)
            self.__dict__["_w16_key"] = key if rc == 0 and lowp else None
        _lib.check(rc, f"rrt_{head}_forward_f32")

    @torch.no_grad()
    def _schedule_bags(self, bags, streams, one, tensors):
        """``one(x2d, solo)`` for every slide of ``bags`` (each (N_i, input_dim) or (1, N_i, input_dim)) with up to
        ``streams`` slides in flight -> list of its results in the order of ``bags``.  Each slide runs with a workspace of
        its own on one of the process's bag streams (the same list RRTEncoder.forward_bags uses; at most four: the chip
        schedules four hardware queues), big slides first, each on the least loaded stream.  Ordered like one op of the
        caller's stream: the bag streams wait for it, and the host waits for them before the call returns (the call BLOCKS
        the host; it swaps the module's workspace per stream slot while it runs, so one call at a time per module: not
        re-entrant, not thread-safe).  ``tensors(result)`` enumerates a result's tensors."""
        from .encoder import _BAG_STREAMS
        dev = bags[0].device
        S = max(1, min(int(streams), 4, len(bags)))
        pool = _BAG_STREAMS.setdefault(dev, [])
        while len(pool) < S:
            pool.append(torch.cuda.Stream(dev))
        slots = self.__dict__.setdefault("_slots", {})
        cur = torch.cuda.current_stream(dev)
        order = sorted(range(len(bags)), key=lambda i: -bags[i].shape[-2])
        load, outs = [0] * S, [None] * len(bags)
        for st in pool[:S]:
            st.wait_stream(cur)
        ws_was, key_was = self._ws, self.__dict__.get("_w16_key")
        try:
            for i in order:
                s_ = min(range(S), key=lambda t: load[t])
                load[s_] += bags[i].shape[-2]
                b = bags[i]
                self._ws, self.__dict__["_w16_key"] = slots.get((dev, s_), (None, None))
                with torch.cuda.stream(pool[s_]):
                    outs[i] = one(b[0] if b.dim() == 3 else b, S == 1)
                slots[(dev, s_)] = (self._ws, self.__dict__.get("_w16_key"))
                # the outputs were allocated under the bag stream (the caching allocator ties a block to the stream it was
                # taken on) and are consumed on the caller's: tell the allocator, so that a freed logits / attention row
                # is not handed out again on the bag stream while the caller's stream still reads it
                for t_ in tensors(outs[i]):
                    t_.record_stream(cur)
        finally:
            self._ws, self.__dict__["_w16_key"] = ws_was, key_was
            for st in pool[:S]:
                st.synchronize()      # host wait: nothing is parked on the caller's stream
        return outs


def instance_max(y, weight, bias, return_classes=False):
    """y (N, dim) fp32 device tensor, weight (C, dim), bias (C,) or None -> (cmax (C,), argmax (C,) int64[, classes (N, C)])
    through rrt_instance_max_f32 (no graph)."""
    lib = _lib.load()
    if not y.is_cuda:
        raise _lib.RRTHipError("rrt_mil_amd.dsmil runs on MI355X only; there is no CPU fallback")
    y, w = y.detach().float().contiguous(), weight.detach().float().contiguous()
    b = bias.detach().float().contiguous() if bias is not None else None
    (n, d), c = y.shape, w.shape[0]
    dev = y.device
    cmax = torch.empty(c, dtype=torch.float32, device=dev)
    idx = torch.empty(c, dtype=torch.int64, device=dev)
    classes = torch.empty((n, c), dtype=torch.float32, device=dev) if return_classes else None
    need = C.c_size_t()
    _lib.check(lib.rrt_instance_max_workspace_size(n, d, c, C.byref(need)), "rrt_instance_max_workspace_size")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.rrt_instance_max_f32(y.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                            classes.data_ptr() if classes is not None else None, cmax.data_ptr(), idx.data_ptr(),
                                            n, d, c, ws.data_ptr(), ws.numel(), st), "rrt_instance_max_f32")
    return (cmax, idx, classes) if return_classes else (cmax, idx)


class _InstanceMax(torch.autograd.Function):
    """cmax[j] = max_n (y_n . w[j] + b[j]) and its row m_j as ONE pass over y (rrt_instance_max_f32); the [N, C] scores are
    never stored.  The backward is sparse -- d y[m_j] += d cmax_j w[j], d w[j] = d cmax_j y[m_j], d b = d cmax -- never a
    dense [N, C] product.  (MILNet's instance stream and MaxMIL's tail.)"""

    @staticmethod
    def forward(ctx, y, weight, bias):
        cmax, idx = instance_max(y, weight, bias)
        ctx.save_for_backward(y.detach().float().index_select(0, idx), weight, idx)
        ctx.n, ctx.has_bias = y.shape[0], bias is not None
        ctx.mark_non_differentiable(idx)
        return cmax, idx

    @staticmethod
    def backward(ctx, d_cmax, _d_idx):
        ym, weight, idx = ctx.saved_tensors
        d_cmax = d_cmax.float()
        rows = d_cmax[:, None] * weight.float()
        dy = torch.zeros((ctx.n, ym.shape[1]), dtype=torch.float32, device=ym.device)
        for j in range(idx.shape[0]):              # one class at a time: two classes may share a critical instance
            dy.index_add_(0, idx[j:j + 1], rows[j:j + 1])
        return dy, d_cmax[:, None] * ym, (d_cmax if ctx.has_bias else None)


class _BagMean(torch.autograd.Function):
    """logits[j] = mean_n (y_n . w[j] + b[j]) = w[j] . colmean(y) + b[j] as ONE pass over y (rrt_bag_mean_f32; [N, C] never
    exists) and its adjoint (rrt_bag_mean_backward_f32: one row written N times, d w from the stashed column mean)."""

    @staticmethod
    def forward(ctx, y, weight, bias):
        lib = _lib.load()
        if not y.is_cuda:
            raise _lib.RRTHipError("rrt_mil_amd.mean_max runs on MI355X only; there is no CPU fallback")
        y, w = y.detach().float().contiguous(), weight.detach().float().contiguous()
        b = bias.detach().float().contiguous() if bias is not None else None
        (n, d), c = y.shape, w.shape[0]
        dev = y.device
        logits = torch.empty(c, dtype=torch.float32, device=dev)
        colmean = torch.empty(d, dtype=torch.float32, device=dev)
        need = C.c_size_t()
        _lib.check(lib.rrt_bag_mean_workspace_size(n, d, c, C.byref(need)), "rrt_bag_mean_workspace_size")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_bag_mean_f32(y.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, logits.data_ptr(),
                                            colmean.data_ptr(), n, d, c, ws.data_ptr(), ws.numel(), st), "rrt_bag_mean_f32")
        ctx.save_for_backward(colmean, w)
        ctx.n, ctx.has_bias = n, bias is not None
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        lib = _lib.load()
        colmean, w = ctx.saved_tensors
        d_logits = d_logits.float().contiguous()
        (c, d), dev = w.shape, w.device
        dy = torch.empty((ctx.n, d), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        db = torch.empty(c, dtype=torch.float32, device=dev) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        if dy is None and dw is None and db is None:
            return None, None, None
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.rrt_bag_mean_backward_f32(d_logits.data_ptr(), colmean.data_ptr(), w.data_ptr(), p(dy), p(dw), p(db),
                                                     ctx.n, d, c, st), "rrt_bag_mean_backward_f32")
        return dy, dw, db


def copy_encoder_desc(dst, enc, who):
    """The ONE place a head copies its encoder's descriptor into its own (RRTMIL, CLAM, DSMIL and the BagHead family): the
    one-call head kernels run the plain R-MSA layers, so an encoder built with attn='ntrans' / region_attn='ntrans' -- whose
    layers hold NystromAttention parameters in other slots -- must never reach them."""
    if getattr(enc, "_nys_mode", 0):
        raise NotImplementedError(f"rrt_mil_amd.{who}: the one-call head entries (forward_bag, forward_bags) run the R-MSA "
                                  "kernels and do not cover an RRTEncoder with attn='ntrans' / region_attn='ntrans' "
                                  "(NystromAttention layers); call the encoder itself in eval() under torch.no_grad() "
                                  "(RRTMIL: the module call)")
    C.memmove(C.byref(dst), C.byref(enc._desc), C.sizeof(_lib.EncoderDesc))


class BagHead(HeadState):
    """What the reference's plain MIL heads share (modules/attmil.py, attmil_ibmil.py, mean_max.py): a front -- embedding
    Linear + activation (+ Dropout) (+ ``rrt``) -- and a pool-specific tail.  In ``eval()`` without a graph a bag is ONE
    C-ABI call (rrt_bagmil_forward_f32: forward_bag / forward_bags); in ``train()`` or with a graph ``forward`` takes the
    layer path: torch Dropout + the library GEMM for the embedding, the encoder's HIP autograd Function, then ``_tail``.

    A subclass states: ``_POOL`` (RRT_BAGPOOL_*), ``_NAME``, ``_front()`` (the front's modules in order), ``_emb_act``,
    ``_classifier()`` (the nn.Linear behind the pool), ``_fill(d, w, p)`` (the pool's descriptor fields and weights),
    ``_tail(y, no_norm, compute)`` -> (logits (1, C), attention or None) and ``_check_call()`` for what must raise at the call."""
    _POOL = None
    _NAME = "BagHead"

    @staticmethod
    def _check_rrt(rrt):
        from .encoder import RRTEncoder
        if rrt is not None:
            if not isinstance(rrt, RRTEncoder):
                raise TypeError("rrt must be an rrt_mil_amd.RRTEncoder or None")
            if rrt.final_dim != 512:
                raise ValueError(f"rrt.final_dim must be 512 (the embedding width), got {rrt.final_dim}")

    # ------------------------------------------------------------------ pieces
    def _enc(self):
        from .encoder import RRTEncoder
        return next((m for m in self._front() if isinstance(m, RRTEncoder)), None)

    def _compute(self):
        return head_compute(self._enc())

    def _dropouts(self):
        """the nn.Dropout modules the forward applies outside the encoder (a subclass adds those of its pool)"""
        return [m for m in self._front() if isinstance(m, torch.nn.Dropout)]

    def _stochastic(self):
        enc = self._enc()
        return self.training and (any(m.p > 0 for m in self._dropouts()) or (enc is not None and enc._stochastic()))

    def _check_call(self, n):
        """what the reference cannot run (a ValueError that says why), for a bag of n instances"""

    def _check_bag(self, x2d):
        lin = self._front()[0]
        if x2d.dim() != 2 or x2d.shape[0] == 0:
            raise ValueError(f"expected a bag of shape (N, {lin.in_features}), got {tuple(x2d.shape)}")
        self._check_call(x2d.shape[0])
        if x2d.shape[1] != lin.in_features:
            raise ValueError(f"expected a bag of shape (N, {lin.in_features}), got {tuple(x2d.shape)}")
        if not x2d.is_cuda:
            raise _lib.RRTHipError(f"rrt_mil_amd.{self._NAME} runs on MI355X only: move the bag to a 'cuda' (HIP) device; there "
                                   "is no CPU fallback")

    # ------------------------------------------------------------------ the one-call HIP path
    def _desc_weights(self, solo):
        from .encoder import RRTEncoder
        enc, p = self._enc(), RRTEncoder._ptr
        d, w = _lib.BagmilDesc(), _lib.BagmilWeights()
        if enc is not None:
            copy_encoder_desc(d.enc, enc, self._NAME)
            w.enc = enc._weights()
        d.enc.dim = 512
        d.enc.compute = self._compute()
        d.enc.solo = int(bool(solo))       # per-call scheduling hint, never inherited (see RRTMIL._mil_desc)
        lin, cls = self._front()[0], self._classifier()
        d.input_dim, d.emb_act, d.has_rrt = lin.in_features, self._emb_act, int(enc is not None)
        d.n_classes, d.pool = cls.out_features, self._POOL
        w.emb_w, w.emb_b = p(lin.weight), p(lin.bias)
        w.cls_w, w.cls_b = p(cls.weight), p(cls.bias)
        self._fill(d, w, p)
        return d, w

    def forward_bag(self, x2d, return_attn=False, no_norm=False, return_features=False, return_argmax=False,
                    return_deconf=False, solo=True):
        """One bag, eval, no graph: x2d (N, input_dim) fp32 device tensor -> logits (1, n_classes) through ONE
        rrt_bagmil_forward_f32 call.  With any ``return_*`` a dict {logits, attn (N,) (the raw scores with ``no_norm``),
        features (512,) (the pooled embedding; MeanMIL: the column mean), argmax (C,) int64 (MaxMIL), deconf_a (K,) and
        deconf_cf (V,) (IBMIL)} of what was asked for; asking a head for what its pool does not produce is a ValueError.
        ``solo``: the slide has the GPU to itself (forward_bags passes False with several slides in flight)."""
        self._check_bag(x2d)
        if self._stochastic():
            raise NotImplementedError("forward_bag is the one-call inference entry (no dropout inside); in train() call the "
                                      "module itself")
        att = self._POOL in (_lib.BAGPOOL_ATTN, _lib.BAGPOOL_ATTN_GATED, _lib.BAGPOOL_ATTN_DECONF)
        deconf = self._POOL == _lib.BAGPOOL_ATTN_DECONF and getattr(self, "confounder_path", False)
        if ((return_attn and not att) or (return_features and self._POOL == _lib.BAGPOOL_MAX)
                or (return_argmax and self._POOL != _lib.BAGPOOL_MAX) or (return_deconf and not deconf)):
            raise ValueError(f"{self._NAME}: its pool does not produce that output")
        x2d = x2d.float().contiguous()
        n, dev = x2d.shape[0], x2d.device
        d, w = self._desc_weights(solo)
        new = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)   # noqa: E731
        logits = new(1, d.n_classes)
        attn = new(n) if return_attn else None
        feat = new(512) if return_features else None
        amax = new(d.n_classes, dt=torch.int64) if return_argmax else None
        da, dcf = (new(d.deconf_k), new(d.deconf_v)) if return_deconf else (None, None)
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        self._head_forward("bagmil", d, w, x2d, (logits.data_ptr(), p(attn), int(bool(no_norm)), p(feat), p(amax), p(da), p(dcf)),
                           d.enc.compute != _lib.COMPUTE_F32 and d.has_rrt)
        if not (return_attn or return_features or return_argmax or return_deconf):
            return logits
        return {k: v for k, v in (("logits", logits), ("attn", attn), ("features", feat), ("argmax", amax), ("deconf_a", da),
                                  ("deconf_cf", dcf)) if v is not None}

    def forward_bags(self, bags, streams=4, **kw):
        """A batch of independent slides (each (N_i, input_dim) or (1, N_i, input_dim)) -> list of forward_bag results, with
        ``streams`` slides in flight on the heads' bag scheduler (HeadState._schedule_bags: one rrt_bagmil_forward_f32 call
        per slide with its own workspace; the call blocks the host; one call at a time per module), bit for bit
        forward_bag(..., solo=(one stream)) per bag."""
        if not bags:
            return []
        if not bags[0].is_cuda:
            raise _lib.RRTHipError(f"rrt_mil_amd.{self._NAME} runs on MI355X only; there is no CPU fallback")
        if self._stochastic():
            raise NotImplementedError("forward_bags is an inference entry; in train() call the module itself")
        return self._schedule_bags(bags, streams, lambda x2, solo: self.forward_bag(x2, solo=solo, **kw),
                                   lambda o: o.values() if isinstance(o, dict) else (o,))

    # ------------------------------------------------------------------ the layer path (graph, dropout)
    def _gemm_compute(self):
        """the operand precision of the bag-sized Linears on the layer path (F32X3 concerns the R-MSA layers only)"""
        compute = self._compute()
        return _lib.COMPUTE_F32 if compute == _lib.COMPUTE_F32X3 else compute

    @staticmethod
    def _lin(lin, t, compute):
        from .mil import lib_linear
        return lib_linear(lin, t, compute).float()

    def _embed_encode(self, x2d):
        """the front: Linear + act (+ Dropout) (+ encoder) -> (N, 512)"""
        mods = self._front()
        x = self._lin(mods[0], x2d, self._gemm_compute())
        for m in mods[1:]:
            x = m(x)
        return x

    def _run(self, x, return_attn=False, no_norm=False):
        """model(x): x (1, N, input_dim) or (N, input_dim) -> (logits (1, C), attention or None)"""
        if x.dim() == 3 and x.shape[0] != 1:
            raise ValueError(f"{self._NAME} takes one bag per call, got a batch of {x.shape[0]}")
        x2d = x.reshape(-1, x.shape[-1])
        self._check_bag(x2d)
        graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if not graph and not self._stochastic():
            out = self.forward_bag(x2d, return_attn=return_attn, no_norm=no_norm)
            return (out["logits"], out["attn"]) if return_attn else (out, None)
        with torch.set_grad_enabled(graph):
            y = self._embed_encode(x2d)
            compute = self._gemm_compute()
            with torch.autocast("cuda", enabled=False):      # the [1, .] pieces of a tail are fp32 torch ops in every mode
                return self._tail(y.float(), no_norm, compute)
