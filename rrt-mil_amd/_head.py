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
