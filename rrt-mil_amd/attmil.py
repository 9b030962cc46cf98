"""ABMIL and gated ABMIL -- the reference's ``--model attmil`` / ``--model gattmil`` heads (modules/attmil.py ``DAttention``,
``AttentionGated``) around the MI355X encoder.

``--only_rrt_enc --model attmil|gattmil`` builds an RRTEncoder and hands it to the head as ``rrt=``.  Same constructors, the
same ``feature`` ``nn.Sequential`` layout (the index of ``rrt`` moves with ``dropout``), the same parameter names: reference
checkpoints load with ``strict=True``.  At the top level the classes are ``rrt_mil_amd.ABMIL`` and ``rrt_mil_amd.GatedABMIL``
(``rrt_mil_amd.DAttention`` / ``AttentionGated`` name the pooling modules of modules/datten.py).

In ``eval()`` without a graph a bag is ONE C-ABI call (rrt_bagmil_forward_f32: the shared head front, the ABMIL pool of
csrc/mil_pool.hip and the classifier in its merge block); with a graph or in ``train()`` the encoder is its HIP autograd
Function, the attention Linears run on the library GEMMs and the pooling is ``_AttnPool``.

The reference's quirks, kept: ``AttentionGated`` hard-codes ``Linear(1024, 512)``, a 2-class classifier and an always-on
``Dropout(0.25)``; its ``input_dim`` is the attention width L, so only ``input_dim=512`` can run -- other values construct
(their checkpoints load) and raise ``ValueError`` at the call.
"""
from torch import nn

from . import _lib
from ._head import BagHead
from .mil import _AttnPool


def initialize_weights(module):
    """modules/attmil.py:6-25"""
    for m in module.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.xavier_normal_(m.weight)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)


def attn_tail(head, y, a_mods, b_mods, lin_c, compute):
    """y (N, 512) through an attention pool on the layer path: the first Linears on the library GEMMs, their activations (and
    Dropouts) as torch modules, scores + softmax over the bag + weighted sum as `_AttnPool` -> (pooled (512,), attn (N,),
    a_raw (N,))"""
    def seq(mods):
        t = head._lin(mods[0], y, compute)
        for m in list(mods)[1:]:
            t = m(t)
        return t
    return _AttnPool.apply(y, seq(a_mods), seq(b_mods) if b_mods is not None else None, lin_c.weight, lin_c.bias)


class DAttention(BagHead, nn.Module):
    """modules/attmil.py:112-158.  ``rrt``: an rrt_mil_amd.RRTEncoder of width 512, or None.

    ``forward(x, return_attn=False, no_norm=False)`` returns what the reference returns: ``Y_prob`` (1, n_classes), or
    ``(Y_prob, A)`` with A (1, N) the softmax over the bag -- with ``no_norm`` the raw scores in the reference's (N, 1)."""
    _POOL = _lib.BAGPOOL_ATTN
    _NAME = "ABMIL"

    def __init__(self, input_dim, n_classes, dropout, act, rrt=None):
        super().__init__()
        self._check_rrt(rrt)
        self.L, self.D, self.K = 512, 128, 1
        feature = [nn.Linear(input_dim, 512), nn.GELU() if act.lower() == 'gelu' else nn.ReLU()]
        if dropout:
            feature += [nn.Dropout(0.25)]
        if rrt is not None:
            feature += [rrt]
        self.feature = nn.Sequential(*feature)
        self.attention = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh(), nn.Linear(self.D, self.K))
        self.classifier = nn.Sequential(nn.Linear(self.L * self.K, n_classes))
        self.apply(initialize_weights)
        self._emb_act = _lib.ACT_GELU if act.lower() == 'gelu' else _lib.ACT_RELU
        self._ws = None

    def _front(self):
        return list(self.feature)

    def _classifier(self):
        return self.classifier[0]

    def _fill(self, d, w, p):
        a, c = self.attention[0], self.attention[2]
        d.pool_hidden, d.pool_act = self.D, _lib.ACT_TANH
        w.a_w, w.a_b, w.c_w, w.c_b = p(a.weight), p(a.bias), p(c.weight), p(c.bias)

    def _tail(self, y, no_norm, compute):
        pooled, attn, a_raw = attn_tail(self, y, list(self.attention)[:2], None, self.attention[2], compute)
        return self.classifier(pooled.unsqueeze(0)), (a_raw if no_norm else attn)

    def forward(self, x, return_attn=False, no_norm=False):
        logits, a = self._run(x, return_attn=True, no_norm=no_norm) if return_attn else self._run(x)
        if not return_attn:
            return logits
        return logits, (a.reshape(-1, 1) if no_norm else a.reshape(1, -1))


class AttentionGated(BagHead, nn.Module):
    """modules/attmil.py:55-110.  ``forward(x)`` returns ``Y_prob`` (1, 2)."""
    _POOL = _lib.BAGPOOL_ATTN_GATED
    _NAME = "GatedABMIL"

    def __init__(self, input_dim, act='relu', bias=False, dropout=False, rrt=None):
        super().__init__()
        self._check_rrt(rrt)
        self.L, self.D, self.K = input_dim, 128, 1
        feature = [nn.Linear(1024, 512), nn.ReLU(), nn.Dropout(0.25)]
        if rrt is not None:
            feature += [rrt]
        self.feature = nn.Sequential(*feature)
        self.classifier = nn.Sequential(nn.Linear(self.L * self.K, 2))
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
        self.apply(initialize_weights)
        self._emb_act = _lib.ACT_RELU
        self._pool_act = _lib.ACT_BY_NAME.get(act, _lib.ACT_NONE)
        self._ws = None

    def _front(self):
        return list(self.feature)

    def _classifier(self):
        return self.classifier[0]

    def _dropouts(self):
        return [m for m in list(self.feature) + list(self.attention_a) + list(self.attention_b) if isinstance(m, nn.Dropout)]

    def _check_call(self, n):
        if self.L != 512:
            raise ValueError(f"GatedABMIL(input_dim={self.L}): input_dim is the attention width behind the hard-coded "
                             "Linear(1024, 512) (modules/attmil.py:58-62), so only input_dim=512 can run -- the reference "
                             "fails on this combination too")

    def _fill(self, d, w, p):
        a, b, c = self.attention_a[0], self.attention_b[0], self.attention_c
        d.pool_hidden, d.pool_act = self.D, self._pool_act
        w.a_w, w.a_b, w.b_w, w.b_b, w.c_w, w.c_b = p(a.weight), p(a.bias), p(b.weight), p(b.bias), p(c.weight), p(c.bias)

    def _tail(self, y, no_norm, compute):
        pooled, attn, a_raw = attn_tail(self, y, self.attention_a, self.attention_b, self.attention_c, compute)
        return self.classifier(pooled.unsqueeze(0)), (a_raw if no_norm else attn)

    def forward(self, x):
        return self._run(x)[0]


ABMIL, GatedABMIL = DAttention, AttentionGated
