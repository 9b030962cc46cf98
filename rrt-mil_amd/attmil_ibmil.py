"""IBMIL -- the reference's ``--model ibmil`` head (modules/attmil_ibmil.py ``Dattention_ori`` + ``FCLayer``) around the MI355X
encoder: ABMIL whose pooled bag embedding attends over a fixed set of confounders (cluster centres loaded from ``.npy``
files) and is classified together with the attended confounder.

Same constructors, module tree (``embedding.embed.*``, ``embedding.rrt.*``, ``attention.*``, ``W_q``, ``W_k``, ``head``) and
the ``confounder_feat`` buffer: reference checkpoints load with ``strict=True``.  At the top level the class is
``rrt_mil_amd.IBMIL``.

In ``eval()`` without a graph a bag is ONE C-ABI call (rrt_bagmil_forward_f32: the shared head front, the ABMIL pool with its
pooled row left in device memory, then the one-block deconfounder of csrc/bag_pool.hip).  With a graph or in ``train()`` the
pooling is ``_AttnPool`` and the O(1)-sized deconfounder tail is torch ops on device tensors.

The reference's quirks, kept: ``self.dropout`` (p = 0.5) is defined with a confounder and never applied; a bag of ONE
instance raises ``ValueError`` (the reference's ``x.squeeze()`` drops the bag axis there and its ``torch.mm`` fails).  With
``confounder_path=False`` it is the plain ABMIL head (the reference reads an attribute it never set in that case).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._head import BagHead
from .attmil import attn_tail, initialize_weights  # noqa: F401  (modules/attmil_ibmil.py:6-20 is the same rule)


class FCLayer(nn.Module):
    """modules/attmil_ibmil.py:22-42: the embedding Linear + activation (+ Dropout), then ``rrt`` (Identity without one)."""

    def __init__(self, dropout=0.25, act='relu', in_size=1024, rrt=None):
        super().__init__()
        BagHead._check_rrt(rrt)
        embed = [nn.Linear(in_size, 512), nn.GELU() if act.lower() == 'gelu' else nn.ReLU()]
        if dropout:
            embed += [nn.Dropout(dropout)]
        self.rrt = rrt if rrt is not None else nn.Identity()
        self.embed = nn.Sequential(*embed)
        self._act = _lib.ACT_GELU if act.lower() == 'gelu' else _lib.ACT_RELU

    def forward(self, feats):
        return self.rrt(self.embed(feats))


class Dattention_ori(BagHead, nn.Module):
    """modules/attmil_ibmil.py:44-102.  ``confounder_path``: one ``.npy`` path or a list of them (each reshaped to
    (-1, 512) and concatenated; at most 64 confounders in all), or False.  ``forward(x)`` returns the logits (1, out_dim)."""
    _POOL = _lib.BAGPOOL_ATTN_DECONF
    _NAME = "IBMIL"

    def __init__(self, out_dim=2, in_size=1024, dropout=0.25, confounder_path=False, **kwargs):
        super().__init__()
        self.L, self.D, self.K = 512, 128, 1
        self.embedding = FCLayer(in_size=in_size, dropout=dropout, **kwargs)
        self.attention = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh(), nn.Linear(self.D, self.K))
        self.head = nn.Linear(512, out_dim)
        self.confounder_path = confounder_path
        if confounder_path:
            paths = confounder_path if isinstance(confounder_path, list) else [confounder_path]
            conf_tensor = torch.cat([torch.from_numpy(np.load(i)).view(-1, 512).float() for i in paths], 0)
            conf_tensor_dim = conf_tensor.shape[-1]
            self.register_buffer("confounder_feat", conf_tensor)
            joint_space_dim = 128
            self.W_q = nn.Linear(512, joint_space_dim)
            self.W_k = nn.Linear(conf_tensor_dim, joint_space_dim)
            self.head = nn.Linear(self.L * self.K + conf_tensor_dim, out_dim)
            self.dropout = nn.Dropout(0.5)          # (never applied, attmil_ibmil.py:77)
        self.apply(initialize_weights)
        self._emb_act = self.embedding._act
        self._ws = None

    def _front(self):
        from .encoder import RRTEncoder
        mods = list(self.embedding.embed)
        return mods + [self.embedding.rrt] if isinstance(self.embedding.rrt, RRTEncoder) else mods

    def _classifier(self):
        return self.head

    def _check_call(self, n):
        if n == 1:
            raise ValueError("IBMIL: a bag of one instance cannot run -- the reference's x.squeeze() drops the bag axis there "
                             "(modules/attmil_ibmil.py:82) and its torch.mm fails")

    def _fill(self, d, w, p):
        a, c = self.attention[0], self.attention[2]
        d.pool_hidden, d.pool_act = self.D, _lib.ACT_TANH
        w.a_w, w.a_b, w.c_w, w.c_b = p(a.weight), p(a.bias), p(c.weight), p(c.bias)
        if not self.confounder_path:
            d.pool = _lib.BAGPOOL_ATTN          # the plain head: the classifier sits in the pool's merge block
            return
        conf = self.confounder_feat
        d.deconf_k, d.deconf_v, d.deconf_j = conf.shape[0], conf.shape[1], self.W_q.out_features
        w.conf = p(conf)
        w.q_w, w.q_b, w.k_w, w.k_b = p(self.W_q.weight), p(self.W_q.bias), p(self.W_k.weight), p(self.W_k.bias)

    def _tail(self, y, no_norm, compute):
        pooled, attn, a_raw = attn_tail(self, y, list(self.attention)[:2], None, self.attention[2], compute)
        x = pooled.unsqueeze(0)
        if self.confounder_path:                     # attmil_ibmil.py:90-99 on [1, .] / [K, .] device tensors
            bag_q = self.W_q(x)
            conf_k = self.W_k(self.confounder_feat)
            deconf_A = F.softmax(torch.mm(conf_k, bag_q.transpose(0, 1)) / math.sqrt(conf_k.shape[1]), 0)
            x = torch.cat((x, torch.mm(deconf_A.transpose(0, 1), self.confounder_feat)), dim=1)
        return self.head(x), (a_raw if no_norm else attn)

    def forward(self, x):
        return self._run(x)[0]


IBMIL = Dattention_ori
