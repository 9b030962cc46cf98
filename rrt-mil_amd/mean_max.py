"""MeanMIL and MaxMIL -- the reference's ``--model meanmil`` / ``--model maxmil`` heads (modules/mean_max.py) around the
MI355X encoder: one ``head`` ``nn.Sequential`` -- Linear + activation (+ Dropout) (+ ``rrt``) + the classifier Linear -- whose
per-instance scores are averaged / maximised over the bag.

Same constructors, the same ``head`` layout (the indices of ``rrt`` and of the classifier move with ``act`` / ``dropout`` /
``rrt``), the same parameter names: reference checkpoints load with ``strict=True``.

Tails (fp32 in every compute mode -- a 16-bit instance score could select another instance):
  * mean: the mean commutes with the classifier, logits = W colmean(y) + b -- ONE pass over y, [N, C] never exists
    (csrc/bag_pool.hip rrt_bag_mean_f32; `_BagMean` with a graph);
  * max: rrt_instance_max_f32, the DSMIL instance stream (among equal scores the lowest index; a NaN score is never
    selected; `_InstanceMax` with its sparse adjoint with a graph).
In ``eval()`` without a graph a bag is ONE C-ABI call (rrt_bagmil_forward_f32).

The reference's quirk, kept: ``MaxMIL`` hard-codes ``Linear(1024, 512)`` whatever ``input_dim`` says.  ``forward(x)`` takes
one bag, (1, N, input_dim) or (N, input_dim), and returns the logits (1, n_classes).
"""
from torch import nn

from . import _lib
from ._head import BagHead, _BagMean, _InstanceMax
from .attmil import initialize_weights  # noqa: F401  (modules/mean_max.py:3-22 is the same rule)


class _ScoreHead(BagHead, nn.Module):
    def _build(self, in_features, n_classes, dropout, act, rrt):
        self._check_rrt(rrt)
        head = [nn.Linear(in_features, 512)]
        if act.lower() == 'relu':
            head += [nn.ReLU()]
        elif act.lower() == 'gelu':
            head += [nn.GELU()]
        if dropout:
            head += [nn.Dropout(0.25)]
        if rrt is not None:
            head += [rrt]
        head += [nn.Linear(512, n_classes)]
        self.head = nn.Sequential(*head)
        self.apply(initialize_weights)
        self._emb_act = {"relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU}.get(act.lower(), _lib.ACT_NONE)
        self._ws = None

    def _front(self):
        return list(self.head)[:-1]

    def _classifier(self):
        return self.head[-1]

    def _fill(self, d, w, p):
        pass

    def forward(self, x):
        return self._run(x)[0]


class MeanMIL(_ScoreHead):
    """modules/mean_max.py:25-52"""
    _POOL = _lib.BAGPOOL_MEAN
    _NAME = "MeanMIL"

    def __init__(self, input_dim, n_classes=1, dropout=True, act='relu', rrt=None):
        super().__init__()
        self._build(input_dim, n_classes, dropout, act, rrt)

    def _tail(self, y, no_norm, compute):
        cls = self._classifier()
        return _BagMean.apply(y, cls.weight, cls.bias).unsqueeze(0), None


class MaxMIL(_ScoreHead):
    """modules/mean_max.py:56-79"""
    _POOL = _lib.BAGPOOL_MAX
    _NAME = "MaxMIL"

    def __init__(self, input_dim, n_classes=1, dropout=True, act='relu', rrt=None):
        super().__init__()
        self._build(1024, n_classes, dropout, act, rrt)

    def _tail(self, y, no_norm, compute):
        cls = self._classifier()
        return _InstanceMax.apply(y, cls.weight, cls.bias)[0].unsqueeze(0), None
