"""Downstream classifier probes on frozen CLIP embeddings: the four heads of the reference's old/classifier.py with its
constructor signatures, defaults and state_dict keys (a reference checkpoint loads), on the exact-f32 HIP kernels.

Every head ends in nn.Linear(h, num_classes) under nn.CrossEntropyLoss (old/ablation.py:30).  Three entry points:
  forward(x)                          the logits - the reference's API (old/classifier.py:17,28,39,50)
  loss(x, labels, x2=None, ...)       the fused Linear + cross-entropy (clipk_linear_ce_*; more than 64 classes: the
                                      class-tiled clipk_linear_ce_tiled_*): the logits never exist
  predict(x, x2=None)                 the first-occurrence argmax of every row (torch.max(logits, 1) of ablation.py:46)
x2: a second input whose columns follow x's - torch.cat([rna_embeds, protein_embeds], -1) of old/ablation.py:29,44.
LinearClassifier, whose first layer is the fused one, reads the two sources in place; the other heads make the one
torch.cat (a two-source first Linear does not fall out of clipk_gemm_f32: it takes one A operand).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import functional as KF
from . import ops


def _seeds(n: int):
    """32-bit dropout seeds from torch's default CPU generator (torch.manual_seed() makes a run reproducible)."""
    return torch.randint(0, 2 ** 31 - 1, (n,), dtype=torch.int64).tolist()


def _wide(last: nn.Linear) -> bool:
    """More classes than clipk_linear_ce_* take: the class-tiled kernels (narrower heads keep the kernels they had)."""
    return last.out_features > ops.LINEAR_CE_MAX_CLASSES


def _fused_loss(x, last, labels, x2=None, return_pred=False):
    fn = KF.linear_cross_entropy_tiled if _wide(last) else KF.linear_cross_entropy
    return fn(x, last.weight, last.bias, labels, x2=x2, return_pred=return_pred)


def _fused_pred(x, last, x2=None):
    if _wide(last):
        return ops.linear_ce_tiled_fwd(x, last.weight, last.bias, x2=x2)[2]
    return ops.linear_ce_fwd(x, last.weight, last.bias, x2=x2)[2]


def _rows(x, x2=None):
    if x2 is not None:
        x = torch.cat([x, x2], dim=-1)
    return x.float().contiguous()


class _Head(nn.Module):
    """features(x) -> the input of the last Linear; `_last` names that Linear."""

    def _last(self) -> nn.Linear:
        raise NotImplementedError

    def features(self, x):
        raise NotImplementedError

    def forward(self, x):
        last = self._last()
        return KF.linear_f32(self.features(_rows(x)), last.weight, last.bias)

    def loss(self, x, labels, x2=None, return_pred=False):
        """Mean cross-entropy of the head's logits against integer `labels` [M] (and the detached predictions)."""
        return _fused_loss(self.features(_rows(x, x2)), self._last(), labels, return_pred=return_pred)

    @torch.no_grad()
    def predict(self, x, x2=None):
        return _fused_pred(self.features(_rows(x, x2)), self._last())


class MLPClassifier(_Head):
    """old/classifier.py:5-18: Linear (+ ReLU + Dropout) per hidden width, then Linear."""

    def __init__(self, input_dim, hidden_dims, output_dim, dropout_rate=0.1):
        super().__init__()
        layers = []
        dims = [input_dim] + list(hidden_dims) + [output_dim]
        for i in range(len(dims) - 1):
            layers.append(nn.Linear(dims[i], dims[i + 1]))
            if i < len(dims) - 2:
                layers.append(nn.ReLU())
                layers.append(nn.Dropout(dropout_rate))
        self.mlp = nn.Sequential(*layers)
        self.dropout_rate = float(dropout_rate)

    def _last(self):
        return self.mlp[-1]

    def features(self, x):
        linears = [m for m in self.mlp if isinstance(m, nn.Linear)][:-1]
        drop = self.training and self.dropout_rate > 0.0
        seeds = _seeds(len(linears)) if drop else None
        for i, lin in enumerate(linears):
            x = KF.ActFn.apply(KF.linear_f32(x, lin.weight, lin.bias), "relu")
            if drop:
                x = KF.dropout_f32(x, (self.dropout_rate, seeds[i]))
        return x


class TransformerClassifier(_Head):
    """old/classifier.py:20-32.  The reference feeds x.unsqueeze(0) to batch-second encoder layers: sequence length 1,
    every row attends to itself alone and its softmax weight is exactly 1, so the attention block is
    out_proj(v_proj(x)) with the V rows of in_proj_weight.  The q / k rows stay in the state dict and receive exact zero
    gradients (slices of one Parameter), as torch's autograd gives them.  Post-LN residual, ReLU FFN (2048), post-LN.
    In train() mode the attention-probability dropout acts on that single weight: one keep / (1 - p) factor per row and
    head."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers, num_heads, dropout_rate=0.1):
        super().__init__()
        self.input_projection = nn.Linear(input_dim, hidden_dim)
        encoder_layer = nn.TransformerEncoderLayer(d_model=hidden_dim, nhead=num_heads, dropout=dropout_rate)
        self.transformer_encoder = nn.TransformerEncoder(encoder_layer, num_layers=num_layers, enable_nested_tensor=False)
        self.output_projection = nn.Linear(hidden_dim, output_dim)
        self.hidden_dim, self.num_heads, self.dropout_rate = hidden_dim, num_heads, float(dropout_rate)

    def _last(self):
        return self.output_projection

    def features(self, x):
        E, H = self.hidden_dim, self.num_heads
        p = self.dropout_rate
        drop = self.training and p > 0.0
        h = KF.linear_f32(x, self.input_projection.weight, self.input_projection.bias)
        M = h.shape[0]
        for l in self.transformer_encoder.layers:
            a = l.self_attn
            sd = _seeds(4) if drop else None
            v = KF.linear_f32(h, a.in_proj_weight[2 * E:], a.in_proj_bias[2 * E:])
            if drop:
                keep = KF.dropout_f32(torch.ones((M, H), dtype=torch.float32, device=h.device), (p, sd[0]))
                v = (v.view(M, H, E // H) * keep.unsqueeze(-1)).reshape(M, E)
                s1 = KF.dropout_f32(KF.linear_f32(v, a.out_proj.weight, a.out_proj.bias), (p, sd[1]), addend=h)
            else:
                s1 = KF.linear_f32(v, a.out_proj.weight, a.out_proj.bias, addend=h)
            x1 = KF.layer_norm(s1, l.norm1.weight, l.norm1.bias, l.norm1.eps)
            g = KF.ActFn.apply(KF.linear_f32(x1, l.linear1.weight, l.linear1.bias), "relu")
            if drop:
                g = KF.dropout_f32(g, (p, sd[2]))
                s2 = KF.dropout_f32(KF.linear_f32(g, l.linear2.weight, l.linear2.bias), (p, sd[3]), addend=x1)
            else:
                s2 = KF.linear_f32(g, l.linear2.weight, l.linear2.bias, addend=x1)
            h = KF.layer_norm(s2, l.norm2.weight, l.norm2.bias, l.norm2.eps)
        return h


class LinearClassifier(_Head):
    """old/classifier.py:34-40: one Linear - the fused kernel is the whole head, and reads x and x2 in place."""

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.linear = nn.Linear(input_dim, output_dim)

    def _last(self):
        return self.linear

    def features(self, x):
        return x

    def loss(self, x, labels, x2=None, return_pred=False):
        x2 = None if x2 is None else x2.float().contiguous()
        return _fused_loss(x.float().contiguous(), self.linear, labels, x2=x2, return_pred=return_pred)

    @torch.no_grad()
    def predict(self, x, x2=None):
        x2 = None if x2 is None else x2.float().contiguous()
        return _fused_pred(x.float().contiguous(), self.linear, x2=x2)


class SimpleNonLinearClassifier(_Head):
    """old/classifier.py:42-54: Linear, ReLU, LayerNorm, Dropout, Linear."""

    def __init__(self, input_dim, hidden_dim, output_dim, dropout_rate=0.1):
        super().__init__()
        self.layer1 = nn.Linear(input_dim, hidden_dim)
        self.layer2 = nn.Linear(hidden_dim, output_dim)
        self.dropout = nn.Dropout(dropout_rate)
        self.norm = nn.LayerNorm(hidden_dim)
        self.dropout_rate = float(dropout_rate)

    def _last(self):
        return self.layer2

    def features(self, x):
        x = KF.ActFn.apply(KF.linear_f32(x, self.layer1.weight, self.layer1.bias), "relu")
        x = KF.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        if self.training and self.dropout_rate > 0.0:
            x = KF.dropout_f32(x, (self.dropout_rate, _seeds(1)[0]))
        return x
