"""f64 numpy restatement of clipk_linear_ce_fwd / clipk_linear_ce_bwd (include/clipk.h): the definition the kernels are
tested against, including the out-of-range-label rule and the tie rule.  tests/test_classifier_host.py checks it against
torch.nn.functional.cross_entropy and autograd in f64."""
import numpy as np


def _cat(x1, x2):
    x1 = np.asarray(x1, np.float64)
    return x1 if x2 is None else np.concatenate([x1, np.asarray(x2, np.float64)], axis=1)


def logits(x1, w, bias=None, x2=None):
    z = _cat(x1, x2) @ np.asarray(w, np.float64).T
    return z if bias is None else z + np.asarray(bias, np.float64)


def abs_logits(x1, w, bias=None, x2=None):
    """sum_k |x_k w_k| + |b|: what the rounding error of a logit is relative to."""
    a = np.abs(_cat(x1, x2)) @ np.abs(np.asarray(w, np.float64)).T
    return a if bias is None else a + np.abs(np.asarray(bias, np.float64))


def first_argmax(z):
    """First-occurrence argmax per row: equal logits resolve to the lower class (np.argmax's rule, torch.max's too)."""
    return np.argmax(z, axis=1).astype(np.int64)


def fwd(x1, w, bias, labels, x2=None):
    """(lse, tgt, pred, Z).  tgt is NaN where the label is outside [0, C)."""
    z = logits(x1, w, bias, x2)
    M, C = z.shape
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    labels = np.asarray(labels, np.int64)
    ok = (labels >= 0) & (labels < C)
    tgt = np.full(M, np.nan)
    tgt[ok] = z[np.nonzero(ok)[0], labels[ok]]
    return lse, tgt, first_argmax(z), z


def grad_logits(z, lse, labels, g=1.0):
    """G[i, c] = g / M (exp(Z - lse) - onehot); rows whose label is outside [0, C) are zero (1 / M keeps the full M)."""
    M, C = z.shape
    labels = np.asarray(labels, np.int64)
    ok = (labels >= 0) & (labels < C)
    G = np.exp(z - np.asarray(lse, np.float64)[:, None])
    G[np.nonzero(ok)[0], labels[ok]] -= 1.0
    G[~ok] = 0.0
    return G * (float(g) / M)


def bwd(x1, w, bias, labels, g=1.0, x2=None, lse=None):
    """(dW, dbias, dX1, dX2 or None, G)."""
    lse_ref, _, _, z = fwd(x1, w, bias, labels, x2)
    G = grad_logits(z, lse_ref if lse is None else lse, labels, g)
    x = _cat(x1, x2)
    K1 = np.asarray(x1).shape[1]
    dx = G @ np.asarray(w, np.float64)
    return G.T @ x, G.sum(axis=0), dx[:, :K1], (None if x2 is None else dx[:, K1:]), G


def mean_loss(lse, tgt):
    return float(np.sum(np.asarray(lse, np.float64) - np.asarray(tgt, np.float64)) / len(lse))
