"""Argument checks and small preparations shared by the embedding-cloud wrappers of ops.py and the analysis modules
on top of them (cluster, manifold, neighbors, mixing, diffusion).  Plain functions; every one raises before any device
work.  Nothing here needs the library or a device."""
from __future__ import annotations

import math

import torch


def int_in(name, value, lo, hi=None, what=None, optional=False, type_error=False):
    """`value` is an int - a bool is none - in [lo, hi] (hi=None: no upper end; optional: or None), else ValueError
    "<name> must be <what>, got <value>".  what: how the message words the range; by default "a positive int" (lo 1),
    "an int >= lo" or "an int in [lo, hi]", after "None or " with optional.  type_error: a value that is no int raises
    TypeError "<name> must be an int, got <value>" first, for the callers that tell the two faults apart."""
    if optional and value is None:
        return
    if what is None:
        what = ("a positive int" if lo == 1 else f"an int >= {lo}") if hi is None else f"an int in [{lo}, {hi}]"
        if optional:
            what = "None or " + what
    is_int = isinstance(value, int) and not isinstance(value, bool)
    if type_error and not is_int:
        raise TypeError(f"{name} must be an int, got {value!r}")
    if not is_int or value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name} must be {what}, got {value!r}")


def check_metric(metric, metrics):
    if metric not in metrics:
        raise ValueError(f"metric must be one of {metrics}, got {metric!r}")


def need_device(who, *ts):
    """Every tensor given (None: an optional one left out) is on the device, else ValueError "<who> device tensors
    (there is no CPU fallback)"; who: the caller's subject and verb."""
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError(f"{who} device tensors (there is no CPU fallback)")


def check_cloud(x, name="x", min_rows=1, max_width=None):
    """x is a 2-D float32 tensor of at least min_rows rows whose width is a multiple of 4, at most max_width (None: the
    kNN search, which has no limit and words emptiness and width as one fault)."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a float32 device tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError(f"{name} must be a 2-D tensor, got shape {tuple(x.shape)}")
    N, P = x.shape
    if max_width is None:
        if N == 0 or P == 0 or P % 4:
            raise ValueError(f"{name} must be non-empty with a width that is a multiple of 4, got shape {tuple(x.shape)}")
        return
    if N < min_rows:
        raise ValueError(f"at least {min_rows} rows, got {N}")
    if P == 0 or P % 4 or P > max_width:
        raise ValueError(f"the width must be a multiple of 4 and at most {max_width}, got {P}")


def labels_arg(name, t, rows=None):
    """An integer annotation [n] as an int64 vector; rows: the n it must have."""
    if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise TypeError(f"{name} must be an integer tensor")
    if t.dim() != 1:
        raise ValueError(f"{name} must be 1-D, got shape {tuple(t.shape)}")
    if rows is not None and t.shape[0] != rows:
        raise ValueError(f"{name} has {t.shape[0]} entries for {rows} rows")
    return t.long()


def prepare(x, metric, half=True):
    """The cloud detached and contiguous; metric "cosine": its rows L2-normalised, and with half scaled by 1 / sqrt 2, so
    that their squared distances are 1 - cos."""
    x = x.detach().contiguous()
    if metric != "cosine":
        return x
    x = torch.nn.functional.normalize(x, dim=1)
    return x * math.sqrt(0.5) if half else x


def generator_for(generator, device):
    """A generator on `device`: the one given, or one seeded by a draw from it when it lives elsewhere (a host
    generator with a device cloud) - a host-side draw, nothing is read back from the device."""
    if generator is None or generator.device.type == torch.device(device).type:
        return generator
    seed = int(torch.randint(2 ** 62, (1,), generator=generator, device=generator.device))
    return torch.Generator(device=device).manual_seed(seed)
