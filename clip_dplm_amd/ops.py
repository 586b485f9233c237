"""Thin tensor-level wrappers over the libclipk C ABI (no autograd here, no fallbacks).

Every function enqueues HIP kernels on torch's current stream and returns torch tensors that own the
output memory.  Inputs must live on a CUDA(HIP) device; anything else raises.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _args, _ffi
from ._ffi import ACT, BF16, F32, U8, GemmArgs, check, ptr

_WS: dict = {}


class KernelTimer:
    """Optional HIP-event timing of individual kernel launches on torch's current stream (the stream the
    kernels are enqueued on).  bench.py uses it for the live roofline numbers; off by default."""

    def __init__(self, only=None):
        self.records = {}          # name -> list of (start_event, end_event, algorithmic work)
        self.only = None if only is None else set(only)    # restrict to these kernel names (two events per launch cost
                                                           # ~1 % of a training step when every launch is timed)

    def add(self, name, s, e, work, nbytes=0.0, sub=None):
        self.records.setdefault(name, []).append((s, e, work, nbytes, sub))

    def summary_by_sub(self, name):
        """The launches of kernel `name` grouped by their sub-tag (gemm_nt: the epilogue mode) -> same fields as
        summary().  Call after torch.cuda.synchronize()."""
        groups = {}
        for r in self.records.get(name, []):
            groups.setdefault(r[4] or "-", []).append(r)
        out = {}
        for sub, recs in groups.items():
            ms = sum(r[0].elapsed_time(r[1]) for r in recs)
            out[sub] = {"launches": len(recs), "total_ms": ms, "avg_us": 1e3 * ms / max(len(recs), 1),
                        "work": float(sum(r[2] for r in recs)), "bytes": float(sum(r[3] for r in recs))}
        return out

    def summary(self):
        """name -> dict(launches, total_ms, avg_us, work) — call after torch.cuda.synchronize()."""
        out = {}
        for name, recs in self.records.items():
            ms = sum(r[0].elapsed_time(r[1]) for r in recs)
            out[name] = {"launches": len(recs), "total_ms": ms, "avg_us": 1e3 * ms / max(len(recs), 1),
                         "work": float(sum(r[2] for r in recs)), "bytes": float(sum(r[3] for r in recs))}
        return out


_TIMER: Optional[KernelTimer] = None


def set_kernel_timer(t: Optional[KernelTimer]) -> None:
    global _TIMER
    _TIMER = t


def _timed(name: str, work: float, fn, nbytes: float = 0.0, sub=None):
    if _TIMER is None or (_TIMER.only is not None and name not in _TIMER.only):
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = fn()
    e.record()
    _TIMER.add(name, s, e, work, nbytes, sub)
    return r


def _lib():
    return _ffi.load()


def set_option(name: str, value: int) -> None:
    """Kernel-selection option of libclipk (include/clipk.h: clipk_set_option).  Results never depend on options."""
    check(_lib().clipk_set_option(name.encode(), int(value)), f"clipk_set_option({name})")


def get_option(name: str) -> int:
    v = C.c_int(0)
    check(_lib().clipk_get_option(name.encode(), C.byref(v)), f"clipk_get_option({name})")
    return v.value


def reset_options() -> None:
    check(_lib().clipk_reset_options(), "clipk_reset_options")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported dtype {t.dtype}")


def _need_cuda(*ts):
    """Every tensor on the GPU, and on the CURRENT one: the kernels are enqueued on the current device's stream, so a
    tensor of another device would be read through a foreign pointer.  Fails loudly instead."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _ffi.ClipkError("libclipk kernels need device tensors (there is no CPU fallback)")
        if dev is None:
            dev = t.device
            if dev.index is not None and dev.index != torch.cuda.current_device():
                raise _ffi.ClipkError(f"tensor on {dev} but the current device is cuda:{torch.cuda.current_device()}: "
                                      "wrap the call in `with torch.cuda.device(tensor.device):`")
        elif t.device != dev:
            raise _ffi.ClipkError(f"tensors on different devices: {dev} and {t.device}")


# hipGraph capture (training.GraphedTrainStep, icnn.GraphedTransport): a captured launch holds the raw pointers of the
# host-cached buffers it was given - workspaces, descriptor tables - and the caches below replace (grow) or clear them
# later.  A buffer the eager warm-up allocated (the model's persistent branch streams: same cache key in warm-up, capture
# and later eager calls) would then go back to the caching allocator while replays still write into it.  While a
# capture is open every such buffer handed out is also appended to the list of the graph object that captures
# (`owned_by_capture`): the cache may drop its reference, the memory lives as long as the graph.
_CAPTURE_KEEP: Optional[list] = None


class owned_by_capture:
    """`with ops.owned_by_capture(keep): with torch.cuda.graph(g): ...` - `keep` (a list the graph's owner holds for the
    graph's lifetime) receives every cached buffer handed out to a capturing stream meanwhile."""

    def __init__(self, keep: list):
        self.keep = keep

    def __enter__(self):
        global _CAPTURE_KEEP
        self._prev, _CAPTURE_KEEP = _CAPTURE_KEEP, self.keep
        return self.keep

    def __exit__(self, *exc):
        global _CAPTURE_KEEP
        _CAPTURE_KEEP = self._prev
        return False


def keep_for_capture(t: torch.Tensor) -> torch.Tensor:
    """Register a host-cached buffer with the open capture, if the current stream is capturing (branch streams forked
    into the capture included).  Returns t."""
    if _CAPTURE_KEEP is not None and torch.cuda.is_current_stream_capturing():
        _CAPTURE_KEEP.append(t)
    return t


def workspace(nbytes: int, device, tag: str = "ws", stream: Optional[int] = None) -> torch.Tensor:
    """Grow-only per-(device, stream, tag) scratch buffer (kernels never allocate).  stream: the current stream's handle
    where the caller has fetched it already."""
    key = (str(device), _stream() if stream is None else stream, tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 16), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return keep_for_capture(buf)


# --------------------------------------------------------------------------------------------------
def gemm_nt(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, act=None,
            out_dtype=torch.bfloat16, residual: Optional[torch.Tensor] = None, out_preact: bool = False,
            dact_aux: Optional[torch.Tensor] = None, dact=None, alpha: float = 1.0,
            out: Optional[torch.Tensor] = None, dropout=None, rope=None, aux_u8: bool = False,
            rope_interleaved: bool = False):
    """C = epilogue(a[M,K] @ b[N,K]^T) with a, b bf16.  Returns C (and the bf16 pre-activation if asked).
    aux_u8 (act = "gelu", out_preact): the second output is GELU'(pre-activation) as 8-bit codes (uint8 [M, N]) instead of
    the bf16 pre-activation; a uint8 `dact_aux` (dact = "gelu") is read as such codes (clipk.h aux_dtype).
    dropout = (p, seed): nn.Dropout on the value after the activation (before act'(aux) and the residual add).
    rope = (cos, sin, L, hd, cols): rotate-half RoPE (tables f32 [L, hd/2], position = row mod L) on the first `cols`
    output columns in the epilogue (ESM-2's fused qkv projection: cols = 2 * hidden).  rope_interleaved: those columns'
    heads are in pair-interleaved order (b's rows permuted by cast_transpose(il=...)): partners are neighbours, any hd % 8 == 0."""
    _need_cuda(a, b, bias, residual, dact_aux, *(rope[:2] if rope else ()))
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1]
    assert a.stride(1) == 1 and b.stride(1) == 1
    M, K = a.shape
    N = b.shape[0]
    c = out if out is not None else torch.empty((M, N), dtype=out_dtype, device=a.device)
    aux8 = bool(aux_u8 and out_preact) or (dact_aux is not None and dact_aux.dtype == torch.uint8)
    if aux8:
        assert (act == "gelu" or not out_preact) and (dact == "gelu" or dact_aux is None), "8-bit aux: GELU only"
        assert dact_aux is None or dact_aux.dtype == torch.uint8
    pre = torch.empty((M, N), dtype=torch.uint8 if aux8 else torch.bfloat16, device=a.device) if out_preact else None
    args = GemmArgs()
    args.A, args.lda = a.data_ptr(), a.stride(0)
    args.B, args.ldb = b.data_ptr(), b.stride(0)
    args.C, args.ldc, args.c_dtype = c.data_ptr(), c.stride(0), _dt(c)
    args.M, args.N, args.K = M, N, K
    args.bias = ptr(bias)
    args.act = ACT[act]
    args.out_preact, args.ldp = ptr(pre), (pre.stride(0) if pre is not None else 0)
    args.dact_aux, args.ldd = ptr(dact_aux), (dact_aux.stride(0) if dact_aux is not None else 0)
    args.dact = ACT[dact]
    if residual is not None:
        args.residual, args.ldr, args.r_dtype = residual.data_ptr(), residual.stride(0), _dt(residual)
    else:
        args.residual, args.ldr, args.r_dtype = None, 0, 0
    args.alpha = alpha
    args.aux_dtype = U8 if aux8 else BF16
    args.drop_p, args.drop_seed = (float(dropout[0]), int(dropout[1]) & 0xFFFFFFFF) if dropout else (0.0, 0)
    if rope is not None:
        cos, sin, rl, hd, cols = rope
        assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
        assert cos.shape == (rl, hd // 2) and sin.shape == (rl, hd // 2)
        args.rope_cos, args.rope_sin = cos.data_ptr(), sin.data_ptr()
        args.rope_L, args.rope_hd, args.rope_cols, args.rope_row0 = int(rl), int(hd), int(cols), 0
        args.rope_interleaved = int(bool(rope_interleaved))
    else:
        args.rope_interleaved = 0
        args.rope_cos, args.rope_sin = None, None
        args.rope_L = args.rope_hd = args.rope_cols = args.rope_row0 = 0
    # algorithmic bytes: both operands once, every output / epilogue operand once
    nb = 2.0 * (M * K + N * K) + M * N * (c.element_size() + (pre.element_size() if out_preact else 0) +
                                          (dact_aux.element_size() if dact_aux is not None else 0)
                                          + (residual.element_size() if residual is not None else 0))
    sub = None
    if _TIMER is not None:                                   # epilogue mode of this launch (bench.py: per-mode rates)
        sub = ("dact_" + str(dact) + ("8" if aux8 else "") if dact_aux is not None else ("act_" + str(act) if act else "linear")) + \
              (("+dact8" if aux8 else "+preact") if out_preact else "") + ("+rope" if rope is not None else "") + \
              ("+res_" + ("f32" if residual.dtype == torch.float32 else "bf16") if residual is not None else "") + \
              ("+drop" if dropout else "") + ("->f32" if c.dtype == torch.float32 else "->bf16")
    check(_timed("gemm_nt", 2.0 * M * N * K, lambda: _lib().clipk_gemm_nt(C.byref(args), _stream()), nb, sub),
          "clipk_gemm_nt")
    return (c, pre) if out_preact else c


def gelu_aux_u8_applies(k_in: int, n_ffn: int) -> bool:
    """Shapes for which the 8-bit GELU' code can be the FFN pair's saved operand: the specialised epilogues need the
    LDS-DMA main loop (K % 32 == 0; the generic-K kernel returns CLIPK_ERR_UNSUPPORTED for CLIPK_U8, gemm_nt.hip) and
    code rows of whole 8-byte chunks (ldp / ldd % 8 == 0).  Both GEMMs of the pair - fc1 forward [M, n_ffn] and the
    fc2 input gradient [M, n_ffn] - contract over k_in = the model width.  Other widths (the notebook's 120) keep the
    bf16 pre-activation."""
    return k_in % 32 == 0 and n_ffn % 8 == 0


def gemm_wgrad(dy: torch.Tensor, x: torch.Tensor, dw: Optional[torch.Tensor] = None,
               dbias: Optional[torch.Tensor] = None, accumulate: bool = False, want_bias: bool = False, il=(0, 0)):
    """dW[N,K] (+)= dy[M,N]^T @ x[M,K] (f32), optionally db[N] = colsum(dy).  il = (head columns, il_cols): dy's first
    il_cols columns are in pair-interleaved head order; dW / db come out in the original order (clipk.h)."""
    _need_cuda(dy, x)
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
    M, N = dy.shape
    K = x.shape[1]
    if dw is None:
        dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
        accumulate = False
    if want_bias and dbias is None:
        dbias = torch.empty((N,), dtype=torch.float32, device=dy.device)
    lib = _lib()
    nbytes = lib.clipk_gemm_wgrad_workspace(M, N, K)
    ws = workspace(nbytes, dy.device, "wgrad")
    check(_timed("gemm_wgrad", 2.0 * M * N * K,
                 lambda: lib.clipk_gemm_wgrad(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(),
                                              dw.stride(0), ptr(dbias), M, N, K, int(accumulate), int(il[0]), int(il[1]),
                                              ws.data_ptr(), ws.numel(), _stream())), "clipk_gemm_wgrad")
    return dw, dbias


# --------------------------------------------------------------------------------------------------
# kind -> (the entry point that sizes its workspace, its name in error messages)
_SIMCE_KINDS = {"plain": ("clipk_simce_workspace", "simce"),
                "cls": ("clipk_simce_cls_workspace", "simce (class-aware)"),
                "hard": ("clipk_simce_hard_workspace", "simce (hard-negative)")}


def _simce(entry, kind, x, y, scale, cache, args, outs):
    """The body the six simce wrappers share, after each has checked its operands: shapes, outputs, workspace, the call.
    entry: the C entry point; kind: a key of _SIMCE_KINDS; args: the entry point's arguments between scale and the
    outputs; outs: (torch.empty or torch.zeros, shape) per f32 output.  Returns the outputs."""
    Mx, P = x.shape
    Ny = y.shape[0]
    Nc = 0 if cache is None else cache.shape[0]
    dev = x.device
    res = [new(*shape, dtype=torch.float32, device=dev) for new, shape in outs]      # sizes unpacked: cheaper to parse
    lib = _lib()
    ws_entry, what = _SIMCE_KINDS[kind]
    nbytes = getattr(lib, ws_entry)(Mx, Ny + Nc, P)
    if nbytes == 0:
        raise _ffi.ClipkError(f"{what}: unsupported shape Mx={Mx} Nkeys={Ny + Nc} P={P}")
    stream = _stream()                                  # fetched once: for the workspace's key and for the launch
    ws = workspace(nbytes, dev, "simce", stream)
    check(getattr(lib, entry)(x.data_ptr(), Mx, y.data_ptr(), Ny, ptr(cache), Nc, P, scale.data_ptr(), *args,
                              *[t.data_ptr() for t in res], ws.data_ptr(), ws.numel(), stream), entry)
    return tuple(res)


def simce_lse(x, y, scale, label_offset=0, cache=None):
    """lse[i] = logsumexp_j scale*<x_i, keys_j>, pos[i] = scale*<x_i, y_{label_offset+i}>."""
    _need_cuda(x, y, scale, cache)
    assert x.dtype == torch.float32 and y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous()
    rows = (x.shape[0],)
    return _simce("clipk_simce_lse", "plain", x, y, scale, cache, (label_offset,),
                  ((torch.empty, rows), (torch.zeros, rows)))                       # lse, pos


def ce_combine(lse_r, pos_r, lse_c, pos_c, w_row, w_col, bg):
    """(w_row * sum(lse_r - pos_r) + w_col * sum(lse_c - pos_c)) / bg as a 0-d device tensor, one launch
    (lse_c = pos_c = None: the one-sided loss)."""
    _need_cuda(lse_r, pos_r, lse_c, pos_c)
    out = torch.empty((), dtype=torch.float32, device=lse_r.device)
    check(_lib().clipk_ce_combine(lse_r.data_ptr(), pos_r.data_ptr(), ptr(lse_c), ptr(pos_c), lse_r.numel(), float(w_row),
                                  float(w_col), float(bg), out.data_ptr(), _stream()), "clipk_ce_combine")
    return out


LINEAR_CE_MAX_CLASSES = 64           # clipk_linear_ce_*: a row's logits in at most four 16-class accumulator tiles
LINEAR_CE_TILED_MAX_CLASSES = 65536  # clipk_linear_ce_tiled_*: the classes walked in 64-class tiles


def _linear_ce_args(x, weight, bias, labels, x2, max_classes=LINEAR_CE_MAX_CLASSES):
    """Checks shared by linear_ce_fwd / linear_ce_bwd and their class-tiled siblings (ValueError: the caller's mistake;
    nothing is launched).  Label VALUES are not looked at - that would be a host sync; a label outside [0, C) makes the
    loss NaN (include/clipk.h).  max_classes: the class limit of the kernels the caller is about to run.
    Returns (M, K1, K2, C)."""
    for name, t in (("x", x), ("weight", weight), ("bias", bias), ("x2", x2)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"linear_ce: {name} must be float32, got {t.dtype}")
    if x.dim() != 2 or weight.dim() != 2 or (x2 is not None and (x2.dim() != 2 or x2.shape[0] != x.shape[0])):
        raise ValueError("linear_ce: x [M, K1], x2 [M, K2] and weight [C, K1 + K2] must be 2-D with the same M")
    M, K1 = x.shape
    K2 = 0 if x2 is None else x2.shape[1]
    C = weight.shape[0]
    if weight.shape[1] != K1 + K2 or (bias is not None and bias.shape != (C,)):
        raise ValueError(f"linear_ce: weight {tuple(weight.shape)} / bias do not fit inputs of {K1} + {K2} columns")
    if labels is not None:
        if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.dtype.is_complex:
            raise ValueError(f"linear_ce: labels must be an integer tensor, got {labels.dtype}")
        if labels.shape != (M,):
            raise ValueError(f"linear_ce: labels must have shape ({M},), got {tuple(labels.shape)}")
    devs = {t.device for t in (x, weight, bias, labels, x2) if t is not None}
    if len(devs) != 1:
        raise ValueError(f"linear_ce: tensors on different devices: {sorted(map(str, devs))}")
    if C > max_classes:
        raise ValueError(f"linear_ce: {C} classes; the fused kernel takes at most {max_classes}")
    if M < 1 or C < 1 or K1 < 1 or K1 % 4 or K2 % 4 or K1 + K2 > 4096:
        raise ValueError(f"linear_ce: K1 = {K1}, K2 = {K2} must be multiples of 4 with K1 + K2 <= 4096 (M = {M}, C = {C})")
    return M, K1, K2, C


def _linear_ce_prep(x, weight, bias, labels, x2, max_classes=LINEAR_CE_MAX_CLASSES):
    M, K1, K2, C = _linear_ce_args(x, weight, bias, labels, x2, max_classes)
    _need_cuda(x, weight, bias, labels, x2)
    x, weight = x.contiguous(), weight.contiguous()
    x2 = None if x2 is None or K2 == 0 else x2.contiguous()
    bias = None if bias is None else bias.contiguous()
    labels = None if labels is None else labels.to(torch.int64).contiguous()
    return (M, K1, K2 if x2 is not None else 0, C), x, weight, bias, labels, x2


def linear_ce_fwd(x, weight, bias=None, labels=None, x2=None, want_logits=False, want_stats=True):
    """One pass over [x | x2]: (lse [M], tgt [M] or None without labels, pred int64 [M], logits [M, C] or None) of
    Z = [x | x2] weight^T + bias (include/clipk.h: clipk_linear_ce_fwd).  want_stats=False: the logits alone."""
    (M, K1, K2, C), x, weight, bias, labels, x2 = _linear_ce_prep(x, weight, bias, labels, x2)
    dev = x.device
    lse = torch.empty(M, dtype=torch.float32, device=dev) if want_stats else None
    tgt = torch.empty(M, dtype=torch.float32, device=dev) if want_stats and labels is not None else None
    pred = torch.empty(M, dtype=torch.int64, device=dev) if want_stats else None
    logits = torch.empty((M, C), dtype=torch.float32, device=dev) if want_logits or not want_stats else None
    lib = _lib()
    check(_timed("linear_ce_fwd", 2.0 * M * C * (K1 + K2),
                 lambda: lib.clipk_linear_ce_fwd(x.data_ptr(), K1, ptr(x2), K2, weight.data_ptr(), ptr(bias), ptr(labels), M,
                                                 C, ptr(lse), ptr(tgt), ptr(pred), ptr(logits), C, _stream()),
                 4.0 * (M * (K1 + K2) + C * (K1 + K2))), "clipk_linear_ce_fwd")
    return lse, tgt, pred, logits


def _linear_ce_bwd(tiled, x, weight, bias, labels, lse, g, x2, dw, dbias, accumulate, want_w, want_bias, want_dx, want_dx2):
    """One body for linear_ce_bwd / linear_ce_tiled_bwd: the two C entries take the same arguments."""
    name = "linear_ce_tiled" if tiled else "linear_ce"
    (M, K1, K2, C), x, weight, bias, labels, x2 = _linear_ce_prep(
        x, weight, bias, labels, x2, LINEAR_CE_TILED_MAX_CLASSES if tiled else LINEAR_CE_MAX_CLASSES)
    _need_cuda(x, lse, g, dw, dbias)
    dev = x.device
    assert lse.dtype == torch.float32 and lse.shape == (M,) and lse.is_contiguous()
    assert g.dtype == torch.float32 and g.numel() == 1
    if dw is None and want_w:
        assert not accumulate, "accumulate with a new dw tensor"
        dw = torch.empty((C, K1 + K2), dtype=torch.float32, device=dev)
    if dbias is None and want_bias:
        assert not accumulate, "accumulate with a new dbias tensor"
        dbias = torch.empty(C, dtype=torch.float32, device=dev)
    assert dw is None or (dw.dtype == torch.float32 and dw.shape == (C, K1 + K2) and dw.is_contiguous())
    assert dbias is None or (dbias.dtype == torch.float32 and dbias.shape == (C,) and dbias.is_contiguous())
    dx = torch.empty((M, K1), dtype=torch.float32, device=dev) if want_dx else None
    dx2 = torch.empty((M, K2), dtype=torch.float32, device=dev) if want_dx2 and K2 else None
    if dw is None and dbias is None and dx is None and dx2 is None:
        return None, None, None, None
    lib = _lib()
    entry = lib.clipk_linear_ce_tiled_bwd if tiled else lib.clipk_linear_ce_bwd
    nws = (lib.clipk_linear_ce_tiled_workspace if tiled else lib.clipk_linear_ce_workspace)(M, K1, K2, C)
    ws = workspace(nws, dev, name)
    check(_timed(name + "_bwd", 4.0 * M * C * (K1 + K2),
                 lambda: entry(x.data_ptr(), K1, ptr(x2), K2, weight.data_ptr(), ptr(bias), labels.data_ptr(), M, C,
                               lse.data_ptr(), g.data_ptr(), int(bool(accumulate)), ptr(dw), ptr(dbias), ptr(dx), ptr(dx2),
                               ws.data_ptr(), ws.numel(), _stream()),
                 8.0 * M * (K1 + K2)), f"clipk_{name}_bwd")
    return dw, dbias, dx, dx2


def linear_ce_bwd(x, weight, bias, labels, lse, g, x2=None, dw=None, dbias=None, accumulate=False, want_w=True,
                  want_bias=True, want_dx=False, want_dx2=False):
    """Gradients of mean(lse - tgt) times the device scalar g (clipk_linear_ce_bwd).  dw / dbias: write (accumulate: add)
    into these tensors, e.g. the parameters' .grad; otherwise new tensors where want_w / want_bias.  Returns
    (dw, dbias, dx, dx2), None where not asked for."""
    return _linear_ce_bwd(False, x, weight, bias, labels, lse, g, x2, dw, dbias, accumulate, want_w, want_bias, want_dx,
                          want_dx2)


def linear_ce_tiled_fwd(x, weight, bias=None, labels=None, x2=None):
    """linear_ce_fwd for any class count up to 65536 (include/clipk.h: clipk_linear_ce_tiled_fwd): (lse [M], tgt [M] or None
    without labels, pred int64 [M]).  No logits output: head(x) serves them."""
    (M, K1, K2, C), x, weight, bias, labels, x2 = _linear_ce_prep(x, weight, bias, labels, x2, LINEAR_CE_TILED_MAX_CLASSES)
    dev = x.device
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    tgt = torch.empty(M, dtype=torch.float32, device=dev) if labels is not None else None
    pred = torch.empty(M, dtype=torch.int64, device=dev)
    lib = _lib()
    ws = workspace(lib.clipk_linear_ce_tiled_workspace(M, K1, K2, C), dev, "linear_ce_tiled")
    check(_timed("linear_ce_tiled_fwd", 2.0 * M * C * (K1 + K2),
                 lambda: lib.clipk_linear_ce_tiled_fwd(x.data_ptr(), K1, ptr(x2), K2, weight.data_ptr(), ptr(bias), ptr(labels),
                                                       M, C, lse.data_ptr(), ptr(tgt), pred.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), _stream()),
                 4.0 * (M * (K1 + K2) + C * (K1 + K2))), "clipk_linear_ce_tiled_fwd")
    return lse, tgt, pred


def linear_ce_tiled_bwd(x, weight, bias, labels, lse, g, x2=None, dw=None, dbias=None, accumulate=False, want_w=True,
                        want_bias=True, want_dx=False, want_dx2=False):
    """linear_ce_bwd for any class count up to 65536 (clipk_linear_ce_tiled_bwd): the same arguments and returns."""
    return _linear_ce_bwd(True, x, weight, bias, labels, lse, g, x2, dw, dbias, accumulate, want_w, want_bias, want_dx,
                          want_dx2)


def _grad_outs(x):
    return (torch.empty, x.shape), (torch.empty, x.shape[:1])               # dx, dscale partials


def simce_grad(x, y, scale, lse_x, lse_y, w_row, w_col, inv_bg, label_offset=0, cache=None, upstream=None):
    """upstream: 1-element device tensor multiplied into the gradient inside the kernel (the loss' grad_output)."""
    _need_cuda(x, y, scale, lse_x, lse_y, cache, upstream)
    return _simce("clipk_simce_grad_scaled", "plain", x, y, scale, cache,
                  (label_offset, lse_x.data_ptr(), lse_y.data_ptr(), float(w_row), float(w_col), float(inv_bg),
                   ptr(upstream)), _grad_outs(x))


def _cls_args(x, y, scale, cache, cls_x, cls_y, same_class, eps, vectors=()):
    """Shapes and dtypes of the class-aware passes' operands (the kernels read them as raw f32 / int64 arrays of these
    lengths): ValueError on anything else.  vectors: (name, tensor or None, length) of further f32 [length] inputs."""
    def f32(name, t, shape):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape}, got {t.dtype} "
                             f"{tuple(t.shape)}")
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError(f"x and y must be 2-D, got {tuple(x.shape)} and {tuple(y.shape)}")
    Mx, P = x.shape
    Ny = y.shape[0]
    f32("x", x, (Mx, P))
    f32("y", y, (Ny, P))
    if cache is not None:
        f32("cache", cache, (cache.shape[0], P))
    if scale.dtype != torch.float32 or scale.numel() != 1:
        raise ValueError(f"scale must be a 1-element float32 tensor, got {scale.dtype} {tuple(scale.shape)}")
    if (cls_x is None) != (cls_y is None):
        raise ValueError("cls_x and cls_y: both or neither")
    for name, t, n in (("cls_x", cls_x, Mx), ("cls_y", cls_y, Ny)):
        if t is not None and (t.dtype != torch.int64 or tuple(t.shape) != (n,) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int64 tensor of shape ({n},), got {t.dtype} {tuple(t.shape)}")
    for name, t, n in vectors:
        if t is not None:
            f32(name, t, (n,))
    if same_class not in _ffi.SAME_CLASS:
        raise ValueError(f"same_class must be one of {tuple(_ffi.SAME_CLASS)}, got {same_class!r}")
    if not 0.0 <= float(eps) < 1.0:
        raise ValueError(f"eps must be in [0, 1), got {eps}")


def simce_lse_cls(x, y, scale, cls_x=None, cls_y=None, same_class="mask", eps=0.0, label_offset=0, cache=None):
    """Class-aware LSE pass (include/clipk.h: clipk_simce_lse_cls): (lse, tgt, cnt), each f32 [Mx].  cls_x [Mx] /
    cls_y [Ny]: device int64 class ids, both or neither (None: all distinct); the cache rows carry no class."""
    _cls_args(x, y, scale, cache, cls_x, cls_y, same_class, eps)
    _need_cuda(x, y, scale, cache, cls_x, cls_y)
    return _simce("clipk_simce_lse_cls", "cls", x, y, scale, cache,
                  (label_offset, ptr(cls_x), ptr(cls_y), _ffi.SAME_CLASS[same_class], float(eps)),
                  ((torch.empty, (x.shape[0],)),) * 3)


def simce_grad_cls(x, y, scale, lse_x, lse_y, cnt_x, cnt_y, w_row, w_col, inv_bg, nkeys_y, cls_x=None, cls_y=None,
                   same_class="mask", eps=0.0, label_offset=0, cache=None, upstream=None):
    """Class-aware gradient pass (include/clipk.h: clipk_simce_grad_cls): (dx, dscale partials).  nkeys_y: the key
    count of the column direction (its rows' denominator before masking)."""
    _cls_args(x, y, scale, cache, cls_x, cls_y, same_class, eps,
              (("lse_x", lse_x, x.shape[0]), ("lse_y", lse_y, y.shape[0]), ("cnt_x", cnt_x, x.shape[0]),
               ("cnt_y", cnt_y, y.shape[0]), ("upstream", upstream, 1)))
    _need_cuda(x, y, scale, lse_x, lse_y, cnt_x, cnt_y, cls_x, cls_y, cache, upstream)
    return _simce("clipk_simce_grad_cls", "cls", x, y, scale, cache,
                  (label_offset, lse_x.data_ptr(), lse_y.data_ptr(), ptr(cnt_x), ptr(cnt_y), ptr(cls_x), ptr(cls_y),
                   _ffi.SAME_CLASS[same_class], float(eps), int(nkeys_y), float(w_row), float(w_col), float(inv_bg),
                   ptr(upstream)), _grad_outs(x))


def _hard_beta(beta) -> float:
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 <= float(beta) < float("inf"):
        raise ValueError(f"beta must be a finite number >= 0, got {beta!r}")
    return float(beta)


def simce_lse_hard(x, y, scale, beta, cls_x=None, cls_y=None, label_offset=0, cache=None):
    """Hard-negative-weighted LSE pass (include/clipk.h: clipk_simce_lse_hard): (lse_h, pos, coef); lse_h, pos f32
    [Mx], coef f32 [3, Mx] = (q, k1, k2), the per-row coefficients of simce_grad_hard.  cls_x [Mx] / cls_y [Ny]: device
    int64 class ids, both or neither (None: all distinct); same-class batch keys leave the negatives, cache rows never."""
    _cls_args(x, y, scale, cache, cls_x, cls_y, "mask", 0.0)
    beta = _hard_beta(beta)
    _need_cuda(x, y, scale, cache, cls_x, cls_y)
    Mx = x.shape[0]
    return _simce("clipk_simce_lse_hard", "hard", x, y, scale, cache, (beta, label_offset, ptr(cls_x), ptr(cls_y)),
                  ((torch.empty, (Mx,)), (torch.empty, (Mx,)), (torch.empty, (3, Mx))))


def simce_grad_hard(x, y, scale, beta, coef_x, coef_y, w_row, w_col, inv_bg, cls_x=None, cls_y=None, label_offset=0,
                    cache=None, upstream=None):
    """Hard-negative-weighted gradient pass (include/clipk.h: clipk_simce_grad_hard): (dx, dscale partials).  coef_x
    [3, Mx]: simce_lse_hard's coefficients of the rows; coef_y [3, Ny]: those of every batch key's own direction."""
    _cls_args(x, y, scale, cache, cls_x, cls_y, "mask", 0.0, (("upstream", upstream, 1),))
    beta = _hard_beta(beta)
    for name, t, n in (("coef_x", coef_x, x.shape[0]), ("coef_y", coef_y, y.shape[0])):
        if t.dtype != torch.float32 or tuple(t.shape) != (3, n) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape (3, {n}), got {t.dtype} "
                             f"{tuple(t.shape)}")
    _need_cuda(x, y, scale, coef_x, coef_y, cls_x, cls_y, cache, upstream)
    return _simce("clipk_simce_grad_hard", "hard", x, y, scale, cache,
                  (beta, label_offset, coef_x.data_ptr(), coef_y.data_ptr(), ptr(cls_x), ptr(cls_y), float(w_row),
                   float(w_col), float(inv_bg), ptr(upstream)), _grad_outs(x))


def _pairs_arrays(pairs):
    flat = [int(v) for pr in pairs for v in pr]
    rev = [pairs.index((b, a)) if (b, a) in pairs else i for i, (a, b) in enumerate(pairs)]
    return (C.c_int * len(flat))(*flat), (C.c_int * len(rev))(*rev)


def simce_lse_pairs(E, pairs, scale):
    """E f32 [nmod, B, P]; pairs = [(x_mod, y_mod), ...] (<= 6).  One launch: lse, pos each [npairs, B]."""
    _need_cuda(E, scale)
    assert E.dtype == torch.float32 and E.dim() == 3 and E.is_contiguous()
    nmod, B, P = E.shape
    n = len(pairs)
    pa, _ = _pairs_arrays(list(pairs))
    lse = torch.empty((n, B), dtype=torch.float32, device=E.device)
    pos = torch.zeros((n, B), dtype=torch.float32, device=E.device)
    lib = _lib()
    nbytes = lib.clipk_simce_pairs_workspace(n, B, P)
    if nbytes == 0:
        raise _ffi.ClipkError(f"simce pairs: unsupported shape npairs={n} B={B} P={P}")
    ws = workspace(nbytes, E.device, "simce")
    check(lib.clipk_simce_lse_pairs(E.data_ptr(), nmod, B, P, pa, n, scale.data_ptr(), lse.data_ptr(), pos.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream()), "clipk_simce_lse_pairs")
    return lse, pos


def simce_grad_pairs(E, pairs, scale, lse, w_row, w_col, inv_bg):
    """Gradients of every directed problem w.r.t. its X rows: dX [npairs, B, P], dscale partials [npairs, B]."""
    _need_cuda(E, scale, lse)
    nmod, B, P = E.shape
    n = len(pairs)
    pa, ra = _pairs_arrays(list(pairs))
    dX = torch.empty((n, B, P), dtype=torch.float32, device=E.device)
    dsc = torch.empty((n, B), dtype=torch.float32, device=E.device)
    lib = _lib()
    ws = workspace(lib.clipk_simce_pairs_workspace(n, B, P), E.device, "simce")
    check(lib.clipk_simce_grad_pairs(E.data_ptr(), nmod, B, P, pa, ra, n, scale.data_ptr(), lse.data_ptr(), float(w_row),
                                     float(w_col), float(inv_bg), dX.data_ptr(), dsc.data_ptr(), ws.data_ptr(),
                                     ws.numel(), _stream()), "clipk_simce_grad_pairs")
    return dX, dsc


def _pairs_variant_args(E, pairs, scale, ids, same_class="mask", eps=0.0, tensors=()):
    """Shapes and dtypes of the batched class-aware / hard-negative passes' operands (the kernels read them as raw f32 /
    int64 arrays of these lengths): ValueError on anything else.  ids: None or one entry per problem, each None or int64
    [B]; both directions of a pair carry the same ids.  tensors: (name, tensor or None, shape) of further f32 inputs.
    Returns (the host pairs array, the reverse array, the host array of id pointers)."""
    if E.dtype != torch.float32 or E.dim() != 3 or not E.is_contiguous():
        raise ValueError(f"E must be a contiguous float32 [nmod, B, P] tensor, got {E.dtype} {tuple(E.shape)}")
    nmod, B, P = E.shape
    pairs = [(int(a), int(b)) for a, b in pairs]
    n = len(pairs)
    if not 1 <= n <= 6:
        raise ValueError(f"1 to 6 problems per launch, got {n}")
    if any(not (0 <= a < nmod and 0 <= b < nmod) for a, b in pairs):
        raise ValueError(f"pairs index the {nmod} modalities of E, got {pairs}")
    if B == 0 or P == 0 or P % 4 or P > 512:
        raise ValueError(f"the batched class-aware / hard-negative passes support B > 0, P % 4 == 0 and P <= 512, got "
                         f"B = {B}, P = {P}")
    if scale.dtype != torch.float32 or scale.numel() != 1:
        raise ValueError(f"scale must be a 1-element float32 tensor, got {scale.dtype} {tuple(scale.shape)}")
    ids = [None] * n if ids is None else list(ids)
    if len(ids) != n:
        raise ValueError(f"ids: one entry (a tensor or None) per problem, got {len(ids)} for {n} problems")
    for i, t in enumerate(ids):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != (B,)
                              or not t.is_contiguous()):
            raise ValueError(f"ids[{i}] must be a contiguous int64 tensor of shape ({B},) or None, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
    pa, ra = _pairs_arrays(pairs)
    for i, r in enumerate(ra):
        if ptr(ids[i]) != ptr(ids[r]):
            raise ValueError(f"problems {i} and {r} are the two directions of one pair: they must carry the same ids")
    for name, t, shape in tensors:
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape}, got {t.dtype} "
                             f"{tuple(t.shape)}")
    if same_class not in _ffi.SAME_CLASS:
        raise ValueError(f"same_class must be one of {tuple(_ffi.SAME_CLASS)}, got {same_class!r}")
    if not 0.0 <= float(eps) < 1.0:
        raise ValueError(f"eps must be in [0, 1), got {eps}")
    _need_cuda(E, scale, *ids, *[t for _, t, _ in tensors])
    return pa, ra, (C.c_void_p * n)(*[ptr(t) for t in ids])


def _simce_pairs(entry, kind, E, n, args, outs):
    """The call the four batched variant wrappers share: outputs (f32, torch.empty), workspace, the entry point.  args:
    its arguments between P and the outputs."""
    nmod, B, P = E.shape
    res = [torch.empty(shape, dtype=torch.float32, device=E.device) for shape in outs]
    lib = _lib()
    nbytes = getattr(lib, f"clipk_simce_pairs_{kind}_workspace")(n, B, P)
    if nbytes == 0:
        raise _ffi.ClipkError(f"simce pairs ({kind}): unsupported shape npairs={n} B={B} P={P}")
    stream = _stream()
    ws = workspace(nbytes, E.device, "simce", stream)
    check(getattr(lib, entry)(E.data_ptr(), nmod, B, P, *args, *[t.data_ptr() for t in res], ws.data_ptr(), ws.numel(),
                              stream), entry)
    return tuple(res)


def simce_lse_pairs_cls(E, pairs, scale, ids=None, same_class="mask", eps=0.0):
    """Batched class-aware LSE pass (include/clipk.h: clipk_simce_lse_pairs_cls): (lse, tgt, cnt), each f32 [npairs, B].
    ids: per problem a device int64 [B] or None (all distinct)."""
    pa, _, ia = _pairs_variant_args(E, pairs, scale, ids, same_class, eps)
    n, B = len(pairs), E.shape[1]
    return _simce_pairs("clipk_simce_lse_pairs_cls", "cls", E, n,
                        (pa, n, scale.data_ptr(), ia, _ffi.SAME_CLASS[same_class], float(eps)), ((n, B),) * 3)


def simce_grad_pairs_cls(E, pairs, scale, lse, cnt, w_row, w_col, inv_bg, ids=None, same_class="mask", eps=0.0,
                         upstream=None):
    """Batched class-aware gradient pass (clipk_simce_grad_pairs_cls): dX [npairs, B, P], dscale partials [npairs, B].
    lse, cnt: simce_lse_pairs_cls's; upstream: f32 [npairs] multiplied into each problem's gradient, or None."""
    n, (_, B, P) = len(pairs), E.shape
    pa, ra, ia = _pairs_variant_args(E, pairs, scale, ids, same_class, eps,
                                     (("lse", lse, (n, B)), ("cnt", cnt, (n, B)), ("upstream", upstream, (n,))))
    return _simce_pairs("clipk_simce_grad_pairs_cls", "cls", E, n,
                        (pa, ra, n, scale.data_ptr(), ia, _ffi.SAME_CLASS[same_class], float(eps), lse.data_ptr(),
                         cnt.data_ptr(), float(w_row), float(w_col), float(inv_bg), ptr(upstream)), ((n, B, P), (n, B)))


def simce_lse_pairs_hard(E, pairs, scale, beta, ids=None):
    """Batched hard-negative LSE pass (clipk_simce_lse_pairs_hard): lse_h, pos f32 [npairs, B], coef f32 [npairs, 3, B]."""
    beta = _hard_beta(beta)
    pa, _, ia = _pairs_variant_args(E, pairs, scale, ids)
    n, B = len(pairs), E.shape[1]
    return _simce_pairs("clipk_simce_lse_pairs_hard", "hard", E, n, (pa, n, scale.data_ptr(), beta, ia),
                        ((n, B), (n, B), (n, 3, B)))


def simce_grad_pairs_hard(E, pairs, scale, beta, coef, w_row, w_col, inv_bg, ids=None, upstream=None):
    """Batched hard-negative gradient pass (clipk_simce_grad_pairs_hard): dX [npairs, B, P], dscale partials
    [npairs, B].  coef: simce_lse_pairs_hard's; upstream: f32 [npairs] or None."""
    beta = _hard_beta(beta)
    n, (_, B, P) = len(pairs), E.shape
    pa, ra, ia = _pairs_variant_args(E, pairs, scale, ids, tensors=(("coef", coef, (n, 3, B)),
                                                                     ("upstream", upstream, (n,))))
    return _simce_pairs("clipk_simce_grad_pairs_hard", "hard", E, n,
                        (pa, ra, n, scale.data_ptr(), beta, ia, coef.data_ptr(), float(w_row), float(w_col),
                         float(inv_bg), ptr(upstream)), ((n, B, P), (n, B)))


def sim_logits(x, y, scale):
    _need_cuda(x, y, scale)
    Mx, P = x.shape
    Ny = y.shape[0]
    s = torch.empty((Mx, Ny), dtype=torch.float32, device=x.device)
    check(_lib().clipk_sim_logits(x.data_ptr(), Mx, y.data_ptr(), Ny, P, scale.data_ptr(), s.data_ptr(), s.stride(0),
                                  _stream()), "clipk_sim_logits")
    return s


def _retrieval_args(x, y):
    for name, t in (("queries", x), ("gallery", y)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 2-D tensor, got shape {tuple(t.shape)}")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"queries have {x.shape[1]} columns, the gallery {y.shape[1]}")
    Mx, P = x.shape
    Ny = y.shape[0]
    if Mx == 0 or Ny == 0 or P == 0 or P % 4:
        raise ValueError(f"need non-empty inputs and P % 4 == 0 (Mx={Mx}, Ny={Ny}, P={P})")
    return Mx, Ny, P


# ---- the shared pieces of the embedding-cloud wrappers below (sim_topk .. tsne_update)
def _check_width(P, max_p):
    if P <= 0 or P % 4 or P > max_p:
        raise ValueError(f"P = {P} is outside the kernel's limit (P % 4 == 0, P <= {max_p})")


def _cloud_args(x, y, max_p):
    """(Mx, Ny, P) of a pair of clouds: _retrieval_args and the kernel's width limit."""
    Mx, Ny, P = _retrieval_args(x, y)
    _check_width(P, max_p)
    return Mx, Ny, P


def _device_args(who, *ts):
    """The tensors given (None: an optional one left out) are on the current device; who: the subject and verb of the
    ValueError a host tensor raises."""
    _args.need_device(who, *ts)
    _need_cuda(*ts)


def _sq_norms(x, y, nx, ny, wanted=True):
    """(nx, ny): the squared norms of the rows of x and y where the caller gave none; one product for a cloud with
    itself.  wanted=False (a metric that reads no norms) leaves them as they came."""
    if wanted:
        if nx is None:
            nx = (x * x).sum(1)
        if ny is None:
            ny = nx if y is x else (y * y).sum(1)
    return nx, ny


def _diag_offset(diag_offset) -> int:
    diag_offset = int(diag_offset)
    if diag_offset < -1:
        raise ValueError(f"diag_offset must be -1 (nothing skipped) or >= 0, got {diag_offset}")
    return diag_offset


def _key_split_plan(entry, rows, Ny):
    """(query blocks, key-range splits) that `entry`, a clipk_*_plan function, reports for these sizes."""
    nqb, ks = C.c_int(0), C.c_int(0)
    check(getattr(_lib(), entry)(int(rows), int(Ny), C.byref(nqb), C.byref(ks)), entry)
    return nqb.value, ks.value


def _launch(name, work, args, ws=None, entry=None):
    """Enqueue clipk_<name>(*args[, workspace, its bytes], stream) on torch's current stream, timed as `name` with the
    algorithmic `work`, and check its status.  ws = (device, tag, *the arguments of clipk_<name>_workspace): the
    kernel's scratch, from the grow-only buffer `tag`.  entry: the function where it is not clipk_<name>."""
    lib = _lib()
    stream = _stream()
    if ws is not None:
        buf = workspace(getattr(lib, f"clipk_{name}_workspace")(*ws[2:]), ws[0], ws[1], stream)
        args = (*args, buf.data_ptr(), buf.numel())
    entry = "clipk_" + (entry or name)
    check(_timed(name, work, lambda: getattr(lib, entry)(*args, stream)), entry)


def sim_topk(x, y, k: int, scale: Optional[float] = None):
    """(scores f32 [Mx, k], idx int64 [Mx, k]): the k best keys of S = scale * x y^T per row, score descending, equal
    scores by the lower index (include/clipk.h: clipk_sim_topk).  scale: host number, None = 1."""
    Mx, Ny, P = _retrieval_args(x, y)
    k = int(k)
    if not 1 <= k <= 64:
        raise ValueError(f"k must be in [1, 64], got {k}")
    if k > Ny:
        raise ValueError(f"k = {k} exceeds the gallery size {Ny}")
    _need_cuda(x, y)
    scores = torch.empty((Mx, k), dtype=torch.float32, device=x.device)
    idx = torch.empty((Mx, k), dtype=torch.int64, device=x.device)
    _launch("sim_topk", 2.0 * Mx * Ny * P,
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, 1.0 if scale is None else float(scale), k, scores.data_ptr(),
             idx.data_ptr()), (x.device, "retrieval", Mx, Ny, P, k))
    return scores, idx


def sim_knn(x, y, k: int, scale: Optional[float] = None, bias=None, diag_offset: int = -1, after=None):
    """(scores f32 [Mx, k], idx int64 [Mx, k]): the k best ELIGIBLE keys of z = scale * x y^T + bias[None, :] per row in
    the order of sim_topk (include/clipk.h: clipk_sim_knn).  bias: device f32 [Ny] or None; diag_offset >= 0: row i skips
    key i + diag_offset (-1: none); after = (scores f32 [Mx], idx int64 [Mx]): a cursor in the order - only keys strictly
    after it are eligible.  1 <= k <= 64; with fewer than k eligible keys the trailing slots are (-inf, -1)."""
    Mx, Ny, P = _retrieval_args(x, y)
    _args.int_in("k", k, 1, 64)
    _args.int_in("diag_offset", diag_offset, -1, what="-1 or a non-negative int")     # (no bool, unlike _diag_offset)
    if bias is not None and (bias.dtype != torch.float32 or bias.shape != (Ny,) or not bias.is_contiguous()):
        raise ValueError(f"bias must be a contiguous float32 tensor of shape ({Ny},)")
    after_s = after_i = None
    if after is not None:
        if not isinstance(after, (tuple, list)) or len(after) != 2:
            raise ValueError("after must be a (scores, idx) pair")
        after_s, after_i = after
        if after_s.dtype != torch.float32 or after_s.shape != (Mx,) or not after_s.is_contiguous() \
                or after_i.dtype != torch.int64 or after_i.shape != (Mx,) or not after_i.is_contiguous():
            raise ValueError(f"after must be contiguous (float32, int64) tensors of shape ({Mx},)")
    _need_cuda(x, y, bias, after_s, after_i)
    scores = torch.empty((Mx, k), dtype=torch.float32, device=x.device)
    idx = torch.empty((Mx, k), dtype=torch.int64, device=x.device)
    _launch("sim_knn", 2.0 * Mx * Ny * P,
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, 1.0 if scale is None else float(scale), ptr(bias), diag_offset,
             ptr(after_s), ptr(after_i), k, scores.data_ptr(), idx.data_ptr()), (x.device, "retrieval", Mx, Ny, P, k))
    return scores, idx


def pair_sqdist(x, y, idx):
    """f32 [Mx, k]: |x_i - y_{idx[i, t]}|^2 summed from the differences in a fixed order (include/clipk.h:
    clipk_pair_sqdist); idx int64 [Mx, k], an entry outside [0, Ny) gives +inf."""
    Mx, Ny, P = _retrieval_args(x, y)
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != Mx or idx.shape[1] == 0 or not idx.is_contiguous():
        raise ValueError(f"idx must be a contiguous int64 tensor of shape ({Mx}, k), k >= 1")
    _need_cuda(x, y, idx)
    d2 = torch.empty(idx.shape, dtype=torch.float32, device=x.device)
    _launch("pair_sqdist", 3.0 * idx.numel() * P,
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, idx.data_ptr(), idx.shape[1], d2.data_ptr()))
    return d2


SPMM_CHUNK = 64              # CLIPK_SPMM_CHUNK: entries of one chunk sum
SPMM_MAX_M = 64              # CLIPK_SPMM_MAX_M


def _csr_spmm_args(indptr, indices, w, x, s, b, c, out):
    """(N, nnz, m) after every argument check of csr_spmm that needs no device."""
    for name, t, dt in (("indptr", indptr, torch.int64), ("indices", indices, torch.int32), ("w", w, torch.float64),
                        ("x", x, torch.float64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor")
    if x.dim() != 2 or x.shape[0] == 0 or not 1 <= x.shape[1] <= SPMM_MAX_M:
        raise ValueError(f"x must be [N, m] with N >= 1 and 1 <= m <= {SPMM_MAX_M}, got shape {tuple(x.shape)}")
    N, m = x.shape
    if indptr.shape != (N + 1,):
        raise ValueError(f"indptr must have shape ({N + 1},), got {tuple(indptr.shape)}")
    if indices.dim() != 1 or w.shape != indices.shape:
        raise ValueError("indices and w must be 1-D tensors of one length")
    if s is not None and (not isinstance(s, torch.Tensor) or s.dtype != torch.float64 or s.shape != (N,)
                          or not s.is_contiguous()):
        raise ValueError(f"s must be a contiguous float64 tensor of shape ({N},)")
    for name, t in (("b", b), ("c", c), ("out", out)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.shape != x.shape
                              or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float64 tensor of shape {tuple(x.shape)}")
    if out is not None and out.data_ptr() == x.data_ptr():
        raise ValueError("out may be b or c but never x: rows of x are gathered while rows of out are written")
    return N, indices.shape[0], m


def csr_spmm(indptr, indices, w, x, s=None, alpha: float = 1.0, b=None, beta: float = 0.0, c=None, gamma: float = 0.0,
             out=None):
    """f64 [N, m]: alpha * diag(s) W diag(s) x + beta * b + gamma * c for a CSR matrix W (indptr int64 [N + 1], indices
    int32 [nnz], w f64 [nnz]) on a block x f64 [N, m], 1 <= m <= 64; s f64 [N] or None (ones); b, c f64 [N, m] or None.
    out: where to write (may be b or c, never x); None allocates.  The arithmetic is fixed and stated in include/clipk.h
    (clipk_csr_spmm_f64): a numpy restatement gives the same bits.  No host read."""
    N, nnz, m = _csr_spmm_args(indptr, indices, w, x, s, b, c, out)
    _need_cuda(indptr, indices, w, x, s, b, c, out)
    y = torch.empty_like(x) if out is None else out
    _launch("csr_spmm", 2.0 * nnz * m,
            (indptr.data_ptr(), indices.data_ptr(), w.data_ptr(), ptr(s), N, nnz, m, x.data_ptr(), float(alpha), ptr(b),
             float(beta), ptr(c), float(gamma), y.data_ptr()), (x.device, "spmm", nnz, m), entry="csr_spmm_f64")
    return y


LABEL_PAIRS_MAX_G = 1024      # CLIPK_LABEL_PAIRS_MAX_G: an int64 table of at most 8 MB
LABEL_PAIRS_MAX_K = 1024


def _knn_label_pairs_args(idx, row_labels, num_groups, key_labels, out):
    """(M, k, Ny, G) after every argument check of knn_label_pairs that needs no device."""
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] == 0 \
            or not 1 <= idx.shape[1] <= LABEL_PAIRS_MAX_K or not idx.is_contiguous():
        raise ValueError(f"idx must be a contiguous int64 tensor of shape (M, k), M >= 1, 1 <= k <= {LABEL_PAIRS_MAX_K}")
    _args.int_in("num_groups", num_groups, 1, LABEL_PAIRS_MAX_G)
    M, k = idx.shape
    for name, t, n in (("row_labels", row_labels, M), ("key_labels", key_labels, None)):
        if name == "key_labels" and t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] == 0 \
                or (n is not None and t.shape[0] != n) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 tensor of shape ({'Ny' if n is None else n},)")
    G = num_groups
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or out.shape != (G, G)
                            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 tensor of shape ({G}, {G})")
    return M, k, (M if key_labels is None else key_labels.shape[0]), G


def knn_label_pairs(idx, row_labels, num_groups: int, key_labels=None, out=None):
    """int64 [G, G]: counts[a, b] = how many entries idx[i, t] have row_labels[i] = a and key_labels[idx[i, t]] = b, in one
    pass over the indices (include/clipk.h: clipk_knn_label_pairs).  idx int64 [M, k], k <= 1024; row_labels int32 [M];
    key_labels int32 [Ny] or None (the row labels: a graph of a cloud against itself); 1 <= num_groups <= 1024.  A label
    outside [0, G) and an index outside [0, Ny) count nowhere.  out: an int64 [G, G] table that is ADDED into; None
    allocates zeros.  Exact integer counts; no host read."""
    M, k, Ny, G = _knn_label_pairs_args(idx, row_labels, num_groups, key_labels, out)
    _need_cuda(idx, row_labels, key_labels, out)
    counts = torch.zeros((G, G), dtype=torch.int64, device=idx.device) if out is None else out
    keys = row_labels if key_labels is None else key_labels
    _launch("knn_label_pairs", float(idx.numel()),
            (idx.data_ptr(), M, k, row_labels.data_ptr(), keys.data_ptr(), Ny, G, counts.data_ptr()))
    return counts


def plane_pitch(P: int) -> int:
    """Row pitch (bf16 elements) of the planes clipk_split_bf16 writes: P rounded up to 32, pads zero."""
    return (int(P) + 31) // 32 * 32


def split_bf16(x, hi, lo=None, norm_max=None):
    """Rows of f32 x [n, P] -> bf16 plane hi (and lo = bf16(x - hi)), both [n, plane_pitch(P)] (any 2-byte dtype);
    norm_max (device f32 [1]) is raised to the largest row norm, rounded upward (include/clipk.h: clipk_split_bf16)."""
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        raise TypeError("split_bf16 needs a contiguous 2-D float32 tensor")
    n, P = x.shape
    for t in (hi, lo):
        if t is not None and (t.element_size() != 2 or tuple(t.shape) != (n, plane_pitch(P)) or not t.is_contiguous()):
            raise ValueError(f"planes must be contiguous 2-byte tensors of shape ({n}, {plane_pitch(P)})")
    if norm_max is not None and (norm_max.dtype != torch.float32 or norm_max.numel() != 1):
        raise ValueError("norm_max must be a float32 tensor of one element")
    _need_cuda(x, hi, lo, norm_max)
    if n == 0:
        return
    _launch("split_bf16", 0.0, (x.data_ptr(), n, P, hi.data_ptr(), ptr(lo), ptr(norm_max)))


def sim_topk_cand(x, yhi, ylo, Ny: int, P: int, kc: int, scale: Optional[float] = None):
    """(scores f32 [Mx, kc], idx int64 [Mx, kc]): the kc best keys of the bf16 (ylo None) or bf16x3 similarity
    scale * x y^T from the gallery's planes, in the order of sim_topk (include/clipk.h: clipk_sim_topk_cand)."""
    if x.dtype != torch.float32:
        raise TypeError(f"queries must be float32, got {x.dtype}")
    if x.dim() != 2 or not x.is_contiguous() or x.shape[1] != P or x.data_ptr() % 16:
        raise ValueError("queries must be a contiguous, 16-byte aligned [Mx, P] tensor")
    for t in (yhi, ylo):
        if t is not None and (t.element_size() != 2 or t.dim() != 2 or t.shape[0] < Ny or t.shape[1] != plane_pitch(P)
                              or not t.is_contiguous() or t.data_ptr() % 16):
            raise ValueError(f"gallery planes must be contiguous, aligned [>= {Ny}, {plane_pitch(P)}] 2-byte tensors")
    kc = int(kc)
    if not 1 <= kc <= 64:
        raise ValueError(f"candidates must be in [1, 64], got {kc}")
    Mx = x.shape[0]
    if Mx == 0 or Ny <= 0 or P <= 0 or P % 4:
        raise ValueError(f"need non-empty inputs and P % 4 == 0 (Mx={Mx}, Ny={Ny}, P={P})")
    _need_cuda(x, yhi, ylo)
    scores = torch.empty((Mx, kc), dtype=torch.float32, device=x.device)
    idx = torch.empty((Mx, kc), dtype=torch.int64, device=x.device)
    _launch("sim_topk_cand", 2.0 * Mx * Ny * plane_pitch(P) * (1 if ylo is None else 3),
            (x.data_ptr(), Mx, yhi.data_ptr(), ptr(ylo), Ny, P, 1.0 if scale is None else float(scale), kc,
             scores.data_ptr(), idx.data_ptr()), (x.device, "retrieval", Mx, Ny, P, kc, 1 if ylo is None else 2))
    return scores, idx


def sim_rerank(x, y, cand_scores, cand_idx, k: int, eps_rel: float, y_norm_max, scale: Optional[float] = None):
    """(scores f32 [Mx, k], idx int64 [Mx, k], certified int32 [Mx]): the exact top k among each row's candidates, with the
    bits of sim_topk, and whether the bound proves them the top k of the whole gallery (include/clipk.h:
    clipk_sim_rerank).  Rows with certified == 0 hold unspecified results."""
    Mx, Ny, P = _retrieval_args(x, y)
    kc, k = cand_idx.shape[1], int(k)
    if cand_idx.dtype != torch.int64 or cand_scores.dtype != torch.float32 or cand_idx.shape != (Mx, kc) \
            or cand_scores.shape != (Mx, kc) or not cand_idx.is_contiguous() or not cand_scores.is_contiguous():
        raise ValueError("candidates must be contiguous [Mx, kc] float32 scores and int64 indices")
    if not 1 <= k <= kc <= 64 or k > Ny:
        raise ValueError(f"need 1 <= k <= candidates <= 64 and k <= Ny (k={k}, candidates={kc}, Ny={Ny})")
    if y_norm_max.dtype != torch.float32 or y_norm_max.numel() != 1:
        raise ValueError("y_norm_max must be a float32 tensor of one element")
    _need_cuda(x, y, cand_scores, cand_idx, y_norm_max)
    scores = torch.empty((Mx, k), dtype=torch.float32, device=x.device)
    idx = torch.empty((Mx, k), dtype=torch.int64, device=x.device)
    cert = torch.empty(Mx, dtype=torch.int32, device=x.device)
    _launch("sim_rerank", 2.0 * Mx * kc * P,
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, 1.0 if scale is None else float(scale), cand_idx.data_ptr(),
             cand_scores.data_ptr(), kc, k, float(eps_rel), y_norm_max.data_ptr(), scores.data_ptr(), idx.data_ptr(),
             cert.data_ptr()))
    return scores, idx, cert


def sim_rank(x, y, labels=None, label_offset: int = 0, scale: Optional[float] = None, class_ids=None):
    """(rank int64 [Mx], pos f32 [Mx]): 0-based rank of key l_i in row i of S = scale * x y^T under the same order as
    sim_topk, and S[i, l_i] (include/clipk.h: clipk_sim_rank).  l_i = labels[i] (device int64 [Mx]) or label_offset + i.
    A label outside [0, Ny) gives rank -1 and pos NaN.  class_ids (device int64 [Ny], gallery class ids): count only
    gallery rows of another class than l_i's (clipk_sim_rank_cls)."""
    Mx, Ny, P = _retrieval_args(x, y)
    if labels is not None:
        if labels.dtype != torch.int64 or labels.shape != (Mx,) or not labels.is_contiguous():
            raise ValueError(f"labels must be a contiguous int64 tensor of shape ({Mx},)")
    elif not (0 <= int(label_offset) and int(label_offset) + Mx <= Ny):
        raise ValueError(f"labels label_offset + i = {label_offset} .. {int(label_offset) + Mx - 1} outside [0, {Ny})")
    if class_ids is not None:
        if class_ids.dtype != torch.int64 or class_ids.shape != (Ny,) or not class_ids.is_contiguous():
            raise ValueError(f"class_ids must be a contiguous int64 tensor of shape ({Ny},)")
    _need_cuda(x, y, labels, class_ids)
    rank = torch.empty(Mx, dtype=torch.int64, device=x.device)
    pos = torch.empty(Mx, dtype=torch.float32, device=x.device)
    cls = () if class_ids is None else (class_ids.data_ptr(),)
    _launch("sim_rank", 2.0 * Mx * Ny * P,
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, 1.0 if scale is None else float(scale), ptr(labels), int(label_offset),
             *cls, rank.data_ptr(), pos.data_ptr()), (x.device, "retrieval", Mx, Ny, P),
            entry="sim_rank_cls" if cls else None)
    return rank, pos


class SimStats(NamedTuple):
    """The outputs of clipk_sim_stats, in the order of include/clipk.h."""
    pos: torch.Tensor          # f32 [Mx]
    best: torch.Tensor         # f32 [Mx]
    best_idx: torch.Tensor     # int64 [Mx]
    hard: torch.Tensor         # f32 [Mx]
    hard_idx: torch.Tensor     # int64 [Mx]
    lse: torch.Tensor          # f32 [Mx]
    neg_sum: torch.Tensor      # f64 [Mx]
    neg_sumsq: torch.Tensor    # f64 [Mx]
    hist_neg: torch.Tensor     # int64 [nbins + 2]
    hist_pos: torch.Tensor     # int64 [nbins + 2]


def sim_stats(x, y, *, scale: float = 1.0, labels=None, label_offset: int = 0, cls_x=None, cls_y=None, nbins: int = 64,
              lo: Optional[float] = None, hi: Optional[float] = None) -> SimStats:
    """Row statistics and histograms of S = scale * x y^T in one fused pass (include/clipk.h: clipk_sim_stats has the
    definitions and the binning rule).  l_i = labels[i] (device int64 [Mx]) or label_offset + i; cls_x [Mx] / cls_y [Ny]
    (device int64, both or neither) exclude the keys of the query's class other than its label.  The histograms have
    nbins in [1, 256] bins over [lo, hi) plus the two outer slots; lo / hi default to -|scale| / |scale|."""
    Mx, Ny, P = _retrieval_args(x, y)
    if labels is not None:
        if labels.dtype != torch.int64 or labels.shape != (Mx,) or not labels.is_contiguous():
            raise ValueError(f"labels must be a contiguous int64 tensor of shape ({Mx},)")
    elif not (0 <= int(label_offset) and int(label_offset) + Mx <= Ny):
        raise ValueError(f"labels label_offset + i = {label_offset} .. {int(label_offset) + Mx - 1} outside [0, {Ny})")
    if (cls_x is None) != (cls_y is None):
        raise ValueError("class ids are needed on both sides (cls_x and cls_y) or on neither")
    for name, t, n in (("cls_x", cls_x, Mx), ("cls_y", cls_y, Ny)):
        if t is not None and (t.dtype != torch.int64 or t.shape != (n,) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int64 tensor of shape ({n},)")
    nbins = int(nbins)
    if not 1 <= nbins <= 256:
        raise ValueError(f"nbins must be in [1, 256], got {nbins}")
    sc = float(scale)
    lo = -abs(sc) if lo is None else float(lo)
    hi = abs(sc) if hi is None else float(hi)
    lo32, hi32 = C.c_float(lo).value, C.c_float(hi).value      # what the kernel sees
    if not (lo32 < hi32) or lo32 in (float("-inf"), float("inf")) or hi32 in (float("-inf"), float("inf")):
        raise ValueError(f"need finite lo < hi, got lo = {lo}, hi = {hi}")
    _need_cuda(x, y, labels, cls_x, cls_y)
    dev = x.device
    f32 = lambda: torch.empty(Mx, dtype=torch.float32, device=dev)
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
    f64 = lambda: torch.empty(Mx, dtype=torch.float64, device=dev)
    out = SimStats(f32(), f32(), i64(Mx), f32(), i64(Mx), f32(), f64(), f64(), i64(nbins + 2), i64(nbins + 2))
    _launch("sim_stats", 2.0 * Mx * Ny * P,
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, sc, ptr(labels), int(label_offset), ptr(cls_x), ptr(cls_y), nbins, lo32,
             hi32, *(t.data_ptr() for t in out)), (dev, "retrieval", Mx, Ny, P, nbins))
    return out


SIM_LSE_BIAS_MAX_P = 768        # clipk_sim_lse_bias
SINKHORN_APPLY_MAX_P = 512      # clipk_sinkhorn_apply


def _f32_vectors(vectors):
    """Dtype, shape and contiguity of optional f32 vectors.  vectors: (name, tensor or None, length)."""
    for name, t, n in vectors:
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.shape != (n,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous tensor of shape ({n},), got {tuple(t.shape)}")


def _sinkhorn_args(x, y, scale, max_p, vectors=()):
    """Operand checks of the two Sinkhorn entries, before any launch.  vectors: (name, tensor or None, length)."""
    Mx, Ny, P = _cloud_args(x, y, max_p)
    _device_scalar("scale", scale)
    _f32_vectors(vectors)
    _device_args("the Sinkhorn kernels need", x, y, scale, *(v[1] for v in vectors))
    return Mx, Ny, P


def _device_scalar(name, t):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1:
        raise TypeError(f"{name} must be a one-element float32 device tensor")


def sim_lse_bias_plan(Mx: int, Ny: int):
    """(64-query blocks, key-range splits) of the grid clipk_sim_lse_bias launches for these sizes."""
    return _key_split_plan("clipk_sim_lse_bias_plan", Mx, Ny)


def sim_lse_bias(x, y, scale, bias=None, logw=None, prev=None, average=False, out=None, err=None):
    """One Sinkhorn half-iteration (include/clipk.h: clipk_sim_lse_bias): nv[i] = logw[i] - logsumexp_j(scale * <x_i, y_j>
    + bias[j]); returns out = nv, or (prev + nv) / 2 with average=True.  scale: device scalar; bias [Ny], logw [Mx], prev
    [Mx]: f32 device vectors or None.  err: device scalar that receives += sum_i exp(logw_i) |exp(prev_i - nv_i) - 1|
    (needs prev).  out may be given, and may be prev."""
    Mx, Ny, P = _sinkhorn_args(x, y, scale, SIM_LSE_BIAS_MAX_P,
                               (("bias", bias, y.shape[0]), ("logw", logw, x.shape[0]), ("prev", prev, x.shape[0]),
                                ("out", out, x.shape[0]), ("err", None if err is None else err.reshape(-1), 1)))
    if (average or err is not None) and prev is None:
        raise ValueError("average=True and err need prev")
    if out is None:
        out = torch.empty(Mx, dtype=torch.float32, device=x.device)
    _launch("sim_lse_bias", 2.0 * Mx * Ny * P,
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, scale.data_ptr(), ptr(bias), ptr(logw), ptr(prev), int(bool(average)),
             out.data_ptr(), ptr(err)), (x.device, "sinkhorn", Mx, Ny, P))
    return out


def sim_lse_bias_x3_plan(Mx: int, Ny: int):
    """(128-query blocks, key-range splits) of the grid clipk_sim_lse_bias_x3 launches for these sizes."""
    return _key_split_plan("clipk_sim_lse_bias_x3_plan", Mx, Ny)


def sim_lse_bias_x3(xhi, xlo, yhi, ylo, P: int, scale, bias=None, logw=None, prev=None, average=False, out=None, err=None):
    """sim_lse_bias with the product as a bf16x3 split on the bf16 matrix pipe (include/clipk.h: clipk_sim_lse_bias_x3):
    nv[i] = logw[i] - logsumexp_j(scale * A_ij + bias[j]), A = hi.hi + hi.lo + lo.hi.  xhi / xlo [Mx, plane_pitch(P)] and
    yhi / ylo [Ny, plane_pitch(P)]: the planes split_bf16 writes for the two clouds of width P.  Everything else as in
    sim_lse_bias; |nv - sim_lse_bias's| <= |scale| max|x| max|y| retrieval.prefilter_eps_rel(P, "bf16x3") + eps_abs."""
    P = int(P)
    _check_width(P, SIM_LSE_BIAS_MAX_P)
    for name, t in (("xhi", xhi), ("xlo", xlo), ("yhi", yhi), ("ylo", ylo)):
        if not isinstance(t, torch.Tensor) or t.element_size() != 2:
            raise TypeError(f"{name} must be a 2-byte (bf16) plane tensor")
        if t.dim() != 2 or t.shape[0] == 0 or t.shape[1] != plane_pitch(P) or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"{name} must be a contiguous, 16-byte aligned [rows, {plane_pitch(P)}] plane, got "
                             f"{tuple(t.shape)}")
    if xlo.shape != xhi.shape or ylo.shape != yhi.shape:
        raise ValueError("the hi and lo planes of a cloud must have one shape")
    Mx, Ny = xhi.shape[0], yhi.shape[0]
    _device_scalar("scale", scale)
    vectors = (("bias", bias, Ny), ("logw", logw, Mx), ("prev", prev, Mx), ("out", out, Mx),
               ("err", None if err is None else err.reshape(-1), 1))
    _f32_vectors(vectors)
    if (average or err is not None) and prev is None:
        raise ValueError("average=True and err need prev")
    _device_args("the Sinkhorn kernels need", xhi, xlo, yhi, ylo, scale, *(v[1] for v in vectors))
    if out is None:
        out = torch.empty(Mx, dtype=torch.float32, device=xhi.device)
    _launch("sim_lse_bias_x3", 6.0 * Mx * Ny * plane_pitch(P),
            (xhi.data_ptr(), xlo.data_ptr(), Mx, yhi.data_ptr(), ylo.data_ptr(), Ny, P, scale.data_ptr(), ptr(bias),
             ptr(logw), ptr(prev), int(bool(average)), out.data_ptr(), ptr(err)), (xhi.device, "sinkhorn", Mx, Ny, P))
    return out


def sinkhorn_apply(x, y, scale, u, v, nx=None, ny=None, want_mass=True, want_bary=True, want_cost=True):
    """Row sums over the plan P_ij = exp(scale * <x_i, y_j> + u_i + v_j) (include/clipk.h: clipk_sinkhorn_apply):
    (mass [Mx] = sum_j P_ij, bary [Mx, P] = sum_j P_ij y_j, cost [Mx] = sum_j P_ij |x_i - y_j|^2), None for an output not
    wanted.  cost needs the squared norms nx [Mx], ny [Ny]."""
    Mx, Ny, P = _sinkhorn_args(x, y, scale, SINKHORN_APPLY_MAX_P,
                               (("u", u, x.shape[0]), ("v", v, y.shape[0]), ("nx", nx, x.shape[0]), ("ny", ny, y.shape[0])))
    if u is None or v is None:
        raise ValueError("u and v are needed")
    if not (want_mass or want_bary or want_cost):
        raise ValueError("no output wanted")
    if want_cost and (nx is None or ny is None):
        raise ValueError("cost needs the squared norms nx and ny")
    dev = x.device
    mass = torch.empty(Mx, dtype=torch.float32, device=dev) if want_mass else None
    bary = torch.empty((Mx, P), dtype=torch.float32, device=dev) if want_bary else None
    cost = torch.empty(Mx, dtype=torch.float32, device=dev) if want_cost else None
    _launch("sinkhorn_apply", 2.0 * Mx * Ny * P * (2 if want_bary else 1),
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, scale.data_ptr(), u.data_ptr(), v.data_ptr(), ptr(nx), ptr(ny),
             ptr(mass), ptr(bary), ptr(cost)), (dev, "sinkhorn", Mx, Ny, P))
    return mass, bary, cost


def _seed_offset(seed, stream_offset, device=None):
    """{seed, stream_offset} as the kernel reads them: `seed` may be the int64 device tensor of two elements itself
    (stream_offset is then left at 0), or both are Python ints, taken modulo 2^64.  device=None: checks only."""
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.shape != (2,) or not seed.is_contiguous():
            raise TypeError("a seed tensor must be a contiguous int64 tensor of two elements, {seed, stream_offset}")
        if isinstance(stream_offset, torch.Tensor) or int(stream_offset) != 0:
            raise ValueError("a seed tensor carries the stream offset as its second element: leave stream_offset at 0")
        return seed
    vals = []
    for name, v in (("seed", seed), ("stream_offset", stream_offset)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} must be an int (or seed an int64 device tensor of two elements), got {type(v).__name__}")
        v &= (1 << 64) - 1
        vals.append(v - (1 << 64) if v >= 1 << 63 else v)
    return None if device is None else torch.tensor(vals, dtype=torch.int64, device=device)


def sim_sample(x, y, scale, bias=None, seed=0, stream_offset=0, want_score=False):
    """One Gumbel-max draw per row (include/clipk.h: clipk_sim_sample has the noise contract): idx[i] = argmax_j
    scale * <x_i, y_j> + bias[j] + G(seed, stream_offset + i, j), int64 [Mx], distributed as softmax_j(scale * <x_i, y_j>
    + bias[j]); with want_score also the winning value, f32 [Mx].  scale: device scalar; bias [Ny] f32 or None.  seed,
    stream_offset: Python ints, or `seed` one int64 device tensor {seed, stream_offset} that the kernel reads (a captured
    graph draws fresh noise once the caller changes it).  The result depends on (inputs, seed, stream) alone."""
    _seed_offset(seed, stream_offset)
    Mx, Ny, P = _sinkhorn_args(x, y, scale, SIM_LSE_BIAS_MAX_P, (("bias", bias, y.shape[0]),))
    if isinstance(seed, torch.Tensor):
        _device_args("the Sinkhorn kernels need", x, seed)
    so = _seed_offset(seed, stream_offset, x.device)
    idx = torch.empty(Mx, dtype=torch.int64, device=x.device)
    score = torch.empty(Mx, dtype=torch.float32, device=x.device) if want_score else None
    _launch("sim_sample", 2.0 * Mx * Ny * P,
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, scale.data_ptr(), ptr(bias), so.data_ptr(), idx.data_ptr(), ptr(score)),
            (x.device, "sinkhorn", Mx, Ny, P))
    return (idx, score) if want_score else idx


AUCTION_MAX_N = 65536           # clipk_auction_rounds: one workgroup compacts the unassigned rows


def _int32_vector(name, t, n, device):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{name} must be an int32 tensor")
    if t.shape != (n,) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor of shape ({n},), got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the clouds on {device}")


def sim_top2_bias_plan(Mr: int, Ny: int):
    """(64-query blocks, key-range splits) of the grid clipk_sim_top2_bias launches for Mr listed rows and Ny keys."""
    return _key_split_plan("clipk_sim_top2_bias_plan", Mr, Ny)


def sim_top2_bias(x, y, scale, bias=None, rows=None, n_active=None, want_best=True, want_gap=True, out=None):
    """The two best keys of every listed row (include/clipk.h: clipk_sim_top2_bias): z_rj = scale * <x[row(r)], y_j> +
    bias[j]; returns (idx int32 [Mr] = argmax_j, best f32 [Mr] = max_j, gap f32 [Mr] = best - runner-up, +inf with one
    key), None for an output not wanted.  A higher z is best, equal z goes to the lower key, an exact tie gives gap 0.
    scale: device scalar; bias [Ny] f32 or None.  rows: int32 [Mr] device indices into x's rows (repeats allowed; the
    caller answers for their range, nothing is read back), None = every row.  n_active: one-element int32 device tensor,
    only the list positions below it are computed, the others keep what `out` held.  out: (idx, best, gap) to write into
    (best / gap may be None when not wanted)."""
    Mr = _retrieval_args(x, y)[0]
    if rows is not None:
        if not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.numel() == 0:
            raise TypeError("rows must be a non-empty 1-D int32 index tensor")
        Mr = rows.shape[0]
        _int32_vector("rows", rows, Mr, x.device)
    if n_active is not None:
        _int32_vector("n_active", n_active, 1, x.device)
    dev = x.device
    if out is not None:
        idx, best, gap = out
        _int32_vector("out[0]", idx, Mr, dev)
        if (want_best and best is None) or (want_gap and gap is None):
            raise ValueError("out lacks an output that is wanted")
    else:
        best = gap = None
    Mx, Ny, P = _sinkhorn_args(x, y, scale, SIM_LSE_BIAS_MAX_P,
                               (("bias", bias, y.shape[0]), ("out[1]", best, Mr), ("out[2]", gap, Mr)))
    if out is None:
        idx = torch.empty(Mr, dtype=torch.int32, device=dev)
        best = torch.empty(Mr, dtype=torch.float32, device=dev) if want_best else None
        gap = torch.empty(Mr, dtype=torch.float32, device=dev) if want_gap else None
    _launch("sim_top2_bias", 2.0 * Mr * Ny * P,
            (x.data_ptr(), Mx, ptr(rows), Mr, ptr(n_active), y.data_ptr(), Ny, P, scale.data_ptr(), ptr(bias), idx.data_ptr(),
             ptr(best) if want_best else None, ptr(gap) if want_gap else None), (dev, "sinkhorn", Mr, Ny, P))
    return idx, (best if want_best else None), (gap if want_gap else None)


def auction_rounds(x, y, bias, eps, assigned, owner, n_unassigned, stalled, n_rounds: int):
    """n_rounds bidding rounds of the auction on device state, enqueued without a host read (include/clipk.h:
    clipk_auction_rounds): x, y [N, P] f32; bias [N] f32 = -|y_j|^2 - price_j, assigned [N] int32 (row -> key or -1) and
    owner [N] int32 (key -> row or -1) are updated in place; eps: one-element f32 device tensor; n_unassigned, stalled:
    one-element int32 device tensors - the count after the last round, and a flag set (never cleared) when an offer left
    a price unchanged.  n_rounds = 0 only counts.  Returns None."""
    _args.int_in("n_rounds", n_rounds, 0, what="a non-negative int")
    _device_scalar("eps", eps)
    N, Ny, P = _retrieval_args(x, y)
    if bias is None:
        raise ValueError("bias is needed")
    if N != Ny:
        raise ValueError(f"the auction needs clouds of one size, got {N} and {Ny}")
    if N > AUCTION_MAX_N:
        raise ValueError(f"the auction handles at most {AUCTION_MAX_N} rows, got {N}")
    for name, t, n in (("assigned", assigned, N), ("owner", owner, N), ("n_unassigned", n_unassigned, 1), ("stalled", stalled, 1)):
        _int32_vector(name, t, n, x.device)
    _sinkhorn_args(x, y, eps, SIM_LSE_BIAS_MAX_P, (("bias", bias, N),))
    _launch("auction_rounds", 2.0 * N * N * P,
            (x.data_ptr(), y.data_ptr(), N, P, bias.data_ptr(), eps.data_ptr(), assigned.data_ptr(), owner.data_ptr(),
             n_unassigned.data_ptr(), stalled.data_ptr(), n_rounds), (x.device, "sinkhorn", N, P))


KERNEL_SUMS_MAX_P = 512        # clipk_kernel_sums
KERNEL_SUMS_MAX_B = 8


def kernel_sums_plan(Mx: int, Ny: int):
    """(64-query blocks, key-range splits) of the grid clipk_kernel_sums launches: that of clipk_sim_lse_bias."""
    return sim_lse_bias_plan(Mx, Ny)


def kernel_sums(x, y, gammas, weights, nx=None, ny=None, diag_offset=-1, want_sum=True, want_bary=False):
    """Row sums over the Gaussian mixture K_ij = sum_b weights[b] exp(-gammas[b] d2_ij), d2_ij = max(nx_i + ny_j -
    2 <x_i, y_j>, 0) (include/clipk.h: clipk_kernel_sums): (ksum [Mx] = sum_j K_ij, kbary [Mx, P] = sum_j K_ij y_j), None
    for an output not wanted.  gammas, weights: f32 device vectors of B <= 8 entries, read by the kernel.  nx, ny: the
    squared norms, computed here when not given.  diag_offset >= 0: row i skips key i + diag_offset (0 for a cloud with
    itself); -1: nothing is skipped."""
    Mx, Ny, P = _cloud_args(x, y, KERNEL_SUMS_MAX_P)
    for name, t in (("gammas", gammas), ("weights", weights)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 device tensor")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-D tensor, got shape {tuple(t.shape)}")
    B = gammas.shape[0]
    if not 1 <= B <= KERNEL_SUMS_MAX_B or weights.shape[0] != B:
        raise ValueError(f"gammas and weights must have the same 1..{KERNEL_SUMS_MAX_B} entries, got {B} and "
                         f"{weights.shape[0]}")
    _f32_vectors((("nx", nx, Mx), ("ny", ny, Ny)))
    diag_offset = _diag_offset(diag_offset)
    if not (want_sum or want_bary):
        raise ValueError("no output wanted")
    _device_args("the kernel-sum kernel needs", x, y, gammas, weights, nx, ny)
    nx, ny = _sq_norms(x, y, nx, ny)
    dev = x.device
    ksum = torch.empty(Mx, dtype=torch.float32, device=dev) if want_sum else None
    kbary = torch.empty((Mx, P), dtype=torch.float32, device=dev) if want_bary else None
    _launch("kernel_sums", 2.0 * Mx * Ny * P * (2 if want_bary else 1),
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, gammas.data_ptr(), weights.data_ptr(), B, nx.data_ptr(), ny.data_ptr(),
             diag_offset, ptr(ksum), ptr(kbary)), (dev, "kernel_sums", Mx, Ny, P, B))
    return ksum, kbary


KMEANS_MAX_P = 512             # clipk_kmeans_step
KMEANS_MAX_K_FUSED = 64        # ... assignment and update in one launch
KMEANS_MAX_K = 65536           # ... with the labels given
KMEANS_MAX_N = 1 << 24         # ... the f32 counts are exact


def kmeans_step_plan(N: int, K: int):
    """(64-centroid blocks, point-range splits) of the grid clipk_kmeans_step launches: that of clipk_sim_lse_bias with
    the centroids as the queries and the points as the keys."""
    return sim_lse_bias_plan(K, N)


def kmeans_step(x, c, nc=None, labels=None):
    """One Lloyd iteration (include/clipk.h: clipk_kmeans_step): (labels int32 [N], best f32 [N], sums f32 [K, P],
    counts f32 [K]).  x [N, P], c [K, P] f32; nc [K]: the centroids' squared norms, computed here when not given (pass
    zeros for the cosine form).  labels=None (K <= 64): labels[i] = argmax_c 2 <x_i, c_c> - nc[c] with equal scores to
    the lower c, best[i] = that maximum, sums / counts of those labels - one launch.  labels int32 [N] (K <= 65536): sums
    and counts of the given labels; the labels are returned as they came and best is None."""
    N, K, P = _cloud_args(x, c, KMEANS_MAX_P)
    if N > KMEANS_MAX_N:
        raise ValueError(f"N = {N} is outside the kernel's limit (N <= {KMEANS_MAX_N})")
    kmax = KMEANS_MAX_K_FUSED if labels is None else KMEANS_MAX_K
    if K > kmax:
        raise ValueError(f"K = {K} is outside the kernel's limit (K <= {KMEANS_MAX_K_FUSED} without labels, "
                         f"K <= {KMEANS_MAX_K} with them)")
    _f32_vectors((("nc", nc, K),))
    if labels is not None:
        _int32_vector("labels", labels, N, x.device)
    _device_args("the k-means kernel needs", x, c, nc, labels)
    dev = x.device
    fused = labels is None
    if fused:
        if nc is None:
            nc = (c * c).sum(1)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        best = torch.empty(N, dtype=torch.float32, device=dev)
    else:
        best = None
    sums = torch.empty((K, P), dtype=torch.float32, device=dev)
    counts = torch.empty(K, dtype=torch.float32, device=dev)
    _launch("kmeans_step", 2.0 * N * min(K, 64) * P * (2 if fused else 1),
            (x.data_ptr(), N, c.data_ptr(), K, P, ptr(nc) if fused else None, None if fused else labels.data_ptr(),
             labels.data_ptr() if fused else None, ptr(best), sums.data_ptr(), counts.data_ptr()), (dev, "kmeans", N, K, P))
    return labels, best, sums, counts


LABEL_DIST_MAX_P = 512         # clipk_label_dist_sums
LABEL_DIST_MAX_G = 512         # ... labels per launch
LABEL_DIST_MAX_LABELS = 65536  # ops.label_dist_sums: in 512-label blocks, one walk each
LABEL_DIST_METRICS = ("euclidean", "sqeuclidean", "cosine")


def label_dist_sums_plan(Mx: int, Ny: int):
    """(64-query blocks, key-range splits) of the grid clipk_label_dist_sums launches: that of clipk_sim_lse_bias."""
    return sim_lse_bias_plan(Mx, Ny)


def label_dist_sums(x, y, labels, n_labels, metric="euclidean", nx=None, ny=None, diag_offset=-1):
    """Per-label distance sums (include/clipk.h: clipk_label_dist_sums): out f32 [Mx, n_labels] with out[i, g] = the sum
    of d(x_i, y_j) over the keys j with labels[j] == g.  x [Mx, P], y [Ny, P] f32, labels int32 [Ny]; a label outside
    [0, n_labels) belongs to no column.  metric: "euclidean" (sqrt(max(nx_i + ny_j - 2 <x_i, y_j>, 0))), "sqeuclidean"
    (without the root) or "cosine" (max(1 - <x_i, y_j>, 0): the caller passes unit rows, the norms are not read).  nx, ny:
    the squared norms, computed here when not given.  diag_offset >= 0: row i skips key i + diag_offset (0 for a cloud
    with itself, r0 for its rows [r0, r1) against the whole cloud); -1: nothing is skipped.
    n_labels > 512 (up to 65536) runs in 512-label blocks, and EACH BLOCK IS A FULL WALK over the Mx x Ny tiles."""
    Mx, Ny, P = _cloud_args(x, y, LABEL_DIST_MAX_P)
    _args.check_metric(metric, LABEL_DIST_METRICS)
    _args.int_in("n_labels", n_labels, 1, LABEL_DIST_MAX_LABELS, what=f"in [1, {LABEL_DIST_MAX_LABELS}]", type_error=True)
    _int32_vector("labels", labels, Ny, x.device)
    _f32_vectors((("nx", nx, Mx), ("ny", ny, Ny)))
    diag_offset = _diag_offset(diag_offset)
    _device_args("the label-distance kernel needs", x, y, labels, nx, ny)
    mode = LABEL_DIST_METRICS.index(metric)
    nx, ny = _sq_norms(x, y, nx, ny, wanted=metric != "cosine")
    dev = x.device
    blocks = []
    for g0 in range(0, n_labels, LABEL_DIST_MAX_G):
        G = min(LABEL_DIST_MAX_G, n_labels - g0)
        Gp = (G + 3) // 4 * 4
        lab = labels if g0 == 0 else labels - g0                 # the block's labels as its columns 0 .. G - 1
        out = torch.empty((Mx, Gp), dtype=torch.float32, device=dev)
        _launch("label_dist_sums", 2.0 * Mx * Ny * (P + Gp),
                (x.data_ptr(), Mx, y.data_ptr(), Ny, P, lab.data_ptr(), G, mode, ptr(nx), ptr(ny), diag_offset,
                 out.data_ptr()), (dev, "label_dist", Mx, Ny, P, G))
        blocks.append(out if Gp == G else out[:, :G])
    return blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1)


def label_kernel_sums(x, y, labels, n_labels, beta, shift=None, nx=None, ny=None, diag_offset=-1, want_out=True,
                      want_stats=True):
    """Per-label Gaussian masses (include/clipk.h: clipk_label_kernel_sums): (out, mass, sumsq, top, best) with
    out f32 [Mx, n_labels], out[i, g] = the sum of exp(-beta[i] (d_ij - shift[i])) over the keys j with labels[j] == g,
    d_ij = max(nx_i + ny_j - 2 <x_i, y_j>, 0); mass = sum_g out, sumsq = sum_g out^2, top int32 = arg max_g out (equal
    values: the lower g) and best = that value, [Mx] each.  want_out=False: out is None and the Mx x n_labels result is never
    written; want_stats=False: the four row statistics are None.  x [Mx, P], y [Ny, P] f32, labels int32 [Ny] (a label
    outside [0, n_labels) belongs to no column), n_labels <= 512: ONE walk - a caller with more labels walks once per
    512 and merges.  beta f32 [Mx] > 0 per row, shift f32 [Mx] or None (zeros); nx, ny: the squared norms, computed here
    when not given.  diag_offset as in label_dist_sums.  ops.cond_entropy_sums_plan reports the grid for Mx = Ny."""
    Mx, Ny, P = _cloud_args(x, y, LABEL_DIST_MAX_P)
    _args.int_in("n_labels", n_labels, 1, LABEL_DIST_MAX_G, what=f"in [1, {LABEL_DIST_MAX_G}]", type_error=True)
    if not (want_out or want_stats):
        raise ValueError("neither out nor the row statistics wanted")
    _int32_vector("labels", labels, Ny, x.device)
    if beta is None:
        raise TypeError("beta must be a float32 device tensor")
    _f32_vectors((("beta", beta, Mx), ("shift", shift, Mx), ("nx", nx, Mx), ("ny", ny, Ny)))
    diag_offset = _diag_offset(diag_offset)
    _device_args("the label-kernel walk needs", x, y, labels, beta, shift, nx, ny)
    nx, ny = _sq_norms(x, y, nx, ny)
    dev = x.device
    G, Gp = n_labels, (n_labels + 3) // 4 * 4
    out = torch.empty((Mx, Gp), dtype=torch.float32, device=dev) if want_out else None
    mass, sumsq, best = (torch.empty(Mx, dtype=torch.float32, device=dev) if want_stats else None for _ in range(3))
    top = torch.empty(Mx, dtype=torch.int32, device=dev) if want_stats else None
    _launch("label_kernel_sums", 2.0 * Mx * Ny * (P + Gp),
            (x.data_ptr(), Mx, y.data_ptr(), Ny, P, labels.data_ptr(), G, beta.data_ptr(), ptr(shift), nx.data_ptr(),
             ny.data_ptr(), diag_offset, ptr(out), ptr(mass), ptr(sumsq), ptr(top), ptr(best)),
            (dev, "label_dist", Mx, Ny, P, G))
    if want_out and Gp != G:
        out = out[:, :G]
    return out, mass, sumsq, top, best


TSNE_MAX_P = 512              # clipk_cond_entropy_sums, clipk_tsne_grad
TSNE_MAX_B = 8                 # ... candidate bandwidths per row and walk
TSNE_MIN_N = 3


def cond_entropy_sums_plan(N: int):
    """(64-query blocks, key-range splits) of the grid clipk_cond_entropy_sums launches: that of clipk_sim_lse_bias."""
    return sim_lse_bias_plan(N, N)


def tsne_grad_plan(N: int):
    """(64-query blocks, key-range splits) of the grid clipk_tsne_grad launches: that of clipk_sim_lse_bias."""
    return sim_lse_bias_plan(N, N)


def _tsne_cloud(x, vectors, others=()):
    """Operand checks of the t-SNE walks, before any launch.  vectors: (name, tensor or None, length)."""
    N, _, P = _cloud_args(x, x, TSNE_MAX_P)
    if N < TSNE_MIN_N:
        raise ValueError(f"N = {N} is outside the kernel's limit (N >= {TSNE_MIN_N})")
    _f32_vectors(vectors)
    _device_args("the t-SNE kernels need", x, *(v[1] for v in vectors), *others)
    return N, P


def _f32_matrix(name, t, shape):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 device tensor")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor of shape {tuple(shape)}, got {tuple(t.shape)}")


def cond_entropy_sums(x, betas=None, shift=None, nx=None, diag_offset=0, want_min=False, want_s0=True, want_s1=True):
    """One walk of the cloud x [N, P] against itself (include/clipk.h: clipk_cond_entropy_sums): (dmin [N], s0 [N, B],
    s1 [N, B]), None for an output not wanted.  betas f32 [N, B], B <= 8: per-row candidate bandwidths; betas=None asks
    for the row minimum dmin of d_ij alone.  s0 = sum_j exp(-betas t_ij), s1 = sum_j t_ij exp(-betas t_ij) with t_ij =
    d_ij - shift[i] (shift=None: zeros).  nx: the squared norms, computed here when not given.  diag_offset = 0 drops
    the pair (i, i) as a term; -1 keeps it."""
    if betas is None:
        B, want_min, want_s0, want_s1 = 0, True, False, False
    else:
        if not isinstance(betas, torch.Tensor) or betas.dtype != torch.float32:
            raise TypeError("betas must be a float32 device tensor")
        if betas.dim() != 2 or betas.shape[0] != x.shape[0] or not betas.is_contiguous():
            raise ValueError(f"betas must be a contiguous [N, B] tensor, got shape {tuple(betas.shape)}")
        B = betas.shape[1]
        if not 1 <= B <= TSNE_MAX_B:
            raise ValueError(f"betas must hold 1..{TSNE_MAX_B} candidates per row, got {B}")
        if not (want_s0 or want_s1):
            raise ValueError("betas given but neither s0 nor s1 wanted")
    N, P = _tsne_cloud(x, (("shift", shift, x.shape[0]), ("nx", nx, x.shape[0])), (betas,))
    diag_offset = _diag_offset(diag_offset)
    nx = _sq_norms(x, x, nx, nx)[0]
    dev = x.device
    dmin = torch.empty(N, dtype=torch.float32, device=dev) if want_min else None
    s0 = torch.empty((N, B), dtype=torch.float32, device=dev) if want_s0 else None
    s1 = torch.empty((N, B), dtype=torch.float32, device=dev) if want_s1 else None
    _launch("cond_entropy_sums", 2.0 * N * N * P,
            (x.data_ptr(), N, P, nx.data_ptr(), ptr(betas), B, ptr(shift), diag_offset, ptr(dmin), ptr(s0), ptr(s1)),
            (dev, "tsne", N, P, B))
    return dmin, s0, s1


def tsne_grad(x, y, beta, dmin, log_s0, nx=None, diag_offset=0, want_kl=False, out=None):
    """The row sums of one t-SNE gradient step (include/clipk.h: clipk_tsne_grad): rows f32 [N, 6] with want_kl, [N, 5]
    without - per row the attractive sum (2), the repulsive sum (2), sum_j w_ij and sum_j P_ij (log P_ij - log w_ij).
    x [N, P], y [N, 2] f32; beta, dmin, log_s0 [N] from the perplexity calibration."""
    N, P = _tsne_cloud(x, (("beta", beta, x.shape[0]), ("dmin", dmin, x.shape[0]), ("log_s0", log_s0, x.shape[0]),
                           ("nx", nx, x.shape[0])), (y, out))
    for name, t in (("beta", beta), ("dmin", dmin), ("log_s0", log_s0)):
        if t is None:
            raise TypeError(f"{name} must be a float32 device tensor")
    _f32_matrix("y", y, (N, 2))
    nc = 6 if want_kl else 5
    if out is not None:
        _f32_matrix("out", out, (N, nc))
    diag_offset = _diag_offset(diag_offset)
    nx = _sq_norms(x, x, nx, nx)[0]
    rows = torch.empty((N, nc), dtype=torch.float32, device=x.device) if out is None else out
    _launch("tsne_grad", 2.0 * N * N * P,
            (x.data_ptr(), N, P, nx.data_ptr(), beta.data_ptr(), dmin.data_ptr(), log_s0.data_ptr(), y.data_ptr(),
             diag_offset, int(want_kl), rows.data_ptr()), (x.device, "tsne", N, P, int(want_kl)))
    return rows


def tsne_update(rows, y=None, update=None, gains=None, alpha=1.0, momentum=0.8, lr=200.0, want_kl=False, want_gnorm=False,
                z=None):
    """The fixed-order reductions of tsne_grad's rows and, with y / update / gains [N, 2] (changed in place), the
    delta-bar-delta step (include/clipk.h: clipk_tsne_update).  Returns (z, kl, gnorm): device scalars Z = sum_i rows[i,
    4], the KL value (rows [N, 6] only) and the gradient's 2-norm, None where not wanted."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32:
        raise TypeError("rows must be a float32 device tensor")
    if rows.dim() != 2 or rows.shape[1] not in (5, 6) or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous [N, 5] or [N, 6] tensor, got shape {tuple(rows.shape)}")
    N, nc = rows.shape
    if N < TSNE_MIN_N:
        raise ValueError(f"N = {N} is outside the kernel's limit (N >= {TSNE_MIN_N})")
    if want_kl and nc != 6:
        raise ValueError("the KL value needs rows [N, 6] (tsne_grad with want_kl=True)")
    state = (y, update, gains)
    if any(t is not None for t in state):
        for name, t in zip(("y", "update", "gains"), state):
            _f32_matrix(name, t, (N, 2))
    _device_args("the t-SNE kernels need", rows, *state, z)
    dev = rows.device
    if z is None:
        z = torch.empty((), dtype=torch.float32, device=dev)
    else:
        _device_scalar("z", z)
    kl = torch.empty((), dtype=torch.float32, device=dev) if want_kl else None
    gnorm = torch.empty((), dtype=torch.float32, device=dev) if want_gnorm else None
    _launch("tsne_update", 0.0, (rows.data_ptr(), N, nc, float(alpha), float(momentum), float(lr), ptr(y), ptr(update),
                                 ptr(gains), z.data_ptr(), ptr(kl), ptr(gnorm)))
    return z, kl, gnorm


def ce_logits_lse(S, S2=None, columns=False, label_offset=0):
    """LSE over the rows (optionally of [S | S2]) or the columns of materialised f32 logits + the diagonal logit."""
    _need_cuda(S, S2)
    assert S.dtype == torch.float32 and S.dim() == 2 and S.stride(1) == 1
    M, N = S.shape
    N2 = 0 if S2 is None else S2.shape[1]
    if N2:
        assert S2.dtype == torch.float32 and S2.stride(1) == 1 and S2.shape[0] == M
    n = N if columns else M
    lse = torch.empty(n, dtype=torch.float32, device=S.device)
    pos = torch.empty(n, dtype=torch.float32, device=S.device)
    check(_lib().clipk_ce_logits_lse(S.data_ptr(), S.stride(0), M, N, ptr(S2) if N2 else None, S2.stride(0) if N2 else 0,
                                     N2, int(bool(columns)), label_offset, lse.data_ptr(), pos.data_ptr(), _stream()),
          "clipk_ce_logits_lse")
    return lse, pos


def ce_logits_bwd(S, S2, lse_row, lse_col, w_row, w_col, g, off_row=0, off_col=0):
    _need_cuda(S, S2, lse_row, lse_col, g)
    M, N = S.shape
    N2 = 0 if S2 is None else S2.shape[1]
    dS = torch.empty((M, N), dtype=torch.float32, device=S.device)
    dS2 = torch.empty((M, N2), dtype=torch.float32, device=S.device) if N2 else None
    check(_lib().clipk_ce_logits_bwd(S.data_ptr(), S.stride(0), M, N, ptr(S2) if N2 else None, S2.stride(0) if N2 else 0,
                                     N2, ptr(lse_row), ptr(lse_col), float(w_row), float(w_col), off_row, off_col,
                                     g.data_ptr(), dS.data_ptr(), dS.stride(0), ptr(dS2), dS2.stride(0) if N2 else 0,
                                     _stream()), "clipk_ce_logits_bwd")
    return dS, dS2


def transpose_scale_f32(x, scale=None):
    """scale[0] * x^T for a contiguous f32 [R, C] matrix (scale: device scalar tensor or None)."""
    _need_cuda(x, scale)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    R, Cc = x.shape
    out = torch.empty((Cc, R), dtype=torch.float32, device=x.device)
    check(_lib().clipk_transpose_scale_f32(x.data_ptr(), R, Cc, ptr(scale), out.data_ptr(), _stream()),
          "clipk_transpose_scale_f32")
    return out


_DROP_EPOCH = None


def set_dropout_epoch(epoch: Optional[torch.Tensor]) -> None:
    """Register (or, with None, clear) the device word every dropout site adds to its seed (clipk_set_dropout_epoch): int32 /
    uint32 tensor with one element, kept alive here while registered.  Used by training.GraphedTrainStep so that a replayed
    step draws new masks; eager code never needs it."""
    global _DROP_EPOCH
    if epoch is not None:
        _need_cuda(epoch)
        assert epoch.numel() == 1 and epoch.element_size() == 4 and epoch.dtype in (torch.int32, torch.uint32)
    check(_lib().clipk_set_dropout_epoch(0 if epoch is None else epoch.data_ptr()), "clipk_set_dropout_epoch")
    _DROP_EPOCH = epoch


def colsum_f32(x, out=None, accumulate=False):
    """out[c] (+)= sum_r x[r, c] (f32): bias gradients, written straight into `out` (e.g. a parameter's .grad)."""
    _need_cuda(x, out)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    if out is None:
        out, accumulate = torch.empty(x.shape[1], dtype=torch.float32, device=x.device), False
    check(_lib().clipk_colsum_f32(x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), int(accumulate), _stream()),
          "clipk_colsum_f32")
    return out


def gemm_wgrad_f32(dy, x, dw=None, dbias=None, accumulate=False, want_bias=True):
    """Parameter gradients of an exact-f32 Linear: dW[N, K] (+)= dy[M, N]^T @ x[M, K], db[N] (+)= dy.sum(0), one launch when
    M <= 64.  dw / dbias: write (accumulate: add) into these tensors, e.g. the parameters' .grad; otherwise new tensors
    (want_bias=False and no dbias: no bias gradient).  Returns (dw, dbias)."""
    _need_cuda(dy, x, dw, dbias)
    assert dy.dtype == torch.float32 and x.dtype == torch.float32 and dy.dim() == 2 and x.dim() == 2
    assert dy.shape[0] == x.shape[0]
    if dy.stride(1) != 1:
        dy = dy.contiguous()
    if x.stride(1) != 1:
        x = x.contiguous()
    M, N = dy.shape
    K = x.shape[1]
    fresh = dw is None
    if fresh:
        dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    if dbias is None and want_bias:
        assert fresh or not accumulate, "accumulate with a new dbias tensor"
        dbias = torch.empty(N, dtype=torch.float32, device=dy.device)
    assert dw.dtype == torch.float32 and dw.shape == (N, K) and dw.stride(1) == 1
    assert dbias is None or (dbias.dtype == torch.float32 and dbias.numel() == N and dbias.is_contiguous())
    acc = bool(accumulate and not fresh)
    if M > 64:                 # many rows: the tiled kernel (its wrapper pads odd leading dimensions) + the column reduce
        gemm_f32(dy, x, trans_a=True, trans_b=True, addend=dw if acc else None, out=dw)
        if dbias is not None:
            colsum_f32(dy.contiguous(), out=dbias, accumulate=acc)
        return dw, dbias
    lib = _lib()
    check(_timed("gemm_f32", 2.0 * M * N * K,
                 lambda: lib.clipk_gemm_wgrad_f32(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(),
                                                  dw.stride(0), ptr(dbias), M, N, K, int(acc), _stream()),
                 4.0 * (M * (N + K) + N * K * (2 if acc else 1))), "clipk_gemm_wgrad_f32")
    return dw, dbias


def gemm_f32(a, b, trans_a=False, trans_b=False, bias=None, addend=None, addend_scale=None, alpha=None, out=None):
    """Exact-f32 out[M, N] = alpha * opA(a) @ opB(b) (+ bias) (+ addend_scale * addend) on the tiled f32-MFMA kernel
    (alpha / addend_scale: 1-element device tensors).
    trans_a: a is stored [K, M];  trans_b: b is stored [K, N] (else [N, K], the nn.Linear layout).
    out: write into this [M, N] f32 tensor (row stride = its stride(0)); out may BE the addend (in-place accumulation:
    every element is read and written by the same thread)."""
    _need_cuda(a, b, bias, addend, addend_scale, alpha)
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 2 and b.dim() == 2
    if a.stride(1) != 1 or a.stride(0) % 4:
        a = a.contiguous()
    if b.stride(1) != 1 or b.stride(0) % 4:
        b = b.contiguous()
    K, M = (a.shape if trans_a else (a.shape[1], a.shape[0]))
    Kb, N = (b.shape if trans_b else (b.shape[1], b.shape[0]))
    assert K == Kb, (a.shape, b.shape, trans_a, trans_b)
    # float4 staging wants 16-byte aligned rows: zero-pad the stored rows of an operand with an odd leading dimension
    # (plumbing; M, N, K stay what they are, the kernel never reads the pad as data)
    if a.stride(0) % 4:
        a = torch.nn.functional.pad(a, (0, (-a.shape[1]) % 4))
    if b.stride(0) % 4:
        b = torch.nn.functional.pad(b, (0, (-b.shape[1]) % 4))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    else:
        assert out.shape == (M, N) and out.dtype == torch.float32 and out.stride(1) == 1 and out.device == a.device
    if addend is not None:
        assert addend.shape == (M, N) and addend.stride(1) == 1
    nb = 4.0 * (M * K + N * K + M * N * (2 if addend is not None else 1))     # operands once, output (+ addend) once
    lib = _lib()
    wsb = lib.clipk_gemm_f32_workspace(M, N, K, int(trans_a), int(trans_b))
    ws = workspace(wsb, a.device, "gemm_f32") if wsb else None
    check(_timed("gemm_f32", 2.0 * M * N * K,
                 lambda: lib.clipk_gemm_f32(a.data_ptr(), a.stride(0), int(trans_a), b.data_ptr(), b.stride(0),
                                            int(trans_b), M, N, K, ptr(alpha), ptr(bias), ptr(addend),
                                            addend.stride(0) if addend is not None else 0, ptr(addend_scale),
                                            out.data_ptr(), out.stride(0), ptr(ws), ws.numel() if ws is not None else 0,
                                            _stream()), nb), "clipk_gemm_f32")
    return out


def matmul_f32_nt(a, b):
    """a[M, K] @ b[N, K]^T in exact f32, any K."""
    return gemm_f32(a, b)


def gemm_f32_nt(x, w, bias=None, addend=None, addend_scale=None):
    """Exact-f32 out = x @ w.T (+ bias) (+ addend_scale * addend): the ICNN's Linear layers."""
    return gemm_f32(x, w, bias=bias, addend=addend, addend_scale=addend_scale)


# --------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, act=None, want_f32=True, want_bf16=False, want_stats=True):
    _need_cuda(x, gamma, beta)
    rows, cols = x.shape
    y32 = torch.empty((rows, cols), dtype=torch.float32, device=x.device) if want_f32 else None
    y16 = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if want_stats else None
    nbytes = rows * cols * (x.element_size() + (4 if want_f32 else 0) + (2 if want_bf16 else 0))
    check(_timed("layernorm_fwd", nbytes,
                 lambda: _lib().clipk_layernorm_fwd(x.data_ptr(), _dt(x), x.stride(0), gamma.data_ptr(), beta.data_ptr(),
                                                    float(eps), ACT[act], ptr(y32), ptr(y16), cols, ptr(mean),
                                                    ptr(rstd), rows, cols, _stream())), "clipk_layernorm_fwd")
    return y32, y16, mean, rstd


def layernorm_bwd_partial_shape(rows: int, cols: int):
    """(blocks, floats) of the per-block dgamma / dbeta partial rows clipk_layernorm_bwd leaves in its workspace."""
    nbytes = _lib().clipk_layernorm_bwd_workspace(rows, cols)
    return nbytes // (2 * cols * 4), nbytes // 4


def colreduce_batched(desc: torch.Tensor, n: int, max_cols: int) -> None:
    """Reduce the partial rows of n LayerNorm backwards in one launch (clipk_colreduce_batched; desc int64 [n, 6] on the
    device: partial rows, blocks, cols, dgamma, dbeta, accumulate)."""
    _need_cuda(desc)
    assert desc.dtype == torch.int64 and desc.is_contiguous() and desc.numel() >= 6 * n
    check(_lib().clipk_colreduce_batched(desc.data_ptr(), int(n), int(max_cols), _stream()), "clipk_colreduce_batched")


_COLRED_DESC = {}


def colreduce_entries(entries) -> None:
    """entries: (partial rows tensor, blocks, cols, dgamma, dbeta) per LayerNorm; dgamma / dbeta += column sums, one launch per
    device.  The descriptor table lives on the device and is cached by the pointers it holds (a captured step finds the table
    its warm-up built)."""
    by_dev = {}
    for e in entries:
        by_dev.setdefault(e[0].device, []).append(e)
    for dev, es in by_dev.items():
        rows = tuple((p.data_ptr(), int(b), int(c), g.data_ptr(), bt.data_ptr(), 1) for p, b, c, g, bt in es)
        desc = _COLRED_DESC.get((dev, rows))
        if desc is None:
            if len(_COLRED_DESC) > 32:
                _COLRED_DESC.clear()
            desc = _COLRED_DESC[(dev, rows)] = torch.tensor(rows, dtype=torch.int64).to(dev)
        keep_for_capture(desc)
        with torch.cuda.device(dev):
            colreduce_batched(desc, len(es), max(int(c) for _, _, c, _, _ in es))


def layernorm_bwd(dy, x, gamma, beta, mean, rstd, act=None, dx_add=None, want_f32=True, want_bf16=False,
                  dgamma=None, dbeta=None, accumulate=False, want_param_grads=True, dropout_bf16=None, part_out=None):
    """part_out (f32, >= layernorm_bwd_partial_shape(rows, cols)[1] elements): the kernel's workspace is THIS buffer and no
    parameter gradient is reduced - the caller reduces the partial rows left in it later (colreduce_batched)."""
    _need_cuda(dy, x, gamma, mean, rstd, part_out)
    rows, cols = x.shape
    dx32 = torch.empty((rows, cols), dtype=torch.float32, device=x.device) if want_f32 else None
    dx16 = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    if part_out is not None:
        want_param_grads = False
    if not want_param_grads:                               # input gradient only (transport maps in eval mode)
        dgamma = dbeta = None
    elif dgamma is None:
        dgamma = torch.empty(cols, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(cols, dtype=torch.float32, device=x.device)
        accumulate = False
    lib = _lib()
    nbytes = lib.clipk_layernorm_bwd_workspace(rows, cols)
    if part_out is not None:
        assert part_out.dtype == torch.float32 and part_out.is_contiguous() and part_out.numel() * 4 >= nbytes
        ws = part_out.view(torch.uint8) if part_out.dim() == 1 else part_out.reshape(-1).view(torch.uint8)
    else:
        ws = workspace(nbytes, x.device, "ln")
    nb = rows * cols * (dy.element_size() + x.element_size() + (dx_add.element_size() if dx_add is not None else 0) +
                        (4 if want_f32 else 0) + (2 if want_bf16 else 0))
    check(_timed("layernorm_bwd", nb,
                 lambda: lib.clipk_layernorm_bwd(dy.data_ptr(), _dt(dy), dy.stride(0), x.data_ptr(), _dt(x), x.stride(0),
                                                 gamma.data_ptr(), ptr(beta), mean.data_ptr(), rstd.data_ptr(), ACT[act],
                                                 ptr(dx_add), _dt(dx_add) if dx_add is not None else F32, ptr(dx32),
                                                 ptr(dx16), cols, ptr(dgamma),
                                                 ptr(dbeta), int(accumulate), rows, cols,
                                                 float(dropout_bf16[0]) if dropout_bf16 else 0.0,
                                                 (int(dropout_bf16[1]) & 0xFFFFFFFF) if dropout_bf16 else 0, ws.data_ptr(),
                                                 ws.numel(), _stream())), "clipk_layernorm_bwd")
    return dx32, dx16, dgamma, dbeta


def layernorm_bwd2(g, dy, a, gamma, beta, mean, rstd, act=None, dgamma=None, dbeta=None, accumulate=False):
    """Backward of layernorm_bwd (second order, f32; act in {None, "celu", "softplus"}): cotangent g of da ->
    (d_dy, d_a, d_gamma, d_beta).  See clipk_layernorm_bwd2."""
    _need_cuda(g, dy, a, gamma, mean, rstd)
    rows, cols = a.shape
    g, dy, a = g.contiguous(), dy.contiguous(), a.contiguous()
    assert g.dtype == dy.dtype == a.dtype == torch.float32
    d_dy, d_a = torch.empty_like(a), torch.empty_like(a)
    if dgamma is None:
        dgamma = torch.empty(cols, dtype=torch.float32, device=a.device)
        dbeta = torch.empty(cols, dtype=torch.float32, device=a.device)
        accumulate = False
    lib = _lib()
    nbytes = lib.clipk_layernorm_bwd_workspace(rows, cols)
    ws = workspace(nbytes, a.device, "ln")
    check(_timed("layernorm_bwd2", 5.0 * rows * cols * 4,
                 lambda: lib.clipk_layernorm_bwd2(g.data_ptr(), dy.data_ptr(), a.data_ptr(), a.stride(0), gamma.data_ptr(),
                                                  ptr(beta), mean.data_ptr(), rstd.data_ptr(), ACT[act], d_dy.data_ptr(),
                                                  d_a.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), int(accumulate),
                                                  rows, cols, ws.data_ptr(), nbytes, _stream())), "clipk_layernorm_bwd2")
    return d_dy, d_a, dgamma, dbeta


def meanpool_fused_supported(cols: int) -> bool:
    """Row widths clipk_layernorm_meanpool_fwd takes (its four partial rows must fit 64 KiB of LDS)."""
    return cols % 4 == 0 and (4 * cols + 4) * 4 <= 65536


def layernorm_meanpool_fwd(x, gamma, beta, eps, B, L, mask=None):
    """pooled[b] = mean over the valid rows l of LayerNorm(x[b * L + l]) in one pass (the normalised rows are never
    written).  x f32 / bf16 [B*L, cols]; mask u8 [B*L] (1 = valid) or None.  Returns pooled [B, cols], mean, rstd [B*L] and
    row_weight [B*L] (each row's weight in its sample's mean: what the backward needs)."""
    _need_cuda(x, gamma, beta, mask)
    rows, cols = x.shape
    assert rows == B * L and x.dtype in (torch.float32, torch.bfloat16) and x.stride(1) == 1
    pooled = torch.empty((B, cols), dtype=torch.float32, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    wrow = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_timed("layernorm_fwd", rows * cols * x.element_size(),
                 lambda: _lib().clipk_layernorm_meanpool_fwd(x.data_ptr(), _dt(x), x.stride(0), gamma.data_ptr(), beta.data_ptr(),
                                                             float(eps), ptr(mask), B, L, cols, pooled.data_ptr(),
                                                             mean.data_ptr(), rstd.data_ptr(), wrow.data_ptr(),
                                                             _stream())), "clipk_layernorm_meanpool_fwd")
    return pooled, mean, rstd, wrow


def layernorm_meanpool_bwd(dpooled, row_weight, x, gamma, mean, rstd, B, L, want_f32=True, want_bf16=False,
                           dgamma=None, dbeta=None, accumulate=False):
    """Backward of layernorm_meanpool_fwd: dx f32 and / or bf16 [B*L, cols], dgamma, dbeta."""
    _need_cuda(dpooled, row_weight, x, gamma, mean, rstd)
    rows, cols = x.shape
    assert rows == B * L and dpooled.shape == (B, cols) and dpooled.dtype == torch.float32 and dpooled.is_contiguous()
    dx32 = torch.empty((rows, cols), dtype=torch.float32, device=x.device) if want_f32 else None
    dx16 = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    if dgamma is None:
        dgamma = torch.empty(cols, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(cols, dtype=torch.float32, device=x.device)
        accumulate = False
    lib = _lib()
    ws = workspace(lib.clipk_layernorm_bwd_workspace(rows, cols), x.device, "ln")
    nb = rows * cols * (x.element_size() + (4 if want_f32 else 0) + (2 if want_bf16 else 0))
    check(_timed("layernorm_bwd", nb,
                 lambda: lib.clipk_layernorm_meanpool_bwd(dpooled.data_ptr(), row_weight.data_ptr(), B, L,
                                                          x.data_ptr(), _dt(x), x.stride(0), gamma.data_ptr(), mean.data_ptr(),
                                                          rstd.data_ptr(), ptr(dx32), ptr(dx16), cols, ptr(dgamma),
                                                          ptr(dbeta), int(accumulate), cols, ws.data_ptr(), ws.numel(),
                                                          _stream())), "clipk_layernorm_meanpool_bwd")
    return dx32, dx16, dgamma, dbeta


def l2norm_fwd(x, eps=1e-12):
    _need_cuda(x)
    rows, cols = x.shape
    y = torch.empty_like(x)
    n = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_lib().clipk_l2norm_fwd(x.data_ptr(), y.data_ptr(), n.data_ptr(), rows, cols, eps, _stream()), "clipk_l2norm_fwd")
    return y, n


def l2norm_bwd(dy, y, n, eps=1e-12):
    rows, cols = y.shape
    dx = torch.empty_like(y)
    check(_lib().clipk_l2norm_bwd(dy.data_ptr(), y.data_ptr(), n.data_ptr(), dx.data_ptr(), rows, cols, eps, _stream()),
          "clipk_l2norm_bwd")
    return dx


# --------------------------------------------------------------------------------------------------
def to_bf16(x: torch.Tensor) -> torch.Tensor:
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(_lib().clipk_cast_f32_to_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "clipk_cast_f32_to_bf16")
    return y


def to_f32(x: torch.Tensor) -> torch.Tensor:
    _need_cuda(x)
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(_lib().clipk_cast_bf16_to_f32(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "clipk_cast_bf16_to_f32")
    return y


def il_source_rows(n_rows: int, hd: int, il_rows: int) -> torch.Tensor:
    """int64 [n_rows]: the ORIGINAL row each row of a pair-interleaved copy holds (csrc/common.h il_src): within every
    head of `hd` rows of the first `il_rows` rows, copy row 2 j / 2 j + 1 = original row j / j + hd / 2."""
    r = torch.arange(n_rows, dtype=torch.int64)
    d = r % hd
    src = (r - d) + (d // 2) + (d % 2) * (hd // 2)
    return torch.where(r < il_rows, src, r)


def cast_transpose(w: torch.Tensor, want_w=True, want_wt=True, w_out=None, wt_out=None, il=(0, 0)):
    """il = (head rows, il_rows): the first il_rows rows of both copies in pair-interleaved head order (clipk.h)."""
    _need_cuda(w)
    rows, cols = w.shape
    wb = w_out if w_out is not None else (torch.empty((rows, cols), dtype=torch.bfloat16, device=w.device) if want_w else None)
    wt = wt_out if wt_out is not None else (torch.empty((cols, rows), dtype=torch.bfloat16, device=w.device) if want_wt else None)
    check(_lib().clipk_cast_transpose(w.data_ptr(), ptr(wb), ptr(wt), rows, cols, int(il[0]), int(il[1]), _stream()),
          "clipk_cast_transpose")
    return wb, wt


def cast_transpose_batched(desc: torch.Tensor):
    """desc: int64 [n, 7] device tensor of (w_ptr, wb_ptr, wt_ptr, rows, cols, il_hd, il_rows): all n weights in one launch."""
    _need_cuda(desc)
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 7 and desc.is_contiguous()
    check(_lib().clipk_cast_transpose_batched(desc.data_ptr(), desc.shape[0], _stream()), "clipk_cast_transpose_batched")


def act_fwd(x, act):
    y = torch.empty_like(x)
    check(_lib().clipk_act_fwd(x.data_ptr(), y.data_ptr(), ACT[act], x.numel(), _stream()), "clipk_act_fwd")
    return y


def act_bwd(dy, x, act):
    dx = torch.empty_like(x)
    check(_lib().clipk_act_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), ACT[act], x.numel(), _stream()), "clipk_act_bwd")
    return dx


def dact(dy, aux_bf16, act):
    """bf16( dy * act'(aux) )"""
    out = torch.empty(aux_bf16.shape, dtype=torch.bfloat16, device=aux_bf16.device)
    check(_lib().clipk_dact(dy.data_ptr(), _dt(dy), aux_bf16.data_ptr(), ACT[act], out.data_ptr(), aux_bf16.numel(),
                            _stream()), "clipk_dact")
    return out


def axpby_dev(a, b, s):
    """a + s * b with s a 1-element device tensor (a = None: s * b)."""
    y = torch.empty_like(b)
    check(_lib().clipk_axpby_dev(ptr(a), b.data_ptr(), s.data_ptr(), y.data_ptr(), b.numel(), _stream()),
          "clipk_axpby_dev")
    return y


# --------------------------------------------------------------------------------------------------
def _drop(dropout):
    return (float(dropout[0]), int(dropout[1]) & 0xFFFFFFFF) if dropout else (0.0, 0)


def _attn(entry, name, work, qkv, side, rope, B, L, H, D, tail, grads=None, packed=False):
    """The body the six attention wrappers share: asserts, outputs, the timed call.  entry: the C entry point; name / work:
    the kernel timer's; side: the key mask [B, L] (padded batch) or, packed, cu_seqlens int32 [B+1] with L the longest
    sequence and B unused; tail: the entry point's arguments after the geometry; grads: None (forward -> (out, lse)) or
    (out, dout, lse) (backward -> (dqkv, delta))."""
    dev = qkv.device
    if packed:
        assert side.dtype == torch.int32 and side.is_contiguous()
        rows = qkv.shape[0]
        dims, stat = (side.numel() - 1, rows, int(L), H, D), (H, rows)
    else:
        rows = B * L
        dims, stat = (B, L, H, D), (B, H, L)
    if grads is None:                  # (result first, then the statistic: the allocator's block choice follows the order)
        assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and qkv.shape == (rows, 3 * H * D)
        res = torch.empty(rows, H * D, dtype=torch.bfloat16, device=dev)      # sizes unpacked: cheaper to parse
        st = torch.empty(*stat, dtype=torch.float32, device=dev)
        ptrs = (res.data_ptr(), st.data_ptr())
    else:
        res = torch.empty_like(qkv)
        st = torch.empty(*stat, dtype=torch.float32, device=dev)
        ptrs = (grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), st.data_ptr(), res.data_ptr())
    cos, sin = rope if rope is not None else (None, None)
    fn, stream = getattr(_lib(), entry), _stream()
    check(_timed(name, work, lambda: fn(qkv.data_ptr(), ptr(side), ptr(cos), ptr(sin), *ptrs, *dims, *tail, stream)), entry)
    return res, st


def attn_fwd(qkv, B, L, H, D, key_mask=None, rope=None, q_scale=1.0, dropout=None):
    _need_cuda(qkv, key_mask)
    return _attn("clipk_attn_fwd", "attn_fwd", 4.0 * B * H * L * L * D, qkv, key_mask, rope, B, L, H, D,
                 (float(q_scale), *_drop(dropout)))


def rope_qk_(qkv, B, L, H, D, rope):
    """In-place RoPE of the q and k sections of qkv (then: attn_fwd(rope=None), attn_bwd(rope=..., prerotated=True))."""
    _need_cuda(qkv)
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and qkv.shape == (B * L, 3 * H * D)
    cos, sin = rope
    check(_lib().clipk_rope_qk(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, L, H, D, _stream()), "clipk_rope_qk")
    return qkv


def attn_fwd_rot_(qkv, B, L, H, D, rope, key_mask=None, q_scale=1.0):
    """rope_qk_ + attn_fwd(rope=None) in one call (one kernel for short heads): rotates q / k of `qkv` in place and
    returns (out, lse) computed from the rotated values; backward: attn_bwd(rope=..., prerotated=True)."""
    _need_cuda(qkv, key_mask)
    return _attn("clipk_attn_fwd_rot", "attn_fwd", 4.0 * B * H * L * L * D, qkv, key_mask, rope, B, L, H, D,
                 (float(q_scale),))


def attn_bwd(qkv, out, dout, lse, B, L, H, D, key_mask=None, rope=None, q_scale=1.0, prerotated=False, dropout=None):
    _need_cuda(qkv, out, dout, lse)
    return _attn("clipk_attn_bwd", "attn_bwd", 10.0 * B * H * L * L * D, qkv, key_mask, rope, B, L, H, D,
                 (float(q_scale), int(prerotated), *_drop(dropout)), (out, dout, lse))[0]


def attn_f32_fwd(qkv, B, L, H, D, key_mask=None, q_scale=1.0, dropout=None):
    """Exact-f32 self-attention (clipk_attn_f32_fwd): qkv f32 [B*L, 3*H*D] -> out f32 [B*L, H*D], lse f32 [B, H, L]."""
    _need_cuda(qkv, key_mask)
    assert qkv.dtype == torch.float32 and qkv.is_contiguous() and qkv.shape == (B * L, 3 * H * D)
    out = torch.empty((B * L, H * D), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
    check(_timed("attn_f32_fwd", 4.0 * B * H * L * L * D,
                 lambda: _lib().clipk_attn_f32_fwd(qkv.data_ptr(), ptr(key_mask), out.data_ptr(), lse.data_ptr(), B, L, H,
                                                   D, float(q_scale), *_drop(dropout), _stream())), "clipk_attn_f32_fwd")
    return out, lse


def attn_f32_bwd(qkv, out, dout, lse, B, L, H, D, key_mask=None, q_scale=1.0, dropout=None):
    _need_cuda(qkv, out, dout, lse, key_mask)
    assert qkv.dtype == torch.float32 and dout.dtype == torch.float32 and dout.is_contiguous() and out.is_contiguous()
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
    check(_timed("attn_f32_bwd", 14.0 * B * H * L * L * D,
                 lambda: _lib().clipk_attn_f32_bwd(qkv.data_ptr(), ptr(key_mask), out.data_ptr(), dout.data_ptr(),
                                                   lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, L, H, D,
                                                   float(q_scale), *_drop(dropout), _stream())), "clipk_attn_f32_bwd")
    return dqkv


def dropout_f32(x, dropout, addend=None):
    """x * keep / (1 - p) (+ addend) with the kernels' counter-based mask over x's row-major element index."""
    _need_cuda(x, addend)
    assert x.dtype == torch.float32 and x.is_contiguous() and (addend is None or (addend.is_contiguous() and
                                                                                  addend.shape == x.shape))
    y = torch.empty_like(x)
    p_, seed = _drop(dropout)
    check(_lib().clipk_dropout_f32(x.data_ptr(), ptr(addend), y.data_ptr(), x.numel(), p_, seed, _stream()),
          "clipk_dropout_f32")
    return y


def attn_varlen_fwd(qkv, cu_seqlens, max_len, H, D, rope=None, q_scale=1.0, dropout=None):
    """Packed variable-length self-attention: qkv bf16 [T, 3*H*D], cu_seqlens int32 [B+1] on the device."""
    _need_cuda(qkv, cu_seqlens)
    return _attn("clipk_attn_varlen_fwd", "attn_fwd", 0.0, qkv, cu_seqlens, rope, None, max_len, H, D,
                 (float(q_scale), *_drop(dropout)), packed=True)


def attn_varlen_fwd_rot_(qkv, cu_seqlens, max_len, H, D, rope, q_scale=1.0):
    """attn_fwd_rot_ for a packed batch (whole-head kernel, D in {16, 24, 32}, 128 < max_len <= 256): q / k of `qkv`
    are rotated in place; backward: attn_varlen_bwd(..., prerotated=True)."""
    _need_cuda(qkv, cu_seqlens)
    return _attn("clipk_attn_varlen_fwd_rot", "attn_fwd", 0.0, qkv, cu_seqlens, rope, None, max_len, H, D,
                 (float(q_scale),), packed=True)


def varlen_whole_head_applies(max_len: int, D: int) -> bool:
    """Shapes clipk_attn_varlen_fwd_rot accepts (the whole-head short-sequence kernels)."""
    return D in (16, 24, 32) and 128 < int(max_len) <= 256


def attn_varlen_bwd(qkv, out, dout, lse, cu_seqlens, max_len, H, D, rope=None, q_scale=1.0, dropout=None,
                    prerotated=False):
    _need_cuda(qkv, out, dout, lse, cu_seqlens)
    return _attn("clipk_attn_varlen_bwd", "attn_bwd", 0.0, qkv, cu_seqlens, rope, None, max_len, H, D,
                 (float(q_scale), int(bool(prerotated)), *_drop(dropout)), (out, dout, lse), packed=True)[0]


# --------------------------------------------------------------------------------------------------
def embed_fwd(ids, table, row_scale=None, mask=None, mask_token_id=-1):
    _need_cuda(ids, table)
    B, L = ids.shape
    d = table.shape[1]
    x = torch.empty((B * L, d), dtype=torch.float32, device=table.device)
    check(_lib().clipk_embed_fwd(ids.data_ptr(), table.data_ptr(), ptr(row_scale), ptr(mask), mask_token_id, x.data_ptr(),
                                 B, L, d, table.shape[0], _stream()), "clipk_embed_fwd")
    return x


def embed_bwd(ids, dx, dtable, row_scale=None, mask=None, mask_token_id=-1):
    B, L = ids.shape
    V, d = dtable.shape
    lib = _lib()
    nbytes = lib.clipk_embed_bwd_workspace(B, L, d, V)
    ws = workspace(nbytes, dx.device, "embed") if nbytes else None
    check(lib.clipk_embed_bwd(ids.data_ptr(), dx.data_ptr(), ptr(row_scale), ptr(mask), mask_token_id,
                              dtable.data_ptr(), B, L, d, V, ptr(ws), ws.numel() if ws is not None else 0, _stream()),
          "clipk_embed_bwd")
    return dtable


def pool_fwd(x, B, L, mask=None, mode=1):
    d = x.shape[-1]
    y = torch.empty((B, d), dtype=torch.float32, device=x.device)
    check(_lib().clipk_pool_fwd(x.data_ptr(), ptr(mask), y.data_ptr(), B, L, d, mode, _stream()), "clipk_pool_fwd")
    return y


def pool_bwd(dy, B, L, mask=None, mode=1):
    d = dy.shape[-1]
    dx = torch.empty((B * L, d), dtype=torch.float32, device=dy.device)
    check(_lib().clipk_pool_bwd(dy.data_ptr(), ptr(mask), dx.data_ptr(), B, L, d, mode, _stream()), "clipk_pool_bwd")
    return dx


def pool_varlen_fwd(x, cu_seqlens, mode=1):
    _need_cuda(x, cu_seqlens)
    B, d = cu_seqlens.numel() - 1, x.shape[-1]
    y = torch.empty((B, d), dtype=torch.float32, device=x.device)
    check(_lib().clipk_pool_varlen_fwd(x.data_ptr(), cu_seqlens.data_ptr(), y.data_ptr(), B, d, mode, _stream()),
          "clipk_pool_varlen_fwd")
    return y


def pool_varlen_bwd(dy, cu_seqlens, T, mode=1):
    _need_cuda(dy, cu_seqlens)
    B, d = dy.shape
    dx = torch.empty((T, d), dtype=torch.float32, device=dy.device)
    check(_lib().clipk_pool_varlen_bwd(dy.data_ptr(), cu_seqlens.data_ptr(), dx.data_ptr(), B, d, mode, _stream()),
          "clipk_pool_varlen_bwd")
    return dx


# --------------------------------------------------------------------------------------------------
def sumsq(g: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _need_cuda(g)
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=g.device)
    lib = _lib()
    ws = workspace(lib.clipk_sumsq_workspace(g.numel()), g.device, "sumsq")
    check(lib.clipk_sumsq(g.data_ptr(), g.numel(), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "clipk_sumsq")
    return out


def adamw_step(w, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_norm_sq=None, max_norm=0.0,
               grad_scale=1.0, w_bf16=None, hyper=None):
    """hyper: device f32 [3] = {lr, 1 - beta1^t, sqrt(1 - beta2^t)} read by the kernel instead of lr / step (graph replay)."""
    _need_cuda(w, g, m, v, hyper)
    check(_lib().clipk_adamw_step(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(w_bf16), w.numel(),
                                  float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                  ptr(grad_norm_sq), float(max_norm), float(grad_scale), ptr(hyper), _stream()),
          "clipk_adamw_step")
