"""Kernel splatting and the per-image logit maximum (csrc/kernel_splat.hip)."""
import torch

from .._lib import check, lib
from ._base import _Timed, _as_nhwc_nograd, _need_cuda, _ptr, _stream, _v, as_nhwc, nhwc_empty

SPLAT_SOFTMAX, SPLAT_SHIFT = 0, 1


def _splat_dims(data, logits):
    if logits.dim() != 4 or data.dim() != 4:
        raise ValueError("kernel_splat: data and logits must be (N, C, h, w) and (N, k*k, h, w) (got %s and %s)"
                         % (tuple(data.shape), tuple(logits.shape)))
    n, k2, h, w = logits.shape
    c = data.shape[1]
    if data.shape[0] != n or tuple(data.shape[2:]) != (h, w):
        raise ValueError("kernel_splat: data %s and logits %s differ in batch or image size"
                         % (tuple(data.shape), tuple(logits.shape)))
    return n, c, h, w, k2


class _KernelSplat(torch.autograd.Function):
    """(sum_r, sum_w) of one splat; ``prev_r`` / ``prev_w``: sums to add into (out of place: the result is a copy of them plus
    the contribution, their gradient is the incoming gradient)."""

    @staticmethod
    def forward(ctx, data, logits, shift, prev_r, prev_w):
        _need_cuda(data, logits, shift, prev_r, prev_w)
        n, c, h, w, k2 = _splat_dims(data, logits)
        mode = SPLAT_SOFTMAX if shift is None else SPLAT_SHIFT
        if shift is not None:
            if tuple(shift.shape) != (n,):
                raise ValueError("kernel_splat: shift must be (N,) = (%d,) (got %s)" % (n, tuple(shift.shape)))
            shift = shift.detach().contiguous()
        if (prev_r is None) != (prev_w is None):
            raise ValueError("kernel_splat: into takes both sums, (sum_r, sum_w)")
        if prev_r is not None:
            if tuple(prev_r.shape) != (n, c, h, w) or tuple(prev_w.shape) != (n, h, w):
                raise ValueError("kernel_splat: into must be ((N, C, h, w), (N, h, w)) = (%s, %s) (got %s and %s)"
                                 % ((n, c, h, w), (n, h, w), tuple(prev_r.shape), tuple(prev_w.shape)))
            sum_r = prev_r.detach().clone(memory_format=torch.contiguous_format)
            sum_w = prev_w.detach().clone(memory_format=torch.contiguous_format)
        else:
            sum_r = torch.empty((n, c, h, w), device=logits.device, dtype=torch.float32)
            sum_w = torch.empty((n, h, w), device=logits.device, dtype=torch.float32)
        lse = torch.empty(n * h * w, device=logits.device, dtype=torch.float32) if mode == SPLAT_SOFTMAX else None
        nbytes = lib().wcmc_kernel_splat_fwd_workspace_bytes(n, c, h, w, k2)
        if nbytes == 0:
            check(-1, "kernel_splat_fwd")              # (the library's message names the unsupported argument)
        ws = torch.empty(nbytes // 4, device=logits.device, dtype=torch.float32)
        # algorithmic bytes: logits + radiance in, the C + 1 sums read and written
        with _Timed("kernel_splat_fwd", 4.0 * n * h * w * (k2 + c + 2 * (c + 1)), "byte"):
            check(lib().wcmc_kernel_splat_fwd(*_v(logits), _ptr(data), *data.stride(), _ptr(sum_r), _ptr(sum_w), _ptr(lse),
                                              mode, _ptr(shift), int(prev_r is not None), _ptr(ws), nbytes, n, c, h, w, k2,
                                              _stream()), "kernel_splat_fwd")
        ctx.save_for_backward(data, logits, shift, lse)
        ctx.mode, ctx.has_prev = mode, prev_r is not None
        ctx.set_materialize_grads(False)
        return sum_r, sum_w

    @staticmethod
    def backward(ctx, g_r, g_w):
        if g_r is None and g_w is None:
            return None, None, None, None, None
        data, logits, shift, lse = ctx.saved_tensors
        n, k2, h, w = logits.shape
        c = data.shape[1]
        dl = nhwc_empty(n, k2, h, w, logits.device)
        # (without g_r the gradient of data is zero: None)
        dd = torch.empty((n, c, h, w), device=logits.device, dtype=torch.float32) \
            if ctx.needs_input_grad[0] and g_r is not None else None
        gr_s = g_r.stride() if g_r is not None else (0, 0, 0, 0)
        gw_s = g_w.stride() if g_w is not None else (0, 0, 0)
        # algorithmic bytes: logits in + d_logits out + radiance and its gradient, the C + 1 incoming gradients
        with _Timed("kernel_splat_bwd", 4.0 * n * h * w * (2 * k2 + 3 * c + 1), "byte"):
            check(lib().wcmc_kernel_splat_bwd(*_v(logits), _ptr(data), *data.stride(), _ptr(g_r), *gr_s, _ptr(g_w), *gw_s,
                                              _ptr(lse), ctx.mode, _ptr(shift), *_v(dl), _ptr(dd), n, c, h, w, k2, _stream()),
                  "kernel_splat_bwd")
        return dd, dl, None, (g_r if ctx.has_prev else None), (g_w if ctx.has_prev else None)


def kernel_splat(data, logits, shift=None, into=None):
    """Splat ``data`` with per-source-pixel k x k kernels: ``(sum_r, sum_w)``, un-normalised.  ``shift=None``: the weights are a
    softmax over each source pixel's taps; else ``exp(logits - shift[n])`` with ``shift`` a device (N,) tensor that carries no
    gradient.  ``into=(prev_r, prev_w)``: the results are ``prev + contribution``."""
    _need_cuda(data, logits)
    _splat_dims(data, logits)
    prev_r, prev_w = into if into is not None else (None, None)
    return _KernelSplat.apply(data, as_nhwc(logits), shift, prev_r, prev_w)


def logit_max(logits):
    """``logits.amax(dim=(1, 2, 3))`` of (N, k*k, h, w) logits, detached: (N,).  A NaN logit gives NaN."""
    _need_cuda(logits)
    if logits.dim() != 4:
        raise ValueError("logit_max: logits must be (N, k*k, h, w) (got %s)" % (tuple(logits.shape),))
    lg = _as_nhwc_nograd(logits.detach())
    n, k2, h, w = lg.shape
    out = torch.empty(n, device=lg.device, dtype=torch.float32)
    ws = torch.empty(lib().wcmc_logit_max_workspace_bytes(n) // 4, device=lg.device, dtype=torch.float32)
    with _Timed("logit_max", 4.0 * n * h * w * k2, "byte"):
        check(lib().wcmc_logit_max(*_v(lg), _ptr(out), _ptr(ws), ws.numel() * 4, n, h, w, k2, _stream()), "logit_max")
    return out
