"""Gradient clipping, the fused clip + Adam update and the step guards (csrc/optim.hip)."""
import ctypes

import torch

from .._lib import check, lib
from ._base import _need_cuda, _ptr, _stream


def clip_grad_norm_(parameters, max_norm):
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (interfaces.py:454-458, 826-833) as three HIP launches per 96
    gradient tensors (``wcmc_grad_norm_clip``); returns the total norm before clipping as a 0-d device tensor."""
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros(())
    _need_cuda(*grads)
    grads = [g if g.is_contiguous() else None for g in grads]
    if any(g is None for g in grads):
        raise RuntimeError("clip_grad_norm_: gradients must be contiguous")
    if len(grads) > 96:
        # (more tensors than one table holds: norms of the groups first, then one common factor -- not needed by any model here)
        raise NotImplementedError("clip_grad_norm_: more than 96 gradient tensors")
    m = len(grads)
    numel = (ctypes.c_int64 * m)(*[g.numel() for g in grads])
    nbytes = lib().wcmc_grad_norm_clip_workspace_bytes(m, numel)
    ws = torch.empty((nbytes + 3) // 4, device=grads[0].device, dtype=torch.float32)
    out = torch.empty(2, device=grads[0].device, dtype=torch.float32)
    check(lib().wcmc_grad_norm_clip(m, (ctypes.c_void_p * m)(*[g.data_ptr() for g in grads]), numel, float(max_norm), _ptr(out),
                                    _ptr(ws), ws.numel() * 4, _stream()), "grad_norm_clip")
    return out[0]


# ------------------------------------------------------------------------ optimiser
def clip_adam_(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, clip=1.0,
               grad_scale=1.0, guard=None):
    """In-place fused clip_grad_value_ + Adam over flat fp32 buffers (no-op when the device float
    ``guard`` is 0)."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq, guard)
    check(lib().wcmc_clip_adam(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                               clip, lr, beta1, beta2, eps, int(step), grad_scale, _ptr(guard), _stream()),
          "clip_adam")


def clip_adam_hyper(step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """The seven per-step floats of ``clip_adam_dev_`` (host arithmetic of ``wcmc_clip_adam``; no GPU call)."""
    out = (ctypes.c_float * 7)()
    lib().wcmc_clip_adam_hyper(float(lr), float(beta1), float(beta2), float(eps), int(step), out)
    return list(out)


def clip_adam_dev_(param, grad, exp_avg, exp_avg_sq, hyper, clip=1.0, grad_scale=1.0, guard=None):
    """``clip_adam_`` with its per-step scalars read from the device tensor ``hyper`` (7 floats, ``clip_adam_hyper``): the
    form a hipGraph can replay with other values every step."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq, hyper, guard)
    assert hyper.numel() >= 7 and hyper.is_contiguous()
    check(lib().wcmc_clip_adam_dev(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), clip,
                                   grad_scale, _ptr(hyper), _ptr(guard), _stream()), "clip_adam_dev")


def step_guard_(losses, ok, sums, flags):
    """``wcmc_step_guard``: flags[i] = isfinite(losses[i]), flags[n] = guard = all finite and ok; ok <- guard; sums[i] += losses[i]
    under the guard.  losses: 0-d fp32 device tensors; ok (1), sums (n), flags (n + 1): fp32 device tensors."""
    n = len(losses)
    _need_cuda(ok, sums, flags, *losses)
    assert sums.numel() == n and flags.numel() == n + 1 and sums.is_contiguous() and flags.is_contiguous()
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in losses])
    check(lib().wcmc_step_guard(arr, n, _ptr(ok), _ptr(sums), _ptr(flags), _stream()), "step_guard")


def step_guard_local_(losses, ok, flags, flag_slot):
    """``wcmc_step_guard_local`` (multi-rank tail, graph A): flags[i] = isfinite(losses[i]); flag_slot[0] = 1 - (all finite and ok)."""
    n = len(losses)
    _need_cuda(ok, flags, flag_slot, *losses)
    assert flags.numel() == n + 1 and flags.is_contiguous()
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in losses])
    check(lib().wcmc_step_guard_local(arr, n, _ptr(ok), _ptr(flags), _ptr(flag_slot), _stream()), "step_guard_local")


def step_guard_global_(losses, flag_slot, ok, sums, flags):
    """``wcmc_step_guard_global`` (multi-rank tail, graph B): guard = (flag_slot[0] == 0) -> flags[n], ok; sums[i] += losses[i] under it."""
    n = len(losses)
    _need_cuda(ok, sums, flags, flag_slot, *losses)
    assert sums.numel() == n and flags.numel() == n + 1
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in losses])
    check(lib().wcmc_step_guard_global(arr, n, _ptr(flag_slot), _ptr(ok), _ptr(sums), _ptr(flags), _stream()), "step_guard_global")
