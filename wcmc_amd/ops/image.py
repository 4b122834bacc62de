"""Kernel apply (csrc/kernel_apply.hip), recombination, the image losses (pointwise, and the structural one of csrc/dssim_loss.hip)
and the full-frame evaluation (csrc/image_eval.hip)."""
import torch

from .._lib import check, lib
from ._base import _Timed, _need_cuda, _ptr, _stream, _v, as_nhwc, nhwc_empty
from .conv_split import conv_chain


# ------------------------------------------------------------------------ kernel apply
class _KernelApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, logits):
        _need_cuda(data, logits)
        n, k2, h, w = logits.shape
        k = int(round(k2 ** 0.5))
        c = data.shape[1]
        assert k * k == k2 and data.shape[0] == n and data.shape[2:] == logits.shape[2:]
        out = torch.empty((n, c, h, w), device=logits.device, dtype=torch.float32)
        lse = torch.empty(n * h * w, device=logits.device, dtype=torch.float32)
        # algorithmic bytes: logits + radiance in + result out (15.13 MB per 92x92 patch-branch)
        with _Timed("kernel_apply_fwd", 4.0 * n * h * w * (k2 + 2 * c), "byte"):
            check(lib().wcmc_kernel_apply_fwd(*_v(logits), _ptr(data), *data.stride(), _ptr(out), *out.stride(),
                                              _ptr(lse), n, c, h, w, k, _stream()), "kernel_apply_fwd")
        ctx.save_for_backward(data, logits, out, lse)
        ctx.k = k
        return out

    @staticmethod
    def backward(ctx, g):
        data, logits, out, lse = ctx.saved_tensors
        n, k2, h, w = logits.shape
        c = data.shape[1]
        dl = nhwc_empty(n, k2, h, w, logits.device)
        dd = torch.zeros((n, c, h, w), device=logits.device, dtype=torch.float32) \
            if ctx.needs_input_grad[0] else None
        # algorithmic bytes: logits in + d_logits out + radiance, result and its gradient in (30.06 MB / patch-branch)
        with _Timed("kernel_apply_bwd", 4.0 * n * h * w * (2 * k2 + 3 * c), "byte"):
            check(lib().wcmc_kernel_apply_bwd(*_v(logits), _ptr(data), *data.stride(), _ptr(out), *out.stride(),
                                              _ptr(g), *g.stride(), _ptr(lse), *_v(dl), _ptr(dd),
                                              n, c, h, w, ctx.k, _stream()), "kernel_apply_bwd")
        return dd, dl


def kernel_apply(data, logits):
    """softmax(k*k logits) applied as a zero-extended gather kernel over ``data``."""
    return _KernelApply.apply(data, as_nhwc(logits))


def chain_kernel_apply(x, data, ksize, pad, acts, params):
    """``kernel_apply(data, conv_chain(x, ...))`` with ``data`` already cropped to the chain's output size.  (Round 2 also had
    the two as ONE autograd node whose backward wrote d_logits straight into the chain's split gradient; it measured neutral
    -- 369-371 patches/s either way -- and was removed in round 3.)"""
    return kernel_apply(data, conv_chain(x, ksize, pad, acts, params))


class _Recombine(torch.autograd.Function):
    """radiance = albedo * r_diffuse + exp(r_specular) - 1 (albedo is data: no gradient)."""

    @staticmethod
    def forward(ctx, albedo, r_d, r_s):
        _need_cuda(albedo, r_d, r_s)
        n, c, h, w = r_d.shape
        out = torch.empty((n, c, h, w), device=r_d.device, dtype=torch.float32)
        check(lib().wcmc_recombine_fwd(_ptr(albedo), *albedo.stride(), _ptr(r_d), *r_d.stride(), _ptr(r_s),
                                       *r_s.stride(), _ptr(out), n, c, h, w, _stream()), "recombine_fwd")
        ctx.save_for_backward(albedo, r_s)
        return out

    @staticmethod
    def backward(ctx, g):
        albedo, r_s = ctx.saved_tensors
        n, c, h, w = r_s.shape
        g = g.contiguous()
        dd = torch.empty((n, c, h, w), device=g.device, dtype=torch.float32)
        ds = torch.empty((n, c, h, w), device=g.device, dtype=torch.float32)
        check(lib().wcmc_recombine_bwd(_ptr(g), _ptr(albedo), *albedo.stride(), _ptr(r_s), *r_s.stride(), _ptr(dd),
                                       _ptr(ds), n, c, h, w, _stream()), "recombine_bwd")
        return None, dd, ds


def recombine(albedo, r_diffuse, r_specular):
    return _Recombine.apply(albedo, r_diffuse, r_specular)


# ------------------------------------------------------------------------ image losses
def _image_loss_raw(x, ref, eps, want_l1, want_rel):
    _need_cuda(x, ref)
    assert x.shape == ref.shape and x.dim() == 4, (x.shape, ref.shape)
    n, c, h, w = x.shape
    ws = torch.empty(lib().wcmc_image_loss_workspace_bytes() // 4, device=x.device, dtype=torch.float32)
    l1 = torch.empty((), device=x.device, dtype=torch.float32) if want_l1 else None
    rel = torch.empty((), device=x.device, dtype=torch.float32) if want_rel else None
    check(lib().wcmc_image_loss_fwd(_ptr(x), *x.stride(), _ptr(ref), *ref.stride(), float(eps), _ptr(l1), _ptr(rel), _ptr(ws),
                                    ws.numel() * 4, n, c, h, w, _stream()), "image_loss_fwd")
    return l1, rel


class _L1Mean(torch.autograd.Function):
    """``torch.nn.L1Loss()(x, ref)`` (mean reduction; ref carries no gradient) as one pass + a one-block finish; the
    backward is one launch: ``g * sign(x - ref) / numel``."""

    @staticmethod
    def forward(ctx, x, ref):
        l1, _ = _image_loss_raw(x, ref, 0.0, True, False)
        ctx.save_for_backward(x, ref)
        return l1

    @staticmethod
    def backward(ctx, g):
        x, ref = ctx.saved_tensors
        n, c, h, w = x.shape
        dx = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
        g = g.contiguous()
        check(lib().wcmc_l1_mean_bwd(_ptr(x), *x.stride(), _ptr(ref), *ref.stride(), _ptr(g), _ptr(dx), n, c, h, w, _stream()),
              "l1_mean_bwd")
        return dx, None


def l1_mean(x, ref):
    """mean |x - ref| of two (N,C,H,W) tensors (any strides); differentiable in x."""
    return _L1Mean.apply(x, ref.detach())


def image_metrics(x, ref, eps=1e-2):
    """(L1 mean, RelativeMSE) of x against ref in one pass, no gradient (the logged ``l_total`` and ``rmse`` of a step,
    ``interfaces.py:240-249``)."""
    return _image_loss_raw(x.detach(), ref.detach(), eps, True, True)


def relative_mse(x, ref, eps=1e-2):
    """``support.losses.RelativeMSE`` without a gradient (validation, ``interfaces.py:296-300``)."""
    return _image_loss_raw(x.detach(), ref.detach(), eps, False, True)[1]


LOSS2_KINDS = {"smape": 0, "tonemapped_mse": 1, "tonemapped_relative_mse": 2}


class _ImageLoss2(torch.autograd.Function):
    """SMAPE / TonemappedMSE / TonemappedRelativeMSE (support/losses.py:267-320) of an (N,C,H,W) pair: one HIP pass + a one-block
    finish forward (``wcmc_image_loss2_fwd``), one pass backward (``wcmc_image_loss2_bwd``); ref carries no gradient."""

    @staticmethod
    def forward(ctx, x, ref, kind, eps):
        _need_cuda(x, ref)
        assert x.shape == ref.shape and x.dim() == 4, (x.shape, ref.shape)
        n, c, h, w = x.shape
        ws = torch.empty(lib().wcmc_image_loss_workspace_bytes() // 4, device=x.device, dtype=torch.float32)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        check(lib().wcmc_image_loss2_fwd(kind, _ptr(x), *x.stride(), _ptr(ref), *ref.stride(), float(eps), _ptr(loss), _ptr(ws),
                                         ws.numel() * 4, n, c, h, w, _stream()), "image_loss2_fwd")
        ctx.save_for_backward(x, ref)
        ctx.kind, ctx.eps = kind, float(eps)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, ref = ctx.saved_tensors
        n, c, h, w = x.shape
        dx = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
        g = g.contiguous()
        check(lib().wcmc_image_loss2_bwd(ctx.kind, _ptr(x), *x.stride(), _ptr(ref), *ref.stride(), ctx.eps, _ptr(g), _ptr(dx),
                                         n, c, h, w, _stream()), "image_loss2_bwd")
        return dx, None, None, None


def image_loss2(x, ref, kind, eps=1e-2):
    """kind: 'smape' | 'tonemapped_mse' | 'tonemapped_relative_mse'; differentiable in x."""
    return _ImageLoss2.apply(x, ref.detach(), LOSS2_KINDS[kind], eps)


DSSIM_TONEMAPS = {"none": 0, "reinhard": 1}


def dssim_loss_supported(n, c, h, w):
    """Does ``wcmc_dssim_loss_*`` take an (n, c, h, w) pair?  (A 7x7 window must fit; the planes must fit one grid.)"""
    return lib().wcmc_dssim_loss_workspace_bytes(n, c, h, w) > 0


class _DssimLoss(torch.autograd.Function):
    """1 - mean SSIM over every 7x7 window of every plane (csrc/dssim_loss.hip): one pass + a one-block finish
    forward, one pass backward that recomputes the per-window coefficients from the saved inputs; ref carries no gradient."""

    @staticmethod
    def forward(ctx, x, ref, tonemap, data_range):
        _need_cuda(x, ref)
        if x.dim() != 4 or x.shape != ref.shape:
            raise ValueError("dssim_loss: x and ref must be (N, C, H, W) of one size (got %s and %s)" % (tuple(x.shape), tuple(ref.shape)))
        if x.dtype != torch.float32 or ref.dtype != torch.float32:
            raise TypeError("dssim_loss: x and ref must be float32 (got %s and %s)" % (x.dtype, ref.dtype))
        n, c, h, w = x.shape
        nbytes = lib().wcmc_dssim_loss_workspace_bytes(n, c, h, w)
        ws = torch.empty(max(1, (nbytes + 7) // 8), device=x.device, dtype=torch.float64)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        check(lib().wcmc_dssim_loss_fwd(_ptr(x), *x.stride(), _ptr(ref), *ref.stride(), tonemap, float(data_range), _ptr(loss),
                                        _ptr(ws), nbytes, n, c, h, w, _stream()), "dssim_loss_fwd")
        ctx.save_for_backward(x, ref)
        ctx.tonemap, ctx.data_range = tonemap, float(data_range)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, ref = ctx.saved_tensors
        n, c, h, w = x.shape
        dx = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
        g = g.contiguous()
        check(lib().wcmc_dssim_loss_bwd(_ptr(x), *x.stride(), _ptr(ref), *ref.stride(), ctx.tonemap, ctx.data_range, _ptr(g), _ptr(dx),
                                        n, c, h, w, _stream()), "dssim_loss_bwd")
        return dx, None, None, None


def dssim_loss(x, ref, tonemap="reinhard", data_range=2.0):
    """1 - mean SSIM (7x7 uniform windows at valid positions, K1 0.01, K2 0.03, sample covariance) of two fp32 (N,C,H,W) tensors of
    any strides, H, W >= 7; differentiable in x.  tonemap: 'none' | 'reinhard' (``metrics._tonemap`` on both images).  With
    'reinhard', data_range 2 and one 3-channel frame this is the ``_tonemap`` DSSIM of ``image_eval``.  A shape the kernel refuses
    raises; NaN pixels give a NaN loss."""
    if tonemap not in DSSIM_TONEMAPS:
        raise ValueError("dssim_loss: tonemap %r is not one of %s" % (tonemap, sorted(DSSIM_TONEMAPS)))
    return _DssimLoss.apply(x, ref.detach(), DSSIM_TONEMAPS[tonemap], data_range)


# ------------------------------------------------------------------------------------------------- full-frame evaluation
def image_eval(out, ipt, tgt, has_hit=None, eps=1e-4):
    """The 40 image metrics of one denoised frame (``wcmc_image_eval``; test_models.py:234-251, support/metrics.py): a (2, 4, 5)
    fp64 device tensor [comparison (out vs tgt, ipt vs tgt)][tone map (linear, _tonemap, tonemap, tonemap28)][metric (RelMSE,
    RelL1, DSSIM, L1, MSE)].  out / ipt / tgt: fp32 (H, W, 3) device tensors of any strides (a channel-first frame passes as
    ``frame.permute(1, 2, 0)`` without a copy); has_hit: the same form or None -- out is taken from ipt wherever it is 0."""
    _need_cuda(out, ipt, tgt, has_hit)
    h, w = out.shape[:2]
    for t in (out, ipt, tgt) + ((has_hit,) if has_hit is not None else ()):
        if t.dim() != 3 or tuple(t.shape) != (h, w, 3):
            raise ValueError("image_eval: images must be (H, W, 3) of one size (got %s and %s)"
                             % (tuple(out.shape), tuple(t.shape)))
    if h < 7 or w < 7:
        raise ValueError("image_eval: the image is %d x %d; SSIM's 7x7 window needs at least 7 x 7" % (h, w))
    dev = out.device
    res = torch.empty((2, 4, 5), device=dev, dtype=torch.float64)
    nbytes = lib().wcmc_image_eval_workspace_bytes(h, w)
    ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
    hh = has_hit if has_hit is not None else None
    hs = hh.stride() if hh is not None else (0, 0, 0)
    check(lib().wcmc_image_eval(_ptr(out), *out.stride(), _ptr(ipt), *ipt.stride(), _ptr(tgt), *tgt.stride(), _ptr(hh), *hs,
                                h, w, float(eps), _ptr(res), _ptr(ws), ws.numel() * 8, _stream()), "image_eval")
    return res
