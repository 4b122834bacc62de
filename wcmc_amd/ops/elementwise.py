"""Pooling, upsampling, concatenations and the per-sample glue of the U-Net, the PathNets and the interface (csrc/elementwise.hip)."""
import torch

from .._lib import check, lib
from ._base import _as_nhwc_nograd, _need_cuda, _ptr, _stream, _v, as_nhwc, nhwc_empty


# ------------------------------------------------------------------------ U-Net glue
class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, c, h, w = x.shape
        y = nhwc_empty(n, c, h // 2, w // 2, x.device)
        check(lib().wcmc_maxpool2_fwd(*_v(x), *_v(y), n, h, w, c, _stream()), "maxpool2_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        g = _as_nhwc_nograd(g)
        dx = nhwc_empty(n, c, h, w, x.device)
        check(lib().wcmc_maxpool2_bwd(*_v(x), *_v(g), *_v(dx), n, h, w, c, _stream()), "maxpool2_bwd")
        return dx


class _MaxPool2Skip(torch.autograd.Function):
    """``(x, maxpool2(x))`` as ONE node (a U-Net level: x feeds the skip connection, its pooled copy the level below): the two
    gradients of x arrive together and are summed inside the pooling backward's pass (``wcmc_maxpool2_bwd_add``) instead of by
    autograd's elementwise add -- one launch and one pass over the tensor less per level."""

    @staticmethod
    def forward(ctx, x):
        n, c, h, w = x.shape
        y = nhwc_empty(n, c, h // 2, w // 2, x.device)
        check(lib().wcmc_maxpool2_fwd(*_v(x), *_v(y), n, h, w, c, _stream()), "maxpool2_fwd")
        ctx.save_for_backward(x)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, g_skip, g_pool):
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        if g_pool is None:
            return g_skip
        g_pool = _as_nhwc_nograd(g_pool)
        dx = nhwc_empty(n, c, h, w, x.device)
        if g_skip is None:
            check(lib().wcmc_maxpool2_bwd(*_v(x), *_v(g_pool), *_v(dx), n, h, w, c, _stream()), "maxpool2_bwd")
        else:
            g_skip = _as_nhwc_nograd(g_skip)
            check(lib().wcmc_maxpool2_bwd_add(*_v(x), *_v(g_pool), *_v(g_skip), *_v(dx), n, h, w, c, _stream()), "maxpool2_bwd_add")
        return dx


def maxpool2_skip(x):
    """``(x, maxpool2(x))``: see ``_MaxPool2Skip``."""
    return _MaxPool2Skip.apply(as_nhwc(x))


class _Upsample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, c, h, w = x.shape
        y = nhwc_empty(n, c, 2 * h, 2 * w, x.device)
        check(lib().wcmc_upsample2_fwd(*_v(x), *_v(y), n, h, w, c, _stream()), "upsample2_fwd")
        return y

    @staticmethod
    def backward(ctx, g):
        n, c, h2, w2 = g.shape
        g = _as_nhwc_nograd(g)
        dx = nhwc_empty(n, c, h2 // 2, w2 // 2, g.device)
        check(lib().wcmc_upsample2_bwd(*_v(g), *_v(dx), n, h2 // 2, w2 // 2, c, _stream()), "upsample2_bwd")
        return dx


def maxpool2(x):
    return _MaxPool2.apply(as_nhwc(x))


def upsample2(x):
    return _Upsample2.apply(as_nhwc(x))


class _CatChannels(torch.autograd.Function):
    """cat([a, b], 1) into one NHWC buffer (channel counts multiples of 4); backward = two views."""

    @staticmethod
    def forward(ctx, a, b):
        n, ca, h, w = a.shape
        cb = b.shape[1]
        assert ca % 4 == 0, "concat offset must keep 16-byte alignment"
        out = nhwc_empty(n, ca + cb, h, w, a.device)
        out[:, :ca].copy_(a)      # strided device copies (plumbing, no arithmetic)
        out[:, ca:].copy_(b)
        ctx.ca = ca
        return out

    @staticmethod
    def backward(ctx, g):
        g = _as_nhwc_nograd(g)
        return g[:, :ctx.ca], g[:, ctx.ca:]


def cat_channels(a, b):
    return _CatChannels.apply(as_nhwc(a), as_nhwc(b))


# ------------------------------------------------------------------------ PathNet glue
class _SppMean(torch.autograd.Function):
    """(B*S,C,H,W) -> (B,C,H,W): mean over the S samples of a patch (networks.py:35-36)."""

    @staticmethod
    def forward(ctx, x, s):
        bs, c, h, w = x.shape
        b = bs // s
        y = nhwc_empty(b, c, h, w, x.device)
        check(lib().wcmc_spp_reduce(*_v(x), *_v(y), b, s, h, w, c, 1.0 / s, _stream()), "spp_reduce")
        ctx.s = s
        return y

    @staticmethod
    def backward(ctx, g):
        g = _as_nhwc_nograd(g)
        b, c, h, w = g.shape
        dx = nhwc_empty(b * ctx.s, c, h, w, g.device)
        check(lib().wcmc_spp_broadcast(*_v(g), *_v(dx), b, ctx.s, h, w, c, 1.0 / ctx.s, 0, _stream()),
              "spp_broadcast")
        return dx, None


def spp_mean(x, s):
    return _SppMean.apply(as_nhwc(x), s)


class _CatBroadcast(torch.autograd.Function):
    """cat([flat (B*S,C1), repeat_S(ctx (B,C2))], 1) without materialising the repeat twice
    (networks.py:39-40)."""

    @staticmethod
    def forward(ctx, flat, prop, s):
        bs, c1, h, w = flat.shape
        b, c2 = prop.shape[0], prop.shape[1]
        assert c1 % 4 == 0 and bs == b * s
        out = nhwc_empty(bs, c1 + c2, h, w, flat.device)
        out[:, :c1].copy_(flat)
        check(lib().wcmc_spp_broadcast(*_v(prop), *_v(out[:, c1:]), b, s, h, w, c2, 1.0, 0, _stream()),
              "spp_broadcast")
        ctx.dims = (b, s, c1, c2)
        return out

    @staticmethod
    def backward(ctx, g):
        b, s, c1, c2 = ctx.dims
        g = _as_nhwc_nograd(g)
        _, _, h, w = g.shape
        dprop = nhwc_empty(b, c2, h, w, g.device)
        check(lib().wcmc_spp_reduce(*_v(g[:, c1:]), *_v(dprop), b, s, h, w, c2, 1.0, _stream()), "spp_reduce")
        return g[:, :c1], dprop, None


def cat_broadcast(flat, prop, s):
    return _CatBroadcast.apply(as_nhwc(flat), as_nhwc(prop), s)


# ------------------------------------------------------------------------ interface glue
class _PBufferCat(torch.autograd.Function):
    """cat([base, P.mean(1), P.var(1).mean(1,keepdim).detach()/S], 1)  (interfaces.py:165-176)."""

    @staticmethod
    def forward(ctx, base, p):
        _need_cuda(base, p)
        b, s, cp, h, w = p.shape
        cb = base.shape[1]
        out = nhwc_empty(b, cb + cp + 1, h, w, p.device)
        check(lib().wcmc_pbuffer_cat_fwd(_ptr(base), *base.stride(), _ptr(p), *p.stride(), *_v(out),
                                         b, s, cb, cp, h, w, _stream()), "pbuffer_cat_fwd")
        ctx.dims = (b, s, cb, cp, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        b, s, cb, cp, h, w = ctx.dims
        g = _as_nhwc_nograd(g)
        dp = nhwc_empty(b * s, cp, h, w, g.device).unflatten(0, (b, s))
        check(lib().wcmc_pbuffer_cat_bwd(*_v(g), _ptr(dp), *dp.stride(), b, s, cb, cp, h, w, _stream()),
              "pbuffer_cat_bwd")
        return None, dp


def pbuffer_cat(base, p):
    out = _PBufferCat.apply(base, p)
    # the backward reads the gradient of channels [cb, cb + cp) only (the variance channel is detached, the base is data): a
    # conv chain that consumes `out` forms no more of its input gradient than that (conv_chain)
    out._wcmc_grad_channels = (base.shape[1], base.shape[1] + p.shape[2])
    return out


class _SampleCat(torch.autograd.Function):
    """cat([features, P, repeat_S(P.var(1).mean(1, keepdims).detach() / S)], 2) on (B,S,C,H,W) per-sample tensors
    (interfaces.py:394-403, 797-806)."""

    @staticmethod
    def forward(ctx, features, p):
        _need_cuda(features, p)
        b, s, c, h, w = features.shape
        cp = p.shape[2]
        assert p.shape[:2] == (b, s) and p.shape[3:] == (h, w)
        out = torch.empty((b, s, c + cp + 1, h, w), device=p.device, dtype=torch.float32)
        check(lib().wcmc_sample_cat_fwd(_ptr(features), *features.stride(), _ptr(p), *p.stride(), _ptr(out),
                                        b, s, c, cp, h, w, _stream()), "sample_cat_fwd")
        ctx.split = (c, cp)
        return out

    @staticmethod
    def backward(ctx, g):
        c, cp = ctx.split
        return g[:, :, :c], g[:, :, c:c + cp]


def sample_features_cat(features, p):
    return _SampleCat.apply(features, p)
