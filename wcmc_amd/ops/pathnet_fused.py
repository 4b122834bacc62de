"""PathNet.embedding and PathNet.final as one launch per direction (csrc/pathnet_fused.hip), and the chain entries that choose
between the fused nodes and the layer-by-layer chains of conv_split.py (``cat_upsample_chain`` is here for its fall-back onto
``cat_broadcast_chain``)."""
import torch

from .. import ops as _sw          # the package itself: switches and rebound state are read there, when a function runs
from .._lib import check, lib
from ._base import _Timed, _as_nhwc_nograd, _need_cuda, _ptr, _stream, _v, as_nhwc, is_nhwc_view, nhwc_empty, to_nhwc_raw
from .conv_split import (_CatBroadcastChainX, _CatUpsampleChainX, _ChainSppMeanX, _pack_chain_x, _split_shared,
                         conv_chain, presplit_shared, split_from_nchw_raw)
from .elementwise import cat_broadcast, spp_mean, upsample2
from .grads import _sink


def _dense_pixel_stride(g):
    """Pixel stride (floats) of an NHWC view whose pixels form one dense run (rows and images back to back), else None."""
    n, c, h, w = g.shape
    sn, sc, sh, sw = g.stride()
    if sc == 1 and sw >= c and sw % 4 == 0 and sh == w * sw and (n == 1 or sn == h * sh) and g.data_ptr() % 16 == 0:
        return sw
    return None


def embed_in_place_supported(x, widths=(64, 64, 64)):
    """True when the fused embedding chain (layer widths ``widths``) will read the channel-first fp32 tensor `x` where it lies
    (the ``x_nchw`` form of ``wcmc_embed3_mean_fwd`` / ``_bwd``): the switches, the mode, the chain's channel counts and ``wcmc_embed3_nchw_supported`` on x's shape
    and strides.  Launches nothing and needs no device."""
    if not (_sw.EMBED_IN_PLACE and _sw.FUSE_EMBED and _sw.DEBUG_ACTS is None and _sw.reduced_backward()):
        return False
    if x.dim() != 4 or x.dtype != torch.float32 or x.requires_grad or x.data_ptr() % 4:
        return False
    n, c, h, w = x.shape
    return bool(lib().wcmc_embed3_supported(c, *widths) and lib().wcmc_embed3_nchw_supported(c, n, h, w, *x.stride()))


def embed_in_place(x, widths=(64, 64, 64)):
    """Tag the channel-first tensor `x` so that ``conv_chain_spp_mean(x, ...)`` reads it in place -- the counterpart of
    ``presplit_shared``, which it falls back on where ``embed_in_place_supported`` says no.  Returns x."""
    if embed_in_place_supported(x, widths):
        x._wcmc_in_place = x._version
        return x
    return presplit_shared(x)


def _reads_in_place(x):
    """`x` carries a valid in-place tag (and no split copy, which would be read instead)."""
    return (_sw.EMBED_IN_PLACE and getattr(x, "_wcmc_in_place", None) == x._version and getattr(x, "_wcmc_split", None) is None
            and embed_in_place_supported(x))


class _EmbedSppMeanFusedX(torch.autograd.Function):
    """``y = chain3(x); m = y.view(B,S,...).mean(1)`` (networks.py:33-36) with the three 1x1 layers in ONE launch
    (``wcmc_embed3_fwd``) and a backward that recomputes the hidden activations (``wcmc_embed3_bwd``): nothing but x, y and
    the two gradients of y ever touches HBM.  x: an NHWC view or a tensor with its split attached (``_split_shared``), or a
    channel-first tensor tagged by ``embed_in_place``, which both launches read where it lies (their ``x_nchw`` argument)."""

    @staticmethod
    def forward(ctx, x, s, *params):
        _need_cuda(x, *params)
        in_place = _reads_in_place(x)
        xs = x.detach() if in_place else _split_shared(x)
        n, cin, h, w = x.shape
        ws_ = [params[0], params[2], params[4]]
        packs = _pack_chain_x(ws_, 1)                        # [(forward, data-gradient orientation)] per layer
        y = torch.empty((n, h, w, 64), device=x.device, dtype=torch.float32).permute(0, 3, 1, 2)
        m = nhwc_empty(n // s, 64, h, w, y.device)
        wb = (_ptr(packs[0][0]), _ptr(params[1].detach()), _ptr(packs[1][0]), _ptr(params[3].detach()), _ptr(packs[2][0]),
              _ptr(params[5].detach()))
        # the source, as (x_split, x_nchw, sample stride, channel stride), and the floats per pixel the launches read of it
        src = (_ptr(None), _ptr(xs), xs.stride(0), xs.stride(1)) if in_place else (_ptr(xs), _ptr(None), 0, 0)
        xf = cin if in_place else (cin + 7) // 8 * 8
        if in_place or lib().wcmc_embed3_mean_supported(s, h * w):          # (in place: HW % 64 == 0)
            # the mean leaves with y (the kernel walks the S samples of a pixel tile and keeps their sum in registers)
            with _Timed("embed3_fwd", 4.0 * n * h * w * (xf + 64 + 64 // s), "byte"):
                check(lib().wcmc_embed3_mean_fwd(*src, n * h * w, cin, *wb, _ptr(y), _ptr(m), s, h * w, _stream()), "embed3_mean_fwd")
        else:
            with _Timed("embed3_fwd", 4.0 * n * h * w * (xf + 64), "byte"):
                check(lib().wcmc_embed3_fwd(_ptr(xs), n * h * w, cin, *wb, _ptr(y), _stream()), "embed3_fwd")
            check(lib().wcmc_spp_reduce(*_v(y), *_v(m), n // s, s, h, w, 64, 1.0 / s, _stream()), "spp_reduce")
        ctx.s, ctx.dims, ctx.in_place = s, (n, cin, h, w), in_place
        ctx.packs = packs
        ctx.save_for_backward(xs, *params)
        return y, m

    @staticmethod
    def backward(ctx, gy, gm):
        s = ctx.s
        n, cin, h, w = ctx.dims
        xs, w0, b0, w1, b1, w2, b2 = ctx.saved_tensors
        gy = _as_nhwc_nograd(gy) if gy is not None else None
        gm = _as_nhwc_nograd(gm) if gm is not None else None
        if gy is not None and _dense_pixel_stride(gy) is None:
            gy = to_nhwc_raw(gy)
        if gm is not None and _dense_pixel_stride(gm) is None:
            gm = to_nhwc_raw(gm)
        dev = xs.device
        sk = lambda t: _sink(t.data_ptr() if isinstance(t, torch.nn.Parameter) else 0, t.shape, dev)
        dw0, dw1, dw2, db0, db1, db2 = sk(w0), sk(w1), sk(w2), sk(b0), sk(b1), sk(b2)
        nb = lib().wcmc_embed3_bwd_workspace_bytes()
        ws = torch.empty(nb // 4, device=dev, dtype=torch.float32)
        packs = ctx.packs
        src = (_ptr(None), _ptr(xs), xs.stride(0), xs.stride(1)) if ctx.in_place else (_ptr(xs), _ptr(None), 0, 0)
        xf = cin if ctx.in_place else (cin + 7) // 8 * 8
        with _Timed("embed3_bwd", 4.0 * n * h * w * (xf + 64 + (64 // s if gm is not None else 0)), "byte"):
            check(lib().wcmc_embed3_bwd(*src, n * h * w, cin, _ptr(packs[0][0]), _ptr(b0), _ptr(packs[1][0]), _ptr(b1), _ptr(packs[1][1]),
                                        _ptr(packs[2][1]), _ptr(gy), _dense_pixel_stride(gy) if gy is not None else 0, _ptr(gm),
                                        _dense_pixel_stride(gm) if gm is not None else 0, s, h * w, 1.0 / s, _ptr(dw0), _ptr(db0),
                                        _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(ws), nb, _stream()), "embed3_bwd")
        return (None, None, dw0, db0, dw1, db1, dw2, db2)


class _FinalFusedX(torch.autograd.Function):
    """``chain2(cat([flat, repeat_S(prop)], 1))`` (networks.py:39-42) as one launch per direction (``wcmc_final2_*``): the
    128-channel concatenation is never written.  Of the hidden activation the backward needs the bf16 hi plane only and of the
    output its sign: with ``ops.SAVE_FINAL_HIDDEN`` a forward that a backward will follow writes that plane ([M][128] bf16)
    beside the output and the backward reads both (``h_hi`` / ``out, h_hi`` of the two entries); otherwise nothing is kept and the
    backward recomputes the chain (null pointers there).  Same results bit for bit."""

    @staticmethod
    def forward(ctx, flat, prop, s, *params):
        _need_cuda(flat, prop, *params)
        bs, c1, h, w = flat.shape
        b = prop.shape[0]
        outc = params[2].shape[0]
        packs = _pack_chain_x([params[0], params[2]], 1)
        osz = 4 if outc <= 4 else 8                           # pixel stride of the output: round_up(outc, 4)
        buf = torch.empty((bs, h, w, osz), device=flat.device, dtype=torch.float32)
        hhi = None
        if _sw.SAVE_FINAL_HIDDEN and any(ctx.needs_input_grad):
            # h's hi plane: 128 bf16 = 64 floats' worth of bytes per pixel, written here and read once by the backward
            hhi = torch.empty((bs * h * w, 128), device=flat.device, dtype=torch.bfloat16)
        with _Timed("final2_fwd", 4.0 * bs * h * w * (64 + 64 // s + osz + (64 if hhi is not None else 0)), "byte"):
            check(lib().wcmc_final2_fwd(_ptr(flat), _dense_pixel_stride(flat), _ptr(prop), _dense_pixel_stride(prop), b, s, h * w,
                                        _ptr(packs[0][0]), _ptr(params[1].detach()), _ptr(packs[1][0]), _ptr(params[3].detach()), outc,
                                        _ptr(buf), _ptr(hhi), _stream()), "final2_fwd")
        # (buf through save_for_backward: its version counter guards the output the caller holds)
        saved = (hhi, buf) if hhi is not None else ()
        ctx.geom, ctx.packs = (b, s, h, w, outc), packs
        ctx.save_for_backward(flat, prop, *params, *saved)
        return buf.permute(0, 3, 1, 2)[:, :outc]

    @staticmethod
    def backward(ctx, g):
        b, s, h, w, outc = ctx.geom
        flat, prop, w0, b0, w1, b1, *saved = ctx.saved_tensors
        g = _as_nhwc_nograd(g)
        osz = 4 if outc <= 4 else 8
        if not (_dense_pixel_stride(g) == osz):
            g = to_nhwc_raw(g)
        dev = flat.device
        dy = torch.empty((b * s, h, w, 64), device=dev, dtype=torch.float32).permute(0, 3, 1, 2)
        dprop = nhwc_empty(b, 64, h, w, dev)
        sk = lambda t: _sink(t.data_ptr() if isinstance(t, torch.nn.Parameter) else 0, t.shape, dev)
        dw0, dw1, db0, db1 = sk(w0), sk(w1), sk(b0), sk(b1)
        nb = lib().wcmc_final2_bwd_workspace_bytes()
        ws = torch.empty(nb // 4, device=dev, dtype=torch.float32)
        packs = ctx.packs
        hhi, buf = saved if saved else (None, None)
        with _Timed("final2_bwd", 4.0 * b * s * h * w * (64 + 64 // s + osz + 64 + 64 // s + (64 + osz if saved else 0)), "byte"):
            check(lib().wcmc_final2_bwd(_ptr(flat), _dense_pixel_stride(flat), _ptr(prop), _dense_pixel_stride(prop), b, s, h * w,
                                        _ptr(packs[0][0]), _ptr(b0), _ptr(packs[1][0]), _ptr(b1), outc, _ptr(packs[0][1]), _ptr(packs[1][1]),
                                        _ptr(g), _ptr(buf), _ptr(hhi), _ptr(dy), _ptr(dprop), _ptr(dw0), _ptr(db0), _ptr(dw1), _ptr(db1),
                                        _ptr(ws), nb, _stream()), "final2_bwd")
        return (dy if ctx.needs_input_grad[0] else None, dprop if ctx.needs_input_grad[1] else None, None, dw0, db0, dw1, db1)


_UNFUSED_NOTED = set()


def _note_unfused(what, why):
    """A fused PathNet chain exists for the reference's shapes (support/networks.py:18-24) in the reduced-backward modes; another
    shape or mode runs the same arithmetic layer by layer in HIP -- correct, slower -- and says so once."""
    if (what, why) not in _UNFUSED_NOTED:
        _UNFUSED_NOTED.add((what, why))
        import warnings
        warnings.warn("wcmc_amd: %s runs layer by layer (no fused kernel for %s)" % (what, why), RuntimeWarning, stacklevel=3)


def conv_chain_spp_mean(x, s, ksize, pad, acts, params):
    """``y = conv_chain(x, ...); return y, spp_mean(y, s)``; one autograd node on the split-bf16 path."""
    # (DEBUG_ACTS: the parity tests' hook wants the hidden activations, which the fused chain never materialises)
    if (_sw.FUSE_EMBED and _sw.DEBUG_ACTS is None and ksize == 1 and pad == 0 and len(acts) == 3 and
            tuple(acts) == ("relu", "relu", "linear") and not x.requires_grad and x.is_cuda):
        if not _sw.reduced_backward():
            _note_unfused("PathNet.embedding", "precision mode %s" % _sw.PRECISION)
        elif not lib().wcmc_embed3_supported(params[0].shape[1], params[0].shape[0], params[2].shape[0], params[4].shape[0]):
            _note_unfused("PathNet.embedding", "channels %d -> %d -> %d -> %d" % (params[0].shape[1], params[0].shape[0],
                                                                                 params[2].shape[0], params[4].shape[0]))
        elif getattr(x, "_wcmc_split", None) is not None or is_nhwc_view(x) or _reads_in_place(x):
            return _EmbedSppMeanFusedX.apply(x, s, *params)
    if _sw.split_path() and acts[-1] == "linear":
        pre = getattr(x, "_wcmc_split", None)
        if (pre is None and getattr(x, "_wcmc_in_place", None) == x._version and not x.requires_grad and x.is_cuda
                and x.shape[1] <= 64 and x.shape[0] * x.shape[2] <= 65535):
            # tagged for in-place reading, but the layer-by-layer chain is the one that runs (a switch or the mode changed since):
            # its split is made now, for this call and this stream alone
            x = x.detach()
            x._wcmc_split = pre = ((x._version, None), split_from_nchw_raw(x))
        if pre is not None and pre[0] == (x._version, None) and not x.requires_grad:
            return _ChainSppMeanX.apply(x, s, (ksize, pad, tuple(acts)), *params)      # channel-first x, split attached
        return _ChainSppMeanX.apply(as_nhwc(x), s, (ksize, pad, tuple(acts)), *params)
    y = conv_chain(x, ksize, pad, acts, params)
    return y, spp_mean(y, s)


def cat_broadcast_chain(flat, prop, s, ksize, pad, acts, params):
    """``conv_chain(cat_broadcast(flat, prop, s), ...)``; fused into one autograd node on the split-bf16 path."""
    if (_sw.FUSE_FINAL and _sw.DEBUG_ACTS is None and ksize == 1 and pad == 0 and
            tuple(acts) == ("relu", "relu") and flat.is_cuda and prop.shape[0] * s == flat.shape[0]):
        if not _sw.reduced_backward():
            _note_unfused("PathNet.final", "precision mode %s" % _sw.PRECISION)
        elif not (lib().wcmc_final2_supported(flat.shape[1], prop.shape[1], params[0].shape[0], params[2].shape[0],
                                             flat.shape[2] * flat.shape[3]) and params[0].shape[1] == 128):
            _note_unfused("PathNet.final", "channels %d + %d -> %d -> %d at %d pixels per image" %
                          (flat.shape[1], prop.shape[1], params[0].shape[0], params[2].shape[0], flat.shape[2] * flat.shape[3]))
        else:
            fl, pr = as_nhwc(flat), as_nhwc(prop)
            if _dense_pixel_stride(fl) is not None and _dense_pixel_stride(pr) is not None:
                return _FinalFusedX.apply(fl, pr, s, *params)
    if _sw.split_path() and flat.shape[1] % 8 == 0:
        return _CatBroadcastChainX.apply(as_nhwc(flat), as_nhwc(prop), s, (ksize, pad, tuple(acts)), *params)
    return conv_chain(cat_broadcast(flat, prop, s), ksize, pad, acts, params)


def cat_upsample_chain(deep, skip, ksize, pad, acts, params):
    """``conv_chain(cat([upsample2(deep), skip], 1), ...)``; one autograd node on the split-bf16 path."""
    if _sw.split_path() and deep.shape[1] % 8 == 0:
        return _CatUpsampleChainX.apply(as_nhwc(deep), as_nhwc(skip), (ksize, pad, tuple(acts)), *params)
    return cat_broadcast_chain(upsample2(deep), skip, 1, ksize, pad, acts, params)
