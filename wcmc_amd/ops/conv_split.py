"""The split-bf16 conv chains (csrc/conv_bf16x3.hip and the bf16x3_* units): split / pack primitives, the GEMM launches, the shared
chain forward / backward and the autograd nodes built on them."""
import ctypes

import torch

from .. import ops as _sw          # the package itself: switches and rebound state are read there, when a function runs
from .._lib import check, lib
from ._base import (ACT, LEAKY_SLOPE, _Timed, _as_nhwc_nograd, _need_cuda, _ptr, _stream, _timed_conv, _v, wgrad_launch_plan,
                    as_nhwc, nhwc_empty)
from .conv_fp32 import _ConvChain
from .grads import _flushed_by_consumer, _on_side_stream, _sink_ex
from .streams import _side_stream


# ---- split-bf16 chain ----------------------------------------------------------------------
def _split_empty(n, c, h, w, device):
    return torch.empty(lib().wcmc_split_elems(n, h, w, c), device=device, dtype=torch.int16)


def split_raw(x):
    """fp32 NHWC view -> dense split tensor (int16 storage of [N][H][W][2][round_up(C,8)] bf16)."""
    n, c, h, w = x.shape
    out = _split_empty(n, c, h, w, x.device)
    check(lib().wcmc_split_bf16(*_v(x), _ptr(out), n, h, w, c, _stream()), "split_bf16")
    return out


def split_from_nchw_raw(x):
    """Strided channel-first (N,C,H,W) fp32 -> split tensor in one pass (wcmc_split_from_nchw; C <= 64)."""
    n, c, h, w = x.shape
    out = _split_empty(n, c, h, w, x.device)
    check(lib().wcmc_split_from_nchw(_ptr(x), *x.stride(), _ptr(out), n, c, h, w, _stream()), "split_from_nchw")
    return out


def presplit_shared(x):
    """Attach the split form of the channel-first tensor `x` to it so that ``conv_chain_spp_mean(x, ...)`` consumes it
    directly -- on ANY stream that was forked after this call (the two PathNets embed the same `paths`, the second one on
    the forked specular stream: the split is made once, before the fork).  Returns x."""
    _need_cuda(x)
    x._wcmc_split = ((x._version, None), split_from_nchw_raw(x))
    return x


def split_gated_raw(dy, post, act):
    """split(dy * act'(post)) in one pass (wcmc_split_gated_bf16): act_backward_raw + split_raw."""
    n, c, h, w = dy.shape
    out = _split_empty(n, c, h, w, dy.device)
    check(lib().wcmc_split_gated_bf16(*_v(dy), *_v(post), ACT[act], LEAKY_SLOPE, _ptr(out), n, h, w, c, _stream()),
          "split_gated_bf16")
    return out


def split_dy_colsum_raw(dims, dy=None, post=None, act="linear", gm=None, s=1, scale=1.0):
    """``split((dy [+ repeat_S(gm) * scale]) [* act'(post)])`` and the per-block column sums of the result in one pass
    (wcmc_split_dy_colsum_bf16): the split gradient entering a chain's backward plus its last layer's bias-gradient
    partials.  dims = (N, C, H, W) of the result."""
    n, c, h, w = dims
    dev = (dy if dy is not None else gm).device
    out = _split_empty(n, c, h, w, dev)
    part = torch.empty(lib().wcmc_conv2d_igemm_colsum_elems(n, h, w, c), device=dev, dtype=torch.float32)
    z = (_ptr(None), 0, 0, 0)
    check(lib().wcmc_split_dy_colsum_bf16(*(_v(dy) if dy is not None else z), *(_v(post) if post is not None else z), ACT[act],
                                          LEAKY_SLOPE, *(_v(gm) if gm is not None else z), s, float(scale), _ptr(out), _ptr(part),
                                          n, h, w, c, _stream()), "split_dy_colsum_bf16")
    return out, part


def unsplit_debug(t, n, c, h, w):
    """split tensor -> fp32 (N,C,H,W) with torch ops; test / debug only."""
    cp = (c + 7) // 8 * 8
    v = t.view(torch.bfloat16).view(n, h, w, 2, cp).float()
    return (v[:, :, :, 0] + v[:, :, :, 1])[..., :c].permute(0, 3, 1, 2)


def _dgrad_mode(terms=None):
    """Packing mode of the data-gradient weights: 1 = three-term launch, 2 = the K order of a two-term launch (x hi plane only)."""
    return 2 if (_sw.dgrad_terms() if terms is None else terms) == 2 else 1


def _pack_x(weight, mode):
    """mode 0: forward orientation; 1 / 2: the data-gradient orientation for a three- / two-term launch (_dgrad_mode); 3: the
    forward orientation in the K order of a two- / one-term launch (an output layer of the "bf16x321o" mode)."""
    cout, cin, ks, _ = weight.shape
    rows, kch = (cout, cin) if mode in (0, 3, 4) else (cin, cout)
    wp = torch.empty(lib().wcmc_conv2d_packed_elems_bf16x3(rows, kch, ks, mode), device=weight.device, dtype=torch.int16)
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    check(lib().wcmc_conv2d_pack_weight_bf16x3(_ptr(w), _ptr(wp), cout, cin, ks, mode, _stream()),
          "pack_weight_bf16x3")
    return wp


# One packing launch per chain (all layers, both orientations: wcmc_conv2d_pack_chain_bf16x3) instead of two per layer:
# 114 launches per step become 16 (bit-identical to per-layer packing, which chains of more than 10 layers still take).


def _fwd_pack_mode(out_terms):
    """Packing mode of an output layer's forward weights: 0 (three terms), 3 (hi-plane K order: two / one bf16 term), 4 (fp16)."""
    return 4 if out_terms == "h" else 0 if out_terms == 3 else 3


PACK_MAX_ENTRIES = 32       # (layer, orientation) pairs per wcmc_conv2d_pack_chain_bf16x3 launch


def _pack_chains_x(chains, ks):
    """chains: [(weights, out_terms)] of filter size ks -> per chain [(wp_mode0, wp_mode1, (mode0, mode1))] per layer, ALL packed by
    ONE launch.  out_terms < 3: that chain's LAST layer's forward pack is made in the K order of a hi-plane launch (mode 3 / 4)."""
    assert sum(2 * len(w) for w, _ in chains) <= PACK_MAX_ENTRIES
    dev = chains[0][0][0].device
    ws, outs, couts, cins, modes, keep, res = [], [], [], [], [], [], []
    for weights, out_terms in chains:
        n = len(weights)
        dmode = _dgrad_mode(_sw.chain_terms(ks, weights[0].shape[1])[1])
        per = []
        for li, wt in enumerate(weights):
            w = wt.detach()
            if not w.is_contiguous():
                w = w.contiguous()
            keep.append(w)
            cout, cin = w.shape[0], w.shape[1]
            pair = []
            for mode in (_fwd_pack_mode(out_terms) if li == n - 1 else 0, dmode):
                rows, kch = (cout, cin) if mode in (0, 3, 4) else (cin, cout)
                wp = torch.empty(lib().wcmc_conv2d_packed_elems_bf16x3(rows, kch, ks, mode), device=dev, dtype=torch.int16)
                ws.append(w.data_ptr()); outs.append(wp.data_ptr()); couts.append(cout); cins.append(cin); modes.append(mode)
                pair.append(wp)
            per.append((pair[0], pair[1], (_fwd_pack_mode(out_terms) if li == n - 1 else 0, dmode)))
        res.append(per)
    m = len(ws)
    arr_p, arr_i = ctypes.c_void_p * m, ctypes.c_int * m
    check(lib().wcmc_conv2d_pack_chain_bf16x3(m, arr_p(*ws), arr_p(*outs), arr_i(*couts), arr_i(*cins), arr_i(*modes), ks,
                                              _stream()), "conv2d_pack_chain_bf16x3")
    return res


def _pack_chain_x(weights, ks, out_terms=3):
    """[(wp_mode0, wp_mode1)] of the OIHW weights of one chain, packed by ONE launch."""
    return [(a, b) for a, b, _ in _pack_chains_x([(weights, out_terms)], ks)[0]]


def _chain_out_terms(ks, act_last, cin_last, cout_last, pair):
    """MFMAs per product of a chain's output layer's forward (3, 1, or "h": one fp16 MFMA), as _chainx_forward decides it."""
    oterms = 3 if pair else _sw.out_layer_terms(ks, act_last)
    if oterms == "h" and not lib().wcmc_conv2d_out_f16_supported(cin_last, cout_last, ks):
        oterms = 3
    return oterms


def conv2d_x_raw(xs, dims, wp, bias, cout, ks, pad, act, out_split, gate=None, gate_act="linear", colsum=False,
                 gate_mask=None, mask_out=False, terms=3, out=None):
    """One split-bf16 implicit-GEMM launch.  xs: split tensor of dims (n,cin,h,w).
    terms: bf16 MFMAs per product -- 3, 2 = the hi plane of xs only (wp packed with mode 2: the data gradient of the
    "bf16x321" modes, whose xs is dy; or mode 3: a forward launch), 1 = the hi planes of xs and wp only (mode 3: the un-gated
    output layer of the "bf16x321o" mode).
    Returns a split tensor when out_split else an fp32 NHWC view; with colsum=True also the per-tile
    column sums of the result (the consumer layer's bias gradient, see colsum_finish_raw); with mask_out=True
    also the (hi plane > 0) bit mask of the result, which a later launch can take as gate_mask instead of
    re-reading the tensor as gate."""
    n, cin, h, w = dims
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    dev = xs.device
    if out_split:
        ysp, yf, yv = _split_empty(n, cout, ho, wo, dev), None, (_ptr(None), 0, 0, 0)
    else:
        # (out: an fp32 NHWC view of (n, cout, ho, wo) to write into -- e.g. a channel slice of a wider tensor)
        yf = nhwc_empty(n, cout, ho, wo, dev) if out is None else out
        assert tuple(yf.shape) == (n, cout, ho, wo)
        ysp, yv = None, _v(yf)
    part = None
    if colsum:
        part = torch.empty(lib().wcmc_conv2d_igemm_colsum_elems(n, ho, wo, cout), device=dev, dtype=torch.float32)
    mask = None
    if mask_out:
        mask = torch.empty(n * ho * wo * ((cout + 7) // 8), device=dev, dtype=torch.uint8)
    with _timed_conv(dims, cout, ks, pad, terms, yf, gate is not None):
        check(lib().wcmc_conv2d_igemm_bf16x3(_ptr(xs), n, h, w, cin, _ptr(wp), _ptr(bias), *yv, _ptr(ysp), cout,
                                             ks, pad, ACT[act], LEAKY_SLOPE, _ptr(gate), ACT[gate_act], LEAKY_SLOPE,
                                             _ptr(part), _ptr(gate_mask), _ptr(mask), terms, _stream()), "conv2d_igemm_bf16x3")
    out = ysp if out_split else yf
    ret = (out,) + ((part,) if colsum else ()) + ((mask,) if mask_out else ())
    return ret if len(ret) > 1 else out


def conv2d_out_f16_raw(xs, dims, wp16, bias, cout, ks, pad):
    """The forward of an un-gated 5x5 output layer with one fp16 MFMA per product (wcmc_split_to_f16 + wcmc_conv2d_out_f16): xs the
    split input of dims (n, cin, h, w), wp16 packed with mode 4; returns conv(x, W) + bias as an fp32 NHWC view."""
    n, cin, h, w = dims
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    x16 = torch.empty(lib().wcmc_split_to_f16_elems(n, h, w, cin), device=xs.device, dtype=torch.int16)
    check(lib().wcmc_split_to_f16(_ptr(xs), n, h, w, cin, _ptr(x16), _stream()), "split_to_f16")
    y = nhwc_empty(n, cout, ho, wo, xs.device)
    with _timed_conv(dims, cout, ks, pad, 1, y, False, f16=True):
        check(lib().wcmc_conv2d_out_f16(_ptr(x16), n, h, w, cin, _ptr(wp16), _ptr(bias), *_v(y), cout, ks, pad, _stream()), "conv2d_out_f16")
    return y


def conv1x1_pair_x_raw(xs, dims, wp1, b1, cout1, act1, wp2, b2, cout2, act2, gate_mask=None, gate_act="linear",
                       colsum=False, mask_out=True):
    """Two 1x1 layers in one launch (wcmc_conv1x1_pair_bf16x3): returns (split result of the first layer, its 1-bit
    mask or None, its column-sum partials or None, fp32 NHWC output of the second layer)."""
    n, cin, h, w = dims
    dev = xs.device
    ysp = _split_empty(n, cout1, h, w, dev)
    mask = torch.empty(n * h * w * ((cout1 + 7) // 8), device=dev, dtype=torch.uint8) if mask_out else None
    part = None
    if colsum:
        part = torch.empty(lib().wcmc_conv2d_igemm_colsum_elems(n, h, w, cout1), device=dev, dtype=torch.float32)
    y2 = nhwc_empty(n, cout2, h, w, dev)
    with _Timed("conv_pw", 4.0 * n * h * w * ((cin + 7) // 8 * 8 + cout1 + (cout2 + 3) // 4 * 4), "byte"):
        check(lib().wcmc_conv1x1_pair_bf16x3(_ptr(xs), n, h, w, cin, _ptr(wp1), _ptr(b1), cout1, ACT[act1], LEAKY_SLOPE,
                                             _ptr(ysp), _ptr(mask), _ptr(gate_mask), ACT[gate_act], LEAKY_SLOPE,
                                             _ptr(part), _ptr(wp2), _ptr(b2), cout2, ACT[act2], LEAKY_SLOPE,
                                             *_v(y2), _stream()), "conv1x1_pair_bf16x3")
    return ysp, mask, part, y2


def colsum_finish_raw(part, dims):
    n, c, h, w = dims
    db = torch.empty(c, device=part.device, dtype=torch.float32)
    check(lib().wcmc_colsum_finish(_ptr(part), n, h, w, c, _ptr(db), _stream()), "colsum_finish")
    return db


def conv2d_wgrad_x_raw(xs, xdims, dys, cout, ks, pad, weight_shape, want_bias=True, colsum_part=None, terms=None, sinks=(0, 0),
                       dw_flushed=False):
    """dw (and db) of one layer.  colsum_part: the per-tile column sums of dys that the launch producing dys left; the bias
    gradient is then finished by the slab-reduction launch itself (no column-sum pass, no finish launch).  sinks: data_ptr of the
    weight / bias PARAMETER (0: none) -- their gradients go straight into the optimiser's bucket where one is registered.
    dw_flushed: the weight is an output of ``_WeightNormMulti``, whose backward flushes this stream's deferred reductions before
    it reads dw (``_flushed_by_consumer``)."""
    n, cin, h, w = xdims
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    nbytes = lib().wcmc_conv2d_wgrad_bf16x3_workspace_bytes(n, ho, wo, cout, cin, ks)
    ws = torch.empty((nbytes + 3) // 4, device=xs.device, dtype=torch.float32)
    dw, dw_view = _sink_ex(sinks[0], weight_shape, xs.device)
    db, db_view = _sink_ex(sinks[1], (cout,), xs.device) if (want_bias or colsum_part is not None) else (None, True)
    args = (_ptr(xs), n, h, w, cin, _ptr(dys), cout, ks, pad, _ptr(dw), _ptr(db), _ptr(ws), ws.numel() * 4)
    cs = _ptr(colsum_part)
    terms = _sw.wgrad_terms() if terms is None else terms
    # A reduction may be deferred only where the memory it will write is certain to be the gradient's when it runs:
    # a bucket view (the optimiser's memory; AccumulateGrad adopts the tensor -- a parameter that already has a .grad, or needs
    # none, gets a fresh tensor from _sink_ex, which autograd adds into .grad or drops at once), or the weight gradient of an
    # effective weight of a weight-normalised layer (dw_flushed: consumed by the weight-norm node, which flushes first; the entry
    # then holds the tensor itself).  Any other weight -- a leaf that is no Parameter, a scaled, tied or otherwise computed
    # tensor -- is reduced inline: its consumer reads dw without flushing.  And never on a weight-gradient side
    # stream: the reader flushes ITS stream's entries.
    safe = (dw_view or dw_flushed) and db_view
    if (_sw._PROFILER is None and _sw._DEFERRED is not None and safe and nbytes <= _sw.DEFER_MAX_BYTES and (db is None or colsum_part is not None)
            and not _on_side_stream()):
        check(lib().wcmc_conv2d_wgrad_bf16x3(*args, 1, cs, terms, _stream()), "conv2d_wgrad_bf16x3")      # the GEMM now,
        st = torch.cuda.current_stream()                                                                 # the reduction later
        # (bucket views by ADDRESS: a reference held here would keep AccumulateGrad from adopting the tensor -- it would clone it, unreduced)
        _sw._DEFERRED.setdefault(st.cuda_stream, (st, []))[1].append((ws, dw.data_ptr() if dw_view else dw, db.data_ptr() if db is not None else 0,
                                                                  colsum_part, n, ho, wo, cout, cin, ks, terms))
    elif _sw._PROFILER is None:
        check(lib().wcmc_conv2d_wgrad_bf16x3(*args, 0, cs, terms, _stream()), "conv2d_wgrad_bf16x3")
    else:       # bracket the split-K GEMM launch alone; the slab reduce + bias gradient is its own class
        with _Timed(wgrad_launch_plan(n, h, w, cin, cout, ks, pad, terms)[0], 2.0 * n * ho * wo * cout * cin * ks * ks, "flop"):
            check(lib().wcmc_conv2d_wgrad_bf16x3(*args, 1, cs, terms, _stream()), "conv2d_wgrad_bf16x3")
        with _Timed("conv_wgrad_finish", 0.0, "flop"):
            check(lib().wcmc_conv2d_wgrad_bf16x3(*args, 2, cs, terms, _stream()), "conv2d_wgrad_bf16x3")
    return dw, db


# The data gradient's activation gate comes from the 1-bit mask the forward launch left (1/16 of the bytes of re-reading the
# activation's hi plane; the predicate is the same, so results are bit-identical to gating on the activation).
#
# The bias gradient of a layer is the column sum of its dy.  The data-gradient GEMM that produces dy leaves per-tile column
# sums; the slab-reduction launch of the layer's weight gradient finishes them (wcmc_conv2d_wgrad_bf16x3, dy_colsum_partial)
# instead of a wcmc_colsum_finish launch per layer: ~55 launches less per step.


def _chainx_forward(ctx, xs0, dims0, spec, params, extra_saved=None):
    """Shared forward of the split-bf16 chains: xs0 is the chain input as a split tensor of dims0.  extra_saved: a
    callable y -> tensors saved behind the chain's own (a fused consumer of the chain's output)."""
    ks, pad, acts = spec[:3]
    # spec[3] (optional): the input channels [c0, c1) whose gradient the producer of x will read (``pbuffer_cat``: only the
    # P-buffer's mean carries gradient, 3 of KPCN's 39 input channels) -- the first layer's data gradient is then formed for
    # the 8-aligned range round them only
    ctx.dx_channels = spec[3] if len(spec) > 3 else None
    spec = tuple(spec[:3])
    nl = len(acts)
    n = dims0[0]
    dims = [dims0]
    xs = [xs0]
    masks = []
    y = None
    # the last two layers of a 1x1 chain in one launch where the library has a fused instance (PathNet.final:
    # 128 -> 128 -> 3): the hidden activation is written once and not re-read
    pair = (ks == 1 and pad == 0 and nl >= 2 and
            lib().wcmc_conv1x1_pair_supported(params[2 * nl - 4].shape[1], params[2 * nl - 4].shape[0],
                                              params[2 * nl - 2].shape[0]))
    ctx.terms = _sw.chain_terms(ks, dims0[1])          # the backward multiplies as the mode of ITS forward says
    oterms = _chain_out_terms(ks, acts[-1], params[2 * nl - 2].shape[1], params[2 * nl - 2].shape[0], pair)     # ("h": one fp16 MFMA)
    # (packing every chain of a sub-network AHEAD in one launch -- five U-Net chains, a KPCN branch before its PathNet runs -- was
    # built and measured in round 6: 10.93 -> 10.96 ms per step, same box, three alternations: the 16 pack launches of a step cost nothing)
    packs = _pack_chain_x([params[2 * l] for l in range(nl)], ks, oterms) if 2 * nl <= PACK_MAX_ENTRIES else None
    ctx.wp1 = [pk[1] for pk in packs] if packs is not None else None      # the data-gradient orientation, for the backward
    pack0 = (lambda l: packs[l][0]) if packs is not None else (lambda l: _pack_x(params[2 * l], _fwd_pack_mode(oterms) if l == nl - 1 else 0))
    for l in range(nl):
        wt, b = params[2 * l], params[2 * l + 1]
        cout = wt.shape[0]
        if wt.shape[1] != dims[l][1]:
            raise RuntimeError("conv chain layer %d: weight expects %d input channels, got a tensor with %d"
                               % (l, wt.shape[1], dims[l][1]))
        wp = pack0(l)
        hidden = l < nl - 1
        if pair and l == nl - 2:
            xs1, mask1, _, y = conv1x1_pair_x_raw(xs[l], dims[l], wp, b.detach(), cout, acts[l], pack0(l + 1),
                                                  params[2 * l + 3].detach(), params[2 * l + 2].shape[0], acts[l + 1])
            hh, ww = dims[l][2], dims[l][3]
            dims.append((n, cout, hh, ww))
            dims.append((n, params[2 * l + 2].shape[0], hh, ww))
            xs.append(xs1)
            masks.append(mask1)
            break
        if not hidden and oterms == "h":
            out = conv2d_out_f16_raw(xs[l], dims[l], wp, b.detach(), cout, ks, pad)
        else:
            out = conv2d_x_raw(xs[l], dims[l], wp, b.detach(), cout, ks, pad, acts[l], out_split=hidden, mask_out=hidden,
                               terms=3 if hidden else oterms)
        hh, ww = dims[l][2] + 2 * pad - ks + 1, dims[l][3] + 2 * pad - ks + 1
        dims.append((n, cout, hh, ww))
        if hidden:
            xs.append(out[0] if _sw.EMULATE_HIDDEN is None else _sw.EMULATE_HIDDEN(out[0], dims[-1], ks))
            masks.append(out[1])       # (hi > 0) bits of the hidden activation: the data gradient's ReLU gate
        else:
            y = out
    ctx.spec, ctx.dims = spec, dims
    ctx.bias_ptrs = [params[2 * l + 1].data_ptr() if isinstance(params[2 * l + 1], torch.nn.Parameter) else 0 for l in range(nl)]
    keep_y = [y] if acts[-1] != "linear" else []
    extra = tuple(extra_saved(y)) if extra_saved is not None else ()
    ctx.n_extra = len(extra)
    ctx.save_for_backward(*xs, *masks, *keep_y, *[params[2 * l] for l in range(nl)], *extra)
    if _sw.DEBUG_ACTS is not None:
        _sw.DEBUG_ACTS.extend(unsplit_debug(xs[l + 1], *dims[l + 1]) for l in range(nl - 1))
        if acts[-1] != "linear":
            _sw.DEBUG_ACTS.append(y)
    return y


def _chainx_backward(ctx, dy, need_dx, dys=None, part=None):
    """Shared backward: returns (dx as an fp32 NHWC view or None, [dw0, db0, dw1, db1, ...]).
    dys: the output gradient already as a split tensor (linear output layers only); part: its column-sum partials."""
    ks, pad, acts = ctx.spec
    dims = ctx.dims
    nl = len(acts)
    saved = ctx.saved_tensors
    xs = saved[:nl]
    masks = saved[nl:2 * nl - 1]
    off = 2 * nl - 1
    if dys is None:
        dy = _as_nhwc_nograd(dy)
        gated = acts[-1] != "linear"
        # split (output-activation backward folded in) + the last layer's bias-gradient partials in one pass over dy
        dys, part = split_dy_colsum_raw(dims[nl], dy=dy, post=saved[off] if gated else None, act=acts[-1])
        off += 1 if gated else 0
    else:
        assert acts[-1] == "linear"
    ws = saved[off:len(saved) - getattr(ctx, "n_extra", 0)]
    # part: per-tile column sums of dys when the launch that produced dys left them
    grads = [None] * (2 * nl)
    dx = None
    main = torch.cuda.current_stream()
    side = _side_stream(dys.device)
    keep = []
    wp1 = getattr(ctx, "wp1", None)
    wterms, dterms = ctx.terms
    bptrs = getattr(ctx, "bias_ptrs", None) or [0] * nl
    sink_of = lambda l: (ws[l].data_ptr() if isinstance(ws[l], torch.nn.Parameter) else 0, bptrs[l])
    flushed = [_flushed_by_consumer(w) for w in ws]
    pack1 = (lambda l: wp1[l]) if wp1 is not None else (lambda l: _pack_x(ws[l], _dgrad_mode(dterms)))
    for l in range(nl - 1, -1, -1):
        wt = ws[l]
        cout = wt.shape[0]
        if side is not None:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                dw, db = conv2d_wgrad_x_raw(xs[l], dims[l], dys, cout, ks, pad, wt.shape, want_bias=part is None,
                                            colsum_part=part, terms=wterms, sinks=sink_of(l), dw_flushed=flushed[l])
            dw.record_stream(main)
            db.record_stream(main)
            keep.append(dys)
            keep.append(part)
        else:
            dw, db = conv2d_wgrad_x_raw(xs[l], dims[l], dys, cout, ks, pad, wt.shape, want_bias=part is None,
                                        colsum_part=part, terms=wterms, sinks=sink_of(l), dw_flushed=flushed[l])
        grads[2 * l], grads[2 * l + 1] = dw, db
        if (l == 1 and need_dx and ks == 1 and pad == 0 and
                lib().wcmc_conv1x1_pair_supported(cout, wt.shape[1], ws[0].shape[1])):
            # the data gradients of layers 1 and 0 in one launch (PathNet.final: 3 -> 128 -> 128): the 128-channel
            # gradient of the hidden activation is written once (the weight gradient of layer 0 reads it) and feeds
            # the second GEMM from LDS
            dys, _, part, dx = conv1x1_pair_x_raw(dys, dims[2], pack1(1), None, wt.shape[1], "linear",
                                                  pack1(0), None, ws[0].shape[1], "linear",
                                                  gate_mask=masks[0], gate_act=acts[0], colsum=True, mask_out=False)
        elif l > 0:
            wpt = pack1(l)
            dys, part = conv2d_x_raw(dys, dims[l + 1], wpt, None, wt.shape[1], ks, ks - 1 - pad, "linear",
                                     out_split=True, gate_act=acts[l - 1], colsum=True, terms=dterms, gate_mask=masks[l - 1])
        elif need_dx and dx is None:
            sub = getattr(ctx, "dx_channels", None)
            if sub is not None and (sub[1] + 7) // 8 * 8 - sub[0] // 8 * 8 <= wt.shape[1] // 2:
                # the consumer reads channels [c0, c1) only: a GEMM over the 8-aligned rows round them (KPCN's first layer: 16 of
                # 48 padded rows, one cout tile instead of four); the rest of dx is zero, never read
                a0, a1 = sub[0] // 8 * 8, min((sub[1] + 7) // 8 * 8, wt.shape[1])
                nn_, _, hh_, ww_ = dims[0]
                dx = nhwc_empty(nn_, wt.shape[1], hh_, ww_, dys.device, zero=True)
                wsub = _pack_x(wt.detach()[:, a0:a1].contiguous(), _dgrad_mode(dterms))
                conv2d_x_raw(dys, dims[l + 1], wsub, None, a1 - a0, ks, ks - 1 - pad, "linear", out_split=False, terms=dterms,
                             out=dx[:, a0:a1])
            else:
                wpt = pack1(l)
                dx = conv2d_x_raw(dys, dims[l + 1], wpt, None, wt.shape[1], ks, ks - 1 - pad, "linear",
                                  out_split=False, terms=dterms)
    if side is not None:
        main.wait_stream(side)
    del keep
    return dx, grads


class _ConvChainX(torch.autograd.Function):
    """``_ConvChain`` on the split-bf16 GEMMs: intermediates live as split tensors (same bytes as
    fp32), only the chain's input and output are fp32 NHWC views."""

    @staticmethod
    def forward(ctx, x, spec, *params):
        _need_cuda(x, *params)
        return _chainx_forward(ctx, split_raw(x), tuple(x.shape), spec, params)

    @staticmethod
    def backward(ctx, dy):
        dx, grads = _chainx_backward(ctx, dy, ctx.needs_input_grad[0])
        return (dx, None, *grads)


def _split_shared(x):
    """split_raw, remembered ON the tensor object: the two PathNets embed the SAME converted ``paths`` tensor
    (interfaces.py:195-196; PathNet._paths_nhwc keeps that object in the batch dictionary for one step), so its
    168 MB split is made once per step.  Valid for the version and stream it was made on."""
    tag = (x._version, torch.cuda.current_stream().cuda_stream)
    cached = getattr(x, "_wcmc_split", None)
    if cached is not None and cached[0] == tag:
        return cached[1]
    if cached is not None and cached[0] == (x._version, None):      # presplit_shared: made before the streams forked
        cached[1].record_stream(torch.cuda.current_stream())
        return cached[1]
    xs = split_raw(x)
    if not x.requires_grad:
        x._wcmc_split = (tag, xs)
    return xs


class _ChainSppMeanX(torch.autograd.Function):
    """``y = chain(x); m = y.view(B,S,...).mean(1)`` (networks.py:33-36) as one node.  y feeds the concatenation
    and m the U-Net, so y's gradient is ``g_y + repeat_S(g_m) / S``: formed once, directly as the split dy of
    the chain's backward (``wcmc_add_broadcast_split``) instead of broadcast + add + split."""

    @staticmethod
    def forward(ctx, x, s, spec, *params):
        _need_cuda(x, *params)
        assert spec[2][-1] == "linear"
        y = _chainx_forward(ctx, _split_shared(x), tuple(x.shape), spec, params)
        bs, c, h, w = y.shape
        m = nhwc_empty(bs // s, c, h, w, y.device)
        check(lib().wcmc_spp_reduce(*_v(y), *_v(m), bs // s, s, h, w, c, 1.0 / s, _stream()), "spp_reduce")
        ctx.s = s
        return y, m

    @staticmethod
    def backward(ctx, gy, gm):
        s = ctx.s
        bs, c, h, w = ctx.dims[-1]
        gy = _as_nhwc_nograd(gy) if gy is not None else None
        gm = _as_nhwc_nograd(gm) if gm is not None else None
        dys, part = split_dy_colsum_raw((bs, c, h, w), dy=gy, gm=gm, s=s, scale=1.0 / s)
        dx, grads = _chainx_backward(ctx, None, ctx.needs_input_grad[0], dys=dys, part=part)
        return (dx, None, None, *grads)


class _CatBroadcastChainX(torch.autograd.Function):
    """``chain(cat([flat, repeat_S(prop)], 1))`` (networks.py:39-42) with the concatenation written once,
    directly as the chain's split input (``wcmc_cat_broadcast_split``); the backward splits the chain's
    input gradient into the per-sample half (a view) and the spp-summed half."""

    @staticmethod
    def forward(ctx, flat, prop, s, spec, *params):
        _need_cuda(flat, prop, *params)
        bs, c1, h, w = flat.shape
        b, c2 = prop.shape[0], prop.shape[1]
        assert bs == b * s and c1 % 8 == 0 and prop.shape[2:] == flat.shape[2:]
        xs0 = _split_empty(bs, c1 + c2, h, w, flat.device)
        check(lib().wcmc_cat_broadcast_split(*_v(flat), *_v(prop), _ptr(xs0), b, s, h, w, c1, c2, _stream()),
              "cat_broadcast_split")
        ctx.cat = (b, s, c1, c2)
        return _chainx_forward(ctx, xs0, (bs, c1 + c2, h, w), spec, params)

    @staticmethod
    def backward(ctx, dy):
        b, s, c1, c2 = ctx.cat
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dx, grads = _chainx_backward(ctx, dy, need)
        dflat = dprop = None
        if need:
            _, _, h, w = dx.shape
            dflat = dx[:, :c1]
            if s == 1:                               # plain concatenation: both halves are views
                dprop = dx[:, c1:]
            else:
                dprop = nhwc_empty(b, c2, h, w, dx.device)
                check(lib().wcmc_spp_reduce(*_v(dx[:, c1:]), *_v(dprop), b, s, h, w, c2, 1.0, _stream()), "spp_reduce")
        return (dflat, dprop, None, None, *grads)


class _CatUpsampleChainX(torch.autograd.Function):
    """``chain(cat([upsample2(deep), skip], 1))`` (a U-Net level's right chain) with the bilinear upsampling evaluated
    inside the concatenation kernel (``wcmc_cat_upsample_split``): the upsampled tensor is never written; the
    backward is the chain's, then ``upsample2``'s on the first channels of its input gradient."""

    @staticmethod
    def forward(ctx, deep, skip, spec, *params):
        _need_cuda(deep, skip, *params)
        n, c1, hd, wd = deep.shape
        c2, h, w = skip.shape[1:]
        assert skip.shape[0] == n and h == 2 * hd and w == 2 * wd and c1 % 8 == 0
        xs0 = _split_empty(n, c1 + c2, h, w, deep.device)
        check(lib().wcmc_cat_upsample_split(*_v(deep), *_v(skip), _ptr(xs0), n, h, w, c1, c2, _stream()), "cat_upsample_split")
        ctx.cat = (n, c1, c2, h, w)
        return _chainx_forward(ctx, xs0, (n, c1 + c2, h, w), spec, params)

    @staticmethod
    def backward(ctx, dy):
        n, c1, c2, h, w = ctx.cat
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dx, grads = _chainx_backward(ctx, dy, need)
        ddeep = dskip = None
        if need:
            g = dx[:, :c1]
            ddeep = nhwc_empty(n, c1, h // 2, w // 2, dx.device)
            check(lib().wcmc_upsample2_bwd(*_v(g), *_v(ddeep), n, h // 2, w // 2, c1, _stream()), "upsample2_bwd")
            dskip = dx[:, c1:]
        return (ddeep, dskip, None, *grads)


def conv_chain(x, ksize, pad, acts, params):
    if not _sw.split_path():
        return _ConvChain.apply(as_nhwc(x), (ksize, pad, tuple(acts)), *params)
    hint = getattr(x, "_wcmc_grad_channels", None)          # left by pbuffer_cat on its output
    spec = (ksize, pad, tuple(acts)) + ((tuple(hint),) if hint is not None else ())
    return _ConvChainX.apply(as_nhwc(x), spec, *params)
