"""The glue kernels of csrc/elementwise.hip against tests/glue_ref.py, element by element: bit for bit where the operation is
exact, inside a derived per-element bound where it rounds (the derivations: glue_ref.py and DESIGN.md, "Glue and optimiser-tail
contracts").  Every case runs on a dense NHWC buffer and on the channel slice [4 : 4 + C] of a wider one, with the pad lanes and
the neighbouring channels of the inputs holding NaN in one run and 0 in the other: no valid lane may notice."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import glue_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -777.0
LAYOUTS = ("dense", "slice")


def ops():
    from wcmc_amd import ops as _ops
    return _ops


def L():
    from wcmc_amd._lib import lib
    return lib()


def wide_of(c, layout):
    return None if layout == "dense" else (4, 4 + (c + 3) // 4 * 4 + 4)


def dview(valid, layout, fill):
    """NHWC device view of the CPU tensor ``valid`` (dense, or a slice of a wider buffer), pad lanes and neighbours = fill."""
    n, c, h, w = valid.shape
    return R.nhwc_buffer(n, c, h, w, fill, wide=wide_of(c, layout), device=DEV, valid=valid)[0]


def dout(n, c, h, w, layout):
    """(view, whole buffer) of an output pre-filled with the sentinel."""
    return R.nhwc_buffer(n, c, h, w, SENTINEL, wide=wide_of(c, layout), device=DEV)


def V(t):
    return ctypes.c_void_p(t.data_ptr()), t.stride(0), t.stride(2), t.stride(3)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check_extent(buf, c, layout, masked, what):
    """Pad lanes of a written output are 0 where the kernel masks; nothing outside [c0, c0 + round_up(C,4)) changed."""
    pad, out = R.outside(buf, c, wide_of(c, layout))
    if masked and pad.numel():
        assert float(pad.abs().max()) == 0.0, what + ": pad lanes are not zero"
    assert bool((out == SENTINEL).all()), what + ": wrote outside its channel slice"


def both_fills(fn):
    """fn(fill) -> tuple of device tensors; runs it with NaN and with 0 in the pad lanes, asserts the runs are bit-equal and returns one."""
    a, b = fn(R.NAN), fn(0.0)
    for i, (u, v) in enumerate(zip(a, b)):
        R.assert_bit_equal(u, v, "NaN pad lanes against zero pad lanes, output %d" % i)
    return a


# ---------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", R.POOL_KINDS)
@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_maxpool2_is_bit_equal_to_max_pool2d_and_its_autograd(shape, kind, layout):
    """Exact operation: outputs and input gradients -- bwd_add's one fp32 add included -- equal CPU fp32 F.max_pool2d + autograd bit
    for bit; NaN positions match.  Ties: first maximum in window order; NaN: reaches the output, the last NaN of the window takes
    the gradient (what ATen does; the reference decides, not this sentence)."""
    o = ops()
    n, c, h, w = shape
    xc = R.pool_data(shape, kind, seed=3)
    dyc, addc = R.rnd(n, c, h // 2, w // 2, seed=4), R.rnd(*shape, seed=5)
    xr = xc.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    (dxr,) = torch.autograd.grad(yr, xr, dyc)
    dxr_add = dxr + addc

    def run(fill):
        x = dview(xc, layout, fill).detach().requires_grad_(True)
        y = o.maxpool2(x)
        (dx,) = torch.autograd.grad(y, x, dview(dyc, layout, fill))
        x2 = dview(xc, layout, fill).detach().requires_grad_(True)
        skip, y2 = o.maxpool2_skip(x2)
        (dx2,) = torch.autograd.grad([skip, y2], x2, [dview(addc, layout, fill), dview(dyc, layout, fill)])
        return y, dx, y2, dx2
    y, dx, y2, dx2 = both_fills(run)
    R.assert_bit_equal(y, yr.detach(), "maxpool2 fwd")
    R.assert_bit_equal(dx, dxr, "maxpool2 bwd")
    R.assert_bit_equal(y2, yr.detach(), "maxpool2_skip fwd")
    R.assert_bit_equal(dx2, dxr_add, "maxpool2_skip bwd_add")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [s for s in R.POOL_SHAPES if s[1] % 4])
def test_maxpool2_writes_zero_pad_lanes_and_stays_inside_its_slice(shape, layout):
    n, c, h, w = shape
    xc = R.pool_data(shape, "ties", seed=3)
    dyc, addc = R.rnd(n, c, h // 2, w // 2, seed=4), R.rnd(*shape, seed=5)
    x, dy, add = dview(xc, layout, R.NAN), dview(dyc, layout, R.NAN), dview(addc, layout, R.NAN)
    y, ybuf = dout(n, c, h // 2, w // 2, layout)
    assert L().wcmc_maxpool2_fwd(*V(x), *V(y), n, h, w, c, stream()) == 0
    check_extent(ybuf, c, layout, True, "maxpool2_fwd")
    R.assert_bit_equal(y, F.max_pool2d(xc, 2), "maxpool2_fwd into a sentinel buffer")
    for use_add in (False, True):
        dx, dxbuf = dout(n, c, h, w, layout)
        if use_add:
            assert L().wcmc_maxpool2_bwd_add(*V(x), *V(dy), *V(add), *V(dx), n, h, w, c, stream()) == 0
        else:
            assert L().wcmc_maxpool2_bwd(*V(x), *V(dy), *V(dx), n, h, w, c, stream()) == 0
        check_extent(dxbuf, c, layout, True, "maxpool2_bwd")
        R.assert_bit_equal(dx, R.maxpool2_bwd(xc, dyc, addc if use_add else None), "maxpool2_bwd into a sentinel buffer")


@pytest.mark.parametrize("shape", [(1, 4, 3, 4), (1, 4, 4, 3), (2, 5, 1, 2)])
def test_maxpool2_refuses_odd_extents_and_writes_nothing(shape):
    o = ops()
    n, c, h, w = shape
    x = dview(R.rnd(*shape, seed=1), "dense", 0.0)
    with pytest.raises(RuntimeError, match="even"):
        o.maxpool2(x)
    with pytest.raises(RuntimeError, match="even"):
        o.maxpool2_skip(x)
    y, ybuf = dout(n, c, max(h // 2, 1), max(w // 2, 1), "dense")
    dx, dxbuf = dout(n, c, h, w, "dense")
    assert L().wcmc_maxpool2_fwd(*V(x), *V(y), n, h, w, c, stream()) != 0
    assert L().wcmc_maxpool2_bwd(*V(x), *V(y), *V(dx), n, h, w, c, stream()) != 0
    assert L().wcmc_maxpool2_bwd_add(*V(x), *V(y), *V(x), *V(dx), n, h, w, c, stream()) != 0
    torch.cuda.synchronize()
    assert bool((ybuf == SENTINEL).all()) and bool((dxbuf == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- bilinear x2
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", R.UP_SHAPES)
def test_upsample2_per_element_against_fp64_interpolate(shape, layout):
    """|got - want| <= 2 * k * 2^-24 * A(|x|) per element against fp64 F.interpolate(bilinear, align_corners=False) and its autograd
    (glue_ref.upsample2_fwd / _bwd hold the restatement to it on the CPU).  Forward k = 4: fl(.5625 v00) and three fused
    multiply-adds, dyadic weights.  Backward k = 16: at most 4 x 4 taps, one fused multiply-add each from 0.  The factor 2 is the
    safety factor against a second rounding per multiply-add.  H == 1, W == 1 and 1 x 1: both clamp branches hit the same pixel."""
    o = ops()
    n, c, h, w = shape
    xc, dyc = R.rnd(*shape, seed=7), R.rnd(n, c, 2 * h, 2 * w, seed=8)
    want, bound = R.upsample2_fwd(xc)
    wantb, boundb = R.upsample2_bwd(dyc)

    def run(fill):
        x = dview(xc, layout, fill).detach().requires_grad_(True)
        y = o.upsample2(x)
        (dx,) = torch.autograd.grad(y, x, dview(dyc, layout, fill))
        return y, dx
    y, dx = both_fills(run)
    R.assert_within(y, want, bound, "upsample2_fwd %s %s" % (shape, layout))
    R.assert_within(dx, wantb, boundb, "upsample2_bwd %s %s" % (shape, layout))
    if c % 4:
        x, dy = dview(xc, layout, R.NAN), dview(dyc, layout, R.NAN)
        y2, ybuf = dout(n, c, 2 * h, 2 * w, layout)
        dx2, dxbuf = dout(n, c, h, w, layout)
        assert L().wcmc_upsample2_fwd(*V(x), *V(y2), n, h, w, c, stream()) == 0
        assert L().wcmc_upsample2_bwd(*V(dy), *V(dx2), n, h, w, c, stream()) == 0
        check_extent(ybuf, c, layout, True, "upsample2_fwd")
        check_extent(dxbuf, c, layout, True, "upsample2_bwd")
        R.assert_bit_equal(y2, y, "upsample2_fwd into a sentinel buffer")
        R.assert_bit_equal(dx2, dx, "upsample2_bwd into a sentinel buffer")


# ---------------------------------------------------------------------------------------------------- spp mean, broadcast, cat
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", R.SPP_SHAPES)
def test_spp_mean_reduce_within_bound_broadcast_bit_equal(shape, layout):
    """Reduction: per element <= 2 * (S + 1) * 2^-24 * sum|v| * scale (S - 1 rounded adds and the multiply; the bar the issue sets is
    S + 1).  Its backward and accumulate = 1 are ONE fp32 multiply (by fl(1/S)) and one fp32 add: bit-equal to CPU fp32."""
    o = ops()
    b, s, c, h, w = shape
    xc, gc = R.rnd(b * s, c, h, w, seed=9), R.rnd(b, c, h, w, seed=10)
    want, bound = R.spp_reduce(xc, s, 1.0 / s)

    def run(fill):
        x = dview(xc, layout, fill).detach().requires_grad_(True)
        y = o.spp_mean(x, s)
        (dx,) = torch.autograd.grad(y, x, dview(gc, layout, fill))
        return y, dx
    y, dx = both_fills(run)
    R.assert_within(y, want, bound, "spp_reduce %s %s" % (shape, layout))
    R.assert_bit_equal(dx, R.spp_broadcast(gc, s, 1.0 / s), "spp_mean backward")
    # through the C ABI into sentinel buffers: extent, zero pad lanes, and spp_broadcast with accumulate = 1 (no wrapper exposes it)
    x, g = dview(xc, layout, R.NAN), dview(gc, layout, R.NAN)
    y2, ybuf = dout(b, c, h, w, layout)
    assert L().wcmc_spp_reduce(*V(x), *V(y2), b, s, h, w, c, 1.0 / s, stream()) == 0
    check_extent(ybuf, c, layout, True, "spp_reduce")
    R.assert_bit_equal(y2, y, "spp_reduce into a sentinel buffer")
    d2, dbuf = dout(b * s, c, h, w, layout)
    assert L().wcmc_spp_broadcast(*V(g), *V(d2), b, s, h, w, c, 1.0 / s, 0, stream()) == 0
    check_extent(dbuf, c, layout, True, "spp_broadcast")
    R.assert_bit_equal(d2, dx, "spp_broadcast into a sentinel buffer")
    acc = dview(xc, layout, R.NAN)
    assert L().wcmc_spp_broadcast(*V(g), *V(acc), b, s, h, w, c, 1.0 / s, 1, stream()) == 0
    R.assert_bit_equal(acc, R.spp_broadcast(gc, s, 1.0 / s, into=xc), "spp_broadcast accumulate=1")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", R.CATB_SHAPES)
def test_cat_broadcast_and_cat_channels_forward_bit_equal_backward_within_bound(shape, layout):
    """Copies are exact.  The gradient into the broadcast operand is the sum over the S samples (scale 1, exact multiply):
    per element <= 2 * (S + 1) * 2^-24 * sum|g|."""
    o = ops()
    b, s, c1, c2, h, w = shape
    flatc, propc = R.rnd(b * s, c1, h, w, seed=11), R.rnd(b, c2, h, w, seed=12)
    gc = R.rnd(b * s, c1 + c2, h, w, seed=13)
    wantr, bound = R.spp_reduce(gc[:, c1:].contiguous(), s, 1.0)

    def run(fill):
        flat = dview(flatc, layout, fill).detach().requires_grad_(True)
        prop = dview(propc, layout, fill).detach().requires_grad_(True)
        out = o.cat_broadcast(flat, prop, s)
        df, dp = torch.autograd.grad(out, [flat, prop], dview(gc, layout, fill))
        a = dview(flatc, layout, fill).detach().requires_grad_(True)
        bb = dview(propc.repeat_interleave(s, 0), layout, fill).detach().requires_grad_(True)
        out2 = o.cat_channels(a, bb)
        da, db = torch.autograd.grad(out2, [a, bb], dview(gc, layout, fill))
        return out, df, dp, out2, da, db
    out, df, dp, out2, da, db = both_fills(run)
    R.assert_bit_equal(out, R.cat_broadcast(flatc, propc, s), "cat_broadcast fwd")
    R.assert_bit_equal(df, gc[:, :c1], "cat_broadcast d flat")
    R.assert_within(dp, wantr, bound, "cat_broadcast_bwd %s %s" % (shape, layout))
    R.assert_bit_equal(out2, R.cat_channels(flatc, propc.repeat_interleave(s, 0)), "cat_channels fwd")
    R.assert_bit_equal(da, gc[:, :c1], "cat_channels d a")
    R.assert_bit_equal(db, gc[:, c1:], "cat_channels d b")


# ---------------------------------------------------------------------------------------------------- P-buffer cat, sample cat
def _strided_base(basec):
    """base with non-contiguous NCHW strides: a crop of a larger channel-first tensor."""
    b, cb, h, w = basec.shape
    big = torch.full((b, cb + 2, h + 1, w + 3), R.NAN)
    big[:, 1:1 + cb, 1:, 2:2 + w] = basec
    return big.to(DEV)[:, 1:1 + cb, 1:, 2:2 + w]


def _sliced_p(pc):
    """p as a channel slice of 2 * cp channels (B,S,2cp,H,W)."""
    b, s, cp, h, w = pc.shape
    big = torch.full((b, s, 2 * cp, h, w), R.NAN)
    big[:, :, cp // 2:cp // 2 + cp] = pc
    return big.to(DEV)[:, :, cp // 2:cp // 2 + cp]


@pytest.mark.parametrize("w", R.PB_W)
def test_pbuffer_cat_and_sample_features_cat(w):
    """Copied channels and both backwards bit-equal; mean channels <= 2 * (S + 1) * 2^-24 * sum|v| / S; the variance channel inside
    the two-pass bound of glue_ref.pvar_and_bound:  2 * [(S + Cp + 5) * 2^-24 * (var + shift) + shift],  shift = sum_c S em_c^2 /
    (S - 1) / (Cp S),  em_c = 2^-24 * sum|x_s|  -- the error of the mean enters squared, (S 2^-24 |mean| / sigma)^2 relative, so the
    |mean| = 100 sigma pixel of the data is held as tightly as the others; the constant-over-samples pixel gives exactly 0."""
    o = ops()
    for s, h, cb, cp in R.PB_REST:
        b = 2 if w < 100 else 1
        basec, pc = R.rnd(b, cb, h, w, seed=14), R.pdata(b, s, cp, h, w, seed=15)
        gc = R.rnd(b, cb + cp + 1, h, w, seed=17)
        want, bound = R.pbuffer_cat(basec, pc)
        what = "(w=%d s=%d h=%d cb=%d cp=%d)" % (w, s, h, cb, cp)
        for layout in LAYOUTS:
            p = _sliced_p(pc).detach().requires_grad_(True)
            out = o.pbuffer_cat(_strided_base(basec), p)
            (dp,) = torch.autograd.grad(out, p, dview(gc, layout, R.NAN))
            R.assert_bit_equal(out[:, :cb], basec, "pbuffer_cat base " + what)
            R.assert_within(out[:, cb:cb + cp], want[:, cb:cb + cp], bound[:, cb:cb + cp], "pbuffer_cat_mean " + what)
            R.assert_within(out[:, cb + cp:], want[:, cb + cp:], bound[:, cb + cp:], "pbuffer_cat_var " + what)
            if w > 1:
                assert float(out.detach()[:, cb + cp, :, w - 1].abs().max()) == 0.0, "constant samples: variance not exactly 0 " + what
            R.assert_bit_equal(dp, R.pbuffer_cat_bwd(gc, s, cb, cp), "pbuffer_cat backward " + what)
        # the forward through the C ABI into a sentinel slice: pad lanes zero, nothing outside the slice
        ct = cb + cp + 1
        for layout in LAYOUTS:
            o2, obuf = dout(b, ct, h, w, layout)
            base, p = _strided_base(basec), _sliced_p(pc)
            assert L().wcmc_pbuffer_cat_fwd(ctypes.c_void_p(base.data_ptr()), *base.stride(), ctypes.c_void_p(p.data_ptr()), *p.stride(),
                                            *V(o2), b, s, cb, cp, h, w, stream()) == 0
            check_extent(obuf, ct, layout, True, "pbuffer_cat_fwd " + what)
            R.assert_bit_equal(o2, out, "pbuffer_cat_fwd into a sentinel buffer " + what)
        # the per-sample form
        featc = R.rnd(b, s, cb, h, w, seed=16)
        want2, bound2 = R.sample_cat(featc, pc)
        big = torch.full((b, s, cb + 1, h + 2, w), R.NAN)
        big[:, :, :cb, 1:h + 1] = featc
        feat = big.to(DEV)[:, :, :cb, 1:h + 1].detach().requires_grad_(True)
        p = _sliced_p(pc).detach().requires_grad_(True)
        out3 = o.sample_features_cat(feat, p)
        g3 = R.rnd(*out3.shape, seed=18)
        df, dp3 = torch.autograd.grad(out3, [feat, p], g3.to(DEV))
        R.assert_bit_equal(out3[:, :, :cb + cp], torch.cat([featc, pc], 2), "sample_cat copies " + what)
        R.assert_within(out3[:, :, cb + cp:], want2[:, :, cb + cp:], bound2[:, :, cb + cp:], "sample_cat_var " + what)
        R.assert_bit_equal(df, g3[:, :, :cb], "sample_cat d features")
        R.assert_bit_equal(dp3, g3[:, :, cb:cb + cp], "sample_cat d p")


def test_one_sample_is_refused_without_a_launch():
    o = ops()
    base, p = torch.zeros(1, 3, 4, 5, device=DEV), torch.zeros(1, 1, 2, 4, 5, device=DEV)
    with pytest.raises(RuntimeError, match="S must be >= 2"):
        o.pbuffer_cat(base, p)
    with pytest.raises(RuntimeError, match="S must be >= 2"):
        o.sample_features_cat(torch.zeros(1, 1, 3, 4, 5, device=DEV), p)
    out, obuf = dout(1, 6, 4, 5, "dense")
    rc = L().wcmc_pbuffer_cat_fwd(ctypes.c_void_p(base.data_ptr()), *base.stride(), ctypes.c_void_p(p.data_ptr()), *p.stride(), *V(out),
                                  1, 1, 3, 2, 4, 5, stream())
    flat = torch.full((1, 1, 6, 4, 5), SENTINEL, device=DEV)
    f = torch.zeros(1, 1, 3, 4, 5, device=DEV)
    rc2 = L().wcmc_sample_cat_fwd(ctypes.c_void_p(f.data_ptr()), *f.stride(), ctypes.c_void_p(p.data_ptr()), *p.stride(),
                                  ctypes.c_void_p(flat.data_ptr()), 1, 1, 3, 2, 4, 5, stream())
    torch.cuda.synchronize()
    assert rc != 0 and rc2 != 0
    assert bool((obuf == SENTINEL).all()) and bool((flat == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- layout converters
@pytest.mark.parametrize("shape", [(2, 1, 3, 1), (1, 31, 2, 63), (2, 33, 3, 65), (1, 129, 2, 65), (1, 129, 1, 1), (3, 5, 2, 130)])
def test_layout_round_trip_is_bit_equal_at_tile_edges(shape):
    """W in {1, 63, 65, 130} against the 64-pixel tile, C in {1, 31, 33, 129} against the 32-channel tile (the z-grid is capped at 4
    blocks, so C > 128 loops), strided channel-first sources; to_nhwc writes its pad lanes as zeros and nothing outside its slice."""
    o = ops()
    n, c, h, w = shape
    xc = R.rnd(*shape, seed=21)
    big = torch.full((n, c + 2, h + 1, w + 3), R.NAN)
    big[:, 1:1 + c, 1:, 2:2 + w] = xc
    for src in (xc.to(DEV), big.to(DEV)[:, 1:1 + c, 1:, 2:2 + w], xc.to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)):
        y = o.to_nhwc_raw(src)
        assert o.is_nhwc_view(y)
        R.assert_bit_equal(y, xc, "to_nhwc")
        back = o.from_nhwc_raw(y)
        assert back.is_contiguous()
        R.assert_bit_equal(back, xc, "from_nhwc")
        for layout in LAYOUTS:
            y2, ybuf = dout(n, c, h, w, layout)
            assert L().wcmc_to_nhwc(ctypes.c_void_p(src.data_ptr()), *src.stride(), *V(y2), n, c, h, w, stream()) == 0
            check_extent(ybuf, c, layout, True, "to_nhwc")
            R.assert_bit_equal(y2, xc, "to_nhwc into a sentinel slice")
            # from a NaN-padded slice into a strided channel-first destination: only the crop is written
            dst = torch.full((n, c + 1, h + 2, w + 1), SENTINEL, device=DEV)
            crop = dst[:, 1:, 1:h + 1, :w]
            assert L().wcmc_from_nhwc(*V(dview(xc, layout, R.NAN)), ctypes.c_void_p(crop.data_ptr()), *crop.stride(), n, c, h, w, stream()) == 0
            R.assert_bit_equal(crop, xc, "from_nhwc into a crop")
            dst[:, 1:, 1:h + 1, :w] = SENTINEL
            assert bool((dst == SENTINEL).all()), "from_nhwc wrote outside its destination"


def test_layout_refuses_65536_rows():
    x = torch.zeros(1, 4, 65536, 1, device=DEV)
    y, ybuf = dout(1, 4, 65536, 1, "dense")
    assert L().wcmc_to_nhwc(ctypes.c_void_p(x.data_ptr()), *x.stride(), *V(y), 1, 4, 65536, 1, stream()) != 0
    back = torch.full((1, 4, 65536, 1), SENTINEL, device=DEV)
    assert L().wcmc_from_nhwc(*V(y), ctypes.c_void_p(back.data_ptr()), *back.stride(), 1, 4, 65536, 1, stream()) != 0
    torch.cuda.synchronize()
    assert bool((ybuf == SENTINEL).all()) and bool((back == SENTINEL).all())
    ok = dout(1, 4, 65535, 1, "dense")[0]
    assert L().wcmc_to_nhwc(ctypes.c_void_p(x.data_ptr()), *x.stride(), *V(ok), 1, 4, 65535, 1, stream()) == 0
    assert float(ok.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- consumers of unwritten pad lanes
# pbuffer_cat_bwd and the copy_ concatenations leave the pad lanes of their outputs unwritten (whatever the caching allocator
# hands back): what consumes those outputs in the step must not let a pad lane reach a valid one.
@pytest.mark.parametrize("mode", ["default", "fp32"])
@pytest.mark.parametrize("case", [(2, 7, 6, 5, 5, 3, 1, "relu"), (1, 34, 9, 9, 6, 5, 0, "linear"), (2, 13, 4, 6, 3, 1, 0, "relu")])
def test_conv_chain_ignores_nan_pad_lanes_of_its_input_and_of_its_gradient(case, mode):
    o = ops()
    n, cin, h, w, cout, ks, pad, act = case
    xc = R.rnd(n, cin, h, w, seed=2)
    wt = R.rnd(cout, cin, ks, ks, seed=3, scale=0.3).to(DEV)
    bs = R.rnd(cout, seed=4, scale=0.2).to(DEV)
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    gyc = R.rnd(n, cout, ho, wo, seed=5)
    old = o.PRECISION
    o.set_precision(o.MODES[0] if mode == "default" else mode)
    try:
        def run(fill):
            x = dview(xc, "slice", fill).detach().requires_grad_(True)
            wd, bd = wt.clone().requires_grad_(True), bs.clone().requires_grad_(True)
            y = o.conv_chain(x, ks, pad, [act], [wd, bd])
            dx, dw, db = torch.autograd.grad(y, [x, wd, bd], dview(gyc, "slice", fill))
            return y, dx, dw, db
        y, dx, dw, db = both_fills(run)
    finally:
        o.set_precision(old)
    for t in (y, dx, dw, db):
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("shape", [(2, 7, 3, 5), (1, 34, 2, 9)])
def test_split_bf16_ignores_nan_pad_lanes(shape):
    o = ops()
    xc = R.rnd(*shape, seed=6)
    (s,) = both_fills(lambda fill: (o.split_raw(dview(xc, "slice", fill)),))
    assert bool(torch.isfinite(s.float()).all())


# ---------------------------------------------------------------------------------------------------- past the grid cap
# grid_for caps a launch at 16 384 blocks of 256 lanes: the grid-stride loops run a second time above 4 194 304 items only.  One case
# per kernel family; every element is checked against something that does not depend on the over-cap launch.
CAP = 16384 * 256


def _nhwc_rand(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, h, w, c, generator=g) * 2 - 1).permute(0, 3, 1, 2)


def test_maxpool2_past_the_grid_cap_equals_cpu():
    o = ops()
    n, c, h, w = 1, 8, 2900, 2896
    assert n * (h // 2) * (w // 2) * (c // 4) > CAP
    xc = _nhwc_rand(n, c, h, w, 31)
    dyc = _nhwc_rand(n, c, h // 2, w // 2, 32)
    xr = xc.contiguous().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    (dxr,) = torch.autograd.grad(yr, xr, dyc.contiguous())
    x = xc.to(DEV).requires_grad_(True)
    assert o.is_nhwc_view(x)
    y = o.maxpool2(x)
    (dx,) = torch.autograd.grad(y, x, dyc.to(DEV))
    assert torch.equal(y.cpu(), yr.detach()) and torch.equal(dx.cpu(), dxr)


def test_upsample2_past_the_grid_cap_equals_its_half_batches():
    """Not exact: the over-cap launch equals, bit for bit, the same op on two half-batches that stay under the cap; those are held
    to fp64 per element (forward: everywhere; backward: the 12 top and bottom rows, from a crop of the gradient)."""
    o = ops()
    n, c, h, w = 2, 4, 730, 730
    assert n * 4 * h * w * (c // 4) > CAP > 4 * h * w * (c // 4)
    xc = _nhwc_rand(n, c, h, w, 33)
    x = xc.to(DEV)
    y = o.upsample2(x)
    halves = torch.cat([o.upsample2(x[:1]), o.upsample2(x[1:])])
    assert torch.equal(y, halves)
    want = F.interpolate(xc.double(), scale_factor=2, mode="bilinear", align_corners=False)
    bound = R.SAFETY * R.UP_FWD_K * R.U * F.interpolate(xc.abs().double(), scale_factor=2, mode="bilinear", align_corners=False)
    R.assert_within(y, want, bound, "upsample2_fwd past the cap")
    del y, halves, want, bound
    n, c, h, w = 2, 8, 1028, 1028                           # backward: one item per INPUT float4
    assert n * h * w * (c // 4) > CAP > h * w * (c // 4)
    dyc = _nhwc_rand(n, c, 2 * h, 2 * w, 34)
    dy = dyc.to(DEV)
    L_ = L()
    dx = ops().nhwc_empty(n, c, h, w, DEV)
    assert L_.wcmc_upsample2_bwd(*V(dy), *V(dx), n, h, w, c, stream()) == 0
    for i in range(2):
        half = ops().nhwc_empty(1, c, h, w, DEV)
        assert L_.wcmc_upsample2_bwd(*V(dy[i:i + 1]), *V(half), 1, h, w, c, stream()) == 0
        assert torch.equal(dx[i:i + 1], half)
    for rows, crop in ((slice(0, 12), dyc[:, :, :32]), (slice(h - 12, h), dyc[:, :, -32:])):
        wantb, boundb = R.upsample2_bwd(crop.contiguous())
        sub = slice(0, 12) if rows.start == 0 else slice(4, 16)
        R.assert_within(dx[:, :, rows].cpu(), wantb[:, :, sub], boundb[:, :, sub], "upsample2_bwd past the cap")


def test_spp_reduce_and_broadcast_past_the_grid_cap_equal_cpu():
    """S = 2: fl(x0 + x1) * 0.5 and g * 0.5 are single roundings, so CPU fp32 is the exact answer."""
    b, s, c, h, w = 2, 2, 4, 1456, 1456
    assert b * h * w * (c // 4) > CAP
    xc = _nhwc_rand(b * s, c, h, w, 35)
    x = xc.to(DEV)
    y = ops().nhwc_empty(b, c, h, w, DEV)
    assert L().wcmc_spp_reduce(*V(x), *V(y), b, s, h, w, c, 0.5, stream()) == 0
    v = xc.reshape(b, s, c, h, w)
    assert torch.equal(y.cpu(), (v[:, 0] + v[:, 1]) * 0.5)
    out = ops().nhwc_empty(b * s, c, h, w, DEV)
    assert L().wcmc_spp_broadcast(*V(y), *V(out), b, s, h, w, c, 0.5, 0, stream()) == 0
    assert torch.equal(out.cpu(), (y.cpu() * 0.5).repeat_interleave(s, 0))


def test_pbuffer_cat_bwd_and_sample_cat_past_the_grid_cap():
    o = ops()
    b, s, cb, cp, h, w = 1, 2, 1, 1, 2050, 2050
    assert b * h * w > CAP
    gc = _nhwc_rand(b, cb + cp + 1, h, w, 36)
    dp = o.nhwc_empty(b * s, cp, h, w, DEV).unflatten(0, (b, s))
    g = R.nhwc_buffer(b, cb + cp + 1, h, w, 0.0, device=DEV, valid=gc)[0]
    assert L().wcmc_pbuffer_cat_bwd(*V(g), ctypes.c_void_p(dp.data_ptr()), *dp.stride(), b, s, cb, cp, h, w, stream()) == 0
    assert torch.equal(dp.cpu(), R.pbuffer_cat_bwd(gc, s, cb, cp))
    del dp, g
    pc = R.rnd(b, s, cp, h, w, seed=37)
    featc = R.rnd(b, s, cb, h, w, seed=38)
    out = o.sample_features_cat(featc.to(DEV), pc.to(DEV)).cpu()
    want, bound = R.sample_cat(featc, pc)
    assert torch.equal(out[:, :, :cb + cp], torch.cat([featc, pc], 2))
    R.assert_within(out[:, :, cb + cp:], want[:, :, cb + cp:], bound[:, :, cb + cp:], "sample_cat_var past the cap")
