"""The fused PathNet.embedding reading the channel-first ``paths`` where it lies (the ``x_nchw`` source of ``wcmc_embed3_mean_fwd`` /
``wcmc_embed3_bwd``, ``ops.embed_in_place``) against the same fused chain on the split copy (``ops.presplit_shared``): y, its spp mean and the six parameter
gradients BIT FOR BIT -- the in-place kernels split with the split pass's arithmetic into the very LDS tile the GEMMs read, and
everything behind that tile is the same code."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ACTS = ["relu", "relu", "linear"]


def ops():
    from wcmc_amd import ops as _ops
    return _ops


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _params(cin, seed):
    ws = [gen(64, cin, 1, 1, seed=seed, scale=(2.0 / cin) ** 0.5 * 1.7), gen(64, 64, 1, 1, seed=seed + 1, scale=(2.0 / 64) ** 0.5 * 1.7),
          gen(64, 64, 1, 1, seed=seed + 2, scale=(2.0 / 64) ** 0.5 * 1.7)]
    bs = [gen(64, seed=seed + 3 + i, scale=0.2) for i in range(3)]
    return [t for pair in zip(ws, bs) for t in pair]


def _run(o, xd, s, params, gy, gm):
    """One forward + backward of the chain on the prepared input xd; gy / gm: device gradients of y / its mean (either may be None)."""
    ps = [t.to(DEV).requires_grad_(True) for t in params]
    y, m = o.conv_chain_spp_mean(xd, s, 1, 0, ACTS, ps)
    outs, grads = zip(*[(t, g) for t, g in ((y, gy), (m, gm)) if g is not None])
    torch.autograd.backward(list(outs), list(grads))
    torch.cuda.synchronize()
    return y.detach().clone(), m.detach().clone(), [t.grad.clone() for t in ps]


def _assert_same(a, b):
    assert torch.equal(a[0], b[0]), "y"
    assert torch.equal(a[1], b[1]), "spp mean"
    for ga, gb, name in zip(a[2], b[2], ("dw0", "db0", "dw1", "db1", "dw2", "db2")):
        assert torch.equal(ga, gb), name


def _both(o, x_dev, s, params, gy, gm, expect_in_place=True):
    """The chain on embed_in_place(x) and on presplit_shared(a copy of x)."""
    assert o.reduced_backward() and o.FUSE_EMBED and o.EMBED_IN_PLACE
    assert o.embed_in_place_supported(x_dev) == expect_in_place
    xi = o.embed_in_place(x_dev)
    assert o._reads_in_place(xi) == expect_in_place
    assert (getattr(xi, "_wcmc_split", None) is None) == expect_in_place        # refused: today's split pass
    got = _run(o, xi, s, params, gy, gm)
    want = _run(o, o.presplit_shared(x_dev.clone()), s, params, gy, gm)
    _assert_same(got, want)
    return got


# (B*S, S, Cin, H, W): smallest; second smallest; more samples per pixel; fewest / most input channels; 432 units for 256 workgroups (the
# backward's grid-stride loop and both prefetches run)
CASES = [(2, 1, 36, 8, 8), (4, 2, 36, 8, 16), (16, 8, 36, 16, 16), (4, 2, 8, 8, 8), (4, 2, 64, 8, 8), (6, 2, 36, 96, 96)]


@pytest.mark.parametrize("case", CASES)
def test_in_place_equals_the_split_copy_bit_for_bit(case):
    o = ops()
    n, s, cin, h, w = case
    x = gen(n, cin, h, w, seed=500).to(DEV)
    gy = o.to_nhwc_raw(gen(n, 64, h, w, seed=501).to(DEV))
    gm = o.to_nhwc_raw(gen(n // s, 64, h, w, seed=502).to(DEV))
    got = _both(o, x, s, _params(cin, 510), gy, gm)
    assert all(torch.isfinite(t).all() for t in got[2]) and got[0].abs().max() > 0


def test_source_that_is_a_slice_of_a_larger_buffer_in_n_and_c():
    """Sample and channel strides are those of the parent; the channel rows behind Cin belong to the parent and must not be read
    as data (they hold a large sentinel here)."""
    o = ops()
    n, s, cin, h, w = 4, 2, 36, 8, 16
    big = torch.full((n + 3, cin + 9, h, w), 1.0e30, device=DEV)
    x = big[2:2 + n, 5:5 + cin]
    x.copy_(gen(n, cin, h, w, seed=520).to(DEV))
    assert not x.is_contiguous() and x.stride(1) == h * w and x.stride(0) == (cin + 9) * h * w
    gy = o.to_nhwc_raw(gen(n, 64, h, w, seed=521).to(DEV))
    gm = o.to_nhwc_raw(gen(n // s, 64, h, w, seed=522).to(DEV))
    got = _both(o, x, s, _params(cin, 530), gy, gm)
    assert all(torch.isfinite(t).all() and t.abs().max() < 1.0e6 for t in (got[0], got[1], *got[2]))


def test_gradient_of_y_as_a_channel_slice_and_a_missing_gradient_of_the_mean():
    o = ops()
    n, s, cin, h, w = 4, 2, 36, 8, 16
    x = gen(n, cin, h, w, seed=540).to(DEV)
    gwide = o.to_nhwc_raw(gen(n, 128, h, w, seed=541).to(DEV))       # g_y: the first 64 channels of the concatenation's gradient
    gm = o.to_nhwc_raw(gen(n // s, 64, h, w, seed=542).to(DEV))
    params = _params(cin, 550)
    _both(o, x, s, params, gwide[:, :64], gm)
    _both(o, x.clone(), s, params, gwide[:, :64], None)              # no gradient of the mean
    _both(o, x.clone(), s, params, None, gm)                         # ... and none of y


@pytest.mark.parametrize("which", ["ragged", "wstride2"])
def test_refused_sources_take_the_split_pass_and_give_the_same_result(which):
    """H * W % 64 != 0 (a tile would straddle two samples) and a plane that is not contiguous: the query says no, embed_in_place makes
    the split copy, and the result is that of presplit_shared."""
    o = ops()
    if which == "ragged":
        n, s, cin, h, w = 6, 3, 36, 20, 23
        x = gen(n, cin, h, w, seed=560).to(DEV)
    else:
        n, s, cin, h, w = 4, 2, 36, 8, 8
        x = gen(n, cin, h, 2 * w, seed=561).to(DEV)[..., ::2]
        assert x.stride(3) == 2
    gy = o.to_nhwc_raw(gen(n, 64, h, w, seed=562).to(DEV))
    gm = o.to_nhwc_raw(gen(n // s, 64, h, w, seed=563).to(DEV))
    _both(o, x, s, _params(cin, 570), gy, gm, expect_in_place=False)


def test_switch_off_and_a_tag_that_outlives_its_switch(monkeypatch):
    """EMBED_IN_PLACE off: embed_in_place is presplit_shared.  A tag made while it was on, met by the layer-by-layer chain (FUSE_EMBED
    off afterwards): that chain makes its own split and computes what it computes from presplit_shared."""
    o = ops()
    n, s, cin, h, w = 4, 2, 36, 8, 16
    x = gen(n, cin, h, w, seed=580).to(DEV)
    gy = o.to_nhwc_raw(gen(n, 64, h, w, seed=581).to(DEV))
    gm = o.to_nhwc_raw(gen(n // s, 64, h, w, seed=582).to(DEV))
    params = _params(cin, 590)
    tagged = o.embed_in_place(x.clone())
    assert o._reads_in_place(tagged)
    monkeypatch.setattr(o, "EMBED_IN_PLACE", False)
    off = o.embed_in_place(x.clone())
    assert getattr(off, "_wcmc_split", None) is not None and not o._reads_in_place(off)
    monkeypatch.setattr(o, "EMBED_IN_PLACE", True)
    monkeypatch.setattr(o, "FUSE_EMBED", False)
    got = _run(o, tagged, s, params, gy, gm)
    want = _run(o, o.presplit_shared(x.clone()), s, params, gy, gm)
    _assert_same(got, want)
