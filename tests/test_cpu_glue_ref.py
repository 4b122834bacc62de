"""The yardstick of the glue and optimiser-tail GPU tests, checked without a GPU (tests/glue_ref.py):
  * every reference equals the torch functional it stands for;
  * every bound is honest: an fp32 emulation of the kernel's own formula stays inside it, on every input the GPU tests use;
  * every comparison can fail: a deliberately wrong variant of each op fails the same comparison function the GPU test calls."""
import math

import pytest
import torch
import torch.nn.functional as F

import glue_ref as R


def fails(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("kind", R.POOL_KINDS)
@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_maxpool_reference_is_max_pool2d_with_its_autograd(shape, kind):
    x = R.pool_data(shape, kind, seed=3).requires_grad_(True)
    y = F.max_pool2d(x, 2)
    dy = R.rnd(*y.shape, seed=4)
    add = R.rnd(*shape, seed=5)
    (dx,) = torch.autograd.grad(y, x, dy)
    R.assert_bit_equal(R.maxpool2_fwd(x.detach()), y.detach(), "fwd")
    R.assert_bit_equal(R.maxpool2_bwd(x.detach(), dy), dx, "bwd")
    # the skip connection's gradient arrives by autograd's one add
    x2 = x.detach().clone().requires_grad_(True)
    (F.max_pool2d(x2, 2) * dy).sum().backward()
    (x2 * add).sum().backward()
    R.assert_bit_equal(R.maxpool2_bwd(x.detach(), dy, add), x2.grad, "bwd_add")


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_wrong_maxpool_variants_fail_the_bitwise_comparison(shape):
    dy = R.rnd(shape[0], shape[1], shape[2] // 2, shape[3] // 2, seed=4) + 2.0        # (no zero gradient that would hide a route)
    for kind in ("ties", "relu"):
        x = R.pool_data(shape, kind, seed=3)
        assert fails(R.assert_bit_equal, R.maxpool2_bwd(x, dy, tie="last"), R.maxpool2_bwd(x, dy)), "last maximum on ties passed"
    x = R.pool_data(shape, "nan", seed=3)
    assert fails(R.assert_bit_equal, R.maxpool2_fwd(x, nan="drop"), R.maxpool2_fwd(x)), "a dropped NaN passed (forward)"
    assert fails(R.assert_bit_equal, R.maxpool2_bwd(x, dy, nan="drop"), R.maxpool2_bwd(x, dy)), "a dropped NaN passed (backward)"
    # what the kernel did before this test existed (first-maximum routing whose `>` never selects a NaN): position 0 keeps the gradient
    if x[0, 0].numel() > 4 or shape[1] > 1:
        w = R.windows(x)
        k_old = torch.zeros(w[0].shape, dtype=torch.int64)
        m = w[0].clone()
        for j in range(1, 4):
            upd = w[j] > m
            m, k_old = torch.where(upd, w[j], m), torch.where(upd, torch.full_like(k_old, j), k_old)
        old = R.unwindows(torch.stack([torch.where(k_old == j, dy, torch.zeros_like(dy)) for j in range(4)]))
        assert fails(R.assert_bit_equal, old, R.maxpool2_bwd(x, dy))


# ---------------------------------------------------------------------------------------------------- bilinear x2
@pytest.mark.parametrize("shape", R.UP_SHAPES)
def test_upsample_reference_bound_and_wrong_variant(shape):
    x = R.rnd(*shape, seed=7)
    xd = x.double().requires_grad_(True)
    y = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False)
    dy = R.rnd(*y.shape, seed=8)
    (dx,) = torch.autograd.grad(y, xd, dy.double())
    want, bound = R.upsample2_fwd(x)
    assert torch.allclose(want, y.detach(), rtol=0, atol=1e-15)
    wantb, boundb = R.upsample2_bwd(dy)
    assert torch.allclose(wantb, dx, rtol=0, atol=1e-14)
    R.assert_within(R.upsample2_fwd_fp32(x), want, bound, "upsample2_fwd(fp32 emulation)")
    R.assert_within(R.upsample2_bwd_fp32(dy), wantb, boundb, "upsample2_bwd(fp32 emulation)")
    # without the border clamp every border pixel is off by a quarter of its neighbour
    assert fails(R.assert_within, R.upsample2_fwd(x, clamp=False)[0], want, bound, "wrong")
    assert fails(R.assert_within, R.upsample2_bwd(dy, clamp=False)[0], wantb, boundb, "wrong")
    # and an error of a few ulps at ONE border pixel fails, which the max-norm metric over the tensor lets through
    off = R.upsample2_fwd_fp32(x)
    off[0, 0, -1, -1] *= 1.0 + 32 * R.U
    assert fails(R.assert_within, off, want, bound, "wrong")


# ---------------------------------------------------------------------------------------------------- spp mean, broadcast, cat
@pytest.mark.parametrize("shape", R.SPP_SHAPES)
def test_spp_mean_reference_bound_and_wrong_variant(shape):
    b, s, c, h, w = shape
    x = R.rnd(b * s, c, h, w, seed=9)
    xd = x.double().requires_grad_(True)
    y = xd.view(b, s, c, h, w).mean(1)                     # networks.py:35-36
    g = R.rnd(b, c, h, w, seed=10)
    (dx,) = torch.autograd.grad(y, xd, g.double())
    want, bound = R.spp_reduce(x, s, 1.0 / s)
    assert torch.allclose(want, y.detach(), rtol=1e-15, atol=0)
    R.assert_within(R.spp_reduce_fp32(x, s, 1.0 / s), want, bound, "spp_reduce(fp32 emulation)")
    # the broadcast backward: one multiply by fl(1/S) -- torch divides by S: equal for S a power of two, one rounding apart otherwise
    got = R.spp_broadcast(g, s, 1.0 / s)
    if s & (s - 1) == 0:
        R.assert_bit_equal(got, dx.float(), "spp_broadcast")
    R.assert_within(got, dx, R.SAFETY * R.U * dx.abs(), "spp_broadcast(vs torch's division)")
    R.assert_bit_equal(R.spp_broadcast(g, s, 1.0 / s, into=x), x + got, "accumulate")
    if s > 1:                                              # wrong: one sample left out
        assert fails(R.assert_within, R.spp_reduce_fp32(x[: b * s - 1].repeat(2, 1, 1, 1)[: b * s], s, 1.0 / s), want, bound, "wrong")


@pytest.mark.parametrize("shape", R.CATB_SHAPES)
def test_cat_references_are_the_expressions_of_the_networks(shape):
    b, s, c1, c2, h, w = shape
    flat, prop = R.rnd(b * s, c1, h, w, seed=11), R.rnd(b, c2, h, w, seed=12)
    want = torch.cat([flat, prop.unsqueeze(1).repeat(1, s, 1, 1, 1).view(b * s, c2, h, w)], 1)      # networks.py:39-40
    R.assert_bit_equal(R.cat_broadcast(flat, prop, s), want, "cat_broadcast")
    R.assert_bit_equal(R.cat_channels(flat, flat[:, :c1]), torch.cat([flat, flat], 1), "cat_channels")
    # its backward into prop is the sum over the samples
    g = R.rnd(b * s, c1 + c2, h, w, seed=13)
    pd = prop.double().requires_grad_(True)
    out = torch.cat([flat.double(), pd.unsqueeze(1).repeat(1, s, 1, 1, 1).view(b * s, c2, h, w)], 1)
    (dp,) = torch.autograd.grad(out, pd, g.double())
    wantr, bound = R.spp_reduce(g[:, c1:], s, 1.0)
    assert torch.allclose(wantr, dp, rtol=1e-15, atol=1e-300)
    R.assert_within(R.spp_reduce_fp32(g[:, c1:].contiguous(), s, 1.0), wantr, bound, "cat_broadcast_bwd(fp32 emulation)")
    if s > 1:
        assert fails(R.assert_bit_equal, R.cat_broadcast(flat, prop.flip(0) if b > 1 else prop * 1.0000001, s), want)


# ---------------------------------------------------------------------------------------------------- P-buffer cat, sample cat
@pytest.mark.parametrize("w", R.PB_W)
def test_pbuffer_cat_reference_bound_and_wrong_variants(w):
    for s, h, cb, cp in R.PB_REST:
        b = 2 if w < 100 else 1
        base, p = R.rnd(b, cb, h, w, seed=14), R.pdata(b, s, cp, h, w, seed=15)
        ref = torch.cat([base.double(), p.double().mean(1), p.double().var(1).mean(1, keepdim=True) / s], 1)       # interfaces.py:165-176
        want, bound = R.pbuffer_cat(base, p)
        assert torch.equal(want, ref)
        mean, var = R.pstats_fp32(p)
        got = torch.cat([base, mean, var], 1)
        R.assert_within(got, want, bound, "pbuffer_cat(fp32 emulation)")
        if w > 1:                                              # constant over the samples: the variance is exactly 0
            assert float(var[..., w - 1].abs().max()) == 0.0 and float(want[:, -1, :, w - 1].abs().max()) == 0.0
        # wrong: biased variance (S = 2: half of it; S = 8: 7/8)
        assert fails(R.assert_within, R.pbuffer_cat(base, p, biased=True)[0], want, bound, "wrong")
        # wrong: one-pass variance at |mean| = 100 sigma
        _, var1 = R.pstats_fp32(p, one_pass=True)
        assert fails(R.assert_within, torch.cat([base, mean, var1], 1), want, bound, "wrong")
        # the sample-based form
        feat = R.rnd(b, s, cb, h, w, seed=16)
        ref2 = torch.cat([feat.double(), p.double(), (p.double().var(1).mean(1, keepdims=True) / s).unsqueeze(1).repeat(1, s, 1, 1, 1)], 2)
        want2, bound2 = R.sample_cat(feat, p)
        assert torch.equal(want2, ref2)
        R.assert_within(torch.cat([feat, p, var.unsqueeze(1).expand(-1, s, -1, -1, -1)], 2), want2, bound2, "sample_cat(fp32 emulation)")
        # backward: mean's share, 1/S of the gradient of the mean channels to every sample
        g = R.rnd(b, cb + cp + 1, h, w, seed=17)
        pd = p.double().requires_grad_(True)
        out = torch.cat([base.double(), pd.mean(1), (pd.var(1).mean(1, keepdim=True) / s).detach()], 1)
        (dp,) = torch.autograd.grad(out, pd, g.double())
        gotb = R.pbuffer_cat_bwd(g, s, cb, cp)
        R.assert_within(gotb, dp, R.SAFETY * R.U * dp.abs(), "pbuffer_cat_bwd(vs torch's division)")
        if s & (s - 1) == 0:
            R.assert_bit_equal(gotb, dp.float(), "pbuffer_cat_bwd")


# ---------------------------------------------------------------------------------------------------- clip + Adam
ADAM_N = [1, 2, 3, 4, 5, 7, 1023, 4097]
ADAM_HYPER = [dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8), dict(lr=3e-4, beta1=0.8, beta2=0.95, eps=1e-6)]


def _adam_run(n, hyper, scale, kind, wrong=None, steps=5):
    """(fp32 emulation state, reference) after `steps` steps."""
    p0 = R.rnd(n, seed=20)
    ref = R.AdamRef(p0, wrong=wrong, **hyper)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    h = (hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"])
    for t in range(1, steps + 1):
        g = R.adam_grads(n, seed=30 + t, kind=kind) / scale
        gc = ref.step(g.clone(), scale)
        adam_fp32_g = g.clone()
        R.adam_fp32_step(p, adam_fp32_g, m, v, t, h, grad_scale=scale)
        if wrong is None:
            R.assert_bit_equal(adam_fp32_g, gc, "clipped gradient")
    return (p, m, v), ref


def adam_compare(state, ref, what):
    """The comparison of the GPU test: NaN positions equal, every other element within the trajectory bound."""
    p, m, v = state
    for got, want, bound, name in ((p, ref.p, ref.Ep, "p"), (m, ref.m, ref.Em, "m"), (v, ref.v, ref.Ev, "v")):
        got = got.detach().cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), "%s %s: NaN positions differ" % (what, name)
        R.assert_within(got[~nan], want[~nan], bound[~nan], "clip_adam(%s) %s" % (name, what))


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("hyper", ADAM_HYPER, ids=["default", "other"])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_reference_is_torch_adam_and_its_bound_holds_the_fp32_formula(n, hyper, scale):
    for kind in ("edges", "nan", "zeros"):
        state, ref = _adam_run(n, hyper, scale, kind)
        adam_compare(state, ref, "fp32 emulation")
        if kind == "zeros":                                # zero gradient, zero moments: nothing moves
            assert torch.equal(state[0], R.rnd(n, seed=20)) and float(state[1].abs().max()) == 0.0
    # torch.optim.Adam + clip_grad_value_ in fp64 (its scalars are not rounded to fp32: 2 U relative on each of the seven)
    pr = R.rnd(n, seed=20).double().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"])
    ref = R.AdamRef(R.rnd(n, seed=20), **hyper)
    for t in range(1, 6):
        g = R.adam_grads(n, seed=30 + t)
        pr.grad = g.double()
        torch.nn.utils.clip_grad_value_([pr], 1.0)
        opt.step()
        gc = ref.step(g)
        assert torch.equal(gc.double(), pr.grad)           # (+-Inf clamps to +-clip)
    assert torch.allclose(ref.p, pr.detach(), rtol=0, atol=20 * R.U * hyper["lr"])
    assert torch.allclose(ref.m, opt.state[pr]["exp_avg"], rtol=0, atol=8 * R.U)          # (|gc| <= clip = 1, signs mix)
    assert torch.allclose(ref.v, opt.state[pr]["exp_avg_sq"], rtol=0, atol=8 * R.U)


@pytest.mark.parametrize("n", ADAM_N)
def test_wrong_adam_variants_fail_the_comparison(n):
    hyper = ADAM_HYPER[0]
    state, _ = _adam_run(n, hyper, 1.0, "nan")
    _, wrong = _adam_run(n, hyper, 1.0, "nan", wrong="minmax")              # fminf(fmaxf()) turns the NaN into -clip
    assert fails(adam_compare, state, wrong, "wrong")
    state, _ = _adam_run(n, hyper, 1.0, "edges")
    _, wrong = _adam_run(n, hyper, 1.0, "edges", wrong="no_bc2")            # no bias correction on v
    assert fails(adam_compare, state, wrong, "wrong")


# ---------------------------------------------------------------------------------------------------- step guard
@pytest.mark.parametrize("n", [1, 7, 16])
def test_guard_reference_truth_table_and_wrong_variant(n):
    for bad in (None, R.NAN, R.INF, -R.INF):
        for slot in (0, n - 1):
            for ok in (0.0, 1.0):
                losses = [0.25 * (i + 1) for i in range(n)]
                if bad is not None:
                    losses[slot] = bad
                sums = [1.0 + i for i in range(n)]
                flags, guard, new = R.guard_ref(losses, ok, sums)
                assert guard == (ok if bad is None else 0.0) and flags[n] == guard
                assert flags[:n] == [0.0 if (bad is not None and i == slot) else 1.0 for i in range(n)]
                want = [a + b for a, b in zip(sums, losses)] if guard else sums
                R.assert_bit_equal(new, torch.tensor(want), "sums")
                if bad is not None and (bad != bad or ok):
                    _, _, wrong = R.guard_ref(losses, ok, sums, add_nan=True)
                    assert fails(R.assert_bit_equal, wrong, new)


# ---------------------------------------------------------------------------------------------------- clip_grad_norm_
@pytest.mark.parametrize("sizes", [[1], [4095], [4096], [4097], [8192], [3, 5000, 17, 4096]])
def test_grad_norm_reference_is_clip_grad_norm(sizes):
    gs = [R.rnd(n, seed=40 + i, scale=2.0) for i, n in enumerate(sizes)]
    ps = [torch.zeros(n, dtype=torch.float64).requires_grad_(True) for n in sizes]
    for p, g in zip(ps, gs):
        p.grad = g.double().clone()
    total = torch.nn.utils.clip_grad_norm_(ps, 0.5)
    nrm, rel, coef = R.grad_norm(gs, 0.5)
    assert abs(nrm - float(total)) <= 1e-12 * nrm
    for p, g in zip(ps, gs):
        assert torch.allclose(p.grad, g.double() * coef, rtol=1e-12, atol=0)
    # fp32 emulation of the chunked sum (sequential per lane, then pairwise): inside the bound
    acc = 0.0
    for g in gs:
        for c in g.split(R.GN_CHUNK):
            sq = torch.zeros(4096)
            sq[: c.numel()] = c * c
            lanes = torch.zeros(256)
            for k in range(16):
                lanes = lanes + sq[k * 256:(k + 1) * 256]
            while lanes.numel() > 1:
                lanes = lanes[0::2] + lanes[1::2]
            acc = (torch.tensor(acc, dtype=torch.float32) + lanes[0]).item()
    assert abs(math.sqrt(acc) - nrm) <= rel * nrm
    assert abs(math.sqrt(acc) * (1 + 1e-4) - nrm) > rel * nrm         # and a 1e-4 error of the norm is outside it
