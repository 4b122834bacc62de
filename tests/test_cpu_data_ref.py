"""The yardstick of tests/test_gpu_data_edges.py, checked without a GPU (tests/data_ref.py):
  * the fp64 values agree with oracle/datasets.py (numpy fp32, pinned to the reference's own outputs) inside the bounds;
  * the bounds are honest: fp32 emulations of the three summation orders in play -- sequential (pp_kpcn_stats_kernel, the prefix
    pass), an xor tree (pp_kpcn_stats_lanes_kernel) and numpy's -- stay inside them on the frames the GPU tests use;
  * the comparison can fail: each wrong variant of the functions falls outside them on those same frames."""
import os
import sys

import numpy as np
import pytest

import data_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from oracle import datasets as od  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "preprocess.npz")


def fails(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


def frame(h, w, s, md=5, C=None, seed=0, **kw):
    return R.make_frame(h, w, s, md, C, seed, **kw).numpy()


def oracle_kpcn(raw, md=5):
    with np.errstate(all="ignore"):
        return od.preprocess_kpcn(raw, md)


# ---------------------------------------------------------------------------------------------------- fp32 emulations
def sum32(v, order):
    """Sum of (h, w, s, c) fp32 over the samples in one of the three orders."""
    s = v.shape[2]
    if order == "sequential":
        acc = np.zeros(v.shape[:2] + v.shape[3:], np.float32)
        for k in range(s):
            acc = acc + v[:, :, k]
        return acc
    if order == "xor":
        assert s & (s - 1) == 0
        a, o, lanes = v.copy(), 1, np.arange(s)
        while o < s:
            a = a + a[:, :, lanes ^ o]
            o <<= 1
        return a[:, :, 0]
    return np.ascontiguousarray(np.moveaxis(v, 2, -1)).sum(-1)               # numpy's pairwise loop over a contiguous axis


def kpcn_fp32(raw, md, order, clip_drops_nan=False):
    """_preprocess_kpcn in fp32 as the kernels form it (csrc/data_step.h), with the sums in ``order``."""
    f = np.float32
    x = raw[..., R.kpcn_channels(md)]
    s = f(x.shape[2])
    eps = f(0.00316)
    with np.errstate(all="ignore"):
        difp = np.maximum(x[..., 3:6], f(0))
        spec = np.maximum(np.maximum(x[..., 0:3], f(0)) - difp, f(0))

        def mv(v):
            mean = sum32(v, order) / s
            d = v - mean[:, :, None]
            return mean, sum32(d * d, order) / s

        gvar = lambda var: ((var[..., 0:1] + var[..., 1:2] + var[..., 2:3]) / f(3)) / s          # noqa: E731
        sqr = lambda a: (a[..., 0:1] * a[..., 0:1] + a[..., 1:2] * a[..., 1:2] + a[..., 2:3] * a[..., 2:3]) / f(3)  # noqa: E731
        normal, nv = mv(x[..., 9:12])
        depth, dv = mv(x[..., 12:13])
        albedo, av = mv(x[..., 6:9])
        diffuse, fv = mv(difp)
        specular, sv = mv(spec)
        M = max(f(depth.max()), f(0))
        if M > 0:
            depth, dv = depth / M, dv / (M * M * s)
        nan = np.isnan(depth)
        depth = np.clip(depth, f(0), f(1))
        if clip_drops_nan:
            depth = np.where(nan, f(0), depth)
        a, t = albedo + eps, f(1) + specular
        feats = []
        for val, var in ((diffuse / a, gvar(fv) / sqr(a)), (np.log(t), gvar(sv) / sqr(t)), (normal, gvar(nv)), (depth, dv),
                         (albedo, gvar(av))):
            feats += [val, var, R.gradients(val)]
        out = np.concatenate(feats, 2)
    assert out.dtype == np.float32
    return out


# ---------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name", ["a", "b", "zero_depth"])
def test_reference_holds_the_recorded_outputs_of_the_reference_implementation(name):
    d = np.load(GOLDEN)
    raw = d[name + "/raw"]
    want, bound = R.kpcn(raw)
    R.assert_within(d[name + "/kpcn"], want, bound, "kpcn golden " + name)
    R.assert_within(oracle_kpcn(raw), want, bound, "kpcn oracle " + name)
    want, bound = R.llpm(raw)
    R.assert_within(d[name + "/llpm"], want, bound, "llpm golden " + name)
    R.assert_within(od.preprocess_llpm(raw), want, bound, "llpm oracle " + name)


def test_gradients_reference_is_bit_equal_to_the_recorded_output():
    d = np.load(GOLDEN)
    R.assert_bit_equal(R.gradients(d["grad/buf"]), d["grad/out"], "gradients golden")
    R.assert_bit_equal(R.gradients(d["grad/buf"]), od.gradients(d["grad/buf"]), "gradients oracle")
    assert fails(R.assert_bit_equal, R.gradients(d["grad/buf"], forward=True), d["grad/out"])


@pytest.mark.parametrize("md,C", R.MAPS)
def test_reference_agrees_with_the_oracle_for_every_channel_map(md, C):
    for h, w in R.SMALL_SHAPES:
        for s in (3, 4):
            raw = frame(h, w, s, md, C, seed=10 * md + s)
            want, bound = R.kpcn(raw, md)
            assert not np.isnan(want).any()
            R.assert_within(oracle_kpcn(raw, md), want, bound, "kpcn %dx%dx%d md %d C %d" % (h, w, s, md, C))
        raw = frame(h, w, 2, md, C, seed=7, fill="llpm")
        want, bound = R.llpm(raw, md)
        assert want.shape == (h, w, 2, 7 + 5 * (md + 1)) and not np.isnan(want).any()
        with np.errstate(all="ignore"):
            R.assert_within(od.preprocess_llpm(raw, md), want, bound, "llpm %dx%d md %d C %d" % (h, w, md, C))
        # the compact form the large GPU cases use: the channels from the bounce types on
        w2, b2 = R.llpm_tail(raw[..., R.cmap(md)["bounce"]:], md)
        assert np.array_equal(w2, want) and np.array_equal(b2, bound)


@pytest.mark.parametrize("kind", ["zero", "negative", "one_positive", "first", "last"])
def test_reference_depth_maximum_cases_agree_with_the_oracle(kind):
    for s in (3, 4):
        raw = frame(5, 7, s, seed=20 + s, depth=kind)
        want, bound = R.kpcn(raw)
        R.assert_within(oracle_kpcn(raw), want, bound, "depth %s s %d" % (kind, s))
        R.assert_within(kpcn_fp32(raw, 5, "sequential"), want, bound, "depth %s s %d (fp32)" % (kind, s))
        d = want[..., 30].reshape(-1)
        if kind in ("zero", "negative"):
            assert float(np.abs(d).max()) == 0.0 and float(np.abs(want[..., 32:34]).max()) == 0.0
        else:
            q = {"one_positive": 17, "first": 0, "last": 34}[kind]
            assert d[q] == 1.0 and int(d.argmax()) == q
            if kind == "one_positive":
                assert float(np.delete(d, q).max()) == 0.0


# ---------------------------------------------------------------------------------------------------- the bounds are honest
@pytest.mark.parametrize("s", R.LANES_S + R.PIXEL_S)
def test_fp32_summation_orders_stay_inside_the_bounds(s):
    orders = ["sequential", "numpy"] + (["xor"] if s & (s - 1) == 0 else [])
    for h, w in R.SMALL_SHAPES:
        raw = frame(h, w, s, seed=100 + s)
        want, bound = R.kpcn(raw)
        for order in orders:
            R.assert_within(kpcn_fp32(raw, 5, order), want, bound, "%s %dx%dx%d" % (order, h, w, s))
        R.assert_within(oracle_kpcn(raw), want, bound, "oracle %dx%dx%d" % (h, w, s))


def test_fp32_prefixes_stay_inside_the_bounds_of_their_own_prefix():
    raw = frame(21, 19, 8, seed=3)
    for s in range(1, 9):
        want, bound = R.kpcn(raw[:, :, :s])
        R.assert_within(kpcn_fp32(np.ascontiguousarray(raw[:, :, :s]), 5, "sequential"), want, bound, "prefix of %d" % s)


@pytest.mark.parametrize("S", [3, 5, 8, 64])
def test_fp32_prefixes_of_the_own_maximum_frames_stay_inside_the_bounds(S):
    for h, w in ((5, 7), (21, 19)):
        raw = R.own_maximum_frame(h, w, S).numpy()
        for s in sorted({1, 2, 3, S // 2 + 1, S}):
            sub = np.ascontiguousarray(raw[:, :, :s])
            want, bound = R.kpcn(sub)
            R.assert_within(kpcn_fp32(sub, 5, "sequential"), want, bound, "prefix of %d of %d" % (s, S))
            R.assert_within(oracle_kpcn(sub), want, bound, "prefix of %d of %d, oracle" % (s, S))
            assert (int(want[..., 30].argmax()) == (h * w) // 3) == (s > 1) and float(want[..., 30].max()) == 1.0


# ---------------------------------------------------------------------------------------------------- the comparison can fail
@pytest.mark.parametrize("h,w", R.SMALL_SHAPES)
@pytest.mark.parametrize("s", [3, 4, 64])
def test_wrong_variants_fall_outside_the_bounds(h, w, s):
    """On the frames of the GPU dispatch test (seed 100 + s)."""
    raw = frame(h, w, s, seed=100 + s)
    want, bound = R.kpcn(raw)
    ok = kpcn_fp32(raw, 5, "sequential")
    R.assert_within(ok, want, bound, "right")
    variants = ["ddof", "no_spp", "unclamped"] + (["forward"] if h * w > 1 else [])
    for v in variants:
        assert fails(R.assert_within, R.kpcn(raw, wrong=v)[0], want, bound, v), v + " passed"
    assert fails(R.assert_within, R.kpcn(raw, shift=1)[0], want, bound, "shift"), "channel offsets + 1 passed"
    # ONE element off: the normal's variance by 1e-4 relative; the albedo mean (positive samples: mean|v| = mean, bound 2 s U mean)
    # by twice its bound
    for c, rel in ((23, 1e-4), (34, 4 * (s + 1) * R.U)):
        off = ok.copy()
        off[0, 0, c] *= np.float32(1.0 + rel)
        if off[0, 0, c] != ok[0, 0, c]:
            assert fails(R.assert_within, off, want, bound, "off"), (c, rel)


@pytest.mark.parametrize("md,C", [(0, 49), (5, 104), (6, 115)])
def test_wrong_llpm_variants_fall_outside_the_bounds(md, C):
    raw = frame(5, 7, 2, md, C, seed=9, fill="llpm")
    want, bound = R.llpm(raw, md)
    assert fails(R.assert_within, R.llpm(raw, md, shift=1)[0], want, bound, "shift"), "channel offsets + 1 passed"
    assert fails(R.assert_within, R.llpm(raw, md, shift=-1)[0], want, bound, "shift"), "channel offsets - 1 passed"
    with np.errstate(all="ignore"):
        off = od.preprocess_llpm(raw, md)
    off[2, 3, 1, 0] *= np.float32(1.0 + 64 * R.U)
    assert fails(R.assert_within, off, want, bound, "off")


@pytest.mark.parametrize("s", [3, 4])
def test_a_maximum_over_one_trip_falls_outside_the_bounds(s):
    """On the frame of the GPU maximum test whose deepest pixel is the last one: a maximum that misses the pixels of a second trip
    normalises by another pixel's depth."""
    raw = frame(5, 7, s, seed=20 + s, depth="last")
    want, bound = R.kpcn(raw)
    for n in (34, 17, 1):
        assert fails(R.assert_within, R.kpcn(raw, max_pixels=n)[0], want, bound, "max"), "a maximum over the first %d pixels passed" % n


# ---------------------------------------------------------------------------------------------------- the overflowing depth mean
overflow_frame = R.overflow_frame


@pytest.mark.parametrize("s", [4, 5])
def test_overflowing_depth_mean_has_the_oracles_nan_pattern(s):
    raw = overflow_frame(s)
    want, bound = R.kpcn(raw)
    nan = np.isnan(want)
    expect = np.zeros_like(nan)
    expect[2, 3, 30:34] = True
    expect[2, 4, 32] = True
    expect[3, 3, 33] = True
    assert np.array_equal(nan, expect)
    assert float(np.abs(want[..., 30][~nan[..., 30]]).max()) == 0.0           # finite / Inf
    for order in ("sequential", "numpy") + (("xor",) if s == 4 else ()):
        R.assert_within(kpcn_fp32(raw, 5, order), want, bound, "overflow %s" % order)
    R.assert_within(oracle_kpcn(raw), want, bound, "overflow oracle")
    # the clip the kernel had: fminf(fmaxf(d, 0), 1) gives 0 for the NaN
    assert fails(R.assert_within, kpcn_fp32(raw, 5, "sequential", clip_drops_nan=True), want, bound, "old clip")
    assert fails(R.assert_within, R.kpcn(raw, wrong="clip_nan")[0], want, bound, "old clip")


def test_prefixes_of_the_overflow_frame_overflow_at_four_samples_only():
    raw = overflow_frame(4)
    for s in (1, 2, 3):
        want, bound = R.kpcn(raw[:, :, :s])
        assert not np.isnan(want).any() and want[2, 3, 30] == 1.0 and float(np.abs(want[..., 31]).max()) == 0.0   # M^2 overflows
        R.assert_within(kpcn_fp32(np.ascontiguousarray(raw[:, :, :s]), 5, "sequential"), want, bound, "prefix of %d" % s)
        R.assert_within(oracle_kpcn(np.ascontiguousarray(raw[:, :, :s])), want, bound, "prefix of %d oracle" % s)
    assert np.isnan(R.kpcn(raw)[0][2, 3, 30])
