"""The yardsticks of tests/test_gpu_sampling_edges.py and tests/test_gpu_sbmc_edges.py, checked without a GPU:
tests/sampling_ref.py against the reference's goldens (tests/golden/sampling_map.npz) and against scipy's own gaussian_filter +
sobel pipeline at every size the GPU tests use; its wrong variants against the bar those tests hold the kernels to;
data_ref.sbmc against the reference's goldens (tests/golden/sbmc_data.npz) and against its own wrong variant."""
import os
import sys

import numpy as np
import pytest

import data_ref as D
import sampling_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden as mg  # noqa: E402
import make_golden_dataset as mgd  # noqa: E402
import make_golden_sbmc as mgs  # noqa: E402

LIVE = [s for s in R.IMP_SIZES + R.IMP_EXTRA if s not in R.IMP_DEGENERATE]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "sampling_map.npz"))


# ---------------------------------------------------------------------------------------------------- the reference's goldens
@pytest.mark.parametrize("name", list(mgd.IMAGES))
def test_importance_map_restatement_is_within_the_goldens_own_floor(gold, name):
    got = R.importance_map(gold["imp/%s/img" % name])
    assert got.dtype == np.float32
    err, floor = float(np.abs(got.astype(np.float64) - gold["imp/%s/out" % name]).max()), float(gold["imp/%s/floor" % name])
    print("importance_map %s: error %.3e, recorded floor %.3e" % (name, err, floor))
    assert err <= floor


@pytest.mark.parametrize("name", list(mgd.PROBS))
def test_sampling_prob_restatement_is_within_the_goldens_own_floor(gold, name):
    h, w, s, patch, seed, gseed = (int(v) for v in gold["prob/%s/params" % name])
    raw, gt = mg.raw_samples(h, w, s, seed), mgd.test_gt(h, w, gseed)
    assert mgd.raw_checksum(raw) == int(gold["prob/%s/raw_crc" % name])
    want, floor = gold["prob/%s/out" % name], float(gold["prob/%s/floor" % name])
    got = R.sampling_prob(raw, gt, patch, 5)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max() / want.max())
    print("sampling_prob %s: error %.3e of the maximum, recorded floor %.3e" % (name, err, floor))
    assert err <= floor
    assert abs(float(got.astype(np.float64).sum()) - float(want.astype(np.float64).sum())) <= 4 * np.finfo(np.float32).eps


# ---------------------------------------------------------------------------------------------------- scipy
def _scipy_map(img):
    from scipy.ndimage import gaussian_filter, sobel
    img = img[..., None] if img.ndim == 2 else img
    s = None
    for c in range(img.shape[2]):
        b = gaussian_filter(img[:, :, c], 31)
        gx, gy = sobel(b, axis=0, mode="nearest"), sobel(b, axis=1, mode="nearest")
        s = gx * gx + gy * gy if s is None else (s + gx * gx) + gy * gy
    v = np.sqrt(s)
    return (v - np.min(v)) / ((np.max(v) - np.min(v)) + v.dtype.type(1e-5))


@pytest.mark.parametrize("size", R.IMP_SIZES + R.IMP_EXTRA + [R.IMP_PAST_CAP])
def test_importance_map_restatement_equals_scipy(size):
    """Measured difference: 0 at every size (fp32 and fp64).  Asserted at the bar the GPU tests use; a degenerate size (floor above
    1e-4: the map is rounding noise) is held to bitwise equality instead, which is what was measured."""
    pytest.importorskip("scipy")
    img = R.imp_image(*size)
    got, floor = R.floor_of(img)
    want = _scipy_map(img)
    assert want.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: floor %.3e, bar %.3e, |restatement - scipy| %.3e" % (size, floor, R.bar_of(floor), err))
    assert err <= (0.0 if floor > R.DEGENERATE else R.bar_of(floor))
    err64 = float(np.abs(R.importance_map(img, round32=False) - _scipy_map(img.astype(np.float64))).max())
    assert err64 <= 1e-12, err64


# ---------------------------------------------------------------------------------------------------- floors
def test_only_the_two_tiny_frames_are_degenerate():
    for size in R.IMP_SIZES + R.IMP_EXTRA + [R.IMP_PAST_CAP]:
        m, floor = R.floor_of(R.imp_image(*size))
        print(size, "floor %.3e" % floor)
        if size == (1, 1, 1):
            assert floor == 0.0 and float(np.abs(m).max()) == 0.0
        else:
            assert (floor > R.DEGENERATE) == (size in R.IMP_DEGENERATE), (size, floor)
            assert float(m.min()) == 0.0 and float(m.max()) > (0.1 if size in R.IMP_DEGENERATE else 0.99)
    for name, (h, w, s, md, C, patch) in R.PROB_CASES.items():
        normal, bounce, gt = R.prob_inputs(h, w, s)
        p, floor = R.prob_floor_of(normal, bounce, gt[..., :3], patch)
        print(name, "floor %.3e of the maximum" % floor)
        assert floor <= R.DEGENERATE and p.shape == (h - patch, w - patch)
        for v in R.BOUNCE_EDGES:
            assert (bounce == np.float32(v)).sum() >= 2


def test_the_past_cap_probability_map_is_not_degenerate():
    h, w, s, md, C, patch = R.PROB_PAST_CAP
    assert (h - patch) * (w - patch) > 4096 * 256
    normal, bounce, gt = R.prob_inputs(h, w, s)
    floor = R.prob_floor_of(normal, bounce, gt[..., :3], patch)[1]
    print("past cap: floor %.3e of the maximum" % floor)
    assert floor <= R.DEGENERATE


# ---------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("mutant", ["drop_outer_pair", "mirror"])
def test_a_wrong_gaussian_falls_outside_the_bar(mutant):
    """At every non-degenerate size of the GPU tests.  'mirror' cannot differ where no filtered line is longer than the radius
    (both boundary rules agree there by construction of the mutant): (1, 40, 1) and (40, 1, 3) are left out for it."""
    caught = 0
    for size in LIVE:
        if mutant == "mirror" and max(size[:2]) <= R.RADIUS:
            continue
        img = R.imp_image(*size)
        m, floor = R.floor_of(img)
        gap = float(np.abs(R.importance_map(img, True, mutant).astype(np.float64) - m).max())
        print("%s %s: gap %.3e, bar %.3e" % (mutant, size, gap, R.bar_of(floor)))
        assert gap > R.bar_of(floor), (mutant, size)
        caught += 1
    assert caught >= 2


@pytest.mark.parametrize("mutant", ["drop_outer_pair", "mirror", "bounce_off", "crop_half"])
def test_a_wrong_probability_map_falls_outside_the_bar(mutant):
    """On the inputs of the GPU cases, unread channels NaN.  'mirror' cannot differ on the frames of 70 x 90 and 96 x 80 (no line
    longer than the radius), 'crop_half' on an even patch (patch / 2 == patch - patch / 2): those pairs are left out.  The crop
    mutant's map has one row and one column more; the common part is compared (it differs through the sum)."""
    caught = 0
    for name, (h, w, s, md, C, patch) in R.PROB_CASES.items():
        if (mutant == "crop_half" and patch % 2 == 0) or (mutant == "mirror" and max(h, w) <= R.RADIUS):
            continue
        normal, bounce, gt = R.prob_inputs(h, w, s)
        raw = np.full((h, w, s, C), np.nan, dtype=np.float32)
        raw[..., 17:20], raw[..., R.bounce_channel(md)] = normal, bounce
        if mutant == "bounce_off":
            assert R.bounce_channel(md, mutant) == R.bounce_channel(md) - 6
        p, floor = R.prob_floor_of(normal, bounce, gt[..., :3], patch)
        assert np.array_equal(p, R.sampling_prob(raw, gt, patch, md))
        with np.errstate(all="ignore"):
            q = R.sampling_prob(raw, gt, patch, md, True, mutant)[:h - patch, :w - patch].astype(np.float64)
        gap = np.abs(q - p) / float(p.max())
        gap = float(np.where(np.isnan(gap), np.inf, gap).max())            # (a NaN from an unread channel is caught)
        print("%s %s: gap %.3e of the maximum, bar %.3e" % (mutant, name, gap, R.bar_of(floor)))
        assert gap > R.bar_of(floor), (mutant, name)
        caught += 1
    # ('mirror' has one frame longer than the radius here; the importance-map test above catches it at six sizes)
    assert caught >= (1 if mutant == "mirror" else 2)


def test_sanitize_rule():
    big = np.float32(1e38)
    below = np.nextafter(big, np.float32(0))
    x = np.array([np.nan, np.inf, -np.inf, 1e38, 3e38, below, -3e38, 0.0, -1.5], dtype=np.float32)
    want = np.array([big, big, big, big, big, below, -3e38, 0.0, -1.5], dtype=np.float32)
    assert R.sanitize(x).tobytes() == want.tobytes()
    from wcmc_amd.support.datasets import sanitized
    assert sanitized(x).tobytes() == want.tobytes()


def test_sanitize_of_no_elements_is_no_error():
    """An empty tensor has a null data pointer: wcmc_sanitize(null, 0) is no work, not a bad argument (it was one; found by
    tests/test_gpu_sampling_edges.py::test_sanitize_past_the_flat_grid_cap_and_at_no_elements).  The argument check needs no GPU."""
    from wcmc_amd._lib import lib
    L = lib()
    assert L.wcmc_sanitize(None, 0, None) == 0
    assert L.wcmc_sanitize(None, 1, None) != 0 and b"null pointer" in L.wcmc_last_error()


# ---------------------------------------------------------------------------------------------------- data_ref.sbmc
@pytest.mark.parametrize("name", list(mgs.PRE))
def test_sbmc_reference_against_the_goldens(name):
    gold = np.load(os.path.join(GOLDEN, "sbmc_data.npz"))
    h, w, s, seed = mgs.PRE[name]
    x = mgs.sbmc_raw(h, w, s, seed)
    assert mgs.crc(x) == int(gold["pre/%s/raw_crc" % name])
    want_s, want_p, bound_s, bound_p = D.sbmc(x, 5)
    log_s, log_p = D.sbmc_split(5)
    for what, got, want, bound, log in (("sbmc_s", gold["pre/%s/sbmc_s" % name], want_s, bound_s, log_s),
                                        ("sbmc_p", gold["pre/%s/sbmc_p" % name], want_p, bound_p, log_p)):
        assert got.shape == want.shape and not bound[..., ~log].any() and (bound[..., log] > 0).all()
        assert np.array_equal(got[..., ~log].astype(np.float64), want[..., ~log]), what
        D.assert_within(got, want, bound, "%s %s (the reference's numpy in fp32)" % (name, what))


def test_sbmc_frame_plants_its_edges_and_a_wrong_offset_shows():
    for md, C in ((5, 104), (0, 49), (1, 60)):
        d = md + 1
        n = 3 * 128 + 5
        x = D.make_sbmc_frame(n, md, C, seed=3).numpy()
        assert x.shape == (n, 1, 1, C) and np.isnan(x[..., 24 + 7 * d:]).all() and np.isfinite(x[..., :24 + 7 * d]).all()
        recs = D.sbmc_edge_records(n)
        assert {0, 127, 128, n - 1} <= set(recs) and len(recs) >= 2 * len(D.SBMC_EDGES)
        want_s, want_p, bound_s, bound_p = D.sbmc(x, md)
        assert np.isfinite(want_s).all() and np.isfinite(want_p).all()
        f, ws, wp = x.reshape(n, C), want_s.reshape(n, 27), want_p.reshape(n, 11 * d)
        codes = f[recs, 24 + 6 * d:24 + 7 * d].astype(np.float64)
        for v in (5.9, -3.0, 32767.5, -32768.0, 1e38, -32768.5, 32768.5, -0.9, -5.5) if d > 1 else (5.9, 32767.5, -32768.0, 1e38):
            assert (codes == float(np.float32(v))).any(), v
        # total < diffuse: log 1 = 0; a non-positive probability: log(1e-5) / 30; directions at +-1 pass the clip unchanged
        assert (ws[0, 6:9] == 0).all() and f[0, 2] < f[0, 5]
        assert np.allclose(wp[[0, 1], :4 * d], np.log(float(np.float32(1e-5))) / 30.0, rtol=0, atol=0)
        assert set(np.abs(wp[recs[:3], 4 * d:6 * d]).reshape(-1)) == {1.0}
        # tags of record 0, bounce 0: int16(5.9) = 5 = 0b00101
        assert list(wp[0, 6 * d::d]) == [1, 0, 1, 0, 0]
        assert D.bounce_code([5.9, -3.0, -0.9, 32767.5, -32768.5, 32768.5, -32769.0, 1e38]).tolist() == [5, -3, 0, 32767, -32768, 0, 0, 0]
        # the wrong variant (every channel from the probabilities on one further up) is outside the bound, or NaN at C's minimum
        bad_s, bad_p, _, _ = D.sbmc(x, md, shift=1)
        with pytest.raises(AssertionError):
            D.assert_within(bad_p, want_p, bound_p, "shifted")
        assert np.array_equal(bad_s, want_s)
