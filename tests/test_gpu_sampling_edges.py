"""The sampling-map kernels (csrc/sampling_map.hip: wcmc_importance_map, wcmc_sampling_prob, wcmc_sanitize) against the numpy
restatement of tests/sampling_ref.py, at the edges of their tiles, past the flat-grid cap, with more than 256 partials in the
one-block finishes, on NaN / Inf input and on every input form of sampling_prob.

Bars.  Every map is compared in EVERY element with the restatement in its fp32 form (``round32=True``).  The bar of a case is
max(4 x floor, 1e-6) -- the rule of tests/test_gpu_dataset_dir.py --, where the floor is the restatement's own rounding error on
that input: the largest gap between its fp32 form and the same computation in fp64 without intermediate rounding.  It is never
taken from the kernel.  For the probability map both the floor and the error are relative to the map's maximum, and the fp64 sum
of the result is within 4 eps32 of the restatement's.  A case whose floor exceeds 1e-4 is degenerate (the blurred image is constant
to rounding, the map is rounding noise over max - min + 1e-5): (2, 3, 1) only; it gets structural assertions.  (1, 1, 1) is exactly
0.  tests/test_cpu_sampling_ref.py shows that the restatement is scipy's pipeline bit for bit at these sizes, that no other case is
degenerate, and that a Gaussian without its outermost tap pair, a 'mirror' boundary, a bounce channel one depth off and a crop of
patch / 2 on both sides fall outside these bars.  sanitize_ is compared bit for bit.

What the sizes cross (restated from the kernels and asserted below):
  sm_gauss_kernel      128 outputs along the filtered axis x 32 lines: 127 / 128 / 129 and 33 / 32 / 31; n = 1 along either axis
                       (every tap reflects onto the one entry; the Sobel clamps meet); 377 = 128 + 2 x 124 + 1 along either axis,
                       and 380 = 128 + 252: block 1 stages positions 4 .. 379 and reflects none
  one-block finishes   264 x 256 has 264 min / max tiles of 32 x 8, a 266 x 266 crop 306 sum tiles: more than 256 threads
  flat grids           4096 x 256 = 1,048,576: 1032 x 1024 pixels (normalise), a 1036 x 1026 crop (divide), 1,048,833 floats (sanitize)

Measured on one MI355X (profiles/sampling_sbmc_edges_error.txt), largest error per case:
  importance_map   0 at all thirteen sizes, the past-cap one included (bars 2.1e-5 .. 2.3e-4; floors 5.2e-6 .. 5.8e-5); (2, 3, 1),
                   floor 1.0e-2, is bit-equal to the restatement too
  sampling_prob    (70, 90, 1, 0, 49, 33): 3.9e-6 of the maximum (bar 1.9e-5)     (96, 80, 3, 3, 84, 32): 8.4e-6 (3.8e-5)
                   (96, 80, 2, 5, 108, 31): 1.2e-5 (5.0e-5)     (330, 330, 1, 0, 49, 64): 7.8e-6 (3.2e-5)
                   (1100, 1090, 1, 0, 49, 64): 8.0e-6 (3.0e-5); |sum - restatement's sum| <= 2.5e-8 (powf of the tone map against
                   numpy's in the last place, amplified by the Sobel differences of the blurred luminance)
  sanitize_        bit-equal; n = 0 raised "null pointer" before this file (an empty tensor has none): fixed in wcmc_sanitize
"""
import functools
import os

import numpy as np
import pytest
import torch

import sampling_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("WCMC_TEST_REPORTS", os.path.join(ROOT, "test_reports"))     # (git-ignored)
DEV = "cuda:0"
FLAT_CAP = 4096 * 256                                   # sm_flat_grid: blocks x threads
ROWS = []                                               # (case, floor, bar, error) of this run


def _ops():
    from wcmc_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _tiles(h, w):
    return ((w + 31) // 32) * ((h + 7) // 8)


@functools.lru_cache(maxsize=None)
def _imp_ref(size):
    img = R.imp_image(*size)
    want, floor = R.floor_of(img)
    return img, want, floor


def _structure(got, h, w):
    assert got.shape == (h, w) and got.dtype == torch.float32
    g = got.cpu().numpy()
    assert np.isfinite(g).all() and float(g.min()) >= 0.0 and float(g.max()) <= 1.0
    return g


def _hold_map(size):
    ops = _ops()
    h, w, c = size
    img, want, floor = _imp_ref(size)
    x = _dev(img)
    got = ops.importance_map(x)
    g = _structure(got, h, w)
    assert _same_bits(got, ops.importance_map(x)), "two calls must agree bitwise"
    if c == 1:                                              # (H, W) and (H, W, 1) are the same image
        assert _same_bits(got, ops.importance_map(x.view(h, w, 1)))
    bar = R.bar_of(floor)
    err = float(np.abs(g.astype(np.float64) - want).max())
    print("importance_map %s: floor %.3e bar %.3e error %.3e" % (size, floor, bar, err))
    if floor > R.DEGENERATE:
        assert size in R.IMP_DEGENERATE
        ROWS.append(("importance_map %s" % (size,), floor, None, err))
        return
    ROWS.append(("importance_map %s" % (size,), floor, bar, err))
    assert err <= bar, (size, err, bar)
    assert float(g.min()) == 0.0


# ---------------------------------------------------------------------------------------------------- importance_map
@pytest.mark.parametrize("size", R.IMP_SIZES + R.IMP_EXTRA)
def test_importance_map_at_the_tile_edges(size):
    h, w, c = size
    if size == (1, 1, 1):
        got = _ops().importance_map(_dev(R.imp_image(1, 1, 1)))
        assert got.shape == (1, 1) and float(got[0, 0]) == 0.0 and not bool(torch.signbit(got).any())
    if size == (264, 256, 1):
        assert _tiles(h, w) == 264 > 256                    # sm_minmax_finish_kernel: a second iteration of its 256 threads
    if size in R.IMP_EXTRA:
        n = max(h, w)                                       # block 1 stages [128 - 124, 128 + 127 + 124] = [4, 379]
        assert 128 - R.RADIUS >= 0 and 128 + 127 + R.RADIUS <= n - 1 and 128 + 127 + R.RADIUS > 377 - 1
    _hold_map(size)


def test_importance_map_past_the_flat_grid_cap():
    h, w, c = R.IMP_PAST_CAP
    assert h * w == 1056768 > FLAT_CAP == 1048576 and _tiles(h, w) > 256
    _hold_map(R.IMP_PAST_CAP)


@pytest.mark.parametrize("value", ["nan", "inf"])
@pytest.mark.parametrize("c", [1, 3])
def test_importance_map_keeps_numpys_nan(value, c):
    """One NaN pixel (in the middle channel of the rgb image): numpy's min / max return NaN and every pixel of the map is NaN.
    One +Inf pixel: the blur is +Inf within the radius -- the whole 150 x 140 image --, its differences are NaN."""
    ops = _ops()
    img = R.imp_image(150, 140, c).copy()
    img[(77, 31) if c == 1 else (77, 31, 1)] = {"nan": np.nan, "inf": np.inf}[value]
    want = R.importance_map(img)
    assert np.isnan(want).all()
    got = ops.importance_map(_dev(img))
    assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want))
    assert bool(torch.isnan(ops.importance_map(_dev(img))).all())
    if value == "nan":                                      # off-centre in a larger image: pixels beyond the radius are still NaN
        big = R.imp_image(264, 256, 1).copy()
        big[3, 250] = np.nan
        assert bool(torch.isnan(ops.importance_map(_dev(big))).all())


# ---------------------------------------------------------------------------------------------------- sampling_prob
def _raw_on_device(normal, bounce, md, C):
    """(H, W, S, C) on the device: NaN everywhere but the normal triple 17..19 and the bounce-0 type 24 + 6 (max_depth + 1)."""
    h, w, s = bounce.shape
    x = torch.full((h, w, s, C), float("nan"), device=DEV, dtype=torch.float32)
    x[..., 17:20] = _dev(normal)
    x[..., R.bounce_channel(md)] = _dev(bounce)
    return x


def _hold_prob(name, case):
    ops = _ops()
    h, w, s, md, C, patch = case
    assert C >= 38 + 11 * (md + 1)
    normal, bounce, gt = R.prob_inputs(h, w, s)
    gt = gt.copy()
    gt[..., 3:] = np.nan                                    # (only the radiance is read)
    raw, d_gt = _raw_on_device(normal, bounce, md, C), _dev(gt)
    got = ops.sampling_prob(raw, d_gt, patch, md)
    again = ops.sampling_prob(raw, d_gt, patch, md)
    # the reference sees the four channels as they lie on the device
    ch = [17, 18, 19, R.bounce_channel(md)]
    back = raw[..., ch].cpu().numpy()
    del raw
    assert np.array_equal(back[..., :3], normal) and np.array_equal(back[..., 3], bounce)
    want, floor = R.prob_floor_of(back[..., :3], back[..., 3], gt[..., :3], patch)
    bar = R.bar_of(floor)
    assert floor <= R.DEGENERATE
    assert got.shape == (h - patch, w - patch) == want.shape and got.dtype == torch.float32
    assert _same_bits(got, again), "two calls must agree bitwise"
    g = got.cpu().numpy().astype(np.float64)
    assert not np.isnan(g).any(), "a NaN: a channel the function must not read"
    err = float(np.abs(g - want).max() / want.max())
    print("sampling_prob %s %s: floor %.3e bar %.3e error %.3e (of the map's maximum)" % (name, case, floor, bar, err))
    ROWS.append(("sampling_prob %s" % (case,), floor, bar, err))
    assert err <= bar, (name, err, bar)
    assert float(g.min()) >= 0.0
    ds = abs(float(g.sum()) - float(want.astype(np.float64).sum()))
    print("    |sum - restatement's sum| = %.3e" % ds)
    assert ds <= 4 * np.finfo(np.float32).eps


@pytest.mark.parametrize("name", list(R.PROB_CASES))
def test_sampling_prob_every_input_form(name):
    h, w, s, md, C, patch = R.PROB_CASES[name]
    if name == "266 x 266 crop":
        assert _tiles(h - patch, w - patch) == 306 > 256    # sm_sum_finish_kernel: a second iteration of its 256 threads
    _hold_prob(name, R.PROB_CASES[name])


def test_sampling_prob_past_the_flat_grid_cap():
    h, w, s, md, C, patch = R.PROB_PAST_CAP
    assert (h - patch) * (w - patch) == 1062936 > FLAT_CAP  # sm_divide_kernel takes a second trip
    torch.cuda.empty_cache()
    _hold_prob("past the cap", R.PROB_PAST_CAP)
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- sanitize_
def test_sanitize_past_the_flat_grid_cap_and_at_no_elements():
    ops = _ops()
    n = FLAT_CAP + 257
    big = np.float32(1e38)
    edges = np.array([np.nan, np.inf, -np.inf, 1e38, 3e38, np.nextafter(big, np.float32(0)), -3e38, -0.0], dtype=np.float32)
    x = np.random.RandomState(6).randn(n).astype(np.float32)
    for start in (0, 1000, FLAT_CAP - len(edges), FLAT_CAP, FLAT_CAP + 1, n - len(edges)):      # both trips, and across the seam
        x[start:start + len(edges)] = edges
    want = R.sanitize(x)
    assert want[FLAT_CAP + 6] == np.nextafter(big, np.float32(0)) and want[n - len(edges)] == big and np.isfinite(want).all()
    for rep in range(2):
        t = _dev(x)
        assert ops.sanitize_(t) is t
        assert t.cpu().numpy().tobytes() == want.tobytes()
    ops.sanitize_(t)                                        # idempotent
    assert t.cpu().numpy().tobytes() == want.tobytes()
    empty = torch.empty(0, device=DEV)
    assert ops.sanitize_(empty) is empty
    for v in edges:
        one = _dev(np.array([v]))
        assert ops.sanitize_(one).cpu().numpy().tobytes() == R.sanitize(np.array([v], dtype=np.float32)).tobytes()
    guard = _dev(np.array([np.nan, np.nan, np.nan]))
    ops.sanitize_(guard[1:2])                               # n = 1 touches one element
    assert bool(torch.isnan(guard[0])) and bool(torch.isnan(guard[2])) and float(guard[1]) == float(big)


# ---------------------------------------------------------------------------------------------------- the table
def format_rows():
    lines = ["%-52s%12s%12s%12s" % ("case", "floor", "bar", "error")]
    for what, floor, bar, err in ROWS:
        lines.append("%-52s%12.3e%12s%12.3e" % (what, floor, "structure" if bar is None else "%.3e" % bar, err))
    return "\n".join(lines) + "\n"


def test_error_table_of_this_run():
    """Printed, and written to the report directory, for whatever part of this file has run before."""
    text = format_rows()
    print(text)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "sampling_edges_error.txt"), "w") as f:
        f.write(text)
    assert all(bar is None or err <= bar for _, _, bar, err in ROWS)
