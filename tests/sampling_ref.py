"""Plain numpy restatements of the patch-sampling maps (csrc/sampling_map.hip: wcmc_importance_map, wcmc_sampling_prob,
wcmc_sanitize) as include/wcmc_hip.h specifies them: the yardstick of tests/test_gpu_sampling_edges.py.
tests/test_cpu_sampling_ref.py holds them to the reference's goldens (tests/golden/sampling_map.npz) and to scipy's own
gaussian_filter + sobel pipeline, and shows that the wrong variants below fall outside the bar.

importance_map(img)
  1. the 249-tap Gaussian, sigma = 31, radius int(4 * 31 + 0.5) = 124: weights exp(-0.5 / sigma^2 * i^2), normalised in fp64;
     axis 0 first; boundary 'reflect' (d c b a | a b c d | d c b a: period 2n, any n >= 1 -- numpy.pad's 'symmetric'); fp64
     accumulation in scipy's order (the centre tap, then the pairs from the outermost inwards); the result is rounded to fp32
     between the passes;
  2. sobel along both axes with 'nearest': [-1 0 1] along the axis, [1 2 1] across it, each stage rounded to fp32;
  3. (s + gx^2) + gy^2 over the channels in fp32, the root;
  4. (v - min) / ((max - min) + 1e-5) in fp32 with numpy's NaN-propagating min / max.
``round32=False`` runs the same in fp64 without any intermediate rounding: the floor measure.  The FLOOR of a case is the largest
gap between the two; the bar of every comparison is max(4 x floor, 1e-6) (the rule of tests/test_gpu_dataset_dir.py).  A case
whose floor exceeds DEGENERATE = 1e-4 has a blurred image that is constant to rounding: its map is rounding noise over
(max - min + 1e-5) and only its structure can be checked.

sampling_prob(raw, gt, patch, max_depth)
  lum    = luminance (0.2126, 0.7152, 0.0722) of clip((gt[..., :3] / (1 + luminance(gt) / 1.5)) ** (1 / 2.2), 0, 1)
  normal = sample mean of raw channels 17..19, * 0.5 + 0.5
  mat    = (diffuse + 4 glossy + 2 specular) / 7: sample means of bits 2, 3, 4 of raw channel 24 + 6 (max_depth + 1), the float
           truncated toward zero where int16 holds it, no bits otherwise
  prob   = (0.3 importance_map(lum) + 0.2 importance_map(normal)) + 0.5 mat, cropped by patch // 2 at the top / left and by
           patch - patch // 2 at the bottom / right, divided by (float32(sum) + 1e-5).

MUTANTS (``mutant=`` makes the restatement wrong on purpose; the CPU self-check shows each falls outside the bar):
  "drop_outer_pair"  the Gaussian without its outermost tap pair (distance 124)
  "mirror"           boundary 'mirror' (d c b | a b c d | c b a: the edge not repeated) on lines longer than the radius
  "bounce_off"       the bounce channel one depth off: 24 + 6 max_depth
  "crop_half"        a crop of patch // 2 on both sides (one row and one column more for an odd patch; compared on the common part)
"""
import numpy as np

SIGMA, RADIUS = 31, 124
DEGENERATE = 1e-4
MUTANTS = ("drop_outer_pair", "mirror", "bounce_off", "crop_half")
F32 = np.float32


# ---------------------------------------------------------------------------------------------------- the cases of the GPU tests
# (H, W, C).  Tiles of the kernels: 128 outputs along the filtered axis x 32 lines across it (sm_gauss_kernel), 32 x 8 pixels
# (sobel, combine), 4096 blocks x 256 threads (the flat grids).
IMP_SIZES = [(1, 1, 1), (2, 3, 1), (1, 40, 1), (40, 1, 3), (127, 33, 1), (128, 32, 3), (129, 31, 1), (377, 130, 1), (130, 377, 3),
             (264, 256, 1)]
IMP_DEGENERATE = [(1, 1, 1), (2, 3, 1)]               # floor 0 (the map is exactly 0) / floor above DEGENERATE
# 380 = 128 + 252: block 1 of the Gaussian stages positions 4 .. 379 and reflects none (at 377 it still reflects three)
IMP_EXTRA = [(380, 33, 1), (33, 380, 3)]
IMP_PAST_CAP = (1032, 1024, 1)
# name: (H, W, S, max_depth, C, patch)
PROB_CASES = {"odd patch, one sample": (70, 90, 1, 0, 49, 33), "max_depth 3": (96, 80, 3, 3, 84, 32),
              "odd patch, wide records": (96, 80, 2, 5, 108, 31), "266 x 266 crop": (330, 330, 1, 0, 49, 64)}
PROB_PAST_CAP = (1100, 1090, 1, 0, 49, 64)
BOUNCE_EDGES = (1e38, -3.0, 5.9, 32767.5)


def _golden():
    import os
    import sys
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if p not in sys.path:
        sys.path.insert(0, p)
    import make_golden_dataset as mgd
    return mgd


def imp_image(h, w, c):
    """The block-structured test image of make_golden_dataset for a size of the lists above."""
    return _golden().test_image(h, w, c, 1000 + h + w)


def prob_inputs(h, w, s, seed=None):
    """(normal (h, w, s, 3), bounce (h, w, s), gt (h, w, 9)) fp32 on the host: block-structured normals in [-1, 1] with per-sample
    noise, bounce codes 0..31 with BOUNCE_EDGES at the four corners' first pixels and in the middle of the frame."""
    mgd = _golden()
    seed = 2000 + h + w + s if seed is None else seed
    rng = np.random.RandomState(seed)
    normal = (mgd.test_image(h, w, 3, seed + 1) * 2.0 - 1.0)[:, :, None, :] + rng.randint(-32, 33, size=(h, w, s, 3)) / 256.0
    bounce = rng.randint(0, 32, size=(h, w, s)).astype(F32)
    for k, v in enumerate(BOUNCE_EDGES):
        bounce[h // 2, w // 2 + k, 0] = v
        bounce[(0, 0, h - 1, h - 1)[k], (0, w - 1, 0, w - 1)[k], s - 1] = v
    return normal.astype(F32), bounce, mgd.test_gt(h, w, seed + 2)


def weights():
    """w[d], d = 0..124: the normalised tap at distance d, in fp64."""
    i = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (SIGMA * SIGMA) * i ** 2)
    phi = phi / phi.sum()
    return phi[RADIUS:]


def _gauss_axis(x, axis, mutant=None):
    """One pass over fp64 planes (..., H, W) -> fp64, accumulated in scipy's order."""
    w = weights()
    n = x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (RADIUS, RADIUS)
    p = np.pad(x, pad, mode="reflect" if (mutant == "mirror" and n > RADIUS) else "symmetric")

    def at(off):
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(RADIUS + off, RADIUS + off + n)
        return p[tuple(sl)]

    acc = at(0) * w[0]
    for d in range(RADIUS - 1 if mutant == "drop_outer_pair" else RADIUS, 0, -1):
        acc += (at(-d) + at(d)) * w[d]
    return acc


def _near(x, axis, off):
    """x shifted by ``off`` along ``axis`` with the edge repeated ('nearest')."""
    n = x.shape[axis]
    return np.take(x, np.clip(np.arange(n) + off, 0, n - 1), axis=axis)


def _sobel(x, axis, rnd):
    """[-1 0 1] along ``axis``, [1 2 1] across the other of the last two axes; fp64 arithmetic, ``rnd`` after each stage."""
    other = x.ndim - 1 if axis == x.ndim - 2 else x.ndim - 2
    d = rnd(_near(x, axis, 1) - _near(x, axis, -1))
    return rnd(d * 2.0 + (_near(d, other, -1) + _near(d, other, 1)))


def _normalise(v, ft):
    mn, mx = np.min(v), np.max(v)                     # (NaN-propagating)
    return (v - mn) / ((mx - mn) + ft(1e-5))


def importance_map(img, round32=True, mutant=None):
    """(H, W), (H, W, 1) or (H, W, 3) -> (H, W): fp32 with ``round32``, else fp64."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    assert img.ndim == 3 and img.shape[2] in (1, 3), img.shape
    ft = F32 if round32 else np.float64
    rnd = (lambda a: a.astype(F32).astype(np.float64)) if round32 else (lambda a: a)
    with np.errstate(all="ignore"):
        x = np.ascontiguousarray(np.moveaxis(img, 2, 0)).astype(np.float64)          # planar (C, H, W)
        x = rnd(_gauss_axis(x, 1, mutant))
        x = rnd(_gauss_axis(x, 2, mutant))
        gx, gy = _sobel(x, 1, rnd).astype(ft), _sobel(x, 2, rnd).astype(ft)
        s = gx[0] * gx[0] + gy[0] * gy[0]
        for c in range(1, x.shape[0]):
            s = (s + gx[c] * gx[c]) + gy[c] * gy[c]
        return _normalise(np.sqrt(s), ft)


def floor_of(img):
    """(map with fp32 roundings, its floor): the largest gap to the same computation in fp64."""
    m32 = importance_map(img, True)
    return m32, float(np.abs(m32.astype(np.float64) - importance_map(img, False)).max())


def bar_of(floor):
    return max(4.0 * floor, 1e-6)


def bounce_channel(max_depth, mutant=None):
    return 24 + 6 * (max_depth if mutant == "bounce_off" else max_depth + 1)


def material_bits(code):
    """The bounce code as astype(int16) gives it where int16 holds the truncated value; 0 (no bits) otherwise."""
    t = np.trunc(np.asarray(code, dtype=np.float64))
    ok = (t >= -32768) & (t <= 32767)
    return np.where(ok, t, 0.0).astype(np.int64)


def planes(normal, bounce, gt3, round32=True):
    """normal (H, W, S, 3), bounce (H, W, S), gt3 (H, W, 3) -> lum (H, W), normal (H, W, 3), mat (H, W)."""
    ft = F32 if round32 else np.float64
    g = np.asarray(gt3).astype(ft)
    lw = [ft(0.2126), ft(0.7152), ft(0.0722)]
    with np.errstate(all="ignore"):
        lum_in = (lw[0] * g[..., 0] + lw[1] * g[..., 1]) + lw[2] * g[..., 2]
        den = ft(1.0) + lum_in / ft(1.5)
        t = np.clip(np.power(g / den[..., None], ft(1.0 / 2.2)), ft(0.0), ft(1.0))
        lum = (lw[0] * t[..., 0] + lw[1] * t[..., 1]) + lw[2] * t[..., 2]
        nrm = np.asarray(normal).astype(ft)
        S = nrm.shape[2]
        acc = np.zeros(nrm.shape[:2] + (3,), dtype=ft)
        for s in range(S):
            acc = acc + nrm[:, :, s]
        nmean = (acc / ft(S)) * ft(0.5) + ft(0.5)
        bits = material_bits(bounce)
        dif, glo, spe = (((bits >> k) & 1).sum(2).astype(ft) / ft(S) for k in (2, 3, 4))
        mat = ((dif + glo * ft(4.0)) + spe * ft(2.0)) / ft(7.0)
    return lum, nmean, mat


def sampling_prob_planes(normal, bounce, gt3, patch, round32=True, mutant=None):
    """The map from the four raw channels it reads (normal (H, W, S, 3), bounce (H, W, S)) and gt[..., :3]."""
    ft = F32 if round32 else np.float64
    lum, nmean, mat = planes(normal, bounce, gt3, round32)
    H, W = lum.shape
    assert patch >= 1 and H > patch and W > patch
    gm = mutant if mutant in ("drop_outer_pair", "mirror") else None
    d_lum, d_norm = importance_map(lum, round32, gm), importance_map(nmean, round32, gm)
    with np.errstate(all="ignore"):
        prob = (ft(0.3) * d_lum + ft(0.2) * d_norm) + ft(0.5) * mat
        top = patch // 2
        bottom = top if mutant == "crop_half" else patch - top
        prob = prob[top:H - bottom, top:W - bottom]
        total = prob.astype(np.float64).sum()
        if round32:
            total = F32(total)                         # numpy.sum of fp32 returns fp32
        return prob / (total + ft(1e-5))


def sampling_prob(raw, gt, patch, max_depth, round32=True, mutant=None):
    """raw (H, W, S, C >= 38 + 11 (max_depth + 1)), gt (H, W, >= 3) -> (H - patch, W - patch)."""
    raw, gt = np.asarray(raw), np.asarray(gt)
    assert raw.ndim == 4 and raw.shape[3] >= 38 + 11 * (max_depth + 1)
    return sampling_prob_planes(raw[..., 17:20], raw[..., bounce_channel(max_depth, mutant)], gt[..., :3], patch, round32, mutant)


def prob_floor_of(normal, bounce, gt3, patch):
    """(map with fp32 roundings, its floor relative to the fp64 map's maximum)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(2) as pool:                # (numpy releases the interpreter lock: the two forms run side by side)
        f32 = pool.submit(sampling_prob_planes, normal, bounce, gt3, patch, True)
        p64 = sampling_prob_planes(normal, bounce, gt3, patch, False)
        p32 = f32.result()
    return p32, float(np.abs(p32.astype(np.float64) - p64).max() / p64.max())


def sanitize(x):
    """NaN, +-Inf and everything >= 1e38 become float32(1e38)."""
    x = np.asarray(x, dtype=F32)
    big = F32(1.0e+38)
    with np.errstate(all="ignore"):
        x = np.where(np.isfinite(x), x, big)
        return np.where(x < big, x, big).astype(F32)
