"""Plain fp64 restatements of the per-image preprocessing (csrc/preprocess.hip, csrc/data_step.h, the statistics pass of
csrc/multi_spp.hip) with a per-element error bound for an fp32 evaluation in ANY summation order: the yardstick of
tests/test_gpu_data_edges.py.  tests/test_cpu_data_ref.py holds the values to oracle/datasets.py, the bounds to fp32 emulations of
the three summation orders in play, and shows that wrong variants of the functions fall outside them.

Written from the specification (oracle/datasets.py; DESIGN.md sections 11 and 14), for any ``max_depth`` and any
C >= 38 + 11 (max_depth + 1).  Raw channel map, d = max_depth + 1:
    radiance 2..4, diffuse 5..7, bounce types 24+6d (d), albedo 24+7d (3), normal 27+7d (3), depth 30+7d, path weight 31+7d,
    radiance without weight 32+7d (3), light intensity 35+7d (3), throughputs 38+7d (3d), roughnesses 38+10d (d).

Conventions (those of tests/glue_ref.py)
  U = 2^-24: one correctly rounded fp32 operation has relative error <= U of its result; ETA = 2^-149 is added once per channel
  for results in the subnormal range, where the error is absolute.  "k ulps of x" is bounded by 2 k U |x|.  Every KPCN bound is
  first order in U and multiplied by SAFETY = 2 at the end (second-order terms; the spread between summation orders).
  fp32 division and square root are correctly rounded (1 ulp is granted); logf is granted LOG_ULPS = 4 ulps: the device
  library documents 1, numpy's vector loop 3.83.

KPCN, per pixel over its s samples
  per-sample values      v = normal, depth, albedo, max(diffuse, 0): exact.  max(max(radiance, 0) - max(diffuse, 0), 0): one
                         rounded subtraction, |dv_k| <= U |v_k|  (r = 1 below, else r = 0).
  mean                   s - 1 adds whose partial sums are bounded by sum |v|, and the division:
                             em = (s + r) U mean|v|.                         With SAFETY that is the 2 s U mean|v| of the issue.
  population variance    two passes, the form of glue_ref.pvar_and_bound: with mh = mean + e, |e| <= em, in exact arithmetic
                         mean (v - mh)^2 = var + e^2 (the deviations sum to zero): the mean's error enters as the ABSOLUTE part
                         em^2.  d_k = fl(v_k - mh) U, its square 2 U + U, the sum <= (s - 1) U, the division U:
                             ev = (s + 3) U (var + em^2) + em^2 + r 2 U mean(|d| |v|).
                         A pixel whose samples are all equal has var = 0 and is held to (s + 4) U em^2: tiny, not zero.
  group variance         gv = ((var_0 + var_1 + var_2) / 3) / s: two adds, two divisions on non-negative terms:
                             egv = (ev_0 + ev_1 + ev_2) / (3 s) + 4 U gv.
  albedo + eps           a = A + eps (eps = fl32(0.00316)):  ea' = ea + U |a|.
  diffuse / a            e = ed / |a| + |D| ea' / a^2 + U |D / a|.
  albedo_sqr             Q = (a_0^2 + a_1^2 + a_2^2) / 3: each square 2 |a| ea' + U a^2, two adds and a division 3 U Q:
                             eQ = sum_c (2 |a_c| ea'_c + U a_c^2) / 3 + 3 U Q.       The same for specular_sqr with a = 1 + S.
  variance / Q           e = egv / Q + gv eQ / Q^2 + U gv / Q.
  log(1 + S)             t = 1 + S, et = eS + U t;  e = et / t + 2 LOG_ULPS U |log t|  (the first term covers t near 1, where the
                         absolute error U of the addition is all of the result's error).
  depth maximum          M = max(max_p mean depth_p, 0).  max is 1-Lipschitz in the sup norm: eM = max_p em_p.  It enters EVERY
                         depth channel of EVERY pixel.
  depth / M  (M > 0)     e = em / M + |D| eM / M^2 + U |D / M|;  the clip to [0, 1] is 1-Lipschitz and adds nothing.
  depth_v / (M^2 s)      two multiplications and the division: e = ev / (M^2 s) + 2 V eM / (M^3 s) + 3 U V / (M^2 s).
  backward differences   out[p] - out[p - 1] of the fp32 channel values: e = e_p + e_{p-1} + U |difference|; first column / row 0.

fp32 overflow semantics (section "the overflowing depth mean" of the GPU tests).  The reference forms every quantity that can leave
the fp32 range IN fp32 range: the per-pixel SUM of the samples (so the mean is Inf where fp32 overflows, whatever the order, for
samples of one sign), each squared deviation and their sum, M^2 and M^2 s are replaced by +-Inf where they exceed FLT_MAX.  From
there numpy's IEEE arithmetic gives what fp32 gives: Inf / Inf = NaN, finite / Inf = 0, and the clip keeps a NaN as np.clip does.
Where the reference is NaN only the NaN pattern is compared; where M = Inf every finite output is an exact 0 and its bound is 0.

LLPM, per sample and channel:  log(x + c) / k:  U / k for the addition (relative U of the argument is absolute U of the logarithm),
LOG_ULPS of the logarithm and 1 ulp of the division relative to the result;  bounce / 19: 1 ulp;  sqrt(roughness): 1 ulp.  No SAFETY:
these are ulp counts, not first-order sums.

``gradients`` is one fp32 subtraction of fp32 values: restated in fp32, compared bit for bit.

SBMC (csrc/sbmc_data.hip: wcmc_preprocess_sbmc; the yardstick of tests/test_gpu_sbmc_edges.py), per sample and channel: ``sbmc``
below -- bound 0 on every copied, clamped or bit-derived channel, the LLPM rule on the three log groups (its docstring); raw channel
map: subpixel 0:2, radiance 2:5, diffuse 5:8, g-buffer 8:24, probabilities 24 (4d), light directions 24+4d (2d), bounce types 24+6d (d).
"""
import numpy as np
import torch

from glue_ref import SAFETY, U

ETA = 2.0 ** -149
FLT_MAX = float(np.finfo(np.float32).max)
EPS = float(np.float32(0.00316))
LOG_ULPS = 4
ULP = 2.0 * U
KP_GROUPS = ("diffuse", "specular", "normal", "depth", "albedo")
KP_START = {"diffuse": 0, "specular": 10, "normal": 20, "depth": 30, "albedo": 34}


def min_channels(max_depth):
    return 38 + 11 * (max_depth + 1)


def cmap(max_depth=5, shift=0):
    """First raw channel of every group (shift = 1 is the WRONG variant: every offset off by one)."""
    d = max_depth + 1
    m = {"radiance": 2, "diffuse": 5, "bounce": 24 + 6 * d, "albedo": 24 + 7 * d, "normal": 27 + 7 * d, "depth": 30 + 7 * d,
         "pweight": 31 + 7 * d, "rwow": 32 + 7 * d, "light": 35 + 7 * d, "thr": 38 + 7 * d, "rough": 38 + 10 * d}
    return {k: v + shift for k, v in m.items()}


def kpcn_channels(max_depth=5, shift=0):
    """The thirteen raw channels _preprocess_kpcn reads, in the order radiance(3) diffuse(3) albedo(3) normal(3) depth(1)."""
    m = cmap(max_depth, shift)
    return [m[k] + c for k in ("radiance", "diffuse", "albedo", "normal") for c in range(3)] + [m["depth"]]


def _ovf(x):
    """fp32 range: what exceeds FLT_MAX is +-Inf."""
    return np.where(np.abs(x) > FLT_MAX, np.copysign(np.inf, x), x)


def _sum(x, axis):
    """Sum over a SHORT axis as a loop of whole-array adds (numpy's reduction over a short inner axis is several times slower)."""
    x = np.moveaxis(x, axis, 0)
    acc = x[0].copy()
    for k in range(1, x.shape[0]):
        acc += x[k]
    return acc


def _stats(v, r):
    """v (n, s, c) fp64 -> mean, em, var, ev over axis 1 (module docstring); r = 1 where v carries one rounded operation."""
    s = v.shape[1]
    av = np.abs(v)
    mean = _ovf(_sum(v, 1)) / s
    em = (s + r) * U * _sum(av, 1) / s
    d = v - mean[:, None]
    var = _ovf(_sum(_ovf(d * d), 1)) / s
    ev = (s + 3) * U * (var + em * em) + em * em + (r * 2 * U * _sum(np.abs(d) * av, 1) / s if r else 0.0)
    return mean, em, var, ev


def _sqr(a, ea):
    """Q = mean_c a_c^2 of (n, 3) and its bound; ea already holds the rounding of a itself."""
    q = _sum(a * a, 1)[:, None] / 3
    return q, _sum(2 * np.abs(a) * ea + U * a * a, 1)[:, None] / 3 + 3 * U * q


def _diff(val, err, forward=False):
    """(h, w, c) -> (h, w, 2c) backward differences with their bound (forward=True: the WRONG variant)."""
    dx, dy, ex, ey = (np.zeros_like(val) for _ in range(4))
    if forward:
        dx[:, :-1], dy[:-1] = val[:, 1:] - val[:, :-1], val[1:] - val[:-1]
    else:
        dx[:, 1:], dy[1:] = val[:, 1:] - val[:, :-1], val[1:] - val[:-1]
    ex[:, 1:], ey[1:] = err[:, 1:] + err[:, :-1], err[1:] + err[:-1]
    return np.concatenate([dx, dy], 2), np.concatenate([ex + U * np.abs(dx), ey + U * np.abs(dy)], 2)


def kpcn13(x13, wrong=None, max_pixels=None, chunk=1 << 16):
    """(h, w, s, 13) fp32 values of ``kpcn_channels`` -> (fp64 (h, w, 44), bound (h, w, 44)).

    WRONG variants: "ddof" (variance / (s - 1)), "no_spp" (the normal variance channel without / spp), "unclamped" (specular =
    max(radiance - diffuse, 0)), "forward" (forward differences), "clip_nan" (fminf(fmaxf()): the clip turns NaN into 0);
    max_pixels = n: the depth maximum over the first n pixels only (the pixels behind a grid cap dropped)."""
    h, w, s = x13.shape[:3]
    n = h * w
    flat = x13.reshape(n, s, 13)
    names = ("normal", "depth", "albedo", "diffuse", "specular")
    width = {"normal": 3, "depth": 1, "albedo": 3, "diffuse": 3, "specular": 3}
    acc = {k: [np.empty((n, width[k])) for _ in range(4)] for k in names}
    with np.errstate(all="ignore"):
        for p0 in range(0, n, chunk):                       # the statistics in pixel chunks: bounded temporaries at 2 M pixels
            x = flat[p0:p0 + chunk].astype(np.float64)
            rad, dif = x[..., 0:3], x[..., 3:6]
            spec = np.maximum(rad - dif, 0) if wrong == "unclamped" else np.maximum(np.maximum(rad, 0) - np.maximum(dif, 0), 0)
            vals = {"normal": (x[..., 9:12], 0), "depth": (x[..., 12:13], 0), "albedo": (x[..., 6:9], 0),
                    "diffuse": (np.maximum(dif, 0), 0), "specular": (spec, 1)}
            for k, (v, r) in vals.items():
                for dst, src in zip(acc[k], _stats(v, r)):
                    dst[p0:p0 + chunk] = src
        if wrong == "ddof":
            for k in names:
                acc[k][2] *= s / (s - 1.0)
        out, err = {}, {}

        def group_var(k, div=float(s)):
            var, ev = acc[k][2], acc[k][3]
            gv = _sum(var, 1)[:, None] / 3 / div
            return gv, _sum(ev, 1)[:, None] / (3 * div) + 4 * U * gv

        # normal
        gv, egv = group_var("normal", 1.0 if wrong == "no_spp" else float(s))
        out["normal"], err["normal"] = (acc["normal"][0], gv), (acc["normal"][1], egv)
        # albedo, and diffuse over it
        A, eA = acc["albedo"][0], acc["albedo"][1]
        gv, egv = group_var("albedo")
        out["albedo"], err["albedo"] = (A, gv), (eA, egv)
        a = A + EPS
        ea = eA + U * np.abs(a)
        Q, eQ = _sqr(a, ea)
        D, eD = acc["diffuse"][0], acc["diffuse"][1]
        gv, egv = group_var("diffuse")
        out["diffuse"] = (D / a, gv / Q)
        err["diffuse"] = (eD / np.abs(a) + np.abs(D) * ea / (a * a) + U * np.abs(D / a), egv / Q + gv * eQ / (Q * Q) + U * gv / Q)
        # specular
        S, eS = acc["specular"][0], acc["specular"][1]
        t = 1 + S
        et = eS + U * np.abs(t)
        Q, eQ = _sqr(t, et)
        gv, egv = group_var("specular")
        lg = np.log(t)
        out["specular"] = (lg, gv / Q)
        err["specular"] = (et / np.abs(t) + LOG_ULPS * ULP * np.abs(lg), egv / Q + gv * eQ / (Q * Q) + U * gv / Q)
        # depth
        Dm, em, V, ev = acc["depth"]
        lim = n if max_pixels is None else max_pixels
        M = max(float(Dm[:lim].max()), 0.0)
        eM = float(em[:lim].max())
        if M > 0:
            M2s = _ovf(_ovf(M * M) * s)
            dep, edep = Dm / M, em / M + np.abs(Dm) * eM / (M * M) + U * np.abs(Dm / M)
            dv, edv = V / M2s, ev / M2s + 2 * V * eM / (M ** 3 * s) + 3 * U * V / M2s
        else:
            dep, edep, dv, edv = Dm, em, V, ev
        nan = np.isnan(dep)
        dep = np.clip(dep, 0, 1)
        if wrong == "clip_nan":
            dep = np.where(nan, 0.0, dep)
        out["depth"], err["depth"] = (dep, dv), (edep, edv)
        want, bound = np.empty((h, w, 44)), np.empty((h, w, 44))
        for k in KP_GROUPS:
            c0, nv = KP_START[k], width[k]
            val, var = (t_.reshape(h, w, -1) for t_ in out[k])
            eval_, evar = (t_.reshape(h, w, -1) for t_ in err[k])
            g, eg = _diff(val, eval_, forward=wrong == "forward")
            want[..., c0:c0 + nv], want[..., c0 + nv:c0 + nv + 1], want[..., c0 + nv + 1:c0 + 3 * nv + 1] = val, var, g
            bound[..., c0:c0 + nv], bound[..., c0 + nv:c0 + nv + 1], bound[..., c0 + nv + 1:c0 + 3 * nv + 1] = eval_, evar, eg
        bound = SAFETY * bound + ETA
        if np.isinf(M):     # every finite depth output is finite / Inf = 0 exactly; the rest of those channels is NaN
            bound[~np.isfinite(bound)] = 0.0
        assert np.isfinite(bound[np.isfinite(want)]).all()
    return want, bound


def kpcn(raw, max_depth=5, wrong=None, shift=0, **kw):
    """raw (h, w, s, C) fp32 -> (fp64 (h, w, 44), bound); shift = 1: the WRONG variant with every channel offset off by one."""
    assert raw.shape[3] >= min_channels(max_depth)
    return kpcn13(np.asarray(raw)[..., kpcn_channels(max_depth, shift)], wrong=wrong, **kw)


def llpm_tail(x, max_depth=5, first=None, shift=0):
    """x (..., C - first) fp32: the raw channels from ``first`` (default: the bounce types, the lowest channel _preprocess_llpm
    reads) on -> (fp64 (..., 7 + 5d), bound)."""
    d = max_depth + 1
    m = cmap(max_depth, shift)
    first = cmap(max_depth)["bounce"] if first is None else first
    g = lambda k, n: np.asarray(x[..., m[k] - first:m[k] - first + n], dtype=np.float64)      # noqa: E731
    vals, bounds = [], []
    with np.errstate(all="ignore"):
        for k, n, c, div in (("pweight", 1, 1e-6, 90.0), ("rwow", 3, 1e-6, 30.0), ("light", 3, 1e-8, 10.0), ("thr", 3 * d, 1e-6, 30.0)):
            v = np.log(g(k, n) + float(np.float32(c))) / div
            vals.append(v)
            bounds.append(U / div + (LOG_ULPS + 1) * ULP * np.abs(v) + ETA)
        v = g("bounce", d) / 19.0
        vals.append(v)
        bounds.append(ULP * np.abs(v) + ETA)
        v = np.sqrt(g("rough", d))
        vals.append(v)
        bounds.append(ULP * np.abs(v) + ETA)
    return np.concatenate(vals, -1), np.concatenate(bounds, -1)


def llpm(raw, max_depth=5, shift=0):
    assert raw.shape[-1] >= min_channels(max_depth)
    return llpm_tail(np.asarray(raw), max_depth, first=0, shift=shift)


SB_S = 27


def sbmc_split(max_depth=5):
    """The exact (copied, clamped, bit-derived) and the log channels of sbmc_s (27) and sbmc_p (11 d), as boolean masks."""
    d = max_depth + 1
    log_s, log_p = np.zeros(SB_S, dtype=bool), np.zeros(11 * d, dtype=bool)
    log_s[3:9], log_p[:4 * d] = True, True
    return log_s, log_p


def bounce_code(v):
    """astype(int16) of a bounce code where int16 holds the value truncated toward zero; 0 (no tags) otherwise."""
    t = np.trunc(np.asarray(v, dtype=np.float64))
    return np.where((t >= -32768) & (t <= 32767), t, 0.0).astype(np.int64)


def sbmc(raw, max_depth=5, shift=0):
    """raw (..., C >= 24 + 7 d) fp32, the channels _preprocess_sbmc reads (subpixel 0:2, radiance 2:5, diffuse 5:8, g-buffer 8:24,
    probabilities 24:24+4d, light directions 24+4d:24+6d, bounce types 24+6d:24+7d) -> (want_s (..., 27), want_p (..., 11 d),
    bound_s, bound_p) in fp64.  bound = 0 on every copied, clamped or bit-derived channel.  The log groups follow llpm_tail's
    rule -- U / k for each rounded operation in front of the logarithm (relative U of the argument is absolute U of the logarithm),
    LOG_ULPS of logf and 1 ulp of the division relative to the result:
        log(1 + max(total, 0)) / 10                        one addition:                      U / 10 + (LOG_ULPS + 1) ULP |v|
        log(1 + max(max(total, 0) - max(diffuse, 0), 0)) / 10   a subtraction (|its error| <= U |difference| <= U (1 + difference))
                                                           and an addition:                 2 U / 10 + (LOG_ULPS + 1) ULP |v|
        log(max(prob, 0) + 1e-5) / 30                      one addition:                      U / 30 + (LOG_ULPS + 1) ULP |v|
    shift = 1: the WRONG variant with the channels from the probabilities on read one further up."""
    raw = np.asarray(raw)
    d = max_depth + 1
    assert raw.shape[-1] >= 24 + 7 * d + shift
    x = lambda a, b: raw[..., a:b].astype(np.float64)          # noqa: E731
    p0 = 24 + shift
    with np.errstate(all="ignore"):
        total, dif = np.maximum(x(2, 5), 0), np.maximum(x(5, 8), 0)
        lt = np.log(1 + total) / 10.0
        ls = np.log(1 + np.maximum(total - dif, 0)) / 10.0
        want_s = np.concatenate([total, lt, ls, x(0, 2), x(8, 24)], -1)
        bound_s = np.zeros_like(want_s)
        bound_s[..., 3:6] = U / 10.0 + (LOG_ULPS + 1) * ULP * np.abs(lt) + ETA
        bound_s[..., 6:9] = 2 * U / 10.0 + (LOG_ULPS + 1) * ULP * np.abs(ls) + ETA
        lp = np.log(np.maximum(x(p0, p0 + 4 * d), 0) + float(np.float32(1e-5))) / 30.0
        code = bounce_code(raw[..., p0 + 6 * d:p0 + 7 * d])
        tags = [((code >> k) & 1).astype(np.float64) for k in range(5)]
        want_p = np.concatenate([lp, np.clip(x(p0 + 4 * d, p0 + 6 * d), -1.0, 1.0)] + tags, -1)
        bound_p = np.zeros_like(want_p)
        bound_p[..., :4 * d] = U / 30.0 + (LOG_ULPS + 1) * ULP * np.abs(lp) + ETA
    return want_s, want_p, bound_s, bound_p


def gradients(buf, forward=False):
    """(h, w, c) fp32 -> (h, w, 2c) fp32: one fp32 subtraction per element, zero first column / row -- compared bit for bit."""
    buf = np.asarray(buf, dtype=np.float32)
    dx, dy = np.zeros_like(buf), np.zeros_like(buf)
    if forward:
        dx[:, :-1], dy[:-1] = buf[:, 1:] - buf[:, :-1], buf[1:] - buf[:-1]
    else:
        dx[:, 1:], dy[1:] = buf[:, 1:] - buf[:, :-1], buf[1:] - buf[:-1]
    return np.concatenate([dx, dy], 2)


# ---------------------------------------------------------------------------------------------------- comparisons
TABLE = {}           # (kernel, channel group) -> largest |err| / bound seen


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _kp_slices():
    for k in KP_GROUPS:
        c0, nv = KP_START[k], 1 if k == "depth" else 3
        yield k, slice(c0, c0 + nv)
        yield k + "_v", slice(c0 + nv, c0 + nv + 1)
        yield "d_" + k, slice(c0 + nv + 1, c0 + 3 * nv + 1)


def assert_within(got, want, bound, what="", kernel=None):
    """EVERY element: NaN exactly where the reference is NaN, |got - want| <= bound elsewhere.  kernel: the row of TABLE the largest
    ratio of each channel group goes to (KPCN buffers: the fifteen groups; anything else: one column)."""
    got, want, bound = _np(got).astype(np.float64), _np(want), _np(bound)
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ (%d got, %d wanted; first at %s)" % (
        what, int(gn.sum()), int(wn.sum()), tuple(int(i) for i in np.argwhere(gn != wn)[0]))
    with np.errstate(all="ignore"):
        err = np.where(wn, 0.0, np.abs(got - want))
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    worst = float(r.max()) if r.size else 0.0
    if kernel is not None:
        cols = list(_kp_slices()) if got.shape[-1] == 44 and got.ndim >= 3 else [("all", slice(None))]
        for name, sl in cols:
            key = (kernel, name)
            TABLE[key] = max(TABLE.get(key, 0.0), float(r[..., sl].max()) if r.size else 0.0)
    print("%s: max |err| / bound = %.3f" % (what, worst))
    if worst > 1.0:
        i = tuple(int(v) for v in np.unravel_index(int(r.argmax()), r.shape))
        raise AssertionError("%s: |err| / bound = %.3e > 1 at %s: got %r, want %r, bound %.3e" % (what, worst, i, got[i], want[i], bound[i]))


def assert_bit_equal(got, want, what=""):
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ (%d got, %d wanted)" % (what, int(gn.sum()), int(wn.sum()))
    bad = (got != want) & ~gn
    assert not bad.any(), "%s: %d entries differ, first at %s" % (what, int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))


def format_table():
    """The largest |err| / bound per kernel (rows) and channel group (columns) seen so far, as text."""
    kernels = sorted({k for k, _ in TABLE})
    cols = [n for n, _ in _kp_slices()] + ["all"]
    cols = [c for c in cols if any((k, c) in TABLE for k in kernels)]
    lines = ["%-22s" % "kernel" + "".join("%11s" % c for c in cols)]
    for k in kernels:
        lines.append("%-22s" % k + "".join(("%11.3f" % TABLE[(k, c)]) if (k, c) in TABLE else "%11s" % "-" for c in cols))
    return "\n".join(lines) + "\n"


# ---------------------------------------------------------------------------------------------------- inputs
SMALL_SHAPES = [(5, 7), (1, 13), (13, 1), (1, 1), (21, 19)]
LANES_S = [1, 2, 4, 8, 16, 32, 64]
PIXEL_S = [3, 5, 7, 12, 65, 128]
MAPS = [(0, 49), (1, 60), (3, 84), (4, 93), (5, 104), (5, 105), (5, 108), (6, 115)]
NAN = float("nan")


def make_frame(h, w, s, max_depth=5, C=None, seed=0, fill="kpcn", device="cpu", depth="default"):
    """Raw renderer output (h, w, s, C) with the value ranges of tests/golden/make_golden.raw_samples for any channel map, made from
    a seed on ``device``.  Channels the function under test must not read hold NaN -- fill "kpcn": everything but 2..7 and
    albedo..depth; fill "llpm": everything below the bounce types, albedo..depth, and the channels past the map's last.
    Pixel p (row-major) is special when
        p % 5 == 1   all samples equal to the first one (variance exactly 0)
        p % 7 == 3   depth near 1e4 with a spread of 1e-2 (the mean's error squared is of the variance's size)
        p % 11 == 5  exact zeros in radiance, diffuse, albedo and depth
    depth: "default" | "zero" | "negative" (all in [-40, 0): no scaling, clipped to 0) | "one_positive" (negative but pixel
    npix // 2) | "first" / "last" (the deepest pixel, 2e4, at pixel 0 / npix - 1)."""
    C = min_channels(max_depth) if C is None else C
    m, d = cmap(max_depth), max_depth + 1
    g = torch.Generator(device=device).manual_seed(seed)
    rand = lambda *sh: torch.rand(*sh, generator=g, device=device)          # noqa: E731
    randn = lambda *sh: torch.randn(*sh, generator=g, device=device)        # noqa: E731
    x = torch.full((h, w, s, C), NAN, device=device, dtype=torch.float32)
    n = (h, w, s)
    if fill == "kpcn":
        x[..., 2:8] = randn(*n, 6) * 2.0
        x[..., m["albedo"]:m["albedo"] + 3] = rand(*n, 3)
        x[..., m["normal"]:m["normal"] + 3] = randn(*n, 3)
        x[..., m["depth"]] = rand(*n) * 40.0
        p = torch.arange(h * w, device=device).view(h, w)
        dch = x[..., m["depth"]]                                              # (a view)
        if depth == "zero":
            dch.zero_()
        elif depth in ("negative", "one_positive"):
            dch.neg_().sub_(1e-3)
        near = (p % 7 == 3)
        if depth in ("default", "first", "last"):
            dch[near] = 1e4 + (rand(*n)[near] - 0.5) * 1e-2
        zero = (p % 11 == 5)
        for c in list(range(2, 8)) + list(range(m["albedo"], m["albedo"] + 3)) + ([m["depth"]] if depth == "default" else []):
            x[..., c][zero] = 0.0
        same = (p % 5 == 1)
        x[same] = x[same][:, :1].expand(-1, s, -1)
        if depth == "one_positive":
            dch.view(h * w, s)[(h * w) // 2] = 3.0
        elif depth == "first":
            dch.view(h * w, s)[0] = 2e4
        elif depth == "last":
            dch.view(h * w, s)[h * w - 1] = 2e4
    elif fill == "llpm":
        x[..., m["bounce"]:m["bounce"] + d] = torch.randint(0, 20, (*n, d), generator=g, device=device).float()
        x[..., m["pweight"]] = torch.exp(randn(*n) * 3.0)
        x[..., m["rwow"]:m["rwow"] + 3] = torch.exp(randn(*n, 3) * 2.0)
        x[..., m["light"]:m["light"] + 3] = rand(*n, 3) * 1e4
        thr = torch.exp(randn(*n, 3 * d) * 2.0)
        thr[rand(*n, 3 * d) < 0.3] = 0.0                                     # exact zeros: the path ended
        x[..., m["thr"]:m["thr"] + 3 * d] = thr
        x[..., m["rough"]:m["rough"] + d] = rand(*n, d)
    else:
        raise ValueError(fill)
    return x


# The value edges of _preprocess_sbmc, one set per planted record.  bounce: codes cycled over the d bounce channels --
# truncation toward zero of non-integer and negative codes, the int16 boundaries (-32768 and 32767.x are held, +-32768.x and
# beyond are not), the 1e38 of sanitising; rad / dif: radiance and diffuse (total < diffuse: log 1 = 0; equal: exactly 0);
# prob: a non-positive probability is log(1e-5) / 30; light: directions exactly at and one ulp past +-1.
_ONE_UP = float(np.nextafter(np.float32(1), np.float32(2)))
SBMC_EDGES = (
    dict(bounce=(5.9, -3.0, 32767.5, -32768.0), rad=0.5, dif=2.0, prob=0.0, light=(1.0, -1.0)),
    dict(bounce=(1e38, -32768.5, 32768.5, -1e38), rad=-1.0, dif=3.0, prob=-0.25, light=(-1.0, 1.0)),
    dict(bounce=(-0.9, 31.999, -5.5, 32767.0), rad=1.75, dif=1.75, prob=1e-5, light=(_ONE_UP, -_ONE_UP)),
    dict(bounce=(-32767.5, 32768.0, -32769.0, 0.5), rad=0.0, dif=-2.0, prob=-0.0, light=(0.0, -0.0)),
)


def sbmc_edge_records(n):
    """The planted records of make_sbmc_frame: 0, the tile edges 127 / 128 (SB_TILE = 128), n - 1 and their neighbours."""
    return sorted({r for r in (0, 1, 2, 3, 126, 127, 128, 129, n - 2, n - 1) if 0 <= r < n})


def make_sbmc_frame(n, max_depth=5, C=None, seed=0, device="cpu"):
    """Raw renderer output of n records as (n, 1, 1, C), made from a seed on ``device``: what _preprocess_sbmc reads (channels
    [0, 24 + 7 d)) on both sides of every clamp, every channel above (which it must not read) NaN.  Record sbmc_edge_records(n)[i]
    holds SBMC_EDGES[i % 4] in every channel of the group."""
    C = min_channels(max_depth) if C is None else C
    d = max_depth + 1
    used = 24 + 7 * d
    assert C >= used
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.full((n, 1, 1, C), NAN, device=device, dtype=torch.float32)
    f = x.view(n, C)
    f[:, 0:2] = torch.rand(n, 2, generator=g, device=device)
    f[:, 2:8] = torch.randn(n, 6, generator=g, device=device) * 2.0
    f[:, 8:24] = torch.randn(n, 16, generator=g, device=device)
    prob = torch.exp(torch.randn(n, 4 * d, generator=g, device=device) * 2.0)
    prob[torch.rand(n, 4 * d, generator=g, device=device) < 0.3] *= -1.0
    f[:, 24:24 + 4 * d] = prob
    f[:, 24 + 4 * d:24 + 6 * d] = torch.rand(n, 2 * d, generator=g, device=device) * 3.0 - 1.5
    f[:, 24 + 6 * d:used] = torch.randint(0, 32, (n, d), generator=g, device=device).float()
    for i, r in enumerate(sbmc_edge_records(n)):
        e = SBMC_EDGES[i % len(SBMC_EDGES)]
        f[r, 2:5], f[r, 5:8], f[r, 24:24 + 4 * d] = e["rad"], e["dif"], e["prob"]
        f[r, 24 + 4 * d:24 + 6 * d] = torch.tensor([e["light"][k % 2] for k in range(2 * d)], device=device)
        f[r, 24 + 6 * d:used] = torch.tensor([e["bounce"][(k + r) % 4] for k in range(d)], device=device)
    return x


def own_maximum_frame(h, w, S):
    """Pixel q = npix // 3 holds depth 0 in its first sample and 3e4 in every later one: the prefix of one sample normalises by
    another pixel's mean depth, every longer prefix by this pixel's.  One shared maximum slot could not serve both."""
    raw = make_frame(h, w, S, seed=300 + S)
    d = raw[..., cmap(5)["depth"]].view(h * w, S)
    q = (h * w) // 3
    d[q, 0] = 0.0
    d[q, 1:] = 3e4
    return raw


def overflow_frame(s):
    """The 5 x 7 x s frame of make_golden.raw_samples whose pixel (2, 3) holds 1e38 in every depth sample (what sanitize_ leaves of
    Inf): from four samples on the fp32 sum overflows, the mean and with it the image maximum are Inf."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as mg
    raw = mg.raw_samples(5, 7, s, 55)
    raw[2, 3, :, cmap(5)["depth"]] = 1e38
    return raw


def offset_view(x, off):
    """The same contiguous tensor at a storage offset of ``off`` floats (data pointer 4 * off bytes past a 16-byte boundary)."""
    flat = torch.empty(x.numel() + 4, device=x.device, dtype=x.dtype)
    assert flat.data_ptr() % 16 == 0
    flat[off:off + x.numel()].copy_(x.reshape(-1))
    v = flat[off:off + x.numel()].view(x.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v
