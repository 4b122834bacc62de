"""fp64 numpy restatement of the evaluation metrics (support/metrics.py, test_models.py:24-34, 231-251): the yardstick the
HIP kernel ``wcmc_image_eval`` is tested against.  SSIM follows the specification in DESIGN.md section 10 (skimage's
``structural_similarity`` before 0.21 with ``multichannel=True``): 7x7 uniform window, K1 0.01, K2 0.03, sample covariance,
data_range 2, float64, interior cropped by 3 pixels."""
import numpy as np
from scipy.ndimage import uniform_filter

EPS = 1e-4


def tm_linear(x):
    return x


def tm_reinhard(x):                  # metrics._tonemap
    col = np.clip(np.array(x, dtype=np.float64), 0.0, None)
    return col / (1.0 + col)


def tonemap(c, ref=None, kInvGamma=1.0 / 2.2):
    c = np.asarray(c, dtype=np.float64)
    ref = c if ref is None else np.asarray(ref, dtype=np.float64)
    lum = 0.2126 * ref[:, :, 0] + 0.7152 * ref[:, :, 1] + 0.0722 * ref[:, :, 2]
    col = c / (1 + lum / 1.5)[:, :, None]
    col = np.clip(col, 0, None)
    return np.clip(col ** kInvGamma, 0.0, 1.0)


def tonemap28(x):
    return tonemap(x, kInvGamma=1 / 2.8)


TONEMAPS = (tm_linear, tm_reinhard, tonemap, tonemap28)


def mse(a, r):
    return np.square(a - r).mean()


def l1(a, r):
    return np.abs(a - r).mean()


def rel_l1(a, r, eps=EPS):
    return (np.abs(a - r) / (np.abs(r) + eps)).mean()


def rel_mse(a, r, eps=EPS):
    d = np.ravel(np.square(a - r) / (np.square(r) + eps))
    d = d[~np.isnan(d)]
    return d.mean() if d.size else np.nan


def ssim(a, r):
    """Mean SSIM over the 3-pixel-cropped interior and the channels (uniform_filter form)."""
    a = np.asarray(a, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    win, K1, K2, R = 7, 0.01, 0.03, 2.0
    cov = win * win / (win * win - 1.0)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    pad = (win - 1) // 2
    vals = []
    for ch in range(a.shape[2]):
        X, Y = a[:, :, ch], r[:, :, ch]
        f = lambda z: uniform_filter(z, size=win)           # noqa: E731
        ux, uy = f(X), f(Y)
        uxx, uyy, uxy = f(X * X), f(Y * Y), f(X * Y)
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        vals.append(S[pad:-pad, pad:-pad].mean())
    return float(np.mean(vals))


def ssim_direct(a, r):
    """The same SSIM as an explicit 7x7 loop over every interior pixel (small images only)."""
    a = np.asarray(a, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    C1, C2, cov = (0.01 * 2) ** 2, (0.03 * 2) ** 2, 49.0 / 48.0
    h, w, c = a.shape
    vals = []
    for ch in range(c):
        tot = 0.0
        for y in range(3, h - 3):
            for x in range(3, w - 3):
                X = a[y - 3:y + 4, x - 3:x + 4, ch].ravel()
                Y = r[y - 3:y + 4, x - 3:x + 4, ch].ravel()
                ux, uy = X.mean(), Y.mean()
                vx = cov * ((X * X).mean() - ux * ux)
                vy = cov * ((Y * Y).mean() - uy * uy)
                vxy = cov * ((X * Y).mean() - ux * uy)
                tot += ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        vals.append(tot / ((h - 6) * (w - 6)))
    return float(np.mean(vals))


def metrics_row(a, r):
    """[RelMSE, RelL1, DSSIM, L1, MSE] of a vs r (test_models.py:245)."""
    return [rel_mse(a, r), rel_l1(a, r), 1.0 - ssim(a, r), l1(a, r), mse(a, r)]


def evaluate(out, ipt, tgt, has_hit=None):
    """(2, 4, 5) fp64: [out vs tgt, ipt vs tgt][tone map][metric], with the has_hit composite of test_models.py:231-232."""
    out, ipt, tgt = (np.asarray(x, dtype=np.float64) for x in (out, ipt, tgt))
    if has_hit is not None:
        out = np.where(np.asarray(has_hit) == 0, ipt, out)
    res = np.zeros((2, 4, 5))
    for t, tm in enumerate(TONEMAPS):
        r = tm(tgt)
        res[0, t] = metrics_row(tm(out), r)
        res[1, t] = metrics_row(tm(ipt), r)
    return res
