"""The feathered stitch of DESIGN.md section 22 restated in fp64 numpy, for tests/test_cpu_denoise_tiles.py and
tests/test_gpu_denoise_tiles.py.  It shares no code with the library: the tile table is taken as data (``frame_tiles`` has its own
tests), the weights are the section's formulas evaluated in fp64, and the sums are plain fp64 sums."""
import numpy as np


def axis_weight(x, a, b, n, f):
    """u(x) = L(x) * R(x) of the owned interval [a, b) on an axis of length n, for integer positions x (any array)."""
    x = np.asarray(x, np.float64)
    if f == 0:
        return ((x >= a) & (x < b)).astype(np.float64)
    left = np.ones_like(x) if a == 0 else np.clip((x - a + f + 0.5) / (2.0 * f), 0.0, 1.0)
    right = np.ones_like(x) if b == n else np.clip((b + f - x - 0.5) / (2.0 * f), 0.0, 1.0)
    return left * right


def axis_range(a, b, n, f):
    """[a - F, b + F) clipped to [0, n): where the tile that owns [a, b) contributes."""
    return max(a - f, 0), min(b + f, n)


def tile_weight(row, ht, wt, f):
    """(ys, xs, w): the rows and columns a tile of the table contributes to and its 2-D weight there, (len(ys), len(xs))."""
    i0, j0, i1, j1 = row[:4]
    ys, xs = np.arange(*axis_range(i0, i1, ht, f)), np.arange(*axis_range(j0, j1, wt, f))
    return ys, xs, np.outer(axis_weight(ys, i0, i1, ht, f), axis_weight(xs, j0, j1, wt, f))


def replicate_pad(out, patch):
    """The network output (..., ho, wo) padded back to (..., patch, patch) as ``F.pad(..., 'replicate')`` of the reference's inference
    loop does it: ``(patch - ho) // 2`` pixels before, the rest after."""
    out = np.asarray(out)
    ph, pw = patch - out.shape[-2], patch - out.shape[-1]
    width = [(0, 0)] * (out.ndim - 2) + [(ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2)]
    return np.pad(out, width, "edge")


def turn(a, t, axes=(0, 1)):
    """T_t on two axes of an array: a left-right flip where t & 4, then t & 3 quarter turns."""
    a = np.flip(a, axes[1]) if t & 4 else a
    return np.rot90(a, k=t & 3, axes=axes)


def turn_back(a, t, axes=(0, 1)):
    a = np.rot90(a, k=-(t & 3), axes=axes)
    return np.flip(a, axes[1]) if t & 4 else a


def blend(table, tiles, ht, wt, f, patch):
    """(num, den, mag) of the ht x wt frame in fp64: the sums over the table's tiles of w * v, w and w * |v|, v the replicate-padded
    (B, 3, ho, wo) ``tiles``.  num, mag: (3, ht, wt); den: (ht, wt).  The blended frame is num / den."""
    v = replicate_pad(np.asarray(tiles, np.float64), patch)
    num, den, mag = np.zeros((3, ht, wt)), np.zeros((ht, wt)), np.zeros((3, ht, wt))
    for k, row in enumerate(table):
        ys, xs, w = tile_weight(row, ht, wt, f)
        if not len(ys) or not len(xs):
            continue
        val = v[k][:, ys[0] - row[4]:ys[-1] + 1 - row[4], xs[0] - row[5]:xs[-1] + 1 - row[5]]
        sl = (slice(None), slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
        num[sl] += w * val
        mag[sl] += w * np.abs(val)
        den[sl[1:]] += w
    return num, den, mag


def blend_source(table, tiles, h, w, t, f, patch):
    """``blend`` for the table of the frame transformed by code t, turned back to the h x w SOURCE orientation."""
    ht, wt = (w, h) if t & 1 else (h, w)
    num, den, mag = blend(table, tiles, ht, wt, f, patch)
    return turn_back(num, t, (1, 2)), turn_back(den, t, (0, 1)), turn_back(mag, t, (1, 2))


BAR = 16 * 2.0 ** -24       # per pixel, times sum w |v| / sum w (section 22: <= 3 roundings of a weight, 1 of the product, <= 8 additions
#                             per sum, 1 division)
