"""fp64 restatement of the kernel-splat specification, for tests and scripts.

A source pixel q sends tap t = (dy + r) * k + (dx + r) to the destination q + (dy, dx); destinations outside the image are
dropped.  ``F.fold``'s overlap-add with ``kernel_size=k, padding=r`` is exactly that sum: block q's element (ky, kx) lands on the
padded coordinate q + (ky, kx), i.e. on q + (ky - r, kx - r) of the image.  ``splat_loop`` is the same sum as a direct loop
(tests/test_cpu_kernel_splat.py holds the two to 1e-15)."""
import torch
import torch.nn.functional as F


def splat_weights(logits, shift=None):
    """(N, k2, h, w) weights: a softmax over each source pixel's taps, or ``exp(logits - shift[n])``."""
    if shift is None:
        m = logits.amax(dim=1, keepdim=True)
        e = torch.exp(logits - m)
        return e / e.sum(dim=1, keepdim=True)
    return torch.exp(logits - shift.view(-1, 1, 1, 1))


def splat_ref(data, logits, shift=None):
    """(sum_r (N, C, h, w), sum_w (N, h, w)) of the dtype of the inputs (fp64 in the tests); differentiable."""
    n, k2, h, w = logits.shape
    c = data.shape[1]
    k = int(round(k2 ** 0.5))
    assert k * k == k2 and k % 2 == 1
    wt = splat_weights(logits, shift)
    cols = (data.unsqueeze(2) * wt.unsqueeze(1)).reshape(n, c * k2, h * w)
    sum_r = F.fold(cols, (h, w), kernel_size=k, padding=k // 2)
    sum_w = F.fold(wt.reshape(n, k2, h * w), (h, w), kernel_size=k, padding=k // 2)
    return sum_r, sum_w[:, 0]


def splat_loop(data, logits, shift=None):
    """The same sums by the four-deep loop of the specification (small shapes only)."""
    n, k2, h, w = logits.shape
    c = data.shape[1]
    k = int(round(k2 ** 0.5))
    r = k // 2
    wt = splat_weights(logits, shift)
    sum_r = torch.zeros((n, c, h, w), dtype=data.dtype)
    sum_w = torch.zeros((n, h, w), dtype=data.dtype)
    for qy in range(h):
        for qx in range(w):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    py, px = qy + dy, qx + dx
                    if 0 <= py < h and 0 <= px < w:
                        t = (dy + r) * k + (dx + r)
                        sum_r[:, :, py, px] += wt[:, t, qy, qx].unsqueeze(1) * data[:, :, qy, qx]
                        sum_w[:, py, px] += wt[:, t, qy, qx]
    return sum_r, sum_w
