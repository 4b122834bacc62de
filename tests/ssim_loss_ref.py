"""fp64 torch restatement of the structural-similarity training loss: the yardstick the HIP op
``wcmc_dssim_loss_*`` is tested against.  ``F.avg_pool2d(., 7, stride=1)`` moments, differentiable; the same expression run on fp32
tensors is the gradient test's yardstick.  ``box_gradient`` is the closed form the backward kernel implements (three box sums of
per-window coefficient planes), kept apart from autograd so that one can be held to the other."""
import torch
import torch.nn.functional as F

WIN, K1, K2, COV = 7, 0.01, 0.03, 49.0 / 48.0


def tonemapped(v, tonemap):
    if tonemap == "none":
        return v
    assert tonemap == "reinhard", tonemap
    c = torch.clamp(v, min=0)
    return c / (1 + c)


def ssim_map(x, y, data_range=2.0):
    """S of every valid 7x7 window of two tone-mapped (N,C,H,W) tensors: (N,C,H-6,W-6), in the tensors' dtype."""
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    pool = lambda z: F.avg_pool2d(z, WIN, stride=1)                        # noqa: E731
    mx, my = pool(x), pool(y)
    vx, vy, vxy = COV * (pool(x * x) - mx * mx), COV * (pool(y * y) - my * my), COV * (pool(x * y) - mx * my)
    return ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def dssim(x, ref, tonemap="reinhard", data_range=2.0):
    """1 - mean S over every window of every plane; differentiable in x.  Computed in the dtype of ``x`` (pass fp64 for the reference)."""
    return 1 - ssim_map(tonemapped(x, tonemap), tonemapped(ref, tonemap), data_range).mean()


def dssim64(x, ref, tonemap="reinhard", data_range=2.0):
    """(loss, d loss / d x) in fp64 by autograd, on the CPU."""
    x64 = x.detach().double().cpu().clone().requires_grad_(True)
    loss = dssim(x64, ref.detach().double().cpu(), tonemap, data_range)
    loss.backward()
    return loss.detach(), x64.grad


def box_gradient(x, ref, tonemap="reinhard", data_range=2.0, g=1.0):
    """d loss / d x by the closed form of section 23: per window (a, b, c), then dL/dx_i = -g / (49 n_windows) *
    (box(a) + T(x_i) box(b) + T(y_i) box(c)) * T'(x_i), box = the zero-extended 7x7 sum over the windows that contain i."""
    x, ref = x.double(), ref.double()
    tx, ty = tonemapped(x, tonemap), tonemapped(ref, tonemap)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    pool = lambda z: F.avg_pool2d(z, WIN, stride=1)                        # noqa: E731
    mx, my = pool(tx), pool(ty)
    vx, vy, vxy = COV * (pool(tx * tx) - mx * mx), COV * (pool(ty * ty) - my * my), COV * (pool(tx * ty) - mx * my)
    A1, A2, B1, B2 = 2 * mx * my + c1, 2 * vxy + c2, mx * mx + my * my + c1, vx + vy + c2
    D = B1 * B2
    S = A1 * A2 / D
    dmu = 2 * my * A2 / D - 2 * mx * S / B1
    dvx, dvxy = -S / B2, 2 * A1 / D
    a, b, c = dmu - 2 * COV * dvx * mx - COV * dvxy * my, 2 * COV * dvx, COV * dvxy
    n, ch = x.shape[:2]
    ones = torch.ones(1, 1, WIN, WIN, dtype=torch.float64)
    box = lambda z: F.conv2d(z.reshape(n * ch, 1, *z.shape[2:]), ones, padding=WIN - 1).reshape(x.shape)    # noqa: E731
    dT = torch.ones_like(x) if tonemap == "none" else torch.where(x >= 0, 1 / (1 + x) ** 2, torch.zeros_like(x))
    return -g / (WIN * WIN * S.numel()) * (box(a) + tx * box(b) + ty * box(c)) * dT


def radiance(shape, seed, scale=1.0, negative=0.1):
    """Log-normal radiance with a fraction of negative entries and no exact zero (fp32, CPU)."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.exp(torch.randn(shape, generator=gen)) * scale
    flip = torch.rand(shape, generator=gen) < negative
    return torch.where(flip, -0.05 * v, v).float()
