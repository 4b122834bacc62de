"""The P-buffer filter restated from shifted planes, as a plain function of torch tensors, and as the
direct loop nest of the specification.  ``dtype`` is the arithmetic: fp64 is the reference that ``ops.pbuffer_filter`` is held to,
fp32 the same code at the kernel's precision -- its distance from fp64 is the reference's own fp32 error."""
import torch
import torch.nn.functional as F


def _shift(t, dy, dx):
    """t[..., y + dy, x + dx], zero where that lies outside."""
    h, w = t.shape[-2:]
    out = torch.zeros_like(t)
    ys, ye, xs, xe = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        out[..., ys:ye, xs:xe] = t[..., ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def rhf_stats(p_buffer, dtype=torch.float64):
    """(mu, v), each (C, H, W): the mean over the samples and the variance of the mean."""
    p = p_buffer.to(dtype)
    s = p.shape[0]
    mu = p.sum(0) / s
    return mu, ((p - mu) ** 2).sum(0) / (s * s)


def rhf_ref(image, p_buffer, radius=10, patch_radius=1, bandwidth=1.0, eps=1e-3, mask=None, dtype=torch.float64):
    """``(out (H, W, Cr), wsum (H, W))`` of image (H, W, Cr) and p_buffer (S, C, H, W) in ``dtype`` arithmetic."""
    img = image.to(dtype).permute(2, 0, 1)                                # (Cr, H, W)
    mu, v = rhf_stats(p_buffer, dtype)
    c, h, w = mu.shape
    r, f = int(radius), int(patch_radius)
    inside = torch.ones((h, w), dtype=torch.bool, device=mu.device)
    ok = inside if mask is None else (mask != 0)
    box = lambda t: F.avg_pool2d(t[None, None], 2 * f + 1, stride=1, padding=f, divisor_override=1)[0, 0]      # noqa: E731
    zero = torch.zeros((), dtype=dtype, device=mu.device)
    acc, wsum = torch.zeros_like(img), torch.zeros((h, w), dtype=dtype, device=mu.device)
    b2 = torch.tensor(bandwidth, dtype=dtype) ** 2
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            q_in = _shift(inside, dy, dx)                                 # q = p + (dy, dx) lies inside the image
            delta = ((mu - _shift(mu, dy, dx)) ** 2 / (eps + v + _shift(v, dy, dx))).sum(0) / c
            delta = torch.where(q_in, delta, zero)                        # pairs that do not exist add nothing and are not counted
            dist = box(delta) / box(q_in.to(dtype)).clamp(min=1.0)
            wgt = torch.where(q_in & _shift(ok, dy, dx), torch.exp(-dist / b2), zero)
            wsum = wsum + wgt
            acc = acc + wgt * _shift(img, dy, dx)
    out = torch.where(ok, acc / torch.where(ok, wsum, torch.ones_like(wsum)), img)
    return out.permute(1, 2, 0).contiguous(), torch.where(ok, wsum, zero)


def rhf_loop(image, p_buffer, radius, patch_radius, bandwidth=1.0, eps=1e-3, mask=None):
    """The specification as a loop nest over (p, q, o, c), in fp64 (small frames only)."""
    import math
    img = image.double()
    p = p_buffer.double()
    s, c, h, w = p.shape
    r, f = radius, patch_radius
    mu = [[[sum(p[k, ch, y, x].item() for k in range(s)) / s for x in range(w)] for y in range(h)] for ch in range(c)]
    var = [[[sum((p[k, ch, y, x].item() - mu[ch][y][x]) ** 2 for k in range(s)) / (s * s) for x in range(w)] for y in range(h)]
           for ch in range(c)]
    out, wsum = torch.zeros_like(img), torch.zeros((h, w), dtype=torch.float64)

    def delta(py, px, qy, qx):
        return sum((mu[ch][py][px] - mu[ch][qy][qx]) ** 2 / (eps + var[ch][py][px] + var[ch][qy][qx]) for ch in range(c)) / c
    for py in range(h):
        for px in range(w):
            if mask is not None and not bool(mask[py, px]):
                out[py, px] = img[py, px]
                continue
            acc, tot = torch.zeros(img.shape[2], dtype=torch.float64), 0.0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    qy, qx = py + dy, px + dx
                    if not (0 <= qy < h and 0 <= qx < w) or (mask is not None and not bool(mask[qy, qx])):
                        continue
                    dsum, cnt = 0.0, 0
                    for oy in range(-f, f + 1):
                        for ox in range(-f, f + 1):
                            if 0 <= py + oy < h and 0 <= px + ox < w and 0 <= qy + oy < h and 0 <= qx + ox < w:
                                dsum += delta(py + oy, px + ox, qy + oy, qx + ox)
                                cnt += 1
                    wgt = math.exp(-(dsum / cnt) / bandwidth ** 2)
                    tot += wgt
                    acc += wgt * img[qy, qx]
            out[py, px] = acc / tot
            wsum[py, px] = tot
    return out, wsum


def window_count(h, w, radius, device="cpu"):
    """(H, W): the number of window positions q that lie inside the image."""
    ys, xs = torch.arange(h, device=device), torch.arange(w, device=device)
    ny = torch.minimum(ys, torch.full_like(ys, radius)) + torch.minimum(h - 1 - ys, torch.full_like(ys, radius)) + 1
    nx = torch.minimum(xs, torch.full_like(xs, radius)) + torch.minimum(w - 1 - xs, torch.full_like(xs, radius)) + 1
    return (ny[:, None] * nx[None, :]).double()


def scene(h, w, s, c, cr=3, sigma=0.3, seed=0):
    """(image (H, W, Cr), p_buffer (S, C, H, W)), fp32: the smooth pattern sin(0.3 x + c) + 1.5 (c + 1) [y > H / 2] per channel plus
    per-sample noise, and an image with the same step edge.  Enlarging S, C or Cr keeps what smaller values gave (one base scene)."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(h, dtype=torch.float32)[:, None], torch.arange(w, dtype=torch.float32)[None, :]
    step = (ys > h / 2).float().expand(h, w)
    noise = torch.stack([torch.stack([torch.randn((h, w), generator=torch.Generator().manual_seed(1000 * (seed + 1) + 32 * k + j))
                                      for j in range(c)]) for k in range(s)])
    ch = torch.arange(c, dtype=torch.float32)[:, None, None]
    p = torch.sin(0.3 * xs + ch) + 1.5 * (ch + 1) * step + sigma * noise
    img = torch.rand((h, w, 4), generator=g)[:, :, :cr] + 0.5 * torch.cos(0.2 * ys + 0.1 * xs)[..., None] + 1.0 + 2.0 * step[..., None]
    return img.contiguous(), p.contiguous()
