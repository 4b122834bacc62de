"""Filtering a frame by its P-buffer (csrc/pbuffer_filter.hip)."""
import torch

from .._lib import check, lib
from ._base import _Timed, _ptr, _stream

PBF_MAX_RADIUS, PBF_MAX_PATCH_RADIUS, PBF_MAX_CHANNELS, PBF_MAX_IMAGE_CHANNELS = 10, 3, 32, 4
PBF_STATS, PBF_FILTER = 1, 2                   # the launches of one call (``passes``: their sum by default)


def _pbuffer_filter_check(image, p_buffer, radius, patch_radius, bandwidth, eps, mask):
    """Everything that can be refused before a device is touched; returns (H, W, Cr, S, C)."""
    for name, t in (("image", image), ("p_buffer", p_buffer)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("pbuffer_filter: %s must be a tensor (got %s)" % (name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("pbuffer_filter: %s must be float32 (got %s)" % (name, t.dtype))
        if t.requires_grad:
            raise RuntimeError("pbuffer_filter: %s requires grad, and the filter has no backward: detach it" % name)
    if image.dim() != 3 or p_buffer.dim() != 4:
        raise ValueError("pbuffer_filter: image must be (H, W, Cr) and p_buffer (S, C, H, W) (got %s and %s)"
                         % (tuple(image.shape), tuple(p_buffer.shape)))
    h, w, cr = image.shape
    s, c = p_buffer.shape[:2]
    if tuple(p_buffer.shape[2:]) != (h, w):
        raise ValueError("pbuffer_filter: image %s and p_buffer %s differ in frame size" % (tuple(image.shape), tuple(p_buffer.shape)))
    if h < 1 or w < 1 or s < 1:
        raise ValueError("pbuffer_filter: empty frame or no samples (image %s, p_buffer %s)" % (tuple(image.shape), tuple(p_buffer.shape)))
    if not 1 <= cr <= PBF_MAX_IMAGE_CHANNELS:
        raise ValueError("pbuffer_filter: the image has %d channels (1..%d are supported)" % (cr, PBF_MAX_IMAGE_CHANNELS))
    if not 1 <= c <= PBF_MAX_CHANNELS:
        raise ValueError("pbuffer_filter: the P-buffer has %d channels (1..%d are supported)" % (c, PBF_MAX_CHANNELS))
    if int(radius) != radius or not 0 <= radius <= PBF_MAX_RADIUS:
        raise ValueError("pbuffer_filter: radius %r (an integer in 0..%d)" % (radius, PBF_MAX_RADIUS))
    if int(patch_radius) != patch_radius or not 0 <= patch_radius <= PBF_MAX_PATCH_RADIUS:
        raise ValueError("pbuffer_filter: patch_radius %r (an integer in 0..%d)" % (patch_radius, PBF_MAX_PATCH_RADIUS))
    if not bandwidth > 0 or not eps > 0:
        raise ValueError("pbuffer_filter: bandwidth %r and eps %r must be positive" % (bandwidth, eps))
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (h, w):
            raise ValueError("pbuffer_filter: mask must be an (H, W) = (%d, %d) tensor (got %s)"
                             % (h, w, tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__))
        if mask.dtype not in (torch.uint8, torch.bool, torch.float32):
            raise TypeError("pbuffer_filter: mask must be uint8, bool or float32 (got %s)" % mask.dtype)
    return h, w, cr, s, c


def pbuffer_filter(image, p_buffer, radius=10, patch_radius=1, bandwidth=1.0, eps=1e-3, mask=None, passes=PBF_STATS | PBF_FILTER,
                   workspace=None):
    """Average every pixel of ``image`` (H, W, Cr <= 4) with the neighbours, within ``radius``, whose P-buffer statistics agree with
    its own: ``(out (H, W, Cr), wsum (H, W))``.  ``p_buffer`` is (S, C, H, W), C <= 32; both inputs are taken with the strides they
    have (a permuted CHW image, the permuted (H, W, S, C) array of ``--save_pbuffer``: no copy).  ``mask`` (H, W) uint8, bool or
    float32: a pixel whose element is zero keeps its value, gets ``wsum`` 0 and is left out of its neighbours' averages.  ``wsum``
    is the effective number of neighbours the manifold takes for the same surface and light path.  No autograd.  The defaults are
    starting points: nobody has tuned them on a trained model's P-buffer.  ``passes`` and ``workspace`` (the float32 tensor a
    previous call's statistics lie in) are for timing the two launches apart."""
    h, w, cr, s, c = _pbuffer_filter_check(image, p_buffer, radius, patch_radius, bandwidth, eps, mask)
    for t in (image, p_buffer, mask):
        if t is not None and not t.is_cuda:
            raise RuntimeError("wcmc_amd ops run on the MI355X only (got a %s tensor); there is no CPU path" % t.device)
    mask_bytes = 0
    if mask is not None:
        mask = mask.contiguous()
        mask_bytes = 4 if mask.dtype == torch.float32 else 1
    nbytes = lib().wcmc_pbuffer_filter_workspace_bytes(s, c, h, w)
    if nbytes == 0:
        raise ValueError("pbuffer_filter: unsupported shape (S=%d C=%d H=%d W=%d)" % (s, c, h, w))
    if workspace is not None and not (workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous()):
        raise ValueError("pbuffer_filter: workspace must be a contiguous float32 device tensor")
    ws = workspace if workspace is not None else torch.empty(nbytes // 4, device=image.device, dtype=torch.float32)
    out = torch.empty((h, w, cr), device=image.device, dtype=torch.float32)
    wsum = torch.empty((h, w), device=image.device, dtype=torch.float32)
    # algorithmic bytes: the P-buffer and the image in, the image and the weight sum out
    with _Timed("pbuffer_filter", 4.0 * h * w * (s * c + 2 * cr + 1), "byte"):
        check(lib().wcmc_pbuffer_filter(_ptr(image), *image.stride(), _ptr(p_buffer), *p_buffer.stride(), _ptr(mask), mask_bytes,
                                        _ptr(out), _ptr(wsum), _ptr(ws), ws.numel() * 4, h, w, s, c, cr, int(radius),
                                        int(patch_radius), float(bandwidth), float(eps), int(passes), _stream()), "pbuffer_filter")
    return out, wsum
