"""Image metrics of the evaluation script (the reference's ``support/metrics.py`` and the tone maps of
``test_models.py:24-34``), on the MI355X.

Same names and signatures as the reference: ``_tonemap``, ``MSE``, ``RelMSE``, ``TRelMSE``, ``L1``, ``RelL1``, ``SSIM``
(``reduce=``, ``eps=``), plus ``tonemap`` and ``evaluate_frame``.  Inputs are (H, W, 3) numpy arrays or torch tensors; numpy
input is moved to the current device as fp32.

* ``reduce=True`` runs the HIP kernel ``wcmc_image_eval`` (fp64 inside) and returns a Python float.
* ``reduce=False`` returns what the reference returns, as a device tensor computed with torch elementwise ops: the per-entry
  error map, and for ``RelMSE`` the raveled array of its non-NaN entries.  ``SSIM(reduce=False)`` raises: the reference's
  ``1 - ssim(..., full=True)`` subtracts a tuple, a TypeError.

SSIM is this build's specification of ``skimage.metrics.structural_similarity(im, ref, multichannel=True)`` (skimage is not a
dependency here and the reference does not pin its version): a 7x7 uniform window, K1 = 0.01, K2 = 0.03, the sample covariance
(49/48), ``data_range = 2`` (skimage before 0.21 -- the last versions that accept ``multichannel=`` -- derives it from the
float dtype's range (-1, 1)), float64 arithmetic, and the SSIM map averaged over the interior cropped by 3 pixels on every
side, per channel, then over the three channels.  Images smaller than 7 x 7 are rejected.  DESIGN.md section 10.
"""
import numpy as np
import torch

from .. import ops as _ops

EPS = 1e-4                                   # metrics.py: RelMSE / RelL1 (the training loss RelativeMSE uses 1e-2)
TONEMAPS = ("linear", "_tonemap", "tonemap", "tonemap28")          # test_models.py:246
METRICS = ("RelMSE", "RelL1", "DSSIM", "L1", "MSE")                # test_models.py:245


def _dev(x):
    if isinstance(x, torch.Tensor):
        return x if x.is_cuda else x.to(torch.cuda.current_device())
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=torch.cuda.current_device())


def _f32(x):
    x = _dev(x)
    return x if x.dtype == torch.float32 else x.float()


def _eval(im, ref, eps=EPS):
    """image_eval with ``im`` in the first comparison slot: [tone map][metric] of im vs ref (fp64 device)."""
    im, ref = _f32(im), _f32(ref)
    return _ops.image_eval(im, im, ref, eps=eps)[0]


def _tonemap(im):
    """metrics.py:24-27: max(x, 0) / (1 + max(x, 0)) (NaN stays NaN, as with np.clip)."""
    col = _dev(im).clone()
    col = torch.where(col < 0, torch.zeros_like(col), col)
    return col / (1.0 + col)


def tonemap(c, ref=None, kInvGamma=1.0 / 2.2):
    """test_models.py:24-34: c / (1 + L(ref) / 1.5), clipped to >= 0, raised to kInvGamma, clipped to <= 1; L is the
    Rec. 709 luminance of ``ref`` (default: of ``c`` itself)."""
    c = _dev(c)
    ref = c if ref is None else _dev(ref)
    lum = 0.2126 * ref[:, :, 0] + 0.7152 * ref[:, :, 1] + 0.0722 * ref[:, :, 2]
    col = c / (1 + lum / 1.5)[:, :, None]
    col = torch.where(col < 0, torch.zeros_like(col), col)
    col = col ** kInvGamma
    return torch.where(col > 1, torch.ones_like(col), col)


def MSE(im, ref, reduce=True):
    """Mean-squared error between images."""
    if reduce:
        return float(_eval(im, ref)[0, 4])
    return (_dev(im) - _dev(ref)) ** 2


def RelMSE(im, ref, eps=EPS, reduce=True):
    """Relative mean-squared error (a-r)^2 / (r^2 + eps), over the non-NaN entries."""
    if reduce:
        return float(_eval(im, ref, eps)[0, 0])
    im, ref = _dev(im), _dev(ref)
    diff = ((im - ref) ** 2 / (ref ** 2 + eps)).reshape(-1)
    return diff[~torch.isnan(diff)]


def TRelMSE(im, ref, eps=EPS, reduce=True):
    """RelMSE of the ``_tonemap``-ed images."""
    if reduce:
        return float(_eval(im, ref, eps)[1, 0])
    return RelMSE(_tonemap(im), _tonemap(ref), eps, reduce=False)


def L1(im, ref, reduce=True):
    """Absolute error between images."""
    if reduce:
        return float(_eval(im, ref)[0, 3])
    return (_dev(im) - _dev(ref)).abs()


def RelL1(im, ref, eps=EPS, reduce=True):
    """Relative absolute error |a-r| / (|r| + eps)."""
    if reduce:
        return float(_eval(im, ref, eps)[0, 1])
    im, ref = _dev(im), _dev(ref)
    return (im - ref).abs() / (ref.abs() + eps)


def SSIM(im, ref, reduce=True):
    """Structural dissimilarity 1 - SSIM (the module docstring has the specification)."""
    if not reduce:
        raise TypeError("SSIM(reduce=False): the reference returns 1 - ssim(..., full=True), which subtracts a tuple; "
                        "there is no per-pixel DSSIM map to return")
    return float(_eval(im, ref)[0, 2])


def evaluate_frame(out, ipt, tgt, has_hit=None):
    """All 40 numbers of one frame in one launch and one synchronisation: ``(out_row, ipt_row)``, two fp64 numpy 20-vectors in
    the CSV's row order 5 * t + k (tone map t in TONEMAPS, metric k in METRICS).  ``out`` is replaced by ``ipt`` where
    ``has_hit == 0`` (test_models.py:231-232) inside the kernel."""
    r = _ops.image_eval(_f32(out), _f32(ipt), _f32(tgt), None if has_hit is None else _f32(has_hit))
    r = r.reshape(2, 20).cpu().numpy()
    return r[0], r[1]
