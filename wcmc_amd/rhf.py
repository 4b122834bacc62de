"""Look at a learned path manifold: filter a frame by its P-buffer, as Ray Histogram Fusion does by ray-colour histograms.

    python -m wcmc_amd.rhf --image X.npy --pbuffer P.npy [--mask M.npy] --output_dir OUT
        [--radius 10] [--patch_radius 1] [--bandwidth 1.0] [--eps 1e-3] [--png]

``--image`` is an (H, W, 3) float frame (the noisy input, or any frame of the same size), ``--pbuffer`` the (H, W, S, C) array that
``wcmc_amd.evaluate --rhf`` (``p_buffer_<scene>_<model>.npy``) and ``wcmc_amd.denoise --save_pbuffer`` (``<stem>_pbuffer.npy``) write,
``--mask`` an optional (H, W) array: a pixel whose element is zero is left as it is and out of its neighbours' averages.  Every
pixel is averaged with the neighbours, within ``--radius``, whose P-buffer statistics agree with its own over a patch of
``--patch_radius`` (``ops.pbuffer_filter``).  ``OUT/<stem>_rhf.npy`` is the filtered frame,
``OUT/<stem>_rhf_neighbours.npy`` the (H, W) sum of the weights: the effective number of neighbours that the manifold takes for the
same surface and light path -- the picture of what the manifold has learned.  ``<stem>`` is that of ``--image``.  ``--png`` adds
8-bit previews: the frame under the tone map of the other previews, the neighbour count as ``wsum / (2R + 1)^2`` in grey.

The defaults (radius 10, patch radius 1, bandwidth 1.0, eps 1e-3) are starting points: nobody has tuned them on a trained model's
P-buffer.  ``wcmc_amd.denoise --rhf`` runs the same filter on the noisy input right after a frame is denoised.
"""
import argparse
import os

import numpy as np
import torch

from . import ops

DEFAULTS = dict(radius=10, patch_radius=1, bandwidth=1.0, eps=1e-3)
UNTUNED = "a starting point: nobody has tuned it on a trained model's P-buffer"


def rhf_filter(image, p_buffers, has_hit=None, **kw):
    """``ops.pbuffer_filter(image, P, mask=has_hit, **kw)`` with ``P`` the (S, C, H, W) tensor ``p_buffers``, or the channels of
    the ``{'diffuse', 'specular'}`` dict of a KPCN model concatenated along C (diffuse first): one distance over both manifolds.
    Returns ``(out (H, W, Cr), wsum (H, W))``."""
    if isinstance(p_buffers, dict):
        if not p_buffers:
            raise ValueError("rhf_filter: an empty dict of P-buffers")
        keys = [k for k in ("diffuse", "specular") if k in p_buffers] + sorted(k for k in p_buffers if k not in ("diffuse", "specular"))
        parts = [p_buffers[k] for k in keys]
        for k, t in zip(keys, parts):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[0] != parts[0].shape[0] or t.shape[2:] != parts[0].shape[2:]:
                raise ValueError("rhf_filter: the P-buffers of the branches must be (S, C, H, W) tensors of one S, H and W ('%s': %s)"
                                 % (k, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
        p_buffers = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    return ops.pbuffer_filter(image, p_buffers, mask=has_hit, **kw)


def neighbour_preview(wsum, radius):
    """(H, W, 3) uint8 grey picture of ``wsum / (2R + 1)^2`` (1: every pixel of the window counts in full)."""
    g = torch.nan_to_num(wsum / float((2 * radius + 1) ** 2), nan=0.0).clamp(0.0, 1.0)
    return torch.round(g * 255.0).to(torch.uint8)[..., None].expand(-1, -1, 3).contiguous().cpu().numpy()


def frame_preview(img):
    """(H, W, 3) uint8 picture of an (H, W, 3) frame under ``support.metrics.tonemap`` (gamma 1 / 2.2); NaN gives 0."""
    from .support.metrics import tonemap
    return torch.round(torch.nan_to_num(tonemap(img), nan=0.0) * 255.0).to(torch.uint8).cpu().numpy()


def write_outputs(output_dir, stem, out, wsum, radius, png=False):
    """``<stem>_rhf.npy``, ``<stem>_rhf_neighbours.npy`` and, with ``png``, their previews; returns the paths written."""
    from .denoise import write_png
    os.makedirs(output_dir, exist_ok=True)
    paths = [os.path.join(output_dir, stem + "_rhf.npy"), os.path.join(output_dir, stem + "_rhf_neighbours.npy")]
    np.save(paths[0], out.cpu().numpy())
    np.save(paths[1], wsum.cpu().numpy())
    if png:
        if out.shape[2] != 3:
            raise ValueError("--png: the preview needs a 3-channel frame (got %d channels)" % out.shape[2])
        paths += [os.path.join(output_dir, stem + "_rhf.png"), os.path.join(output_dir, stem + "_rhf_neighbours.png")]
        write_png(paths[2], frame_preview(out))
        write_png(paths[3], neighbour_preview(wsum, radius))
    return paths


def add_filter_arguments(p, prefix=""):
    """The four parameters of the filter as ``--<prefix>radius`` ... (``denoise``: prefix 'rhf_')."""
    p.add_argument("--%sradius" % prefix, type=int, default=DEFAULTS["radius"],
                   help="half side of the search window, 0..%d (default %d; %s)" % (ops.PBF_MAX_RADIUS, DEFAULTS["radius"], UNTUNED))
    p.add_argument("--%spatch_radius" % prefix, type=int, default=DEFAULTS["patch_radius"],
                   help="half side of the patch the distance is averaged over, 0..%d (default %d; %s)"
                        % (ops.PBF_MAX_PATCH_RADIUS, DEFAULTS["patch_radius"], UNTUNED))
    p.add_argument("--%sbandwidth" % prefix, type=float, default=DEFAULTS["bandwidth"],
                   help="b of the weight exp(-D / b^2) (default %g; %s)" % (DEFAULTS["bandwidth"], UNTUNED))
    p.add_argument("--%seps" % prefix, type=float, default=DEFAULTS["eps"],
                   help="added to the variances under the squared difference of the means (default %g; %s)" % (DEFAULTS["eps"], UNTUNED))
    return p


def check_filter_arguments(radius, patch_radius, bandwidth, eps, flag="--"):
    if not 0 <= radius <= ops.PBF_MAX_RADIUS:
        raise ValueError("%sradius should be in 0..%d, got %d" % (flag, ops.PBF_MAX_RADIUS, radius))
    if not 0 <= patch_radius <= ops.PBF_MAX_PATCH_RADIUS:
        raise ValueError("%spatch_radius should be in 0..%d, got %d" % (flag, ops.PBF_MAX_PATCH_RADIUS, patch_radius))
    if not bandwidth > 0:
        raise ValueError("%sbandwidth should be positive, got %g" % (flag, bandwidth))
    if not eps > 0:
        raise ValueError("%seps should be positive, got %g" % (flag, eps))
    return dict(radius=radius, patch_radius=patch_radius, bandwidth=bandwidth, eps=eps)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m wcmc_amd.rhf",
                                description="Filter a frame by its P-buffer: an RHF-like picture of a learned path manifold.")
    p.add_argument("--image", type=str, required=True, help="(H, W, 3) float frame, .npy")
    p.add_argument("--pbuffer", type=str, required=True,
                   help="(H, W, S, C) P-buffer, .npy, as evaluate --rhf and denoise --save_pbuffer write it")
    p.add_argument("--mask", type=str, default=None, help="optional (H, W) array, .npy: pixels whose element is zero are left alone")
    p.add_argument("--output_dir", type=str, required=True, help="where <stem>_rhf.npy and <stem>_rhf_neighbours.npy go")
    add_filter_arguments(p)
    p.add_argument("--png", action="store_true", help="also write <stem>_rhf.png and <stem>_rhf_neighbours.png")
    p.add_argument("--device_id", type=int, default=0)
    return p


def load_inputs(args):
    """The host arrays of the command line, checked: (image (H, W, 3) fp32, P-buffer (H, W, S, C) fp32, mask (H, W) uint8 or None)."""
    for fn in (args.image, args.pbuffer) + ((args.mask,) if args.mask else ()):
        if not os.path.isfile(fn):
            raise FileNotFoundError(fn)
    img = np.load(args.image)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("--image %s: shape %s is not an (H, W, 3) frame" % (args.image, img.shape))
    pb = np.load(args.pbuffer, mmap_mode="r")
    if pb.ndim != 4 or pb.shape[:2] != img.shape[:2]:
        raise ValueError("--pbuffer %s: shape %s is not (H, W, S, C) with the %d x %d of the image" % ((args.pbuffer, pb.shape) + img.shape[:2]))
    if not 1 <= pb.shape[3] <= ops.PBF_MAX_CHANNELS:
        raise ValueError("--pbuffer %s: %d channels (1..%d are supported)" % (args.pbuffer, pb.shape[3], ops.PBF_MAX_CHANNELS))
    mask = None
    if args.mask:
        mask = np.load(args.mask)
        if mask.shape != img.shape[:2]:
            raise ValueError("--mask %s: shape %s is not the (H, W) = %s of the image" % (args.mask, mask.shape, img.shape[:2]))
        mask = (mask != 0).astype(np.uint8)
    return np.asarray(img, dtype=np.float32), np.array(pb, dtype=np.float32), mask          # (the memory map is read once, here)


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = check_filter_arguments(args.radius, args.patch_radius, args.bandwidth, args.eps)
    img, pb, mask = load_inputs(args)
    device = torch.device("cuda", args.device_id)
    torch.cuda.set_device(device)
    image = torch.from_numpy(img).to(device)
    p_buffer = torch.from_numpy(pb).to(device).permute(2, 3, 0, 1)           # (S, C, H, W), a view of the file's layout
    has_hit = torch.from_numpy(mask).to(device) if mask is not None else None
    out, wsum = rhf_filter(image, p_buffer, has_hit, **kw)
    stem = os.path.splitext(os.path.basename(args.image))[0]
    return write_outputs(args.output_dir, stem, out, wsum, args.radius, png=args.png)


if __name__ == "__main__":
    main()
