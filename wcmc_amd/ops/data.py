"""The data step on the device: preprocessing and patch assembly (csrc/preprocess.hip), the sampling maps (csrc/sampling_map.hip),
the buffers and batches of the sample-based denoisers (csrc/sbmc_data.hip), every sample count of a frame from one pass
(csrc/multi_spp.hip), permutations, the tile stitching of full-frame inference, and the tiles and the closing pass of denoising a
render of any size (csrc/frame_tiles.hip)."""
import ctypes
import math
import numbers

import torch

from .._lib import check, lib
from ._base import _need_cuda, _ptr, _stream


# ---------------------------------------------------------------------------------- data step
def _need_dense(t, ndim):
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != ndim or not t.is_contiguous():
        raise RuntimeError("wcmc_amd preprocessing takes contiguous fp32 CUDA tensors in the reference's numpy "
                           "layout (got %s %s %s); there is no CPU path" % (t.device, t.dtype, tuple(t.shape)))


def preprocess_llpm(sample, max_depth=5, out=None):
    """``DenoiseDataset._preprocess_llpm`` (datasets.py:302-361): raw (h,w,s,C) -> (h,w,s,37).  ``out``: a contiguous (h,w,s,37)
    tensor to write into -- a row slice of a frame's buffer when ``sample`` is a band of its rows (the function is per sample)."""
    _need_dense(sample, 4)
    h, w, s, c = sample.shape
    oc = 7 + 5 * (max_depth + 1)
    if out is None:
        out = torch.empty((h, w, s, oc), device=sample.device, dtype=torch.float32)
    else:
        _need_dense(out, 4)
        if tuple(out.shape) != (h, w, s, oc) or out.device != sample.device:
            raise ValueError("preprocess_llpm: out should be (%d, %d, %d, %d) on %s, got %s on %s"
                             % (h, w, s, oc, sample.device, tuple(out.shape), out.device))
    check(lib().wcmc_preprocess_llpm(_ptr(sample), h * w * s, c, max_depth, _ptr(out), _stream()), "preprocess_llpm")
    return out


def preprocess_kpcn(sample, max_depth=5):
    """``DenoiseDataset._preprocess_kpcn`` (datasets.py:487-582): raw (h,w,s,C) -> (h,w,44)."""
    _need_dense(sample, 4)
    h, w, s, c = sample.shape
    out = torch.empty((h, w, 44), device=sample.device, dtype=torch.float32)
    nbytes = lib().wcmc_preprocess_kpcn_workspace_bytes(h, w)
    ws = torch.empty((nbytes + 3) // 4, device=sample.device, dtype=torch.float32)
    check(lib().wcmc_preprocess_kpcn(_ptr(sample), h, w, s, c, max_depth, _ptr(out), _ptr(ws), ws.numel() * 4, _stream()),
          "preprocess_kpcn")
    return out


def preprocess_kpcn_begin(h, w, device):
    """Start ``preprocess_kpcn`` of an (h, w) frame that arrives in row bands: ``(out (h,w,44), workspace)``, the workspace's maximum
    slot zeroed on the current stream.  Every row then goes through ``preprocess_kpcn_rows`` once, in any partition and order, and
    ``preprocess_kpcn_end`` closes the frame -- bit for bit ``preprocess_kpcn`` of the whole frame.  One stream, or the caller orders."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("preprocess_kpcn_begin: the frame (%d x %d) must be positive" % (h, w))
    out = torch.empty((h, w, 44), device=device, dtype=torch.float32)
    nbytes = lib().wcmc_preprocess_kpcn_workspace_bytes(h, w)
    ws = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
    check(lib().wcmc_preprocess_kpcn_begin(_ptr(ws), ws.numel() * 4, h, w, _stream()), "preprocess_kpcn_begin")
    return out, ws


def _need_kpcn_frame(who, out, ws):
    _need_dense(out, 3)
    if out.shape[2] != 44 or not ws.is_cuda or ws.dtype != torch.float32 or not ws.is_contiguous() or ws.device != out.device:
        raise ValueError("%s: out should be (h, w, 44) and the workspace the fp32 tensor of preprocess_kpcn_begin on its device, got %s "
                         "and %s %s" % (who, tuple(out.shape), ws.dtype, ws.device))


def preprocess_kpcn_rows(band, row0, out, ws, max_depth=5):
    """Pass 1 of ``preprocess_kpcn`` on frame rows ``[row0, row0 + rows)``: ``band`` is their raw samples (rows, w, s, C), ``out`` and
    ``ws`` the frame's, from ``preprocess_kpcn_begin``.  A band that does not start on a 16-byte boundary takes the scalar loads."""
    _need_dense(band, 4)
    _need_kpcn_frame("preprocess_kpcn_rows", out, ws)
    rows, w, s, c = band.shape
    h = out.shape[0]
    if out.shape[1] != w or band.device != out.device:
        raise ValueError("preprocess_kpcn_rows: a band %d pixels wide on %s for a frame %d wide on %s" % (w, band.device, out.shape[1], out.device))
    check(lib().wcmc_preprocess_kpcn_rows(_ptr(band), h, w, int(row0), rows, s, c, max_depth, _ptr(out), _ptr(ws), ws.numel() * 4,
                                          _stream()), "preprocess_kpcn_rows")
    return out


def preprocess_kpcn_end(out, ws, s):
    """Pass 2 of ``preprocess_kpcn`` over the frame whose rows have all been through ``preprocess_kpcn_rows`` at ``s`` samples per
    pixel: depth normalised by the frame's maximum, backward differences.  Returns ``out``, now final."""
    _need_kpcn_frame("preprocess_kpcn_end", out, ws)
    h, w = out.shape[:2]
    check(lib().wcmc_preprocess_kpcn_end(_ptr(out), _ptr(ws), ws.numel() * 4, h, w, int(s), _stream()), "preprocess_kpcn_end")
    return out


def preprocess_kpcn_prefix(raw, s_lo, s_hi, max_depth=5):
    """``_preprocess_kpcn(raw[:, :, :s])`` for every s in s_lo..s_hi from one read of the frame (``wcmc_preprocess_kpcn_prefix``;
    what ``MSDenoiseDataset``, datasets.py:1149-1171, computes once per count): raw (h,w,S,C), 1 <= s_lo <= s_hi <= S <= 64 ->
    (s_hi - s_lo + 1, h, w, 44); slab ``s - s_lo`` is ``preprocess_kpcn(raw[:, :, :s].contiguous())`` up to the order of the sums.
    A view with another storage offset is taken as it is (records that are not 16-byte aligned take the scalar loads)."""
    _need_dense(raw, 4)
    h, w, s, c = raw.shape
    s_lo, s_hi = int(s_lo), int(s_hi)
    if not 1 <= s_lo <= s_hi <= s or s > 64:
        raise ValueError("preprocess_kpcn_prefix: the counts must satisfy 1 <= s_lo <= s_hi <= S <= 64, got %d, %d and S = %d"
                         % (s_lo, s_hi, s))
    n = s_hi - s_lo + 1
    out = torch.empty((n, h, w, 44), device=raw.device, dtype=torch.float32)
    nbytes = lib().wcmc_preprocess_kpcn_prefix_workspace_bytes(h, w, n)
    ws = torch.empty((nbytes + 3) // 4, device=raw.device, dtype=torch.float32)
    check(lib().wcmc_preprocess_kpcn_prefix(_ptr(raw), h, w, s, c, max_depth, s_lo, s_hi, _ptr(out), _ptr(ws), ws.numel() * 4,
                                            _stream()), "preprocess_kpcn_prefix")
    return out


def _check_prefix(who, spp, s_total):
    if not 1 <= int(spp) <= s_total:
        raise ValueError("%s: spp = %d is not a prefix of the %d samples the buffers hold" % (who, spp, s_total))
    return int(spp)


def _aligned_views(shapes, device):
    """``{name: fp32 tensor of shape}`` for the ordered ``shapes``, every entry a view of ONE allocation and starting on a 256-byte
    boundary of it: a consumer on another stream keeps the batch alive with one `record_stream` and frees one block (nine of each
    cost the training thread 0.25 ms per step: scripts/diag_loader_gap.py)."""
    counts = [math.prod(shp) for shp in shapes.values()]
    flat = torch.empty(sum((n + 63) // 64 * 64 for n in counts), device=device, dtype=torch.float32)
    out, off = {}, 0
    for (k, shp), n in zip(shapes.items(), counts):
        out[k] = flat[off:off + n].view(shp)
        off += (n + 63) // 64 * 64
    return out


def _need_origins(who, origins):
    """The (B, 2) window origins as the assembly kernels read them: a contiguous int32 device tensor."""
    if not origins.is_cuda:
        raise RuntimeError("%s: origins must be a device tensor" % who)
    assert origins.dtype == torch.int32 and origins.dim() == 2 and origins.shape[1] == 2 and origins.is_contiguous()


def _need_coords(who, coords):
    """The (B, 6) tile table as the stitch kernels read it: a contiguous int32 device tensor."""
    if not (coords.is_cuda and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 6 and coords.is_contiguous()):
        raise RuntimeError("%s: coords must be a contiguous device int32 (B, 6) tensor" % who)


def check_patch_transforms(transforms, b, who="assemble_kpcn_patches"):
    """Host check of a table of patch transform codes: ``b`` int32 codes in 0..7, one per patch, as a 1-D
    tensor or array.  The codes are data, as origins are: a device tensor is read back here (which synchronises), so a caller that
    assembles many batches from one table checks it once and passes ``check_transforms=False``."""
    import numpy as np
    if isinstance(transforms, torch.Tensor):
        if transforms.dtype != torch.int32:
            raise ValueError("%s: transforms should be int32, got %s" % (who, transforms.dtype))
        t = transforms.detach().cpu().numpy()
    else:
        t = np.asarray(transforms)
        if t.dtype != np.int32:
            raise ValueError("%s: transforms should be int32, got %s" % (who, t.dtype))
    if t.ndim != 1 or t.shape[0] != int(b):
        raise ValueError("%s: transforms should hold one code per patch, shape (%d,), got %s" % (who, int(b), tuple(t.shape)))
    if t.size and (int(t.min()) < 0 or int(t.max()) > 7):
        raise ValueError("%s: a transform code lies outside 0..7 (got %d..%d)" % (who, int(t.min()), int(t.max())))


def _transforms_dev(who, transforms, b, device, check):
    """The (b,) int32 device table the patch kernels read.  ``check=False`` still refuses a wrong dtype or length (no read-back)."""
    if check:
        check_patch_transforms(transforms, b, who)
    if not isinstance(transforms, torch.Tensor):
        import numpy as np
        transforms = torch.from_numpy(np.ascontiguousarray(transforms))
    if transforms.dtype != torch.int32 or transforms.dim() != 1 or transforms.shape[0] != b:
        raise ValueError("%s: transforms should be (%d,) int32, got %s %s" % (who, b, tuple(transforms.shape), transforms.dtype))
    return transforms.to(device).contiguous()


def _kpcn_batch_shapes(b, s, patch, targets):
    """Entries of a KPCN batch of ``b`` windows (patches with ``targets``, tiles without); ``s``: llpm's samples, None without llpm."""
    cin = 34 if s is None else 35
    shapes = {"kpcn_diffuse_in": (b, cin, patch, patch), "kpcn_specular_in": (b, cin, patch, patch),
              "kpcn_diffuse_buffer": (b, 3, patch, patch), "kpcn_specular_buffer": (b, 3, patch, patch),
              "kpcn_albedo": (b, 3, patch, patch)}
    if targets:
        shapes.update({k: (b, 3, patch, patch) for k in ("target_diffuse", "target_specular", "target_total")})
    if s is not None:
        shapes["paths"] = (b, s, 36, patch, patch)
    return shapes


def assemble_kpcn_patches(kpcn, llpm, gt, origins, patch, spp=None, transforms=None, check_transforms=True):
    """The batch dictionary of the KPCN base model for windows of `patch` pixels at `origins` ((B, 2) int32 device
    tensor of (row, column)) of one image's preprocessed buffers (datasets.py:1026-1146 on the device;
    ``wcmc_assemble_kpcn_patches``).  ``spp``: the batch takes the first ``spp`` of llpm's samples (``kpcn`` is then that count's
    buffer); None: all.  ``transforms``: None, or one dihedral code 0..7 per patch ((B,) int32 tensor or array;
    DESIGN.md section 20): entry b is ``rot90(fliplr(w) if t & 4 else w, t & 3)`` of its window w as if the whole frame had been
    transformed before preprocessing -- per-pixel channels copied, the backward differences retaken along the new axes."""
    _need_cuda(kpcn, gt)
    _need_origins("assemble_kpcn_patches", origins)
    h, w = kpcn.shape[:2]
    assert kpcn.shape == (h, w, 44) and gt.shape == (h, w, 9) and kpcn.is_contiguous() and gt.is_contiguous()
    b, s = origins.shape[0], 0
    if llpm is not None:
        assert llpm.shape[:2] == (h, w) and llpm.shape[3] == 37 and llpm.is_contiguous()
        s = llpm.shape[2]
    s_total = s
    if spp is not None and llpm is not None:
        s = _check_prefix("assemble_kpcn_patches", spp, s_total)
    out = _aligned_views(_kpcn_batch_shapes(b, s if llpm is not None else None, patch, targets=True), kpcn.device)
    tr = None if transforms is None else _transforms_dev("assemble_kpcn_patches", transforms, b, kpcn.device, check_transforms)
    # (without llpm nothing in the batch depends on the sample counts: 0, 0)
    check(lib().wcmc_assemble_kpcn_patches(_ptr(kpcn), _ptr(llpm), _ptr(gt), ctypes.c_void_p(origins.data_ptr()), _ptr(tr), b, h, w,
                                           s_total, s, patch, _ptr(out["kpcn_diffuse_in"]), _ptr(out["kpcn_specular_in"]),
                                           _ptr(out["kpcn_diffuse_buffer"]), _ptr(out["kpcn_specular_buffer"]),
                                           _ptr(out["kpcn_albedo"]), _ptr(out.get("paths")), _ptr(out["target_diffuse"]),
                                           _ptr(out["target_specular"]), _ptr(out["target_total"]), _stream()),
          "assemble_kpcn_patches")
    return out


def preprocess_sbmc(sample, max_depth=5, tiled=None, out_s=None, out_p=None):
    """``DenoiseDataset._preprocess_sbmc`` (datasets.py:363-485): sanitised raw (h,w,s,C) -> (sbmc_s (h,w,s,27), sbmc_p (h,w,s,66)).
    ``tiled``: None lets the library pick the form, False / True force the one-thread-per-element / the LDS-staged form (which
    refuses records that are not 16-byte aligned); the two are bit-identical.  ``out_s`` / ``out_p``: contiguous tensors of those
    shapes to write into -- row slices of a frame's buffers when ``sample`` is a band of its rows (the function is per sample)."""
    _need_dense(sample, 4)
    h, w, s, c = sample.shape
    pc = 11 * (max_depth + 1)
    for name, t, oc in (("out_s", out_s, 27), ("out_p", out_p, pc)):
        if t is not None:
            _need_dense(t, 4)
            if tuple(t.shape) != (h, w, s, oc) or t.device != sample.device:
                raise ValueError("preprocess_sbmc: %s should be (%d, %d, %d, %d) on %s, got %s on %s"
                                 % (name, h, w, s, oc, sample.device, tuple(t.shape), t.device))
    if out_s is None:
        out_s = torch.empty((h, w, s, 27), device=sample.device, dtype=torch.float32)
    if out_p is None:
        out_p = torch.empty((h, w, s, pc), device=sample.device, dtype=torch.float32)
    check(lib().wcmc_preprocess_sbmc(_ptr(sample), h * w * s, c, max_depth, _ptr(out_s), _ptr(out_p),
                                     -1 if tiled is None else int(bool(tiled)), _stream()), "preprocess_sbmc")
    return out_s, out_p


def check_patch_origins(origins, h, w, patch, who="assemble_sample_patches"):
    """Host check of (B, 2) window origins (rows, columns): every ``patch``-pixel window lies inside the h x w image."""
    import numpy as np
    o = origins.cpu().numpy() if isinstance(origins, torch.Tensor) else np.asarray(origins)
    if o.size and (int(o[:, 0].max()) + patch > h or int(o[:, 1].max()) + patch > w or int(o.min()) < 0):
        raise ValueError("%s: a %d-pixel patch origin lies outside the %dx%d image" % (who, patch, h, w))


def sample_feature_size(use_g_buf=True, use_sbmc_buf=True, use_llpm_buf=False):
    """Channels of the ``features`` entry of a sample-based batch (datasets.py:1058-1073, 1094-1098): 90 / 24 / 69 / 3, + 1."""
    return (24 if use_g_buf else 3) + (66 if use_sbmc_buf else 0) + (1 if use_llpm_buf else 0)


def _check_sample_buffers(who, sbmc_p, llpm, h, w, s):
    """The optional per-sample buffers beside an (h, w, s, 27) ``sbmc_s``: each is None or a contiguous fp32 device tensor of its
    own channel count over the same pixels and samples."""
    for name, t, c in (("sbmc_p", sbmc_p, 66), ("llpm", llpm, 37)):
        if t is not None and (tuple(t.shape) != (h, w, s, c) or not t.is_contiguous() or t.dtype != torch.float32 or not t.is_cuda):
            raise ValueError("%s: %s should be a contiguous fp32 (%d, %d, %d, %d) device tensor, got %s"
                             % (who, name, h, w, s, c, tuple(t.shape)))


def _sample_batch_shapes(b, s, patch, use_g_buf, use_sbmc_buf, use_llpm_buf, target):
    """Entries of a sample-based batch of ``b`` windows at ``s`` samples (patches with the ``target`` image, tiles without)."""
    f = sample_feature_size(use_g_buf, use_sbmc_buf, use_llpm_buf)
    shapes = {"radiance": (b, s, 3, patch, patch), "features": (b, s, f, patch, patch)}
    if use_llpm_buf:
        shapes["paths"] = (b, s, 36, patch, patch)
    if target:
        shapes["target_image"] = (b, 3, patch, patch)
    return shapes


def assemble_sample_patches(sbmc_s, sbmc_p, llpm, gt, origins, patch, use_g_buf=True, use_sbmc_buf=True, check_origins=True,
                            spp=None, transforms=None):
    """The batch dictionary of the SBMC / LBMC interfaces (``radiance``, ``features``, ``paths`` as (B, S, C, P, P) and
    ``target_image``) for windows of ``patch`` pixels at ``origins`` ((B, 2) int32 (row, column); numpy or tensor) of one image's
    buffers (datasets.py:1045-1073, 1086-1118 and ``_transpose`` on the device, one launch: ``wcmc_assemble_sample_patches``).
    ``sbmc_p`` may be None without ``use_sbmc_buf``; ``llpm`` None leaves ``paths`` and the path weight out.
    ``check_origins=False``: the caller has checked them on the host (checking a device tensor here synchronises).  ``spp``: the
    batch takes the first ``spp`` samples of the buffers (they are per-sample, so the prefix is a slice); None: all of them.
    ``transforms``: None, or one dihedral code 0..7 per patch ((B,) int32 tensor or array;
    DESIGN.md section 20): every entry of patch b is ``rot90(fliplr(w) if t & 4 else w, t & 3)`` of its window w on the two pixel
    axes -- all channels are per sample, so all are copies (subpixel and light directions included: not re-expressed).  The table is
    checked on the host together with the origins (``check_origins``)."""
    _need_cuda(sbmc_s, gt)
    h, w, s = sbmc_s.shape[:3]
    if tuple(sbmc_s.shape) != (h, w, s, 27) or tuple(gt.shape) != (h, w, 9) or not (sbmc_s.is_contiguous() and gt.is_contiguous()):
        raise ValueError("assemble_sample_patches: sbmc_s should be contiguous (H, W, S, 27) and gt (H, W, 9), got %s and %s"
                         % (tuple(sbmc_s.shape), tuple(gt.shape)))
    if use_sbmc_buf:
        _need_cuda(sbmc_p)
    _check_sample_buffers("assemble_sample_patches", sbmc_p if use_sbmc_buf else None, llpm, h, w, s)
    if patch < 1 or patch > h or patch > w:
        raise ValueError("assemble_sample_patches: a %d-pixel patch does not fit the %dx%d image" % (patch, h, w))
    if check_origins:
        check_patch_origins(origins, h, w, patch)
    if not isinstance(origins, torch.Tensor):
        import numpy as np
        origins = torch.as_tensor(np.asarray(origins), dtype=torch.int32)
    origins = origins.to(sbmc_s.device, torch.int32).contiguous()
    assert origins.dim() == 2 and origins.shape[1] == 2
    b = origins.shape[0]
    s_total = s
    if spp is not None:
        s = _check_prefix("assemble_sample_patches", spp, s_total)
    out = _aligned_views(_sample_batch_shapes(b, s, patch, use_g_buf, use_sbmc_buf, llpm is not None, target=True), sbmc_s.device)
    tr = None if transforms is None else _transforms_dev("assemble_sample_patches", transforms, b, sbmc_s.device, check_origins)
    check(lib().wcmc_assemble_sample_patches(_ptr(sbmc_s), _ptr(sbmc_p if use_sbmc_buf else None), _ptr(llpm), _ptr(gt),
                                             ctypes.c_void_p(origins.data_ptr()), _ptr(tr), b, h, w, s_total, s, patch,
                                             int(bool(use_g_buf)), int(bool(use_sbmc_buf)), _ptr(out["radiance"]),
                                             _ptr(out["features"]), _ptr(out.get("paths")), _ptr(out["target_image"]), _stream()),
          "assemble_sample_patches")
    return out


def gradients(buf):
    """``DenoiseDataset._gradients`` (datasets.py:286-300): (h,w,c) -> (h,w,2c)."""
    _need_dense(buf, 3)
    h, w, c = buf.shape
    out = torch.empty((h, w, 2 * c), device=buf.device, dtype=torch.float32)
    check(lib().wcmc_gradients(_ptr(buf), h, w, c, _ptr(out), _stream()), "gradients")
    return out


def reflect_index(i, n):
    """Source index of position ``i`` of a line of ``n`` entries under scipy's 'reflect' boundary (``wcmc_reflect_index``: the
    map the Gaussian passes of ``importance_map`` use; no GPU call)."""
    return int(lib().wcmc_reflect_index(int(i), int(n)))


def importance_map(img):
    """``gradient_importance_map`` (datasets.py:17-36): (H, W) or (H, W, 3) -> (H, W) in [0, 1]."""
    if img.dim() == 2:
        h, w, c = img.shape[0], img.shape[1], 1
    elif img.dim() == 3 and img.shape[2] in (1, 3):
        h, w, c = img.shape
    else:
        raise ValueError("importance_map: the image should be (H, W) or (H, W, 3), got %s" % (tuple(img.shape),))
    _need_dense(img, img.dim())
    out = torch.empty((h, w), device=img.device, dtype=torch.float32)
    nbytes = lib().wcmc_importance_map_workspace_bytes(h, w, c)
    ws = torch.empty((nbytes + 3) // 4, device=img.device, dtype=torch.float32)
    check(lib().wcmc_importance_map(_ptr(img), h, w, c, _ptr(out), _ptr(ws), ws.numel() * 4, _stream()), "importance_map")
    return out


def sampling_prob(raw, gt, patch_size=128, max_depth=5):
    """The patch-sampling map of ``_offline_preprocess`` (datasets.py:697-715): sanitised raw (H, W, S, 104) and gt (H, W, 9)
    -> (H - patch_size, W - patch_size), a distribution over patch origins."""
    _need_dense(raw, 4)
    _need_dense(gt, 3)
    h, w, s, c = raw.shape
    if tuple(gt.shape) != (h, w, 9):
        raise ValueError("sampling_prob: gt should be (%d, %d, 9), got %s" % (h, w, tuple(gt.shape)))
    if h <= patch_size or w <= patch_size:
        raise ValueError("sampling_prob: the image (%d x %d) must be larger than the patch (%d) in both dimensions"
                         % (h, w, patch_size))
    out = torch.empty((h - patch_size, w - patch_size), device=raw.device, dtype=torch.float32)
    nbytes = lib().wcmc_sampling_prob_workspace_bytes(h, w, patch_size)
    ws = torch.empty((nbytes + 7) // 8, device=raw.device, dtype=torch.float64)
    check(lib().wcmc_sampling_prob(_ptr(raw), _ptr(gt), h, w, s, c, max_depth, patch_size, _ptr(out), _ptr(ws), ws.numel() * 8,
                                   _stream()), "sampling_prob")
    return out


def sanitize_(x):
    """NaN / Inf / >= 1e38 -> 1e38 in place (datasets.py:623-624)."""
    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("sanitize_ takes a contiguous fp32 CUDA tensor (got %s %s); there is no CPU path" % (x.device, x.dtype))
    check(lib().wcmc_sanitize(_ptr(x), x.numel(), _stream()), "sanitize")
    return x


def random_permutation(n, device, out=None, seed=None):
    """A pseudo-random permutation of range(n) as an int64 device tensor, without the sort behind
    ``torch.randperm(n, device=...)`` (``wcmc_random_permutation``: keyed Feistel network).  The 62-bit key is drawn
    from torch's default CPU generator, so ``torch.manual_seed`` fixes the sequence of permutations."""
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=device)
    assert out.is_cuda and out.dtype == torch.int64 and out.numel() == n and out.is_contiguous()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    check(lib().wcmc_random_permutation(_ptr(out), n, int(seed), _stream()), "random_permutation")
    return out


def random_permutation_dev(out, state, slot):
    """``random_permutation`` keyed from the device tensor ``state`` = [seed, step counter] (int64) and ``slot``: the form a hipGraph
    can replay with another key every step (``wcmc_random_permutation_dev``)."""
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and state.is_cuda and state.dtype == torch.int64 and state.numel() >= 2
    check(lib().wcmc_random_permutation_dev(_ptr(out), out.numel(), _ptr(state), int(slot), _stream()), "random_permutation_dev")
    return out


def step_counter_advance(state):
    """state[1] += 1 on the device (``wcmc_step_counter_advance``)."""
    check(lib().wcmc_step_counter_advance(_ptr(state), _stream()), "step_counter_advance")


def permutation_key(seed, counter, slot):
    """Host mirror of the key ``random_permutation_dev`` forms (``wcmc_permutation_key``; no GPU call)."""
    return int(lib().wcmc_permutation_key(int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), int(slot)))


def check_tile_coords(coords, h, w, patch):
    """Host check of a (B, 6) tile table (i_start, j_start, i_end, j_end, i, j) before it goes to ``stitch_tiles``: every owned
    window lies inside the frame and inside its tile."""
    for i0, j0, i1, j1, i, j in coords:
        if not (0 <= i0 < i1 <= h and 0 <= j0 < j1 <= w and i <= i0 and j <= j0 and i1 <= i + patch and j1 <= j + patch):
            raise ValueError("stitch_tiles: tile %s does not fit a %d x %d frame of %d-pixel tiles"
                             % ((i0, j0, i1, j1, i, j), h, w, patch))


def stitch_tiles(out, p_buffers, coords, out_rad, out_path=None, patch=128):
    """Paste one batch of tiles into the full frame (``wcmc_stitch_tiles``; the slice loop of test_models.py:75-89).
    out: (B, 3, ho, wo) network output ('replicate'-padded back to ``patch`` on the fly when smaller); p_buffers: None, a
    (B, S, C, patch, patch) tensor or a dict of them; coords: device int32 (B, 6) table whose rows passed
    ``check_tile_coords``; out_rad (3, H, W) and out_path ((S, C, H, W), or a dict of them keyed like p_buffers) are written
    in place.  Bit-identical to the slice copies."""
    _need_cuda(out, out_rad)
    _need_coords("stitch_tiles", coords)
    b, c3, ho, wo = out.shape
    _, h, w = out_rad.shape
    assert c3 == 3 and coords.shape[0] == b and out_rad.shape[0] == 3 and out_rad.is_contiguous()
    pairs = []
    if p_buffers is not None:
        if isinstance(p_buffers, dict):
            pairs = [(p_buffers[k], out_path[k]) for k in p_buffers]
        else:
            pairs = [(p_buffers, out_path)]
    for pb, op in pairs:
        _need_cuda(pb, op)
        assert pb.dim() == 5 and pb.shape[0] == b and tuple(pb.shape[3:]) == (patch, patch) and pb.is_contiguous()
        assert tuple(op.shape) == (pb.shape[1], pb.shape[2], h, w) and op.is_contiguous()
    # two P-buffers of one shape per launch; anything else in further launches (the radiance is re-copied: same values)
    groups = [pairs[i:i + 2] for i in range(0, len(pairs), 2)] or [[]]
    if len(pairs) == 2 and pairs[0][0].shape != pairs[1][0].shape:
        groups = [[pairs[0]], [pairs[1]]]
    for g in groups:
        pa, oa = g[0] if len(g) > 0 else (None, None)
        pbb, ob = g[1] if len(g) > 1 else (None, None)
        s, c = (pa.shape[1], pa.shape[2]) if pa is not None else (0, 0)
        check(lib().wcmc_stitch_tiles(_ptr(out), *out.stride(), ho, wo, _ptr(pa), _ptr(pbb), s, c, patch,
                                      ctypes.c_void_p(coords.data_ptr()), b, h, w, _ptr(out_rad), _ptr(oa), _ptr(ob),
                                      _stream()), "stitch_tiles")
    return out_rad, out_path


# ---------------------------------------------------------------------------------- denoising a render (csrc/frame_tiles.hip)
def check_tile_origins(origins, h, w, patch, pad, who="assemble_kpcn_tiles"):
    """Host check of (B, 2) tile origins (rows, columns) in frame coordinates: every ``patch``-pixel tile lies inside the h x w
    frame extended by ``pad`` pixels on every side, ``-pad <= o <= dim + pad - patch``."""
    import numpy as np
    o = origins.cpu().numpy() if isinstance(origins, torch.Tensor) else np.asarray(origins)
    if o.size and (int(o.min()) < -pad or int(o[:, 0].max()) > h + pad - patch or int(o[:, 1].max()) > w + pad - patch):
        raise ValueError("%s: a %d-pixel tile origin lies outside the %dx%d frame extended by %d" % (who, patch, h, w, pad))


def check_frame_transforms(codes):
    """Host check of a self-ensemble set: distinct dihedral codes in 0..7 that contain 0 (the identity pass
    gives the P-buffers).  Returns them as a sorted tuple, the order the passes are summed in."""
    try:
        codes = [c for c in codes]
    except TypeError:
        raise ValueError("check_frame_transforms: the ensemble should be a sequence of codes 0..7, got %r" % (codes,))
    for c in codes:
        if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 0 <= int(c) <= 7:
            raise ValueError("check_frame_transforms: code %r lies outside 0..7" % (c,))
    codes = [int(c) for c in codes]
    if len(set(codes)) != len(codes):
        raise ValueError("check_frame_transforms: a code is repeated in %s" % (codes,))
    if 0 not in codes:
        raise ValueError("check_frame_transforms: the set %s does not contain 0 (the identity pass gives the P-buffers)" % (codes,))
    return tuple(sorted(codes))


def _frame_transform(who, transform):
    """One whole-frame code: None is 0, the frame as it is."""
    if transform is None:
        return 0
    if isinstance(transform, bool) or not isinstance(transform, numbers.Integral) or not 0 <= int(transform) <= 7:
        raise ValueError("%s: the transform code %r lies outside 0..7" % (who, transform))
    return int(transform)


def stitch_tiles_aug(out, coords, out_rad, transform, accumulate, patch=128):
    """The way back of the self-ensemble (``wcmc_stitch_tiles_aug``): paste (``accumulate`` False) or add (True) one batch of tiles
    of the frame transformed by code ``transform`` into ``out_rad`` (3, H, W), which stays in SOURCE orientation.  out: (B, 3, ho, wo)
    network output, 'replicate'-padded back to ``patch`` on the fly as ``stitch_tiles`` does it; coords: device int32 (B, 6) rows of
    the TRANSFORMED frame's table, which passed ``check_tile_coords`` against the transformed sizes.  No P-buffers."""
    _need_cuda(out, out_rad)
    t = _frame_transform("stitch_tiles_aug", transform)
    _need_coords("stitch_tiles_aug", coords)
    b, c3, ho, wo = out.shape
    _, h, w = out_rad.shape
    assert c3 == 3 and coords.shape[0] == b and out_rad.shape[0] == 3 and out_rad.is_contiguous() and out_rad.dtype == torch.float32
    check(lib().wcmc_stitch_tiles_aug(_ptr(out), *out.stride(), ho, wo, patch, ctypes.c_void_p(coords.data_ptr()), b, t, h, w,
                                      int(bool(accumulate)), _ptr(out_rad), _stream()), "stitch_tiles_aug")
    return out_rad


def stitch_tiles_blend(out, coords, acc, wsum, blend, transform=0, patch=128, pad=None):
    """The feathered stitch (``wcmc_stitch_tiles_blend``): every tile of the batch adds ``w * v`` to ``acc``
    (3, H, W) and ``w`` to ``wsum`` (H, W), both fp32, contiguous, in SOURCE orientation and zero before the first batch of a pass, on
    its owned window widened by ``blend`` pixels; ``w`` ramps from 0 to 1 over the ``2 * blend`` pixels around every seam.  out:
    (B, 3, ho, wo) network output, read as ``stitch_tiles`` reads it; coords: device int32 (B, 6) rows of the table of the frame
    transformed by code ``transform``, which passed ``check_tile_coords``.  The tiles are added in table order by the one thread that
    owns the pixel: the sums do not depend on how the table is cut into batches.  ``pad``: the table's pad; with it the library also
    refuses a ``blend`` above ``(patch - 2 * pad) / 2`` or one that gives weight to a replicated pixel.  No P-buffers."""
    _need_cuda(out, acc, wsum)
    t = _frame_transform("stitch_tiles_blend", transform)
    _need_coords("stitch_tiles_blend", coords)
    if isinstance(blend, bool) or not isinstance(blend, numbers.Integral):
        raise ValueError("stitch_tiles_blend: the feather half-width should be an integer, got %r" % (blend,))
    b, c3, ho, wo = out.shape
    _, h, w = acc.shape
    assert c3 == 3 and coords.shape[0] == b and out.dtype == torch.float32
    assert acc.shape[0] == 3 and acc.is_contiguous() and acc.dtype == torch.float32
    assert tuple(wsum.shape) == (h, w) and wsum.is_contiguous() and wsum.dtype == torch.float32
    check(lib().wcmc_stitch_tiles_blend(_ptr(out), *out.stride(), ho, wo, patch, -1 if pad is None else int(pad),
                                        ctypes.c_void_p(coords.data_ptr()), b, t, h, w, int(blend), _ptr(acc), _ptr(wsum), _stream()),
          "stitch_tiles_blend")
    return acc, wsum


def blend_finish(acc, wsum, out_rad, accumulate=False):
    """``out_rad`` (3, H, W) = ``acc / wsum`` or, with ``accumulate``, ``out_rad + acc / wsum`` (``wcmc_blend_finish``): the pass of one
    transform code, normalised by its own weight sum.  Returns out_rad."""
    _need_cuda(acc, wsum, out_rad)
    _, h, w = acc.shape
    for x, shape in ((acc, (3, h, w)), (wsum, (h, w)), (out_rad, (3, h, w))):
        assert tuple(x.shape) == shape and x.is_contiguous() and x.dtype == torch.float32
    check(lib().wcmc_blend_finish(_ptr(acc), _ptr(wsum), h, w, int(bool(accumulate)), _ptr(out_rad), _stream()), "blend_finish")
    return out_rad


def assemble_kpcn_tiles(kpcn, llpm, origins, patch=128, pad=32, check_origins=True, transform=0):
    """The inference batch of the KPCN base model -- ``assemble_kpcn_patches`` without ``gt`` and without the ``target_*`` entries --
    for tiles of ``patch`` pixels at ``origins`` ((B, 2) int32 device tensor of (row, column) in frame coordinates, from ``-pad``
    upward) of the frame extended by ``pad`` pixels by mirror reflection with the edge repeated (``wcmc_assemble_kpcn_tiles``; bit
    for bit the batch of the ``np.pad(raw, pad, 'symmetric')`` frame at ``origins + pad``, which is never built).  The origins are
    data and are checked on the host (``check_tile_origins``); ``check_origins=False``: the caller has checked the table once
    (checking a device tensor here synchronises).

    ``transform``: a dihedral code 1..7 assembles the tiles of the frame as if the RAW frame had been transformed by ``T_t`` before
    preprocessing: ``origins`` are then in the transformed frame's coordinates and are checked against its
    sizes (W x H for odd codes).  0 or None is the frame as it is."""
    _need_cuda(kpcn)
    _need_origins("assemble_kpcn_tiles", origins)
    h, w = kpcn.shape[:2]
    assert kpcn.shape == (h, w, 44) and kpcn.is_contiguous()
    t = _frame_transform("assemble_kpcn_tiles", transform)
    if check_origins:
        check_tile_origins(origins, *((w, h) if t & 1 else (h, w)), patch, pad)
    b, s = origins.shape[0], 0
    if llpm is not None:
        _need_cuda(llpm)
        assert llpm.shape[:2] == (h, w) and llpm.shape[3] == 37 and llpm.is_contiguous()
        s = llpm.shape[2]
    out = _aligned_views(_kpcn_batch_shapes(b, s if llpm is not None else None, patch, targets=False), kpcn.device)
    check(lib().wcmc_assemble_kpcn_tiles(_ptr(kpcn), _ptr(llpm), ctypes.c_void_p(origins.data_ptr()), b, h, w, s, patch, pad, t,
                                         _ptr(out["kpcn_diffuse_in"]), _ptr(out["kpcn_specular_in"]),
                                         _ptr(out["kpcn_diffuse_buffer"]), _ptr(out["kpcn_specular_buffer"]),
                                         _ptr(out["kpcn_albedo"]), _ptr(out.get("paths")), _stream()), "assemble_kpcn_tiles")
    return out


def finish_frame(out_rad, kpcn, llpm, preview=False):
    """The closing pass of denoising a frame (``wcmc_finish_frame``): out_rad (3, H, W) stitched radiance, kpcn (H, W, 44),
    llpm (H, W, S, 37) -> ``(out, ipt, has_hit)``: the noisy input ``ipt`` (H, W, 3) (datasets.py:1234), ``has_hit`` (H, W) fp32 0 / 1
    (descriptor 24 nonzero in the mean over the S samples, datasets.py:1407-1414) and the composite ``out`` (H, W, 3) = the network's
    output where a surface was hit, the input elsewhere (test_models.py:231-232).  ``preview=True`` adds ``(preview_out,
    preview_ipt)``, the (H, W, 3) uint8 images round(255 * tonemap(.)) (test_models.py:24-34, gamma 1/2.2)."""
    _need_cuda(out_rad, kpcn, llpm)
    h, w = kpcn.shape[:2]
    if (tuple(out_rad.shape) != (3, h, w) or tuple(kpcn.shape) != (h, w, 44) or llpm.dim() != 4 or tuple(llpm.shape[:2]) != (h, w)
            or llpm.shape[3] != 37 or llpm.shape[2] < 1 or not (out_rad.is_contiguous() and kpcn.is_contiguous() and llpm.is_contiguous())):
        raise ValueError("finish_frame: out_rad should be contiguous (3, H, W), kpcn (H, W, 44) and llpm (H, W, S, 37), got %s, %s, %s"
                         % (tuple(out_rad.shape), tuple(kpcn.shape), tuple(llpm.shape)))
    return _finish(lib().wcmc_finish_frame, "finish_frame", out_rad, kpcn, llpm, preview)


def _finish(symbol, who, out_rad, src, llpm, preview):
    """The closing pass of either family: ``symbol`` reads the noisy input from ``src`` (H, W, ...), whose shapes ``who`` has checked."""
    h, w = src.shape[:2]
    dev = src.device
    out = torch.empty((h, w, 3), device=dev, dtype=torch.float32)
    ipt = torch.empty((h, w, 3), device=dev, dtype=torch.float32)
    has_hit = torch.empty((h, w), device=dev, dtype=torch.float32)
    pv = [torch.empty((h, w, 3), device=dev, dtype=torch.uint8) for _ in range(2)] if preview else [None, None]
    check(symbol(_ptr(out_rad), _ptr(src), _ptr(llpm), h, w, llpm.shape[2], _ptr(out), _ptr(ipt), _ptr(has_hit), _ptr(pv[0]),
                 _ptr(pv[1]), _stream()), who)
    return (out, ipt, has_hit, pv[0], pv[1]) if preview else (out, ipt, has_hit)


# ---------------------------------------------------------------------------------- ... with a sample-based model (csrc/sbmc_data.hip)
def assemble_sample_tiles(sbmc_s, sbmc_p, llpm, origins, patch=128, pad=32, use_g_buf=True, use_sbmc_buf=True, check_origins=True,
                          transform=0):
    """The inference batch of the SBMC / LBMC interfaces -- ``assemble_sample_patches`` without ``gt`` and without ``target_image`` --
    for tiles of ``patch`` pixels at ``origins`` ((B, 2) int32 device tensor of (row, column) in frame coordinates, from ``-pad``
    upward) of the frame extended by ``pad`` pixels by mirror reflection with the edge repeated (``wcmc_assemble_sample_tiles``; bit
    for bit the ``radiance`` / ``features`` / ``paths`` of the ``np.pad(raw, pad, 'symmetric')`` frame at ``origins + pad``, which is
    never built).  ``sbmc_p`` may be None without ``use_sbmc_buf``; ``llpm`` None leaves ``paths`` and the path weight out.  The
    origins are data and are checked on the host (``check_tile_origins``); ``check_origins=False``: the caller has checked the
    table once (checking a device tensor here synchronises).  ``transform``: as ``assemble_kpcn_tiles``'s -- a code 1..7 reads the
    frame through ``T_t``, the origins being those of the transformed frame; every channel is a copy."""
    t = _frame_transform("assemble_sample_tiles", transform)
    _need_cuda(sbmc_s)
    _need_origins("assemble_sample_tiles", origins)
    if sbmc_s.dim() != 4 or sbmc_s.shape[3] != 27 or sbmc_s.shape[2] < 1 or not sbmc_s.is_contiguous():
        raise ValueError("assemble_sample_tiles: sbmc_s should be contiguous (H, W, S, 27), got %s" % (tuple(sbmc_s.shape),))
    h, w, s = sbmc_s.shape[:3]
    _check_sample_buffers("assemble_sample_tiles", sbmc_p if use_sbmc_buf else None, llpm, h, w, s)
    if use_sbmc_buf and sbmc_p is None:
        raise ValueError("assemble_sample_tiles: use_sbmc_buf needs sbmc_p")
    if check_origins:
        check_tile_origins(origins, *((w, h) if t & 1 else (h, w)), patch, pad, who="assemble_sample_tiles")
    b = origins.shape[0]
    out = _aligned_views(_sample_batch_shapes(b, s, patch, use_g_buf, use_sbmc_buf, llpm is not None, target=False), sbmc_s.device)
    check(lib().wcmc_assemble_sample_tiles(_ptr(sbmc_s), _ptr(sbmc_p if use_sbmc_buf else None), _ptr(llpm),
                                           ctypes.c_void_p(origins.data_ptr()), b, h, w, s, patch, pad, t, int(bool(use_g_buf)),
                                           int(bool(use_sbmc_buf)), _ptr(out["radiance"]), _ptr(out["features"]),
                                           _ptr(out.get("paths")), _stream()), "assemble_sample_tiles")
    return out


def finish_sample_frame(out_rad, sbmc_s, llpm, preview=False):
    """``finish_frame`` for the sample-based models (``wcmc_finish_sample_frame``): out_rad (3, H, W) stitched radiance, sbmc_s
    (H, W, S, 27), llpm (H, W, S, 37) -> ``(out, ipt, has_hit)`` with the noisy input ``ipt`` (H, W, 3) the mean over the samples of
    ``sbmc_s[..., 0:3]`` (datasets.py:1248; summed in sample order), ``has_hit`` and the composite as ``finish_frame``'s;
    ``preview=True`` adds the two (H, W, 3) uint8 previews."""
    _need_cuda(out_rad, sbmc_s, llpm)
    h, w = sbmc_s.shape[:2]
    if (tuple(out_rad.shape) != (3, h, w) or sbmc_s.dim() != 4 or sbmc_s.shape[3] != 27 or sbmc_s.shape[2] < 1
            or tuple(llpm.shape) != (h, w, sbmc_s.shape[2], 37)
            or not (out_rad.is_contiguous() and sbmc_s.is_contiguous() and llpm.is_contiguous())):
        raise ValueError("finish_sample_frame: out_rad should be contiguous (3, H, W), sbmc_s (H, W, S, 27) and llpm (H, W, S, 37), "
                         "got %s, %s, %s" % (tuple(out_rad.shape), tuple(sbmc_s.shape), tuple(llpm.shape)))
    return _finish(lib().wcmc_finish_sample_frame, "finish_sample_frame", out_rad, sbmc_s, llpm, preview)
