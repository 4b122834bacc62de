"""Tiled full-image inference: the step after the path.

Mirrors, on device tensors, what the reference does around ``validate_batch``:
  * ``FullImageDataset`` tiling  ``support/datasets.py:1276-1299``  overlapping ``patch_size`` tiles at stride
    ``patch_size - 2*pad_size``; each tile owns its interior, tiles on the image border own their border too;
  * ``inference``                ``test_models.py:49-101``          replicate-pad the network output back to the
    tile size, paste each tile's owned window into the full image (radiance and P-buffers);
  * valid crop + has-hit composite ``test_models.py:217-232``       drop the outer (128 - 72) / 2 pixels and keep
    the noisy input where no surface was hit.
``test_models.py`` is not importable as shipped (``from train_kpcn import weights_init`` does not exist there), so
these are restatements checked by known-answer tests, not by a golden (parity unpinned).
"""
import torch
import torch.nn.functional as F


def tile_coords(h, w, patch_size=128, pad_size=32):
    """[(i_start, j_start, i_end, j_end, i, j)] as ``FullImageDataset`` builds them (datasets.py:1276-1294)."""
    stride = patch_size - 2 * pad_size
    assert (h - 2 * pad_size) % stride == 0 and (w - 2 * pad_size) % stride == 0
    coords = []
    for i in range(0, h - 2 * pad_size, stride):
        for j in range(0, w - 2 * pad_size, stride):
            i_start, j_start = i + pad_size, j + pad_size
            i_end, j_end = i + patch_size - pad_size, j + patch_size - pad_size
            if i == 0:
                i_start = 0
            if j == 0:
                j_start = 0
            if i == h - patch_size:
                i_end = i + patch_size
            if j == w - patch_size:
                j_end = j + patch_size
            coords.append((i_start, j_start, i_end, j_end, i, j))
    return coords


def inference(interface, dataloader, h, w, patch_size=128, use_llpm_buf=True, device=None):
    """``test_models.inference``: ``dataloader`` yields ``(batch, i_start, j_start, i_end, j_end, i, j)`` with a
    dict of (B, ...) tensors and per-item integer sequences.  Returns ``(out_rad (3,H,W), out_path)`` on the device
    (the reference additionally moves them to numpy HWC)."""
    interface.to_eval_mode()
    out_rad, out_path = None, None
    with torch.no_grad():
        for batch, i_start, j_start, i_end, j_end, i, j in dataloader:
            for k in batch:
                if isinstance(batch[k], torch.Tensor) and device is not None:
                    batch[k] = batch[k].to(device)
            out, p_buffers = interface.validate_batch(batch)
            if out_rad is None:
                out_rad = torch.zeros((3, h, w), device=out.device)
            pad_h, pad_w = patch_size - out.shape[2], patch_size - out.shape[3]
            if pad_h != 0 and pad_w != 0:
                out = F.pad(out, (pad_w // 2, pad_w - pad_w // 2, pad_h // 2, pad_h - pad_h // 2), 'replicate')
            if use_llpm_buf and out_path is None and p_buffers is not None:
                if isinstance(p_buffers, dict):
                    out_path = {key: torch.zeros((v.shape[1], v.shape[2], h, w), device=v.device)
                                for key, v in p_buffers.items()}
                else:
                    out_path = torch.zeros((p_buffers.shape[1], p_buffers.shape[2], h, w), device=p_buffers.device)
            for b in range(out.shape[0]):
                i0, i1, j0, j1, ib, jb = (int(i_start[b]), int(i_end[b]), int(j_start[b]), int(j_end[b]),
                                          int(i[b]), int(j[b]))
                out_rad[:, i0:i1, j0:j1] = out[b, :, i0 - ib:i1 - ib, j0 - jb:j1 - jb]
                if use_llpm_buf and out_path is not None:
                    if isinstance(p_buffers, dict):
                        for key in p_buffers:
                            out_path[key][:, :, i0:i1, j0:j1] = p_buffers[key][b, :, :, i0 - ib:i1 - ib, j0 - jb:j1 - jb]
                    else:
                        out_path[:, :, i0:i1, j0:j1] = p_buffers[b, :, :, i0 - ib:i1 - ib, j0 - jb:j1 - jb]
    return out_rad, out_path


def crop_and_composite(out_rad, noisy_input, has_hit, patch_size=128, valid_size=72):
    """``test_models.py:217-232`` on (H, W, 3) tensors: valid-core crop, then the noisy input wherever no surface
    was hit (background and emitters are not denoised)."""
    crop = (patch_size - valid_size) // 2
    out_rad = out_rad[crop:-crop, crop:-crop, ...]
    noisy_input = noisy_input[crop:-crop, crop:-crop, ...]
    has_hit = has_hit[crop:-crop, crop:-crop, ...]
    return torch.where(has_hit == 0, noisy_input, out_rad)


def _zero_pbuffers(p_buffers, h, w):
    """The stitched P-buffers of an h x w frame, zeroed: (S, C, h, w) for the (B, S, C, P, P) of a batch, or a dict of them."""
    if isinstance(p_buffers, dict):
        return {key: _zero_pbuffers(v, h, w) for key, v in p_buffers.items()}
    return torch.zeros((p_buffers.shape[1], p_buffers.shape[2], h, w), device=p_buffers.device)


def _stitch_batches(batches, run, h, w, keep_pbuffers, patch_size, first_output=None):
    """THE tile loop of full-frame inference: ``run(batch)`` -> ``(out, p_buffers)`` for every ``(batch, coords)`` of ``batches``
    (``coords``: the device (B, 6) rows of the tile table), one ``ops.stitch_tiles`` launch per batch.  The P-buffers are stitched
    with ``keep_pbuffers`` where the model returns any.  ``first_output(out)`` sees the first batch's output before it is stitched.
    Returns ``(out_rad (3, h, w), out_path)``; out_path is None, or (S, C, h, w) / a dict of them, as the P-buffers come."""
    from .. import ops
    out_rad, out_path = None, None
    for batch, coords in batches:
        out, p_buffers = run(batch)
        if out_rad is None:
            out_rad = torch.zeros((3, h, w), device=out.device)
            if first_output is not None:
                first_output(out)
        if not (keep_pbuffers and p_buffers is not None):
            p_buffers = None
        else:
            if out_path is None:
                out_path = _zero_pbuffers(p_buffers, h, w)
            p_buffers = ({key: v.contiguous() for key, v in p_buffers.items()} if isinstance(p_buffers, dict)
                         else p_buffers.contiguous())
        ops.stitch_tiles(out, p_buffers, coords, out_rad, out_path, patch_size)
    return out_rad, out_path


def stitched_inference(interface, dataset, patch_size=128, use_llpm_buf=True):
    """``inference`` over a ``support.datasets.FullImageDataset`` with one ``wcmc_stitch_tiles`` launch per batch in place of
    the per-tile slice copies (bit-identical to them).  Returns ``(out_rad (3, H, W), out_path)`` on the device; out_path is
    None, or (like the P-buffers of ``validate_batch``) a dict / tensor of (S, C, H, W)."""
    interface.to_eval_mode()
    with torch.no_grad():
        return _stitch_batches(dataset.tile_batches(), interface.validate_batch, dataset.h, dataset.w, use_llpm_buf, patch_size)


# ------------------------------------------------------------------------------- denoising a render of any size (wcmc_amd.denoise)
def frame_tiles(h, w, patch=128, pad=32):
    """The tile table ``[(i_start, j_start, i_end, j_end, i, j)]`` of an h x w frame of any size, in FRAME coordinates.

    The frame is taken as extended by ``pad`` pixels on every side by mirror reflection with the edge repeated (numpy 'symmetric';
    ``ops.assemble_kpcn_tiles`` reads it so, without building it).  Tiles of ``patch`` pixels lie over the extended frame at stride
    ``patch - 2*pad``; the last origin in each direction is clamped to ``dim + 2*pad - patch`` of the extended frame, so the origins
    ``i``, ``j`` run from ``-pad`` to ``dim + pad - patch``.  A tile owns pixels of its own interior only -- ``i + pad <= i_start <
    i_end <= i + patch - pad`` -- and a clamped tile owns what its neighbour left; the owned windows partition the frame."""
    stride = patch - 2 * pad
    if pad < 0 or stride <= 0:
        raise ValueError("frame_tiles: a %d-pixel tile has no interior inside a pad of %d" % (patch, pad))
    if h < stride or w < stride:
        raise ValueError("frame_tiles: the %d x %d frame is smaller than the %d-pixel interior of a tile (patch %d - 2 * pad %d) in "
                         "at least one dimension" % (h, w, stride, patch, pad))

    def spans(n):
        """[(start, end, origin)] along one axis."""
        out, last, start = [], n + pad - patch, 0
        while start < n:
            o = min(start - pad, last)                       # the tile whose interior would begin at `start`, clamped
            end = o + patch - pad
            out.append((start, end, o))
            start = end
        return out
    return [(i0, j0, i1, j1, i, j) for i0, i1, i in spans(h) for j0, j1, j in spans(w)]


def frame_transform_shape(h, w, t):
    """The sizes of ``T_t`` of an h x w frame: (h, w) for the even dihedral codes, (w, h) for the odd ones."""
    if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t <= 7:
        raise ValueError("frame_transform_shape: the transform code %r lies outside 0..7" % (t,))
    return (w, h) if t & 1 else (h, w)


def denoise_frame(interface, kpcn, llpm, use_llpm_buf=True, batch_size=8, want_pbuffers=False, patch_size=128, pad_size=32,
                  preview=False, times=None, ensemble=(0,), blend=0):
    """Denoise one frame of any size from its device buffers ``kpcn`` (H, W, 44) and ``llpm`` (H, W, S, 37), with no ground truth:
    per batch of ``frame_tiles`` one ``ops.assemble_kpcn_tiles`` launch, ``interface.denoise_batch`` and one ``ops.stitch_tiles``
    launch; then ``ops.finish_frame``.  ``llpm`` is always needed (``has_hit``); it feeds the network with ``use_llpm_buf``.

    Returns ``(out, ipt, has_hit)`` -- the denoised frame (H, W, 3) with the noisy input wherever no surface was hit, the noisy
    input (H, W, 3) and the mask (H, W) -- then the stitched P-buffers ((S, C, H, W), a dict of them, or None) when
    ``want_pbuffers``, then the two uint8 previews (of ``out`` and of ``ipt``) when ``preview``.  ``times``: a dict that receives the
    seconds of 'network' (tiles, network, stitching) and 'finish', at the price of two device synchronisations, and 'tiles' (with an
    ensemble of more than one code: the tiles of all passes, and 'codes', the sorted set; away from the default tiling: 'tile',
    'tile_pad' and 'blend').

    ``ensemble``: the dihedral self-ensemble, a set of distinct codes 0..7 that contains 0.  The frame is
    denoised once per code, as if the raw frame had been transformed by ``T_t`` before preprocessing (its own tile table; the 26
    differences retaken along the turned axes), every result is turned back, and the fp32 sum in code order is divided by the number
    of codes.  The P-buffers, ``ipt`` and ``has_hit`` are those of the identity pass; ``(0,)`` is bit for bit the plain frame.

    ``patch_size`` / ``pad_size``: the tile side and its overlap (``--tile`` / ``--tile_pad``); with ``use_llpm_buf`` the result depends
    on both, because the PathNet's zero-padded U-Net sees each tile's border.  ``blend``: the feather
    half-width F of section 22, ``0 <= F <= pad_size - 28`` (the inset inside which a tile's output reads tile data only) and
    ``2 F <= patch_size - 2 * pad_size``; the radiance of every pass is the weighted mean of the tiles that reach a pixel, each pass
    normalised by its own weight sum.  The P-buffers are stitched by owned window.  0 is the owned-window stitch, bit for bit."""
    from .. import ops
    check_blend("denoise_frame", blend, patch_size, pad_size, KPCN_INSET)
    return _denoise_tiles(
        "denoise_frame", interface, kpcn,
        lambda origins, t=0: ops.assemble_kpcn_tiles(kpcn, llpm if use_llpm_buf else None, origins, patch_size, pad_size,
                                                     check_origins=False, transform=t),
        lambda out_rad: ops.finish_frame(out_rad, kpcn, llpm, preview=preview),
        batch_size, want_pbuffers, patch_size, pad_size, preview, times, ensemble=ensemble, blend=blend, inset=KPCN_INSET)


KPCN_INSET = 28      # 36 pixels of 5 x 5 shrink on a 128-pixel tile leave 92, the 21 x 21 apply needs 10 of them


def check_blend(who, blend, patch_size, pad_size, inset=None):
    """Host check of the feather half-width: an integer ``0 <= F``; ``2 F <= patch - 2 * pad``, so that no more
    than three tiles meet on an axis; and, where the ``inset`` of the model is known, ``F <= pad - inset``: a tile contributes to
    ``[a - F, b + F)`` of every axis, which must stay inside the window ``[o + inset, o + patch - inset)`` that its output fills from
    tile data.  Returns F."""
    import numbers
    if isinstance(blend, bool) or not isinstance(blend, numbers.Integral) or blend < 0:
        raise ValueError("%s: --blend should be a non-negative number of pixels, got %r" % (who, blend))
    blend = int(blend)
    if blend and 2 * blend > patch_size - 2 * pad_size:
        raise ValueError("%s: --blend %d: the two ramps of a seam take %d pixels, more than the %d-pixel interior of a tile (--tile %d "
                         "- 2 * --tile_pad %d)" % (who, blend, 2 * blend, patch_size - 2 * pad_size, patch_size, pad_size))
    if blend and inset is not None and blend > pad_size - inset:
        raise ValueError("%s: --blend %d: with --tile_pad %d a feather may be %d pixels wide at the most; the outer %d pixels of a "
                         "tile's output are not computed from the tile's own data alone"
                         % (who, blend, pad_size, max(pad_size - inset, 0), inset))
    return blend


def check_tile_fits(who, h, w, patch_size, pad_size, codes=(0,)):
    """A tile must fit the frame extended by the pad in both dimensions.  The condition is symmetric in the two, so it covers the
    transposed frame of the odd ensemble ``codes`` as well; the message names that frame where it is the one being tiled."""
    if pad_size < 0 or patch_size <= 2 * pad_size:
        return                                                       # (frame_tiles refuses a tile without an interior)
    if patch_size > h + 2 * pad_size or patch_size > w + 2 * pad_size:
        raise ValueError("%s: a %d-pixel tile (--tile) does not fit the %d x %d frame%s extended by the pad of %d (--tile_pad) on "
                         "every side" % (who, patch_size, h, w, " (nor its transpose under the odd ensemble codes)"
                                         if any(t & 1 for t in codes) else "", pad_size))


def _blend_pass(table_dev, batch_size, assemble, run, t, out_rad, sums, blend, patch_size, pad_size, keep_pbuffers=False,
                first_output=None):
    """One pass of the feathered stitch over the table of the frame transformed by code ``t``: per batch
    ``assemble``, ``run`` and one ``ops.stitch_tiles_blend`` launch into the zeroed ``sums`` (acc, wsum), then ``ops.blend_finish``
    into ``out_rad`` -- written by the identity pass, added to by the others.  The identity pass stitches the P-buffers by owned
    window where ``keep_pbuffers``; returns them (or None)."""
    from .. import ops
    acc, wsum = sums
    acc.zero_()
    wsum.zero_()
    out_path = None
    org_dev = table_dev[:, 4:6].contiguous()
    for k in range(0, table_dev.shape[0], batch_size):
        coords = table_dev[k:k + batch_size]
        out, p_buffers = run(assemble(org_dev[k:k + batch_size], t) if t else assemble(org_dev[k:k + batch_size]))
        if k == 0 and first_output is not None:
            first_output(out)
        if keep_pbuffers and p_buffers is not None:
            if out_path is None:
                out_path = _zero_pbuffers(p_buffers, *out_rad.shape[1:])
            p_buffers = ({key: v.contiguous() for key, v in p_buffers.items()} if isinstance(p_buffers, dict)
                         else p_buffers.contiguous())
            ops.stitch_tiles(out, p_buffers, coords, out_rad, out_path, patch_size)       # (its radiance is overwritten below)
        ops.stitch_tiles_blend(out, coords, acc, wsum, blend, t, patch_size, pad_size)
    ops.blend_finish(acc, wsum, out_rad, accumulate=bool(t))
    return out_path


def _denoise_tiles(who, interface, frame, assemble, finish, batch_size, want_pbuffers, patch_size, pad_size, preview, times,
                   check_output=False, ensemble=(0,), blend=0, inset=None):
    """THE frame driver behind ``denoise_frame`` and ``denoise_sample_frame`` (``who``): the tile table of ``frame``, a device buffer (H, W, ...)
    of the family, and its host checks, ``_stitch_batches`` over ``assemble(origins)`` -- the family's batch for a device (B, 2) slice of the tile
    origins -- and ``interface.denoise_batch``, then ``finish(out_rad)``, the family's closing op, and the return tuple.
    ``check_output``: ``check_output_size`` on the first batch's output.  A third model family supplies the two closures.
    ``ensemble``: after the identity pass, one pass per further code t over the tile table of the transformed frame --
    ``assemble(origins, t)``, ``interface.denoise_batch``, ``ops.stitch_tiles_aug`` adding into the same ``out_rad`` -- then one
    division by the number of codes (``denoise_frame``).
    ``blend``: a feather half-width above 0 runs every pass through ``_blend_pass`` instead; ``inset``: the
    model's, where it is known before the first batch; with ``check_output`` the first output's replicated border is held to
    ``pad - blend`` too.  0 launches what it always did."""
    import time
    from .. import ops
    (h, w), device = frame.shape[:2], frame.device
    codes = ops.check_frame_transforms(ensemble)
    blend = check_blend(who, blend, patch_size, pad_size, inset)
    check_tile_fits(who, h, w, patch_size, pad_size, codes)
    coords = frame_tiles(h, w, patch_size, pad_size)
    ops.check_tile_coords(coords, h, w, patch_size)
    ops.check_tile_origins([c[4:6] for c in coords], h, w, patch_size, pad_size, who=who)
    tables = {(h, w): coords}                                    # one table per shape of the transformed frame: at most two
    for t in codes[1:]:
        ht, wt = frame_transform_shape(h, w, t)
        if (ht, wt) not in tables:
            tables[(ht, wt)] = frame_tiles(ht, wt, patch_size, pad_size)
            ops.check_tile_coords(tables[(ht, wt)], ht, wt, patch_size)
            ops.check_tile_origins([c[4:6] for c in tables[(ht, wt)]], ht, wt, patch_size, pad_size, who=who)
    interface.to_eval_mode()
    if times is not None:
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
    with torch.no_grad():
        coords_dev = torch.tensor(coords, dtype=torch.int32, device=device)
        origins_dev = coords_dev[:, 4:6].contiguous()
        batches = ((assemble(origins_dev[k:k + batch_size]), coords_dev[k:k + batch_size]) for k in range(0, len(coords), batch_size))
        first = ((lambda out: check_output_size(out.shape[2], out.shape[3], patch_size, pad_size, blend)) if check_output or
                 (blend and inset is None) else None)
        if blend:
            out_rad = torch.zeros((3, h, w), device=device)
            sums = (torch.empty((3, h, w), device=device), torch.empty((h, w), device=device))
            out_path = _blend_pass(coords_dev, batch_size, assemble, interface.denoise_batch, 0, out_rad, sums, blend, patch_size,
                                   pad_size, want_pbuffers, first)
        else:
            out_rad, out_path = _stitch_batches(batches, interface.denoise_batch, h, w, want_pbuffers, patch_size, first)
        tiles = len(coords)
        for t in codes[1:]:
            table = tables[frame_transform_shape(h, w, t)]
            table_dev = coords_dev if table is coords else torch.tensor(table, dtype=torch.int32, device=device)
            if blend:
                _blend_pass(table_dev, batch_size, assemble, interface.denoise_batch, t, out_rad, sums, blend, patch_size, pad_size)
            else:
                org_dev = table_dev[:, 4:6].contiguous()
                for k in range(0, len(table), batch_size):
                    out, _ = interface.denoise_batch(assemble(org_dev[k:k + batch_size], t))
                    ops.stitch_tiles_aug(out, table_dev[k:k + batch_size], out_rad, t, True, patch_size)
            tiles += len(table)
        if len(codes) > 1:
            out_rad = out_rad / torch.full((), len(codes), dtype=out_rad.dtype, device=device)      # one fp32 division
        if times is not None:
            torch.cuda.synchronize(device)
            t1 = time.perf_counter()
        res = finish(out_rad)
        if times is not None:
            torch.cuda.synchronize(device)
            times.update(network=t1 - t0, finish=time.perf_counter() - t1, tiles=tiles)
            if (patch_size, pad_size, blend) != (128, 32, 0):   # (a frame at the default tiling reports what it always did)
                times.update(tile=patch_size, tile_pad=pad_size, blend=blend)
            if len(codes) > 1:                                   # (an un-ensembled frame reports what it always did)
                times.update(codes=codes)
    return res[:3] + ((out_path,) if want_pbuffers else ()) + (tuple(res[3:]) if preview else ())


def check_output_size(ho, wo, patch_size, pad_size, blend=0):
    """A network output of ``ho x wo`` pixels is padded back to the tile by replication, ``(patch - ho + 1) // 2`` pixels at the most
    on a side (``ops.stitch_tiles``); those pixels must stay outside the owned window ``[pad, patch - pad)``.  The KPCN models'
    receptive field is known; a caller's denoiser is checked here."""
    if (patch_size - ho + 1) // 2 > pad_size or (patch_size - wo + 1) // 2 > pad_size:
        raise ValueError("denoise_sample_frame: the denoiser turns a %d-pixel tile into a %d x %d output, so up to %d pixels of a "
                         "side are replicated, more than the %d of --tile_pad: the owned window of a tile would hold padding"
                         % (patch_size, ho, wo, max((patch_size - ho + 1) // 2, (patch_size - wo + 1) // 2), pad_size))
    check_blend("denoise_sample_frame", blend, patch_size, pad_size, max((patch_size - ho + 1) // 2, (patch_size - wo + 1) // 2))


def denoise_sample_frame(interface, sbmc_s, sbmc_p, llpm, use_llpm_buf=True, use_g_buf=True, use_sbmc_buf=True, batch_size=8,
                         want_pbuffers=False, patch_size=128, pad_size=32, preview=False, times=None, ensemble=(0,), blend=0):
    """``denoise_frame`` for the sample-based interfaces (``SBMCInterface`` / ``LBMCInterface`` around the caller's denoiser), from
    the device buffers ``sbmc_s`` (H, W, S, 27), ``sbmc_p`` (H, W, S, 66; None without ``use_sbmc_buf``) and ``llpm`` (H, W, S, 37):
    per batch of ``frame_tiles`` one ``ops.assemble_sample_tiles`` launch, ``interface.denoise_batch`` and one ``ops.stitch_tiles``
    launch; then ``ops.finish_sample_frame``.  ``llpm`` is always needed (``has_hit``); it feeds the network with ``use_llpm_buf``.
    The denoiser's receptive field is the caller's: an output so small that replicated pixels would reach an owned window is a
    ``ValueError`` after the first batch (``check_output_size``).  Returns what ``denoise_frame`` returns; the P-buffer is one
    (S, C, H, W) tensor.  ``ensemble``: as ``denoise_frame``'s; every channel of these buffers is a copy under a transform.
    ``blend``: as ``denoise_frame``'s, against the inset of the caller's denoiser: the replicated border of its output, known after
    the first batch (``check_output_size``)."""
    from .. import ops
    return _denoise_tiles(
        "denoise_sample_frame", interface, sbmc_s,
        lambda origins, t=0: ops.assemble_sample_tiles(sbmc_s, sbmc_p if use_sbmc_buf else None, llpm if use_llpm_buf else None,
                                                       origins, patch_size, pad_size, use_g_buf, use_sbmc_buf, check_origins=False,
                                                       transform=t),
        lambda out_rad: ops.finish_sample_frame(out_rad, sbmc_s, llpm, preview=preview),
        batch_size, want_pbuffers, patch_size, pad_size, preview, times, check_output=True, ensemble=ensemble, blend=blend)
