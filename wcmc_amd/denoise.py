"""Denoise raw renders of any size with a trained KPCN, SBMC or LBMC model: no ground truth, no offline files, every pixel.

    python -m wcmc_amd.denoise --input A.npy [B.npy ...] --output_dir OUT --save WEIGHTS_DIR --model_name KPCN_manifold \\
        [--spp N] [--tile_batch B] [--tile P] [--tile_pad N] [--blend F] [--band_rows N] [--png] [--save_pbuffer] [--rhf] [--self_ensemble [CODE ...]] \\
        [--use_llpm_buf --manif_learn --manif_loss FMSE ...]
    python -m wcmc_amd.denoise ... --model_name SBMC_manifold --denoiser my_pkg.models:make_multisteps [--use_sbmc_buf] [--tile_pad N]

Per input file (renderer output (H, W, S, 104), H and W at least 64): the first ``--spp`` samples (default: what the file holds; a
file that holds fewer is continued by ``<stem>_1.npy``, ``<stem>_2.npy``, ... beside it) are streamed to the device in row bands,
sanitised and preprocessed there band by band (``support.staging.FrameStreamer``: the raw frame never lies whole in host or device
memory, and the next file's bands cross while this one's network runs; ``--band_rows`` bounds the pinned memory);
``support.inference.denoise_frame`` runs the network over mirror-extended tiles and composites the result;
``OUT/<stem>_denoised.npy`` and ``.pfm`` hold the (H, W, 3) float frame.  ``--png`` adds 8-bit tone-mapped previews of the result
and of the noisy input, ``--save_pbuffer`` the stitched P-buffer as (H, W, S, C).  ``--rhf`` filters the noisy input by the stitched
P-buffer (``wcmc_amd.rhf``; ``--rhf_radius``, ``--rhf_patch_radius``, ``--rhf_bandwidth``, ``--rhf_eps``) with ``has_hit`` as the mask and
writes ``<stem>_rhf.npy`` and the neighbour count ``<stem>_rhf_neighbours.npy`` (PNGs with ``--png``).  ``--self_ensemble [CODE ...]``
denoises the frame under several dihedral codes of ``--augment`` (bare: all eight; ``0 2 4 6``: the flips), turns every result back
and averages them; the P-buffer stays the un-ensembled one.  The model flags are those of
``wcmc_amd.train_kpcn``; the model is ``<save>/<model_name>.pth``.  One line per frame reports the seconds of each phase.

A model whose name holds ``SBMC`` / ``LBMC`` is a ``train_sbmc`` / ``train_lbmc`` checkpoint around the caller's base denoiser
(``--denoiser package.module:factory``, required; ``--disentangle``, ``--use_sbmc_buf``, ``--lr_dncnn`` as those launchers define them).
Its frames are streamed as ``sbmc_s`` / ``sbmc_p`` / ``llpm`` and run through ``support.inference.denoise_sample_frame``; the P-buffer
is one tensor.  ``--tile_pad N`` (default 32) is the overlap of the tiles: the denoiser's receptive field is the caller's,
and an output that leaves fewer real pixels than the pad is refused.

``--tile P`` (a multiple of 64 in 128..512, default 128) is the tile side, ``--tile_pad N`` the overlap (KPCN models: at least 32, and
``P - 2 N >= 64``), ``--blend F`` (default 0) the half-width of a feather that blends the radiance of neighbouring tiles over the
``2 F`` pixels around every seam (KPCN: ``F <= N - 28``; sample-based: ``N`` minus the denoiser's inset; ``2 F <= P - 2 N``).  DESIGN.md
section 22; 128 / 32 / 0 is section 15's path bit for bit.
"""
import os
import struct
import time
import zlib

import numpy as np
import torch

from . import ops, rhf, train_kpcn
from .support.datasets import MAX_CONTINUATIONS, dncnn_in_size
from .support.inference import (KPCN_INSET, check_blend, check_tile_fits, denoise_frame, denoise_sample_frame, frame_tiles)
from .support.staging import FrameStreamer

PATCH_SIZE, PAD_SIZE = 128, 32


# ------------------------------------------------------------------------------------------------- image writers
def write_pfm(fn, img):
    """(H, W, 3) or (H, W) float image -> little-endian PFM (rows bottom to top, scale -1.0)."""
    img = np.asarray(img, dtype='<f4')
    if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError("write_pfm: the image should be (H, W) or (H, W, 3), got %s" % (img.shape,))
    with open(fn, 'wb') as f:
        f.write(b'%s\n%d %d\n-1.0\n' % (b'PF' if img.ndim == 3 else b'Pf', img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img[::-1]).tobytes())


def write_png(fn, img):
    """(H, W, 3) uint8 image -> 8-bit RGB PNG, with the standard library alone (filter 0 on every row)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("write_png: the image should be (H, W, 3) uint8, got %s %s" % (img.dtype, img.shape))
    h, w = img.shape[:2]
    rows = np.concatenate((np.zeros((h, 1), np.uint8), img.reshape(h, w * 3)), axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    with open(fn, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
                + chunk(b'IDAT', zlib.compress(rows, 6)) + chunk(b'IEND', b''))


# ------------------------------------------------------------------------------------------------- input
def tile_batch_size(spp, tile_batch=None, tile=PATCH_SIZE):
    """Tiles per network call: 8 up to 32 spp, 4 up to 64 (test_models.py:147-161) for the 128-pixel tile; a larger ``tile`` keeps that
    pixel budget per call, ``max(1, B128 * 128^2 // tile^2)``.  Above 64 spp the caller decides."""
    if tile_batch is not None:
        if tile_batch < 1:
            raise ValueError("--tile_batch should be at least 1, got %d" % tile_batch)
        return tile_batch
    if spp <= 32:
        return max(1, 8 * PATCH_SIZE * PATCH_SIZE // (tile * tile))
    if spp <= 64:
        return max(1, 4 * PATCH_SIZE * PATCH_SIZE // (tile * tile))
    raise ValueError("no default tile batch size above 64 samples per pixel (got %d): give --tile_batch after looking at the "
                     "device's memory" % spp)


TILE_LIMITS = (
    # (the kernel's limit as its WCMC_REQUIRE states it, the quantity for tiles of P pixels, pad, S samples, B tiles per call, the bound)
    ("to_nhwc / from_nhwc / split_from_nchw: N * H <= 65535 rows per launch (N = B * S for the per-sample tensors)",
     lambda P, pad, S, B: B * S * P, 65535),
    ("final2 / embed3: B * S * H * W * 256 bytes < 0x7ff00000 (the 64-channel per-sample activations in one 2 GiB buffer view)",
     lambda P, pad, S, B: B * S * P * P * 256, 0x7ff00000 - 1),
    ("conv2d: every operand below 2 GiB (the 21 x 21 kernel logits, 441 channels padded to 448 fp32, of one call)",
     lambda P, pad, S, B: B * P * P * 448 * 4, 0x7ff00000 - 1),
    # (kernel_splat's h * w < 2^30 and N <= 65535 and the stitches' B <= 65535 lie behind the first row for every tile of 128..512)
)


def check_tile_limits(tile, pad, spp, tile_batch, per_sample=True):
    """The hard limits that the kernels of the inference forward state in their argument checks, collected: a ``(tile, pad, spp,
    tile_batch)`` that crosses one is refused here, before anything is launched, with the flags to turn and the limit.  No limit is
    lifted; a combination that passes here and is refused by a kernel all the same is a limit missing from ``TILE_LIMITS``.
    ``per_sample``: the model holds per-sample tensors (``--use_llpm_buf``, SBMC / LBMC); without them the limits are those of S = 1.
    One tile of a per-sample model reaches final2's 2 GiB view at 64 spp and 384 pixels and at 32 spp and 512: such frames take a smaller tile."""
    for what, quantity, bound in TILE_LIMITS:
        q = quantity(tile, pad, spp if per_sample else 1, tile_batch)
        if q > bound:
            raise ValueError("--tile %d with --tile_batch %d at %d samples per pixel crosses a kernel's limit (%d > %d): %s.  Give a "
                             "smaller --tile or --tile_batch" % (tile, tile_batch, spp, q, bound, what))
    return tile_batch


def _per_sample(args):
    return bool(args.use_llpm_buf) or sample_launcher(args.model_name) is not None


def check_tile_flags(args):
    """``--tile``, ``--tile_pad`` and ``--blend`` against one another, before any file is looked for.  KPCN
    models: ``32 <= pad``, ``tile - 2 * pad >= 64`` and ``blend <= pad - 28``; the sample-based models' inset is their denoiser's and
    is checked on the first batch.  Returns (tile, pad, blend)."""
    tile, pad, blend = getattr(args, 'tile', PATCH_SIZE), getattr(args, 'tile_pad', PAD_SIZE), getattr(args, 'blend', 0)
    if tile % 64 or not 128 <= tile <= 512:
        raise ValueError("--tile %d: the tile side should be a multiple of 64 in 128..512" % tile)
    sample = sample_launcher(args.model_name) is not None
    if sample:
        frame_tiles(2 * tile, 2 * tile, tile, pad)                                      # (a pad without an interior)
    else:
        if pad < PAD_SIZE:
            raise ValueError("--tile_pad %d: the KPCN models need a pad of at least %d, the one their receptive field was checked "
                             "against (DESIGN.md section 15)" % (pad, PAD_SIZE))
        if tile - 2 * pad < 64:
            raise ValueError("--tile_pad %d with --tile %d leaves a tile an interior of %d pixels; the KPCN models are run with at "
                             "least 64" % (pad, tile, tile - 2 * pad))
    check_blend("denoise", blend, tile, pad, None if sample else KPCN_INSET)
    return tile, pad, blend


def _open_raw(fn):
    if not os.path.isfile(fn):
        raise FileNotFoundError(fn)
    a = np.load(fn, mmap_mode='r')
    if a.ndim != 4 or a.shape[-1] != 104:
        raise ValueError("%s: shape %s is not renderer output (H, W, S, 104)" % (fn, tuple(a.shape)))
    return a


def read_raw(fn, spp=None):
    """The memory-mapped parts ``[(H, W, s_k, 104)]`` that hold the first ``spp`` samples of frame ``fn`` (default: the samples in
    the file), and ``spp``.  A file with fewer samples is continued by ``<stem>_1.npy``, ``<stem>_2.npy``, ... (datasets.py:632-640);
    a series that ends before ``spp`` samples are there is a ``ValueError``."""
    a = _open_raw(fn)
    if spp is None:
        spp = a.shape[2]
    if spp < 1:
        raise ValueError("--spp should be at least 1, got %d" % spp)
    parts, have = [a[:, :, :spp]], min(a.shape[2], spp)
    stem, ext = os.path.splitext(fn)
    for k in range(1, MAX_CONTINUATIONS + 1):
        if have >= spp:
            break
        cont = stem + '_' + str(k) + ext
        if not os.path.isfile(cont):
            break
        c = _open_raw(cont)
        if c.shape[:2] != a.shape[:2]:
            raise ValueError("%s: a %d x %d continuation of the %d x %d frame %s" % ((cont,) + c.shape[:2] + a.shape[:2] + (fn,)))
        parts.append(c[:, :, :spp - have])
        have += parts[-1].shape[2]
    if have < spp:
        raise ValueError("%s and its continuation files (%s_1%s, ...) hold %d samples per pixel, fewer than the %d asked for (--spp)"
                         % (fn, stem, ext, have, spp))
    return parts, spp


def upload_raw(parts, device):
    """One contiguous (H, W, spp, 104) device tensor from the host parts (each read from disk once), sanitised.  The whole-frame
    route: ``support.staging.FrameStreamer`` is what the command runs, and this is what its tests hold it to."""
    h, w = parts[0].shape[:2]
    spp = sum(p.shape[2] for p in parts)
    raw = torch.empty((h, w, spp, 104), device=device, dtype=torch.float32)
    s0 = 0
    for p in parts:
        t = torch.from_numpy(np.array(p, dtype=np.float32, order='C'))
        if len(parts) == 1:
            raw.copy_(t)
        else:
            raw[:, :, s0:s0 + p.shape[2]] = t.to(device)
        s0 += p.shape[2]
    return ops.sanitize_(raw)


# ------------------------------------------------------------------------------------------------- one frame
def denoise_file(interface, fn, output_dir, args, device, frames=None):
    """Denoise ``fn`` and write its outputs; returns the dict of phase seconds.  ``frames``: a ``FrameStreamer`` whose next frame is
    ``fn`` (``main``: one streamer over all the inputs, so that the next file is prefetched); None: one for ``fn`` alone.
    'upload' is the host's wait for the frame's buffers -- after the first frame of a sequence, what the prefetch did not hide --
    and 'preprocess' the finish pass of the preprocessing."""
    stem = os.path.splitext(os.path.basename(fn))[0]
    own = frames is None
    t0 = time.perf_counter()
    if own:
        frames = make_streamer([fn], args, device)
    try:
        bufs = next(frames)
        ev0, ev1 = frames.finish_events
        ev1.synchronize()
    finally:
        if own:
            frames.close()
    return _denoise_buffers(interface, stem, bufs, output_dir, args, time.perf_counter() - t0, ev0.elapsed_time(ev1) * 1e-3)


def denoise_buffers(interface, stem, kpcn, llpm, output_dir, args, upload=0.0, preprocess=0.0):
    """Denoise the frame from its device buffers ``kpcn`` (H, W, 44) and ``llpm`` (H, W, S, 37), ready on the current stream, and write
    the outputs of ``stem``; returns the dict of phase seconds, with ``upload`` and ``preprocess`` as the caller measured them."""
    return _denoise_buffers(interface, stem, (kpcn, llpm), output_dir, args, upload, preprocess)


def denoise_sample_buffers(interface, stem, sbmc_s, sbmc_p, llpm, output_dir, args, upload=0.0, preprocess=0.0):
    """``denoise_buffers`` for an SBMC / LBMC model, from ``sbmc_s`` (H, W, S, 27), ``sbmc_p`` (H, W, S, 66) or None, and ``llpm``."""
    return _denoise_buffers(interface, stem, (sbmc_s, sbmc_p, llpm), output_dir, args, upload, preprocess)


def _denoise_buffers(interface, stem, bufs, output_dir, args, upload=0.0, preprocess=0.0):
    """``bufs``: what ``make_streamer``'s ``FrameStreamer`` yields for the family that the model's name stands for."""
    t1 = time.perf_counter()
    llpm = bufs[-1]
    h, w, spp = llpm.shape[:3]
    tile, pad, blend = getattr(args, 'tile', PATCH_SIZE), getattr(args, 'tile_pad', PAD_SIZE), getattr(args, 'blend', 0)
    batch_size = check_tile_limits(tile, pad, spp, tile_batch_size(spp, args.tile_batch, tile), _per_sample(args))
    times = {}
    want_rhf = getattr(args, 'rhf', False)
    want_p = args.save_pbuffer or want_rhf
    if sample_launcher(args.model_name) is not None:
        res = denoise_sample_frame(interface, bufs[0], bufs[1], llpm, args.use_llpm_buf, args.use_g_buf, args.use_sbmc_buf,
                                   batch_size, want_pbuffers=want_p, patch_size=tile, pad_size=pad,
                                   preview=args.png, times=times, ensemble=ensemble_codes(args), blend=blend)
    else:
        res = denoise_frame(interface, bufs[0], llpm, args.use_llpm_buf, batch_size, want_pbuffers=want_p,
                            patch_size=tile, pad_size=pad, preview=args.png, times=times, ensemble=ensemble_codes(args),
                            blend=blend)
    out, out_path = res[0], (res[3] if want_p else None)
    os.makedirs(output_dir, exist_ok=True)
    img = out.cpu().numpy()
    np.save(os.path.join(output_dir, stem + '_denoised.npy'), img)
    write_pfm(os.path.join(output_dir, stem + '_denoised.pfm'), img)
    if args.png:
        pv_out, pv_ipt = res[-2], res[-1]
        write_png(os.path.join(output_dir, stem + '_denoised.png'), pv_out.cpu().numpy())
        write_png(os.path.join(output_dir, stem + '_input.png'), pv_ipt.cpu().numpy())
    if args.save_pbuffer:
        if out_path is None:
            raise ValueError("--save_pbuffer: the model computes no P-buffer (it needs --use_llpm_buf)")
        p = out_path['diffuse'] if isinstance(out_path, dict) else out_path
        np.save(os.path.join(output_dir, stem + '_pbuffer.npy'), p.permute(2, 3, 0, 1).cpu().numpy())
    if want_rhf:
        if out_path is None:
            raise ValueError("--rhf: the model computes no P-buffer (it needs --use_llpm_buf)")
        f_out, f_wsum = rhf.rhf_filter(res[1], out_path, res[2], **rhf_arguments(args))
        rhf.write_outputs(output_dir, stem, f_out, f_wsum, args.rhf_radius, png=args.png)
    times.update(upload=upload, preprocess=preprocess, write=time.perf_counter() - t1 - times['network'] - times['finish'],
                 tile=tile, tile_pad=pad, blend=blend)
    print("%s: %d x %d, %d spp, %d tiles of %d pixels, %d per call: upload %.3f s, preprocess %.3f s, network %.3f s, finish %.3f s"
          % (stem, h, w, spp, times['tiles'], tile, batch_size, times['upload'], times['preprocess'], times['network'],
             times['finish']))
    return times


def _model_path(args):
    name = args.model_name if args.model_name.endswith('.pth') else args.model_name + '.pth'
    return os.path.join(args.save, name)


def sample_launcher(model_name):
    """The launcher module whose ``init_model`` builds a model of this name, as test_models.py:166-171 dispatches: ``train_sbmc`` for
    'SBMC', ``train_lbmc`` for 'LBMC', None for the KPCN route."""
    if 'SBMC' in model_name:
        from . import train_sbmc
        return train_sbmc
    if 'LBMC' in model_name:
        from . import train_lbmc
        return train_lbmc
    return None


def restore_interface(args, device):
    """The trained model ``<save>/<model_name>.pth`` of any family, through ``init_model`` of the launcher that trained it
    (``sample_launcher``, around ``--denoiser``; ``train_kpcn`` otherwise) with ``start_epoch`` forced nonzero: it then restores the
    checkpoint.  The sizes are the evaluation datasets' (test_models.py:37-46): those of 'sbmc' at ``pnet_out_size`` 0 for a
    sample-based model, those of 'kpcn' at ``--pnet_out_size`` otherwise.  Refuses nothing but a missing file."""
    if not os.path.isfile(_model_path(args)):
        raise FileNotFoundError(_model_path(args))
    if args.start_epoch == 0:
        args.start_epoch = 1
    args.model_name = args.model_name[:-4] if args.model_name.endswith('.pth') else args.model_name
    launcher = sample_launcher(args.model_name)
    if launcher is not None:
        pnet_out, n_in = 0, dncnn_in_size('sbmc', args.use_g_buf, args.use_sbmc_buf, args.use_llpm_buf, 0)
    else:
        launcher, pnet_out = train_kpcn, args.pnet_out_size[0]
        n_in = dncnn_in_size('kpcn', True, False, args.use_llpm_buf, pnet_out)
    sizes = {'dncnn_in_size': n_in, 'pnet_in_size': 36 if args.use_llpm_buf else 0, 'pnet_out_size': pnet_out}
    interfaces, _ = launcher.init_model(sizes, args, device)
    return interfaces[0]


load_sample_interface = restore_interface               # (the name the sample-based route was given first)


def make_streamer(files, args, device):
    """The ``FrameStreamer`` of the model's family over ``files``."""
    kw = dict(base_model='sbmc', use_sbmc_buf=args.use_sbmc_buf) if sample_launcher(args.model_name) else {}
    return FrameStreamer(files, args.spp, device, band_rows=getattr(args, 'band_rows', None), **kw)


def load_interface(args, device):
    """``restore_interface`` for a model that can denoise a render without ground truth: a KPCN (not KPCN-Ref), SBMC or LBMC one."""
    if sample_launcher(args.model_name) is None:
        if 'KPCN' not in args.model_name:
            raise NotImplementedError("denoise: '%s' names neither a KPCN nor an SBMC / LBMC model" % args.model_name)
        if args.kpcn_ref:
            raise NotImplementedError("denoise: KPCN-Ref feeds the clean targets to the network; it cannot denoise a render without "
                                      "ground truth")
    return restore_interface(args, device)


def build_parser():
    p = train_kpcn.build_parser()
    p.description = "Denoise raw renders of any size with a trained KPCN, SBMC or LBMC model (no ground truth needed)."
    p.epilog = None
    for a in p._actions:
        if a.dest == 'desc':
            a.required = False                     # a training-run label; not needed to denoise
    p.add_argument('--input', type=str, nargs='+', required=True, help='renderer output files (H, W, S, 104), H and W >= 64')
    p.add_argument('--output_dir', type=str, required=True, help='where <stem>_denoised.npy / .pfm (and the optional files) go')
    p.add_argument('--spp', type=int, default=None,
                   help='samples per pixel to denoise (default: those in the file; more than the file holds are read from '
                        '<stem>_1.npy, <stem>_2.npy, ... beside it)')
    p.add_argument('--tile_batch', type=int, default=None,
                   help='tiles per network call (default: 8 up to 32 spp, 4 up to 64; required above 64)')
    p.add_argument('--band_rows', type=int, default=None,
                   help='rows of the frame per band of the streamed upload (default: bands of about 64 MiB); a memory control: six '
                        'bands are pinned on the host, one lies on the device, and the result does not depend on it')
    p.add_argument('--png', action='store_true', help='also write 8-bit tone-mapped <stem>_denoised.png and <stem>_input.png')
    p.add_argument('--save_pbuffer', action='store_true', help='also write the stitched P-buffer <stem>_pbuffer.npy (H, W, S, C)')
    p.add_argument('--rhf', action='store_true',
                   help='also filter the noisy input by the stitched P-buffer (wcmc_amd.rhf) and write <stem>_rhf.npy and the '
                        'neighbour count <stem>_rhf_neighbours.npy, PNGs with --png; needs --use_llpm_buf')
    p.add_argument('--self_ensemble', type=int, nargs='*', default=None, metavar='CODE',
                   help='dihedral self-ensemble: denoise the frame under several flips / quarter turns (codes 0..7 of --augment: '
                        'rot90 by CODE & 3 after a left-right flip if CODE & 4), turn every result back and average.  Without values: '
                        'all eight codes; `0 2 4 6` are the row-preserving codes (flips only).  The set must contain 0.  The network '
                        'time grows with the number of codes; meant for models trained with --augment')
    rhf.add_filter_arguments(p, prefix='rhf_')
    add_sample_arguments(p)
    p.add_argument('--tile', type=int, default=PATCH_SIZE, metavar='P',
                   help='side of the tiles the network is run on: a multiple of 64 in 128..512 (default 128).  A larger tile throws '
                        'less of every convolution away ((P / (P - 2 N))^2 of the work per pixel) and needs more memory per call')
    p.add_argument('--tile_pad', type=int, default=PAD_SIZE, metavar='N',
                   help='overlap of the tiles on each side (SBMC / LBMC: at least what the denoiser\'s receptive field '
                        'takes off a side of a tile; KPCN models: at least 32, and P - 2 N at least 64): context around the pixels '
                        'a tile owns')
    p.add_argument('--blend', type=int, default=0, metavar='F',
                   help='feather the seams between tiles over 2 F pixels (default 0: each pixel comes from the one tile that owns '
                        'it).  KPCN models: F <= N - 28; SBMC / LBMC: F <= N - what the denoiser takes off a side; 2 F <= P - 2 N')
    return p


def rhf_arguments(args):
    """The filter's parameters from the ``--rhf_*`` flags, checked."""
    return rhf.check_filter_arguments(args.rhf_radius, args.rhf_patch_radius, args.rhf_bandwidth, args.rhf_eps, flag='--rhf_')


def add_sample_arguments(p):
    """What ``train_sbmc.add_common_arguments`` defines and ``train_kpcn.build_parser`` lacks (``--disentangle`` and ``--lr_dncnn`` are
    there already, defined alike): the flags a sample-based model is built from."""
    p.add_argument('--denoiser', type=str, default=None, metavar='package.module:factory',
                   help='SBMC / LBMC: the base denoiser, factory(n_in) -> nn.Module mapping the batch dictionary to (B, 3, h, w).  '
                        'Required for these models')
    p.add_argument('--use_sbmc_buf', action='store_true', help='SBMC: use the sbmc-specific buffer.')
    p.add_argument('--use_g_buf', action='store_false', help='SBMC / LBMC: leave the g-buffer out (as in train_sbmc).')
    return p


def ensemble_codes(args):
    """The self-ensemble set of ``--self_ensemble``, checked: (0,) without the flag, all eight codes for the bare flag, else the listed
    codes sorted.  A set without 0, a repeated code or a code outside 0..7 is a ``ValueError`` that names the flag."""
    codes = getattr(args, 'self_ensemble', None)
    if codes is None:
        return (0,)
    if len(codes) == 0:
        return tuple(range(8))
    try:
        return ops.check_frame_transforms(codes)
    except ValueError as e:
        raise ValueError("--self_ensemble %s: %s" % (' '.join(str(c) for c in codes), str(e).split(': ', 1)[-1])) from None


def check_inputs(args):
    """Everything that can be refused before the GPU is touched: sample counts, continuation files, the tile batch size, the band."""
    ensemble_codes(args)
    if sample_launcher(args.model_name) is not None:
        from .train_sbmc import load_denoiser_factory
        load_denoiser_factory(getattr(args, 'denoiser', None))        # (a DenoiserFactoryError, before any file is looked for)
    tile, pad, _ = check_tile_flags(args)
    codes = ensemble_codes(args)
    if getattr(args, 'band_rows', None) is not None and args.band_rows < 1:
        raise ValueError("--band_rows should be at least 1, got %d" % args.band_rows)
    for fn in args.input:
        parts, spp = read_raw(fn, args.spp)
        batch_size = tile_batch_size(spp, args.tile_batch, tile)
        if (tile, pad) != (PATCH_SIZE, PAD_SIZE):       # (at the default tiling a frame is refused where it always was: frame_tiles)
            check_tile_fits("denoise: " + fn, parts[0].shape[0], parts[0].shape[1], tile, pad, codes)
        check_tile_limits(tile, pad, spp, batch_size, _per_sample(args))
    if args.save_pbuffer and not args.use_llpm_buf:
        raise ValueError("--save_pbuffer: the model computes no P-buffer (it needs --use_llpm_buf)")
    if getattr(args, 'rhf', False):
        if not args.use_llpm_buf:
            raise ValueError("--rhf: the model computes no P-buffer (it needs --use_llpm_buf)")
        rhf_arguments(args)
    return args


def main(argv=None):
    args = check_inputs(train_kpcn.check_args(build_parser().parse_args(argv)))
    device = torch.device('cuda', args.device_id)
    torch.cuda.set_device(device)
    interface = load_interface(args, device)
    frames = make_streamer(args.input, args, device)
    try:
        return [denoise_file(interface, fn, args.output_dir, args, device, frames=frames) for fn in args.input]
    finally:
        frames.close()


if __name__ == '__main__':
    main()
