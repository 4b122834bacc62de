"""GPU counterparts of the per-image preprocessing methods of the reference's ``support.datasets.DenoiseDataset``
(``datasets.py:286-361,487-582``): same names, same layouts, torch CUDA tensors instead of numpy arrays.

The reference runs these in numpy on the loader's CPU worker (``_offline_preprocess`` :584-660 and the online
path of ``__getitem__``); at 24.6 MB of raw samples per 128x128 patch the loader, not the GPUs, bounds a real
training run.  ``PatchBatcher`` is the device-side counterpart of what ``__getitem__`` does per
patch (importance sampling of patch origins, cropping, channel selection, target transforms, channel-first layout,
``datasets.py:795-840,1026-1146``); file handling stays with the caller.
"""
import numpy as np
import torch

from .. import ops as _ops


class DenoisePreprocessor:
    MAX_DEPTH = 5                                   # datasets.py:68

    def __init__(self, max_depth=MAX_DEPTH):
        self.max_depth = max_depth

    def _gradients(self, buf):
        """(h, w, c) -> (h, w, 2c): horizontal and vertical backward differences (datasets.py:286-300)."""
        return _ops.gradients(buf)

    def _preprocess_llpm(self, sample):
        """raw (h, w, s, 104) -> (h, w, s, 37): path weight, radiance w/o weight, light intensity, throughputs,
        bounce types, roughnesses (datasets.py:302-361)."""
        return _ops.preprocess_llpm(sample, self.max_depth)

    def _preprocess_kpcn(self, sample):
        """raw (h, w, s, 104) -> (h, w, 44): diffuse / specular / normal / depth / albedo means, variances and
        gradients (datasets.py:487-582)."""
        return _ops.preprocess_kpcn(sample, self.max_depth)

    def _preprocess_kpcn_prefix(self, sample, s_lo, s_hi):
        """raw (h, w, S, 104) -> (s_hi - s_lo + 1, h, w, 44): ``_preprocess_kpcn(sample[:, :, :s])`` for s = s_lo..s_hi from one read
        of the frame -- what ``MSDenoiseDataset`` (datasets.py:1149-1171) computes once per count."""
        return _ops.preprocess_kpcn_prefix(sample, s_lo, s_hi, self.max_depth)

    def _preprocess_sbmc(self, sample):
        """sanitised raw (h, w, s, 104) -> (sbmc_s (h, w, s, 27), sbmc_p (h, w, s, 66)): per-sample radiance, log radiance, log
        specular, subpixel and g-buffer; log sampling probabilities, clipped light directions and the five planes of
        light-material interaction tags (datasets.py:363-485)."""
        return _ops.preprocess_sbmc(sample, self.max_depth)


def sample_flags(base_model, use_g_buf=True, use_sbmc_buf=True):
    """(base_model, use_g_buf, use_sbmc_buf) as ``DenoiseDataset.__init__`` resolves them (datasets.py:171-174, 198-199): 'lbmc' is
    'sbmc' with the g-buffer and without the SBMC buffers; only 'sbmc' reads the SBMC buffers."""
    if base_model not in ('kpcn', 'sbmc', 'lbmc'):
        raise RuntimeError("Unknown baseline model %s" % base_model)
    if base_model == 'lbmc':
        base_model, use_sbmc_buf, use_g_buf = 'sbmc', False, True
    if base_model != 'sbmc':
        use_sbmc_buf = False
    return base_model, bool(use_g_buf), bool(use_sbmc_buf)


def dncnn_in_size(base_model, use_g_buf, use_sbmc_buf, use_llpm_buf, pnet_out_size):
    """datasets.py:208-219, on flags already resolved by ``sample_flags``."""
    n = 34 if base_model == 'kpcn' else 3 + (21 if use_g_buf else 0) + (66 if use_sbmc_buf else 0)
    return n + (pnet_out_size + 2 if use_llpm_buf else 0)          # path weight, p-buffer, variance


class SamplePatchBatcher:
    """``PatchBatcher`` for the sample-based base models: the dictionary ``SBMCInterface`` / ``LBMCInterface`` assert on
    (``radiance``, ``features``, ``paths`` as (B, S, C, P, P) and ``target_image``; datasets.py:1045-1073, 1086-1118) in one launch
    of ``ops.assemble_sample_patches``."""

    def __init__(self, patch_size=128, batch_size=8, use_g_buf=True, use_sbmc_buf=True):
        self.patch_size, self.use_g_buf, self.use_sbmc_buf = patch_size, use_g_buf, use_sbmc_buf
        self.patches_per_image = (256 // batch_size) * batch_size          # datasets.py:275

    sample_origins = None                               # (bound below to PatchBatcher's: the same draw)

    def check_origins(self, origins, h, w):
        _ops.check_patch_origins(origins, h, w, self.patch_size, who="SamplePatchBatcher")

    def batch(self, sbmc_s, sbmc_p, llpm, gt, origins, check=True, spp=None, transforms=None):
        """``spp``: the first ``spp`` samples of the buffers (datasets.py:1053-1054, 1091); None: all of them.  ``transforms``: one
        dihedral code 0..7 per patch (``ops.check_patch_transforms``; checked with the origins) or None."""
        return _ops.assemble_sample_patches(sbmc_s, sbmc_p if self.use_sbmc_buf else None, llpm, gt, origins, self.patch_size,
                                            self.use_g_buf, self.use_sbmc_buf, check_origins=check, spp=spp, transforms=transforms)


class PatchBatcher:
    """KPCN-base-model batches straight from one image's device-resident buffers.

    ``sample_origins`` is the reference's importance sampling (``_sample_patches``, datasets.py:795-810): one
    ``np.random.choice`` over the flattened probability map (uniform if the map is not a distribution), so the same
    numpy seed yields the same patches; ``x = idx // w`` is the ROW and ``y = idx % w`` the column, as there.
    ``batch`` crops them and builds the dictionary ``KPCNInterface.preprocess`` asserts on (Appendix B of SURVEY.md) in
    one kernel launch (``ops.assemble_kpcn_patches``) -- 128 x 128 x 8 spp: 24.6 MB per patch that never visit the host.
    """
    PATCH_SIZE = 128                                # datasets.py:66

    def __init__(self, patch_size=PATCH_SIZE, batch_size=8):
        self.patch_size = patch_size
        self.patches_per_image = (256 // batch_size) * batch_size          # datasets.py:275

    def sample_origins(self, prob, n=None):
        h, w = prob.shape
        n = self.patches_per_image if n is None else n
        try:
            roi = np.random.choice(h * w, size=n, p=np.asarray(prob).reshape(h * w))
        except ValueError:
            roi = np.random.choice(h * w, size=n)
        return np.stack([roi // w, roi % w], axis=1).astype(np.int32)

    def check_origins(self, origins, h, w):
        """Windows must lie inside the image (the reference would silently return a smaller patch)."""
        _ops.check_patch_origins(origins, h, w, self.patch_size, who="PatchBatcher")

    def batch(self, kpcn, llpm, gt, origins, check=True, spp=None, transforms=None):
        """kpcn (H,W,44), llpm (H,W,S,37) or None, gt (H,W,9): device tensors; origins: (B,2) rows/columns (numpy or
        tensor).  ``check=False``: the caller has run ``check_origins`` on them (``PatchLoader`` does, once per image, on the
        host copy -- checking a device tensor here would synchronise every batch).  ``spp``: ``kpcn`` is the buffer of the first
        ``spp`` samples and the batch takes that prefix of ``llpm`` (datasets.py:1091); None: all of its samples.  ``transforms``: one
        dihedral code 0..7 per patch (``ops.check_patch_transforms``; ``check`` covers it too) or None."""
        if check:
            self.check_origins(origins, *kpcn.shape[:2])
        o = torch.as_tensor(np.asarray(origins), dtype=torch.int32) if not isinstance(origins, torch.Tensor) else origins
        return _ops.assemble_kpcn_patches(kpcn, llpm, gt, o.to(kpcn.device, torch.int32).contiguous(), self.patch_size, spp=spp,
                                          transforms=transforms, check_transforms=check)


SamplePatchBatcher.sample_origins = PatchBatcher.sample_origins


class FullImageDataset:
    """Device-side counterpart of the reference's ``FullImageDataset`` (``datasets.py:1174-1424``): the tiles of one full frame
    for evaluation (``test_models.py``), assembled on the GPU from the offline-preprocessed files.  With ``base_model`` 'sbmc' /
    'lbmc' the files are ``<scene>_sbmc_s.npy`` / ``_sbmc_p.npy`` (``/KPCN/`` -> ``/SBMC/``; continuation files as for ``_llpm``,
    :1323-1351) and the tiles are the sample-based dictionary of ``ops.assemble_sample_patches``; for 'kpcn':

    ``in_fn`` is ``.../input/<scene>.npy``; the files read are those of ``_load_full_buffer`` (:1319-1416):
      * ``<scene>_kpcn_<spp>.npy``  (H, W, 44) KPCN buffers;
      * ``<scene>_llpm.npy`` (+ ``_llpm_1.npy``, ``_llpm_2.npy``, ... until ``spp`` samples are there, ``_load_all_spp_buffer``
        :1302-1317), with ``/KPCN/`` -> ``/LLPM/`` in the path: (H, W, s, 37) path descriptors, read with --use_llpm_buf and
        always for ``has_hit``;
      * the target ``.../gt/<scene>.npy`` (H, W, 9).
    The reference's ``get_valid_path`` fallback across its lab's ``ssd*`` / ``hdd*`` mounts is left out: a missing file is a
    ``FileNotFoundError``.  Each file is uploaded once.

    Iteration yields ``(batch, i_start, j_start, i_end, j_end, i, j)`` per batch of tiles as the reference's DataLoader does
    (``batch``: the patch dictionary of ``wcmc_assemble_kpcn_patches`` on the device, the rest lists of ints), so
    ``support.inference.inference`` accepts it; ``tile_batches()`` yields ``(batch, coords)`` with the device (B, 6) int32
    tile table that ``support.inference.stitched_inference`` needs.  Batch size: 8 up to 32 spp, 4 up to 64
    (``test_models.py:147-161``).
    """
    KPCN, SBMC, LBMC = "kpcn", "sbmc", "lbmc"
    MAX_DEPTH = 5
    PATCH_SIZE = 128
    PAD_SIZE = 32
    SAMPLE_BASED = False                               # SampleFullImageDataset: accepts 'sbmc' / 'lbmc'

    def __init__(self, in_fn, spp, base_model='kpcn', use_g_buf=True, use_sbmc_buf=True, use_llpm_buf=False,
                 pnet_out_size=3, device=None, batch_size=None):
        import os
        from .inference import tile_coords
        asked = base_model
        base_model, use_g_buf, use_sbmc_buf = sample_flags(base_model, use_g_buf, use_sbmc_buf)      # datasets.py:1193-1196
        if asked != self.KPCN and not self.SAMPLE_BASED:
            raise NotImplementedError("FullImageDataset: only the KPCN base model is evaluated here; SampleFullImageDataset "
                                      "yields the tiles of the sample-based models ('sbmc' / 'lbmc'), whose base denoiser the "
                                      "caller supplies")
        assert os.sep + 'input' + os.sep in in_fn, in_fn
        if batch_size is None:
            if spp <= 32:
                batch_size = 8
            elif spp <= 64:
                batch_size = 4
            else:
                raise RuntimeError("Try higher spp after investigating your RAM and GRAM capacity.")
        self.device = torch.device(device if device is not None else torch.cuda.current_device())
        self.in_fn, self.spp, self.base_model, self.batch_size = in_fn, spp, base_model, batch_size
        self.gt_fn = in_fn.replace(os.sep + 'input' + os.sep, os.sep + 'gt' + os.sep)
        self.use_g_buf, self.use_sbmc_buf, self.use_llpm_buf = use_g_buf, use_sbmc_buf, use_llpm_buf
        self.pnet_in_size = 36 if use_llpm_buf else 0
        self.pnet_out_size = pnet_out_size
        self.dncnn_in_size = dncnn_in_size(base_model, use_g_buf, use_sbmc_buf, use_llpm_buf, pnet_out_size)

        stem, ext = in_fn[:in_fn.rfind('.')], in_fn[in_fn.rfind('.'):]
        llpm_fn = (stem + '_llpm' + ext).replace(os.sep + 'KPCN' + os.sep, os.sep + 'LLPM' + os.sep)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)   # noqa: E731

        def all_spp(fn, first=None):
            """``_load_all_spp_buffer`` (:1302-1317): ``fn``, then ``fn`` with _1, _2, ... until ``spp`` samples are there."""
            parts = [up(self._load(fn)) if first is None else first]
            n, i = parts[0].shape[2], 0
            while n < spp:
                i += 1
                parts.append(up(self._load(fn[:-4] + '_' + str(i) + '.npy')))
                n += parts[-1].shape[2]
            return (torch.cat(parts, dim=2) if len(parts) > 1 else parts[0])[:, :, :spp].contiguous()

        self.kpcn = self.sbmc_s = self.sbmc_p = None
        if base_model == self.KPCN:
            self.kpcn = up(self._load(stem + '_kpcn_' + str(spp) + ext))
        else:                                                    # datasets.py:1323-1351
            to_sbmc = lambda fn: fn.replace(os.sep + 'KPCN' + os.sep, os.sep + 'SBMC' + os.sep)      # noqa: E731
            self.sbmc_s = all_spp(to_sbmc(stem + '_sbmc_s' + ext))
            if use_sbmc_buf:
                self.sbmc_p = all_spp(to_sbmc(stem + '_sbmc_p' + ext))
        llpm0 = up(self._load(llpm_fn))
        self.gt = up(self._load(self.gt_fn))
        h, w = self.gt.shape[:2]
        self.h, self.w = h, w
        # datasets.py:1407-1414: the first llpm file, all its samples: bounce type of the first bounce (descriptor 24)
        hit = (llpm0[..., 1:].mean(2)[..., 24:25] != 0.0).float()
        self.has_hit = torch.cat((hit,) * 3, dim=2)
        self.llpm = all_spp(llpm_fn, llpm0) if use_llpm_buf else None
        del llpm0
        if base_model == self.KPCN:
            albedo = self.kpcn[..., 34:37] + 0.00316
            self.full_ipt = self.kpcn[..., :3] * albedo + torch.exp(self.kpcn[..., 10:13]) - 1      # datasets.py:1234
        else:
            self.full_ipt = self.sbmc_s[..., :3].mean(2)                                             # datasets.py:1248
        self.full_tgt = self.gt[..., 0:3]
        self.coords = tile_coords(h, w, self.PATCH_SIZE, self.PAD_SIZE)
        _ops.check_tile_coords(self.coords, h, w, self.PATCH_SIZE)
        self.coords_dev = torch.tensor(self.coords, dtype=torch.int32, device=self.device)
        self.origins_dev = self.coords_dev[:, 4:6].contiguous()

    @staticmethod
    def _load(fn):
        import os
        if not os.path.isfile(fn):
            raise FileNotFoundError(fn)
        return np.load(fn)

    def __len__(self):
        return len(self.coords)

    def num_batches(self):
        return (len(self.coords) + self.batch_size - 1) // self.batch_size

    def batch(self, k):
        """Tiles [k * batch_size, (k + 1) * batch_size): the patch dictionary (datasets.py:1296-1297 on the device) and the
        device tile table."""
        sl = slice(k * self.batch_size, (k + 1) * self.batch_size)
        if self.base_model == self.KPCN:
            batch = _ops.assemble_kpcn_patches(self.kpcn, self.llpm, self.gt, self.origins_dev[sl], self.PATCH_SIZE)
        else:                        # (the tile table passed ``check_tile_coords``: every tile lies inside the frame)
            batch = _ops.assemble_sample_patches(self.sbmc_s, self.sbmc_p, self.llpm, self.gt, self.origins_dev[sl], self.PATCH_SIZE,
                                                 self.use_g_buf, self.use_sbmc_buf, check_origins=False)
        return batch, self.coords_dev[sl]

    def tile_batches(self):
        for k in range(self.num_batches()):
            yield self.batch(k)

    def __iter__(self):
        for k in range(self.num_batches()):
            batch, _ = self.batch(k)
            cs = list(zip(*self.coords[k * self.batch_size:(k + 1) * self.batch_size]))
            yield (batch,) + tuple(list(c) for c in cs)


class SampleFullImageDataset(FullImageDataset):
    """``FullImageDataset`` for ``base_model`` 'sbmc' / 'lbmc' (``datasets.py:1193-1196, 1323-1351, 1364-1416``): the files of
    ``_load_full_buffer`` with ``has_hit``, tiles of the sample-based dictionary.  A class of its own because ``FullImageDataset``
    keeps refusing these models; ``evaluate.py`` picks this one for an SBMC / LBMC model name."""
    SAMPLE_BASED = True


# ------------------------------------------------------------------------------------------------- dataset directories
SHUFFLE_SEED = "Inyoung Cho, Yuchi Huo, Sungeui Yoon @ KAIST"          # datasets.py:270
TEST_SPPS = (2, 4, 8, 16, 32, 64)                                        # datasets.py:655
MAX_CONTINUATIONS = 7                                                    # datasets.py:632: <scene>_1.npy .. <scene>_7.npy


def shuffled_files(files):
    """The seeded shuffle of ``gt_files`` (datasets.py:269-271) on a private generator: ``random.seed(s); random.shuffle(x)``
    without touching the process-wide ``random`` state."""
    import random
    files = list(files)
    random.Random(SHUFFLE_SEED).shuffle(files)
    return files


def grid_origins(h, w, patch_size=PatchBatcher.PATCH_SIZE):
    """The (row, column) window origins of ``_full_patches`` (datasets.py:842-883), in its order.  Windows that start within
    ``patch_size`` of the bottom / right edge are ragged in the reference (it crops what is there)."""
    return np.array([(x, y) for x in range(0, h, patch_size) for y in range(0, w, patch_size)], dtype=np.int32).reshape(-1, 2)


def sanitized(a):
    """Host restatement of the NaN / Inf rule (datasets.py:623-624); ``ops.sanitize_`` is the device kernel."""
    a = np.asarray(a, dtype=np.float32)
    a = np.where(np.isfinite(a), a, np.float32(1.0e+38))
    return np.where(a < np.float32(1.0e+38), a, np.float32(1.0e+38)).astype(np.float32)


def multi_counts(spp):
    """The sample counts of ``MSDenoiseDataset(..., spp, ...)`` (datasets.py:1157-1171): 2..spp; below 2 its ``RuntimeError``."""
    if spp < 2:
        raise RuntimeError("spp too low to randomize sample count")
    return tuple(range(2, int(spp) + 1))


def check_counts(counts, s_total):
    """``counts`` as an ascending tuple of distinct sample counts in 1..s_total."""
    counts = tuple(int(s) for s in counts)
    if not counts or list(counts) != sorted(set(counts)) or counts[0] < 1 or counts[-1] > s_total:
        raise ValueError("counts must be ascending, distinct sample counts in 1..%d, got %s" % (s_total, counts))
    return counts


class _PendingProb:
    """What ``DenoiseDirectory.reader`` returns for 'prob' while ``_prob_imp.npy`` does not exist: ``staged_hook`` computes the
    map from the staged frame and writes ``fn``."""

    def __init__(self, fn):
        self.fn = fn


class DenoiseDirectory:
    """The directory and file layer of the reference's ``DenoiseDataset`` (``datasets.py:161-283, 584-715``) for the base model
    ``base_model`` ('kpcn', the default; 'sbmc'; 'lbmc' = 'sbmc' with the g-buffer and without the SBMC buffers): renderer output under ``<gt_base_dir>/<mode>/{gt,input}/<scene>.npy`` (gt (H, W, 9), input (H, W, S, 104)).

      * discovery: the ``.npy`` files of ``<mode>/gt`` in sorted order (``os.walk`` lists in the file system's order; sorting
        makes a run repeatable), then the reference's seeded shuffle (``shuffled_files``);
      * path rules, as ``FullImageDataset``: ``/gt/`` <-> ``/input/``, and ``/KPCN/`` -> ``/LLPM/`` for the ``_llpm`` files;
      * no ``get_valid_path`` fallback across mounts: a missing file is a ``FileNotFoundError``;
      * ``offline_preprocess`` writes what ``_offline_preprocess`` writes (the SBMC buffers with ``sbmc=True``), computed on the device;
      * ``reader`` / ``staged_hook`` feed ``support.loader.PatchLoader``; ``origins`` are the grid windows of validation.

    A directory is read at ``spp`` samples per pixel.  The reference's ``MSDenoiseDataset`` (datasets.py:1149-1171) -- every count
    2..spp -- is ``counts=`` of ``support.loader.PatchLoader`` and of ``grid_batches``: the frame is staged once at ``spp`` samples
    and every count comes out of it (``multi_counts``).
    """
    MAX_DEPTH = DenoisePreprocessor.MAX_DEPTH
    PATCH_SIZE = PatchBatcher.PATCH_SIZE

    def __init__(self, gt_base_dir, spp, mode='train', batch_size=8, sampling='random', use_llpm_buf=False, device=None,
                 pnet_out_size=3, patch_size=PATCH_SIZE, base_model='kpcn', use_g_buf=True, use_sbmc_buf=True):
        import os
        # 'lbmc' is 'sbmc' with use_sbmc_buf=False, use_g_buf=True (datasets.py:171-174)
        self.base_model, self.use_g_buf, self.use_sbmc_buf = sample_flags(base_model, use_g_buf, use_sbmc_buf)
        if mode not in ('train', 'val', 'test'):
            raise RuntimeError("Unknown training mode %s" % mode)
        if sampling not in ('random', 'grid'):
            raise RuntimeError("Unknown sampling mode %s" % sampling)
        self.gt_dir = os.path.join(gt_base_dir, mode, 'gt')
        if not os.path.isdir(self.gt_dir):
            raise FileNotFoundError(self.gt_dir)
        self.gt_files = shuffled_files(os.path.join(self.gt_dir, f) for f in sorted(os.listdir(self.gt_dir))
                                       if f.endswith('.npy') and os.path.isfile(os.path.join(self.gt_dir, f)))
        self.spp, self.batch_size, self.mode, self.sampling = spp, batch_size, mode, sampling
        self.use_llpm_buf, self.device, self.patch_size = use_llpm_buf, device, patch_size
        self.pnet_in_size = 36 if use_llpm_buf else 0                    # datasets.py:201-219
        self.pnet_out_size = pnet_out_size
        self.dncnn_in_size = dncnn_in_size(self.base_model, self.use_g_buf, self.use_sbmc_buf, use_llpm_buf, pnet_out_size)
        self.patches_per_image = (256 // batch_size) * batch_size if sampling == 'random' else 100      # datasets.py:273-279
        self.pre = DenoisePreprocessor(self.MAX_DEPTH)

    def __len__(self):
        return len(self.gt_files)

    # ---- names
    def paths(self, i):
        """The file names that belong to image ``i`` (datasets.py:602-607, :633-634): 'gt', 'in', 'llpm', 'prob', and the
        functions 'kpcn'(spp), 'in_k'(k), 'llpm_k'(k) of the per-spp and continuation files; 'sbmc_s' / 'sbmc_p' with ``/KPCN/`` ->
        ``/SBMC/`` (:1046-1049) and their continuation names 'sbmc_s_k'(k) / 'sbmc_p_k'(k)."""
        import os
        gt_fn = self.gt_files[i]
        in_fn = gt_fn.replace(os.sep + 'gt' + os.sep, os.sep + 'input' + os.sep)
        stem, ext = in_fn[:in_fn.rfind('.')], in_fn[in_fn.rfind('.'):]
        to_llpm = lambda fn: fn.replace(os.sep + 'KPCN' + os.sep, os.sep + 'LLPM' + os.sep)      # noqa: E731
        to_sbmc = lambda fn: fn.replace(os.sep + 'KPCN' + os.sep, os.sep + 'SBMC' + os.sep)      # noqa: E731
        return {'gt': gt_fn, 'in': in_fn, 'llpm': to_llpm(stem + '_llpm' + ext), 'prob': stem + '_prob_imp' + ext,
                'sbmc_s': to_sbmc(stem + '_sbmc_s' + ext), 'sbmc_p': to_sbmc(stem + '_sbmc_p' + ext),
                'sbmc_s_k': lambda k: to_sbmc(stem + '_sbmc_s_' + str(k) + ext),
                'sbmc_p_k': lambda k: to_sbmc(stem + '_sbmc_p_' + str(k) + ext),
                'kpcn': lambda s: stem + '_kpcn_' + str(s) + ext, 'in_k': lambda k: stem + '_' + str(k) + ext,
                'llpm_k': lambda k: to_llpm(stem + '_llpm_' + str(k) + ext)}

    @staticmethod
    def _load(fn, mmap=False):
        import os
        if not os.path.isfile(fn):
            raise FileNotFoundError(fn)
        return np.load(fn, mmap_mode='r' if mmap else None)

    def _main_raw(self, fn):
        """The main input file, memory-mapped and cut to ``spp`` samples; a file that holds fewer is an error (the reference
        would slice what is there and go on at another sample count than asked)."""
        a = self._load(fn, mmap=True)
        if a.ndim != 4 or a.shape[-1] != 104:
            raise ValueError("%s: shape %s is not renderer output (H, W, S, 104)" % (fn, tuple(a.shape)))
        if a.shape[2] < self.spp:
            raise ValueError("%s holds %d samples per pixel, fewer than the %d asked for (spp)" % (fn, a.shape[2], self.spp))
        return a[:, :, :self.spp]

    @staticmethod
    def _save(fn, arr):
        """Write through a temporary name: a reader never sees half a file."""
        import os
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        tmp = fn + '.tmp%d' % os.getpid()
        with open(tmp, 'wb') as f:
            np.save(f, arr)
        os.replace(tmp, fn)

    def _device(self):
        return torch.device(self.device if self.device is not None else torch.cuda.current_device())

    def _upload(self, a):
        """Host array (a read-only memory map included: it is read into memory first) -> sanitised contiguous fp32 device tensor."""
        a = np.ascontiguousarray(a, dtype=np.float32) if a.flags.writeable else np.array(a, dtype=np.float32, order='C')
        return _ops.sanitize_(torch.from_numpy(a).to(self._device()))

    # ---- offline writer
    def offline_preprocess(self, llpm=True, kpcn=True, overwrite=False, report=None, sbmc=False):
        """``_offline_preprocess`` (datasets.py:584-715).  ``sbmc=True`` writes ``_sbmc_s.npy`` / ``_sbmc_p.npy`` (:643-651) from the
        main file cut to ``spp`` -- in the test mode too, where the reference raises ``NameError`` (it computes the buffers outside
        the test mode only) -- and, an addition, ``_sbmc_s_<k>.npy`` / ``_sbmc_p_<k>.npy`` for the continuation files that exist:
        ``_load_all_spp_buffer`` (:1302-1317) expects them beside ``_llpm_<k>.npy``.  Per scene: ``_llpm.npy`` (and ``_llpm_<k>.npy``
        for the continuation files ``<scene>_<k>.npy`` that exist, k = 1..7), ``_kpcn_<s>.npy`` for s in 2..spp (train / val) or the
        s of 2, 4, 8, 16, 32, 64 that the samples on disk reach (test), the gt file sanitised, and ``_prob_imp.npy`` outside the
        test mode.  A file that exists is kept unless ``overwrite``; a scene whose files all exist is not read at all.  Each raw
        file is uploaded once.  Returns ``[(scene, [files written], seconds)]`` and calls ``report`` with each entry."""
        import os
        import time
        done = []
        for i in range(len(self.gt_files)):
            t0 = time.time()
            p = self.paths(i)
            written = []
            if not os.path.isfile(p['in']):
                raise FileNotFoundError(p['in'])
            want = lambda fn: overwrite or not os.path.isfile(fn)                                   # noqa: E731
            conts = []
            for k in range(1, MAX_CONTINUATIONS + 1):               # a missing continuation file ends the series
                if not os.path.isfile(p['in_k'](k)):
                    break
                conts.append(k)
            uploaded = {}

            def raw(k):
                """Sanitised device samples of the main file cut to spp (k = 0) or of continuation file k, uploaded once."""
                if k not in uploaded:
                    a = self._main_raw(p['in']) if k == 0 else self._load(p['in_k'](k), mmap=True)
                    assert a.shape[-1] == 104, 'input numpy file is not produced by OptaGen'
                    uploaded[k] = self._upload(a)
                return uploaded[k]

            if llpm:
                if want(p['llpm']):
                    self._save(p['llpm'], self.pre._preprocess_llpm(raw(0)).cpu().numpy())
                    written.append(p['llpm'])
                for k in conts:
                    if want(p['llpm_k'](k)):
                        self._save(p['llpm_k'](k), self.pre._preprocess_llpm(raw(k)).cpu().numpy())
                        written.append(p['llpm_k'](k))
            if sbmc:
                for k in [0] + conts:
                    fs, fp = (p['sbmc_s'], p['sbmc_p']) if k == 0 else (p['sbmc_s_k'](k), p['sbmc_p_k'](k))
                    if want(fs) or want(fp):
                        bs, bp = self.pre._preprocess_sbmc(raw(k))
                        for fn, buf in ((fs, bs), (fp, bp)):
                            if want(fn):
                                self._save(fn, buf.cpu().numpy())
                                written.append(fn)
            if kpcn:
                # samples on disk, read once per scene: the main file's first spp (it holds at least spp), then the
                # continuation files in order
                counts = {0: self._main_raw(p['in']).shape[2]}
                counts.update((k, self._load(p['in_k'](k), mmap=True).shape[2]) for k in conts)
                for s in (TEST_SPPS if self.mode == 'test' else range(2, self.spp + 1)):
                    parts, have = [0], counts[0]
                    for k in conts:
                        if have >= s:
                            break
                        parts.append(k)
                        have += counts[k]
                    if have < s:
                        break                                       # (test mode: a missing continuation file ends the series)
                    if want(p['kpcn'](s)):
                        x = raw(0) if len(parts) == 1 else torch.cat([raw(k) for k in parts], dim=2)
                        self._save(p['kpcn'](s), self.pre._preprocess_kpcn(x[:, :, :s].contiguous()).cpu().numpy())
                        written.append(p['kpcn'](s))
            # target: rewritten when it is not yet the sanitised fp32 array (the reference rewrites it on every visit)
            gt = self._load(p['gt'])
            clean = gt.dtype == np.float32 and bool(np.all(np.isfinite(gt))) and bool(np.all(gt <= np.float32(1.0e+38)))
            gt_dev = None
            if overwrite or not clean:
                gt_dev = self._upload(gt)
                self._save(p['gt'], gt_dev.cpu().numpy())
                written.append(p['gt'])
            if self.mode != 'test' and want(p['prob']):
                gt_dev = self._upload(gt) if gt_dev is None else gt_dev
                self._save(p['prob'], _ops.sampling_prob(raw(0), gt_dev, self.patch_size, self.MAX_DEPTH).cpu().numpy())
                written.append(p['prob'])
            uploaded.clear()
            entry = (os.path.basename(p['in'])[:-4], written, time.time() - t0)
            done.append(entry)
            if report is not None:
                report(entry)
        return done

    # ---- loader side
    def reader(self, i):
        """``reader(i)`` of ``support.loader.PatchLoader``: raw memory-mapped and cut to ``[:, :, :spp]``, gt from its file, prob from
        ``_prob_imp.npy`` -- or, while that file does not exist, a marker that ``staged_hook`` resolves on the device."""
        import os
        p = self.paths(i)
        raw = self._main_raw(p['in'])
        gt = self._load(p['gt'])
        prob = _PendingProb(p['prob'])
        if os.path.isfile(p['prob']):
            prob = np.load(p['prob'])
            want = (gt.shape[0] - self.patch_size, gt.shape[1] - self.patch_size)
            if prob.shape != want:
                raise ValueError("%s has shape %s; a %d x %d image and patch size %d need %s -- it was written for another patch "
                                 "size: rewrite it (python -m wcmc_amd.preprocess --patch_size %d --overwrite) or delete it"
                                 % (p['prob'], tuple(prob.shape), gt.shape[0], gt.shape[1], self.patch_size, want,
                                    self.patch_size))
        return {'raw': raw, 'gt': gt, 'prob': prob}

    def staged_hook(self, d_raw, d_gt, prob):
        """``ImageStager``'s hook on the copy stream, before the preprocessing kernels: the frame is sanitised in place as the
        offline writer does, and a missing probability map is computed from it and written."""
        _ops.sanitize_(d_raw)
        _ops.sanitize_(d_gt)
        if isinstance(prob, _PendingProb):
            arr = _ops.sampling_prob(d_raw, d_gt, self.patch_size, self.MAX_DEPTH).cpu().numpy()
            self._save(prob.fn, arr)
            prob = arr
        return prob

    def origins(self, i):
        """Window origins of image ``i``: the grid of ``_full_patches`` for ``sampling='grid'`` (validation)."""
        if self.sampling != 'grid':
            raise RuntimeError("origins(i) is the grid of sampling='grid'; 'random' origins are drawn from the probability map")
        h, w = self._load(self.gt_files[i], mmap=True).shape[:2]
        return grid_origins(h, w, self.patch_size)

    def grid_batches(self, indices=None, batch_size=None, counts=None):
        """Validation batches: every WHOLE window of the grid (the reference's ragged edge windows cannot be batched), image by
        image, ``batch_size`` at a time.  ``counts``: per image, the grid at every one of these sample counts (ascending) from one
        upload and one prefix pass -- image-major, where ``MSDenoiseDataset`` walks all images per count: validation sums its
        batches, so the order does not matter."""
        counts = None if counts is None else check_counts(counts, self.spp)
        bs = self.batch_size if batch_size is None else batch_size
        sample_based = self.base_model == 'sbmc'
        batcher = SamplePatchBatcher(self.patch_size, bs, self.use_g_buf, self.use_sbmc_buf) if sample_based \
            else PatchBatcher(self.patch_size, bs)
        for i in (range(len(self)) if indices is None else indices):
            item = self.reader(i)
            d_raw, d_gt = self._upload(item['raw']), self._upload(item['gt'])
            h, w = d_gt.shape[:2]
            o = self.origins(i)
            o = o[(o[:, 0] + self.patch_size <= h) & (o[:, 1] + self.patch_size <= w)]
            if len(o) == 0:
                raise ValueError("DenoiseDirectory: the %d x %d image %s holds no whole %d-pixel window"
                                 % (h, w, self.gt_files[i], self.patch_size))
            ll = self.pre._preprocess_llpm(d_raw) if self.use_llpm_buf else None
            if sample_based:
                ss, sp = self.pre._preprocess_sbmc(d_raw)
                for s in ([None] if counts is None else counts):
                    for k in range(0, len(o), bs):
                        yield batcher.batch(ss, sp, ll, d_gt, o[k:k + bs], spp=s)
                continue
            if counts is None:
                kp = self.pre._preprocess_kpcn(d_raw)
                for k in range(0, len(o), bs):
                    yield batcher.batch(kp, ll, d_gt, o[k:k + bs])
                continue
            slabs = self.pre._preprocess_kpcn_prefix(d_raw, counts[0], counts[-1])
            for s in counts:
                for k in range(0, len(o), bs):
                    yield batcher.batch(slabs[s - counts[0]], ll, d_gt, o[k:k + bs], spp=s)

    def num_grid_batches(self, indices=None, batch_size=None, counts=None):
        bs = self.batch_size if batch_size is None else batch_size
        return self._num_grid_batches(indices, bs) * (1 if counts is None else len(check_counts(counts, self.spp)))

    def _num_grid_batches(self, indices, bs):
        n = 0
        for i in (range(len(self)) if indices is None else indices):
            h, w = self._load(self.gt_files[i], mmap=True).shape[:2]
            o = self.origins(i)
            n += -(-int(((o[:, 0] + self.patch_size <= h) & (o[:, 1] + self.patch_size <= w)).sum()) // bs)
        return n
