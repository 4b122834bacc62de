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
        o = origins.cpu().numpy() if isinstance(origins, torch.Tensor) else np.asarray(origins)
        if o.size and (int(o[:, 0].max()) + self.patch_size > h or int(o[:, 1].max()) + self.patch_size > w or int(o.min()) < 0):
            raise ValueError("PatchBatcher: a %d-pixel patch origin lies outside the %dx%d image" % (self.patch_size, h, w))

    def batch(self, kpcn, llpm, gt, origins, check=True):
        """kpcn (H,W,44), llpm (H,W,S,37) or None, gt (H,W,9): device tensors; origins: (B,2) rows/columns (numpy or
        tensor).  ``check=False``: the caller has run ``check_origins`` on them (``PatchLoader`` does, once per image, on the
        host copy -- checking a device tensor here would synchronise every batch)."""
        if check:
            self.check_origins(origins, *kpcn.shape[:2])
        o = torch.as_tensor(np.asarray(origins), dtype=torch.int32) if not isinstance(origins, torch.Tensor) else origins
        return _ops.assemble_kpcn_patches(kpcn, llpm, gt, o.to(kpcn.device, torch.int32).contiguous(), self.patch_size)


class FullImageDataset:
    """Device-side counterpart of the reference's ``FullImageDataset`` (``datasets.py:1174-1424``) for the KPCN base model: the
    tiles of one full frame for evaluation (``test_models.py``), assembled on the GPU from the offline-preprocessed files.

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

    def __init__(self, in_fn, spp, base_model='kpcn', use_g_buf=True, use_sbmc_buf=True, use_llpm_buf=False,
                 pnet_out_size=3, device=None, batch_size=None):
        import os
        from .inference import tile_coords
        if base_model not in (self.KPCN, self.SBMC, self.LBMC):
            raise RuntimeError("Unknown baseline model %s" % base_model)
        if base_model != self.KPCN:
            raise NotImplementedError("FullImageDataset: only the KPCN base model is evaluated here (the SBMC / LBMC base "
                                      "denoisers are stand-ins in this build)")
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
        self.dncnn_in_size = 34 + (pnet_out_size + 2 if use_llpm_buf else 0)

        stem, ext = in_fn[:in_fn.rfind('.')], in_fn[in_fn.rfind('.'):]
        kpcn_fn = stem + '_kpcn_' + str(spp) + ext
        llpm_fn = (stem + '_llpm' + ext).replace(os.sep + 'KPCN' + os.sep, os.sep + 'LLPM' + os.sep)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)   # noqa: E731
        self.kpcn = up(self._load(kpcn_fn))
        llpm0 = up(self._load(llpm_fn))
        self.gt = up(self._load(self.gt_fn))
        h, w = self.kpcn.shape[:2]
        self.h, self.w = h, w
        # datasets.py:1407-1414: the first llpm file, all its samples: bounce type of the first bounce (descriptor 24)
        hit = (llpm0[..., 1:].mean(2)[..., 24:25] != 0.0).float()
        self.has_hit = torch.cat((hit,) * 3, dim=2)
        self.llpm = None
        if use_llpm_buf:
            parts, s, i = [llpm0], llpm0.shape[2], 0
            while s < spp:                                       # _load_all_spp_buffer
                i += 1
                parts.append(up(self._load(llpm_fn[:-4] + '_' + str(i) + '.npy')))
                s += parts[-1].shape[2]
            self.llpm = (torch.cat(parts, dim=2) if len(parts) > 1 else llpm0)[:, :, :spp].contiguous()
        del llpm0
        albedo = self.kpcn[..., 34:37] + 0.00316
        self.full_ipt = self.kpcn[..., :3] * albedo + torch.exp(self.kpcn[..., 10:13]) - 1      # datasets.py:1234
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
        batch = _ops.assemble_kpcn_patches(self.kpcn, self.llpm, self.gt, self.origins_dev[sl], self.PATCH_SIZE)
        return batch, self.coords_dev[sl]

    def tile_batches(self):
        for k in range(self.num_batches()):
            yield self.batch(k)

    def __iter__(self):
        for k in range(self.num_batches()):
            batch, _ = self.batch(k)
            cs = list(zip(*self.coords[k * self.batch_size:(k + 1) * self.batch_size]))
            yield (batch,) + tuple(list(c) for c in cs)
