"""Streaming a frame to the device in row bands (csrc/preprocess.hip: wcmc_preprocess_kpcn_begin / _rows / _end; support.staging;
wcmc_amd.denoise), held bit for bit -- through an int32 view, so that NaNs compare -- against the whole-frame route that stays in
the tree: ``ops.preprocess_kpcn`` / ``ops.preprocess_llpm`` of the frame at the kernel level, ``denoise.upload_raw`` +
``DenoisePreprocessor`` at the streamer's, the files of a run without ``--band_rows`` at the command line's."""
import functools
import os
import threading

import numpy as np
import pytest
import torch

from data_ref import cmap, make_frame

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPLITS = ([7], [1] * 7, [3, 4], [5, 2])
DEPTH_CASES = ("max_in_last_pixel", "max_in_first_pixel", "none_positive", "overflowing_mean")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).nonzero()
        raise AssertionError("%s differs at %d entries, channels %s, first %s"
                             % (what, len(bad), sorted(set(bad[:, -1].tolist())), bad[0].tolist()))


def _merged(h, w, s, seed):
    """Raw renderer output: the kpcn and the llpm channels of ``data_ref.make_frame``; the channels neither function reads stay NaN."""
    a, b = make_frame(h, w, s, seed=seed, fill="kpcn"), make_frame(h, w, s, seed=seed + 1, fill="llpm")
    return torch.where(torch.isnan(a), b, a)


def _raw(h, w, s, seed):
    """Unsanitised raw renderer output on the host: ``_merged`` with a few of the read values Inf / NaN (what ``sanitize_`` is for)."""
    x, m = _merged(h, w, s, seed), cmap()
    x[h // 2, w // 3, 0, 3], x[h - 1, 0, s - 1, m["albedo"]], x[0, w - 1, 0, m["pweight"]] = float("inf"), float("nan"), float("inf")
    return x.numpy()


@functools.lru_cache(maxsize=None)
def _small(s, depth_case=None):
    """A 7 x 5 frame on the device, taken as it is (3e38 must stay 3e38), with its whole-frame (kpcn, llpm); computed once."""
    from wcmc_amd import ops
    h, w = 7, 5
    x = _merged(h, w, s, seed=10 + s)
    d = x[..., cmap()["depth"]]                                      # (a view)
    if depth_case is not None:
        d.copy_(torch.rand((h, w, s), generator=torch.Generator().manual_seed(3)) * 40.0)
    if depth_case == "max_in_last_pixel":
        d[h - 1, w - 1] = 2e4
    elif depth_case == "max_in_first_pixel":
        d[0, 0] = 2e4
    elif depth_case == "none_positive":
        d.neg_()
        d[2, 1] = 0.0
    elif depth_case == "overflowing_mean":
        d[3, 2, :2] = 3e38
    raw = x.to(DEV)
    return raw, ops.preprocess_kpcn(raw), ops.preprocess_llpm(raw)


def _in_bands(raw, split, offset=0):
    """(kpcn, llpm) of the frame ``raw`` through begin / rows / end and ``preprocess_llpm(out=rows)``, in bands of ``split`` rows, each
    band a fresh tensor of its own (``offset``: starting that many floats into its allocation)."""
    from wcmc_amd import ops
    h, w, s, c = raw.shape
    assert sum(split) == h
    kpcn, ws = ops.preprocess_kpcn_begin(h, w, raw.device)
    kpcn.fill_(float("nan"))                                         # every entry must be written
    llpm = torch.full((h, w, s, 37), float("nan"), device=raw.device)
    row0 = 0
    for rows in split:
        flat = torch.empty(rows * w * s * c + offset, device=raw.device)
        band = flat[offset:].view(rows, w, s, c)
        band.copy_(raw[row0:row0 + rows])
        assert band.data_ptr() % 16 == (4 * offset) % 16 and band.is_contiguous()
        ops.preprocess_kpcn_rows(band, row0, kpcn, ws)
        got = ops.preprocess_llpm(band, out=llpm[row0:row0 + rows])
        assert got.data_ptr() == llpm[row0:row0 + rows].data_ptr()
        row0 += rows
    return ops.preprocess_kpcn_end(kpcn, ws, s), llpm


@pytest.mark.parametrize("split", SPLITS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("s", (2, 3))                                # the lanes kernel and the per-pixel one
def test_bands_equal_the_whole_frame(s, split):
    raw, kpcn, llpm = _small(s)
    got_k, got_l = _in_bands(raw, split)
    _assert_bits(got_k, kpcn, "kpcn")
    _assert_bits(got_l, llpm, "llpm")
    assert float(kpcn[..., 30].max()) == 1.0                         # a normalised depth: the bands did meet


@pytest.mark.parametrize("split", SPLITS, ids=lambda v: "x".join(map(str, v)))
def test_unaligned_bands_equal_the_whole_frame(split):
    """Every band starts one float into its allocation: the lanes kernel without vector loads, the generic llpm kernel."""
    raw, kpcn, llpm = _small(2)
    got_k, got_l = _in_bands(raw, split, offset=1)
    _assert_bits(got_k, kpcn, "kpcn")
    _assert_bits(got_l, llpm, "llpm")


@pytest.mark.parametrize("case", DEPTH_CASES)
@pytest.mark.parametrize("s", (2, 3))
def test_depth_maximum_across_bands(s, case):
    """The one place where bands interact: the image maximum of the mean depth, found by whichever band holds it."""
    raw, kpcn, llpm = _small(s, case)
    depth = kpcn[..., 30]
    if case == "max_in_last_pixel":
        assert float(depth[-1, -1]) == 1.0 and float(depth.flatten()[:-1].max()) < 0.01
    elif case == "max_in_first_pixel":
        assert float(depth[0, 0]) == 1.0 and float(depth.flatten()[1:].max()) < 0.01
    elif case == "none_positive":
        assert float(depth.abs().max()) == 0.0 and float(kpcn[..., 31].max()) > 1.0    # clipped, and a variance nobody scaled
    else:
        # the mean of the pixel overflows: the maximum is Inf, the pixel's depth Inf / Inf, every other depth finite / Inf = 0
        assert bool(torch.isnan(depth[3, 2])) and int(torch.isnan(depth).sum()) == 1 and float(depth.nan_to_num(0.0).abs().max()) == 0.0
    for split in SPLITS:
        got_k, _ = _in_bands(raw, split)
        _assert_bits(got_k, kpcn, "kpcn (%s, bands of %s rows)" % (case, split))


def test_band_ops_refuse_what_does_not_fit():
    from wcmc_amd import ops
    raw, _, _ = _small(2)
    kpcn, ws = ops.preprocess_kpcn_begin(7, 5, raw.device)
    for row0, band in ((5, raw[:3]), (-1, raw[:2]), (7, raw[:1])):
        with pytest.raises(RuntimeError, match="are not rows of the 7-row frame"):
            ops.preprocess_kpcn_rows(band.contiguous(), row0, kpcn, ws)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.preprocess_kpcn_rows(raw[:2].contiguous(), 0, kpcn, ws[:-1])
    with pytest.raises(ValueError, match="out should be"):
        ops.preprocess_llpm(raw[:2].contiguous(), out=torch.empty((3, 5, 2, 37), device=raw.device))


# ------------------------------------------------------------------------------------------------- the streamer
@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    """scene.npy (70 x 83, 2 samples) + scene_1.npy (1 more), small.npy (64 x 64 x 2) and large.npy (128 x 150 x 2)."""
    d = tmp_path_factory.mktemp("renders")
    np.save(d / "scene.npy", _raw(70, 83, 2, seed=1))
    np.save(d / "scene_1.npy", _raw(70, 83, 1, seed=5))
    np.save(d / "small.npy", _raw(64, 64, 2, seed=7))
    np.save(d / "large.npy", _raw(128, 150, 2, seed=9))
    return d


@functools.lru_cache(maxsize=None)
def _whole_frame_route(fn, spp):
    """(kpcn, llpm) of the frame by ``upload_raw`` + ``DenoisePreprocessor``; computed once per frame."""
    from wcmc_amd import denoise
    from wcmc_amd.support.datasets import DenoisePreprocessor
    parts, _ = denoise.read_raw(fn, spp)
    raw = denoise.upload_raw(parts, torch.device(DEV))
    pre = DenoisePreprocessor()
    return pre._preprocess_kpcn(raw), pre._preprocess_llpm(raw)


def _stream(files, spp, **kw):
    from wcmc_amd.support.staging import FrameStreamer
    frames = FrameStreamer(files, spp, DEV, **kw)
    try:
        out = [(k.clone(), ll.clone()) for k, ll in frames]
    finally:
        frames.close()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("band_rows", (1, 16, 64, 70, None))
@pytest.mark.parametrize("spp", (2, 3))                              # 3: the third sample comes from the continuation file
def test_streamer_equals_the_whole_frame_route(renders, spp, band_rows):
    fn = str(renders / "scene.npy")
    want_k, want_l = _whole_frame_route(fn, spp)
    before = threading.active_count()
    (got_k, got_l), = _stream([fn], spp, band_rows=band_rows)
    assert got_k.shape == (70, 83, 44) and got_l.shape == (70, 83, spp, 37)
    _assert_bits(got_k, want_k, "kpcn")
    _assert_bits(got_l, want_l, "llpm")
    assert threading.active_count() == before


def test_frames_of_different_size_in_one_streamer(renders):
    files = [str(renders / "small.npy"), str(renders / "scene.npy")]
    both = _stream(files, 2, band_rows=16)
    assert [tuple(k.shape) for k, _ in both] == [(64, 64, 44), (70, 83, 44)]
    for fn, (got_k, got_l) in zip(files, both):
        (alone_k, alone_l), = _stream([fn], 2, band_rows=16)
        _assert_bits(got_k, alone_k, "kpcn of " + os.path.basename(fn))
        _assert_bits(got_l, alone_l, "llpm of " + os.path.basename(fn))
        want_k, want_l = _whole_frame_route(fn, 2)
        _assert_bits(got_k, want_k, "kpcn of " + os.path.basename(fn))
        _assert_bits(got_l, want_l, "llpm of " + os.path.basename(fn))


def test_streamer_errors_surface_and_an_early_leave_stops_the_threads(renders):
    from wcmc_amd.support.staging import FrameStreamer, copy_stream
    a, b = FrameStreamer([str(renders / "small.npy")], 2, DEV), FrameStreamer([str(renders / "small.npy")], 2, DEV)
    assert a.copy_stream is b.copy_stream is copy_stream(DEV)         # one copy stream per device, however many streamers
    del a, b
    before = threading.active_count()
    files = [str(renders / "small.npy"), str(renders / "scene.npy"), str(renders / "small.npy")]
    for k, ll in FrameStreamer(files, 2, DEV, band_rows=4):
        break                                                        # the iterator is dropped here: its threads must go
    assert k.shape == (64, 64, 44)
    del k, ll
    assert threading.active_count() == before
    # small.npy holds two samples and has no continuation file: the reader's error reaches the consumer, after the first frame
    frames = FrameStreamer([str(renders / "scene.npy"), str(renders / "small.npy")], 3, DEV)
    assert next(frames)[1].shape == (70, 83, 3, 37)
    with pytest.raises(ValueError, match=r"fewer than the 3 asked for \(--spp\)"):
        next(frames)
    assert threading.active_count() == before


def test_device_memory_stays_within_the_buffers_and_two_bands(renders):
    """128 x 150 x 2 in bands of 8 rows: kpcn + llpm + workspace + two bands + 1 MiB (12.2 MB); the raw frame alone is 16 MB."""
    from wcmc_amd._lib import lib
    from wcmc_amd.support.staging import FrameStreamer
    h, w, s = 128, 150, 2
    fn = str(renders / "large.npy")
    want_k, want_l = _whole_frame_route(fn, s)
    band = 8 * w * s * 104 * 4
    assert band == 998400
    bound = h * w * 44 * 4 + h * w * s * 37 * 4 + lib().wcmc_preprocess_kpcn_workspace_bytes(h, w) + 2 * band + (1 << 20)
    assert bound < h * w * s * 104 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    frames = FrameStreamer([fn], s, DEV, band_rows=8)
    kpcn, llpm = next(frames)
    frames.close()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak device memory of the streamed frame: %d B over the start (bound %d B, raw frame %d B); pinned ring %d B"
          % (rise, bound, h * w * s * 104 * 4, frames.ring.peak_nbytes))
    _assert_bits(kpcn, want_k, "kpcn")
    _assert_bits(llpm, want_l, "llpm")
    assert rise <= bound
    assert 0 < frames.ring.peak_nbytes <= (4 + 2) * band and frames.ring.nbytes() == 0      # pinned: workers + 2 bands, given back on close


# ------------------------------------------------------------------------------------------------- the command line
def _args(save, extra=()):
    from wcmc_amd import denoise
    return denoise.build_parser().parse_args(
        ["--save", save, "--model_name", "KPCN_denoise_test", "--input", "unused", "--output_dir", "unused", "--use_llpm_buf",
         "--manif_learn", "--manif_loss", "FMSE", "--train_branches"] + list(extra))


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """A fresh KPCN-Manifold checkpoint, made as tests/test_gpu_denoise.py makes its own."""
    from wcmc_amd import train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    save = str(tmp_path_factory.mktemp("weights"))
    args = _args(save)
    torch.manual_seed(0)
    sizes = {"dncnn_in_size": 34 + 3 + 2, "pnet_in_size": 36, "pnet_out_size": 3}
    itfs, _ = train_kpcn.init_model(sizes, args, torch.device(DEV))
    torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, "KPCN_denoise_test.pth"))
    return save


FILES = ("_denoised.npy", "_denoised.pfm", "_denoised.png", "_input.png", "_pbuffer.npy")


def test_command_line_writes_the_same_bytes_with_and_without_band_rows(renders, checkpoint, tmp_path):
    from wcmc_amd import denoise
    from wcmc_amd.support.datasets import DenoisePreprocessor
    from wcmc_amd.support.inference import denoise_frame
    scene, small = str(renders / "scene.npy"), str(renders / "small.npy")

    def run(out, inputs, extra):
        times = denoise.main(["--input"] + inputs + ["--output_dir", str(tmp_path / out), "--save", checkpoint, "--model_name",
                                                     "KPCN_denoise_test", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE",
                                                     "--train_branches", "--png", "--save_pbuffer"] + extra)
        assert len(times) == len(inputs) and all({"upload", "preprocess", "network", "finish", "write"} <= set(t) for t in times)
        return {name: open(tmp_path / out / name, "rb").read() for name in sorted(os.listdir(tmp_path / out))}
    one_banded = run("a", [scene], ["--band_rows", "16"])
    two_banded = run("b", [small, scene], ["--band_rows", "16"])
    two_default = run("c", [small, scene], [])
    assert sorted(one_banded) == sorted("scene" + f for f in FILES)
    assert sorted(two_banded) == sorted(two_default) == sorted(stem + f for stem in ("scene", "small") for f in FILES)
    for name, data in two_default.items():
        assert two_banded[name] == data, name
        if name.startswith("scene"):
            assert one_banded[name] == data, name
    # ... and those bytes are the whole-frame route's image
    itf = denoise.load_interface(_args(checkpoint), torch.device(DEV))
    for stem, fn in (("scene", scene), ("small", small)):
        raw = denoise.upload_raw(denoise.read_raw(fn)[0], torch.device(DEV))
        pre = DenoisePreprocessor()
        out = denoise_frame(itf, pre._preprocess_kpcn(raw), pre._preprocess_llpm(raw), True, 8, want_pbuffers=True, preview=True)[0]
        img = np.load(tmp_path / "c" / (stem + "_denoised.npy"))
        assert img.dtype == np.float32 and np.array_equal(img.view(np.int32), out.cpu().numpy().view(np.int32)), stem
