"""Denoising a render of any size with a trained SBMC / LBMC model (csrc/sbmc_data.hip: wcmc_assemble_sample_tiles; csrc/frame_tiles.hip:
wcmc_finish_sample_frame; support.inference.denoise_sample_frame; the sample-based mode of support.staging.FrameStreamer;
wcmc_amd.denoise).

The tiles of the mirror-extended frame are held bit for bit against the route that exists without them -- the per-sample buffers of
the ``np.pad(raw, 'symmetric')`` frame and ``assemble_sample_patches`` at shifted origins --, ``finish_sample_frame`` against torch and
fp64 restatements, the ownership of the tiles with a stand-in that returns the tile's index, a real interface around
``standins.SampleDenoiserStandIn`` (3x3 valid chain: 124-pixel outputs, so the replicate padding runs) against the same kernels driven
through the slice loop of ``support.inference.inference``, the streamer against whole-frame preprocessing, and the command line on a
directory that holds nothing but a raw frame and a checkpoint."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATCH, PAD = 128, 32
SIZES = [(64, 64), (70, 83)]       # one tile mirrored on four sides; clamped last tiles, chunks that straddle both edges, odd width
SPPS = [2, 5]                      # one partial chunk of samples; a full chunk of four and a chunk of one
FLAGS = [(True, True, True), (True, False, True), (True, False, False), (False, True, False)]     # (use_g_buf, use_sbmc_buf, llpm)
BOUNCE = 60                        # raw channel of the first bounce's type (24 + 6 * (MAX_DEPTH + 1)): descriptor 24 of `paths`


def _raw_frame(h, w, s, seed=0):
    """Raw renderer output (h, w, s, 104) on the host, no two records equal: channel 0 (the subpixel offset, which sbmc_s carries
    verbatim) numbers the records, the other channels preprocess_sbmc reads are random in [-0.5, 1.5) (both sides of every clamp) and
    those behind them random in [0, 1.5), the bounce types are integer codes 1..31, and the first bounce's type is zero in every sample on about 10 % of the pixels."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((h, w, s, 104), generator=g) * 2.0 - 0.5
    x[..., 66:] = x[..., 66:].abs()                               # what preprocess_llpm takes logarithms and roots of
    x[..., 0] = (torch.arange(h * w * s, dtype=torch.float32) / (h * w * s)).view(h, w, s)
    x[..., BOUNCE:BOUNCE + 6] = torch.randint(1, 32, (h, w, s, 6), generator=g).float()
    miss = torch.rand((h, w), generator=g) < 0.1
    x[..., BOUNCE][miss] = 0.0
    return x.numpy()


def _buffers(raw):
    from wcmc_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(raw)).to(DEV)
    return ops.preprocess_sbmc(t) + (ops.preprocess_llpm(t),)


@functools.lru_cache(maxsize=None)
def _frame(h, w, s):
    """(raw on the host, (sbmc_s, sbmc_p, llpm) of the frame, the same of its symmetric-padded raw frame + a zero gt); computed once."""
    raw = _raw_frame(h, w, s, seed=h * 1000 + w + s)
    padded = np.pad(raw, ((PAD, PAD), (PAD, PAD), (0, 0), (0, 0)), "symmetric")
    gt0 = torch.zeros((h + 2 * PAD, w + 2 * PAD, 9), device=DEV)
    return raw, _buffers(raw), _buffers(padded) + (gt0,)


def _origins(table):
    return torch.tensor([t[4:6] for t in table], dtype=torch.int32, device=DEV)


def _assert_entries_equal(got, want, keys):
    assert set(got) == set(keys)
    for k in sorted(got):
        assert got[k].data_ptr() % 256 == 0 and got[k].shape == want[k].shape, k
        assert bool(torch.isfinite(want[k]).all()), k
        if not torch.equal(got[k], want[k]):
            bad = (got[k] != want[k]).nonzero()
            raise AssertionError("%s differs at %d entries, channels %s, first %s"
                                 % (k, len(bad), sorted(set(bad[:, 2].tolist())), bad[0].tolist()))


@pytest.mark.parametrize("g_buf,p_buf,with_llpm", FLAGS)
@pytest.mark.parametrize("s", SPPS)
@pytest.mark.parametrize("h,w", SIZES)
def test_tiles_equal_the_batch_of_the_symmetric_padded_raw_frame(h, w, s, g_buf, p_buf, with_llpm):
    from wcmc_amd import ops
    from wcmc_amd.support.inference import frame_tiles
    _, (ss, sp, ll), (ss_p, sp_p, ll_p, gt0) = _frame(h, w, s)
    assert len(torch.unique(ss[..., 9])) == h * w * s             # no two records equal: a wrong mirror cannot pass by coincidence
    org = _origins(frame_tiles(h, w, PATCH, PAD))
    ops.check_tile_origins(org, h, w, PATCH, PAD)
    assert int(org.min()) == -PAD                                # tiles do reach outside the frame
    got = ops.assemble_sample_tiles(ss, sp if p_buf else None, ll if with_llpm else None, org, PATCH, PAD, g_buf, p_buf)
    want = ops.assemble_sample_patches(ss_p, sp_p if p_buf else None, ll_p if with_llpm else None, gt0, org + PAD, PATCH, g_buf, p_buf)
    f = (24 if g_buf else 3) + (66 if p_buf else 0) + (1 if with_llpm else 0)
    assert got["features"].shape == (len(org), s, f, PATCH, PATCH)
    _assert_entries_equal(got, want, {"radiance", "features"} | ({"paths"} if with_llpm else set()))


def test_tiles_inside_the_frame_equal_the_existing_patch_assembly():
    from wcmc_amd import ops
    h, w, s = 128, 150, 2
    ss, sp, ll = _buffers(_raw_frame(h, w, s, seed=7))
    gt0 = torch.zeros((h, w, 9), device=DEV)
    org = torch.tensor([(0, 0), (0, 22), (0, 5), (0, 1), (0, 21), (0, 13)], dtype=torch.int32, device=DEV)
    for g_buf, p_buf, with_llpm in FLAGS:
        got = ops.assemble_sample_tiles(ss, sp if p_buf else None, ll if with_llpm else None, org, PATCH, PAD, g_buf, p_buf)
        want = ops.assemble_sample_patches(ss, sp if p_buf else None, ll if with_llpm else None, gt0, org, PATCH, g_buf, p_buf)
        _assert_entries_equal(got, want, set(want) - {"target_image"})
    with pytest.raises(ValueError, match="outside the 128x150 frame extended by 32"):
        ops.assemble_sample_tiles(ss, sp, ll, org + 100, PATCH, PAD)
    with pytest.raises(ValueError, match="use_sbmc_buf needs sbmc_p"):
        ops.assemble_sample_tiles(ss, None, ll, org, PATCH, PAD)


def _tonemap_u8(img, dtype):
    """round(255 * clip(tonemap(img), 0, 1)) with tonemap of the reference's test_models.py:24-34 (gamma 1 / 2.2) in ``dtype``."""
    c = img.astype(dtype)
    lum = dtype(0.2126) * c[:, :, 0] + dtype(0.7152) * c[:, :, 1] + dtype(0.0722) * c[:, :, 2]
    col = np.clip(c / (dtype(1) + lum / dtype(1.5))[:, :, None], 0, None)
    return np.round(dtype(255) * np.clip(col ** dtype(1.0 / 2.2), 0.0, 1.0)).astype(np.int64)


@pytest.mark.parametrize("s", SPPS)
def test_finish_sample_frame_against_torch_and_fp64(s):
    """``has_hit`` and the composite are exact.  ``ipt`` is a sequential fp32 sum of S non-negative values and one division: first
    order, (S - 1) roundings of partial sums that never exceed the total plus one of the quotient, each 2**-24 relative -- S * 2**-24 *
    mean; the bar is twice that.  The previews are held to the bar of tests/test_gpu_denoise.py (within one level of the fp64
    evaluation everywhere, equal on >= 99 % of the pixels)."""
    from wcmc_amd import ops
    h, w = 70, 83
    g = torch.Generator().manual_seed(h + w + s)
    sbmc_s = torch.rand((h, w, s, 27), generator=g) ** 2 * 2.5     # (channels 0:3 are max(total, 0): non-negative; dark to bright)
    llpm = torch.rand((h, w, s, 37), generator=g) * 0.5
    sel = torch.rand((h, w), generator=g)
    llpm[..., 25][sel < 0.2] = 0.0                                # hit by no sample ...
    only_last = sel < 0.1
    llpm[..., s - 1, 25][only_last] = 0.25                        # ... or by the last one alone
    sbmc_s, llpm = sbmc_s.to(DEV), llpm.to(DEV)
    out_rad = (torch.rand((3, h, w), generator=g) * 1.5).to(DEV)
    out, ipt, has_hit, pv_out, pv_ipt = ops.finish_sample_frame(out_rad, sbmc_s, llpm, preview=True)
    out2, ipt2, has_hit2 = ops.finish_sample_frame(out_rad, sbmc_s, llpm)
    assert torch.equal(out, out2) and torch.equal(ipt, ipt2) and torch.equal(has_hit, has_hit2)
    acc = torch.zeros((h, w), device=DEV)
    for k in range(s):                                           # the rule of finish_frame: summed in sample order, then / S
        acc = acc + llpm[:, :, k, 25]
    hit = (acc / float(s)) != 0.0
    assert torch.equal(has_hit, hit.float())
    assert bool(hit[only_last.to(DEV)].all()) and int((~hit).sum()) == int(((sel >= 0.1) & (sel < 0.2)).sum()) > 0
    assert torch.equal(out, torch.where(hit[..., None], out_rad.permute(1, 2, 0), ipt))
    want = sbmc_s[..., 0:3].double().mean(2).cpu().numpy()
    err = np.abs(ipt.cpu().numpy().astype(np.float64) - want)
    bound = s * 2.0 ** -23 * want
    print("ipt: max error / bound %.3g" % (err / bound).max())
    assert (err <= bound).all()
    for name, pv, src in (("out", pv_out, out), ("ipt", pv_ipt, ipt)):
        assert pv.dtype == torch.uint8 and pv.shape == (h, w, 3)
        src = src.cpu().numpy()
        want8, host8 = _tonemap_u8(src, np.float64), _tonemap_u8(src, np.float32)
        got8 = pv.cpu().numpy().astype(np.int64)
        same = float((got8 == want8).all(axis=2).mean())
        print("preview of %s: equal to fp64 on %.5f of the pixels, max difference %d level(s)" % (name, same, np.abs(got8 - want8).max()))
        assert float((host8 == want8).all(axis=2).mean()) >= 0.99   # the inputs let an fp32 evaluation meet the bar at all
        assert np.abs(got8 - want8).max() <= 1
        assert same >= 0.99
        assert want8.max() - want8.min() > 100                    # the image spans the range: no trivially equal previews


class _TileIndex:
    """A stand-in interface: tile t of the frame (in table order) comes back as the constant t, 124 pixels wide."""

    def __init__(self):
        self.seen = 0

    def to_eval_mode(self):
        pass

    def denoise_batch(self, batch):
        assert set(batch) == {"radiance", "features", "paths"}
        b = batch["radiance"].shape[0]
        idx = torch.arange(self.seen, self.seen + b, device=DEV, dtype=torch.float32)
        self.seen += b
        return idx.view(b, 1, 1, 1).expand(b, 3, 124, 124).contiguous(), None


def test_every_pixel_comes_from_the_tile_that_owns_it():
    from wcmc_amd.support.inference import denoise_sample_frame, frame_tiles
    h, w, s = 70, 83, 2
    _, (ss, sp, ll), _ = _frame(h, w, s)
    ll = ll.clone()
    ll[..., 25] = 1.0                                            # every pixel hit: the composite is the network's output
    model = _TileIndex()
    out, ipt, has_hit = denoise_sample_frame(model, ss, sp, ll, True, True, True, batch_size=3)
    table = frame_tiles(h, w, PATCH, PAD)
    assert model.seen == len(table) == 4 and bool((has_hit == 1).all())
    want = torch.full((h, w), -1.0)
    for t, (i0, j0, i1, j1, _, _) in enumerate(table):
        want[i0:i1, j0:j1] = t
    assert torch.equal(out.cpu(), want[..., None].expand(h, w, 3))


class _Shrinks:
    """A denoiser whose receptive field leaves 60 of a tile's 128 pixels."""

    def to_eval_mode(self):
        pass

    def denoise_batch(self, batch):
        return batch["radiance"][:, 0, :, 34:94, 34:94], None


def test_an_output_smaller_than_the_pad_allows_is_refused():
    from wcmc_amd.support.inference import denoise_sample_frame
    _, (ss, sp, ll), _ = _frame(70, 83, 2)
    with pytest.raises(ValueError, match=r"60 x 60 output.*--tile_pad"):
        denoise_sample_frame(_Shrinks(), ss, sp, ll, False, True, True, batch_size=3)


# ------------------------------------------------------------------------------------------------- real interfaces
COMMON = ["--input", "unused", "--output_dir", "unused", "--denoiser", "standins:SampleDenoiserStandIn", "--use_llpm_buf"]
MODELS = {"SBMC_t": ["--disentangle", "m11r11", "--pnet_out_size", "3"],
          "LBMC_t": ["--disentangle", "m11r01", "--pnet_out_size", "4"]}            # the half slice: 2 of the 4 channels


def _args(save, name, extra=()):
    from wcmc_amd import denoise, train_kpcn
    return train_kpcn.check_args(denoise.build_parser().parse_args(["--save", save, "--model_name", name] + COMMON + MODELS[name]
                                                                   + list(extra)))


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """Freshly seeded SBMC and LBMC checkpoints (a real PathNet backbone around the stand-in denoiser), written as the launchers write
    theirs."""
    from wcmc_amd import denoise
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.datasets import dncnn_in_size
    save = str(tmp_path_factory.mktemp("weights"))
    for name in MODELS:
        args = _args(save, name)
        torch.manual_seed(1)
        sizes = {"dncnn_in_size": dncnn_in_size("sbmc", True, False, True, 0), "pnet_in_size": 36, "pnet_out_size": 0}
        itfs, _ = denoise.sample_launcher(name).init_model(sizes, args, torch.device(DEV))
        ckpt.save_checkpoint(os.path.join(save, name + ".pth"), itfs[0], 0, args)
    return save


class _AsValidate:
    """``support.inference.inference`` calls ``validate_batch``; this hands it ``denoise_batch``."""

    def __init__(self, itf):
        self.to_eval_mode, self.validate_batch = itf.to_eval_mode, itf.denoise_batch


@pytest.mark.parametrize("name", list(MODELS))
def test_real_model_equals_the_padded_raw_route(checkpoints, name):
    from wcmc_amd import denoise, ops
    from wcmc_amd.support.inference import denoise_sample_frame, frame_tiles, inference
    from wcmc_amd.support.interfaces import LBMCInterface, SBMCInterface
    h, w, s, bs = 70, 83, 2, 3
    itf = denoise.load_interface(_args(checkpoints, name), torch.device(DEV))
    assert type(itf) is (SBMCInterface if name.startswith("SBMC") else LBMCInterface)
    _, (ss, sp, ll), (ss_p, sp_p, ll_p, gt0) = _frame(h, w, s)
    out, ipt, has_hit, out_path = denoise_sample_frame(itf, ss, None, ll, True, True, False, batch_size=bs, want_pbuffers=True)
    assert set(itf.m_losses) == {"m_val"} and float(itf.m_losses["m_val"]) == 0.0       # nothing was scored
    table = frame_tiles(h, w, PATCH, PAD)
    org = _origins(table)

    def loader():                                                # the same grouping and order
        for k in range(0, len(table), bs):
            batch = ops.assemble_sample_patches(ss_p, None, ll_p, gt0, org[k:k + bs] + PAD, PATCH, True, False)
            del batch["target_image"]
            yield (batch,) + tuple(list(c) for c in zip(*table[k:k + bs]))
    rad, path = inference(_AsValidate(itf), loader(), h, w, PATCH, use_llpm_buf=True)
    hit = ll[..., 25].mean(2) != 0
    assert torch.equal(has_hit != 0, hit) and 0 < float(has_hit.mean()) < 1
    assert torch.equal(out, torch.where(hit[..., None], rad.permute(1, 2, 0), ipt))
    c = 3 if name.startswith("SBMC") else 2
    assert out_path.shape == path.shape == (s, c, h, w) and torch.equal(out_path, path)
    assert bool(torch.isfinite(out).all()) and float(out_path.abs().max()) > 0
    assert bool(((out != ipt).any(dim=2) == hit).all())          # the network did something on every hit pixel, nothing elsewhere


# ------------------------------------------------------------------------------------------------- the streamer
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    """scene.npy (70 x 83, 2 samples) + scene_1.npy (1 more), with a few Inf / NaN among the values read; large.npy (128 x 150 x 2)."""
    d = tmp_path_factory.mktemp("renders")
    a, b = _raw_frame(70, 83, 2, seed=1), _raw_frame(70, 83, 1, seed=5)
    a[35, 27, 0, 3], a[69, 0, 1, 9], a[0, 82, 0, 30] = float("inf"), float("nan"), float("inf")
    np.save(d / "scene.npy", a)
    np.save(d / "scene_1.npy", b)
    np.save(d / "large.npy", _raw_frame(128, 150, 2, seed=9))
    return d


@functools.lru_cache(maxsize=None)
def _whole_frame_route(fn, spp):
    from wcmc_amd import denoise, ops
    raw = denoise.upload_raw(denoise.read_raw(fn, spp)[0], torch.device(DEV))
    return ops.preprocess_sbmc(raw) + (ops.preprocess_llpm(raw),)


@pytest.mark.parametrize("band_rows", (1, 16, 70))
def test_streamer_in_sbmc_mode_equals_whole_frame_preprocessing(renders, band_rows):
    """Three samples: the third comes from the continuation file."""
    from wcmc_amd.support.staging import FrameStreamer
    fn = str(renders / "scene.npy")
    want = _whole_frame_route(fn, 3)
    frames = FrameStreamer([fn], 3, DEV, band_rows=band_rows, base_model="sbmc", use_sbmc_buf=True)
    try:
        (got,) = [tuple(t.clone() for t in bufs) for bufs in frames]
    finally:
        frames.close()
    torch.cuda.synchronize()
    for name, g, w_, c in zip(("sbmc_s", "sbmc_p", "llpm"), got, want, (27, 66, 37)):
        assert g.shape == (70, 83, 3, c), name
        assert torch.equal(_bits(g), _bits(w_)), name
    assert float(got[0][35, 27, 0].max()) == float(np.float32(1e38))                   # the band was sanitised


def test_streamer_without_the_sbmc_buffer_holds_no_frame_sized_sbmc_p(renders):
    """128 x 150 x 2 in bands of 8 rows, 'lbmc': sbmc_s + llpm + two raw bands + one band of scratch for the kernel's second output +
    1 MiB (13.5 MB); a frame-sized sbmc_p would add 10.1 MB."""
    from wcmc_amd.support.staging import FrameStreamer
    h, w, s = 128, 150, 2
    fn = str(renders / "large.npy")
    want = _whole_frame_route(fn, s)
    band, scratch = 8 * w * s * 104 * 4, 8 * w * s * 66 * 4
    bound = h * w * s * (27 + 37) * 4 + 2 * band + scratch + (1 << 20)
    assert bound < h * w * s * (27 + 37 + 66) * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    frames = FrameStreamer([fn], s, DEV, band_rows=8, base_model="lbmc")
    sbmc_s, sbmc_p, llpm = next(frames)
    frames.close()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak device memory of the streamed frame: %d B over the start (bound %d B)" % (rise, bound))
    assert sbmc_p is None
    assert torch.equal(_bits(sbmc_s), _bits(want[0])) and torch.equal(_bits(llpm), _bits(want[2]))
    assert rise <= bound
    assert frames.ring.nbytes() == 0                              # the pinned ring is given back on close


# ------------------------------------------------------------------------------------------------- the command line
def test_command_line_runs_an_sbmc_checkpoint(checkpoints, tmp_path):
    from wcmc_amd import denoise, ops
    from wcmc_amd.support.inference import denoise_sample_frame
    h, w = 70, 83
    raw = _frame(h, w, 2)[0]
    scenes = tmp_path / "renders"
    scenes.mkdir()
    np.save(scenes / "scene.npy", raw)
    out_dir = tmp_path / "out"
    argv = ["--input", str(scenes / "scene.npy"), "--output_dir", str(out_dir), "--save", checkpoints, "--model_name", "SBMC_t",
            "--denoiser", "standins:SampleDenoiserStandIn", "--use_llpm_buf", "--save_pbuffer"] + MODELS["SBMC_t"]
    times = denoise.main(argv)
    assert len(times) == 1 and {"upload", "preprocess", "network", "finish", "write"} <= set(times[0])
    assert sorted(os.listdir(out_dir)) == ["scene_denoised.npy", "scene_denoised.pfm", "scene_pbuffer.npy"]
    assert sorted(os.listdir(scenes)) == ["scene.npy"]            # nothing written beside the input, no gt looked for
    # the Python route on the whole uploaded frame
    itf = denoise.load_interface(_args(checkpoints, "SBMC_t"), torch.device(DEV))
    dev_raw = denoise.upload_raw(denoise.read_raw(str(scenes / "scene.npy"))[0], torch.device(DEV))
    ss, _ = ops.preprocess_sbmc(dev_raw)
    want, _, _, want_path = denoise_sample_frame(itf, ss, None, ops.preprocess_llpm(dev_raw), True, True, False, 8, want_pbuffers=True)
    want = want.cpu().numpy()
    np.save(tmp_path / "want.npy", want)
    denoise.write_pfm(tmp_path / "want.pfm", want)
    for ext in ("npy", "pfm"):
        assert open(out_dir / ("scene_denoised." + ext), "rb").read() == open(tmp_path / ("want." + ext), "rb").read(), ext
    pb = np.load(out_dir / "scene_pbuffer.npy")
    assert pb.shape == (h, w, 2, 3) and np.array_equal(pb, want_path.permute(2, 3, 0, 1).cpu().numpy())
