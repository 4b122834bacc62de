"""The dihedral self-ensemble of wcmc_amd.denoise on the GPU (csrc/frame_tiles.hip:
wcmc_stitch_tiles_aug, wcmc_assemble_kpcn_tiles with a code t; csrc/sbmc_data.hip: wcmc_assemble_sample_tiles with a code t;
support.inference.denoise_frame / denoise_sample_frame with ``ensemble``; ``--self_ensemble``).

The tile batches under a code are held bit for bit against the route that exists without them -- the plain tile assemblers on the
buffers of the host-transformed frame --, the stitch and the average against a restatement that runs the EXISTING ``denoise_frame`` on
each transformed frame's own buffers, turns the results back with torch, sums them in code order and divides once; with a stand-in
network whose output is asymmetric in both tile axes, with a real KPCN-Manifold model, with a real SBMC interface, and through the
command line."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from data_ref import cmap, make_frame

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATCH, PAD = 128, 32
SIZES = [(64, 64), (70, 83), (128, 150)]          # one tile mirrored on all four sides; 2 x 2 tiles, both clamped, non-square; 2 x 3 tiles
SPPS = [2, 3]                                     # the power-of-two statistics kernel and the other one
CODES = tuple(range(8))
VALUE_CHANNELS = [0, 1, 2, 3, 10, 11, 12, 13, 20, 21, 22, 23, 30, 31, 34, 35, 36, 37]       # values and variances: no differences
BOUNCE = 60                                       # raw channel of the first bounce's type


def T(a, t):
    """T_t on the two leading axes of a numpy array or a tensor."""
    if isinstance(a, torch.Tensor):
        return torch.rot90(a.flip(1) if t & 4 else a, t & 3, (0, 1)).contiguous()
    return np.ascontiguousarray(np.rot90(np.fliplr(a) if t & 4 else a, k=t & 3))


def T_inv(a, t, dims=(0, 1)):
    """The inverse of T_t on the axes ``dims`` of a tensor."""
    a = torch.rot90(a, -(t & 3), dims)
    return (a.flip(dims[1]) if t & 4 else a).contiguous()


def _origins(table):
    return torch.tensor([c[4:6] for c in table], dtype=torch.int32, device=DEV)


def _tables(h, w, t):
    from wcmc_amd.support.inference import frame_tiles, frame_transform_shape
    ht, wt = frame_transform_shape(h, w, t)
    return ht, wt, frame_tiles(ht, wt, PATCH, PAD)


# ------------------------------------------------------------------------------------------------- the KPCN buffers
def _raw_frame(h, w, s, seed=0):
    """The frame recipe of tests/test_gpu_denoise.py: sanitised raw renderer output (h, w, s, 104) on the host, the first bounce's type
    zero in every sample on about 10 % of the pixels."""
    from wcmc_amd.support.datasets import sanitized
    a, b = make_frame(h, w, s, seed=seed, fill="kpcn"), make_frame(h, w, s, seed=seed + 1, fill="llpm")
    x = torch.where(torch.isnan(a), b, a)
    miss = torch.rand((h, w), generator=torch.Generator().manual_seed(seed + 2)) < 0.1
    x[..., cmap()["bounce"]][miss] = 0.0
    return sanitized(x.numpy())


@functools.lru_cache(maxsize=None)
def _raw(h, w, s):
    return _raw_frame(h, w, s, seed=h * 1000 + w + s)


@functools.lru_cache(maxsize=None)
def _frame(h, w, s, t=0):
    """(kpcn, llpm) preprocessed from the HOST-transformed raw frame T_t(raw); computed once and left unchanged."""
    from wcmc_amd import ops
    r = torch.from_numpy(T(_raw(h, w, s), t)).to(DEV)
    return ops.preprocess_kpcn(r), ops.preprocess_llpm(r)


def _assert_entries_equal(got, want, what, chan_dim=-3):
    assert set(got) == set(want), what
    for k in sorted(got):
        assert got[k].data_ptr() % 256 == 0 and got[k].shape == want[k].shape, (what, k)
        assert bool(torch.isfinite(want[k]).all()), (what, k)
        if not torch.equal(got[k], want[k]):
            bad = (got[k] != want[k]).nonzero()
            chans = sorted(set(bad[:, chan_dim].tolist()))
            raise AssertionError("%s: %s differs at %d entries, channels %s, first %s" % (what, k, len(bad), chans, bad[0].tolist()))


@pytest.mark.parametrize("s", SPPS)
@pytest.mark.parametrize("h,w", SIZES)
def test_premise_values_of_the_transformed_raw_frame_are_the_transformed_values(h, w, s):
    kpcn, llpm = _frame(h, w, s)
    for t in CODES:
        kpcn_t, llpm_t = _frame(h, w, s, t)
        assert torch.equal(kpcn_t[..., VALUE_CHANNELS], T(kpcn, t)[..., VALUE_CHANNELS]), t
        assert torch.equal(llpm_t, T(llpm, t)), t
        if t:                                                    # ... and the differences are not: the kernel has work to do
            assert not torch.equal(kpcn_t, T(kpcn, t)), t


@pytest.mark.parametrize("s", SPPS)
@pytest.mark.parametrize("h,w", SIZES)
def test_kpcn_tiles_under_a_code_equal_the_tiles_of_the_host_transformed_frame(h, w, s):
    from wcmc_amd import ops
    kpcn, llpm = _frame(h, w, s)
    for t in CODES:
        ht, wt, table = _tables(h, w, t)
        org = _origins(table)
        assert int(org.min()) == -PAD                            # tiles do reach outside the frame
        kpcn_t, llpm_t = _frame(h, w, s, t)
        assert kpcn_t.shape == (ht, wt, 44)
        for with_llpm in (True, False):
            got = ops.assemble_kpcn_tiles(kpcn, llpm if with_llpm else None, org, PATCH, PAD, transform=t)
            want = ops.assemble_kpcn_tiles(kpcn_t, llpm_t if with_llpm else None, org, PATCH, PAD)
            _assert_entries_equal(got, want, "code %d, llpm %s" % (t, with_llpm))
    # 0 and None take the plain call path
    org = _origins(_tables(h, w, 0)[2])
    want = ops.assemble_kpcn_tiles(kpcn, llpm, org, PATCH, PAD)
    for none in (0, None):
        _assert_entries_equal(ops.assemble_kpcn_tiles(kpcn, llpm, org, PATCH, PAD, transform=none), want, "transform=%r" % (none,))


def test_the_origins_are_checked_against_the_transformed_sizes():
    from wcmc_amd import ops
    h, w, s = 70, 83, 2
    kpcn, llpm = _frame(h, w, s)
    last = torch.tensor([[h + PAD - PATCH, w + PAD - PATCH]], dtype=torch.int32, device=DEV)       # the last origin of the 70 x 83 frame
    ops.assemble_kpcn_tiles(kpcn, None, last, PATCH, PAD, transform=2)
    with pytest.raises(ValueError, match="outside the 83x70 frame extended by 32"):
        ops.assemble_kpcn_tiles(kpcn, None, last, PATCH, PAD, transform=1)
    ops.assemble_kpcn_tiles(kpcn, None, last.flip(1).contiguous(), PATCH, PAD, transform=1)
    for bad in (8, -1, 1.5, "1"):
        with pytest.raises(ValueError, match="outside 0..7"):
            ops.assemble_kpcn_tiles(kpcn, None, last, PATCH, PAD, transform=bad)


# ------------------------------------------------------------------------------------------------- the per-sample buffers
def _sample_raw_frame(h, w, s, seed=0):
    """The frame recipe of tests/test_gpu_denoise_sample.py: no two records equal (channel 0 numbers them)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((h, w, s, 104), generator=g) * 2.0 - 0.5
    x[..., 66:] = x[..., 66:].abs()
    x[..., 0] = (torch.arange(h * w * s, dtype=torch.float32) / (h * w * s)).view(h, w, s)
    x[..., BOUNCE:BOUNCE + 6] = torch.randint(1, 32, (h, w, s, 6), generator=g).float()
    miss = torch.rand((h, w), generator=g) < 0.1
    x[..., BOUNCE][miss] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def _sample_frame(h, w, s):
    from wcmc_amd import ops
    r = _sample_raw_frame(h, w, s, seed=h * 1000 + w + s).to(DEV)
    return ops.preprocess_sbmc(r) + (ops.preprocess_llpm(r),)


FLAGS = list(itertools.product((True, False), repeat=3))    # every (use_g_buf, use_sbmc_buf, llpm): without use_sbmc_buf, sbmc_p is None


# (the three sizes x S = 2, 3, and S = 5 once: a full chunk of four samples and a chunk of one)
@pytest.mark.parametrize("h,w,s", [(h, w, s) for h, w in SIZES for s in SPPS] + [(70, 83, 5)])
def test_sample_tiles_under_a_code_equal_the_tiles_of_the_turned_buffers(h, w, s):
    from wcmc_amd import ops
    ss, sp, ll = _sample_frame(h, w, s)
    assert len(torch.unique(ss[..., 9])) == h * w * s            # no two records equal: a wrong map cannot pass by coincidence
    for t in CODES:
        ht, wt, table = _tables(h, w, t)
        org = _origins(table)
        ss_t, sp_t, ll_t = T(ss, t), T(sp, t), T(ll, t)          # every channel is per sample: the buffers of T_t(raw) are T_t of these
        assert ss_t.shape == (ht, wt, s, 27)
        for g_buf, p_buf, with_llpm in FLAGS:
            got = ops.assemble_sample_tiles(ss, sp if p_buf else None, ll if with_llpm else None, org, PATCH, PAD, g_buf, p_buf,
                                            transform=t)
            want = ops.assemble_sample_tiles(ss_t, sp_t if p_buf else None, ll_t if with_llpm else None, org, PATCH, PAD, g_buf, p_buf)
            _assert_entries_equal(got, want, "code %d, flags %s" % (t, (g_buf, p_buf, with_llpm)), chan_dim=2)
    org = _origins(_tables(h, w, 0)[2])
    want = ops.assemble_sample_tiles(ss, sp, ll, org, PATCH, PAD)
    for none in (0, None):
        _assert_entries_equal(ops.assemble_sample_tiles(ss, sp, ll, org, PATCH, PAD, transform=none), want, "transform=%r" % (none,),
                              chan_dim=2)
    with pytest.raises(ValueError, match="outside 0..7"):
        ops.assemble_sample_tiles(ss, sp, ll, org, PATCH, PAD, transform=8)


# ------------------------------------------------------------------------------------------------- stitch and average
class _RampModel:
    """A stand-in interface: the 92 x 92 output is the diffuse buffer times a fixed ramp that is asymmetric in both tile axes (a
    stitch that forgets to invert, or inverts the wrong way, shows up), and one P-buffer."""

    def __init__(self):
        y, x = torch.meshgrid(torch.arange(92.0), torch.arange(92.0), indexing="ij")
        self.ramp = (1.0 + 0.03125 * y + 0.001953125 * x * x).to(DEV).view(1, 1, 92, 92)

    def to_eval_mode(self):
        pass

    def denoise_batch(self, batch):
        assert not any(k.startswith("target") for k in batch)
        return batch["kpcn_diffuse_buffer"][:, :, 18:110, 18:110] * self.ramp, batch["paths"][:, :, 0:3] * 2.0


def _restated(run_plain, h, w, codes, has_hit, ipt, host_division=False):
    """The specification, from what exists without the feature: per code the un-ensembled frame of the transformed frame's own
    buffers (``run_plain(t)`` -> (H_t, W_t, 3)), turned back, summed in fp32 in code order, one division, the composite."""
    acc = None
    for t in codes:
        back = T_inv(run_plain(t), t)
        assert back.shape == (h, w, 3)
        acc = back if acc is None else acc + back
    if len(codes) > 1:
        if host_division:                                        # IEEE fp32 division on the host: no device op in the quotient
            acc = torch.from_numpy(acc.cpu().numpy() / np.float32(len(codes))).to(DEV)
        else:
            acc = acc / torch.tensor(float(len(codes)), device=DEV)
    return torch.where(has_hit[..., None] != 0, acc, ipt)


@pytest.mark.parametrize("s", SPPS)
@pytest.mark.parametrize("h,w", SIZES)
def test_ensemble_equals_the_plain_frames_of_the_transformed_buffers_turned_back_and_averaged(h, w, s):
    from wcmc_amd.support.inference import denoise_frame
    model = _RampModel()
    kpcn, llpm = _frame(h, w, s)
    plain = denoise_frame(model, kpcn, llpm, True, batch_size=3, want_pbuffers=True)
    out0, ipt, has_hit, path0 = plain
    assert 0 < float(has_hit.mean()) < 1

    @functools.lru_cache(maxsize=None)
    def run_plain(t):
        return denoise_frame(model, *_frame(h, w, s, t), True, batch_size=3)[0]
    # the stand-in does tell the orientations apart: a stitch that does not turn back cannot pass
    assert not torch.equal(T_inv(run_plain(2), 2), out0) and not torch.equal(T_inv(run_plain(4), 4), out0)
    for codes in ((0,), (0, 5), (0, 2, 4, 6), CODES):
        times = {}
        out, ipt_e, hit_e, path = denoise_frame(model, kpcn, llpm, True, batch_size=3, want_pbuffers=True, ensemble=codes, times=times)
        assert times.get("codes", (0,)) == codes and ("codes" in times) == (len(codes) > 1)      # (0,) reports what a plain run does
        assert times["tiles"] == sum(len(_tables(h, w, t)[2]) for t in codes)
        assert torch.equal(ipt_e, ipt) and torch.equal(hit_e, has_hit), codes
        assert torch.equal(path, path0), codes                   # the P-buffer is the identity pass's
        want = _restated(run_plain, h, w, codes, has_hit, ipt)
        if not torch.equal(out, want):
            bad = (out != want).nonzero()
            raise AssertionError("codes %s: %d entries differ, first %s: %r against %r"
                                 % (codes, len(bad), bad[0].tolist(), float(out[tuple(bad[0])]), float(want[tuple(bad[0])])))
        if len(codes) > 1:
            assert not torch.equal(out, out0), codes
    for a, b in zip(denoise_frame(model, kpcn, llpm, True, batch_size=3, want_pbuffers=True, ensemble=(0,)), plain):
        assert torch.equal(a, b)
    # the set is checked, and given in any order it is taken in ascending order
    assert torch.equal(denoise_frame(model, kpcn, llpm, True, batch_size=3, ensemble=[5, 0])[0],
                       denoise_frame(model, kpcn, llpm, True, batch_size=3, ensemble=(0, 5))[0])
    with pytest.raises(ValueError, match="does not contain 0"):
        denoise_frame(model, kpcn, llpm, True, batch_size=3, ensemble=(1, 2))


def test_the_average_is_one_fp32_division_not_a_multiplication_by_the_reciprocal():
    """Three codes: 1 / 3 is no fp32 number, so ``x * (1 / 3)`` and ``x / 3`` differ in the last bit on part of the frame.  The
    quotient of the restatement is numpy's on the host."""
    from wcmc_amd.support.inference import denoise_frame
    h, w, s, codes = 70, 83, 2, (0, 2, 4)
    model = _RampModel()
    kpcn, llpm = _frame(h, w, s)
    out, ipt, has_hit = denoise_frame(model, kpcn, llpm, True, batch_size=3, ensemble=codes)
    run_plain = lambda t: denoise_frame(model, *_frame(h, w, s, t), True, batch_size=3)[0]       # noqa: E731
    want = _restated(run_plain, h, w, codes, has_hit, ipt, host_division=True)
    assert out.dtype == want.dtype == torch.float32 and torch.equal(out, want)
    total = sum(T_inv(run_plain(t), t) for t in codes).cpu().numpy()
    hit = (has_hit != 0).cpu().numpy()
    by_reciprocal = total * (np.float32(1.0) / np.float32(3.0))
    assert (by_reciprocal[hit] != out.cpu().numpy()[hit]).any()              # the two roundings do differ on this frame


def test_stitch_tiles_aug_pastes_and_adds():
    """One launch over the whole table of the transformed frame: without ``accumulate`` every element of out_rad is overwritten
    (NaN before), with it the value is added to what was there; an output of the full tile size is not padded."""
    from wcmc_amd import ops
    h, w = 70, 83
    g = torch.Generator().manual_seed(3)
    for t in (1, 6):
        ht, wt, table = _tables(h, w, t)
        coords = torch.tensor(table, dtype=torch.int32, device=DEV)
        ops.check_tile_coords(table, ht, wt, PATCH)
        for size in (PATCH, 92):
            out = torch.rand((len(table), 3, size, size), generator=g).to(DEV)
            crop = (PATCH - size) // 2
            padded = torch.nn.functional.pad(out, (crop,) * 4, "replicate") if crop else out
            frame_t = torch.zeros((3, ht, wt), device=DEV)
            for b, (i0, j0, i1, j1, i, j) in enumerate(table):
                frame_t[:, i0:i1, j0:j1] = padded[b, :, i0 - i:i1 - i, j0 - j:j1 - j]
            want = T_inv(frame_t, t, (1, 2))
            got = torch.full((3, h, w), float("nan"), device=DEV)
            assert ops.stitch_tiles_aug(out, coords, got, t, False, PATCH) is got
            assert torch.equal(got, want), (t, size)
            base = torch.rand((3, h, w), generator=g).to(DEV)
            got = base.clone()
            ops.stitch_tiles_aug(out, coords, got, t, True, PATCH)
            assert torch.equal(got, base + want), (t, size)


# ------------------------------------------------------------------------------------------------- a real KPCN model
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


def test_real_model_ensemble_equals_the_restatement(checkpoint):
    from wcmc_amd import denoise
    from wcmc_amd.support.inference import denoise_frame
    h, w, s, bs = 70, 83, 2, 3
    itf = denoise.load_interface(_args(checkpoint), torch.device(DEV))
    kpcn, llpm = _frame(h, w, s)
    plain = denoise_frame(itf, kpcn, llpm, True, batch_size=bs, want_pbuffers=True)
    again = denoise_frame(itf, kpcn, llpm, True, batch_size=bs, want_pbuffers=True)
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], again[:3]))                  # the premise: a run repeats bit for bit
    assert all(torch.equal(plain[3][k], again[3][k]) for k in plain[3])
    codes = (0, 3, 6)
    out, ipt, has_hit, path = denoise_frame(itf, kpcn, llpm, True, batch_size=bs, want_pbuffers=True, ensemble=codes)
    assert torch.equal(ipt, plain[1]) and torch.equal(has_hit, plain[2])
    assert set(path) == set(plain[3]) and all(torch.equal(path[k], plain[3][k]) for k in path)
    want = _restated(lambda t: denoise_frame(itf, *_frame(h, w, s, t), True, batch_size=bs)[0], h, w, codes, has_hit, ipt)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, want)
    assert not torch.equal(out, plain[0])


# ------------------------------------------------------------------------------------------------- the sample-based route
SBMC = ["--input", "unused", "--output_dir", "unused", "--denoiser", "standins:SampleDenoiserStandIn", "--use_llpm_buf", "--disentangle",
        "m11r11", "--pnet_out_size", "3"]


def _sbmc_args(save):
    from wcmc_amd import denoise, train_kpcn
    return train_kpcn.check_args(denoise.build_parser().parse_args(["--save", save, "--model_name", "SBMC_t"] + SBMC))


def test_sample_route_ensemble_equals_the_restatement(tmp_path):
    """A real SBMC interface around ``standins.SampleDenoiserStandIn`` (124-pixel outputs: the replicate padding runs), its
    checkpoint made as tests/test_gpu_denoise_sample.py makes its own."""
    from wcmc_amd import denoise
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.datasets import dncnn_in_size
    from wcmc_amd.support.inference import denoise_sample_frame
    save = str(tmp_path)
    args = _sbmc_args(save)
    torch.manual_seed(1)
    sizes = {"dncnn_in_size": dncnn_in_size("sbmc", True, False, True, 0), "pnet_in_size": 36, "pnet_out_size": 0}
    itfs, _ = denoise.sample_launcher("SBMC_t").init_model(sizes, args, torch.device(DEV))
    ckpt.save_checkpoint(os.path.join(save, "SBMC_t.pth"), itfs[0], 0, args)
    itf = denoise.load_interface(_sbmc_args(save), torch.device(DEV))
    h, w, s, bs = 70, 83, 2, 3
    ss, sp, ll = _sample_frame(h, w, s)
    run = lambda a, b, **kw: denoise_sample_frame(itf, a, None, b, True, True, False, batch_size=bs, **kw)       # noqa: E731
    plain = run(ss, ll, want_pbuffers=True)
    codes = (0, 1, 4)
    out, ipt, has_hit, path = run(ss, ll, want_pbuffers=True, ensemble=codes)
    assert 0 < float(has_hit.mean()) < 1
    assert torch.equal(ipt, plain[1]) and torch.equal(has_hit, plain[2]) and torch.equal(path, plain[3])
    want = _restated(lambda t: run(T(ss, t), T(ll, t))[0], h, w, codes, has_hit, ipt)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, want)
    assert not torch.equal(out, plain[0])
    for a, b in zip(run(ss, ll, want_pbuffers=True, ensemble=(0,)), plain):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- the command line
def test_command_line_self_ensemble(checkpoint, tmp_path):
    from wcmc_amd import denoise
    h, w = 70, 83
    scenes = tmp_path / "renders"
    scenes.mkdir()
    np.save(scenes / "scene.npy", _raw(h, w, 2))
    argv = lambda out, extra: ["--input", str(scenes / "scene.npy"), "--output_dir", str(tmp_path / out), "--save", checkpoint,   # noqa: E731
                               "--model_name", "KPCN_denoise_test", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE",
                               "--train_branches", "--save_pbuffer"] + extra
    denoise.main(argv("plain", []))
    denoise.main(argv("again", []))
    times = denoise.main(argv("ens", ["--self_ensemble", "0", "2"]))
    assert times[0]["codes"] == (0, 2)
    names = ["scene_denoised.npy", "scene_denoised.pfm", "scene_pbuffer.npy"]
    read = lambda d, n: open(tmp_path / d / n, "rb").read()      # noqa: E731
    for d in ("plain", "again", "ens"):
        assert sorted(os.listdir(tmp_path / d)) == names, d
    assert sorted(os.listdir(scenes)) == ["scene.npy"]
    for n in names:
        assert read("plain", n) == read("again", n), n           # without the flag: the same bytes, run after run
    plain, ens = np.load(tmp_path / "plain" / names[0]), np.load(tmp_path / "ens" / names[0])
    assert ens.shape == plain.shape == (h, w, 3) and np.isfinite(ens).all() and not np.array_equal(ens, plain)
    assert read("ens", "scene_pbuffer.npy") == read("plain", "scene_pbuffer.npy")
    # ... and what the Python route gives for the same set
    from wcmc_amd.support.inference import denoise_frame
    itf = denoise.load_interface(_args(checkpoint), torch.device(DEV))
    want = denoise_frame(itf, *_frame(h, w, 2), True, batch_size=8, ensemble=(0, 2))[0]
    assert np.array_equal(ens, want.cpu().numpy())
    for bad in (["2", "4"], ["0", "2", "2"], ["0", "8"]):
        with pytest.raises(ValueError, match="--self_ensemble"):
            denoise.main(argv("refused", ["--self_ensemble"] + bad))
    assert not os.path.exists(tmp_path / "refused")
