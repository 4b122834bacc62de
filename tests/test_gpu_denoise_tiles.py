"""Tiles of any size, a wider overlap and feathered seams for wcmc_amd.denoise on the GPU (DESIGN.md section 22;
csrc/frame_tiles.hip: wcmc_stitch_tiles_blend, wcmc_blend_finish; support.inference ``blend=``; ``--tile`` / ``--tile_pad`` / ``--blend``).

The blend op is held to tests/blend_ref.py in fp64 with the bar that section 22 derives, and bit for bit to itself across tile
batches; the driver to the same reference with a stand-in whose tiles disagree at every seam; a real model at a new tile size to
``validate_batch`` on the padded-raw route (section 15's contract restated at P) and, with a finite receptive field, to the fp64
oracle on the whole frame; the ensemble and the command line to the Python route.  Figures go to ``WCMC_TEST_REPORTS``
(profiles/denoise_tiles_error.txt is a copy)."""
import functools
import os

import numpy as np
import pytest
import torch

import blend_ref
from test_gpu_denoise import _raw_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("WCMC_TEST_REPORTS", os.path.join(ROOT, "test_reports"))     # (git-ignored)
DEV = "cuda:0"
U = 2.0 ** -24
ROWS = []


def _report(line):
    print(line)
    ROWS.append(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "denoise_tiles_error.txt"), "w") as f:
        f.write("\n".join(ROWS) + "\n")


def _table(h, w, t, patch, pad):
    from wcmc_amd.support.inference import frame_tiles, frame_transform_shape
    ht, wt = frame_transform_shape(h, w, t)
    return ht, wt, frame_tiles(ht, wt, patch, pad)


def _stitch(out, table, h, w, t, f, patch, pad, batch):
    """acc, wsum and the finished frame of one pass, the table cut into batches of ``batch`` tiles."""
    from wcmc_amd import ops
    coords = torch.tensor(table, dtype=torch.int32, device=DEV)
    acc, wsum = torch.zeros((3, h, w), device=DEV), torch.zeros((h, w), device=DEV)
    for k in range(0, len(table), batch):
        ops.stitch_tiles_blend(out[k:k + batch], coords[k:k + batch], acc, wsum, f, t, patch, pad)
    res = ops.blend_finish(acc, wsum, torch.full((3, h, w), float("nan"), device=DEV))
    return acc, wsum, res


def _tiles(n, size, seed):
    """Random network outputs with a few large values (no Inf / NaN)."""
    g = torch.Generator().manual_seed(seed)
    out = torch.randn((n, 3, size, size), generator=g)
    big = torch.rand((n, 3, size, size), generator=g) < 0.01
    out[big] *= 1e4
    return out


# ------------------------------------------------------------------------------------------------- the op against fp64
@pytest.mark.parametrize("h,w", [(6, 6), (7, 13), (19, 23)])
@pytest.mark.parametrize("pad,f", [(5, 0), (5, 3), (6, 4)])
def test_blend_op_against_the_fp64_reference(h, w, pad, f):
    """|err| <= 16 * 2^-24 * sum w |v| / sum w per pixel: at most 3 roundings of a weight and 1 of the product per term, at most 8
    additions per sum, one division.  (6, 4): two ramps of 8 pixels in an interior of 4 -- the library refuses that where it is
    told the pad, so the pad is withheld there; at most three tiles still meet on an axis, F <= interior.)"""
    patch, worst = 16, 0.0
    for size in (12, 16):
        for t in range(8):
            ht, wt, table = _table(h, w, t, patch, pad)
            out = _tiles(len(table), size, seed=1000 * h + 10 * w + t + size)
            num, den, mag = blend_ref.blend_source(table, out.numpy(), h, w, t, f, patch)
            assert den.min() >= (0.25 if f else 1.0)
            want, bound = num / den, blend_ref.BAR * mag / den
            count = blend_ref.blend_source(table, np.ones((len(table), 3, size, size)), h, w, t, 0, patch)[1]
            assert (count == 1).all()                                 # the owned windows partition the frame
            for batch in (1, 3):
                acc, wsum, res = _stitch(out.to(DEV), table, h, w, t, f, patch, None if 2 * f > patch - 2 * pad else pad, batch)
                err = np.abs(res.double().cpu().numpy() - want)
                assert np.isfinite(res.cpu().numpy()).all()
                ratio = float((err / np.maximum(bound, 1e-300)).max())
                worst = max(worst, ratio)
                assert (err <= bound).all(), (size, t, batch, ratio)
                np.testing.assert_allclose(wsum.double().cpu().numpy(), den, rtol=9 * U, atol=0)
    if f == 0:
        assert worst == 0.0                                           # one term of weight 1: the paste, exactly
    _report("blend op, frame %2d x %2d, P 16, pad %d, F %d: largest error / bound %.3f" % (h, w, pad, f, worst))


def test_blend_op_at_zero_feather_is_the_owned_window_paste():
    from wcmc_amd import ops
    h, w, patch, pad = 70, 83, 128, 32
    for t in (0, 3, 6):
        ht, wt, table = _table(h, w, t, patch, pad)
        out = _tiles(len(table), 92, seed=t).to(DEV)
        coords = torch.tensor(table, dtype=torch.int32, device=DEV)
        want = ops.stitch_tiles_aug(out, coords, torch.full((3, h, w), float("nan"), device=DEV), t, False, patch)
        acc, wsum, res = _stitch(out, table, h, w, t, 0, patch, pad, 3)
        assert torch.equal(acc, want) and torch.equal(res, want) and bool((wsum == 1).all())


# ------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("h,w,patch,pad,f,size", [(19, 23, 16, 6, 4, 12), (150, 200, 128, 40, 12, 92), (70, 83, 128, 40, 12, 128)])
def test_sums_do_not_depend_on_the_tile_batches(h, w, patch, pad, f, size):
    from wcmc_amd import ops
    for t in (0, 5):
        ht, wt, table = _table(h, w, t, patch, pad)
        out = _tiles(len(table), size, seed=h + t).to(DEV)
        p = None if 2 * f > patch - 2 * pad else pad
        first = _stitch(out, table, h, w, t, f, patch, p, len(table))
        again = _stitch(out, table, h, w, t, f, patch, p, len(table))
        assert all(torch.equal(a, b) for a, b in zip(first, again))          # two runs of the same call
        for batch in (1, 3):
            got = _stitch(out, table, h, w, t, f, patch, p, batch)
            for name, a, b in zip(("acc", "wsum", "result"), got, first):
                assert torch.equal(a, b), (t, batch, name)
        assert bool(torch.isfinite(first[2]).all()) and float(first[1].min()) >= 0.25
        # accumulate adds the normalised pass to what is there
        base = torch.rand((3, h, w), generator=torch.Generator().manual_seed(1)).to(DEV)
        assert torch.equal(ops.blend_finish(first[0], first[1], base.clone(), accumulate=True), base + first[2])


# ------------------------------------------------------------------------------------------------- the driver with a stand-in
class _OriginModel:
    """A stand-in interface behind ``_denoise_tiles``: ``assemble`` hands it the tile origins (and the code), and every tile comes
    back as a fixed function of its origin and the pixel -- neighbouring tiles disagree on the pixels they share."""

    def __init__(self, patch, size):
        self.patch, self.size = patch, size

    def to_eval_mode(self):
        pass

    @staticmethod
    def value(oy, ox, t, c, y, x):
        return (1.0 + c) * (0.5 + 0.03125 * oy - 0.0078125 * ox + 0.25 * t) + 0.015625 * y + 0.001953125 * x * x

    def tiles(self, origins, t):
        """(B, 3, size, size) fp32 on the host: the values are sums of a few dyadic terms, exact in fp32."""
        crop = (self.patch - self.size) // 2
        y, x = np.meshgrid(np.arange(crop, crop + self.size, dtype=np.float64), np.arange(crop, crop + self.size, dtype=np.float64),
                           indexing="ij")
        out = np.stack([np.stack([self.value(float(oy), float(ox), t, c, y, x) for c in range(3)]) for oy, ox in origins])
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
        return out.astype(np.float32)

    def denoise_batch(self, batch):
        origins, t = batch
        return torch.from_numpy(self.tiles(origins.cpu().numpy(), t)).to(DEV), None


def _drive(model, h, w, patch, pad, blend, codes, batch_size=3, **kw):
    from wcmc_amd.support.inference import _denoise_tiles
    frame = torch.zeros((h, w, 1), device=DEV)
    res = _denoise_tiles("denoise_frame", model, frame, lambda origins, t=0: (origins, t),
                         lambda out_rad: (out_rad.permute(1, 2, 0).contiguous(), None, None), batch_size, False, patch, pad, False,
                         kw.pop("times", None), ensemble=codes, blend=blend, **kw)
    return res[0]


@pytest.mark.parametrize("codes", [(0,), (0, 3, 5)])
@pytest.mark.parametrize("h,w", [(70, 83), (128, 150)])
def test_driver_blends_a_stand_in_like_the_reference(h, w, codes):
    """The bar of the op per pass; the average over n codes adds n - 1 fp32 additions and one division on the passes' results:
    n * 2^-24 * sum |pass| / n."""
    patch, pad, f = 128, 40, 12
    for size in (128, 92):                                            # 92: the KPCN stack's output; the inset is then 18 <= pad - F
        model = _OriginModel(patch, size)
        times = {}
        got = _drive(model, h, w, patch, pad, f, codes, times=times).double().cpu().numpy()
        assert (times["tile"], times["tile_pad"], times["blend"]) == (patch, pad, f)
        assert times["tiles"] == sum(len(_table(h, w, t, patch, pad)[2]) for t in codes)
        want, bound, mags = 0.0, 0.0, 0.0
        for t in codes:
            ht, wt, table = _table(h, w, t, patch, pad)
            num, den, mag = blend_ref.blend_source(table, model.tiles([r[4:6] for r in table], t), h, w, t, f, patch)
            want, bound, mags = want + num / den, bound + blend_ref.BAR * mag / den, mags + np.abs(num / den)
        n = len(codes)
        want, bound = want / n, bound / n + (n * U * mags / n if n > 1 else 0.0)
        err = np.abs(got.transpose(2, 0, 1) - want)
        ratio = float((err / bound).max())
        assert (err <= bound).all(), ratio
        _report("driver, stand-in, frame %d x %d, P 128, pad 40, F 12, output %d, codes %s: largest error / bound %.3f"
                % (h, w, size, codes, ratio))
        # the seams are blended: the owned-window stitch of the same tiles differs, by steps the feather removes
        plain = _drive(model, h, w, patch, pad, 0, codes).double().cpu().numpy()
        assert np.abs(plain - got).max() > 0.1
        for bs in (1, 100):                                           # ... and bit for bit whatever --tile_batch
            assert np.array_equal(_drive(model, h, w, patch, pad, f, codes, batch_size=bs).double().cpu().numpy(), got)


@pytest.mark.parametrize("codes", [(0,), (0, 3, 5)])
def test_driver_at_zero_feather_is_the_owned_window_path(codes):
    from wcmc_amd.support.inference import _denoise_tiles
    h, w, patch, pad = 70, 83, 128, 40
    model = _OriginModel(patch, 92)
    got = _drive(model, h, w, patch, pad, 0, codes)
    frame = torch.zeros((h, w, 1), device=DEV)
    today = _denoise_tiles("denoise_frame", model, frame, lambda origins, t=0: (origins, t),
                           lambda out_rad: (out_rad.permute(1, 2, 0).contiguous(), None, None), 3, False, patch, pad, False, None,
                           ensemble=codes)[0]                        # the call as it was made before there was a `blend`
    assert torch.equal(got, today)
    # ... which is the paste of the owned windows, summed over the codes in order and divided once
    total = None
    for t in codes:
        ht, wt, table = _table(h, w, t, patch, pad)
        tiles = blend_ref.replicate_pad(model.tiles([r[4:6] for r in table], t), patch)
        frame_t = np.zeros((3, ht, wt), np.float32)
        for b, (i0, j0, i1, j1, i, j) in enumerate(table):
            frame_t[:, i0:i1, j0:j1] = tiles[b][:, i0 - i:i1 - i, j0 - j:j1 - j]
        back = np.ascontiguousarray(blend_ref.turn_back(frame_t, t, (1, 2)))
        total = back if total is None else total + back
    if len(codes) > 1:
        total = total / np.float32(len(codes))
    assert np.array_equal(got.cpu().numpy().transpose(2, 0, 1), total)


def test_driver_refuses_a_feather_that_the_pad_or_the_output_cannot_carry():
    with pytest.raises(ValueError, match="--blend 25"):               # two ramps of 50 in an interior of 48
        _drive(_OriginModel(128, 128), 70, 83, 128, 40, 25, (0,))
    with pytest.raises(ValueError, match="--blend 13.*12 pixels wide at the most"):
        _drive(_OriginModel(128, 128), 70, 83, 128, 40, 13, (0,), inset=28)
    with pytest.raises(ValueError, match="--blend 12"):               # the first output shows an inset of 34
        _drive(_OriginModel(128, 60), 70, 83, 128, 40, 12, (0,))
    _drive(_OriginModel(128, 60), 70, 83, 128, 40, 6, (0,))
    with pytest.raises(ValueError, match="192-pixel tile .* does not fit the 70 x 83 frame"):
        _drive(_OriginModel(192, 192), 70, 83, 192, 40, 8, (0,))


# ------------------------------------------------------------------------------------------------- real models at a new size
H, W, S = 150, 200, 2
FLAGS = {"KPCN_tiles_llpm": ["--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--train_branches"],
         "KPCN_tiles_plain": ["--train_branches"]}


def _args(save, name, extra=()):
    from wcmc_amd import denoise
    return denoise.build_parser().parse_args(["--save", save, "--model_name", name, "--input", "unused", "--output_dir", "unused"]
                                             + FLAGS[name] + list(extra))


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """Fresh KPCN-Manifold and plain KPCN checkpoints, made as tests/test_gpu_denoise.py makes its own."""
    from wcmc_amd import train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    save = str(tmp_path_factory.mktemp("weights"))
    for name in FLAGS:
        args = _args(save, name)
        torch.manual_seed(0)
        llpm = name.endswith("llpm")
        sizes = {"dncnn_in_size": 34 + (3 + 2 if llpm else 0), "pnet_in_size": 36 if llpm else 0, "pnet_out_size": 3 if llpm else 0}
        itfs, _ = train_kpcn.init_model(sizes, args, torch.device(DEV))
        torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, name + ".pth"))
    return save


@functools.lru_cache(maxsize=None)
def _raw(t=0):
    raw = _raw_frame(H, W, S, seed=H * 1000 + W + S)
    return np.ascontiguousarray(blend_ref.turn(raw, t))


@functools.lru_cache(maxsize=None)
def _buffers(t=0, pad=0):
    """(kpcn, llpm) of the raw frame turned by code t on the host and symmetric-padded by ``pad``; computed once, left unchanged."""
    from wcmc_amd import ops
    raw = _raw(t)
    if pad:
        raw = np.ascontiguousarray(np.pad(raw, ((pad, pad), (pad, pad), (0, 0), (0, 0)), "symmetric"))
    r = torch.from_numpy(raw).to(DEV)
    return ops.preprocess_kpcn(r), ops.preprocess_llpm(r)


@pytest.mark.parametrize("name", sorted(FLAGS))
def test_real_model_at_192_equals_validate_batch_on_the_padded_raw_route(checkpoints, name):
    """DESIGN.md section 15's contract restated at P = 192."""
    from wcmc_amd import denoise, ops
    from wcmc_amd.support.inference import denoise_frame, frame_tiles, inference
    patch, pad, bs, llpm_on = 192, 32, 3, name.endswith("llpm")
    itf = denoise.load_interface(_args(checkpoints, name), torch.device(DEV))
    (kpcn, llpm), (kpcn_p, llpm_p) = _buffers(), _buffers(0, pad)
    gt0 = torch.zeros((H + 2 * pad, W + 2 * pad, 9), device=DEV)
    out, ipt, has_hit, out_path = denoise_frame(itf, kpcn, llpm, llpm_on, batch_size=bs, want_pbuffers=True, patch_size=patch,
                                                pad_size=pad)
    table = frame_tiles(H, W, patch, pad)
    assert len(table) == 4
    org = torch.tensor([r[4:6] for r in table], dtype=torch.int32, device=DEV)

    def loader():
        for k in range(0, len(table), bs):
            batch = ops.assemble_kpcn_patches(kpcn_p, llpm_p if llpm_on else None, gt0, org[k:k + bs] + pad, patch)
            yield (batch,) + tuple(list(c) for c in zip(*table[k:k + bs]))
    rad, path = inference(itf, loader(), H, W, patch, use_llpm_buf=llpm_on)
    hit = llpm[..., 25].mean(2) != 0
    assert torch.equal(out, torch.where(hit[..., None], rad.permute(1, 2, 0), ipt))
    assert bool(torch.isfinite(out).all()) and bool(((out != ipt).any(dim=2) == hit).all())
    if llpm_on:
        assert set(out_path) == set(path) and all(torch.equal(out_path[k], path[k]) for k in path)
    else:
        assert out_path is None


def test_a_finite_receptive_field_gives_the_whole_frame_result_at_every_tiling():
    """KPCN(34, width=16) without llpm: 36 pixels of 5 x 5 shrink and 10 of kernel apply, so a pixel 32 inside a tile sees tile data
    only and the tiled result is the network on the whole symmetric-padded frame.  Reference: oracle.models.KPCN in fp64 on the CPU
    with the same weights.  The errors at P = 192 and at P = 192 / pad 40 / F 12 may be at most twice the error of today's P = 128 run
    (other heights may take other kernel instances of the same arithmetic)."""
    import types
    from oracle.models import KPCN as OKPCN
    from wcmc_amd import KPCN, ops
    from wcmc_amd.support.inference import denoise_frame
    from wcmc_amd.support.interfaces import KPCNInterface
    from wcmc_amd.support.losses import RelativeMSE
    torch.manual_seed(5)
    oracle = OKPCN(34, width=16)
    model = KPCN(34, width=16)
    model.load_state_dict(oracle.state_dict())
    lf = {k: torch.nn.L1Loss() for k in ("l_diffuse", "l_specular", "l_recon")}
    lf["l_test"] = RelativeMSE()
    itf = KPCNInterface({"dncnn": model.to(DEV)}, {}, lf, types.SimpleNamespace(model_name="finite"), use_llpm_buf=False)
    (kpcn, llpm), (kpcn_p, _) = _buffers(), _buffers(0, 32)
    # the whole padded frame as one batch, by the channel map of the tile assembler -- held to it on one tile first
    k = kpcn_p.permute(2, 0, 1)[None]
    whole = {"kpcn_diffuse_in": torch.cat([k[:, 0:10], k[:, 20:44]], 1), "kpcn_specular_in": k[:, 10:44],
             "kpcn_diffuse_buffer": k[:, 0:3], "kpcn_specular_buffer": k[:, 10:13], "kpcn_albedo": k[:, 34:37] + 0.00316}
    org = torch.tensor([[7, 40]], dtype=torch.int32, device=DEV)
    tile = ops.assemble_kpcn_patches(kpcn_p, None, torch.zeros(kpcn_p.shape[:2] + (9,), device=DEV), org, 128)
    for key, v in whole.items():
        assert torch.equal(v[:, :, 7:135, 40:168], tile[key]), key
    with torch.no_grad():
        ref = oracle.double()({key: v.double().cpu() for key, v in whole.items()})["radiance"][0]
    crop = (kpcn_p.shape[0] - ref.shape[1]) // 2
    assert ref.shape[1:] == (H + 64 - 2 * crop, W + 64 - 2 * crop) and crop <= 32
    ref = ref[:, 32 - crop:32 - crop + H, 32 - crop:32 - crop + W].permute(1, 2, 0).numpy()
    errs = {}
    for what, kw in (("P 128, pad 32, F 0", dict()), ("P 192, pad 32, F 0", dict(patch_size=192)),
                     ("P 192, pad 40, F 12", dict(patch_size=192, pad_size=40, blend=12))):
        out, ipt, has_hit = denoise_frame(itf, kpcn, llpm, False, batch_size=3, **kw)
        hit = (has_hit != 0).cpu().numpy()
        assert 0 < hit.mean() < 1
        errs[what] = float(np.abs(out.double().cpu().numpy() - ref)[hit].max())
        _report("finite receptive field, KPCN(34, width=16), frame %d x %d, %s: max abs error against the fp64 oracle on the whole "
                "frame %.3e (largest |reference| %.3e)" % (H, W, what, errs[what], np.abs(ref[hit]).max()))
    base = errs["P 128, pad 32, F 0"]
    assert base > 0 and np.abs(ref).max() > 1e3 * base               # the reference is met, not merely approached
    for what, e in errs.items():
        assert e <= 2 * base, (what, e, base)


def test_ensemble_contract_at_a_new_size(checkpoints):
    """The fp32 sum, in code order, of the plain blended runs on the host-transformed raw frames turned back, divided by 3."""
    from wcmc_amd import denoise
    from wcmc_amd.support.inference import denoise_frame
    codes, kw = (0, 3, 5), dict(batch_size=3, patch_size=192, pad_size=40, blend=8)
    itf = denoise.load_interface(_args(checkpoints, "KPCN_tiles_llpm"), torch.device(DEV))
    kpcn, llpm = _buffers()
    out, ipt, has_hit = denoise_frame(itf, kpcn, llpm, True, ensemble=codes, **kw)
    acc = None
    for t in codes:
        plain = denoise_frame(itf, *_buffers(t), True, **kw)[0]
        back = torch.rot90(plain, -(t & 3), (0, 1))
        back = (back.flip(1) if t & 4 else back).contiguous()
        assert back.shape == (H, W, 3)
        acc = back if acc is None else acc + back
    want = torch.where(has_hit[..., None] != 0, acc / torch.tensor(3.0, device=DEV), ipt)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, want)
    assert not torch.equal(out, denoise_frame(itf, kpcn, llpm, True, **kw)[0])
    assert not torch.equal(denoise_frame(itf, kpcn, llpm, True, **kw)[0],
                           denoise_frame(itf, kpcn, llpm, True, **dict(kw, blend=0))[0])          # the feather does something


# ------------------------------------------------------------------------------------------------- the command line
def test_command_line_kpcn(checkpoints, tmp_path):
    from wcmc_amd import denoise
    from wcmc_amd.support.inference import denoise_frame
    scenes = tmp_path / "renders"
    scenes.mkdir()
    np.save(scenes / "scene.npy", _raw())
    name = "KPCN_tiles_llpm"
    argv = ["--input", str(scenes / "scene.npy"), "--output_dir", str(tmp_path / "out"), "--save", checkpoints, "--model_name", name,
            "--tile", "192", "--tile_pad", "40", "--blend", "8", "--save_pbuffer"] + FLAGS[name]
    times = denoise.main(argv)
    assert (times[0]["tile"], times[0]["tile_pad"], times[0]["blend"], times[0]["tiles"]) == (192, 40, 8, 4)
    itf = denoise.load_interface(_args(checkpoints, name), torch.device(DEV))
    want = denoise_frame(itf, *_buffers(), True, batch_size=denoise.tile_batch_size(S, None, 192), want_pbuffers=True, patch_size=192,
                         pad_size=40, blend=8)
    assert denoise.tile_batch_size(S, None, 192) == 3
    got = np.load(tmp_path / "out" / "scene_denoised.npy")
    assert got.shape == (H, W, 3) and np.array_equal(got, want[0].cpu().numpy())
    assert np.array_equal(np.load(tmp_path / "out" / "scene_pbuffer.npy"), want[3]["diffuse"].permute(2, 3, 0, 1).cpu().numpy())
    with pytest.raises(ValueError, match="--blend 13"):
        denoise.main(argv[:argv.index("--blend")] + ["--blend", "13"] + argv[argv.index("--blend") + 2:])


def test_command_line_sample_based(tmp_path):
    """An SBMC checkpoint around ``standins.SampleDenoiserStandIn`` (188-pixel outputs of a 192-pixel tile: an inset of 2), made as
    tests/test_gpu_denoise_sample.py makes its own."""
    from wcmc_amd import denoise, ops, train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.datasets import dncnn_in_size
    from wcmc_amd.support.inference import denoise_sample_frame
    save = str(tmp_path)
    flags = ["--denoiser", "standins:SampleDenoiserStandIn", "--use_llpm_buf", "--disentangle", "m11r11", "--pnet_out_size", "3"]
    parse = lambda extra: train_kpcn.check_args(denoise.build_parser().parse_args(                   # noqa: E731
        ["--save", save, "--model_name", "SBMC_t", "--input", "unused", "--output_dir", "unused"] + flags + extra))
    args = parse([])
    torch.manual_seed(1)
    sizes = {"dncnn_in_size": dncnn_in_size("sbmc", True, False, True, 0), "pnet_in_size": 36, "pnet_out_size": 0}
    itfs, _ = denoise.sample_launcher("SBMC_t").init_model(sizes, args, torch.device(DEV))
    ckpt.save_checkpoint(os.path.join(save, "SBMC_t.pth"), itfs[0], 0, args)
    g = torch.Generator().manual_seed(11)
    raw = torch.rand((H, W, S, 104), generator=g) * 2.0 - 0.5
    raw[..., 66:] = raw[..., 66:].abs()
    raw[..., 60:66] = torch.randint(1, 32, (H, W, S, 6), generator=g).float()
    raw[..., 60][torch.rand((H, W), generator=g) < 0.1] = 0.0
    np.save(tmp_path / "scene.npy", raw.numpy())
    tile_flags = ["--tile", "192", "--tile_pad", "40", "--blend", "8"]
    argv = ["--input", str(tmp_path / "scene.npy"), "--output_dir", str(tmp_path / "out"), "--save", save, "--model_name", "SBMC_t"]
    times = denoise.main(argv + flags + tile_flags)
    assert (times[0]["tile"], times[0]["tile_pad"], times[0]["blend"], times[0]["tiles"]) == (192, 40, 8, 4)
    itf = denoise.load_interface(parse([]), torch.device(DEV))
    dev_raw = denoise.upload_raw(denoise.read_raw(str(tmp_path / "scene.npy"))[0], torch.device(DEV))
    ss, _ = ops.preprocess_sbmc(dev_raw)
    ll = ops.preprocess_llpm(dev_raw)
    run = lambda **kw: denoise_sample_frame(itf, ss, None, ll, True, True, False, 3, patch_size=192, pad_size=40, **kw)[0]   # noqa: E731
    got = np.load(tmp_path / "out" / "scene_denoised.npy")
    assert np.isfinite(got).all() and np.array_equal(got, run(blend=8).cpu().numpy())
    assert not np.array_equal(got, run().cpu().numpy())
    with pytest.raises(ValueError, match="--blend 39"):               # the inset of 2 is known after the first batch
        run(blend=39)
    run(blend=38)
