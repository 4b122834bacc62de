"""The P-buffer filter on the GPU (csrc/pbuffer_filter.hip, ops.pbuffer_filter, wcmc_amd.rhf, ``denoise --rhf``) against its fp64
restatement (tests/rhf_ref.py).

The bar is not fixed in advance: per case, the error of ``rhf_ref`` run in fp32 on the CPU against ``rhf_ref`` in fp64 -- the
reference's own fp32 error -- is measured on the same input, and the kernel must stay within ``FACTOR`` = 8 times that (hardware
reciprocal and exponential of 1 to 2 ulp each, and a different order over up to 441 terms).  Every case asserts that its input tests
the distance at all: in fp64 at least a quarter of the unmasked pixels have ``wsum >= 2`` and at least a quarter have ``wsum`` at most
half their in-image window count.  The measured ratios are written to ``test_reports/pbuffer_filter_error.txt``
(profiles/pbuffer_filter_error.txt is a copy of one run)."""
import functools
import os

import numpy as np
import pytest
import torch

from rhf_ref import rhf_ref, scene, window_count
from test_gpu_denoise import _args, _raw_frame, checkpoint  # noqa: F401      (the fixtures the denoise tests build)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("WCMC_TEST_REPORTS", os.path.join(ROOT, "test_reports"))     # (git-ignored)
DEV = "cuda:0"
FACTOR = 8.0
RECORDS = {}

# name -> (H, W, S, C, Cr, R, f, bandwidth, eps, image layout, p_buffer layout, mask)
# The base scene is the same for every case (rhf_ref.scene: a smaller S, C or Cr takes a slice of it).  eps = 1e-3 with b = 1 leaves
# wsum at 1.000 for S = 1 (v = 0) and near 1 for S = 2 and for the 7 x 7 patch of the small image: those cases raise eps or b until
# the condition above holds (found with the fp64 reference on the CPU).
CASES = {
    "5x7_R10_f3":     (5, 7, 5, 3, 3, 10, 3, 3.0, 1e-3, "hwc", "schw", False),     # smaller than the window and the patch
    "37x53_R10_f1":   (37, 53, 5, 3, 3, 10, 1, 1.0, 1e-3, "hwc", "schw", False),   # the default instance; tiles that do not divide
    "24x40_R6_f2":    (24, 40, 5, 3, 3, 6, 2, 1.0, 1e-3, "hwc", "schw", False),
    "24x40_R0":       (24, 40, 5, 3, 3, 0, 2, 1.0, 1e-3, "hwc", "schw", False),
    "24x40_R6_f0":    (24, 40, 5, 3, 3, 6, 0, 1.0, 1e-3, "hwc", "schw", False),
    "S1":             (24, 40, 1, 3, 3, 6, 1, 1.0, 0.1, "hwc", "schw", False),
    "S2":             (24, 40, 2, 3, 3, 6, 1, 2.0, 1e-3, "hwc", "schw", False),
    "S8":             (24, 40, 8, 3, 3, 6, 1, 1.0, 1e-3, "hwc", "schw", False),
    "C1":             (24, 40, 5, 1, 3, 6, 1, 1.0, 1e-3, "hwc", "schw", False),
    "C8":             (24, 40, 5, 8, 3, 6, 1, 1.0, 1e-3, "hwc", "schw", False),    # LDS-resident above the default LDS grant
    "C8_R10":         (24, 40, 5, 8, 3, 10, 1, 1.0, 1e-3, "hwc", "schw", False),
    "C32":            (24, 40, 5, 32, 3, 6, 1, 1.0, 1e-3, "hwc", "schw", False),   # too wide for LDS: statistics through the caches
    "Cr1":            (24, 40, 5, 3, 1, 6, 1, 1.0, 1e-3, "hwc", "schw", False),
    "Cr4":            (24, 40, 5, 3, 4, 6, 1, 1.0, 1e-3, "hwc", "schw", False),
    "views":          (37, 53, 5, 3, 3, 10, 1, 1.0, 1e-3, "chw", "hwsc", False),   # permuted CHW image, permuted (H, W, S, C) P-buffer
    "views_generic":  (24, 40, 5, 3, 3, 6, 2, 1.0, 1e-3, "chw", "hwsc", False),
    # tiles whose whole halo lies inside the image take the walk without flags (one tile each here: rows 16..23 / 8..15, columns 32..63)
    "inside_R10_f1":  (40, 80, 5, 3, 3, 10, 1, 1.0, 1e-3, "hwc", "schw", False),
    "inside_C8":      (24, 80, 5, 8, 3, 6, 1, 1.0, 1e-3, "hwc", "schw", False),
    "inside_C32":     (24, 80, 5, 32, 3, 6, 1, 1.0, 1e-3, "chw", "hwsc", False),
    "mask":           (37, 53, 5, 3, 3, 10, 1, 1.0, 1e-3, "hwc", "schw", True),
    "mask_generic":   (24, 40, 5, 8, 4, 6, 2, 1.0, 1e-3, "chw", "hwsc", True),
}


def _mask(h, w):
    """Holes on the border (a corner, a run of the top edge, one pixel of the right edge) and in the interior (a block, single pixels)."""
    m = torch.ones((h, w), dtype=torch.uint8)
    m[0, 0] = 0
    m[0, w // 2:w // 2 + 4] = 0
    m[h // 3, w - 1] = 0
    m[h - 1, 3] = 0
    m[h // 2 - 1:h // 2 + 2, 10:13] = 0
    m[5, 20] = m[h - 4, w - 7] = m[7, 8] = 0
    return m


@functools.lru_cache(maxsize=None)
def _case(name):
    """(image, p_buffer, mask, kw) on the host, the fp64 reference and the fp32 reference's errors; computed once."""
    h, w, s, c, cr, r, f, b, eps, _, _, masked = CASES[name]
    img, p = scene(h, w, s, c, cr)
    mask = _mask(h, w) if masked else None
    kw = dict(radius=r, patch_radius=f, bandwidth=b, eps=eps)
    o64, w64 = rhf_ref(img, p, mask=mask, **kw)
    o32, w32 = rhf_ref(img, p, mask=mask, dtype=torch.float32, **kw)
    return img, p, mask, kw, o64, w64, _errors(o32, w32, o64, w64)


def _errors(out, wsum, o64, w64):
    """max |out - fp64| / max |fp64|, and the maximum relative error of wsum over the pixels where it is not zero."""
    out, wsum = out.double().cpu(), wsum.double().cpu()
    nz = w64 != 0
    assert torch.equal(wsum[~nz], w64[~nz])
    return ((out - o64).abs().max() / o64.abs().max()).item(), ((wsum - w64).abs()[nz] / w64[nz]).max().item()


def _device_inputs(name):
    from wcmc_amd import ops  # noqa: F401
    img, p, mask = _case(name)[:3]
    il, pl = CASES[name][9:11]
    image = img.to(DEV) if il == "hwc" else img.permute(2, 0, 1).contiguous().to(DEV).permute(1, 2, 0)
    p_buffer = p.to(DEV) if pl == "schw" else p.permute(2, 3, 0, 1).contiguous().to(DEV).permute(2, 3, 0, 1)
    assert image.is_contiguous() == (il == "hwc" or image.shape[2] == 1) and p_buffer.is_contiguous() == (pl == "schw")
    return image, p_buffer, (mask.to(DEV) if mask is not None else None)


def _write_report():
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "pbuffer_filter_error.txt"), "w") as f:
        f.write("ops.pbuffer_filter against tests/rhf_ref.py in fp64; 'ref32': rhf_ref in fp32 on the CPU against the same; bar: ratio <= %g\n"
                % FACTOR)
        f.write("%-16s %-28s %10s %10s %7s %10s %10s %7s\n" % ("case", "H W S C Cr R f b eps", "out", "ref32", "ratio", "wsum", "ref32", "ratio"))
        for name, (eo, ew, ro, rw) in RECORDS.items():
            f.write("%-16s %-28s %10.3e %10.3e %7.2f %10.3e %10.3e %7.2f\n"
                    % (name, " ".join("%g" % v for v in CASES[name][:9]), eo, ro, eo / ro if ro else 0.0, ew, rw, ew / rw if rw else 0.0))


@pytest.mark.parametrize("name", list(CASES))
def test_against_fp64(name):
    from wcmc_amd import ops
    h, w, s, c, cr, r = CASES[name][:6]
    img, p, mask, kw, o64, w64, (ro, rw) = _case(name)
    image, p_buffer, m = _device_inputs(name)
    out, wsum = ops.pbuffer_filter(image, p_buffer, mask=m, **kw)
    assert out.shape == (h, w, cr) and out.is_contiguous() and wsum.shape == (h, w) and wsum.is_contiguous()
    live = torch.ones((h, w), dtype=torch.bool) if mask is None else mask != 0
    if r == 0:
        # one tap, weight exp(-0) = 1: no distance to test, and nothing to round
        assert torch.equal(out.cpu(), img) and torch.equal(wsum.cpu(), torch.ones(h, w))
        return
    # the input tests the distance: neither every weight near 1 nor every weight near 0
    cnt = window_count(h, w, r)
    many, few = (w64 >= 2)[live].double().mean().item(), (w64 <= 0.5 * cnt)[live].double().mean().item()
    print("%s: fp64 wsum %.3f..%.2f, %.2f of the pixels >= 2, %.2f <= half their window" % (name, w64[live].min(), w64[live].max(), many, few))
    assert many >= 0.25 and few >= 0.25
    eo, ew = _errors(out, wsum, o64, w64)
    RECORDS[name] = (eo, ew, ro, rw)
    _write_report()
    print("%s: out %.3e (fp32 reference %.3e, ratio %.2f), wsum %.3e (fp32 reference %.3e, ratio %.2f)"
          % (name, eo, ro, eo / ro, ew, rw, ew / rw))
    assert ro > 0 and rw > 0
    assert eo <= FACTOR * ro, "out: %.3e > %g x %.3e" % (eo, FACTOR, ro)
    assert ew <= FACTOR * rw, "wsum: %.3e > %g x %.3e" % (ew, FACTOR, rw)
    if mask is not None:
        dead = ~live
        assert torch.equal(out.cpu()[dead], img[dead]) and bool((wsum.cpu()[dead] == 0).all()) and bool((wsum.cpu()[live] >= 1).all())
    else:
        assert bool((wsum >= 1).all())


@pytest.mark.parametrize("name", ["37x53_R10_f1", "mask_generic", "C32"])
def test_two_runs_are_bitwise_equal(name):
    from wcmc_amd import ops
    image, p_buffer, m = _device_inputs(name)
    kw = _case(name)[3]
    a, b = ops.pbuffer_filter(image, p_buffer, mask=m, **kw), ops.pbuffer_filter(image, p_buffer, mask=m, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the two launches apart give what the one call gives
    ws = torch.empty(p_buffer.shape[1] * image.shape[0] * image.shape[1] * 2, device=DEV)
    ops.pbuffer_filter(image, p_buffer, mask=m, passes=ops.PBF_STATS, workspace=ws, **kw)
    c = ops.pbuffer_filter(image, p_buffer, mask=m, passes=ops.PBF_FILTER, workspace=ws, **kw)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize("name", ["inside_R10_f1", "inside_C8", "inside_C32"])
def test_a_mask_of_ones_changes_no_bit(name):
    """With a mask every tile takes the flagged walk; without one, the tile inside the image takes the walk without flags.  Both do
    the same operations in the same order: a pixel's bits do not depend on where the tiles fall."""
    from wcmc_amd import ops
    image, p_buffer, _ = _device_inputs(name)
    kw = _case(name)[3]
    a = ops.pbuffer_filter(image, p_buffer, **kw)
    b = ops.pbuffer_filter(image, p_buffer, mask=torch.ones(image.shape[:2], dtype=torch.uint8, device=DEV), **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ["mask", "mask_generic"])
def test_masked_pixels_change_only_the_pixels_whose_window_holds_them(name):
    """A masked q is left out of p's sums: against the unmasked run, only unmasked pixels with a masked pixel in their window
    change, and they lose weight (a sum of non-negative terms in a fixed order is monotone in every term); by how much is
    ``test_against_fp64``'s to say, which holds the masked run to the reference.  The mask's element type does not matter."""
    from wcmc_amd import ops
    mask, kw = _case(name)[2:4]
    image, p_buffer, m = _device_inputs(name)
    out, wsum = ops.pbuffer_filter(image, p_buffer, mask=m, **kw)
    out_all, wsum_all = ops.pbuffer_filter(image, p_buffer, **kw)
    live = mask != 0
    r = kw["radius"]
    near = torch.nn.functional.max_pool2d((~live).float()[None, None], 2 * r + 1, stride=1, padding=r)[0, 0] > 0
    wsum, wsum_all, out, out_all = wsum.cpu(), wsum_all.cpu(), out.cpu(), out_all.cpu()
    changed = wsum != wsum_all
    assert bool((changed[live] <= near[live]).all()) and bool(changed[live].any()) and 0 < int(near[live].sum())
    assert bool((wsum[live] <= wsum_all[live]).all())
    same = live & ~near
    assert torch.equal(out[same], out_all[same])
    # a float32 mask (``has_hit``) and a bool mask are the uint8 mask
    for other in (m.float() * 3.0, m.bool()):
        o2, w2 = ops.pbuffer_filter(image, p_buffer, mask=other, **kw)
        assert torch.equal(out, o2.cpu()) and torch.equal(wsum, w2.cpu())


@pytest.mark.parametrize("name,where", [("37x53_R10_f1", (2, 18, 30)), ("24x40_R6_f2", (1, 0, 39)), ("mask_generic", (0, 12, 11)),
                                        ("C32", (4, 23, 0))])
def test_one_nan_poisons_the_pixels_that_read_it_and_no_others(name, where):
    """``where``: (sample, row, column) of the NaN, in the last channel."""
    from wcmc_amd import ops
    img, p, mask, kw = _case(name)[:4]
    p = p.clone()
    p[where[0], -1, where[1], where[2]] = float("nan")
    o64, w64 = rhf_ref(img, p, mask=mask, **kw)
    image, _, m = _device_inputs(name)
    pl = CASES[name][10]
    p_buffer = p.to(DEV) if pl == "schw" else p.permute(2, 3, 0, 1).contiguous().to(DEV).permute(2, 3, 0, 1)
    out, wsum = ops.pbuffer_filter(image, p_buffer, mask=m, **kw)
    bad64 = torch.isnan(o64).any(dim=2)
    assert torch.equal(bad64, torch.isnan(o64).all(dim=2)) and torch.equal(bad64, torch.isnan(w64))
    assert 0 < int(bad64.sum()) < bad64.numel()
    assert torch.equal(torch.isnan(out).all(dim=2).cpu(), bad64) and torch.equal(torch.isnan(out).any(dim=2).cpu(), bad64)
    assert torch.equal(torch.isnan(wsum).cpu(), bad64)
    # ... and within (R + 2f) of the NaN; everything else is the clean run's, bit for bit
    clean, _ = ops.pbuffer_filter(image, _device_inputs(name)[1], mask=m, **kw)
    r, f = kw["radius"], kw["patch_radius"]
    reach = torch.zeros_like(bad64)
    reach[max(0, where[1] - r - 2 * f):where[1] + r + 2 * f + 1, max(0, where[2] - r - 2 * f):where[2] + r + 2 * f + 1] = True
    assert bool((bad64 <= reach).all())
    assert torch.equal(out.cpu()[~bad64], clean.cpu()[~bad64])


def test_rhf_filter_on_a_dict_equals_the_op_on_the_concatenated_tensor():
    from wcmc_amd import ops, rhf
    img, p, mask, kw = _case("mask_generic")[:4]
    image, p_buffer, m = img.to(DEV), p.to(DEV), mask.to(DEV).float()
    branches = {"specular": p_buffer[:, 3:], "diffuse": p_buffer[:, :3]}          # (views: the dict's tensors need not be contiguous)
    a = rhf.rhf_filter(image, branches, m, **kw)
    b = ops.pbuffer_filter(image, torch.cat([p_buffer[:, :3], p_buffer[:, 3:]], dim=1), mask=m, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = rhf.rhf_filter(image, p_buffer, m, **kw)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    d = rhf.rhf_filter(image, {"diffuse": p_buffer[:, :3]}, **kw)
    e = ops.pbuffer_filter(image, p_buffer[:, :3], **kw)
    assert torch.equal(d[0], e[0]) and torch.equal(d[1], e[1]) and not torch.equal(d[1], a[1])


def test_denoise_rhf_writes_the_filter_of_the_frame_it_denoised(checkpoint, tmp_path):  # noqa: F811
    from wcmc_amd import denoise, rhf
    from wcmc_amd.support.datasets import DenoisePreprocessor
    from wcmc_amd.support.inference import denoise_frame
    h, w = 64, 70
    scenes = tmp_path / "renders"
    scenes.mkdir()
    np.save(scenes / "scene.npy", _raw_frame(h, w, 2, seed=11))
    argv = lambda out, extra: ["--input", str(scenes / "scene.npy"), "--output_dir", str(tmp_path / out), "--save", checkpoint,   # noqa: E731
                               "--model_name", "KPCN_denoise_test", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE",
                               "--train_branches"] + extra
    denoise.main(argv("plain", ["--png"]))
    plain = sorted(os.listdir(tmp_path / "plain"))
    assert plain == ["scene_denoised.npy", "scene_denoised.pfm", "scene_denoised.png", "scene_input.png"]
    kw = dict(radius=6, patch_radius=2, bandwidth=1.5, eps=0.01)
    denoise.main(argv("rhf", ["--png", "--rhf", "--rhf_radius", "6", "--rhf_patch_radius", "2", "--rhf_bandwidth", "1.5", "--rhf_eps", "0.01"]))
    new = ["scene_rhf.npy", "scene_rhf.png", "scene_rhf_neighbours.npy", "scene_rhf_neighbours.png"]
    assert sorted(os.listdir(tmp_path / "rhf")) == sorted(plain + new)            # no P-buffer file: --save_pbuffer was not given
    for name in plain:
        assert open(tmp_path / "rhf" / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read(), name
    itf = denoise.load_interface(_args(checkpoint), torch.device(DEV))
    raw = denoise.upload_raw(denoise.read_raw(str(scenes / "scene.npy"))[0], torch.device(DEV))
    pre = DenoisePreprocessor()
    _, ipt, has_hit, out_path = denoise_frame(itf, pre._preprocess_kpcn(raw), pre._preprocess_llpm(raw), True, 8, want_pbuffers=True)
    assert set(out_path) == {"diffuse", "specular"} and 0 < float(has_hit.mean()) < 1
    out, wsum = rhf.rhf_filter(ipt, out_path, has_hit, **kw)
    got_out, got_wsum = np.load(tmp_path / "rhf" / "scene_rhf.npy"), np.load(tmp_path / "rhf" / "scene_rhf_neighbours.npy")
    assert got_out.dtype == got_wsum.dtype == np.float32 and got_out.shape == (h, w, 3) and got_wsum.shape == (h, w)
    assert got_out.tobytes() == out.cpu().numpy().tobytes() and got_wsum.tobytes() == wsum.cpu().numpy().tobytes()
    assert bool((wsum[has_hit == 0] == 0).all()) and bool((wsum[has_hit != 0] >= 1).all())
    assert torch.equal(out[has_hit == 0], ipt[has_hit == 0])
    for name in ("scene_rhf.png", "scene_rhf_neighbours.png"):
        assert open(tmp_path / "rhf" / name, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    # the defaults, without previews
    denoise.main(argv("defaults", ["--rhf"]))
    assert sorted(os.listdir(tmp_path / "defaults")) == ["scene_denoised.npy", "scene_denoised.pfm", "scene_rhf.npy",
                                                         "scene_rhf_neighbours.npy"]
    out, wsum = rhf.rhf_filter(ipt, out_path, has_hit)
    assert np.load(tmp_path / "defaults" / "scene_rhf_neighbours.npy").tobytes() == wsum.cpu().numpy().tobytes()


def test_stand_alone_command_round_trips_the_files_of_save_pbuffer(checkpoint, tmp_path):  # noqa: F811
    from wcmc_amd import denoise, ops, rhf
    h, w = 64, 70
    scenes = tmp_path / "renders"
    scenes.mkdir()
    np.save(scenes / "scene.npy", _raw_frame(h, w, 2, seed=11))
    out_dir = tmp_path / "out"
    denoise.main(["--input", str(scenes / "scene.npy"), "--output_dir", str(out_dir), "--save", checkpoint, "--model_name",
                  "KPCN_denoise_test", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--train_branches", "--save_pbuffer"])
    pb = np.load(out_dir / "scene_pbuffer.npy")
    assert pb.shape == (h, w, 2, 3)
    mask = (np.arange(h * w).reshape(h, w) % 7 != 0).astype(np.float32)
    np.save(tmp_path / "mask.npy", mask)
    paths = rhf.main(["--image", str(out_dir / "scene_denoised.npy"), "--pbuffer", str(out_dir / "scene_pbuffer.npy"), "--mask",
                      str(tmp_path / "mask.npy"), "--output_dir", str(tmp_path / "rhf"), "--radius", "5", "--patch_radius", "1",
                      "--bandwidth", "2.0", "--eps", "0.01", "--png"])
    assert [os.path.basename(p) for p in paths] == ["scene_denoised_rhf.npy", "scene_denoised_rhf_neighbours.npy",
                                                    "scene_denoised_rhf.png", "scene_denoised_rhf_neighbours.png"]
    assert sorted(os.listdir(tmp_path / "rhf")) == sorted(os.path.basename(p) for p in paths)
    image = torch.from_numpy(np.load(out_dir / "scene_denoised.npy")).to(DEV)
    p_buffer = torch.from_numpy(pb).to(DEV).permute(2, 3, 0, 1)
    out, wsum = ops.pbuffer_filter(image, p_buffer, 5, 1, 2.0, 0.01, mask=torch.from_numpy(mask).to(DEV))
    assert np.load(paths[0]).tobytes() == out.cpu().numpy().tobytes() and np.load(paths[1]).tobytes() == wsum.cpu().numpy().tobytes()
    assert float(wsum.max()) > 1.0
    png = open(paths[3], "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and len(png) > 100
