"""Host-side checks of the evaluation feature: the fp64 restatement the GPU kernel is tested against (tests/image_eval_ref.py)
against the reference's goldens and a direct SSIM loop, the tone map on hand-computed pixels, the CSV layout and tile table of
wcmc_amd.evaluate, and the argument checks of the three new ABI entries (no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest

import image_eval_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")


def test_restatement_reproduces_the_reference_goldens():
    d = np.load(GOLDEN)
    assert int(d["n_cases"]) >= 4
    for n in range(int(d["n_cases"])):
        p = "c%d_" % n
        im, ref = d[p + "im"].astype(np.float64), d[p + "ref"].astype(np.float64)
        for name, got in (("MSE", R.mse(im, ref)), ("RelMSE", R.rel_mse(im, ref)), ("L1", R.l1(im, ref)),
                          ("RelL1", R.rel_l1(im, ref)), ("TRelMSE", R.rel_mse(R.tm_reinhard(im), R.tm_reinhard(ref))),
                          ("RelMSE_eps1e-2", R.rel_mse(im, ref, eps=1e-2))):
            want = float(d[p + name])
            assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-6 * abs(want), (n, name, got, want)
        np.testing.assert_allclose(R.tm_reinhard(im), d[p + "tonemap_im"], rtol=1e-6, equal_nan=True)
        assert d[p + "RelMSE_full"].size < im.size or n in (0, 2, 4)       # NaN entries dropped where there are NaNs
    assert np.isnan(R.rel_mse(np.full((7, 7, 3), np.nan), np.ones((7, 7, 3))))


@pytest.mark.parametrize("h,w", [(7, 7), (9, 12), (15, 8)])
def test_ssim_restatement_equals_a_direct_window_loop(h, w):
    rng = np.random.default_rng(h * w)
    a = rng.lognormal(0, 1.5, (h, w, 3))
    b = a * rng.lognormal(0, 0.2, (h, w, 3))
    assert abs(R.ssim(a, b) - R.ssim_direct(a, b)) <= 1e-12
    assert R.ssim(a, a) == pytest.approx(1.0, abs=1e-14)
    assert 1.0 - R.ssim(a, a) == pytest.approx(0.0, abs=1e-14)


def test_tonemap_on_hand_computed_pixels():
    c = np.array([[[1.0, 2.0, 0.5], [-1.0, 0.0, 3.0], [100.0, 100.0, 100.0]]])
    got = R.tonemap(c)
    lum = 0.2126 * 1.0 + 0.7152 * 2.0 + 0.0722 * 0.5                  # 1.6791
    np.testing.assert_allclose(got[0, 0], [(v / (1 + lum / 1.5)) ** (1 / 2.2) for v in (1.0, 2.0, 0.5)], rtol=1e-15)
    lum = -0.2126 + 3 * 0.0722
    assert got[0, 1, 0] == 0.0 and got[0, 1, 1] == 0.0
    assert got[0, 1, 2] == pytest.approx(min(1.0, (3.0 / (1 + lum / 1.5)) ** (1 / 2.2)))
    assert (100 / (1 + 100 / 1.5)) ** (1 / 2.2) > 1.0 and np.all(got[0, 2] == 1.0)      # clipped to <= 1
    assert R.tonemap28(c)[0, 0, 0] == pytest.approx((1.0 / (1 + 1.6791 / 1.5)) ** (1 / 2.8))
    assert np.isnan(R.tonemap(np.full((1, 1, 3), np.nan))).all()
    np.testing.assert_allclose(R.tm_reinhard(np.array([-2.0, 0.0, 1.0, 3.0])), [0, 0, 0.5, 0.75])


def test_csv_layout_and_tile_table():
    from wcmc_amd.support import metrics as M
    from wcmc_amd.support.inference import tile_coords
    assert M.TONEMAPS == ("linear", "_tonemap", "tonemap", "tonemap28")
    assert M.METRICS == ("RelMSE", "RelL1", "DSSIM", "L1", "MSE")
    # results[(5*t + k)*len(spps) + j][i]: the reference's row of (tone map t, metric k, spp j) for scene i
    spps = [2, 8, 32]
    rows = {(t, k, j): (5 * t + k) * len(spps) + j for t in range(4) for k in range(5) for j in range(3)}
    assert sorted(rows.values()) == list(range(20 * len(spps)))
    assert rows[(2, 0, 1)] == 31
    c = tile_coords(256, 320)
    assert len(c) == 3 * 4 and c[0] == (0, 0, 96, 96, 0, 0) and c[-1] == (160, 224, 256, 320, 128, 192)
    own = np.zeros((256, 320), int)
    for i0, j0, i1, j1, _, _ in c:
        own[i0:i1, j0:j1] += 1
    assert (own == 1).all()                                           # every pixel owned by exactly one tile
    with pytest.raises(AssertionError):
        tile_coords(250, 320)
    from wcmc_amd import ops
    ops.check_tile_coords(c, 256, 320, 128)
    with pytest.raises(ValueError):
        ops.check_tile_coords([(0, 0, 97, 96, 0, 0)], 256, 320, 96)


def test_full_image_dataset_batch_sizes_and_unsupported_models():
    from wcmc_amd.support.datasets import FullImageDataset
    with pytest.raises(NotImplementedError):
        FullImageDataset(os.sep.join(["", "d", "input", "s.npy"]), 8, "sbmc")
    with pytest.raises(RuntimeError, match="spp"):
        FullImageDataset(os.sep.join(["", "d", "input", "s.npy"]), 128, "kpcn", device="cpu")
    with pytest.raises(FileNotFoundError):
        FullImageDataset(os.sep.join(["", "nonexistent", "input", "s.npy"]), 8, "kpcn", device="cpu")


def test_new_abi_entries_reject_bad_arguments_without_touching_the_gpu():
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert L.wcmc_image_eval_workspace_bytes(6, 100) == 0 and L.wcmc_image_eval_workspace_bytes(100, 6) == 0
    assert L.wcmc_image_eval_workspace_bytes(1224, 1224) == 39 * 153 * 48 * 8
    ws = L.wcmc_image_eval_workspace_bytes(64, 64)
    cases = {
        "null out": ("wcmc_image_eval", (null, 0, 0, 0, one, 0, 0, 0, one, 0, 0, 0, null, 0, 0, 0, 64, 64, 1e-4, one, one, ws,
                                         null)),
        "below 7x7": ("wcmc_image_eval", (one, 0, 0, 0, one, 0, 0, 0, one, 0, 0, 0, null, 0, 0, 0, 6, 64, 1e-4, one, one,
                                          ws, null)),
        "workspace": ("wcmc_image_eval", (one, 0, 0, 0, one, 0, 0, 0, one, 0, 0, 0, null, 0, 0, 0, 64, 64, 1e-4, one, one,
                                          ws - 8, null)),
        "eps": ("wcmc_image_eval", (one, 0, 0, 0, one, 0, 0, 0, one, 0, 0, 0, null, 0, 0, 0, 64, 64, 0.0, one, one, ws, null)),
        "stitch null": ("wcmc_stitch_tiles", (null, 0, 0, 0, 0, 92, 92, null, null, 0, 0, 128, one, 2, 256, 256, one, null,
                                              null, null)),
        "stitch shape": ("wcmc_stitch_tiles", (one, 0, 0, 0, 0, 92, 130, null, null, 0, 0, 128, one, 2, 256, 256, one, null,
                                               null, null)),
        "stitch pbuf": ("wcmc_stitch_tiles", (one, 0, 0, 0, 0, 92, 92, one, null, 8, 3, 128, one, 2, 256, 256, one, null,
                                              null, null)),
    }
    for what, (name, args) in cases.items():
        rc = getattr(L, name)(*args)
        assert rc < 0, what
        msg = L.wcmc_last_error().decode()
        assert msg and name.replace("wcmc_", "") in msg, (what, msg)
    assert L.wcmc_image_eval(*cases["workspace"][1]) == -3


def test_ops_image_eval_fails_loudly_on_cpu_tensors():
    import torch
    from wcmc_amd import ops
    x = torch.zeros((8, 8, 3))
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.image_eval(x, x, x)


def test_evaluate_command_line():
    from wcmc_amd import evaluate
    a = evaluate.build_parser().parse_args(["--save", "w", "--model_name", "KPCN_x", "--input_dir", "d/input", "--scenes",
                                            "a", "b", "--spps", "8", "32", "--use_llpm_buf", "--save_figures"])
    assert a.spps == [8, 32] and a.scenes == ["a", "b"] and a.save_figures and not a.rhf and a.use_llpm_buf
    assert a.pnet_out_size == [3] and a.disentangle == "m11r11"
