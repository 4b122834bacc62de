"""``wcmc_amd.evaluate`` with trained SBMC / LBMC models: a 128 x 192 scene directory (the smallest two-tile frame ``tile_coords`` takes
with a non-empty valid crop, 72 x 136) at 2 spp, written from a synthetic raw frame by ``DenoiseDirectory.offline_preprocess(sbmc=True)``
in the test mode.  The command's rows are held to the slice loop of ``support.inference.inference`` over the dataset's own iteration,
the crop and ``metrics.evaluate_frame`` -- the same kernels on the same inputs, so the comparison is exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W, SPP = 128, 192, 2
MODELS = {"SBMC_e": ["--disentangle", "m11r11", "--pnet_out_size", "3"],
          "LBMC_e": ["--disentangle", "m11r01", "--pnet_out_size", "4"]}


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    """<root>/test/{gt,input}/scene.npy and the files ``offline_preprocess`` writes beside the input."""
    from wcmc_amd.support.datasets import DenoiseDirectory
    root = tmp_path_factory.mktemp("scenes")
    g = torch.Generator().manual_seed(11)
    raw = torch.rand((H, W, SPP, 104), generator=g) * 2.0 - 0.5
    raw[..., 66:] = raw[..., 66:].abs()                           # what preprocess_llpm takes logarithms and roots of
    raw[..., 60:66] = torch.randint(1, 32, (H, W, SPP, 6), generator=g).float()
    raw[..., 60][torch.rand((H, W), generator=g) < 0.1] = 0.0      # the first bounce's type: no surface hit on ~10 % of the pixels
    gt = torch.rand((H, W, 9), generator=g) * 1.5
    for sub, arr in (("gt", gt), ("input", raw)):
        os.makedirs(root / "test" / sub)
        np.save(root / "test" / sub / "scene.npy", arr.numpy())
    DenoiseDirectory(str(root), SPP, "test", device=DEV, base_model="sbmc").offline_preprocess(llpm=True, kpcn=False, sbmc=True)
    assert sorted(os.listdir(root / "test" / "input")) == ["scene.npy", "scene_llpm.npy", "scene_sbmc_p.npy", "scene_sbmc_s.npy"]
    return str(root / "test" / "input") + os.sep


def _args(save, name, extra=()):
    from wcmc_amd import evaluate, train_kpcn
    return train_kpcn.check_args(evaluate.build_parser().parse_args(
        ["--save", save, "--model_name", name, "--input_dir", "unused", "--denoiser", "standins:SampleDenoiserStandIn",
         "--use_llpm_buf"] + MODELS[name] + list(extra)))


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    from wcmc_amd import denoise
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.datasets import dncnn_in_size
    save = str(tmp_path_factory.mktemp("weights"))
    for name in MODELS:
        args = _args(save, name)
        torch.manual_seed(2)
        sizes = {"dncnn_in_size": dncnn_in_size("sbmc", True, False, True, 0), "pnet_in_size": 36, "pnet_out_size": 0}
        itfs, _ = denoise.sample_launcher(name).init_model(sizes, args, torch.device(DEV))
        ckpt.save_checkpoint(os.path.join(save, name + ".pth"), itfs[0], 0, args)
    return save


@pytest.mark.parametrize("name", list(MODELS))
def test_rows_equal_the_slice_loop_and_the_csvs_are_written(scene_dir, checkpoints, tmp_path, name):
    from wcmc_amd import denoise, evaluate
    from wcmc_amd.support import metrics as M
    from wcmc_amd.support.datasets import SampleFullImageDataset
    from wcmc_amd.support.inference import inference
    out_dir = str(tmp_path / "out")
    frames = {}
    results, results_input = evaluate.denoise(_args(checkpoints, name), scene_dir, out_dir, ["scene"], [SPP], device=DEV, frames=frames)
    assert results.shape == results_input.shape == (20, 1) and np.isfinite(results).all()
    assert frames[("scene", SPP)][0].shape == (72, 136, 3)

    args = _args(checkpoints, name)
    itf = denoise.load_interface(args, torch.device(DEV))
    ds = SampleFullImageDataset(scene_dir + "scene.npy", SPP, "sbmc", args.use_g_buf, args.use_sbmc_buf, args.use_llpm_buf, 0, device=DEV)
    assert len(ds) == 2 and ds.sbmc_p is None
    rad, path = inference(itf, iter(ds), H, W, 128, use_llpm_buf=True)
    assert path.shape == (SPP, 3 if name.startswith("SBMC") else 2, H, W)
    crop = (128 - 72) // 2
    cut = lambda t: t[crop:-crop, crop:-crop]                     # noqa: E731
    row_out, row_ipt = M.evaluate_frame(cut(rad.permute(1, 2, 0)), cut(ds.full_ipt), cut(ds.full_tgt), cut(ds.has_hit))
    assert np.array_equal(results[:, 0], np.asarray(row_out, dtype=np.float64))
    assert np.array_equal(results_input[:, 0], np.asarray(row_ipt, dtype=np.float64))
    assert 0 < float(ds.has_hit.mean()) < 1 and not np.array_equal(results, results_input)
    np.testing.assert_array_equal(np.loadtxt(os.path.join(out_dir, "results_%s_%d.csv" % (name, SPP)), delimiter=","), results[:, 0])
    np.testing.assert_array_equal(np.loadtxt(os.path.join(out_dir, "results_input_%d.csv" % SPP), delimiter=","), results_input[:, 0])


def test_rhf_saves_the_tensor_p_buffer_and_stops(scene_dir, checkpoints, tmp_path):
    from wcmc_amd import evaluate
    out_dir = str(tmp_path / "out")
    assert evaluate.denoise(_args(checkpoints, "LBMC_e"), scene_dir, out_dir, ["scene"], [SPP], rhf=True, device=DEV) is None
    p = np.load(os.path.join(out_dir, "p_buffer_scene_LBMC_e.npy"))
    assert p.shape == (H, W, SPP, 2) and np.isfinite(p).all() and np.abs(p).max() > 0
    assert not [f for f in os.listdir(out_dir) if f.endswith(".csv")]
