"""Full-scene evaluation (wcmc_amd.evaluate) on synthetic scene files laid out as the reference's evaluation data:
FullImageDataset against the reference's tiling restated in numpy, the stitch kernel against the slice copies of
support.inference.inference, and the CSVs of evaluate.denoise against the fp64 restatement of the metrics."""
import os

import numpy as np
import pytest
import torch

from image_eval_ref import evaluate as host_evaluate

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCENES = {"room": (256, 256), "car": (320, 192)}
SPPS = [8, 40]


def _write_scene(root, name, h, w, seed, llpm_spp=(32, 16), spps=SPPS):
    rng = np.random.default_rng(seed)
    kpcn = (rng.random((h, w, 44)) * 0.8).astype(np.float32)
    gt = (rng.random((h, w, 9)) * 0.9 + 0.05).astype(np.float32)
    gt[..., 0:3] += gt[..., 3:6]                                       # total >= diffuse: log(1 + total - diffuse) defined
    llpm = [rng.random((h, w, s, 37), dtype=np.float32) * 0.5 for s in llpm_spp]
    miss = rng.random((h, w)) < 0.1                                    # no first-bounce hit: descriptor 24 zero in every sample
    for a in llpm:
        a[miss, :, 25] = 0.0
    for d in ("KPCN/input", "KPCN/gt", "LLPM/input"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for spp in spps:
        np.save(os.path.join(root, "KPCN/input", "%s_kpcn_%d.npy" % (name, spp)), kpcn + 0.01 * spp)
    np.save(os.path.join(root, "KPCN/gt", name + ".npy"), gt)
    for n, a in enumerate(llpm):
        np.save(os.path.join(root, "LLPM/input", name + ("_llpm.npy" if n == 0 else "_llpm_%d.npy" % n)), a)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("scenes"))
    for n, (name, (h, w)) in enumerate(SCENES.items()):
        _write_scene(root, name, h, w, seed=100 + n)
    return root


def _reference_patches(root, name, spp):
    """datasets.py:1227-1297 (KPCN, use_llpm_buf) in numpy: the per-tile patch dictionaries and the frame attributes."""
    ip = os.path.join(root, "KPCN/input")
    _in = np.load(os.path.join(ip, "%s_kpcn_%d.npy" % (name, spp)))
    sample = {"kpcn_diffuse_in": np.concatenate([_in[..., :10], _in[..., 20:]], axis=2), "kpcn_specular_in": _in[..., 10:],
              "kpcn_diffuse_buffer": _in[..., :3], "kpcn_specular_buffer": _in[..., 10:13],
              "kpcn_albedo": _in[..., 34:37] + 0.00316}
    l0 = np.load(os.path.join(root, "LLPM/input", name + "_llpm.npy"))
    l1 = np.load(os.path.join(root, "LLPM/input", name + "_llpm_1.npy"))
    ll = (l0 if l0.shape[2] >= spp else np.concatenate((l0, l1), axis=2))[..., :spp, :]
    sample["kpcn_diffuse_in"] = np.concatenate((sample["kpcn_diffuse_in"], ll[..., :1].mean(2)), axis=2)
    sample["kpcn_specular_in"] = np.concatenate((sample["kpcn_specular_in"], ll[..., :1].mean(2)), axis=2)
    sample["paths"] = np.array(ll[..., 1:])
    g = np.load(os.path.join(root, "KPCN/gt", name + ".npy"))
    total, diffuse, albedo = g[:, :, 0:3], g[:, :, 3:6], g[:, :, 6:]
    sample["target_diffuse"] = diffuse / (albedo + 0.00316)
    sample["target_specular"] = np.log(1 + total - diffuse)
    sample["target_total"] = total
    has_hit = (np.mean(l0[..., 1:], 2)[..., 24:25] != 0.0).astype(np.float32)
    full_ipt = sample["kpcn_diffuse_buffer"] * sample["kpcn_albedo"] + np.exp(sample["kpcn_specular_buffer"]) - 1
    frame = {"has_hit": np.concatenate((has_hit,) * 3, axis=2), "full_ipt": full_ipt, "full_tgt": total}
    for k in sample:
        sample[k] = sample[k].transpose([2, 0, 1]) if sample[k].ndim == 3 else sample[k].transpose([2, 3, 0, 1])
    h, w = total.shape[:2]
    patches, coords = [], []
    for i in range(0, h - 64, 64):
        for j in range(0, w - 64, 64):
            i_start, j_start, i_end, j_end = i + 32, j + 32, i + 96, j + 96
            if i == 0:
                i_start = 0
            if j == 0:
                j_start = 0
            if i == h - 128:
                i_end = i + 128
            if j == w - 128:
                j_end = j + 128
            coords.append((i_start, j_start, i_end, j_end, i, j))
            patches.append({k: v[..., i:i + 128, j:j + 128] for k, v in sample.items()})
    return patches, coords, frame


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("spp", SPPS)
def test_full_image_dataset_matches_the_reference_tiling(data, name, spp):
    from wcmc_amd.support.datasets import FullImageDataset
    ds = FullImageDataset(os.path.join(data, "KPCN/input", name + ".npy"), spp, "kpcn", True, False, True, 3, device=DEV)
    patches, coords, frame = _reference_patches(data, name, spp)
    assert (ds.h, ds.w) == SCENES[name] and ds.coords == coords and len(ds) == len(coords)
    assert ds.batch_size == (8 if spp <= 32 else 4)
    n = 0
    for batch, i_start, j_start, i_end, j_end, i, j in ds:
        assert len(i_start) == batch["target_total"].shape[0] <= ds.batch_size
        for b in range(len(i_start)):
            assert (i_start[b], j_start[b], i_end[b], j_end[b], i[b], j[b]) == coords[n]
            ref = patches[n]
            assert set(batch) == set(ref), set(batch) ^ set(ref)
            for k in ref:
                np.testing.assert_allclose(batch[k][b].cpu().numpy(), ref[k], rtol=1e-6, atol=1e-7, err_msg=k)
            n += 1
    assert n == len(coords)
    np.testing.assert_array_equal(ds.has_hit.cpu().numpy(), frame["has_hit"])
    np.testing.assert_array_equal(ds.full_tgt.cpu().numpy(), frame["full_tgt"])
    # exp on the device vs numpy's: an ulp apart at most, and `- 1` cancels (ulp of the sum up to 2.4e-7 here)
    np.testing.assert_allclose(ds.full_ipt.cpu().numpy(), frame["full_ipt"], rtol=1e-6, atol=5e-7)
    assert 0 < float(ds.has_hit.mean()) < 1


class _TileModel:
    """A stand-in interface whose outputs are a fixed function of the batch (92 x 92 radiance, two P-buffers)."""

    def to_eval_mode(self):
        pass

    def validate_batch(self, batch):
        rad = batch["kpcn_diffuse_buffer"][:, :, 18:110, 18:110] * 3.0 + batch["target_total"][:, :, 18:110, 18:110]
        p = {"diffuse": batch["paths"][:, :, 0:3] * 2.0, "specular": batch["paths"][:, :, 3:6] - 1.0}
        return rad, p


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("spp", SPPS)
def test_stitched_inference_is_bit_identical_to_the_slice_copies(data, name, spp):
    from wcmc_amd.support.datasets import FullImageDataset
    from wcmc_amd.support.inference import inference, stitched_inference
    ds = FullImageDataset(os.path.join(data, "KPCN/input", name + ".npy"), spp, "kpcn", True, False, True, 3, device=DEV)
    h, w = SCENES[name]
    rad_a, path_a = inference(_TileModel(), ds, h, w)
    rad_b, path_b = stitched_inference(_TileModel(), ds)
    assert torch.equal(rad_a, rad_b)
    assert set(path_a) == set(path_b) == {"diffuse", "specular"}
    for k in path_a:
        assert path_a[k].shape == (spp, 3, h, w) and torch.equal(path_a[k], path_b[k]), k


def _args(save, extra=()):
    from wcmc_amd import evaluate
    return evaluate.build_parser().parse_args(
        ["--save", save, "--model_name", "KPCN_eval_test", "--input_dir", "unused", "--use_llpm_buf", "--manif_learn",
         "--manif_loss", "FMSE", "--train_branches"] + list(extra))


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from wcmc_amd import train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    save = str(tmp_path_factory.mktemp("weights"))
    args = _args(save)
    torch.manual_seed(0)
    sizes = {"dncnn_in_size": 34 + 3 + 2, "pnet_in_size": 36, "pnet_out_size": 3}
    itfs, _ = train_kpcn.init_model(sizes, args, torch.device(DEV))
    torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, "KPCN_eval_test.pth"))
    return save


def test_denoise_writes_both_csvs_with_the_metrics_of_the_denoised_frames(data, checkpoint, tmp_path):
    from wcmc_amd import evaluate
    args = _args(checkpoint)
    frames = {}
    out_dir = str(tmp_path / "out")
    res, res_in = evaluate.denoise(args, os.path.join(data, "KPCN/input"), out_dir, scenes=list(SCENES), spps=SPPS,
                                   device=DEV, frames=frames)
    a = np.loadtxt(os.path.join(out_dir, "results_KPCN_eval_test_40.csv"), delimiter=",")
    b = np.loadtxt(os.path.join(out_dir, "results_input_40.csv"), delimiter=",")
    assert a.shape == b.shape == (20 * len(SPPS), len(SCENES))
    np.testing.assert_array_equal(a, res)
    np.testing.assert_array_equal(b, res_in)
    for i, scene in enumerate(SCENES):
        for j, spp in enumerate(SPPS):
            out, ipt, tgt = (x.cpu().numpy() for x in frames[(scene, spp)])
            assert out.shape == (SCENES[scene][0] - 56, SCENES[scene][1] - 56, 3)
            want = host_evaluate(out, ipt, tgt)
            for t in range(4):
                for k in range(5):
                    for got, wv in ((a[(5 * t + k) * len(SPPS) + j, i], want[0, t, k]),
                                    (b[(5 * t + k) * len(SPPS) + j, i], want[1, t, k])):
                        tol = 2e-6 if k == 2 else 1e-6 * abs(wv)
                        assert abs(got - wv) <= tol, (scene, spp, t, k, got, wv)
    # the network did something other than copy the input
    assert not np.allclose(a, b)


def test_denoise_rhf_saves_the_diffuse_p_buffer(data, checkpoint, tmp_path):
    from wcmc_amd import evaluate
    out_dir = str(tmp_path / "rhf")
    os.makedirs(out_dir)
    assert evaluate.denoise(_args(checkpoint), os.path.join(data, "KPCN/input"), out_dir, scenes=["car"], spps=[8],
                            rhf=True, device=DEV) is None
    p = np.load(os.path.join(out_dir, "p_buffer_car_KPCN_eval_test.npy"))
    assert p.shape == (320, 192, 8, 3)
