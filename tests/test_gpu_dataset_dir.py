"""GPU tests of training from a dataset directory: the sampling-map kernels (``wcmc_amd/csrc/sampling_map.hip``) against
goldens of the reference (``tests/golden/sampling_map.npz``, written by ``tests/golden/make_golden_dataset.py``), the offline
writer and the loader of ``support.datasets.DenoiseDirectory`` on directories generated into ``tmp_path``, and the training
CLI with ``--from_data_dir`` in a child process.

Bars of the golden comparisons: the reference's own rounding floor is recorded with each expected output -- the largest gap
between the reference on the fp32 input and the same reference functions on that input cast to fp64 (for the probability map
relative to the fp64 map's maximum).  The bar is 4 x that floor (a different but fixed summation order), never below 1e-6.
  importance_map  floors 9.9e-6 .. 1.5e-5 on the [0, 1] map -> bars 3.9e-5 .. 6.1e-5; measured error of the kernel on one MI355X: 0 on all four
                  (the Gaussian accumulates in fp64 in scipy's order and rounds where scipy rounds)
  sampling_prob   floors 6.9e-5 / 7.7e-5 / 1.26e-4 (2, 3, 8 spp) of the map's maximum -> bars 2.8e-4 / 3.1e-4 / 5.0e-4; measured
                  error: 3.5e-5 / 7.6e-6 / 1.2e-5 (powf of the tone map differs from numpy's in the last place, and the Sobel
                  differences of the blurred luminance amplify it)
Each test prints its floor, bar and measured error before it asserts (run with -s).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden as mg  # noqa: E402
import make_golden_dataset as mgd  # noqa: E402

DEV = "cuda:0"
PATCH = 64                                            # patch size of the directory tests (192 x 160 frames)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "sampling_map.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _same_bits(a, b):
    """Bitwise equality of two fp32 arrays / tensors (a NaN equals the same NaN: a planted 1e38 overflows the variances)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------- 1. importance_map
@pytest.mark.parametrize("name", list(mgd.IMAGES))
def test_importance_map_matches_the_reference(gold, name):
    from wcmc_amd import ops
    h, w, c, seed = mgd.IMAGES[name]
    img = gold["imp/%s/img" % name]
    assert np.array_equal(img, mgd.test_image(h, w, c, seed))
    assert (h < 124) == name.endswith("small")        # the small images are shorter than the Gaussian radius
    want, floor = gold["imp/%s/out" % name], float(gold["imp/%s/floor" % name])
    bar = max(4.0 * floor, 1e-6)
    got = ops.importance_map(_dev(img))
    assert got.shape == (h, w) and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print("importance_map %s: floor %.3e bar %.3e error %.3e" % (name, floor, bar, err))
    assert err <= bar, (name, err, bar)
    assert torch.equal(got, ops.importance_map(_dev(img))), "two calls must agree bitwise"
    assert 0.0 <= float(got.min()) and float(got.max()) <= 1.0


def test_importance_map_of_a_constant_image_is_zero():
    from wcmc_amd import ops
    for shape in ((70, 50), (130, 140, 3)):
        got = ops.importance_map(torch.full(shape, 0.625, device=DEV))
        assert got.shape == shape[:2] and not bool(torch.isnan(got).any()) and float(got.abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.importance_map(torch.zeros(8, 8, 2, device=DEV))


# ------------------------------------------------------------------------------------------------- 2. sampling_prob
def _prob_inputs(gold, name):
    h, w, s, patch, seed, gseed = (int(v) for v in gold["prob/%s/params" % name])
    raw, gt = mg.raw_samples(h, w, s, seed), mgd.test_gt(h, w, gseed)
    assert mgd.raw_checksum(raw) == int(gold["prob/%s/raw_crc" % name]), "the regenerated raw samples differ from the golden's"
    assert np.array_equal(gt[..., :3], gold["prob/%s/gt3" % name])
    return raw, gt, patch


@pytest.mark.parametrize("name", list(mgd.PROBS))
def test_sampling_prob_matches_the_reference_offline_block(gold, name):
    from wcmc_amd import ops
    raw, gt, patch = _prob_inputs(gold, name)
    h, w = gt.shape[:2]
    want, floor = gold["prob/%s/out" % name], float(gold["prob/%s/floor" % name])
    bar = max(4.0 * floor, 1e-6)
    d_raw, d_gt = _dev(raw), _dev(gt)
    got = ops.sampling_prob(d_raw, d_gt, patch)
    assert got.shape == (h - patch, w - patch) and got.dtype == torch.float32
    g = got.cpu().numpy().astype(np.float64)
    err = float(np.abs(g - want).max() / want.max())
    print("sampling_prob %s: floor %.3e bar %.3e error %.3e (of the map's maximum)" % (name, floor, bar, err))
    assert err <= bar, (name, err, bar)
    assert float(g.min()) >= 0.0
    # divided by (sum + 1e-5), the map sums to S / (S + 1e-5) = 1 - 1e-5 / S within fp32 rounding (each of the entries is one
    # rounded quotient; the sum here is taken in fp64).  S > 100 on these fixtures: the material term alone averages above 0.1
    # over more than 3000 pixels
    t = g.sum()
    assert abs(t - 1.0) <= 4 * np.finfo(np.float32).eps + 1e-5 / 100.0, t
    assert abs(t - float(want.astype(np.float64).sum())) <= 4 * np.finfo(np.float32).eps
    assert torch.equal(got, ops.sampling_prob(d_raw, d_gt, patch)), "two calls must agree bitwise"
    with pytest.raises(ValueError, match="larger than the patch"):
        ops.sampling_prob(d_raw, d_gt, h)


def test_sanitize_rule_on_the_device():
    from wcmc_amd import ops
    from wcmc_amd.support.datasets import sanitized
    x = np.random.RandomState(5).randn(1000, 37).astype(np.float32)
    x[3, 4], x[5, 6], x[7, 8], x[9, 10], x[11, 12] = np.nan, np.inf, -np.inf, 3e38, 1e38
    t = _dev(x)
    assert ops.sanitize_(t) is t
    assert np.array_equal(t.cpu().numpy(), sanitized(x))
    assert [float(t[i, j]) for i, j in ((3, 4), (5, 6), (7, 8), (9, 10), (11, 12))] == [float(np.float32(1e38))] * 5


# ------------------------------------------------------------------------------------------------- directories
def _gt(h, w, seed):
    gt = mgd.test_gt(h, w, seed)
    gt[..., 0:3] += 0.25                               # total > diffuse: log(1 + total - diffuse) is defined
    return gt


def _write_scene(root, mode, name, h, w, s, seed, continuations=(), plant=False):
    for d in ("gt", "input"):
        os.makedirs(os.path.join(root, mode, d), exist_ok=True)
    raw, gt = mg.raw_samples(h, w, s, seed), _gt(h, w, seed + 1)
    if plant:
        raw[3, 4, 0, 2], raw[5, 6, 1, 69], raw[7, 8, 0, 80] = np.nan, np.inf, -np.inf
        gt[2, 3, 0], gt[4, 5, 4], gt[6, 7, 8] = np.nan, np.inf, 2e38
    np.save(os.path.join(root, mode, "input", name + ".npy"), raw)
    np.save(os.path.join(root, mode, "gt", name + ".npy"), gt)
    conts = []
    for k, sk in enumerate(continuations, 1):
        conts.append(mg.raw_samples(h, w, sk, seed + 10 * k))
        np.save(os.path.join(root, mode, "input", "%s_%d.npy" % (name, k)), conts[-1])
    return raw, gt, conts


def _listing(root, mode):
    out = {}
    for d in ("gt", "input"):
        for f in os.listdir(os.path.join(root, mode, d)):
            out[d + "/" + f] = os.stat(os.path.join(root, mode, d, f)).st_mtime_ns
    return out


@pytest.fixture(scope="module")
def train_dir(tmp_path_factory):
    """Two scenes of 192 x 160 at 3 samples on disk (2 are read), a NaN / Inf planted in the first; preprocessed at 2 spp."""
    from wcmc_amd.support.datasets import DenoiseDirectory
    root = str(tmp_path_factory.mktemp("data"))
    scenes = {"room": _write_scene(root, "train", "room", 192, 160, 3, 300, plant=True),
              "car": _write_scene(root, "train", "car", 192, 160, 3, 400)}
    before = _listing(root, "train")
    d = DenoiseDirectory(root, 2, "train", batch_size=4, device=DEV, patch_size=PATCH, use_llpm_buf=True)
    report = d.offline_preprocess()
    return root, scenes, d, before, report


def test_offline_preprocess_writes_the_expected_files_once(train_dir):
    from wcmc_amd.support.datasets import DenoiseDirectory
    root, scenes, d, before, report = train_dir
    after = _listing(root, "train")
    want = set()
    for name in scenes:
        want |= {"gt/%s.npy" % name, "input/%s.npy" % name, "input/%s_kpcn_2.npy" % name, "input/%s_llpm.npy" % name,
                 "input/%s_prob_imp.npy" % name}
    assert set(after) == want, set(after) ^ want
    # the raw files are left alone; only the planted gt is rewritten (the other is already clean fp32)
    assert all(after["input/%s.npy" % n] == before["input/%s.npy" % n] for n in scenes)
    assert after["gt/room.npy"] != before["gt/room.npy"] and after["gt/car.npy"] == before["gt/car.npy"]
    by_scene = {e[0]: [os.path.basename(f) for f in e[1]] for e in report}
    assert sorted(by_scene["room"]) == sorted(["room_llpm.npy", "room_kpcn_2.npy", "room.npy", "room_prob_imp.npy"])
    assert sorted(by_scene["car"]) == sorted(["car_llpm.npy", "car_kpcn_2.npy", "car_prob_imp.npy"])
    # a second call writes nothing
    again = d.offline_preprocess()
    assert all(e[1] == [] for e in again) and _listing(root, "train") == after
    # overwrite=True rewrites everything but the raw input
    d.offline_preprocess(overwrite=True)
    third = _listing(root, "train")
    for k in want:
        assert (third[k] == after[k]) == (k in ("input/room.npy", "input/car.npy")), k


def test_offline_files_equal_the_preprocessor_applied_directly(train_dir):
    from wcmc_amd import ops
    from wcmc_amd.support.datasets import DenoisePreprocessor, sanitized
    root, scenes, d, _, _ = train_dir
    pre = DenoisePreprocessor()
    for name, (raw, gt, _) in scenes.items():
        inp = os.path.join(root, "train", "input", name)
        x = _dev(sanitized(raw[:, :, :2]))
        assert _same_bits(np.load(inp + "_kpcn_2.npy"), pre._preprocess_kpcn(x))
        assert _same_bits(np.load(inp + "_llpm.npy"), pre._preprocess_llpm(x))
        g = np.load(os.path.join(root, "train", "gt", name + ".npy"))
        assert g.dtype == np.float32 and np.array_equal(g, sanitized(gt))
        p = np.load(inp + "_prob_imp.npy")
        assert p.shape == (192 - PATCH, 160 - PATCH) and p.dtype == np.float32
        assert _same_bits(p, ops.sampling_prob(x, _dev(sanitized(gt)), PATCH))
    g = np.load(os.path.join(root, "train", "gt", "room.npy"))
    assert g[2, 3, 0] == g[4, 5, 4] == g[6, 7, 8] == np.float32(1e38)


def test_test_mode_output_feeds_full_image_dataset_and_evaluate(tmp_path):
    """``offline_preprocess`` in the test mode: 2 samples in the main file and 2 in one continuation file reach 2 and 4 spp of
    the 2, 4, 8, ... series; then ``FullImageDataset`` and ``evaluate.denoise`` on nothing but what the tool wrote."""
    from wcmc_amd import evaluate, train_kpcn
    from wcmc_amd.preprocess import main as preprocess_main
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.datasets import DenoisePreprocessor, FullImageDataset, sanitized
    root = os.path.join(str(tmp_path), "KPCN")
    raw, gt, conts = _write_scene(root, "test", "room", 192, 192, 2, 500, continuations=(2,), plant=True)
    report = preprocess_main(["--data_dir", root, "--mode", "test", "--spp", "2"])
    inp = os.path.join(root, "test", "input")
    llpm_dir = os.path.join(str(tmp_path), "LLPM", "test", "input")
    assert sorted(os.listdir(inp)) == ["room.npy", "room_1.npy", "room_kpcn_2.npy", "room_kpcn_4.npy"]
    assert sorted(os.listdir(llpm_dir)) == ["room_llpm.npy", "room_llpm_1.npy"]
    assert len(report) == 1 and len(report[0][1]) == 5                    # + the sanitised gt; no probability map in this mode
    pre = DenoisePreprocessor()
    both = _dev(sanitized(np.concatenate((raw, conts[0]), axis=2)))
    assert _same_bits(np.load(os.path.join(inp, "room_kpcn_4.npy")), pre._preprocess_kpcn(both))
    assert _same_bits(np.load(os.path.join(llpm_dir, "room_llpm_1.npy")), pre._preprocess_llpm(_dev(sanitized(conts[0]))))
    os.remove(os.path.join(inp, "room.npy"))
    os.remove(os.path.join(inp, "room_1.npy"))
    ds = FullImageDataset(os.path.join(inp, "room.npy"), 4, "kpcn", True, False, True, 3, device=DEV)
    assert (ds.h, ds.w) == (192, 192) and ds.llpm.shape == (192, 192, 4, 37) and len(ds) == 4
    save = str(tmp_path / "weights")
    os.makedirs(save)
    args = evaluate.build_parser().parse_args(["--save", save, "--model_name", "KPCN_dir_test", "--input_dir", inp,
                                               "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--train_branches"])
    torch.manual_seed(0)
    itfs, _ = train_kpcn.init_model({"dncnn_in_size": 39, "pnet_in_size": 36, "pnet_out_size": 3}, args, torch.device(DEV))
    torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, "KPCN_dir_test.pth"))
    del itfs
    res, res_in = evaluate.denoise(args, inp + os.sep, str(tmp_path / "out"), scenes=None, spps=[2, 4], device=DEV)
    assert res.shape == res_in.shape == (40, 1) and np.isfinite(res_in).all() and np.isfinite(res).all()


# ------------------------------------------------------------------------------------------------- 5. the loader
def _expected_batches(root, d, indices, seed, n_per_image, bs):
    from wcmc_amd.support.datasets import DenoisePreprocessor, PatchBatcher, sanitized
    pre, batcher = DenoisePreprocessor(), PatchBatcher(PATCH, bs)
    batcher.patches_per_image = n_per_image
    np.random.seed(seed)
    out = []
    for i in indices:
        p = d.paths(i)
        x = _dev(sanitized(np.load(p["in"])[:, :, :d.spp]))
        g = _dev(sanitized(np.load(p["gt"])))
        kp, ll = pre._preprocess_kpcn(x), pre._preprocess_llpm(x)
        origins = batcher.sample_origins(np.load(p["prob"]))
        out += [batcher.batch(kp, ll, g, origins[k:k + bs]) for k in range(0, len(origins), bs)]
    return out


def test_patch_loader_over_the_directory_reader_matches_patch_batcher(train_dir):
    from wcmc_amd.support.loader import PatchLoader
    root, _, d, _, _ = train_dir
    want = _expected_batches(root, d, [0, 1], 1234, 8, 4)
    loader = PatchLoader(d.reader, [0, 1], DEV, batch_size=4, patch_size=PATCH, use_llpm=True, patches_per_image=8,
                         staged_hook=d.staged_hook)
    assert len(loader) == 4 == len(want)
    np.random.seed(1234)
    got = [{k: v.clone() for k, v in b.items()} for b in loader]
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert set(a) == set(b)
        for k in a:
            assert a[k].shape[0] == 4 and _same_bits(a[k], b[k]), k


def test_a_missing_probability_map_is_computed_written_and_equal(train_dir):
    from wcmc_amd import ops
    from wcmc_amd.support.datasets import _PendingProb, sanitized
    from wcmc_amd.support.loader import PatchLoader
    root, scenes, d, _, _ = train_dir
    i = [os.path.basename(f) for f in d.gt_files].index("room.npy")
    fn = d.paths(i)["prob"]
    stored = np.load(fn)
    os.remove(fn)
    try:
        assert isinstance(d.reader(i)["prob"], _PendingProb)
        want = _expected_batches_with(stored, root, d, i)
        np.random.seed(77)
        got = [{k: v.clone() for k, v in b.items()}
               for b in PatchLoader(d.reader, [i], DEV, batch_size=4, patch_size=PATCH, use_llpm=True, patches_per_image=4,
                                    staged_hook=d.staged_hook)]
        assert os.path.isfile(fn) and np.array_equal(np.load(fn), stored)
        raw, gt, _ = scenes["room"]
        direct = ops.sampling_prob(_dev(sanitized(raw[:, :, :2])), _dev(sanitized(gt)), PATCH).cpu().numpy()
        assert np.array_equal(np.load(fn), direct)                # the same kernel as test 2 holds to the golden
        assert len(got) == len(want) == 1 and all(_same_bits(got[0][k], want[0][k]) for k in want[0])
    finally:
        if not os.path.isfile(fn):
            np.save(fn, stored)


def _expected_batches_with(prob, root, d, i):
    from wcmc_amd.support.datasets import DenoisePreprocessor, PatchBatcher, sanitized
    pre, batcher = DenoisePreprocessor(), PatchBatcher(PATCH, 4)
    batcher.patches_per_image = 4
    p = d.paths(i)
    x, g = _dev(sanitized(np.load(p["in"])[:, :, :d.spp])), _dev(sanitized(np.load(p["gt"])))
    np.random.seed(77)
    origins = batcher.sample_origins(prob)
    return [batcher.batch(pre._preprocess_kpcn(x), pre._preprocess_llpm(x), g, origins)]


# ------------------------------------------------------------------------------------------------- 6. the training CLI
DRIVER = r"""
import sys, torch
from wcmc_amd import train_kpcn as tk
inner = tk.train
def spy(interfaces, loaders, params, args):
    vec = lambda: torch.cat([p.detach().reshape(-1) for m in interfaces[0].models.values() for p in m.parameters()]).clone()
    before = vec()
    print('TRAIN_BATCHES %d VAL_BATCHES %d' % (len(loaders['train']), len(loaders['val'])))
    inner(interfaces, loaders, params, args)
    after = vec()
    print('PARAM_DELTA %.6e FINITE %d' % (float((after - before).abs().max()), int(torch.isfinite(after).all())))
tk.train = spy
tk.main(sys.argv[1:])
"""


def test_train_kpcn_from_data_dir_runs_an_epoch_in_a_child_process(tmp_path):
    """``python -m wcmc_amd.train_kpcn --from_data_dir`` end to end: two training scenes (one probability map written ahead, one
    computed by the loader), one validation scene on the grid, one epoch, both checkpoint files."""
    from wcmc_amd.support.datasets import DenoiseDirectory
    root, save = str(tmp_path / "data"), str(tmp_path / "weights")
    _write_scene(root, "train", "room", 192, 160, 2, 600)
    _write_scene(root, "train", "car", 192, 160, 2, 700)
    _write_scene(root, "val", "den", 192, 160, 2, 800)
    DenoiseDirectory(root, 2, "train", device=DEV, patch_size=PATCH).offline_preprocess(llpm=False, kpcn=False)
    os.remove(os.path.join(root, "train", "input", "car_prob_imp.npy"))
    argv = ["--from_data_dir", "--data_dir", root, "--num_samples", "2", "--single_gpu", "--batch_size", "2", "--patch_size",
            str(PATCH), "--patches_per_image", "4", "--val_epoch", "1", "--num_epoch", "1", "--model_name", "KPCN_dir",
            "--desc", "directory loop", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--w_manif", "0.1",
            "--train_branches", "--lr_dncnn", "1e-4", "--lr_pnet", "1e-4", "--save", save]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WCMC_DEBUG_LIB", None)
    r = subprocess.run([sys.executable, "-c", DRIVER] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    out = r.stdout
    assert r.returncode == 0, "train_kpcn --from_data_dir failed:\n%s\n%s" % (out[-3000:], r.stderr[-3000:])
    assert "TRAIN_BATCHES 4 VAL_BATCHES 2" in out                       # 2 images x 4 patches / 2; 6 whole grid windows / 4
    assert "[] Training complete!" in out and "Model KPCN_dir.pth saved at epoch 0." in out
    delta = float(out.split("PARAM_DELTA ")[1].split()[0])
    assert delta > 0.0 and "FINITE 1" in out
    assert os.path.isfile(os.path.join(root, "train", "input", "car_prob_imp.npy"))
    ck = torch.load(os.path.join(save, "KPCN_dir.pth"), weights_only=False)
    assert ck["start_epoch"] == 1 and np.isfinite(ck["best_err"]) and 0 < ck["best_err"] < 1e9
    assert os.path.isfile(os.path.join(save, "latest_KPCN_dir.pth"))
