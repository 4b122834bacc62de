"""CPU-side checks of the dataset-directory layer (no GPU): discovery order, file-name and path rules and grid origins of
``support.datasets.DenoiseDirectory`` against goldens of the reference (``tests/golden/dataset_dir.npz``, written by
``tests/golden/make_golden_dataset.py``), the 'reflect' index map of the sampling-map kernels against numpy, and the flag
surface of the training CLI."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the defaults of `train_kpcn.build_parser()` at the commit before --from_data_dir existed
PARENT_DEFAULTS = {
    'sbmc': False, 'p_buf': False, 'model_name': 'tSUNet', 'data_dir': './data', 'visual': False, 'batch_size': 64,
    'num_epoch': 100, 'val_epoch': 1, 'vis_iter': 4, 'start_epoch': 0, 'num_samples': 8, 'save': './weights', 'overfit': False,
    'desc': 'x', 'lr_dncnn': 0.0001, 'lr_pnet': [0.0001], 'lr_ckpt': False, 'best_err': None, 'pnet_out_size': [3],
    'manif_loss': None, 'train_branches': False, 'use_llpm_buf': False, 'manif_learn': False, 'w_manif': [0.1],
    'disentangle': 'm11r11', 'single_gpu': False, 'device_id': 0, 'kpcn_ref': False, 'kpcn_pre': False, 'not_save': False,
    'local': False, 'synthetic': 16, 'patch_size': 128, 'graph': False, 'defer_check': True, 'one_graph': False,
    'overlap_allreduce': False, 'pairing_rng': 'cpu', 'pathnet_weight_norm': True, 'pairing': 'local'}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "dataset_dir.npz"))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def _touch_dir(root, mode, names, shape=None):
    d = os.path.join(root, mode, "gt")
    os.makedirs(d)
    for n in names:
        if shape is None:
            open(os.path.join(d, n), "wb").close()
        else:
            np.save(os.path.join(d, n), np.zeros(shape, dtype=np.float32))
    return d


def test_discovery_order_is_the_reference_seeded_shuffle(gold, tmp_path):
    import random
    from wcmc_amd.support.datasets import DenoiseDirectory, shuffled_files
    names, want = [str(n) for n in gold["names"]], [str(n) for n in gold["shuffled"]]
    state = random.getstate()
    assert shuffled_files(names) == want
    assert random.getstate() == state, "the process-wide random state must not be reseeded"
    # the directory: listed in any order (plus files that are not scenes), discovered sorted, shuffled as the reference does
    _touch_dir(str(tmp_path), "train", list(reversed(names)) + ["notes.txt"])
    d = DenoiseDirectory(str(tmp_path), 8, "train")
    assert [os.path.basename(f) for f in d.gt_files] == want and len(d) == len(want)
    assert all(os.path.dirname(f) == os.path.join(str(tmp_path), "train", "gt") for f in d.gt_files)


def test_patches_per_image_and_input_sizes_follow_the_reference(gold, tmp_path):
    from wcmc_amd.support.datasets import DenoiseDirectory
    _touch_dir(str(tmp_path), "train", ["a.npy"])
    got = [DenoiseDirectory(str(tmp_path), 8, "train", batch_size=b, sampling=s).patches_per_image
           for b, s in ((8, "random"), (6, "random"), (4, "grid"))]
    assert got == [int(v) for v in gold["patches_per_image"]]
    d = DenoiseDirectory(str(tmp_path), 8, "train")
    assert (d.dncnn_in_size, d.pnet_in_size) == (34, 0)                       # datasets.py:201-219
    d = DenoiseDirectory(str(tmp_path), 8, "train", use_llpm_buf=True)
    assert (d.dncnn_in_size, d.pnet_in_size, d.pnet_out_size) == (34 + 3 + 2, 36, 3)
    with pytest.raises(RuntimeError, match="Unknown training mode"):
        DenoiseDirectory(str(tmp_path), 8, "eval")
    with pytest.raises(RuntimeError, match="Unknown sampling mode"):
        DenoiseDirectory(str(tmp_path), 8, "train", sampling="stratified")
    with pytest.raises(FileNotFoundError):
        DenoiseDirectory(str(tmp_path), 8, "val")


def test_file_name_and_path_rules(tmp_path):
    from wcmc_amd.support.datasets import DenoiseDirectory
    root = os.path.join(str(tmp_path), "KPCN")
    _touch_dir(root, "test", ["bath.room.npy"])
    p = DenoiseDirectory(root, 8, "test").paths(0)
    inp = os.path.join(root, "test", "input")
    assert p["gt"] == os.path.join(root, "test", "gt", "bath.room.npy")
    assert p["in"] == os.path.join(inp, "bath.room.npy")
    assert p["kpcn"](4) == os.path.join(inp, "bath.room_kpcn_4.npy")
    assert p["prob"] == os.path.join(inp, "bath.room_prob_imp.npy")
    assert p["in_k"](3) == os.path.join(inp, "bath.room_3.npy")
    llpm_dir = os.path.join(str(tmp_path), "LLPM", "test", "input")             # /KPCN/ -> /LLPM/, as FullImageDataset reads
    assert p["llpm"] == os.path.join(llpm_dir, "bath.room_llpm.npy")
    assert p["llpm_k"](2) == os.path.join(llpm_dir, "bath.room_llpm_2.npy")
    # a missing file raises; there is no fallback across mounts
    with pytest.raises(FileNotFoundError):
        DenoiseDirectory(root, 8, "test").reader(0)


def test_reader_names_a_short_raw_file_and_a_map_of_another_patch_size(tmp_path):
    """Fewer samples on disk than ``spp`` and a ``_prob_imp.npy`` written for another patch size are errors that say so, not a
    run at another sample count or a broadcast failure inside the loader."""
    from wcmc_amd.support.datasets import DenoiseDirectory, _PendingProb
    root = str(tmp_path)
    _touch_dir(root, "train", ["s.npy"], shape=(40, 36, 9))
    os.makedirs(os.path.join(root, "train", "input"))
    np.save(os.path.join(root, "train", "input", "s.npy"), np.zeros((40, 36, 3, 104), dtype=np.float32))
    item = DenoiseDirectory(root, 2, "train", patch_size=16).reader(0)
    assert item["raw"].shape == (40, 36, 2, 104) and item["gt"].shape == (40, 36, 9) and isinstance(item["prob"], _PendingProb)
    with pytest.raises(ValueError, match="holds 3 samples per pixel, fewer than the 4"):
        DenoiseDirectory(root, 4, "train", patch_size=16).reader(0)
    np.save(os.path.join(root, "train", "input", "s_prob_imp.npy"), np.full((24, 20), 1.0 / 480, dtype=np.float32))
    assert DenoiseDirectory(root, 2, "train", patch_size=16).reader(0)["prob"].shape == (24, 20)
    with pytest.raises(ValueError, match="written for another patch size"):
        DenoiseDirectory(root, 2, "train", patch_size=8).reader(0)


def test_grid_origins_are_those_of_full_patches(gold, tmp_path):
    from wcmc_amd.support.datasets import DenoiseDirectory, grid_origins
    n = len([k for k in gold.files if k.startswith("grid/") and k.endswith("/size")])
    assert n == 3
    for i in range(n):
        h, w = (int(v) for v in gold["grid/%d/size" % i])
        np.testing.assert_array_equal(grid_origins(h, w), gold["grid/%d/origins" % i])
    h, w = (int(v) for v in gold["grid/1/size"])
    _touch_dir(str(tmp_path), "val", ["s.npy"], shape=(h, w, 9))
    d = DenoiseDirectory(str(tmp_path), 8, "val", sampling="grid")
    np.testing.assert_array_equal(d.origins(0), gold["grid/1/origins"])
    with pytest.raises(RuntimeError, match="grid"):
        DenoiseDirectory(str(tmp_path), 8, "val").origins(0)


def test_reflect_index_map_is_numpy_symmetric_padding(built):
    """The index map of the Gaussian passes (``wcmc_reflect_index``: the function the kernel calls) for every line length from 1 to
    300 at the radius of sigma 31: shorter than, equal to and longer than the radius."""
    from wcmc_amd import ops
    r = 124
    for n in range(1, 301):
        want = np.pad(np.arange(n), r, mode="symmetric")
        got = np.array([ops.reflect_index(i, n) for i in range(-r, n + r)])
        assert np.array_equal(got, want), n


def test_host_sanitize_rule():
    from wcmc_amd.support.datasets import sanitized
    x = np.array([0.5, np.nan, np.inf, -np.inf, 2e38, -3.0, 1e38], dtype=np.float64)
    want = np.array([0.5, 1e38, 1e38, 1e38, 1e38, -3.0, 1e38], dtype=np.float32)
    got = sanitized(x)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_sampling_map_ops_have_no_cpu_path(built):
    from wcmc_amd import ops
    for fn, args in ((ops.importance_map, (torch.zeros(8, 8),)), (ops.sanitize_, (torch.zeros(4),)),
                     (ops.sampling_prob, (torch.zeros(40, 40, 2, 104), torch.zeros(40, 40, 9), 16))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(*args)
    h = __import__("wcmc_amd._lib", fromlist=["lib"]).lib()
    assert h.wcmc_importance_map_workspace_bytes(96, 80, 3) > 7 * 96 * 80 * 4
    assert h.wcmc_importance_map_workspace_bytes(96, 80, 2) == 0
    assert h.wcmc_sampling_prob_workspace_bytes(128, 200, 128) == 0          # H <= patch is rejected
    assert h.wcmc_sampling_prob_workspace_bytes(129, 200, 128) > 0
    assert h.wcmc_importance_map(None, 8, 8, 1, None, None, 0, None) < 0 and b"null" in h.wcmc_last_error()


def test_training_cli_defaults_are_unchanged_without_the_flag():
    from wcmc_amd import train_kpcn as tk
    got = vars(tk.build_parser().parse_args(["--desc", "x"]))
    assert got.pop("from_data_dir") is False and got.pop("patches_per_image") is None
    assert got == PARENT_DEFAULTS
    from wcmc_amd import preprocess
    a = preprocess.build_parser().parse_args(["--data_dir", "D", "--mode", "val", "--spp", "4"])
    assert (a.data_dir, a.mode, a.spp, a.overwrite, a.no_llpm, a.device_id) == ("D", "val", 4, False, False, 0)
