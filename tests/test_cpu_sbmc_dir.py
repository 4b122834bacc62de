"""Host-side tests (no GPU) of the sample-based data path: channel counts, the 'lbmc' mapping and file names of
``support.datasets.DenoiseDirectory`` and the parsers of ``wcmc_amd.train_sbmc`` / ``wcmc_amd.train_lbmc`` against what the reference's
``DenoiseDataset`` and launchers recorded in ``tests/golden/sbmc_data.npz`` (``tests/golden/make_golden_sbmc.py``)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_sbmc as mgs  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "sbmc_data.npz"))


@pytest.fixture()
def tree(tmp_path):
    gt = tmp_path / "KPCN" / "train" / "gt"
    os.makedirs(gt)
    open(gt / "room.npy", "wb").close()
    return str(tmp_path / "KPCN")


@pytest.mark.parametrize("combo", list(mgs.COMBOS))
def test_channel_counts_and_flags_match_the_reference(gold, tree, combo):
    from wcmc_amd.support.datasets import DenoiseDirectory
    bm, g, p, l = mgs.COMBOS[combo]
    want = [int(v) for v in gold["sizes/%s" % combo]]                     # dncnn / pnet at pnet_out_size 3, then at 0
    d3 = DenoiseDirectory(tree, 4, "train", use_llpm_buf=l, pnet_out_size=3, base_model=bm, use_g_buf=g, use_sbmc_buf=p)
    d0 = DenoiseDirectory(tree, 4, "train", use_llpm_buf=l, pnet_out_size=0, base_model=bm, use_g_buf=g, use_sbmc_buf=p)
    assert [d3.dncnn_in_size, d3.pnet_in_size, d0.dncnn_in_size, d0.pnet_in_size] == want
    flags = [int(d3.base_model == "sbmc"), int(d3.use_g_buf), int(d3.use_sbmc_buf), int(d3.use_llpm_buf)]
    assert flags == [int(v) for v in gold["flags/%s" % combo]]


def test_lbmc_is_sbmc_with_the_g_buffer_and_kpcn_stays_the_default(tree):
    from wcmc_amd.support.datasets import DenoiseDirectory, sample_flags
    assert sample_flags("lbmc", False, True) == ("sbmc", True, False)
    assert sample_flags("sbmc", False, True) == ("sbmc", False, True)
    assert sample_flags("kpcn", True, True) == ("kpcn", True, False)       # only 'sbmc' reads the SBMC buffers
    with pytest.raises(RuntimeError, match="Unknown baseline model"):
        sample_flags("unet")
    d = DenoiseDirectory(tree, 8, "train")
    assert (d.base_model, d.dncnn_in_size, d.pnet_in_size) == ("kpcn", 34, 0)
    assert DenoiseDirectory(tree, 8, "train", use_llpm_buf=True).dncnn_in_size == 39
    with pytest.raises(RuntimeError, match="Unknown baseline model"):
        DenoiseDirectory(tree, 8, "train", base_model="unet")


def test_file_names_of_the_sbmc_buffers(gold, tree):
    from wcmc_amd.support.datasets import DenoiseDirectory
    p = DenoiseDirectory(tree, 4, "train", base_model="sbmc").paths(0)
    top = os.path.dirname(tree)
    j = lambda *a: os.path.join(top, *a)                                                             # noqa: E731
    assert p["in"] == j("KPCN", "train", "input", "room.npy") and p["prob"] == j("KPCN", "train", "input", "room_prob_imp.npy")
    assert p["sbmc_s"] == j("SBMC", "train", "input", "room_sbmc_s.npy") and p["sbmc_p"] == j("SBMC", "train", "input", "room_sbmc_p.npy")
    assert p["llpm"] == j("LLPM", "train", "input", "room_llpm.npy")
    assert p["sbmc_s_k"](2) == j("SBMC", "train", "input", "room_sbmc_s_2.npy") and p["sbmc_p_k"](7) == j("SBMC", "train", "input", "room_sbmc_p_7.npy")
    # the golden run's names (a directory without /KPCN/ in its path: everything beside the input)
    assert {"scene" + os.path.basename(p[k])[len("room"):] for k in ("in", "llpm", "prob", "sbmc_p", "sbmc_s")} == set(str(f) for f in gold["item/files"])


@pytest.mark.parametrize("launcher", ["train_sbmc", "train_lbmc"])
def test_launcher_parser_defaults_equal_the_reference(gold, launcher):
    import importlib
    mod = importlib.import_module("wcmc_amd." + launcher)
    want = json.loads(str(gold["parser/" + launcher]))
    have = {a.dest: a for a in mod.build_parser()._actions}
    assert ("use_sbmc_buf" in want) == (launcher == "train_sbmc")
    for dest, (default, action, options, required) in want.items():
        a = have[dest]
        assert a.default == default and type(a).__name__ == action and list(a.option_strings) == options and a.required == required, dest
    extra = set(have) - set(want) - {"help"}
    assert extra == {"denoiser", "from_data_dir", "patch_size", "patches_per_image"}
    args = mod.build_parser().parse_args(["--desc", "x"])
    assert args.denoiser is None and args.use_g_buf is True


def test_denoiser_factory_errors_quote_the_flag():
    from wcmc_amd.train_sbmc import DenoiserFactoryError, load_denoiser_factory
    for spec in (None, "", "json", "no_such_package_xyz:make", "json:no_such_name", "json:__doc__"):
        with pytest.raises(DenoiserFactoryError, match="--denoiser"):
            load_denoiser_factory(spec)
    assert load_denoiser_factory("json:dumps") is json.dumps


def test_new_names_are_exported_from_ops():
    from wcmc_amd import ops
    from wcmc_amd._lib import SIGNATURES
    from wcmc_amd.ops import data
    for name in ("preprocess_sbmc", "assemble_sample_patches", "check_patch_origins", "sample_feature_size"):
        assert getattr(ops, name) is getattr(data, name)
    assert "wcmc_preprocess_sbmc" in SIGNATURES and "wcmc_assemble_sample_patches" in SIGNATURES
    assert [ops.sample_feature_size(g, p, l) for g in (1, 0) for p in (1, 0) for l in (0, 1)] == [90, 91, 24, 25, 69, 70, 3, 4]
    with pytest.raises(ValueError, match="outside"):
        ops.check_patch_origins(np.array([[0, 0], [25, 0]]), 40, 48, 16)
    ops.check_patch_origins(np.array([[24, 32]]), 40, 48, 16)


def test_full_image_dataset_for_sample_based_models_is_a_class_of_its_own():
    from wcmc_amd.support.datasets import FullImageDataset, SampleFullImageDataset
    assert issubclass(SampleFullImageDataset, FullImageDataset) and SampleFullImageDataset.SAMPLE_BASED and not FullImageDataset.SAMPLE_BASED
    with pytest.raises(FileNotFoundError):
        SampleFullImageDataset(os.sep.join(["", "nonexistent", "input", "s.npy"]), 8, "lbmc", device="cpu")
