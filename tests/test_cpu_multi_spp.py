"""Sample counts 2..spp, the parts that need no GPU: the order of a multi-count epoch (``support.loader.multi_count_schedule``)
against the reference's ``MSDenoiseDataset`` index arithmetic and against a recording of the real class
(``tests/golden/ms_schedule.npz``, written by ``tests/golden/make_golden_ms_schedule.py``), and the launchers' flags."""
import os

import numpy as np
import pytest


def _batches(schedule, ppi, batch):
    """The (image, count) of every batch of an epoch that walks ``schedule`` with ``ppi`` patches per visit."""
    return [pair for pair in schedule for _ in range(ppi // batch)]


def test_full_window_is_the_index_arithmetic_of_ms_denoise_dataset():
    from wcmc_amd.support.loader import multi_count_schedule
    N, counts, ppi = 3, (2, 3, 4), 8
    # datasets.py:1157-1171: ConcatDataset of one DenoiseDataset per count 2..spp, each of N * ppi items (:282-283) whose item idx
    # is image idx // ppi (:1036); the DataLoader does not shuffle (train_kpcn.py:177-188)
    want = [((i % (N * ppi)) // ppi, 2 + i // (N * ppi)) for i in range(N * ppi * len(counts))]
    got = [pair for pair in multi_count_schedule(N, counts, 3) for _ in range(ppi)]
    assert got == want
    assert multi_count_schedule(N, counts, 7) == multi_count_schedule(N, counts, 3)          # window >= N: the same order


def test_full_window_equals_the_recorded_reference_class(golden_dir):
    from wcmc_amd.support.datasets import multi_counts
    from wcmc_amd.support.loader import multi_count_schedule
    d = np.load(os.path.join(golden_dir, "ms_schedule.npz"))
    n, spp, ppi = int(d["n_images"]), int(d["spp"]), int(d["patches_per_image"])
    assert len(d["counts"]) == n * ppi * (spp - 1)
    got = [pair for pair in multi_count_schedule(n, multi_counts(spp), n) for _ in range(ppi)]
    assert [p[0] for p in got] == d["images"].tolist() and [p[1] for p in got] == d["counts"].tolist()
    # a batch never mixes counts: ppi is a multiple of the batch size (datasets.py:275)
    assert ppi % 8 == 0 and all(len(set(d["counts"][k:k + 8].tolist())) == 1 for k in range(0, len(d["counts"]), 8))
    with pytest.raises(RuntimeError) as exc:
        multi_counts(1)
    assert str(exc.value) in str(d["too_low_message"])


@pytest.mark.parametrize("window", [1, 2])
def test_every_pair_once_and_counts_ascend_inside_a_window(window):
    from wcmc_amd.support.loader import multi_count_schedule
    N, counts = 3, (2, 3, 4)
    sched = multi_count_schedule(N, counts, window)
    assert sorted(sched) == sorted((i, s) for i in range(N) for s in counts) and len(set(sched)) == len(sched)
    for w0 in range(0, N, window):
        imgs = list(range(w0, min(w0 + window, N)))
        part = [p for p in sched if p[0] in imgs]
        assert part == [(i, s) for s in counts for i in imgs]                         # counts ascend; images in order per count
        k = sched.index(part[0])
        assert sched[k:k + len(part)] == part                                         # a window is contiguous in the epoch
    if window == 1:
        assert sched == [(i, s) for i in range(N) for s in counts]                    # image-major
    assert _batches(sched, 8, 4)[:3] == [sched[0], sched[0], sched[1]]


def test_schedule_and_counts_reject_nonsense():
    from wcmc_amd.support.datasets import check_counts, multi_counts
    from wcmc_amd.support.loader import multi_count_schedule
    assert multi_counts(2) == (2,) and multi_counts(8) == (2, 3, 4, 5, 6, 7, 8)
    assert multi_count_schedule(0, (2, 3), 1) == []
    assert multi_count_schedule(2, (3, 2), 1) == [(0, 2), (0, 3), (1, 2), (1, 3)]      # ascending whatever the order given
    with pytest.raises(ValueError):
        multi_count_schedule(2, (2, 3), 0)
    for bad in ((), (3, 2), (2, 2), (0, 1), (2, 9)):
        with pytest.raises(ValueError):
            check_counts(bad, 8)
    assert check_counts([2, 4, 8], 8) == (2, 4, 8)


def test_the_three_launchers_take_the_flags_and_default_to_off():
    from wcmc_amd import train_kpcn, train_lbmc, train_sbmc
    for mod in (train_kpcn, train_sbmc, train_lbmc):
        parse = lambda argv: train_kpcn.parse_args(argv, mod.build_parser())                # noqa: E731  (what each main() calls)
        off = parse(["--desc", "x"])
        assert off.multi_spp is False and off.ms_window == train_kpcn.MS_WINDOW >= 1
        on = parse(["--multi_spp", "--desc", "x", "--from_data_dir", "--ms_window", "3", "--num_samples", "5"])
        assert on.multi_spp is True and on.ms_window == 3 and on.from_data_dir is True and on.num_samples == 5
        text = mod.build_parser().format_help()
        assert "--multi_spp" in text and "--ms_window" in text and "additions of this build" in text
        with pytest.raises(SystemExit):
            parse(["--desc", "x", "--ms_window", "three"])
    # the two flags are read by a parser of their own: a launcher's build_parser() keeps the flag surface that earlier tests pin
    assert not hasattr(train_kpcn.build_parser().parse_args(["--desc", "x"]), "multi_spp")


def test_argument_errors_of_multi_spp():
    from wcmc_amd import train_kpcn as tk
    parse = lambda *a: tk.parse_args(["--desc", "x"] + list(a))                        # noqa: E731
    with pytest.raises(RuntimeError) as exc:
        tk.check_args(parse("--multi_spp"))
    assert "--multi_spp" in str(exc.value) and "--from_data_dir" in str(exc.value)
    with pytest.raises(RuntimeError, match="spp too low to randomize sample count"):
        tk.check_args(parse("--multi_spp", "--from_data_dir", "--num_samples", "1"))
    with pytest.raises(RuntimeError, match="ms_window"):
        tk.check_args(parse("--multi_spp", "--from_data_dir", "--ms_window", "0"))
    tk.check_args(parse("--multi_spp", "--from_data_dir", "--num_samples", "2"))
    tk.check_args(parse("--num_samples", "1"))                                          # without the flag nothing changes


def test_abi_declares_the_prefix_entry_points_and_rejects_bad_counts():
    """Argument checks precede any HIP call (include/wcmc_hip.h), so this runs without a GPU."""
    import ctypes
    from wcmc_amd import _lib
    L = _lib.lib()
    assert L.wcmc_abi_version() == 4
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert L.wcmc_preprocess_kpcn_prefix_workspace_bytes(10, 7, 3) == 3 * (2 * 70 + 4) * 4
    assert L.wcmc_preprocess_kpcn_prefix_workspace_bytes(10, 7, 0) == 0
    for s_lo, s_hi, S in ((0, 2, 8), (3, 2, 8), (2, 9, 8), (2, 65, 65)):
        assert L.wcmc_preprocess_kpcn_prefix(one, 4, 4, S, 104, 5, s_lo, s_hi, one, one, 1 << 30, null) == -1, (s_lo, s_hi, S)
        assert "s_lo" in L.wcmc_last_error().decode()
    assert L.wcmc_preprocess_kpcn_prefix(one, 4, 4, 8, 104, 5, 2, 8, one, one, 16, null) < 0            # workspace too small
    assert "workspace" in L.wcmc_last_error().decode()
