"""Streaming a frame to the device in row bands, the parts that need no GPU: the band partition, the argument checks of the three
row-range entry points of csrc/preprocess.hip, the host band reader of ``support.staging`` on pageable slots, and the argument error
of ``--band_rows``."""
import ctypes
import threading
import time

import numpy as np
import pytest

H, W = 70, 83


@pytest.mark.parametrize("h", (1, 64, 70))
def test_band_ranges_partition_the_rows(h):
    from wcmc_amd.support.staging import band_ranges, default_band_rows
    for band_rows in (1, 16, 64, 70, 1000):
        ranges = band_ranges(h, band_rows)
        assert ranges[0][0] == 0 and sum(r for _, r in ranges) == h
        for (a, ra), (b, _) in zip(ranges, ranges[1:]):
            assert a + ra == b and ra == band_rows                   # consecutive, and full but for the last one
        assert 1 <= ranges[-1][1] <= band_rows and len(ranges) == -(-h // band_rows)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="band_rows should be at least 1"):
            band_ranges(h, bad)
    # the default band: target_bytes of float32 samples, between one row and the frame
    assert default_band_rows(720, 1280, 8, 16 << 20) == (16 << 20) // (1280 * 8 * 416) == 3
    assert default_band_rows(70, 83, 2, 16 << 20) == 70 and default_band_rows(1080, 1920, 64, 16 << 20) == 1


def test_row_range_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Negative status + a message, before any HIP call (the contract of include/wcmc_hip.h): this runs without a GPU."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)             # `one`: non-null, aligned, never dereferenced by the checks
    need = L.wcmc_preprocess_kpcn_workspace_bytes(H, W)
    assert need == (2 * H * W + 4) * 4

    def call(name, order, base, kw):
        a = {**base, **kw}
        return getattr(L, name)(*[a[k] for k in order])
    begin = lambda **kw: call("wcmc_preprocess_kpcn_begin", ("ws", "nbytes", "h", "w", "stream"),   # noqa: E731
                              dict(ws=one, nbytes=need, h=H, w=W, stream=null), kw)
    rows = lambda **kw: call("wcmc_preprocess_kpcn_rows",   # noqa: E731
                             ("band", "h", "w", "row0", "rows", "s", "C", "md", "out", "ws", "nbytes", "stream"),
                             dict(band=one, h=H, w=W, row0=3, rows=4, s=2, C=104, md=5, out=one, ws=one, nbytes=need, stream=null), kw)
    end = lambda **kw: call("wcmc_preprocess_kpcn_end", ("out", "ws", "nbytes", "h", "w", "s", "stream"),   # noqa: E731
                            dict(out=one, ws=one, nbytes=need, h=H, w=W, s=2, stream=null), kw)
    bad_arg, bad_ws = _lib.lib().wcmc_preprocess_llpm(null, 1, 104, 5, null, null), None
    assert bad_arg < 0                                               # WCMC_ERR_BAD_ARG, as an existing entry point returns it
    bad_ws = L.wcmc_preprocess_kpcn(one, H, W, 2, 104, 5, one, one, need - 1, null)
    assert bad_ws < 0 and bad_ws != bad_arg                          # WCMC_ERR_WORKSPACE
    cases = [(begin, dict(ws=null), bad_arg, "null pointer"), (begin, dict(nbytes=need - 1), bad_ws, "workspace too small"),
             (begin, dict(h=0), bad_arg, "must be positive"),
             (rows, dict(band=null), bad_arg, "null pointer"), (rows, dict(out=null), bad_arg, "null pointer"),
             (rows, dict(ws=null), bad_arg, "null pointer"),
             (rows, dict(row0=-1), bad_arg, "are not rows of the 70-row frame"),
             (rows, dict(rows=0), bad_arg, "are not rows of the 70-row frame"),
             (rows, dict(rows=-2), bad_arg, "are not rows of the 70-row frame"),
             (rows, dict(row0=67, rows=4), bad_arg, "are not rows of the 70-row frame"),
             (rows, dict(row0=70, rows=1), bad_arg, "are not rows of the 70-row frame"),
             (rows, dict(row0=2 ** 31 - 1, rows=2), bad_arg, "are not rows of the 70-row frame"),    # (row0 + rows must not wrap)
             (rows, dict(nbytes=need - 1), bad_ws, "workspace too small"), (rows, dict(nbytes=0), bad_ws, "workspace too small"),
             (rows, dict(s=0), bad_arg, "bad argument"), (rows, dict(C=103), bad_arg, "bad argument"),
             (end, dict(out=null), bad_arg, "null pointer"), (end, dict(ws=null), bad_arg, "null pointer"),
             (end, dict(nbytes=need - 1), bad_ws, "workspace too small"), (end, dict(s=0), bad_arg, "must be positive")]
    for fn, kw, code, text in cases:
        rc = fn(**kw)
        msg = L.wcmc_last_error().decode()
        assert rc == code, (kw, rc, msg)
        name = {begin: "preprocess_kpcn_begin", rows: "preprocess_kpcn_rows", end: "preprocess_kpcn_end"}[fn]
        assert text in msg and name in msg, (kw, msg)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """scene.npy (2 samples) + scene_1.npy (1 sample) of a 70 x 83 frame, and a float64 copy of the first."""
    d = tmp_path_factory.mktemp("renders")
    rng = np.random.default_rng(0)
    a = rng.standard_normal((H, W, 2, 104)).astype(np.float32)
    b = rng.standard_normal((H, W, 1, 104)).astype(np.float32)
    a[3, 5, 1, 7], a[69, 82, 0, 0], b[0, 0, 0, 103] = np.nan, np.inf, -np.inf          # copied as they are: sanitising is the device's
    np.save(d / "scene.npy", a)
    np.save(d / "scene_1.npy", b)
    np.save(d / "wide.npy", a.astype(np.float64) * (1 + 2.0 ** -30))                   # (not representable in float32)
    return d


def _bands(reader):
    """[(row0, rows, copy of the band)] in the order the reader hands them out; every slot goes straight back."""
    out = []
    for slot, row0, rows in reader:
        out.append((row0, rows, reader.ring.view(slot, (rows, reader.w, reader.spp, 104)).numpy().copy()))
        reader.ring.release(slot)
    return out


@pytest.mark.parametrize("spp", (3, 1))
def test_band_reader_hands_out_every_band_exactly_and_in_row_order(scene, spp):
    from wcmc_amd import denoise
    from wcmc_amd.support.staging import BandReader, band_ranges
    parts, got_spp = denoise.read_raw(str(scene / "scene.npy"), spp)
    assert got_spp == spp and [p.shape[2] for p in parts] == ([2, 1] if spp == 3 else [1])
    if spp == 1:
        assert not parts[0].flags["C_CONTIGUOUS"]                    # a strided prefix of the file's two samples
    whole = np.concatenate([np.asarray(p) for p in parts], 2)
    before = threading.active_count()
    for band_rows in (1, 16, 64, 70, 1000):
        reader = BandReader(parts, band_rows, workers=3, pin=False)
        assert len(reader.ring.slots) == 3 + 2
        bands = _bands(reader)
        assert [(r0, r) for r0, r, _ in bands] == band_ranges(H, band_rows)
        for r0, r, band in bands:
            assert band.dtype == np.float32 and band.shape == (r, W, spp, 104)
            np.testing.assert_array_equal(band.view(np.int32), whole[r0:r0 + r].view(np.int32))      # bit for bit, NaN included
        # nothing of the frame's size on the host: every slot is one band
        assert reader.ring.nbytes() <= 5 * min(band_rows, H) * W * spp * 416
    assert threading.active_count() == before


def test_band_reader_converts_float64_as_numpy_does(scene):
    from wcmc_amd import denoise
    from wcmc_amd.support.staging import BandReader
    parts, spp = denoise.read_raw(str(scene / "wide.npy"))
    assert parts[0].dtype == np.float64 and spp == 2
    want = np.array(parts[0], dtype=np.float32, order="C")
    assert not np.array_equal(want.astype(np.float64), np.asarray(parts[0]), equal_nan=True)       # the conversion rounds
    bands = _bands(BandReader(parts, 16, workers=3, pin=False))
    got = np.concatenate([b for _, _, b in bands], 0)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


class _FailingPart:
    """A part whose rows from ``fail_row0`` on cannot be read."""

    def __init__(self, part, fail_row0):
        self.part, self.shape, self.fail_row0 = part, part.shape, fail_row0

    def __getitem__(self, key):
        if key.start == self.fail_row0:
            raise OSError("cannot read rows from %d" % key.start)
        return self.part[key]


def _wait_for_threads(count, seconds=5.0):
    t0 = time.monotonic()
    while threading.active_count() > count and time.monotonic() - t0 < seconds:
        time.sleep(0.01)
    return threading.active_count()


def test_band_reader_surfaces_errors_and_stops_its_threads(scene):
    from wcmc_amd import denoise
    from wcmc_amd.support.staging import BandReader
    parts, _ = denoise.read_raw(str(scene / "scene.npy"), 3)
    before = threading.active_count()
    # the third band (rows 32..47) raises: the first two arrive, then the consumer sees the reader's error
    reader = BandReader([_FailingPart(parts[0], 32), parts[1]], 16, workers=3, pin=False)
    seen = []
    with pytest.raises(OSError, match="cannot read rows from 32"):
        for slot, row0, rows in reader:
            seen.append(row0)
            reader.ring.release(slot)
    assert seen == [0, 16]
    assert _wait_for_threads(before) == before
    assert reader.ring.free_q.qsize() == 5                           # every slot is back in the ring
    # an early break: the workers, some of them waiting for a slot the consumer never returns, stop too
    reader = BandReader(parts, 1, workers=3, pin=False)
    for n, (slot, row0, rows) in enumerate(reader):
        if n == 4:
            break
    assert row0 == 4
    assert _wait_for_threads(before) == before


def test_band_rows_below_one_is_an_argument_error_before_the_gpu(scene, tmp_path):
    from wcmc_amd import denoise, train_kpcn
    from wcmc_amd.support.staging import FrameStreamer
    argv = lambda extra: ["--input", str(scene / "scene.npy"), "--output_dir", str(tmp_path / "out"), "--save", str(tmp_path),   # noqa: E731
                          "--model_name", "KPCN_x", "--use_llpm_buf"] + extra
    check = lambda extra: denoise.check_inputs(train_kpcn.check_args(denoise.build_parser().parse_args(argv(extra))))   # noqa: E731
    assert check([]).band_rows is None and check(["--band_rows", "1"]).band_rows == 1
    for bad in ("0", "-3"):
        with pytest.raises(ValueError, match="--band_rows should be at least 1"):
            check(["--band_rows", bad])
        with pytest.raises(ValueError, match="--band_rows should be at least 1"):
            denoise.main(argv(["--band_rows", bad]))                 # refused before the model or the device is looked for
    with pytest.raises(ValueError, match="band_rows should be at least 1"):
        FrameStreamer([str(scene / "scene.npy")], None, "cuda:0", band_rows=0)
