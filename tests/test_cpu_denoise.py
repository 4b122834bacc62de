"""Denoising a render of any size, the parts that need no GPU: the tile table of ``support.inference.frame_tiles``, the argument
checks of the two entry points of csrc/frame_tiles.hip, the PFM / PNG writers and the argument errors of ``wcmc_amd.denoise``."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

SIDES = (64, 65, 70, 83, 127, 128, 129, 191, 192, 200)
PATCH, PAD = 128, 32


@pytest.mark.parametrize("h", SIDES)
def test_frame_tiles_partition_the_frame_from_tile_interiors(h):
    from wcmc_amd import ops
    from wcmc_amd.support.inference import frame_tiles
    for w in SIDES:
        table = frame_tiles(h, w, PATCH, PAD)
        count = np.zeros((h, w), dtype=np.int64)
        for i0, j0, i1, j1, i, j in table:
            count[i0:i1, j0:j1] += 1
            # the owned window lies inside the tile's [pad, patch - pad) interior
            assert i + PAD <= i0 < i1 <= i + PATCH - PAD and j + PAD <= j0 < j1 <= j + PATCH - PAD, (h, w, (i0, j0, i1, j1, i, j))
            assert -PAD <= i <= h + PAD - PATCH and -PAD <= j <= w + PAD - PATCH, (h, w, i, j)
        assert (count == 1).all(), (h, w)
        ops.check_tile_coords(table, h, w, PATCH)
        ops.check_tile_origins([t[4:6] for t in table], h, w, PATCH, PAD)


def test_frame_tiles_geometry_and_refusals():
    from wcmc_amd import ops
    from wcmc_amd.support.inference import frame_tiles
    assert frame_tiles(64, 64) == [(0, 0, 64, 64, -32, -32)]
    # 70 x 83: two tiles per direction, the second clamped to dim + pad - patch and owning what the first left
    assert frame_tiles(70, 83) == [(0, 0, 64, 64, -32, -32), (0, 64, 64, 83, -32, -13),
                                   (64, 0, 70, 64, -26, -32), (64, 64, 70, 83, -26, -13)]
    assert len(frame_tiles(1080, 1920)) == 17 * 30
    with pytest.raises(ValueError, match="smaller than the 64-pixel interior"):
        frame_tiles(63, 64)
    with pytest.raises(ValueError, match="smaller than the 64-pixel interior"):
        frame_tiles(64, 63)
    with pytest.raises(ValueError, match="no interior"):
        frame_tiles(128, 128, 64, 32)
    for bad in ([(-33, 0)], [(0, 70 + 32 - 128 + 1)], [(5, -40)]):
        with pytest.raises(ValueError, match="outside the 70x70 frame extended by 32"):
            ops.check_tile_origins(np.array(bad, dtype=np.int32), 70, 70, PATCH, PAD)


def test_new_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Negative status + a message, before any HIP call (the contract of include/wcmc_hip.h): this runs without a GPU."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)          # `one`: non-null, aligned, never dereferenced by the checks
    tiles = lambda **kw: L.wcmc_assemble_kpcn_tiles(*[{**dict(   # noqa: E731
        kpcn=one, llpm=null, origins=one, B=2, H=70, W=83, S=0, P=128, pad=32, t=0, din=one, sin=one, dbuf=one, sbuf=one, alb=one,
        paths=null, stream=null), **kw}[k] for k in ("kpcn", "llpm", "origins", "B", "H", "W", "S", "P", "pad", "t", "din", "sin",
                                                     "dbuf", "sbuf", "alb", "paths", "stream")])
    finish = lambda **kw: L.wcmc_finish_frame(*[{**dict(   # noqa: E731
        out_rad=one, kpcn=one, llpm=one, H=70, W=83, S=2, out=one, ipt=one, has_hit=one, pv_out=null, pv_ipt=null, stream=null),
        **kw}[k] for k in ("out_rad", "kpcn", "llpm", "H", "W", "S", "out", "ipt", "has_hit", "pv_out", "pv_ipt", "stream")])
    cases = [(tiles, dict(kpcn=null), "null pointer"), (tiles, dict(origins=null), "null pointer"),
             (tiles, dict(din=null), "null pointer"), (tiles, dict(alb=null), "null pointer"),
             (tiles, dict(llpm=one, S=2), "paths"),                       # llpm without a paths output
             (tiles, dict(llpm=one, paths=one, S=0), "S > 0"),
             (tiles, dict(H=32), "pad = 32 must be smaller"), (tiles, dict(W=20), "pad = 32 must be smaller"),
             (tiles, dict(P=64), "no interior"), (tiles, dict(P=63), "no interior"),
             (tiles, dict(H=40, W=40, P=128), "does not fit"), (tiles, dict(B=0), "positive"), (tiles, dict(pad=-1), "non-negative"),
             (tiles, dict(t=8), "0..7"),
             (finish, dict(out_rad=null), "null pointer"), (finish, dict(kpcn=null), "null pointer"),
             (finish, dict(llpm=null), "null pointer"), (finish, dict(has_hit=null), "null pointer"),
             (finish, dict(S=0), "must be positive"), (finish, dict(H=0), "must be positive")]
    for fn, kw, text in cases:
        rc = fn(**kw)
        msg = L.wcmc_last_error().decode()
        assert rc < 0, (kw, rc)
        assert text in msg and ("assemble_kpcn_tiles" if fn is tiles else "finish_frame") in msg, (kw, msg)


def _read_pfm(fn):
    """A PFM reader in ten lines: header 'PF' | 'Pf', width height, scale (negative: little-endian), rows bottom to top."""
    with open(fn, "rb") as f:
        kind = f.readline().strip()
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        c = {b"PF": 3, b"Pf": 1}[kind]
        data = np.frombuffer(f.read(), dtype="<f4" if scale < 0 else ">f4")
    assert data.size == h * w * c
    img = data.reshape(h, w, c)[::-1]
    return img if c == 3 else img[..., 0]


def test_pfm_round_trip(tmp_path):
    from wcmc_amd.denoise import write_pfm
    rng = np.random.default_rng(0)
    img = (rng.standard_normal((7, 11, 3)) * 100).astype(np.float32)
    img[0, 0] = (0.0, np.inf, 1e-38)
    fn = str(tmp_path / "a.pfm")
    write_pfm(fn, img)
    np.testing.assert_array_equal(_read_pfm(fn), img)
    assert os.path.getsize(fn) == len(b"PF\n11 7\n-1.0\n") + 7 * 11 * 3 * 4
    write_pfm(fn, img[..., 1])
    np.testing.assert_array_equal(_read_pfm(fn), img[..., 1])
    with pytest.raises(ValueError, match="write_pfm"):
        write_pfm(fn, img[..., :2])


def test_png_is_a_valid_eight_bit_rgb_file(tmp_path):
    from wcmc_amd.denoise import write_png
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (5, 9, 3), dtype=np.uint8)
    fn = str(tmp_path / "a.png")
    write_png(fn, img)
    raw = open(fn, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    chunks, pos = [], 8
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff, tag
        chunks.append((tag, data))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (9, 5, 8, 2, 0, 0, 0)          # width, height, 8 bit, RGB, no interlace
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(5, 1 + 9 * 3)
    assert (rows[:, 0] == 0).all()                                                  # filter type 0 on every row
    np.testing.assert_array_equal(rows[:, 1:].reshape(5, 9, 3), img)
    with pytest.raises(ValueError, match="write_png"):
        write_png(fn, img.astype(np.float32))


def _argv(tmp_path, inputs, extra=()):
    return ["--input"] + [str(i) for i in inputs] + ["--output_dir", str(tmp_path / "out"), "--save", str(tmp_path),
                                                      "--model_name", "KPCN_x", "--use_llpm_buf"] + list(extra)


def test_cli_argument_errors_precede_the_gpu(tmp_path):
    from wcmc_amd import denoise, train_kpcn
    check = lambda argv: denoise.check_inputs(train_kpcn.check_args(denoise.build_parser().parse_args(argv)))   # noqa: E731
    np.save(tmp_path / "scene.npy", np.zeros((64, 64, 2, 104), np.float32))
    np.save(tmp_path / "wide.npy", np.zeros((4, 4, 70, 104), np.float32))
    np.save(tmp_path / "flat.npy", np.zeros((64, 64, 104), np.float32))
    args = check(_argv(tmp_path, [tmp_path / "scene.npy"]))
    assert args.spp is None and args.tile_batch is None and not args.png and not args.save_pbuffer
    assert denoise.read_raw(str(tmp_path / "scene.npy"))[1] == 2
    assert [denoise.tile_batch_size(s) for s in (1, 32, 33, 64)] == [8, 8, 4, 4] and denoise.tile_batch_size(128, 2) == 2
    # more than 64 samples per pixel: the batch size is the user's to give, and the error names the flag
    with pytest.raises(ValueError, match="--tile_batch"):
        check(_argv(tmp_path, [tmp_path / "wide.npy"]))
    check(_argv(tmp_path, [tmp_path / "wide.npy"], ["--tile_batch", "1"]))
    check(_argv(tmp_path, [tmp_path / "wide.npy"], ["--spp", "64"]))
    # too few samples and no continuation file
    with pytest.raises(ValueError, match=r"hold 2 samples per pixel, fewer than the 3 asked for \(--spp\)"):
        check(_argv(tmp_path, [tmp_path / "scene.npy"], ["--spp", "3"]))
    np.save(tmp_path / "scene_1.npy", np.ones((64, 64, 4, 104), np.float32))
    parts, spp = denoise.read_raw(str(tmp_path / "scene.npy"), 3)
    assert spp == 3 and [p.shape for p in parts] == [(64, 64, 2, 104), (64, 64, 1, 104)] and float(parts[1].min()) == 1.0
    with pytest.raises(ValueError, match=r"hold 6 samples per pixel, fewer than the 7 asked"):
        denoise.read_raw(str(tmp_path / "scene.npy"), 7)
    # not renderer output; a file that is not there; a model the command cannot run
    with pytest.raises(ValueError, match=r"is not renderer output \(H, W, S, 104\)"):
        check(_argv(tmp_path, [tmp_path / "flat.npy"]))
    with pytest.raises(FileNotFoundError):
        check(_argv(tmp_path, [tmp_path / "nothing.npy"]))
    with pytest.raises(ValueError, match="--save_pbuffer"):
        denoise.check_inputs(denoise.build_parser().parse_args(
            ["--input", str(tmp_path / "scene.npy"), "--output_dir", "o", "--save_pbuffer"]))
    with pytest.raises(SystemExit):
        denoise.build_parser().parse_args(["--output_dir", "o"])                    # --input is required


def test_reference_interface_refuses_to_denoise_without_targets():
    import torch
    from wcmc_amd.support.interfaces import KPCNRefInterface
    lf = {k: torch.nn.L1Loss() for k in ("l_diffuse", "l_specular", "l_recon", "l_test")}
    itf = KPCNRefInterface({"dncnn": torch.nn.Identity()}, {}, lf, None)
    with pytest.raises(NotImplementedError, match="targets"):
        itf.denoise_batch({})
