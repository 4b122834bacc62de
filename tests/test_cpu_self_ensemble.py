"""The dihedral self-ensemble of wcmc_amd.denoise without a GPU: the three entry points in the header, the
binding and the built library; their argument checks (which precede any HIP call); the host check of a code set; the whole-frame
source map and its composition with the mirror against numpy; the tile tables of the transformed frames; the command line's flag."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wcmc_stitch_tiles_aug": 16, "wcmc_assemble_kpcn_tiles": 17, "wcmc_assemble_sample_tiles": 17}
PATCH, PAD = 128, 32
SIZES = [(64, 64), (70, 83), (128, 150)]


def T(a, t):
    """The transform of code t on the two leading axes."""
    return np.rot90(np.fliplr(a) if t & 4 else a, k=t & 3)


def source(t, y, x, h, w):
    """The specification's whole-frame source map: pixel (y, x) of T_t of an h x w frame <- source pixel (sy, sx)."""
    sy, sx = [(y, x), (x, w - 1 - y), (h - 1 - y, w - 1 - x), (h - 1 - x, y)][t & 3]
    return (sy, w - 1 - sx) if t & 4 else (sy, sx)


def mirror(i, n):
    return -1 - i if i < 0 else 2 * n - 1 - i if i >= n else i


def test_new_symbols_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from wcmc_amd._lib import SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "wcmc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(wcmc_[a-z0-9_]+)\s*\(", header))
    h = lib()
    for name, nargs in NEW.items():                              # (the two tile assemblers: the code t behind pad)
        assert name in declared and name in SIGNATURES, name
        assert getattr(h, name) is not None
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert len(m.group(1).split(",")) == len(SIGNATURES[name][1]) == nargs, name


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Every refusal of the C ABI: the library's error code and a message of its own that names the op; nothing is launched (the
    checks precede every HIP call, so this runs without a GPU)."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)     # `one`: non-null, never dereferenced by the checks
    good = dict(a=one, llpm=one, org=one, B=2, H=70, W=150, S=2, P=128, pad=32, t=3, out=one, paths=one, sbmc_p=one, use_p=1)

    def kpcn(**kw):
        a = dict(good, **kw)
        return L.wcmc_assemble_kpcn_tiles(a["a"], a["llpm"], a["org"], a["B"], a["H"], a["W"], a["S"], a["P"], a["pad"], a["t"],
                                          a["out"], one, one, one, one, a["paths"], null)

    def sample(**kw):
        a = dict(good, **kw)
        return L.wcmc_assemble_sample_tiles(a["a"], a["sbmc_p"], a["llpm"], a["org"], a["B"], a["H"], a["W"], a["S"], a["P"],
                                            a["pad"], a["t"], 1, a["use_p"], a["out"], one, a["paths"], null)
    shared = {"t = 8": (dict(t=8), "0..7"), "t = -1": (dict(t=-1), "0..7"), "null buffer": (dict(a=null), "null pointer"),
              "null origins": (dict(org=null), "null pointer"), "null output": (dict(out=null), "null pointer"),
              "llpm without paths": (dict(paths=null), "paths output"), "B = 0": (dict(B=0), "must be positive"),
              "H = 0": (dict(H=0), "must be positive"), "P = 0": (dict(P=0), "must be positive"),
              "negative pad": (dict(pad=-1), "pad non-negative"), "pad >= a side": (dict(H=32), "one reflection"),
              "no interior": (dict(P=64), "no interior"), "tile too large": (dict(H=60, W=60), "does not fit")}
    for fn, op, extra in ((kpcn, "assemble_kpcn_tiles", {"llpm with S = 0": (dict(S=0), "S > 0")}),
                          (sample, "assemble_sample_tiles", {"use_sbmc_buf without sbmc_p": (dict(sbmc_p=null), "needs sbmc_p"),
                                                             "S = 0": (dict(S=0), "S must be positive")})):
        seen = set()
        assert set(dict(shared, **extra)) > set(shared)
        for what, (kw, word) in dict(shared, **extra).items():
            assert fn(**kw) == -1, (op, what)                                    # WCMC_ERR_BAD_ARG
            msg = L.wcmc_last_error().decode()
            assert msg.startswith(op + ":") and word in msg, (op, what, msg)
            seen.add(word)
        assert len(seen) >= 8                                                    # each kind of refusal has its own message
    # the pad / P conditions are taken against the TRANSFORMED sizes: the message names them turned for an odd code
    assert kpcn(H=60, W=200, t=1) == -1 and "transformed 200 x 60 frame" in L.wcmc_last_error().decode()
    assert kpcn(H=60, W=200, t=2) == -1 and "transformed 60 x 200 frame" in L.wcmc_last_error().decode()
    # ... and t = 0 is the frame as it is: the untransformed sizes
    for fn in (kpcn, sample):
        assert fn(H=60, W=200, t=0) == -1 and "does not fit the transformed 60 x 200 frame" in L.wcmc_last_error().decode()

    sgood = dict(rad=one, ho=92, wo=92, P=128, coords=one, B=2, t=5, H=70, W=83, acc=1, out=one)

    def stitch(**kw):
        a = dict(sgood, **kw)
        return L.wcmc_stitch_tiles_aug(a["rad"], 3 * 92 * 92, 92 * 92, 92, 1, a["ho"], a["wo"], a["P"], a["coords"], a["B"], a["t"],
                                       a["H"], a["W"], a["acc"], a["out"], null)
    cases = {"t = 8": (dict(t=8), "0..7"), "t = -3": (dict(t=-3), "0..7"), "null rad": (dict(rad=null), "null pointer"),
             "null coords": (dict(coords=null), "null pointer"), "null out_rad": (dict(out=null), "null pointer"),
             "B = 0": (dict(B=0), "must be positive"), "W = 0": (dict(W=0), "must be positive"), "P = 0": (dict(P=0), "must be positive"),
             "larger output": (dict(ho=130), "P x P or smaller"), "mixed output": (dict(ho=128), "P x P or smaller"),
             "ho = 0": (dict(ho=0), "P x P or smaller"), "accumulate = 2": (dict(acc=2), "accumulate must be 0 or 1"),
             "accumulate = -1": (dict(acc=-1), "accumulate must be 0 or 1"), "too many tiles": (dict(B=65536), "at most 65535")}
    seen = set()
    for what, (kw, word) in cases.items():
        assert stitch(**kw) == -1, what
        msg = L.wcmc_last_error().decode()
        assert msg.startswith("stitch_tiles_aug:") and word in msg, (what, msg)
        seen.add(word)
    assert len(seen) == 6


def test_check_frame_transforms_on_good_and_bad_sets():
    from wcmc_amd import ops
    assert ops.check_frame_transforms is ops.data.check_frame_transforms and ops.stitch_tiles_aug is ops.data.stitch_tiles_aug
    assert ops.check_frame_transforms((0,)) == (0,)
    assert ops.check_frame_transforms([5, 0]) == (0, 5)
    assert ops.check_frame_transforms((6, 4, 2, 0)) == (0, 2, 4, 6)
    assert ops.check_frame_transforms(range(8)) == tuple(range(8))
    assert ops.check_frame_transforms(np.array([3, 0], np.int32)) == (0, 3)
    assert all(type(c) is int for c in ops.check_frame_transforms(np.array([3, 0], np.int32)))
    for bad, word in (((), "does not contain 0"), ((1, 2), "does not contain 0"), ((0, 2, 2), "repeated"), ((0, 0), "repeated"),
                      ((0, 8), "outside 0..7"), ((0, -1), "outside 0..7"), ((0, 1.0), "outside 0..7"), ((0, "1"), "outside 0..7"),
                      ((0, True), "outside 0..7"), (3, "sequence of codes"), (None, "sequence of codes")):
        with pytest.raises(ValueError, match=word) as e:
            ops.check_frame_transforms(bad)
        assert str(e.value).startswith("check_frame_transforms:")


def test_frame_transform_shape():
    from wcmc_amd.support.inference import frame_transform_shape
    for t in range(8):
        assert frame_transform_shape(70, 83, t) == T(np.zeros((70, 83)), t).shape
    for bad in (8, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="outside 0..7"):
            frame_transform_shape(70, 83, bad)


def test_the_whole_frame_source_map_against_numpy():
    """On a non-square index image, for all eight codes; and composed with the mirror (mirror first, in the transformed frame) it is
    the symmetric padding of the transformed frame -- which equals the transform of the padded frame."""
    from wcmc_amd.support.inference import frame_transform_shape
    h, w, p = 5, 7, 3
    a = np.arange(h * w).reshape(h, w)
    seen = set()
    for t in range(8):
        b = T(a, t)
        ht, wt = frame_transform_shape(h, w, t)                  # the sizes the drivers tile and check origins against
        assert b.shape == (ht, wt) == ((w, h) if t & 1 else (h, w))
        for y, x in itertools.product(range(ht), range(wt)):
            assert b[y, x] == a[source(t, y, x, h, w)], (t, y, x)
        seen.add(b.tobytes())
        ext = np.pad(b, p, "symmetric")
        assert np.array_equal(ext, T(np.pad(a, p, "symmetric"), t))
        for y, x in itertools.product(range(-p, b.shape[0] + p), range(-p, b.shape[1] + p)):
            assert ext[y + p, x + p] == a[source(t, mirror(y, b.shape[0]), mirror(x, b.shape[1]), h, w)], (t, y, x)
    assert len(seen) == 8


@pytest.mark.parametrize("h,w", SIZES)
def test_the_tile_tables_of_the_transformed_frames_partition_them(h, w):
    from wcmc_amd import ops
    from wcmc_amd.support.inference import frame_tiles, frame_transform_shape
    for t in range(8):
        ht, wt = frame_transform_shape(h, w, t)
        table = frame_tiles(ht, wt, PATCH, PAD)
        ops.check_tile_coords(table, ht, wt, PATCH)
        ops.check_tile_origins([c[4:6] for c in table], ht, wt, PATCH, PAD)
        owner = np.zeros((ht, wt), np.int64)
        back = np.zeros((h, w), np.int64)                       # ... and through the map, the SOURCE frame, once each
        for i0, j0, i1, j1, i, j in table:
            assert i + PAD <= i0 < i1 <= i + PATCH - PAD and j + PAD <= j0 < j1 <= j + PATCH - PAD
            owner[i0:i1, j0:j1] += 1
            for y, x in itertools.product((i0, i1 - 1), (j0, j1 - 1)):
                assert 0 <= source(t, y, x, h, w)[0] < h and 0 <= source(t, y, x, h, w)[1] < w
        assert (owner == 1).all()
        ys, xs = np.meshgrid(np.arange(ht), np.arange(wt), indexing="ij")
        sy, sx = source(t, ys, xs, h, w)
        np.add.at(back, (sy, sx), 1)
        assert (back == 1).all()
    if h != w:                                                   # a non-square frame has another table under the odd codes
        assert frame_tiles(w, h, PATCH, PAD) != frame_tiles(h, w, PATCH, PAD)


def _parse(*extra):
    from wcmc_amd import denoise
    return denoise.build_parser().parse_args(["--save", "unused", "--model_name", "KPCN_x", "--input", "unused.npy", "--output_dir",
                                              "unused"] + list(extra))


def test_the_self_ensemble_flag_bare_listed_and_refused():
    from wcmc_amd import denoise
    assert _parse().self_ensemble is None and denoise.ensemble_codes(_parse()) == (0,)
    assert denoise.ensemble_codes(_parse("--self_ensemble")) == tuple(range(8))
    assert denoise.ensemble_codes(_parse("--self_ensemble", "--png")) == tuple(range(8))
    assert denoise.ensemble_codes(_parse("--self_ensemble", "0", "2", "4", "6")) == (0, 2, 4, 6)
    assert denoise.ensemble_codes(_parse("--self_ensemble", "5", "0")) == (0, 5)
    assert denoise.ensemble_codes(_parse("--self_ensemble", "0")) == (0,)
    assert _parse("--self_ensemble", "0", "3", "--input", "a.npy", "b.npy").input == ["a.npy", "b.npy"]
    for bad, word in ((("2", "4"), "does not contain 0"), (("0", "2", "2"), "repeated"), (("0", "8"), "outside 0..7"),
                      (("0", "-1"), "outside 0..7")):
        with pytest.raises(ValueError, match=word) as e:
            denoise.ensemble_codes(_parse("--self_ensemble", *bad))
        assert str(e.value).startswith("--self_ensemble")
        with pytest.raises(ValueError, match="--self_ensemble"):           # refused before any file is looked for
            denoise.check_inputs(_parse("--self_ensemble", *bad))
    with pytest.raises(SystemExit):
        _parse("--self_ensemble", "two")
    text = denoise.build_parser().format_help()
    assert "--self_ensemble" in text and "0 2 4 6" in text
    # a sample-based model takes the flag too
    args = denoise.build_parser().parse_args(["--save", "u", "--model_name", "SBMC_x", "--input", "u.npy", "--output_dir", "u",
                                              "--self_ensemble", "0", "1", "4"])
    assert denoise.ensemble_codes(args) == (0, 1, 4)
