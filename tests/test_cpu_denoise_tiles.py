"""Tiles of any size, a wider overlap and feathered seams for wcmc_amd.denoise, without a GPU: the two entry
points in the header, the binding and the built library, and their argument checks (which precede any HIP call); the weights of
tests/blend_ref.py; the tiles per call and the collected kernel limits; the command line's three flags."""
import ctypes
import os
import re

import numpy as np
import pytest

import blend_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wcmc_stitch_tiles_blend": 18, "wcmc_blend_finish": 7}
WEIGHT_CASES = [(16, 5, 0), (16, 5, 3), (16, 6, 4), (128, 32, 4), (192, 40, 12), (256, 64, 36)]


def test_new_symbols_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from wcmc_amd import ops
    from wcmc_amd._lib import SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "wcmc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(wcmc_[a-z0-9_]+)\s*\(", header))
    h = lib()
    for name, nargs in NEW.items():
        assert name in declared and name in SIGNATURES, name
        assert getattr(h, name) is not None
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert len(m.group(1).split(",")) == len(SIGNATURES[name][1]) == nargs, name
    assert ops.stitch_tiles_blend is ops.data.stitch_tiles_blend and ops.blend_finish is ops.data.blend_finish


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Every refusal of the two entry points: the library's error code and a message that names the op; nothing is launched."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)     # `one`: non-null, never dereferenced by the checks
    good = dict(rad=one, ho=92, wo=92, P=128, pad=40, coords=one, B=2, t=5, H=70, W=83, F=12, acc=one, wsum=one)

    def stitch(**kw):
        a = dict(good, **kw)
        return L.wcmc_stitch_tiles_blend(a["rad"], 3 * 92 * 92, 92 * 92, 92, 1, a["ho"], a["wo"], a["P"], a["pad"], a["coords"], a["B"],
                                         a["t"], a["H"], a["W"], a["F"], a["acc"], a["wsum"], null)
    cases = {"t = 8": (dict(t=8), "0..7"), "t = -1": (dict(t=-1), "0..7"), "null rad": (dict(rad=null), "null pointer"),
             "null coords": (dict(coords=null), "null pointer"), "null acc": (dict(acc=null), "null pointer"),
             "null wsum": (dict(wsum=null), "null pointer"), "B = 0": (dict(B=0), "must be positive"),
             "H = 0": (dict(H=0), "must be positive"), "P = 0": (dict(P=0, ho=0), "must be positive"),
             "larger output": (dict(ho=130), "P x P or smaller"), "mixed output": (dict(ho=128), "P x P or smaller"),
             "wo = 0": (dict(wo=0), "P x P or smaller"), "F = -1": (dict(F=-1), "must not be negative"),
             "F beyond the tile": (dict(F=129, pad=-1), "wider than the 128-pixel tile"),
             "pad without an interior": (dict(pad=64), "no interior"),
             "2F above the interior": (dict(F=25, pad=40), "longer than the 48-pixel interior"),
             "2F above the interior, P = 192": (dict(P=192, ho=156, wo=156, pad=80, F=17), "longer than the 32-pixel interior"),
             "F reaches replicated pixels": (dict(F=12, pad=29), "replicated pixels"),
             "F reaches replicated pixels of a narrow output": (dict(wo=60, pad=40, F=7), "34 replicated pixels"),
             "too many tiles": (dict(B=65536), "at most 65535")}
    seen = set()
    for what, (kw, word) in cases.items():
        assert stitch(**kw) == -1, what                                          # WCMC_ERR_BAD_ARG
        msg = L.wcmc_last_error().decode()
        assert msg.startswith("stitch_tiles_blend:") and word in msg, (what, msg)
        seen.add(word.split(" ")[0])
    assert len(seen) >= 9                                                        # each kind of refusal has its own message

    fgood = dict(acc=one, wsum=one, H=70, W=83, accumulate=1, out=one)

    def finish(**kw):
        a = dict(fgood, **kw)
        return L.wcmc_blend_finish(a["acc"], a["wsum"], a["H"], a["W"], a["accumulate"], a["out"], null)
    for what, (kw, word) in {"null acc": (dict(acc=null), "null pointer"), "null wsum": (dict(wsum=null), "null pointer"),
                             "null out": (dict(out=null), "null pointer"), "H = 0": (dict(H=0), "must be positive"),
                             "W = -1": (dict(W=-1), "must be positive"), "accumulate = 2": (dict(accumulate=2), "must be 0 or 1"),
                             "accumulate = -1": (dict(accumulate=-1), "must be 0 or 1")}.items():
        assert finish(**kw) == -1, what
        msg = L.wcmc_last_error().decode()
        assert msg.startswith("blend_finish:") and word in msg, (what, msg)


def _axis(n, patch, pad):
    """The owned intervals and origins [(a, b, o)] of an axis of length n, from the project's table."""
    from wcmc_amd.support.inference import frame_tiles
    table = frame_tiles(n, patch - 2 * pad, patch, pad)           # (one column of tiles: the rows are the axis)
    return [(i0, i1, i) for i0, _, i1, _, i, _ in table]


@pytest.mark.parametrize("patch,pad,f", WEIGHT_CASES)
def test_weights_of_the_reference(patch, pad, f):
    interior = patch - 2 * pad
    for n in (interior, interior + 1, 3 * interior + 7):
        spans = _axis(n, patch, pad)
        assert spans[0][0] == 0 and spans[-1][1] == n and all(p[1] == q[0] for p, q in zip(spans, spans[1:]))
        if n == interior + 1:
            assert spans[-1][1] - spans[-1][0] == 1               # a last tile that owns one pixel
        x = np.arange(n)
        total, involved = np.zeros(n), np.zeros(n, bool)
        for a, b, o in spans:
            lo, hi = blend_ref.axis_range(a, b, n, f)
            # the contribution range stays inside the window that the tile's output fills from its own data: F <= pad - inset
            inset = pad - f
            assert o + inset <= lo < hi <= o + patch - inset and lo <= a and b <= hi
            u = blend_ref.axis_weight(x, a, b, n, f)
            assert (u[lo:hi] > 0).all() and (u[:lo] == 0).all() and (u[hi:] == 0).all() and u.max() <= 1
            assert (u[a:b] > 0.5).all() if f else (u[a:b] == 1).all()            # the owner's weight: sum w >= 1/4 in 2-D
            total += u
            if b - a < 2 * f:
                involved[lo:hi] = True
            if f == 0:
                assert np.array_equal(u, ((x >= a) & (x < b)).astype(float))     # the indicator of the owned window
        assert (total > 0).all()
        assert np.abs(total[~involved] - 1).max(initial=0) <= 1e-12
    # 2-D: the product of the row and the column weight, on the tiles of a two-axis table
    from wcmc_amd.support.inference import frame_tiles
    ht, wt = interior + 1, 3 * interior + 7
    den = np.zeros((ht, wt))
    for row in frame_tiles(ht, wt, patch, pad):
        ys, xs, w = blend_ref.tile_weight(row, ht, wt, f)
        assert np.array_equal(w, blend_ref.axis_weight(ys, row[0], row[2], ht, f)[:, None]
                              * blend_ref.axis_weight(xs, row[1], row[3], wt, f)[None, :])
        den[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] += w
    assert den.min() >= 0.25


def test_tiles_per_call_and_the_collected_limits():
    from wcmc_amd import denoise
    assert [denoise.tile_batch_size(s) for s in (1, 32, 33, 64)] == [8, 8, 4, 4]                  # today's, unchanged at P = 128
    assert [denoise.tile_batch_size(s, None, 128) for s in (1, 32, 33, 64)] == [8, 8, 4, 4]
    for tile in (192, 256, 384, 512):
        for spp, b128 in ((8, 8), (32, 8), (33, 4), (64, 4)):
            b = denoise.tile_batch_size(spp, None, tile)
            assert b == max(1, b128 * 128 * 128 // (tile * tile))
            assert b == 1 or b * tile * tile <= b128 * 128 * 128                                # the pixel budget per call is kept
    assert [denoise.tile_batch_size(8, None, t) for t in (192, 256, 384, 512)] == [3, 2, 1, 1]
    assert denoise.tile_batch_size(128, 2, 256) == 2                                              # the caller's count is taken as it is
    with pytest.raises(ValueError, match="--tile_batch"):
        denoise.tile_batch_size(8, 0, 256)
    with pytest.raises(ValueError, match="no default tile batch size above 64"):
        denoise.tile_batch_size(65, None, 256)
    # every default passes the limits, but for three corners where ONE tile holds 2 GiB or more of 64-channel per-sample activations
    # (S * P^2 * 256 bytes: 2.25 GiB at 64 spp and 384 pixels, 2 GiB at 32 spp and 512), past final2's view; without per-sample
    # tensors those pass too
    for tile in (128, 192, 256, 384, 512):
        for spp in (1, 8, 32, 64):
            if (spp, tile) in ((64, 384), (64, 512), (32, 512)):
                with pytest.raises(ValueError, match="--tile %d with --tile_batch 1 at %d samples.*0x7ff00000" % (tile, spp)):
                    denoise.check_tile_limits(tile, 32, spp, denoise.tile_batch_size(spp, None, tile))
                assert denoise.check_tile_limits(tile, 32, spp, 1, per_sample=False) == 1
            else:
                assert denoise.check_tile_limits(tile, 32, spp, denoise.tile_batch_size(spp, None, tile)) >= 1
    # ... and one combination past each collected limit is refused, with the flags and the limit in the message
    past = {"65535 rows": (512, 32, 8, 16),             # B * S * P = 65536
            "0x7ff00000": (512, 32, 8, 4),              # B * S * P^2 * 256 = 2^31
            "below 2 GiB": (512, 32, 1, 5)}             # B * P^2 * 448 * 4 > 2 GiB, the rest within bounds
    assert len(past) == len(denoise.TILE_LIMITS)
    for word, (tile, pad, spp, b) in past.items():
        with pytest.raises(ValueError, match="--tile %d with --tile_batch %d" % (tile, b)) as e:
            denoise.check_tile_limits(tile, pad, spp, b)
        assert word in str(e.value) and "--tile_batch" in str(e.value), (word, str(e.value))
    first = [k for k, (_, q, bound) in enumerate(denoise.TILE_LIMITS) if q(512, 32, 1, 5) > bound]
    assert first == [2]                                 # that case is refused by the operand bound alone
    for _, q, bound in denoise.TILE_LIMITS:
        assert q(512, 32, 1, 1) <= bound


def _argv(*extra, model="KPCN_x", inp="nothing.npy"):
    return ["--save", "unused", "--model_name", model, "--input", inp, "--output_dir", "unused"] + list(extra)


def _check(*extra, **kw):
    from wcmc_amd import denoise
    return denoise.check_inputs(denoise.build_parser().parse_args(_argv(*extra, **kw)))


def test_the_command_line_flags(tmp_path):
    from wcmc_amd import denoise
    d = denoise.build_parser().parse_args(_argv())
    assert (d.tile, d.tile_pad, d.blend) == (128, 32, 0)
    assert denoise.check_tile_flags(d) == (128, 32, 0)
    a = denoise.build_parser().parse_args(_argv("--tile", "192", "--tile_pad", "40", "--blend", "12"))
    assert denoise.check_tile_flags(a) == (192, 40, 12)
    missing = str(tmp_path / "nothing.npy")
    # refused before a file is looked for: the input does not exist, and the flag's error comes first
    for extra, word in ((["--tile", "160"], "--tile 160"), (["--tile", "64"], "--tile 64"), (["--tile", "576"], "--tile 576"),
                        (["--blend", "5", "--tile_pad", "32"], "--blend 5"), (["--tile_pad", "100", "--tile", "192"], "--tile_pad 100"),
                        (["--tile_pad", "16"], "--tile_pad 16"), (["--blend", "-1"], "--blend"),
                        (["--tile", "192", "--tile_pad", "64", "--blend", "36"], "--blend 36"),     # two ramps of 72 in an interior of 64
                        (["--tile", "192", "--tile_pad", "48", "--blend", "21"], "--blend 21")):
        with pytest.raises(ValueError, match=word):
            _check(*extra, inp=missing)
    # accepted: the next thing looked for is the file
    for extra in (["--tile", "192"], ["--tile", "512", "--tile_pad", "224", "--blend", "32"], ["--tile_pad", "60", "--tile", "192",
                  "--blend", "32"], ["--tile", "256", "--tile_pad", "64", "--blend", "36"], ["--tile_pad", "32", "--blend", "4"]):
        with pytest.raises(FileNotFoundError):
            _check(*extra, inp=missing)
    # a sample-based model: the pad is the caller's, the blend is held to the interior here and to the denoiser's inset on the first batch
    sample = ["--denoiser", "standins:SampleDenoiserStandIn"]
    with pytest.raises(FileNotFoundError):
        _check("--tile", "192", "--tile_pad", "16", "--blend", "16", *sample, model="SBMC_x", inp=missing)
    with pytest.raises(ValueError, match="--blend 37"):
        _check("--tile", "192", "--tile_pad", "60", "--blend", "37", *sample, model="SBMC_x", inp=missing)
    with pytest.raises(ValueError, match="--tile 160"):
        _check("--tile", "160", *sample, model="SBMC_x", inp=missing)
    # a tile larger than the extended frame: known from the file's header, before the GPU is touched
    small = tmp_path / "small.npy"
    np.save(small, np.zeros((100, 200, 1, 104), np.float32))
    with pytest.raises(ValueError, match="192-pixel tile .* does not fit the 100 x 200 frame"):
        _check("--tile", "192", inp=str(small))
    from wcmc_amd.support.inference import check_tile_fits
    check_tile_fits("x", 130, 300, 192, 32, (0, 1))                # both sides hold a tile: the transposed frame does too
    check_tile_fits("x", 100, 300, 192, 46)                        # 100 + 2 * 46 = 192
    with pytest.raises(ValueError, match=r"does not fit the 100 x 300 frame \(nor its transpose"):
        check_tile_fits("x", 100, 300, 192, 45, (0, 1))
    with pytest.raises(ValueError, match="does not fit the 300 x 100 frame extended by the pad of 45"):
        check_tile_fits("x", 300, 100, 192, 45)
    text = denoise.build_parser().format_help()
    assert "--tile P" in text and "--blend F" in text and "--tile_pad N" in text
