"""The per-image preprocessing kernels (csrc/preprocess.hip, csrc/data_step.h, the statistics pass of csrc/multi_spp.hip) against the
fp64 yardstick of tests/data_ref.py, at every entry of their dispatch tables, at the edges of the depth maximum, past every grid
cap, and on the depth mean that overflows fp32.

Every comparison covers every element of the output (``data_ref.assert_within``: |got - want| <= the derived bound, NaN exactly
where the reference is NaN).  The channels a function must not read hold NaN, so a wrong offset or a vector load at the wrong
place shows as a NaN.  The last test prints the largest |err| / bound per kernel and channel group of the whole run and writes it
to the report directory (profiles/data_edges_error_over_bound.txt is one such run).

Which kernel a call reaches is restated here from the dispatch conditions of the entry points; the table's rows show that every
kernel and every <VEC> instance has been reached."""
import functools
import os

import numpy as np
import pytest
import torch

import data_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("WCMC_TEST_REPORTS", os.path.join(ROOT, "test_reports"))     # (git-ignored)
DEV = "cuda:0"
REACHED = set()


def _ops():
    from wcmc_amd import ops
    return ops


def _pow2(s):
    return s & (s - 1) == 0


def vec_ok(md, C, aligned):
    alb = 24 + 7 * (md + 1)
    return C % 4 == 0 and aligned and alb % 2 == 0 and (alb + 2) % 4 == 0


def kpcn_kernel(s, md, C, aligned=True):
    if s <= 64 and _pow2(s):
        return "kpcn lanes<%s>" % ("true" if vec_ok(md, C, aligned) else "false")
    return "kpcn per-pixel"


def prefix_kernel(md, C, aligned=True):
    return "prefix<%s>" % ("true" if vec_ok(md, C, aligned) else "false")


def llpm_kernel(md, C, aligned=True):
    return "llpm tiled" if C % 4 == 0 and (24 + 6 * (md + 1)) % 4 == 0 and aligned else "llpm generic"


@functools.lru_cache(maxsize=None)
def small(h, w, s, md=5, C=None, seed=0, fill="kpcn", depth="default"):
    """(raw on the host, fp64 reference, bound): computed once, shared, never written to."""
    raw = R.make_frame(h, w, s, md, C, seed, fill=fill, depth=depth)
    want, bound = R.kpcn(raw.numpy(), md) if fill == "kpcn" else R.llpm(raw.numpy(), md)
    return raw, want, bound


def hold(got, want, bound, what, kernel):
    REACHED.add(kernel)
    R.assert_within(got, want, bound, what, kernel)


def check_max(got, want):
    """Depth channel 30 reaches exactly 1.0 at the reference's deepest pixel, and nowhere is it larger."""
    g, q = got[..., 30].reshape(-1), int(want[..., 30].argmax())
    assert want[..., 30].reshape(-1)[q] == 1.0
    assert float(g[q]) == 1.0 and int(g.argmax()) == q and float(g.max()) == 1.0, (q, float(g[q]), int(g.argmax()))


# ---------------------------------------------------------------------------------------------------- dispatch at small frames
@pytest.mark.parametrize("s", R.LANES_S + R.PIXEL_S)
def test_kpcn_every_sample_count_aligned_and_unaligned(s):
    """Lanes kernel at 64, 32, ..., 1 pixels per wave, the per-pixel kernel for odd counts, 12, and the powers of two above 64; the
    one-float offset takes lanes<false>.  (5,7) and (1,1) leave the last wave partial for every s."""
    ops = _ops()
    for h, w in R.SMALL_SHAPES:
        raw, want, bound = small(h, w, s, seed=100 + s)
        x = raw.to(DEV)
        got = ops.preprocess_kpcn(x)
        hold(got, want, bound, "kpcn %dx%dx%d" % (h, w, s), kpcn_kernel(s, 5, 104))
        y = R.offset_view(x, 1)
        got1 = ops.preprocess_kpcn(y)
        hold(got1, want, bound, "kpcn %dx%dx%d +1 float" % (h, w, s), kpcn_kernel(s, 5, 104, aligned=False))
        # <true> / <false> differ in their loads only
        R.assert_bit_equal(got1, got, "kpcn %dx%dx%d: scalar loads against vector loads" % (h, w, s))


@pytest.mark.parametrize("md,C", R.MAPS)
def test_every_channel_map(md, C):
    """pp_kpcn_vec_ok holds for (1,60), (5,104), (5,108); the tiled LLPM condition for (1,60), (3,84), (5,104), (5,108)."""
    ops = _ops()
    for h, w in R.SMALL_SHAPES:
        for s in (4, 3):
            raw, want, bound = small(h, w, s, md, C, seed=10 * md + s)
            got = ops.preprocess_kpcn(raw.to(DEV), md)
            hold(got, want, bound, "kpcn %dx%dx%d md %d C %d" % (h, w, s, md, C), kpcn_kernel(s, md, C))
        raw, _, _ = small(h, w, 4, md, C, seed=10 * md + 4)
        out = ops.preprocess_kpcn_prefix(raw.to(DEV), 2, 4, md)
        for n in (2, 3, 4):
            want, bound = prefix_ref(h, w, 4, md, C, 10 * md + 4, "default", n)
            hold(out[n - 2], want, bound, "prefix of %d, %dx%d md %d C %d" % (n, h, w, md, C), prefix_kernel(md, C))
        raw, want, bound = small(h, w, 2, md, C, seed=7, fill="llpm")
        got = ops.preprocess_llpm(raw.to(DEV), md)
        assert got.shape == (h, w, 2, 7 + 5 * (md + 1))
        hold(got, want, bound, "llpm %dx%d md %d C %d" % (h, w, md, C), llpm_kernel(md, C))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_views_off_16_byte_alignment_are_bit_equal_to_the_aligned_call(off):
    ops = _ops()
    for h, w in ((5, 7), (21, 19)):
        for s in (8, 3):
            raw, want, bound = small(h, w, s, seed=100 + s)
            x = raw.to(DEV)
            got = ops.preprocess_kpcn(R.offset_view(x, off))
            hold(got, want, bound, "kpcn %dx%dx%d +%d" % (h, w, s, off), kpcn_kernel(s, 5, 104, aligned=False))
            R.assert_bit_equal(got, ops.preprocess_kpcn(x), "kpcn %dx%dx%d +%d floats" % (h, w, s, off))
        x = small(h, w, 8, seed=108)[0].to(DEV)
        got = ops.preprocess_kpcn_prefix(R.offset_view(x, off), 1, 8)
        R.assert_bit_equal(got, ops.preprocess_kpcn_prefix(x, 1, 8), "prefix %dx%d +%d floats" % (h, w, off))
        for n in range(1, 9):
            want, bound = prefix_ref(h, w, 8, 5, None, 108, "default", n)
            hold(got[n - 1], want, bound, "prefix of %d, %dx%d +%d" % (n, h, w, off), prefix_kernel(5, 104, aligned=False))
        raw, want, bound = small(h, w, 2, seed=7, fill="llpm")
        x = raw.to(DEV)
        got = ops.preprocess_llpm(R.offset_view(x, off))
        hold(got, want, bound, "llpm %dx%d +%d" % (h, w, off), llpm_kernel(5, 104, aligned=False))
        # tiled and generic share pp_llpm_value
        R.assert_bit_equal(got, ops.preprocess_llpm(x), "llpm %dx%d +%d floats" % (h, w, off))


# ---------------------------------------------------------------------------------------------------- the prefix pass
@functools.lru_cache(maxsize=None)
def prefix_ref(h, w, S, md, C, seed, depth, n):
    raw = small(h, w, S, md, C, seed, "kpcn", depth)[0] if depth != "own" else R.own_maximum_frame(h, w, S)
    return R.kpcn(raw.numpy()[:, :, :n], md)


@pytest.mark.parametrize("S", [3, 5, 8, 64])
@pytest.mark.parametrize("counts", ["1..S", "2..S", "single"])
def test_prefix_pass_every_slab_against_its_own_prefix_and_its_own_maximum(S, counts):
    ops = _ops()
    lo, hi = {"1..S": (1, S), "2..S": (2, S), "single": (S // 2 + 1, S // 2 + 1)}[counts]
    for h, w in ((5, 7), (21, 19)):
        x = R.own_maximum_frame(h, w, S).to(DEV)
        out = ops.preprocess_kpcn_prefix(x, lo, hi)
        assert out.shape == (hi - lo + 1, h, w, 44)
        for n in range(lo, hi + 1):
            want, bound = prefix_ref(h, w, S, 5, None, 0, "own", n)
            hold(out[n - lo], want, bound, "prefix of %d of %d, %dx%d" % (n, S, h, w), prefix_kernel(5, 104))
            check_max(out[n - lo].cpu().numpy(), want)
            assert (int(want[..., 30].argmax()) == (h * w) // 3) == (n > 1)


# ---------------------------------------------------------------------------------------------------- the maximum
@pytest.mark.parametrize("kind", ["zero", "negative", "one_positive", "first", "last"])
def test_depth_maximum_edges(kind):
    """35 pixels: at s = 4 the third wave of the lanes kernel holds pixels 32..34, the per-pixel kernel's only wave 35 lanes; "last"
    puts the deepest pixel at the last pixel of that partial wave."""
    ops = _ops()
    h, w = 5, 7
    for s in (4, 3):
        raw, want, bound = small(h, w, s, seed=20 + s, depth=kind)
        x = raw.to(DEV)
        outs = [(ops.preprocess_kpcn(x), kpcn_kernel(s, 5, 104)), (ops.preprocess_kpcn(R.offset_view(x, 1)), kpcn_kernel(s, 5, 104, False)),
                (ops.preprocess_kpcn_prefix(x, s, s)[0], prefix_kernel(5, 104))]
        for got, kernel in outs:
            hold(got, want, bound, "depth %s s %d %s" % (kind, s, kernel), kernel)
            g = got.cpu().numpy()
            if kind in ("zero", "negative"):            # no scaling; clipped to 0; the variance stays the raw variance
                assert float(np.abs(g[..., 30]).max()) == 0.0 and float(np.abs(g[..., 32:34]).max()) == 0.0
            else:
                check_max(g, want)
                assert int(want[..., 30].argmax()) == {"one_positive": 17, "first": 0, "last": 34}[kind]
            if kind == "one_positive":
                assert float(np.delete(g[..., 30].reshape(-1), 17).max()) == 0.0


# ---------------------------------------------------------------------------------------------------- past every cap
def _device_frame(h, w, s, md, C, seed, fill, depth="default"):
    torch.cuda.empty_cache()
    return R.make_frame(h, w, s, md, C, seed, fill=fill, device=DEV, depth=depth)


def _kpcn_past_cap(h, w, s, md, C, kernel, prefix=None):
    """The frame is made on the device; the thirteen channels the reference needs come back.  The deepest pixel is the LAST one: it
    lies in the second trip of every grid-stride loop, the block-wide maximum and its atomicMax included."""
    ops = _ops()
    x = _device_frame(h, w, s, md, C, 500 + s, "kpcn", depth="last")
    x13 = x[..., R.kpcn_channels(md)].cpu().numpy()
    if prefix is None:
        outs, counts = [ops.preprocess_kpcn(x, md).cpu().numpy()], [s]
    else:
        out = ops.preprocess_kpcn_prefix(x, prefix[0], prefix[1], md).cpu().numpy()
        outs, counts = list(out), list(range(prefix[0], prefix[1] + 1))
    del x
    torch.cuda.empty_cache()
    for got, n in zip(outs, counts):
        want, bound = R.kpcn13(x13[:, :, :n])
        hold(got, want, bound, "%s %dx%dx%d" % (kernel, h, w, n), kernel)
        check_max(got, want)
        assert int(want[..., 30].argmax()) == h * w - 1


def _llpm_past_cap(h, w, md, C, off, kernel, rows=512):
    ops = _ops()
    x = _device_frame(h, w, 1, md, C, 600 + md, "llpm")
    if off:
        y = R.offset_view(x, off)
        del x
        x = y
    got = ops.preprocess_llpm(x, md)
    first = R.cmap(md)["bounce"]
    for r0 in range(0, h, rows):                              # compared in row blocks: bounded host temporaries
        want, bound = R.llpm_tail(x[r0:r0 + rows, ..., first:].cpu().numpy(), md)
        hold(got[r0:r0 + rows], want, bound, "%s rows %d.." % (kernel, r0), kernel)
    del x, got
    torch.cuda.empty_cache()


def _gradients_past_cap():
    g = torch.Generator(device=DEV).manual_seed(9)
    buf = torch.randn(224, 224, 44, generator=g, device=DEV)
    buf[::3, ::5] = 0.0
    got = _ops().gradients(buf)
    R.assert_bit_equal(got, R.gradients(buf.cpu().numpy()), "gradients 224x224x44")
    REACHED.add("gradients")


PAST_CAP = {
    # 2,129,920 lanes > 8192 x 256; the finish pass then runs 11.7 M elements
    "lanes": lambda: _kpcn_past_cap(520, 512, 8, 5, 104, "kpcn lanes<true>"),
    # 2,098,152 pixels > 8192 x 256 (the smallest channel map keeps the frame at 1.23 GB)
    "per-pixel": lambda: _kpcn_past_cap(1449, 1448, 3, 0, 49, "kpcn per-pixel"),
    # 131,404 pixels > 4096 tiles x 32
    "prefix": lambda: _kpcn_past_cap(364, 361, 8, 5, 104, "prefix<true>", prefix=(2, 8)),
    # 4,196,352 samples > 16384 x 256
    "llpm-tiled": lambda: _llpm_past_cap(2049, 2048, 1, 60, 0, "llpm tiled"),
    # 57,600 x 37 = 2,131,200 elements > 8192 x 256
    "llpm-generic": lambda: _llpm_past_cap(240, 240, 5, 104, 1, "llpm generic"),
    # 2,207,744 elements > 8192 x 256
    "gradients": _gradients_past_cap,
}


@pytest.mark.parametrize("case", list(PAST_CAP))
def test_every_grid_stride_loop_takes_a_second_trip(case):
    computed = {"lanes": kpcn_kernel(8, 5, 104), "per-pixel": kpcn_kernel(3, 0, 49), "prefix": prefix_kernel(5, 104),
                "llpm-tiled": llpm_kernel(1, 60), "llpm-generic": llpm_kernel(5, 104, False), "gradients": "gradients"}
    expected = {"lanes": "kpcn lanes<true>", "per-pixel": "kpcn per-pixel", "prefix": "prefix<true>", "llpm-tiled": "llpm tiled",
                "llpm-generic": "llpm generic", "gradients": "gradients"}
    assert computed[case] == expected[case]
    PAST_CAP[case]()


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 13, 5), (13, 1, 3), (5, 7, 44), (21, 19, 10)])
def test_gradients_small_frames_bit_equal(shape):
    buf = R.make_frame(shape[0], shape[1], 1, seed=4)[:, :, 0, 2:8].repeat(1, 1, 8)[..., :shape[2]].contiguous()
    R.assert_bit_equal(_ops().gradients(buf.to(DEV)), R.gradients(buf.numpy()), "gradients %s" % (shape,))
    REACHED.add("gradients")


# ---------------------------------------------------------------------------------------------------- the overflowing depth mean
@pytest.mark.parametrize("target", ["plain", "prefix", "per-pixel"])
def test_overflowing_depth_mean_keeps_numpys_nan(target):
    """Four or more depth samples of 1e38 (what sanitize_ leaves of Inf) in pixel (2, 3): the fp32 sum overflows, the mean and the
    image maximum are Inf, that pixel's depth is Inf / Inf.  np.clip keeps the NaN: channels 30..33 of the pixel, d/dx of its right
    neighbour, d/dy of the pixel below; every other depth is finite / Inf = 0.  Counts 1..3 of the prefix pass stay finite (they
    normalise by 1e38; the maximum squared overflows and the variance channel is 0)."""
    ops = _ops()
    s = 5 if target == "per-pixel" else 4
    raw = R.overflow_frame(s)
    x = torch.from_numpy(raw).to(DEV)
    if target == "prefix":
        outs = [(o, n, prefix_kernel(5, 104)) for o, n in zip(ops.preprocess_kpcn_prefix(x, 1, 4), range(1, 5))]
    else:
        outs = [(ops.preprocess_kpcn(x), s, kpcn_kernel(s, 5, 104))]
    for got, n, kernel in outs:
        want, bound = R.kpcn(raw[:, :, :n])
        nan = np.isnan(want)
        if n >= 4:
            expect = np.zeros_like(nan)
            expect[2, 3, 30:34], expect[2, 4, 32], expect[3, 3, 33] = True, True, True
            assert np.array_equal(nan, expect)
        else:
            assert not nan.any() and want[2, 3, 30] == 1.0
        hold(got, want, bound, "overflow %s, %d samples" % (target, n), kernel)


# ---------------------------------------------------------------------------------------------------- the table
def test_error_over_bound_table_of_this_run(request):
    """Printed, and written to the report directory, for whatever part of this file has run before; after the whole file every
    kernel and every <VEC> instance must have been held to the fp64 reference."""
    text = R.format_table()
    print(text)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "data_edges_error_over_bound.txt"), "w") as f:
        f.write(text)
    assert all(v <= 1.0 for v in R.TABLE.values())
    mine = [i for i in request.session.items if i.module is request.module]
    whole = {i.originalname for i in mine} == {k for k, v in vars(request.module).items() if k.startswith("test_") and callable(v)}
    # every case of every test of this file: 13 sample counts, 8 maps, 3 offsets, 4 x 3 prefix ranges, 5 maxima, 6 caps, 5 small
    # gradients, 3 overflow targets, this test
    if whole and len(mine) == len(R.LANES_S + R.PIXEL_S) + len(R.MAPS) + 3 + 12 + 5 + len(PAST_CAP) + 5 + 3 + 1:
        assert REACHED == {"kpcn lanes<true>", "kpcn lanes<false>", "kpcn per-pixel", "prefix<true>", "prefix<false>", "llpm tiled",
                           "llpm generic", "gradients"}
