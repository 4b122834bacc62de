"""The data step of the sample-based denoisers (csrc/sbmc_data.hip) at its tile edges, on every channel map, off 16-byte
alignment and past every grid cap: wcmc_preprocess_sbmc in both forms against the fp64 yardstick ``data_ref.sbmc``, the sample-patch
and sample-tile assemblers against torch indexing of their source buffers.

Bars.  preprocess_sbmc: EVERY element by ``data_ref.assert_within`` -- bound 0 (bit for bit) on every copied, clamped or bit-derived
channel; on the three log groups the rule ``data_ref.llpm_tail`` holds its logarithms to: U / k per rounded operation in front of the
logarithm, LOG_ULPS = 4 ulps of logf and one of the division (data_ref.sbmc's docstring; tests/test_cpu_sampling_ref.py holds the
reference's own fp32 numpy to the same bound).  The channels the function must not read hold NaN, so a wrong offset shows as a NaN;
``data_ref.make_sbmc_frame`` plants the value edges (truncation of non-integer and negative bounce codes, the int16 boundaries, the
1e38 of sanitising, total < diffuse, a non-positive probability, light directions at +-1) at records 0, 127, 128, n - 1 and their
neighbours.  The assemblers only copy: every patch of every batch is compared bit for bit.

Which kernel a call reaches is restated from wcmc_preprocess_sbmc's dispatch (``sb_kernel``).  What cannot be observed from the
outside is which kernel the automatic choice took on a misaligned base: the test holds the result to the reference and to the
aligned call bit for bit, and checks that forcing the tiled form there is refused.

Caps (restated and asserted below):
  sb_preprocess_tiled_kernel   SB_TILE = 128 records per block iteration, at most 16384 blocks: 2,097,282 records take 16386 tiles
  sb_preprocess_kernel         at most 8192 blocks x 256 elements: 22,600 records x 93 outputs = 2,101,800 > 2,097,152
  sa_assemble_kernel<AUG>      at most 65535 blocks, one work unit each: 1171 patches of 8 x 8 at S = 5 with every buffer on are
                               56 x 1171 = 65,576 units (1170: 65,520)
  sa_assemble_tiles_kernel     the same cap: 1366 tiles are 48 x 1366 = 65,568 units (1365: 65,520)

Measured on one MI355X (profiles/sampling_sbmc_edges_error.txt), largest |err| / bound (sbmc_s / sbmc_p; 0 on the exact channels):
  tile edges       n = 1: 0.02 / 0.11, 127: 0.65 / 0.28, 128: 0.51 / 0.27, 129: 0.60 / 0.28, 255: 0.77 / 0.28, 256: 0.85 / 0.28,
                   257: 0.65 / 0.29, 389: 0.60 / 0.30; tiled, generic and automatic bit-equal
  channel maps     0.49 .. 0.91 / 0.28 .. 0.32 over the eight pairs       off alignment   0.82 / 0.32, bit-equal to the aligned call
  second trips     generic 0.95 / 0.77, tiled 0.99 / 0.77 (log(1 + total) / 10 of a total next to zero: U / 10 is all of the bound)
  assemblers       every patch of the three batches bit-equal
"""
import os

import numpy as np
import pytest
import torch

import data_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("WCMC_TEST_REPORTS", os.path.join(ROOT, "test_reports"))     # (git-ignored)
DEV = "cuda:0"
SB_TILE = 128
TILED, GENERIC = "sb_preprocess tiled", "sb_preprocess generic"
REACHED = set()


def _ops():
    from wcmc_amd import ops
    return ops


def sb_kernel(md, C, aligned=True, tiled=None):
    """wcmc_preprocess_sbmc's dispatch: the tiled form needs whole float4 per record inside C, an aligned base and <= 64 KB of LDS."""
    w4 = (24 + 7 * (md + 1) + 3) // 4
    can = C % 4 == 0 and 4 * w4 <= C and aligned and SB_TILE * (4 * w4 + 1) * 4 <= 64 * 1024
    if tiled:
        assert can
    return TILED if can and tiled is not False else GENERIC


def hold(got, ref, what, kernel):
    """(got_s, got_p) against data_ref.sbmc's (want_s, want_p, bound_s, bound_p): every element."""
    REACHED.add(kernel)
    for name, g, want, bound in (("sbmc_s", got[0], ref[0], ref[2]), ("sbmc_p", got[1], ref[1], ref[3])):
        assert g.dtype == torch.float32 and tuple(g.shape) == want.shape, (what, name, tuple(g.shape), want.shape)
        c = want.shape[-1]                                    # (records x channels: one column of the table per buffer)
        R.assert_within(g.reshape(-1, c), want.reshape(-1, c), bound.reshape(-1, c), "%s %s [%s]" % (what, name, kernel),
                        "%s %s" % (kernel, name))


def _forms(md, C, aligned=True):
    """(tiled argument, kernel reached) of every form that applies."""
    out = [(False, GENERIC), (None, sb_kernel(md, C, aligned))]
    if sb_kernel(md, C, aligned) == TILED:
        out.append((True, TILED))
    return out


# ---------------------------------------------------------------------------------------------------- tile edges
@pytest.mark.parametrize("n", [1, 127, 128, 129, 255, 256, 257, 3 * 128 + 5])
def test_preprocess_sbmc_at_the_tile_edges(n):
    ops = _ops()
    raw = R.make_sbmc_frame(n, 5, 104, seed=40 + n)
    ref = R.sbmc(raw.numpy(), 5)
    x = raw.to(DEV)
    forms = _forms(5, 104)
    assert [k for _, k in forms] == [GENERIC, TILED, TILED]
    outs = []
    for tiled, kernel in forms:
        got = ops.preprocess_sbmc(x, 5, tiled=tiled)
        hold(got, ref, "n = %d, tiled = %s" % (n, tiled), kernel)
        again = ops.preprocess_sbmc(x, 5, tiled=tiled)
        R.assert_bit_equal(again[0], got[0], "two calls")
        R.assert_bit_equal(again[1], got[1], "two calls")
        outs.append(got)
    for got in outs[1:]:                                    # the forms share sb_s_value / sb_p_value
        R.assert_bit_equal(got[0], outs[0][0], "n = %d: tiled against generic, sbmc_s" % n)
        R.assert_bit_equal(got[1], outs[0][1], "n = %d: tiled against generic, sbmc_p" % n)


# ---------------------------------------------------------------------------------------------------- channel maps
@pytest.mark.parametrize("md,C", R.MAPS)
def test_preprocess_sbmc_every_channel_map(md, C):
    """The tiled condition holds for (1, 60), (3, 84), (5, 104), (5, 108).  (h, w, s) = (3, 43, 3): 387 records."""
    ops = _ops()
    assert (sb_kernel(md, C) == TILED) == ((md, C) in ((1, 60), (3, 84), (5, 104), (5, 108)))
    n = 3 * 43 * 3
    raw = R.make_sbmc_frame(n, md, C, seed=60 + md)
    ref = tuple(a.reshape(3, 43, 3, -1) for a in R.sbmc(raw.numpy(), md))
    x = raw.to(DEV).view(3, 43, 3, C)
    for tiled, kernel in _forms(md, C):
        got = ops.preprocess_sbmc(x, md, tiled=tiled)
        assert got[0].shape == (3, 43, 3, 27) and got[1].shape == (3, 43, 3, 11 * (md + 1))
        hold(got, ref, "md %d C %d, tiled = %s" % (md, C, tiled), kernel)
    if sb_kernel(md, C) == GENERIC:
        with pytest.raises(RuntimeError, match="tiled form"):
            ops.preprocess_sbmc(x, md, tiled=True)


# ---------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("off", [1, 2, 3])
def test_preprocess_sbmc_on_a_base_off_16_byte_alignment(off):
    ops = _ops()
    for md, C, n in ((5, 104, 257), (1, 60, 129)):
        raw = R.make_sbmc_frame(n, md, C, seed=80 + off)
        ref = R.sbmc(raw.numpy(), md)
        x = raw.to(DEV)
        y = R.offset_view(x, off)
        assert sb_kernel(md, C) == TILED and sb_kernel(md, C, aligned=False) == GENERIC
        got = ops.preprocess_sbmc(y, md)
        hold(got, ref, "md %d C %d +%d floats" % (md, C, off), GENERIC)
        want = ops.preprocess_sbmc(x, md)
        R.assert_bit_equal(got[0], want[0], "+%d floats against the aligned call, sbmc_s" % off)
        R.assert_bit_equal(got[1], want[1], "+%d floats against the aligned call, sbmc_p" % off)
        forced = ops.preprocess_sbmc(y, md, tiled=False)
        R.assert_bit_equal(forced[0], got[0], "automatic against forced generic")
        R.assert_bit_equal(forced[1], got[1], "automatic against forced generic")
        with pytest.raises(RuntimeError, match="tiled form"):
            ops.preprocess_sbmc(y, md, tiled=True)


# ---------------------------------------------------------------------------------------------------- second trips
def _past_cap(n, md, C, tiled, kernel, rows):
    ops = _ops()
    torch.cuda.empty_cache()
    x = R.make_sbmc_frame(n, md, C, seed=700 + md, device=DEV)
    got = ops.preprocess_sbmc(x, md, tiled=tiled)
    used = 24 + 7 * (md + 1)
    assert bool(torch.isnan(x[n - 1, 0, 0, used:]).all())
    from concurrent.futures import ThreadPoolExecutor
    starts = list(range(0, n, rows))                          # compared in row blocks: bounded host temporaries
    with ThreadPoolExecutor(4) as pool:                       # four references at a time (numpy releases the interpreter lock)
        for g0 in range(0, len(starts), 4):
            group = starts[g0:g0 + 4]
            blocks = [x[r0:r0 + rows, ..., :used].cpu().numpy() for r0 in group]
            for r0, ref in zip(group, pool.map(lambda a: R.sbmc(a, md), blocks)):
                hold((got[0][r0:r0 + rows], got[1][r0:r0 + rows]), ref, "%s records %d.." % (kernel, r0), kernel)
    del x, got
    torch.cuda.empty_cache()


def test_generic_form_takes_a_second_trip():
    n, md = 22600, 5
    outputs = 27 + 11 * (md + 1)
    assert outputs == 93 and n * outputs == 2101800 > 8192 * 256 == 2097152         # sb_grid: blocks x threads
    assert (n - 1) * outputs >= 8192 * 256                   # the planted record n - 1 lies wholly in the second trip
    _past_cap(n, md, 104, False, GENERIC, rows=8192)


def test_tiled_form_takes_a_second_trip():
    n, md, C = 2097152 + 130, 1, 60
    assert sb_kernel(md, C, tiled=True) == TILED
    assert -(-n // SB_TILE) == 16386 > 16384                 # tiles against the block cap: blocks 0 and 1 take a second one
    assert n % SB_TILE == 2                                  # ... and block 1's is partial
    _past_cap(n, md, C, True, TILED, rows=1 << 18)


# ---------------------------------------------------------------------------------------------------- assemblers past 65,535 units
H = W = 40
S, P, PAD = 5, 8, 3
CHUNK = 128                                                  # patches per comparison


def _units(b, with_gt):
    """sa_assemble_launch / wcmc_assemble_sample_tiles: rows = B P ceil(P / 32) per chunk of 4 samples of each per-sample source
    (sbmc_s, sbmc_p, llpm), plus rows for gt."""
    rows = b * P * -(-P // 32)
    return 3 * rows * -(-S // 4) + (rows if with_gt else 0)


def _buffers():
    """Every float of the four source buffers is its own number (exact in fp32: below 2^24)."""
    def mk(c, base, shape):
        return (torch.arange(int(np.prod(shape)) * c, device=DEV, dtype=torch.float32) + base).view(*shape, c)
    out = mk(27, 0.0, (H, W, S)), mk(66, 1.0e6, (H, W, S)), mk(37, 3.0e6, (H, W, S)), mk(9, 4.0e6, (H, W))
    assert float(out[3].max()) < 2 ** 24
    return out


def _dihedral(a, t):
    """Transform code t on the two last axes: rot90(fliplr(a) if t & 4 else a, k = t & 3)."""
    return torch.rot90(a.flip(-1) if t & 4 else a, t & 3, (-2, -1))


def _expected(bufs, origins, codes=None):
    """The batch of the windows at ``origins`` ((b, 2) long, inside the buffers) by torch indexing: (b, S, C, P, P) entries."""
    ss, sp, ll, gt = bufs
    ar = torch.arange(P, device=DEV)
    rows, cols = (origins[:, 0:1] + ar)[:, :, None], (origins[:, 1:2] + ar)[:, None, :]
    win = lambda t: t[rows, cols]                                                    # noqa: E731  (b, P, P, ...)
    to = lambda t: t.permute(0, 3, 4, 1, 2)                                          # noqa: E731
    s_w, p_w, l_w = win(ss), win(sp), win(ll)
    out = {"radiance": to(s_w[..., :3]), "features": torch.cat([to(s_w[..., 3:]), to(p_w), to(l_w[..., :1])], dim=2),
           "paths": to(l_w[..., 1:])}
    if gt is not None:
        out["target_image"] = win(gt)[..., :3].permute(0, 3, 1, 2)
    if codes is not None:
        for k, v in out.items():
            v = v.contiguous()
            for t in range(8):
                sel = (codes == t).nonzero().view(-1)
                if sel.numel():
                    v[sel] = _dihedral(v[sel], t)
            out[k] = v
    return out


def _compare_batch(got, bufs, origins, codes, what):
    b = origins.shape[0]
    assert got["radiance"].shape == (b, S, 3, P, P) and got["features"].shape == (b, S, 91, P, P) and got["paths"].shape == (b, S, 36, P, P)
    for c0 in list(range(0, b, CHUNK)) + [b - 1]:             # every patch, in chunks; the last patch once more on its own
        c1 = min(c0 + CHUNK, b)
        want = _expected(bufs, origins[c0:c1], None if codes is None else codes[c0:c1])
        assert set(want) <= set(got)
        for k, v in want.items():
            g = got[k][c0:c1]
            if not torch.equal(g, v):
                bad = (g != v).nonzero()[0].tolist()
                raise AssertionError("%s: %s differs, first at patch %d %s" % (what, k, c0 + bad[0], bad[1:]))


@pytest.mark.parametrize("aug", [False, True])
def test_sample_patch_assembler_past_65535_units(aug):
    ops = _ops()
    b = 1171
    assert _units(b, True) == 56 * b == 65576 > 65535 >= _units(b - 1, True) == 65520
    bufs = _buffers()
    rng = np.random.RandomState(17)
    origins = np.stack([rng.randint(0, H - P + 1, size=b), rng.randint(0, W - P + 1, size=b)], axis=1).astype(np.int32)
    origins[-1] = (H - P, W - P)
    codes = (np.arange(b) % 8).astype(np.int32) if aug else None
    got = ops.assemble_sample_patches(*bufs, origins, P, transforms=codes)
    assert got["target_image"].shape == (b, 3, P, P)
    o = torch.from_numpy(origins).to(DEV).long()
    c = None if codes is None else torch.from_numpy(codes).to(DEV)
    _compare_batch(got, bufs, o, c, "assemble_sample_patches%s" % ("_aug" if aug else ""))
    again = ops.assemble_sample_patches(*bufs, origins, P, transforms=codes)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_sample_tile_assembler_past_65535_units():
    ops = _ops()
    b = 1366
    assert _units(b, False) == 48 * b == 65568 > 65535 >= _units(b - 1, False) == 65520
    ss, sp, ll, _ = _buffers()
    rng = np.random.RandomState(18)
    origins = np.stack([rng.randint(-PAD, H + PAD - P + 1, size=b), rng.randint(-PAD, W + PAD - P + 1, size=b)], axis=1).astype(np.int32)
    origins[0], origins[-1] = (-PAD, -PAD), (H + PAD - P, W + PAD - P)
    d_org = torch.from_numpy(origins).to(DEV)
    got = ops.assemble_sample_tiles(ss, sp, ll, d_org, P, PAD)
    assert set(got) == {"radiance", "features", "paths"}
    # the frame extended by PAD pixels by reflection with the edge repeated (numpy.pad's 'symmetric'), as a copy
    def mirror(n):
        i = torch.arange(-PAD, n + PAD, device=DEV)
        return torch.where(i < 0, -1 - i, torch.where(i >= n, 2 * n - 1 - i, i))
    padded = tuple(t[mirror(H)][:, mirror(W)].contiguous() for t in (ss, sp, ll))
    assert padded[0].shape == (H + 2 * PAD, W + 2 * PAD, S, 27) and torch.equal(padded[0][0, 0], ss[2, 2]) and torch.equal(padded[0][-1, -1], ss[H - 3, W - 3])
    _compare_batch(got, padded + (None,), d_org.long() + PAD, None, "assemble_sample_tiles")
    again = ops.assemble_sample_tiles(ss, sp, ll, d_org, P, PAD)
    assert all(torch.equal(got[k], again[k]) for k in got)


# ---------------------------------------------------------------------------------------------------- the table
def format_rows():
    keys = sorted(k for k, _ in R.TABLE if k.startswith("sb_preprocess"))
    lines = ["%-32s%18s" % ("kernel, buffer", "max |err| / bound")]
    lines += ["%-32s%18.3f" % (k, R.TABLE[(k, "all")]) for k in keys]
    return "\n".join(lines) + "\n"


def test_error_over_bound_table_of_this_run(request):
    """Printed, and written to the report directory, for whatever part of this file has run before; after the whole file both forms
    of preprocess_sbmc must have been held to the fp64 reference."""
    text = format_rows()
    print(text)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "sbmc_edges_error_over_bound.txt"), "w") as f:
        f.write(text)
    assert all(v <= 1.0 for (k, _), v in R.TABLE.items() if k.startswith("sb_preprocess"))
    mine = [i for i in request.session.items if i.module is request.module]
    whole = {i.originalname for i in mine} == {k for k, v in vars(request.module).items() if k.startswith("test_") and callable(v)}
    # every case of every test of this file: 8 sizes, 8 maps, 3 offsets, 2 second trips, 2 + 1 assemblers, this test
    if whole and len(mine) == 8 + len(R.MAPS) + 3 + 2 + 3 + 1:
        assert REACHED == {TILED, GENERIC}
        assert {k for k, _ in R.TABLE if k.startswith("sb_preprocess")} == {"%s %s" % (k, b) for k in (TILED, GENERIC) for b in ("sbmc_s", "sbmc_p")}
