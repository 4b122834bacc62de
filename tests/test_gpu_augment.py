"""GPU tests of the dihedral patch augmentation in the device patch assemblers (``wcmc_assemble_kpcn_patches``
and ``wcmc_assemble_sample_patches`` with a code table).  Everything is held to ``torch.equal``: the per-pixel channels are copies and every
retaken difference is one fp32 subtraction of two stored floats.

Where a source pixel lies is never computed from the formulas of the specification here: an index image of the frame goes through
``rot90(fliplr(.))`` and is read back (``_window``).

Frames: ``data_ref.make_frame`` (both fills merged, the channels neither fill writes set to seeded uniform values: all finite),
24 x 40 -- not square, so a swapped axis cannot hide -- with 8-pixel patches."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden_dataset as mgd  # noqa: E402
from data_ref import make_frame  # noqa: E402

DEV = "cuda:0"
H, W, P = 24, 40, 8
# all four corners, one window touching each single edge (top, bottom, left, right), one interior window
ORIGINS = [(0, 0), (0, W - P), (H - P, 0), (H - P, W - P), (0, 13), (H - P, 7), (5, 0), (9, W - P), (7, 11)]
# the 44-channel KPCN record: value channels, where their x- and y-differences are stored, and the per-pixel rest
VAL = [0, 1, 2, 10, 11, 12, 20, 21, 22, 30, 34, 35, 36]
DX = [4, 5, 6, 14, 15, 16, 24, 25, 26, 32, 38, 39, 40]
DY = [7, 8, 9, 17, 18, 19, 27, 28, 29, 33, 41, 42, 43]
PER_PIXEL = [c for c in range(44) if c not in DX and c not in DY]


def T(a, t, dims=(0, 1)):
    """Transform code t on two axes of a tensor: rot90(fliplr(a) if t & 4 else a, k = t & 3)."""
    return torch.rot90(a.flip(dims[1]) if t & 4 else a, t & 3, dims)


def _gt(h, w, seed):
    gt = mgd.test_gt(h, w, seed)
    gt[..., 0:3] += 0.25                               # total > diffuse: log(1 + total - diffuse) is defined
    return gt


def finite_frame(h, w, s, seed):
    x, y = make_frame(h, w, s, seed=seed, fill="kpcn"), make_frame(h, w, s, seed=seed + 1, fill="llpm")
    raw = torch.where(torch.isnan(x), y, x)
    rest = torch.rand(raw.shape, generator=torch.Generator().manual_seed(seed + 2))
    raw = torch.where(torch.isnan(raw), rest, raw)
    assert bool(torch.isfinite(raw).all())
    return raw.contiguous()


def _window(t, r0, c0, h, w, p):
    """``(F, R0, C0)``: the index image of the h x w frame under code t and the origin, in it, of the p x p block that holds the
    pixels of the source window at (r0, c0)."""
    index = torch.arange(h * w).view(h, w)
    F = T(index, t).contiguous()
    pos = torch.isin(F, index[r0:r0 + p, c0:c0 + p].reshape(-1)).nonzero()
    R0, C0 = int(pos[:, 0].min()), int(pos[:, 1].min())
    assert int(pos[:, 0].max()) == R0 + p - 1 and int(pos[:, 1].max()) == C0 + p - 1 and len(pos) == p * p
    return F, R0, C0


def _sources(t, r0, c0, h, w, p):
    """Flat frame indices (p, p) of the source of every output pixel, of its left neighbour and of its upper neighbour in the
    transformed frame; -1 where the transformed frame has no such neighbour (its first column / row)."""
    F, R0, C0 = _window(t, r0, c0, h, w, p)
    pad = torch.full((F.shape[0] + 1, F.shape[1] + 1), -1, dtype=F.dtype)
    pad[1:, 1:] = F
    src = pad[R0 + 1:R0 + 1 + p, C0 + 1:C0 + 1 + p]
    left = pad[R0 + 1:R0 + 1 + p, C0:C0 + p]
    up = pad[R0:R0 + p, C0 + 1:C0 + 1 + p]
    return src.to(DEV), left.to(DEV), up.to(DEV)


@pytest.fixture(scope="module")
def frames():
    """Per sample count S: the raw frame, gt and the resident buffers of both families.  Computed once, never written to."""
    from wcmc_amd import ops
    out = {}
    for S in (2, 3):
        raw = finite_frame(H, W, S, 40 + S).to(DEV)
        gt = torch.from_numpy(_gt(H, W, 50 + S)).to(DEV)
        ss, sp = ops.preprocess_sbmc(raw)
        out[S] = {"raw": raw, "gt": gt, "kpcn": ops.preprocess_kpcn(raw), "llpm": ops.preprocess_llpm(raw), "sbmc_s": ss, "sbmc_p": sp}
        for k, v in out[S].items():
            assert bool(torch.isfinite(v).all()), (S, k)
    torch.cuda.synchronize()
    return out


def _origins(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def _frame_planes(f, llpm, spp, h=H, w=W, p=P):
    """(3, h * w) planes of ``target_diffuse`` / ``target_specular`` from the existing assembler over the windows that tile the frame:
    a division and a logarithm per pixel whose device arithmetic is not what these tests are about."""
    from wcmc_amd import ops
    tiles = [(r, c) for r in range(0, h, p) for c in range(0, w, p)]
    plain = ops.assemble_kpcn_patches(f["kpcn"], llpm, f["gt"], _origins(tiles), p, spp=spp)
    plane = lambda x: x.view(h // p, w // p, 3, p, p).permute(2, 0, 3, 1, 4).reshape(3, h * w)       # noqa: E731
    return {k: plane(plain[k]) for k in ("target_diffuse", "target_specular")}


def restate_kpcn(f, llpm, origins, codes, spp, h=H, w=W, p=P):
    """The KPCN batch of the specification in torch, from the resident buffers."""
    kp, gt = f["kpcn"].view(h * w, 44), f["gt"].view(h * w, 9)
    planes = _frame_planes(f, llpm, spp, h, w, p)
    out = {k: [] for k in ("kpcn_diffuse_in", "kpcn_specular_in", "kpcn_diffuse_buffer", "kpcn_specular_buffer", "kpcn_albedo",
                           "target_diffuse", "target_specular", "target_total")}
    if llpm is not None:
        out["paths"] = []
    chw = lambda x: x.permute(2, 0, 1)                                                             # noqa: E731
    for (r0, c0), t in zip(origins, codes):
        src, left, up = _sources(t, r0, c0, h, w, p)
        rec = kp[src].clone()                                                                      # (p, p, 44): per-pixel channels
        for nb, dst in ((left, DX), (up, DY)):                                                     # gradient channels
            diff = rec[..., VAL] - kp[nb.clamp(min=0)][..., VAL]                                   # fp32 subtraction of stored floats
            rec[..., dst] = torch.where((nb >= 0)[..., None], diff, torch.zeros_like(diff))
        din, sin = [rec[..., 0:10], rec[..., 20:44]], [rec[..., 10:44]]
        if llpm is not None:
            l = llpm.view(h * w, llpm.shape[2], 37)[src]                                           # (p, p, S, 37)
            pw = torch.zeros((p, p), device=DEV)
            for s in range(spp):
                pw = pw + l[:, :, s, 0]                                                            # in sample order
            pw = (pw / torch.full_like(pw, float(spp)))[..., None]      # (a tensor divisor: torch multiplies by 1 / scalar otherwise)
            din.append(pw)
            sin.append(pw)
            out["paths"].append(l[:, :, :spp, 1:37].permute(2, 3, 0, 1))
        out["kpcn_diffuse_in"].append(chw(torch.cat(din, dim=2)))
        out["kpcn_specular_in"].append(chw(torch.cat(sin, dim=2)))
        out["kpcn_diffuse_buffer"].append(chw(rec[..., 0:3]))
        out["kpcn_specular_buffer"].append(chw(rec[..., 10:13]))
        out["kpcn_albedo"].append(chw(rec[..., 34:37] + 0.00316))
        out["target_total"].append(chw(gt[src][..., 0:3]))
        for k in ("target_diffuse", "target_specular"):
            out[k].append(planes[k][:, src])
    return {k: torch.stack(v).contiguous() for k, v in out.items()}


def _assert_batches_equal(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        if not torch.equal(got[k], want[k]):
            bad = (got[k] != want[k]).nonzero()
            raise AssertionError("%s: %s differs in %d entries, first at %s" % (what, k, len(bad), bad[0].tolist()))


# ------------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("S,spp,with_llpm", [(2, None, True), (2, None, False), (3, None, True), (3, None, False), (3, 2, True)])
def test_kpcn_batch_equals_the_restatement_from_the_resident_buffers(frames, S, spp, with_llpm):
    from wcmc_amd import ops
    f = frames[S]
    llpm = f["llpm"] if with_llpm else None
    # every origin under every code, in ONE batch: 72 patches (more than one block), neighbouring patches with different codes
    origins = [o for o in ORIGINS for _ in range(8)]
    codes = [t for _ in ORIGINS for t in range(8)]
    assert set(codes[:8]) == set(range(8))                                                       # eight different codes at once
    got = ops.assemble_kpcn_patches(f["kpcn"], llpm, f["gt"], _origins(origins), P, spp=spp, transforms=np.array(codes, np.int32))
    want = restate_kpcn(f, llpm, origins, codes, (spp or S) if with_llpm else None)
    if with_llpm:
        assert got["paths"].shape == (72, spp or S, 36, P, P)
    _assert_batches_equal(got, want, "S = %d, spp = %s, llpm %s" % (S, spp, with_llpm))
    # the zero rule is in play: windows on the transformed frame's first column / row carry exact zeros there, others do not
    dx = got["kpcn_diffuse_in"][:, 4:7]
    assert bool((dx[0 * 8 + 0][:, :, 0] == 0).all()) and not bool((dx[8 * 8 + 0][:, :, 0] == 0).all())


def test_one_small_batch_of_eight_different_codes(frames):
    """Eight patches at ONE origin, each under its own code: one block, a wave that changes code every 64 pixels."""
    from wcmc_amd import ops
    f = frames[2]
    origins, codes = [(7, 11)] * 8, list(range(8))
    got = ops.assemble_kpcn_patches(f["kpcn"], f["llpm"], f["gt"], _origins(origins), P, transforms=torch.tensor(codes, dtype=torch.int32))
    _assert_batches_equal(got, restate_kpcn(f, f["llpm"], origins, codes, 2), "eight codes")
    # an interior window: its per-pixel entries are T_t of the untransformed entry
    for t in range(8):
        assert torch.equal(got["target_total"][t], T(got["target_total"][0], t, (1, 2)))
        assert torch.equal(got["paths"][t], T(got["paths"][0], t, (2, 3)))


def test_patches_that_are_no_multiple_of_the_wave_and_wider_than_a_chunk():
    """P = 37 on a 41 x 75 frame: a wave straddles two patches with different codes (P * P is odd), and the sample assembler's rows
    take two chunks of 32 pixels, the second one partial.  Both families against their references."""
    from wcmc_amd import ops
    h, w, p, S = 41, 75, 37, 2
    raw = finite_frame(h, w, S, 77).to(DEV)
    f = {"raw": raw, "gt": torch.from_numpy(_gt(h, w, 78)).to(DEV), "kpcn": ops.preprocess_kpcn(raw), "llpm": ops.preprocess_llpm(raw)}
    origins, codes = [(0, 0), (4, 38), (2, 17), (4, 0), (0, 38), (3, 3), (1, 30), (4, 38)], list(range(8))
    # (the restatement's target planes come from a tiling: 37 does not tile the frame, so they are checked as gathers below)
    got = ops.assemble_kpcn_patches(f["kpcn"], f["llpm"], f["gt"], _origins(origins), p, transforms=np.array(codes, np.int32))
    plain = ops.assemble_kpcn_patches(f["kpcn"], f["llpm"], f["gt"], _origins(origins), p)
    kp = f["kpcn"].view(h * w, 44)
    for b, ((r0, c0), t) in enumerate(zip(origins, codes)):
        src, left, up = _sources(t, r0, c0, h, w, p)
        rec = kp[src].clone()
        for nb, dst in ((left, DX), (up, DY)):
            diff = rec[..., VAL] - kp[nb.clamp(min=0)][..., VAL]
            rec[..., dst] = torch.where((nb >= 0)[..., None], diff, torch.zeros_like(diff))
        assert torch.equal(got["kpcn_specular_in"][b, :34], rec[..., 10:44].permute(2, 0, 1)), (b, t)
        assert torch.equal(got["kpcn_diffuse_in"][b, :10], rec[..., 0:10].permute(2, 0, 1)), (b, t)
        for k in ("target_diffuse", "target_specular", "target_total", "kpcn_albedo", "paths"):
            assert torch.equal(got[k][b], T(plain[k][b], t, (-2, -1))), (b, t, k)
        assert torch.equal(got["kpcn_diffuse_in"][b, 34], T(plain["kpcn_diffuse_in"][b, 34], t)), (b, t)
    ss, sp = ops.preprocess_sbmc(raw)
    got = ops.assemble_sample_patches(ss, sp, f["llpm"], f["gt"], np.array(origins, np.int32), p, transforms=np.array(codes, np.int32))
    plain = ops.assemble_sample_patches(ss, sp, f["llpm"], f["gt"], np.array(origins, np.int32), p)
    for k in plain:
        for b, t in enumerate(codes):
            assert torch.equal(got[k][b], T(plain[k][b], t, (-2, -1))), (k, b, t)


# ------------------------------------------------------------------------------------------------- 2. the whole frame transformed
@pytest.mark.parametrize("t", range(8))
def test_kpcn_batch_equals_preprocessing_the_transformed_frame(frames, t):
    """Transform raw and gt on the host, preprocess with the existing kernels, assemble with the existing entry at the transformed
    origins: the augmented entry on the untransformed buffers gives those bits."""
    from wcmc_amd import ops
    f = frames[2]
    raw_t, gt_t = T(f["raw"].cpu(), t).contiguous().to(DEV), T(f["gt"].cpu(), t).contiguous().to(DEV)
    kp_t, ll_t = ops.preprocess_kpcn(raw_t), ops.preprocess_llpm(raw_t)
    # the premise: preprocessing is position-independent per pixel (the differences are what is NOT)
    assert torch.equal(kp_t[..., PER_PIXEL], T(f["kpcn"], t)[..., PER_PIXEL]), "preprocess_kpcn depends on the pixel's position"
    assert torch.equal(ll_t, T(f["llpm"], t)), "preprocess_llpm depends on the pixel's position"
    origins_t = [_window(t, r0, c0, H, W, P)[1:] for r0, c0 in ORIGINS]
    want = ops.assemble_kpcn_patches(kp_t, ll_t, gt_t, _origins(origins_t), P)
    got = ops.assemble_kpcn_patches(f["kpcn"], f["llpm"], f["gt"], _origins(ORIGINS), P, transforms=np.full(len(ORIGINS), t, np.int32))
    _assert_batches_equal(got, want, "code %d" % t)


# ------------------------------------------------------------------------------------------------- 3. sample-based batches
@pytest.mark.parametrize("use_g_buf,use_sbmc_buf", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("with_llpm", [True, False])
def test_sample_batch_equals_the_existing_assembler_on_transformed_buffers(frames, use_g_buf, use_sbmc_buf, with_llpm):
    from wcmc_amd import ops
    f = frames[2]
    llpm = f["llpm"] if with_llpm else None
    keys = {"radiance", "features", "target_image"} | ({"paths"} if with_llpm else set())
    origins = np.array(ORIGINS, np.int32)
    mixed = {k: [] for k in keys}
    for t in range(8):
        tr = lambda x: None if x is None else T(x, t).contiguous()                                  # noqa: E731
        origins_t = np.array([_window(t, r0, c0, H, W, P)[1:] for r0, c0 in ORIGINS], np.int32)
        want = ops.assemble_sample_patches(tr(f["sbmc_s"]), tr(f["sbmc_p"]), tr(llpm), tr(f["gt"]), origins_t, P, use_g_buf, use_sbmc_buf)
        got = ops.assemble_sample_patches(f["sbmc_s"], f["sbmc_p"] if use_sbmc_buf else None, llpm, f["gt"], origins, P, use_g_buf,
                                          use_sbmc_buf, transforms=np.full(len(ORIGINS), t, np.int32))
        assert set(got) == keys
        _assert_batches_equal(got, want, "code %d" % t)
        for k in keys:
            mixed[k].append(want[k][t])                                                           # origin t under code t
    # and eight different codes in one batch
    got = ops.assemble_sample_patches(f["sbmc_s"], f["sbmc_p"], llpm, f["gt"], origins[:8], P, use_g_buf, use_sbmc_buf,
                                      transforms=np.arange(8, dtype=np.int32))
    _assert_batches_equal(got, {k: torch.stack(v) for k, v in mixed.items()}, "mixed codes")


def test_sample_batch_from_a_prefix_under_a_transform(frames):
    from wcmc_amd import ops
    f = frames[3]
    origins, codes = np.array(ORIGINS[:8], np.int32), np.arange(8, dtype=np.int32)
    got = ops.assemble_sample_patches(f["sbmc_s"], f["sbmc_p"], f["llpm"], f["gt"], origins, P, spp=2, transforms=codes)
    plain = ops.assemble_sample_patches(f["sbmc_s"], f["sbmc_p"], f["llpm"], f["gt"], origins, P, spp=2)
    assert got["radiance"].shape == (8, 2, 3, P, P)
    for k in plain:
        for b in range(8):
            assert torch.equal(got[k][b], T(plain[k][b], b, (-2, -1))), (k, b)


# ------------------------------------------------------------------------------------------------- 4. identity
@pytest.mark.parametrize("S,spp", [(2, None), (3, None), (3, 2)])
def test_zero_codes_and_no_codes_are_the_plain_entry_points(frames, S, spp):
    from wcmc_amd import ops
    f = frames[S]
    o, zero = _origins(ORIGINS), torch.zeros(len(ORIGINS), dtype=torch.int32, device=DEV)
    for llpm in (f["llpm"], None):
        plain = ops.assemble_kpcn_patches(f["kpcn"], llpm, f["gt"], o, P, spp=spp)
        _assert_batches_equal(ops.assemble_kpcn_patches(f["kpcn"], llpm, f["gt"], o, P, spp=spp, transforms=zero), plain, "kpcn, zeros")
        _assert_batches_equal(ops.assemble_kpcn_patches(f["kpcn"], llpm, f["gt"], o, P, spp=spp, transforms=None), plain, "kpcn, None")
        for use_g_buf, use_sbmc_buf in ((True, True), (True, False), (False, True), (False, False)):
            args = (f["sbmc_s"], f["sbmc_p"], llpm, f["gt"], o, P, use_g_buf, use_sbmc_buf)
            plain = ops.assemble_sample_patches(*args, spp=spp)
            _assert_batches_equal(ops.assemble_sample_patches(*args, spp=spp, transforms=zero), plain, "sample, zeros")
            _assert_batches_equal(ops.assemble_sample_patches(*args, spp=spp, transforms=None), plain, "sample, None")


def test_a_bad_table_is_refused_by_the_python_functions(frames):
    from wcmc_amd import ops
    from wcmc_amd.support.datasets import PatchBatcher, SamplePatchBatcher
    f, o = frames[2], _origins(ORIGINS)
    for bad, word in ((np.full(9, 8, np.int32), "outside 0..7"), (np.zeros(8, np.int32), "one code per patch"),
                      (np.zeros(9, np.int64), "int32"), (torch.full((9,), -1, dtype=torch.int32, device=DEV), "outside 0..7")):
        with pytest.raises(ValueError, match="assemble_kpcn_patches: .*" + word):
            ops.assemble_kpcn_patches(f["kpcn"], f["llpm"], f["gt"], o, P, transforms=bad)
        with pytest.raises(ValueError, match="assemble_sample_patches: .*" + word):
            ops.assemble_sample_patches(f["sbmc_s"], f["sbmc_p"], f["llpm"], f["gt"], o, P, transforms=bad)
        with pytest.raises(ValueError, match=word):
            PatchBatcher(P, 9).batch(f["kpcn"], f["llpm"], f["gt"], o, transforms=bad)
        with pytest.raises(ValueError, match=word):
            SamplePatchBatcher(P, 9).batch(f["sbmc_s"], f["sbmc_p"], f["llpm"], f["gt"], o, transforms=bad)
    # the batchers pass a good one through
    codes = np.arange(9, dtype=np.int32) % 8
    a = PatchBatcher(P, 9).batch(f["kpcn"], f["llpm"], f["gt"], o, transforms=codes)
    _assert_batches_equal(a, ops.assemble_kpcn_patches(f["kpcn"], f["llpm"], f["gt"], o, P, transforms=codes), "PatchBatcher")
    a = SamplePatchBatcher(P, 9).batch(f["sbmc_s"], f["sbmc_p"], f["llpm"], f["gt"], o, transforms=codes)
    _assert_batches_equal(a, ops.assemble_sample_patches(f["sbmc_s"], f["sbmc_p"], f["llpm"], f["gt"], o, P, transforms=codes),
                          "SamplePatchBatcher")


# ------------------------------------------------------------------------------------------------- 5. the loader
LB, PPI, LS = 4, 8, 3


@pytest.fixture(scope="module")
def loader_dir(tmp_path_factory):
    """Two 24 x 40 training frames with 3 samples per pixel in a dataset directory, their probability maps written."""
    from wcmc_amd.support.datasets import DenoiseDirectory
    root = str(tmp_path_factory.mktemp("augment_data"))
    for k, (mode, name) in enumerate((("train", "room"), ("train", "car"), ("val", "den"))):     # (val: for the launchers)
        for d in ("gt", "input"):
            os.makedirs(os.path.join(root, mode, d), exist_ok=True)
        np.save(os.path.join(root, mode, "input", name + ".npy"), finite_frame(H, W, LS, 600 + 10 * k).numpy())
        np.save(os.path.join(root, mode, "gt", name + ".npy"), _gt(H, W, 700 + k))
    d = DenoiseDirectory(root, LS, "train", batch_size=LB, device=DEV, patch_size=P, use_llpm_buf=True)
    d.offline_preprocess(llpm=False, kpcn=False)
    return root


def _run(loader, seed):
    np.random.seed(seed)
    got = [{k: v.clone() for k, v in b.items()} for b in loader]
    torch.cuda.synchronize()
    return got


def _directory(root, base_model):
    from wcmc_amd.support.datasets import DenoiseDirectory
    return DenoiseDirectory(root, LS, "train", batch_size=LB, device=DEV, patch_size=P, use_llpm_buf=True, base_model=base_model)


def _check_augmented_against_plain(aug, plain, codes, base_model):
    """Batch by batch: the same origins (the per-pixel keys of patch b are T_t[b] of the plain loader's patch b, which pins the window)
    and the loader's reported codes."""
    assert len(aug) == len(plain) == len(codes) // LB
    for n, (a, p) in enumerate(zip(aug, plain)):
        assert set(a) == set(p)
        for b in range(LB):
            t = int(codes[n * LB + b])
            for k in p:
                if base_model == "kpcn" and k in ("kpcn_diffuse_in", "kpcn_specular_in"):
                    first = 0 if k == "kpcn_diffuse_in" else 10                    # diffuse_in: record channels 0:10, 20:44
                    chans = [c for c in PER_PIXEL if c >= first and not (k == "kpcn_diffuse_in" and 10 <= c < 20)]
                    rows = [c - first if (k == "kpcn_specular_in" or c < 10) else c - 10 for c in chans] + [34]
                    assert torch.equal(a[k][b][rows], T(p[k][b][rows], t, (-2, -1))), (n, b, t, k)
                else:
                    assert torch.equal(a[k][b], T(p[k][b], t, (-2, -1))), (n, b, t, k)


@pytest.mark.parametrize("base_model", ["kpcn", "sbmc", "lbmc"])
def test_loader_with_augment_draws_the_same_origins_and_transforms_each_patch(loader_dir, base_model):
    from wcmc_amd.support.loader import PatchLoader
    d = _directory(loader_dir, base_model)
    mk = lambda **kw: PatchLoader(d.reader, range(2), DEV, batch_size=LB, patch_size=P, use_llpm=True, patches_per_image=PPI,  # noqa: E731
                                  staged_hook=d.staged_hook, base_model=base_model, **kw)
    plain, loader = _run(mk(), 31), mk(augment=True, augment_seed=5)
    after_plain = np.random.get_state()
    aug = _run(loader, 31)
    after_aug = np.random.get_state()
    # the process-wide stream ends where the plain run left it: the codes are not drawn from it
    assert np.array_equal(after_plain[1], after_aug[1]) and after_plain[2:] == after_aug[2:]
    codes = np.concatenate([loader.patch_transforms(i, epoch=0) for i in range(2)])
    assert codes.shape == (2 * PPI,) and len(set(codes.tolist())) > 2
    _check_augmented_against_plain(aug, plain, codes, base_model)
    # a second pass over the same loader draws other codes (the pass is part of the key), another seed too
    assert loader.epoch == 0
    second = _run(loader, 31)
    assert loader.epoch == 1
    codes2 = np.concatenate([loader.patch_transforms(i, epoch=1) for i in range(2)])
    assert not np.array_equal(codes, codes2)
    _check_augmented_against_plain(second, plain, codes2, base_model)
    assert not np.array_equal(codes, np.concatenate([mk(augment=True, augment_seed=6).patch_transforms(i, epoch=0) for i in range(2)]))


@pytest.mark.parametrize("base_model", ["kpcn", "sbmc"])
def test_loader_with_augment_over_sample_counts(loader_dir, base_model):
    from wcmc_amd.support.loader import PatchLoader, multi_count_schedule
    d = _directory(loader_dir, base_model)
    counts = (2, 3)
    mk = lambda **kw: PatchLoader(d.reader, range(2), DEV, batch_size=LB, patch_size=P, use_llpm=True, patches_per_image=PPI,  # noqa: E731
                                  staged_hook=d.staged_hook, base_model=base_model, counts=counts, window=2, **kw)
    plain, loader = _run(mk(), 8), mk(augment=True, augment_seed=1)
    aug = _run(loader, 8)
    sched = multi_count_schedule(2, counts, 2)
    # a batch never mixes sample counts: each has the count the schedule names
    assert [b["paths"].shape[1] for b in aug] == [s for _, s in sched for _ in range(PPI // LB)]
    codes = np.concatenate([loader.patch_transforms(i, epoch=0, spp=s) for i, s in sched])
    _check_augmented_against_plain(aug, plain, codes, base_model)


@pytest.mark.parametrize("launcher", ["train_kpcn", "train_sbmc", "train_lbmc"])
def test_launchers_hand_the_flags_to_the_training_loader_only(loader_dir, launcher):
    import importlib
    from wcmc_amd import train_kpcn as tk
    from wcmc_amd.support.loader import PatchLoader
    mod = importlib.import_module("wcmc_amd." + launcher)
    argv = ["--from_data_dir", "--data_dir", loader_dir, "--num_samples", str(LS), "-b", str(LB), "--patch_size", str(P),
            "--patches_per_image", str(PPI), "--use_llpm_buf", "--desc", "augment"]
    if launcher != "train_kpcn":
        argv += ["--denoiser", "json:dumps"]                                                  # (resolved, never called here)
    check = tk.check_args if launcher == "train_kpcn" else importlib.import_module("wcmc_amd.train_sbmc").check_args
    for extra, want in (([], (False, 0)), (["--augment"], (True, 0)), (["--augment", "--augment_seed", "4"], (True, 4))):
        args = tk.parse_args(argv + extra, mod.build_parser())
        check(args)
        _, loaders = mod.init_data(args, torch.device(DEV))
        train, val = loaders["train"], loaders["val"]
        assert isinstance(train, PatchLoader) and (train.augment, train.augment_seed) == want
        assert not isinstance(val, PatchLoader) and not getattr(val, "augment", False)      # validation never augments
    # the loader the launcher built draws transformed patches: its first batch is T_t of the un-augmented launcher's
    np.random.seed(3)
    aug = {k: v.clone() for k, v in next(iter(train)).items()}
    codes = train.patch_transforms(train.stager.indices[0], epoch=0)[:LB]
    args = tk.parse_args(argv, mod.build_parser())
    check(args)
    np.random.seed(3)
    plain = {k: v.clone() for k, v in next(iter(mod.init_data(args, torch.device(DEV))[1]["train"])).items()}
    torch.cuda.synchronize()
    key = "target_total" if launcher == "train_kpcn" else "target_image"
    assert len(set(codes.tolist())) > 1
    for b in range(LB):
        assert torch.equal(aug[key][b], T(plain[key][b], int(codes[b]), (-2, -1))), (launcher, b)
