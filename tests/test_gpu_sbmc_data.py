"""GPU tests of the data step of the sample-based interfaces (``wcmc_amd/csrc/sbmc_data.hip`` and the layers above it) against
goldens of the reference's ``DenoiseDataset`` (``tests/golden/sbmc_data.npz``, written by ``tests/golden/make_golden_sbmc.py``).

Bars: everything ``_preprocess_sbmc`` copies, clamps or derives from bits is compared bit for bit; its log groups (log total, log
specular, log probabilities) at rtol 2e-6 / atol 1e-7 -- the bar ``test_gpu_preprocess.py`` holds ``_preprocess_llpm`` to: device
``logf`` against numpy's libm, an ulp or two (measured on one MI355X: 3.0e-8 absolute, 2.5e-7 relative at the most).  The assembly only copies: bit for bit.  Each comparison prints its measured error
before it asserts (run with -s).
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for _p in (GOLDEN, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import make_golden_dataset as mgd  # noqa: E402
import make_golden_sbmc as mgs  # noqa: E402

DEV = "cuda:0"
RTOL, ATOL = 2e-6, 1e-7
S_LOG, P_LOG = slice(3, 9), slice(0, 24)                 # the log groups of sbmc_s / sbmc_p


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "sbmc_data.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _same_bits(a, b):
    a, b = _np(a), _np(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _check_buffers(what, got_s, got_p, want_s, want_p):
    """Exact channels bit for bit, log groups at RTOL / ATOL; prints the worst log error first."""
    got_s, got_p = _np(got_s), _np(got_p)
    for name, got, want, log in (("sbmc_s", got_s, want_s, S_LOG), ("sbmc_p", got_p, want_p, P_LOG)):
        exact = np.ones(got.shape[-1], dtype=bool)
        exact[log] = False
        err = np.abs(got[..., log].astype(np.float64) - want[..., log])
        rel = float((err / np.maximum(np.abs(want[..., log]), 1e-30)).max())
        print("%s %s: log groups max abs error %.3e, max rel error %.3e (bar rtol %.0e atol %.0e)" % (what, name, err.max(), rel, RTOL, ATOL))
        np.testing.assert_array_equal(got[..., exact], want[..., exact], err_msg="%s %s copied / clamped / tag channels" % (what, name))
        np.testing.assert_allclose(got[..., log], want[..., log], rtol=RTOL, atol=ATOL, err_msg="%s %s log groups" % (what, name))


# ------------------------------------------------------------------------------------------------- 1. preprocess_sbmc
@pytest.mark.parametrize("name", list(mgs.PRE))
def test_preprocess_sbmc_matches_the_reference(gold, name):
    from wcmc_amd import ops
    from wcmc_amd.support.datasets import DenoisePreprocessor
    h, w, s, seed = (int(v) for v in gold["pre/%s/params" % name])
    assert (h, w, s, seed) == mgs.PRE[name]
    x = mgs.sbmc_raw(h, w, s, seed)
    assert mgs.crc(x) == int(gold["pre/%s/raw_crc" % name]), "the regenerated raw samples differ from the golden's"
    assert float(x[..., 24:48].min()) < 0 and float(np.abs(x[..., 48:60]).max()) > 1 and set(np.unique(x[..., 60:66])) == set(range(32))
    got_s, got_p = ops.preprocess_sbmc(_dev(x))
    assert got_s.shape == (h, w, s, 27) and got_p.shape == (h, w, s, 66) and got_s.dtype == got_p.dtype == torch.float32
    _check_buffers(name, got_s, got_p, gold["pre/%s/sbmc_s" % name], gold["pre/%s/sbmc_p" % name])
    pair = DenoisePreprocessor()._preprocess_sbmc(_dev(x))
    assert _same_bits(pair[0], got_s) and _same_bits(pair[1], got_p)


def test_a_bounce_code_outside_int16_has_no_tags(gold):
    """wcmc_hip.h: a code with no int16 counterpart (the 1e38 of sanitising) gives all five flags 0.  The golden records whether
    the reference's astype(np.int16) did the same on the machine that wrote it (the cast is undefined there)."""
    from wcmc_amd import ops
    x = mgs.sbmc_raw(2, 3, 2, 914)
    x[..., 60:63] = np.float32(1.0e+38)
    x[..., 63], x[..., 64], x[..., 65] = np.float32(-1.0e+38), np.float32(40000.0), np.float32(-3.0)
    _, p = ops.preprocess_sbmc(_dev(x))
    tags = p.cpu().numpy()[..., 36:].reshape(2, 3, 2, 5, 6)                   # plane-major: [bit][bounce]
    assert not tags[..., :5].any()
    assert (tags[..., 5] == np.array([1, 0, 1, 1, 1], dtype=np.float32)).all()   # int16(-3) = ...11111101
    print("reference on the golden's machine maps 1e38 to no tags:", bool(int(gold["pre/int16_overflow"])))


# ------------------------------------------------------------------------------------------------- 2. tiled == generic
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 * 256 + 3])
def test_tiled_form_equals_generic_form_bitwise(n):
    from wcmc_amd import ops
    x = _dev(mgs.sbmc_raw(1, n, 1, 7000 + n))
    ts, tp = ops.preprocess_sbmc(x, tiled=True)
    gs, gp = ops.preprocess_sbmc(x, tiled=False)
    a_s, a_p = ops.preprocess_sbmc(x)
    assert _same_bits(ts, gs) and _same_bits(tp, gp) and _same_bits(a_s, gs) and _same_bits(a_p, gp)
    assert bool(torch.isfinite(ts).all()) and bool(torch.isfinite(tp).all())


def test_preprocess_sbmc_refuses_what_it_cannot_take():
    from wcmc_amd import ops
    x = _dev(mgs.sbmc_raw(2, 6, 2, 7100))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.preprocess_sbmc(x[:, ::2])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.preprocess_sbmc(x.cpu())
    odd = torch.cat([x, x[..., :1]], dim=3).contiguous()                      # 105 channels: records not 16-byte aligned
    with pytest.raises(RuntimeError, match="tiled form"):
        ops.preprocess_sbmc(odd, tiled=True)
    gs, gp = ops.preprocess_sbmc(odd)                                          # (the generic form takes them)
    ws, wp = ops.preprocess_sbmc(x, tiled=False)
    assert _same_bits(gs, ws) and _same_bits(gp, wp)
    with pytest.raises(RuntimeError, match="channels"):
        ops.preprocess_sbmc(x[..., :64].contiguous())


# ------------------------------------------------------------------------------------------------- 3. assembly
def _scene_buffers(gold, tag, scene, windows, patch):
    """Device buffers of the golden scene: the device's own preprocessing of the regenerated raw, with the windows of the golden
    items (all buffers on) written over it bit for bit -- after checking that they agree within the bars of test 1."""
    from wcmc_amd import ops
    h, w, s, seed, gseed = scene
    assert [int(v) for v in gold["%s/params" % tag]] == [h, w, s, seed, gseed, patch]
    raw, gt = mgs.scene_raw(h, w, s, seed), mgd.test_gt(h, w, gseed)
    assert mgs.crc(raw) == int(gold["%s/raw_crc" % tag])
    d_raw = _dev(raw)
    ss, sp = (t.cpu().numpy() for t in ops.preprocess_sbmc(d_raw))
    ll = ops.preprocess_llpm(d_raw).cpu().numpy()
    for i, (r, c) in windows.items():
        it = {k: gold["%s/g1_p1_l1/%d/%s" % (tag, i, k)] for k in ("radiance", "features", "paths")}
        win = (slice(r, r + patch), slice(c, c + patch))
        to_hw = lambda a: a.transpose(2, 3, 0, 1)                                                    # noqa: E731
        want_s = np.concatenate([to_hw(it["radiance"]), to_hw(it["features"][:, :24])], axis=3)
        want_p = to_hw(it["features"][:, 24:90])
        want_l = np.concatenate([to_hw(it["features"][:, 90:91]), to_hw(it["paths"])], axis=3)
        _check_buffers("%s window %d" % (tag, i), ss[win], sp[win], want_s, want_p)
        np.testing.assert_allclose(ll[win], want_l, rtol=RTOL, atol=ATOL)
        ss[win], sp[win], ll[win] = want_s, want_p, want_l
    return _dev(ss), _dev(sp), _dev(ll), _dev(gt)


@pytest.fixture(scope="module")
def scene(gold):
    return _scene_buffers(gold, "item", mgs.SCENE, mgs.SCENE_WINDOWS, mgs.SCENE_PATCH)


@pytest.mark.parametrize("combo", list(mgs.COMBOS))
def test_assembly_matches_the_reference_items(gold, scene, combo):
    """P = 16, S = 4; origins (0, 0), (0, 16) and the last whole window (16, 32) in one batch."""
    from wcmc_amd import ops
    from wcmc_amd.support.datasets import SamplePatchBatcher, sample_flags
    ss, sp, ll, gt = scene
    bm, g, p, l = mgs.COMBOS[combo]
    base, g, p = sample_flags(bm, g, p)
    assert [int(base == "sbmc"), int(g), int(p), int(l)] == [int(v) for v in gold["flags/%s" % combo]]
    origins = np.array(list(mgs.SCENE_WINDOWS.values()), dtype=np.int32)
    out = ops.assemble_sample_patches(ss, sp if p else None, ll if l else None, gt, origins, mgs.SCENE_PATCH, g, p)
    via = SamplePatchBatcher(mgs.SCENE_PATCH, 8, g, p).batch(ss, sp, ll if l else None, gt, torch.as_tensor(origins).to(DEV))
    keys = {k.split("/")[-1] for k in gold.files if k.startswith("item/%s/0/" % combo)}
    assert set(out) == keys == set(via) and ("paths" in keys) == l
    assert out["features"].shape[2] == ops.sample_feature_size(g, p, l)
    for n, i in enumerate(mgs.SCENE_WINDOWS):
        for k in keys:
            want = gold["item/%s/%d/%s" % (combo, i, k)]
            assert _same_bits(out[k][n], want), (combo, i, k, float(np.abs(_np(out[k][n]) - want).max()))
            assert _same_bits(via[k][n], want)
    base_ptr = out["radiance"].untyped_storage().data_ptr()
    assert all(v.untyped_storage().data_ptr() == base_ptr for v in out.values()), "one allocation"


def test_assembly_at_odd_sizes_matches_the_reference_items(gold):
    """P = 8, S = 3, W = 21: a window that starts inside a staging chunk, sample and pixel chunks that are not full."""
    from wcmc_amd import ops
    ss, sp, ll, gt = _scene_buffers(gold, "item8", mgs.SCENE8, mgs.SCENE8_WINDOWS, mgs.SCENE8_PATCH)
    assert ss.shape == (19, 21, 3, 27)
    origins = np.array(list(mgs.SCENE8_WINDOWS.values()), dtype=np.int32)
    out = ops.assemble_sample_patches(ss, sp, ll, gt, origins, 8)
    for n, i in enumerate(mgs.SCENE8_WINDOWS):
        for k in ("radiance", "features", "paths", "target_image"):
            assert _same_bits(out[k][n], gold["item8/g1_p1_l1/%d/%s" % (i, k)]), (i, k)
    # every other origin of the image, against the slices the reference takes
    allo = np.array([(r, c) for r in (0, 5, 11) for c in (0, 1, 7, 13)], dtype=np.int32)
    out = ops.assemble_sample_patches(ss, sp, ll, gt, allo, 8, True, False)
    for n, (r, c) in enumerate(allo):
        assert _same_bits(out["radiance"][n], ss[r:r + 8, c:c + 8, :, :3].permute(2, 3, 0, 1).contiguous())
        assert _same_bits(out["features"][n, :, :24], ss[r:r + 8, c:c + 8, :, 3:].permute(2, 3, 0, 1).contiguous())
        assert _same_bits(out["features"][n, :, 24], ll[r:r + 8, c:c + 8, :, 0].permute(2, 0, 1).contiguous())
        assert _same_bits(out["paths"][n], ll[r:r + 8, c:c + 8, :, 1:].permute(2, 3, 0, 1).contiguous())
        assert _same_bits(out["target_image"][n], gt[r:r + 8, c:c + 8, :3].permute(2, 0, 1).contiguous())


def test_an_origin_outside_the_image_is_a_value_error(scene):
    from wcmc_amd import ops
    from wcmc_amd.support.datasets import SamplePatchBatcher
    ss, sp, ll, gt = scene
    for bad in ([(25, 0)], [(0, 33)], [(-1, 0)], [(0, 0), (24, 32), (24, 33)]):
        with pytest.raises(ValueError, match="outside"):
            ops.assemble_sample_patches(ss, sp, ll, gt, np.array(bad, dtype=np.int32), 16)
        with pytest.raises(ValueError, match="outside"):
            SamplePatchBatcher(16).batch(ss, sp, ll, gt, torch.tensor(bad, dtype=torch.int32, device=DEV))
    ops.assemble_sample_patches(ss, sp, ll, gt, np.array([(24, 32)], dtype=np.int32), 16)        # the last window that fits
    with pytest.raises(ValueError, match="does not fit"):
        ops.assemble_sample_patches(ss, sp, ll, gt, np.array([(0, 0)], dtype=np.int32), 41)


# ------------------------------------------------------------------------------------------------- directories
def _write_scene(root, mode, name, h, w, s, seed):
    for d in ("gt", "input"):
        os.makedirs(os.path.join(root, mode, d), exist_ok=True)
    raw, gt = mgs.sbmc_raw(h, w, s, seed), mgd.test_gt(h, w, seed + 1)
    gt[..., 0:3] += 0.25
    np.save(os.path.join(root, mode, "input", name + ".npy"), raw)
    np.save(os.path.join(root, mode, "gt", name + ".npy"), gt)
    return raw, gt


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    """Two training scenes and one validation scene of 48 x 48 at 4 spp."""
    root = str(tmp_path_factory.mktemp("sbmc_data"))
    _write_scene(root, "train", "room", 48, 48, 4, 8100)
    _write_scene(root, "train", "car", 48, 48, 4, 8200)
    _write_scene(root, "val", "den", 48, 48, 4, 8300)
    return root


# ------------------------------------------------------------------------------------------------- 4. the loader
def test_patch_loader_for_sbmc_equals_the_direct_path_and_kpcn_is_unchanged(data_dir):
    from wcmc_amd.support.datasets import DenoiseDirectory, DenoisePreprocessor, PatchBatcher, SamplePatchBatcher, sanitized
    from wcmc_amd.support.loader import ImageStager, PatchLoader
    pre = DenoisePreprocessor()
    d = DenoiseDirectory(data_dir, 4, "train", batch_size=2, device=DEV, patch_size=16, use_llpm_buf=True, base_model="sbmc",
                         use_sbmc_buf=True)
    loader = PatchLoader(d.reader, [0, 1], DEV, batch_size=2, patch_size=16, use_llpm=True, patches_per_image=4,
                         staged_hook=d.staged_hook, base_model="sbmc")
    assert len(loader) == 4
    np.random.seed(1234)
    got = [{k: v.clone() for k, v in b.items()} for b in loader]
    torch.cuda.synchronize()

    def frames(i):
        p = d.paths(i)
        return _dev(sanitized(np.load(p["in"])[:, :, :4])), _dev(sanitized(np.load(p["gt"]))), np.load(p["prob"])

    np.random.seed(1234)
    batcher, want = SamplePatchBatcher(16, 2), []
    batcher.patches_per_image = 4
    for i in (0, 1):
        x, g, prob = frames(i)                                               # (the loader's hook wrote the probability map)
        ss, sp = pre._preprocess_sbmc(x)
        o = batcher.sample_origins(prob)
        want += [batcher.batch(ss, sp, pre._preprocess_llpm(x), g, o[k:k + 2]) for k in range(0, 4, 2)]
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert set(a) == set(b) == {"radiance", "features", "paths", "target_image"}
        assert a["features"].shape == (2, 4, 91, 16, 16) and all(_same_bits(a[k], b[k]) for k in a)
    # the stager's tuple for the sample-based models
    first = next(iter(ImageStager(d.reader, [0], DEV, staged_hook=d.staged_hook, base_model="lbmc")))
    assert len(first) == 5 and first[0].shape == (48, 48, 4, 27) and first[1].shape == (48, 48, 4, 66) and first[2].shape == (48, 48, 4, 37)
    # a KPCN loader built with default arguments returns what PatchBatcher.batch returns
    dk = DenoiseDirectory(data_dir, 4, "train", batch_size=2, device=DEV, patch_size=16, use_llpm_buf=True)
    assert dk.base_model == "kpcn" and dk.dncnn_in_size == 39
    np.random.seed(99)
    got = [{k: v.clone() for k, v in b.items()}
           for b in PatchLoader(dk.reader, [0, 1], DEV, batch_size=2, patch_size=16, patches_per_image=2, staged_hook=dk.staged_hook)]
    torch.cuda.synchronize()
    np.random.seed(99)
    kb = PatchBatcher(16, 2)
    kb.patches_per_image = 2
    assert len(got) == 2
    for i in (0, 1):
        x, g, prob = frames(i)
        want = kb.batch(pre._preprocess_kpcn(x), pre._preprocess_llpm(x), g, kb.sample_origins(prob))
        assert set(got[i]) == set(want) and "kpcn_diffuse_in" in want and all(_same_bits(got[i][k], want[k]) for k in want)
    st = next(iter(ImageStager(dk.reader, [0], DEV, staged_hook=dk.staged_hook)))
    assert len(st) == 4 and st[0].shape == (48, 48, 44)


def test_grid_batches_of_a_sample_based_directory(data_dir):
    from wcmc_amd.support.datasets import DenoiseDirectory
    va = DenoiseDirectory(data_dir, 4, "val", 4, "grid", use_llpm_buf=True, device=DEV, patch_size=16, base_model="lbmc")
    batches = list(va.grid_batches())
    assert len(batches) == va.num_grid_batches() == 3 and batches[0]["features"].shape == (4, 4, 25, 16, 16)
    assert batches[2]["radiance"].shape == (1, 4, 3, 16, 16) and batches[0]["paths"].shape == (4, 4, 36, 16, 16)


# ------------------------------------------------------------------------------------------------- 5. the offline writer
def test_offline_preprocess_writes_the_sbmc_buffers(gold, tmp_path):
    from wcmc_amd import ops
    from wcmc_amd.support.datasets import DenoiseDirectory
    h, w, s, seed, gseed = mgs.SCENE
    raw, gt = mgs.scene_raw(h, w, s, seed), mgd.test_gt(h, w, gseed)
    root = str(tmp_path)
    for sub, arr in (("gt", gt), ("input", raw)):
        os.makedirs(os.path.join(root, "train", sub))
        np.save(os.path.join(root, "train", sub, "scene.npy"), arr)
    d = DenoiseDirectory(root, s, "train", device=DEV, patch_size=mgs.SCENE_PATCH, use_llpm_buf=True, base_model="sbmc")
    report = d.offline_preprocess(llpm=True, kpcn=False, sbmc=True)
    inp = os.path.join(root, "train", "input")
    assert sorted(os.listdir(inp)) == [str(f) for f in gold["item/files"]]                # as the golden script's run named them
    assert sorted(os.path.basename(f) for f in report[0][1]) == ["scene_llpm.npy", "scene_prob_imp.npy", "scene_sbmc_p.npy", "scene_sbmc_s.npy"]
    fs, fp = np.load(os.path.join(inp, "scene_sbmc_s.npy")), np.load(os.path.join(inp, "scene_sbmc_p.npy"))
    ds, dp = ops.preprocess_sbmc(_dev(raw))
    assert _same_bits(fs, ds) and _same_bits(fp, dp)
    for i, (r, c) in mgs.SCENE_WINDOWS.items():                                               # ... and to the golden
        it = {k: gold["item/g1_p1_l1/%d/%s" % (i, k)] for k in ("radiance", "features")}
        want_s = np.concatenate([it["radiance"], it["features"][:, :24]], axis=1).transpose(2, 3, 0, 1)
        _check_buffers("file window %d" % i, fs[r:r + 16, c:c + 16], fp[r:r + 16, c:c + 16], want_s, it["features"][:, 24:90].transpose(2, 3, 0, 1))
    assert all(e[1] == [] for e in d.offline_preprocess(llpm=True, kpcn=False, sbmc=True)), "a second call writes nothing"
    # test mode (the reference raises NameError there) and continuation files (an addition)
    for sub, arr in (("gt", gt), ("input", raw[:, :, :2])):
        os.makedirs(os.path.join(root, "test", sub))
        np.save(os.path.join(root, "test", sub, "scene.npy"), arr)
    np.save(os.path.join(root, "test", "input", "scene_1.npy"), raw[:, :, 2:])
    t = DenoiseDirectory(root, 2, "test", device=DEV, base_model="sbmc")
    t.offline_preprocess(llpm=False, kpcn=False, sbmc=True)
    tin = os.path.join(root, "test", "input")
    assert sorted(os.listdir(tin)) == ["scene.npy", "scene_1.npy", "scene_sbmc_p.npy", "scene_sbmc_p_1.npy", "scene_sbmc_s.npy", "scene_sbmc_s_1.npy"]
    assert _same_bits(np.load(os.path.join(tin, "scene_sbmc_s.npy")), ds[:, :, :2].contiguous())
    assert _same_bits(np.load(os.path.join(tin, "scene_sbmc_p_1.npy")), dp[:, :, 2:].contiguous())


def test_sample_full_image_dataset_tile_matches_the_reference(gold, tmp_path):
    """``FullImageDataset('sbmc')`` of the reference over files it wrote itself: here the same files come from the golden tile."""
    from wcmc_amd.support.datasets import SampleFullImageDataset
    h, w, s, seed, gseed = (int(v) for v in gold["full/params"])
    it = {k: gold["full/item/%s" % k] for k in ("radiance", "features", "paths", "target_image")}
    to_hw = lambda a: a.transpose(2, 3, 0, 1)                                                        # noqa: E731
    inp = tmp_path / "KPCN" / "test" / "input"
    for sub in (("KPCN", "test", "input"), ("KPCN", "test", "gt"), ("SBMC", "test", "input"), ("LLPM", "test", "input")):
        os.makedirs(tmp_path.joinpath(*sub))
    np.save(tmp_path / "SBMC" / "test" / "input" / "scene_sbmc_s.npy", np.concatenate([to_hw(it["radiance"]), to_hw(it["features"][:, :24])], axis=3))
    np.save(tmp_path / "SBMC" / "test" / "input" / "scene_sbmc_p.npy", to_hw(it["features"][:, 24:90]))
    np.save(tmp_path / "LLPM" / "test" / "input" / "scene_llpm.npy", np.concatenate([to_hw(it["features"][:, 90:91]), to_hw(it["paths"])], axis=3))
    gt = mgd.test_gt(h, w, gseed)
    assert np.array_equal(gt[..., :3].transpose(2, 0, 1), it["target_image"])
    np.save(tmp_path / "KPCN" / "test" / "gt" / "scene.npy", gt)
    ds = SampleFullImageDataset(str(inp / "scene.npy"), s, "sbmc", True, True, True, 3, device=DEV)
    assert [ds.dncnn_in_size, ds.pnet_in_size] == [int(v) for v in gold["full/sizes"]] and len(ds) == 1
    tiles = list(ds)
    batch, coords = tiles[0][0], [c[0] for c in tiles[0][1:]]
    assert coords == [int(v) for v in gold["full/coords"]]
    assert all(_same_bits(batch[k][0], it[k]) for k in it)
    assert _same_bits(ds.has_hit, gold["full/has_hit"]) and 0.0 < float(ds.has_hit.mean()) < 1.0
    lb = SampleFullImageDataset(str(inp / "scene.npy"), s, "lbmc", False, True, False, 3, device=DEV)
    assert (lb.base_model, lb.use_g_buf, lb.use_sbmc_buf) == ("sbmc", True, False) and lb.sbmc_p is None
    assert _same_bits(next(iter(lb))[0]["features"][0], it["features"][:, :24])


# ------------------------------------------------------------------------------------------------- 6. the launchers
@pytest.mark.parametrize("launcher", ["train_sbmc", "train_lbmc"])
def test_launcher_trains_an_epoch_from_a_data_dir(data_dir, tmp_path, monkeypatch, launcher):
    import importlib
    from wcmc_amd import train_kpcn as tk
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.interfaces import SBMCInterface
    mod = importlib.import_module("wcmc_amd." + launcher)
    seen, inner_train, inner_summary = {}, tk.train, SBMCInterface.get_epoch_summary
    vec = lambda itf: torch.cat([p.detach().reshape(-1) for m in itf.models.values() for p in m.parameters()]).clone()   # noqa: E731

    def spy_train(interfaces, loaders, params, args):
        seen["batches"] = (len(loaders["train"]), len(loaders["val"]))
        before = vec(interfaces[0])
        inner_train(interfaces, loaders, params, args)
        seen["delta"], seen["params"] = float((vec(interfaces[0]) - before).abs().max()), params

    def spy_summary(self, mode, norm):
        if mode == "train":
            seen["losses"] = {k: float(v) for k, v in self.m_losses.items()}
        return inner_summary(self, mode, norm)

    monkeypatch.setattr(tk, "train", spy_train)
    monkeypatch.setattr(SBMCInterface, "get_epoch_summary", spy_summary)
    save, name = str(tmp_path / "weights"), launcher.upper() + "_dir"
    argv = ["--from_data_dir", "--data_dir", data_dir, "--num_samples", "4", "--single_gpu", "--batch_size", "2", "--patch_size", "16",
            "--patches_per_image", "2", "--num_epoch", "1", "--val_epoch", "1", "--model_name", name, "--desc", "directory loop",
            "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--w_manif", "0.1", "--lr_dncnn", "1e-3", "--lr_pnet", "1e-3",
            "--denoiser", "standins:SampleDenoiserStandIn", "--save", save]
    interfaces = mod.main(argv)
    itf = interfaces[0]
    assert str(itf) == ("SBMCInterface" if launcher == "train_sbmc" else "LBMCInterface")
    assert seen["batches"] == (2, 3)                                    # 2 images x 2 patches / 2; 9 whole grid windows / 4
    assert np.isfinite(seen["losses"]["m_l_total"]) and seen["losses"]["m_l_total"] > 0 and np.isfinite(seen["losses"]["m_l_manif"])
    assert seen["delta"] > 0.0 and bool(torch.isfinite(vec(itf)).all())
    assert type(itf.loss_funcs["l_recon"]).__name__ == ("TonemappedRelativeMSE" if launcher == "train_sbmc" else "ClampedSMAPE")
    assert ("sched_dncnn" in seen["params"]) == (launcher == "train_lbmc")
    assert os.path.isfile(os.path.join(save, "latest_%s.pth" % name))
    ck = ckpt.load_checkpoint(os.path.join(save, name + ".pth"))
    assert ck["start_epoch"] == 1 and np.isfinite(ck["best_err"]) and set(itf.models) == {"dncnn", "backbone"}
    from wcmc_amd.train_sbmc import build_models
    fresh = build_models({"dncnn_in_size": 26, "pnet_in_size": 36, "pnet_out_size": 0}, ck["args"], 3, True, "test")
    ckpt.restore_models(ck, fresh)
    for k in fresh:
        for (n, a), (_, b) in zip(fresh[k].state_dict().items(), itf.models[k].state_dict().items()):
            assert torch.equal(a, b.cpu()), (k, n)


@pytest.mark.parametrize("launcher", ["train_sbmc", "train_lbmc"])
def test_a_bad_denoiser_factory_is_a_named_error(data_dir, tmp_path, launcher):
    import importlib
    from wcmc_amd.train_sbmc import DenoiserFactoryError
    mod = importlib.import_module("wcmc_amd." + launcher)
    base = ["--from_data_dir", "--data_dir", data_dir, "--desc", "x", "--save", str(tmp_path / "w")]
    for extra in ([], ["--denoiser", "no_such_package_xyz.models:make"], ["--denoiser", "standins:no_such_factory"],
                  ["--denoiser", "standins"]):
        with pytest.raises(DenoiserFactoryError, match="--denoiser"):
            mod.main(base + extra)
    assert not os.path.exists(str(tmp_path / "w"))
