"""GPU tests of training over the sample counts 2..spp from one staged frame (``wcmc_amd/csrc/multi_spp.hip``, DESIGN.md section
14): the prefix statistics against the numpy oracle and the single-count kernel, patch assembly from a sample prefix against the
plain entry points on the sliced buffers, the loader's schedule, and the three launchers with ``--multi_spp``.

Bars of the statistics: rtol 5e-5, atol 2e-6 -- this project's bars for ``preprocess_kpcn`` against the oracle
(``tests/test_gpu_preprocess.py``).  The prefix pass sums in sample order, the single-count kernel in a shuffle tree for a count that
is a power of two: the two are held to the same bars, not to equality.  Assembly copies: ``torch.equal``.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden as mg  # noqa: E402
import make_golden_dataset as mgd  # noqa: E402

DEV = "cuda:0"
RTOL, ATOL = 5e-5, 2e-6
DEPTH = 30 + 6 * 7                                    # raw channel of the depth (datasets.py:223-267 at MAX_DEPTH 5)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _close(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def _check_slabs(raw, s_lo, s_hi, x=None, what=""):
    """Every slab of the prefix pass against the oracle on the sliced numpy frame and against the single-count op on the
    contiguous device slice."""
    from oracle import datasets as od
    from wcmc_amd import ops
    x = _dev(raw) if x is None else x
    out = ops.preprocess_kpcn_prefix(x, s_lo, s_hi)
    assert out.shape == (s_hi - s_lo + 1,) + raw.shape[:2] + (44,) and out.dtype == torch.float32 and out.is_contiguous()
    for s in range(s_lo, s_hi + 1):
        _close(out[s - s_lo], od.preprocess_kpcn(np.ascontiguousarray(raw[:, :, :s])), "%s oracle, prefix of %d" % (what, s))
        _close(out[s - s_lo], ops.preprocess_kpcn(x[:, :, :s].contiguous()), "%s single-count op, prefix of %d" % (what, s))
    return out


# ------------------------------------------------------------------------------------------------- 1. prefix statistics
@pytest.mark.parametrize("S,s_lo,s_hi,seed", [(8, 2, 8, 91), (5, 1, 5, 92), (8, 8, 8, 93), (8, 3, 6, 94)])
def test_prefix_statistics_match_the_oracle_and_the_single_count_kernel(S, s_lo, s_hi, seed):
    """21 x 19 pixels: 399 is no multiple of the 32 (S = 8) or 51 (S = 5) pixels of a block's tile, and more than one block runs."""
    out = _check_slabs(mg.raw_samples(21, 19, S, seed), s_lo, s_hi, what="S=%d %d..%d" % (S, s_lo, s_hi))
    assert float(out[..., 30].max()) <= 1.0 and float(out[..., 30].min()) >= 0.0          # normalised, clipped depth
    assert torch.equal(out[:, :, 0, 4:7], torch.zeros_like(out[:, :, 0, 4:7]))            # zero first column of d/dx in every slab


def test_prefix_statistics_of_a_view_off_16_byte_alignment():
    """The scalar-load path: the same frame at a storage offset of one float."""
    from wcmc_amd import ops
    raw = mg.raw_samples(21, 19, 8, 95)
    flat = torch.empty(raw.size + 1, device=DEV, dtype=torch.float32)
    flat[1:].copy_(_dev(raw).reshape(-1))
    x = flat[1:].view(raw.shape)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    out = _check_slabs(raw, 2, 8, x=x, what="offset view")
    _close(out, ops.preprocess_kpcn_prefix(_dev(raw), 2, 8), "scalar path against the vector path")


def test_prefix_statistics_where_the_depth_maximum_is_zero(golden_dir):
    raw = np.load(os.path.join(golden_dir, "preprocess.npz"))["zero_depth/raw"]
    assert float(raw[..., DEPTH].max()) == 0.0
    S = raw.shape[2]
    out = _check_slabs(raw, 1, S, what="zero depth")
    assert float(out[..., 30:34].abs().max()) == 0.0                                       # no scaling: 0 stays 0, not NaN


def test_every_count_has_its_own_depth_maximum():
    """One pixel is made the deepest of the frame from sample 2 on: the prefix of 2 still normalises by another pixel's mean depth,
    the prefix of 8 by this one's.  With one shared maximum slot one of the two slabs could not reach 1.0."""
    raw = mg.raw_samples(21, 19, 8, 96)
    d = raw[..., DEPTH]
    assert float(d.min()) > 0.0
    m2 = d[:, :, :2].mean(2)
    qy, qx = np.unravel_index(int(m2.argmin()), m2.shape)
    raw[qy, qx, 2:, DEPTH] *= 100.0 * float(d.max()) / float(raw[qy, qx, 2:, DEPTH].min())
    d = raw[..., DEPTH]
    a2, a8 = int(d[:, :, :2].mean(2).argmax()), int(d.mean(2).argmax())
    assert a8 == qy * 19 + qx and a2 != a8
    out = _check_slabs(raw, 2, 8, what="planted depth")
    assert float(out[0, :, :, 30].max()) == 1.0 and float(out[6, :, :, 30].max()) == 1.0
    assert int(out[0, :, :, 30].argmax()) == a2 and int(out[6, :, :, 30].argmax()) == a8


def test_prefix_op_rejects_bad_counts():
    from wcmc_amd import ops
    x = _dev(mg.raw_samples(4, 4, 4, 1))
    for lo, hi in ((0, 2), (3, 2), (2, 5)):
        with pytest.raises(ValueError, match="s_lo"):
            ops.preprocess_kpcn_prefix(x, lo, hi)


# ------------------------------------------------------------------------------------------------- 2. assembly from a prefix
H, W, P, S_TOTAL = 40, 37, 16, 8
ORIGINS = np.array([(0, 0), (H - P, W - P), (11, 5)], dtype=np.int32)


@pytest.fixture(scope="module")
def buffers():
    g = torch.Generator().manual_seed(7)
    r = lambda *shape: torch.rand(*shape, generator=g).to(DEV)                            # noqa: E731
    return {"kpcn": r(H, W, 44), "llpm": r(H, W, S_TOTAL, 37), "gt": r(H, W, 9) + 1.0, "sbmc_s": r(H, W, S_TOTAL, 27),
            "sbmc_p": r(H, W, S_TOTAL, 66), "origins": torch.from_numpy(ORIGINS).to(DEV)}


@pytest.mark.parametrize("s", [2, 3, 8])
@pytest.mark.parametrize("with_llpm", [True, False])
def test_kpcn_assembly_from_a_prefix_equals_the_plain_entry_point_on_the_slice(buffers, s, with_llpm):
    from wcmc_amd import ops
    b = buffers
    ll = b["llpm"] if with_llpm else None
    got = ops.assemble_kpcn_patches(b["kpcn"], ll, b["gt"], b["origins"], P, spp=s)
    want = ops.assemble_kpcn_patches(b["kpcn"], ll[:, :, :s].contiguous() if with_llpm else None, b["gt"], b["origins"], P)
    assert set(got) == set(want) and ("paths" in got) == with_llpm
    if with_llpm:
        assert got["paths"].shape == (3, s, 36, P, P)
    for k in want:
        assert torch.equal(got[k], want[k]), (s, k)


@pytest.mark.parametrize("s", [2, 3, 8])
@pytest.mark.parametrize("use_g_buf,use_sbmc_buf", [(True, True), (True, False), (False, True), (False, False)])
def test_sample_assembly_from_a_prefix_equals_the_plain_entry_point_on_the_slice(buffers, s, use_g_buf, use_sbmc_buf):
    from wcmc_amd import ops
    b = buffers
    cut = lambda t: t[:, :, :s].contiguous()                                              # noqa: E731
    for ll in (b["llpm"], None):
        got = ops.assemble_sample_patches(b["sbmc_s"], b["sbmc_p"], ll, b["gt"], b["origins"], P, use_g_buf, use_sbmc_buf, spp=s)
        want = ops.assemble_sample_patches(cut(b["sbmc_s"]), cut(b["sbmc_p"]), None if ll is None else cut(ll), b["gt"], b["origins"],
                                           P, use_g_buf, use_sbmc_buf)
        assert set(got) == set(want) and got["radiance"].shape == (3, s, 3, P, P)
        for k in want:
            assert torch.equal(got[k], want[k]), (s, k, ll is None)


def test_prefix_assembly_rejects_bad_arguments_through_the_abi(buffers):
    """Negative status + a message, no launch (include/wcmc_hip.h contract)."""
    from wcmc_amd import _lib
    L, b = _lib.lib(), buffers
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                         # noqa: E731
    null, out = ctypes.c_void_p(0), torch.empty(3 * 8 * 36 * P * P + 3 * 91 * 8 * P * P, device=DEV)
    o = ptr(out)

    def kpcn(s_total, s, paths):
        return L.wcmc_assemble_kpcn_patches(ptr(b["kpcn"]), ptr(b["llpm"]), ptr(b["gt"]), ptr(b["origins"]), null, 3, H, W, s_total, s,
                                            P, o, o, o, o, o, paths, o, o, o, null)

    def sample(s_total, s, paths):
        return L.wcmc_assemble_sample_patches(ptr(b["sbmc_s"]), ptr(b["sbmc_p"]), ptr(b["llpm"]), ptr(b["gt"]), ptr(b["origins"]), null,
                                              3, H, W, s_total, s, P, 1, 1, o, o, paths, o, null)

    for fn, name in ((kpcn, "assemble_kpcn_patches"), (sample, "assemble_sample_patches")):    # (a null table: the plain batch)
        for args, word in (((S_TOTAL, 0, o), "1 <= s <= S_total"), ((S_TOTAL, S_TOTAL + 1, o), "1 <= s <= S_total"),
                           ((0, 0, o), "1 <= s <= S_total"), ((S_TOTAL, 2, null), "without a paths output")):
            assert fn(*args) == -1, (name, args)                                          # WCMC_ERR_BAD_ARG
            msg = L.wcmc_last_error().decode()
            assert msg.startswith(name + ":") and word in msg, (name, args, msg)
    torch.cuda.synchronize()
    from wcmc_amd import ops
    with pytest.raises(ValueError, match="prefix"):
        ops.assemble_kpcn_patches(b["kpcn"], b["llpm"], b["gt"], b["origins"], P, spp=9)
    with pytest.raises(ValueError, match="prefix"):
        ops.assemble_sample_patches(b["sbmc_s"], b["sbmc_p"], b["llpm"], b["gt"], b["origins"], P, spp=0)


# ------------------------------------------------------------------------------------------------- 3. the loader
def _gt(h, w, seed):
    gt = mgd.test_gt(h, w, seed)
    gt[..., 0:3] += 0.25                               # total > diffuse: log(1 + total - diffuse) is defined
    return gt


def _write_scene(root, mode, name, h, w, s, seed):
    for d in ("gt", "input"):
        os.makedirs(os.path.join(root, mode, d), exist_ok=True)
    np.save(os.path.join(root, mode, "input", name + ".npy"), mg.raw_samples(h, w, s, seed))
    np.save(os.path.join(root, mode, "gt", name + ".npy"), _gt(h, w, seed + 1))


COUNTS, LP, LB, PPI = (2, 3, 4), 16, 4, 8
STAT_KEYS = ("kpcn_diffuse_in", "kpcn_specular_in", "kpcn_diffuse_buffer", "kpcn_specular_buffer", "kpcn_albedo")


@pytest.fixture(scope="module")
def loader_dir(tmp_path_factory):
    """Three 48 x 40 training frames with 4 samples, their probability maps written, and every image's device buffers."""
    from wcmc_amd.support.datasets import DenoiseDirectory, DenoisePreprocessor, sanitized
    root = str(tmp_path_factory.mktemp("ms_data"))
    for k, name in enumerate(("room", "car", "den")):
        _write_scene(root, "train", name, 48, 40, 4, 9100 + 100 * k)
    d = DenoiseDirectory(root, 4, "train", batch_size=LB, device=DEV, patch_size=LP, use_llpm_buf=True)
    d.offline_preprocess(llpm=False, kpcn=False)
    pre, frames = DenoisePreprocessor(), []
    for i in range(3):
        p = d.paths(i)
        x = _dev(sanitized(np.load(p["in"])[:, :, :4]))
        ss, sp = pre._preprocess_sbmc(x)
        frames.append({"raw": x, "gt": _dev(sanitized(np.load(p["gt"]))), "prob": np.load(p["prob"]), "llpm": pre._preprocess_llpm(x),
                       "sbmc_s": ss, "sbmc_p": sp})
    return root, d, frames


def _run(loader, seed):
    np.random.seed(seed)
    got = [{k: v.clone() for k, v in b.items()} for b in loader]
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("window", [1, 2, 3])
def test_multi_count_loader_walks_the_schedule_and_equals_the_direct_path(loader_dir, window):
    from wcmc_amd.support.datasets import DenoisePreprocessor, PatchBatcher
    from wcmc_amd.support.loader import PatchLoader, multi_count_schedule
    root, d, frames = loader_dir
    loader = PatchLoader(d.reader, range(3), DEV, batch_size=LB, patch_size=LP, use_llpm=True, patches_per_image=PPI,
                         staged_hook=d.staged_hook, counts=COUNTS, window=window)
    sched = multi_count_schedule(3, COUNTS, window)
    assert len(loader) == 3 * len(COUNTS) * (PPI // LB) == 18
    got = _run(loader, 4321)
    assert [b["paths"].shape[1] for b in got] == [s for _, s in sched for _ in range(PPI // LB)]
    pre, batcher = DenoisePreprocessor(), PatchBatcher(LP, LB)
    batcher.patches_per_image = PPI
    np.random.seed(4321)
    k = 0
    for i, s in sched:                                 # fresh origins per (image, count), drawn in the schedule's order
        f = frames[i]
        origins = batcher.sample_origins(f["prob"])
        kp, ll = pre._preprocess_kpcn(f["raw"][:, :, :s].contiguous()), f["llpm"][:, :, :s].contiguous()
        for o in range(0, PPI, LB):
            want = batcher.batch(kp, ll, f["gt"], origins[o:o + LB])
            assert set(want) == set(got[k])
            for name in want:
                if name in STAT_KEYS:
                    _close(got[k][name], want[name], "batch %d (image %d, %d spp) %s" % (k, i, s, name))
                else:
                    assert torch.equal(got[k][name], want[name]), (k, i, s, name)
            k += 1
    assert k == len(got)


def test_multi_count_loader_for_sbmc_equals_the_direct_path(loader_dir):
    from wcmc_amd.support.datasets import DenoiseDirectory, SamplePatchBatcher
    from wcmc_amd.support.loader import PatchLoader, multi_count_schedule
    root, _, frames = loader_dir
    d = DenoiseDirectory(root, 4, "train", batch_size=LB, device=DEV, patch_size=LP, use_llpm_buf=True, base_model="sbmc")
    said = []
    loader = PatchLoader(d.reader, range(3), DEV, batch_size=LB, patch_size=LP, use_llpm=True, patches_per_image=PPI,
                         staged_hook=d.staged_hook, base_model="sbmc", counts=COUNTS, window=2, report=said.append)
    got = _run(loader, 99)
    sched = multi_count_schedule(3, COUNTS, 2)
    assert len(got) == len(loader) == 18 and [b["radiance"].shape[1] for b in got] == [s for _, s in sched for _ in range(2)]
    assert len(said) == 1 and "window of 2" in said[0]
    batcher = SamplePatchBatcher(LP, LB)
    batcher.patches_per_image = PPI
    np.random.seed(99)
    k = 0
    cut = lambda t, s: t[:, :, :s].contiguous()                                           # noqa: E731
    for i, s in sched:
        f = frames[i]
        origins = batcher.sample_origins(f["prob"])
        for o in range(0, PPI, LB):
            want = batcher.batch(cut(f["sbmc_s"], s), cut(f["sbmc_p"], s), cut(f["llpm"], s), f["gt"], origins[o:o + LB])
            assert set(want) == set(got[k]) == {"radiance", "features", "paths", "target_image"}
            assert all(torch.equal(got[k][n], want[n]) for n in want), (k, i, s)
            k += 1


def test_without_counts_the_loader_yields_what_it_yields_today(loader_dir):
    from wcmc_amd.support.datasets import DenoisePreprocessor, PatchBatcher
    from wcmc_amd.support.loader import PatchLoader
    root, d, frames = loader_dir
    mk = lambda **kw: PatchLoader(d.reader, range(3), DEV, batch_size=LB, patch_size=LP, use_llpm=True, patches_per_image=PPI,  # noqa: E731
                                  staged_hook=d.staged_hook, **kw)
    a, b = _run(mk(counts=None), 5), _run(mk(), 5)
    assert len(a) == len(b) == len(mk()) == 6
    assert all(set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))
    # ... which is the single-count path on the whole frame, bit for bit
    pre, batcher = DenoisePreprocessor(), PatchBatcher(LP, LB)
    batcher.patches_per_image = PPI
    np.random.seed(5)
    f = frames[0]
    origins = batcher.sample_origins(f["prob"])
    want = batcher.batch(pre._preprocess_kpcn(f["raw"]), f["llpm"], f["gt"], origins[:LB])
    assert all(torch.equal(a[0][k], want[k]) for k in want)


def test_grid_batches_over_counts_from_one_upload(loader_dir):
    from wcmc_amd.support.datasets import DenoiseDirectory
    root, _, frames = loader_dir
    va = DenoiseDirectory(root, 4, "train", 4, "grid", use_llpm_buf=True, device=DEV, patch_size=LP)
    plain, multi = list(va.grid_batches([0])), list(va.grid_batches([0], counts=COUNTS))
    assert len(plain) == va.num_grid_batches([0]) == 2 and len(multi) == va.num_grid_batches([0], counts=COUNTS) == 6
    assert [b["paths"].shape[1] for b in multi] == [2, 2, 3, 3, 4, 4]
    for a, b in zip(multi[4:], plain):                                                     # the last count is the whole frame
        for k in b:
            if k in STAT_KEYS:
                _close(a[k], b[k], k)
            else:
                assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------- 4. the launchers
@pytest.fixture(scope="module")
def launch_dir(tmp_path_factory):
    """Two training frames and one validation frame of 64 x 64 at 3 samples."""
    root = str(tmp_path_factory.mktemp("ms_launch"))
    _write_scene(root, "train", "room", 64, 64, 3, 9500)
    _write_scene(root, "train", "car", 64, 64, 3, 9600)
    _write_scene(root, "val", "den", 64, 64, 3, 9700)
    return root


def _argv(root, save, *extra):
    return ["--from_data_dir", "--data_dir", root, "--multi_spp", "--num_samples", "3", "-b", "2", "--patch_size", "48",
            "--patches_per_image", "2", "-e", "1", "--not_save", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE",
            "--desc", "multi spp", "--save", save] + list(extra)


def _spy_on(monkeypatch, itf_class, seen):
    from wcmc_amd import train_kpcn as tk
    inner_summary, inner_val, inner_train = itf_class.get_epoch_summary, itf_class.validate_batch, tk.train

    def summary(self, mode, norm):
        if mode == "train":
            seen["train_norm"] = norm
            seen["losses"] = {k: float(v) for k, v in self.m_losses.items() if k != "m_val"}
        out = inner_summary(self, mode, norm)
        seen.setdefault("summaries", []).append((mode, out))
        return out

    def validate_batch(self, batch):
        seen.setdefault("val_counts", []).append(batch["paths"].shape[1])
        return inner_val(self, batch)

    def train(interfaces, loaders, params, args):
        seen["lens"], seen["params"] = (len(loaders["train"]), len(loaders["val"])), params
        return inner_train(interfaces, loaders, params, args)

    monkeypatch.setattr(itf_class, "get_epoch_summary", summary)
    monkeypatch.setattr(itf_class, "validate_batch", validate_batch)
    monkeypatch.setattr(tk, "train", train)


def _check_epoch(seen):
    assert seen["lens"] == (4, 2)                       # 2 images x 2 counts x 1 batch; 1 whole grid window x 2 counts
    assert seen["train_norm"] == 4
    assert seen["losses"] and all(np.isfinite(v) for v in seen["losses"].values()) and seen["losses"]["m_l_total"] > 0
    assert sorted(seen["val_counts"]) == [2, 3]
    assert all(np.isfinite(v) for _, v in seen["summaries"]) and [m for m, _ in seen["summaries"]] == ["train", "eval"]


def test_train_kpcn_multi_spp_runs_an_epoch_over_both_counts(launch_dir, tmp_path, monkeypatch, capsys):
    from wcmc_amd import train_kpcn as tk
    from wcmc_amd.support.interfaces import KPCNInterface
    seen, shapes, inner = {}, [], KPCNInterface.train_batch

    def train_batch(self, batch):
        shapes.append(batch["paths"].shape[1])
        return inner(self, batch)

    monkeypatch.setattr(KPCNInterface, "train_batch", train_batch)
    _spy_on(monkeypatch, KPCNInterface, seen)
    tk.main(_argv(launch_dir, str(tmp_path / "w"), "--ms_window", "1"))
    _check_epoch(seen)
    assert shapes == [2, 3, 2, 3]                       # window 1: image-major
    assert "multi-count loader" in capsys.readouterr().out                                # the footprint, once


def test_train_kpcn_multi_spp_graph_never_holds_two_live_steps(launch_dir, tmp_path, monkeypatch):
    from wcmc_amd import graph
    from wcmc_amd import train_kpcn as tk
    from wcmc_amd.support.interfaces import KPCNInterface
    seen = {}
    live, log, calls = [0], [], []
    inner_init, inner_close, inner_call, inner_cv = (graph.GraphedTrainStep.__init__, graph.GraphedTrainStep.close,
                                                     graph.GraphedTrainStep.__call__, graph.capture_validated)

    def init(self, itf, batch, *a, **kw):
        assert live[0] == 0, "a step was captured while another one was live"
        live[0] += 1
        log.append(("capture", batch["paths"].shape[1]))
        return inner_init(self, itf, batch, *a, **kw)

    def close(self):
        if self.itf is not None:                        # (close is idempotent: count a step once)
            live[0] -= 1
            log.append(("close",))
        return inner_close(self)

    def call(self, batch):
        log.append(("step", batch["paths"].shape[1]))
        return inner_call(self, batch)

    def cv(itf, batch, **kw):
        step = inner_cv(itf, batch, **kw)
        calls.append(step.capture_attempts)
        return step

    monkeypatch.setattr(graph.GraphedTrainStep, "__init__", init)
    monkeypatch.setattr(graph.GraphedTrainStep, "close", close)
    monkeypatch.setattr(graph.GraphedTrainStep, "__call__", call)
    monkeypatch.setattr(graph, "capture_validated", cv)
    _spy_on(monkeypatch, KPCNInterface, seen)
    try:
        tk.main(_argv(launch_dir, str(tmp_path / "w"), "--graph", "--ms_window", "2"))
    finally:
        for step in seen.get("params", {}).get("graphed_steps", {}).values():            # leave no live step behind
            step.close()
    _check_epoch(seen)
    assert live[0] == 0
    assert [e[1] for e in log if e[0] == "step"] == [2, 2, 3, 3]                          # one window of two images: count-major
    assert len(calls) == 2                                                                # one capture_validated per (window, count)
    assert sum(calls) == len([e for e in log if e[0] == "capture"])                       # plus what it repeats
    # a capture follows a close or nothing; never another capture without a close in between
    kinds = [e[0] for e in log if e[0] != "step"]
    assert all(not (a == "capture" and b == "capture") for a, b in zip(kinds, kinds[1:]))


def test_multi_spp_argument_errors_through_main(launch_dir, tmp_path):
    from wcmc_amd import train_kpcn as tk
    argv = _argv(launch_dir, str(tmp_path / "w"))
    with pytest.raises(RuntimeError, match="spp too low to randomize sample count"):
        tk.main([a if a != "3" else "1" for a in argv])
    with pytest.raises(RuntimeError) as exc:
        tk.main([a for a in argv if a != "--from_data_dir"])
    assert "--multi_spp" in str(exc.value) and "--from_data_dir" in str(exc.value)


@pytest.mark.parametrize("launcher", ["train_sbmc", "train_lbmc"])
def test_sample_based_launchers_run_a_multi_spp_epoch(launch_dir, tmp_path, monkeypatch, launcher):
    import importlib
    from wcmc_amd.support.interfaces import SBMCInterface
    mod = importlib.import_module("wcmc_amd." + launcher)
    seen = {}
    _spy_on(monkeypatch, SBMCInterface, seen)
    itfs = mod.main(_argv(launch_dir, str(tmp_path / "w"), "--denoiser", "standins:SampleDenoiserStandIn", "--ms_window", "2"))
    assert str(itfs[0]) == ("SBMCInterface" if launcher == "train_sbmc" else "LBMCInterface")
    _check_epoch(seen)
