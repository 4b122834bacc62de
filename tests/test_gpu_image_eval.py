"""The frame-evaluation kernel (wcmc_image_eval) against the fp64 numpy restatement (tests/image_eval_ref.py), and the public
support.metrics functions against the reference's support/metrics.py (tests/golden/metrics.npz)."""
import os

import numpy as np
import pytest
import torch

from image_eval_ref import evaluate

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
DEV = "cuda:0"


def _frame(h, w, seed, hdr=False, nan=False):
    rng = np.random.default_rng(seed)
    if hdr:
        tgt = np.minimum(rng.lognormal(1.0, 2.0, (h, w, 3)), 2e3)
    else:
        tgt = rng.random((h, w, 3)) * 1.5
    tgt = tgt.astype(np.float32)
    out = (tgt * rng.lognormal(0.0, 0.05, (h, w, 3)) + rng.normal(0, 0.01, (h, w, 3))).astype(np.float32)
    ipt = (tgt * rng.lognormal(0.0, 0.5, (h, w, 3)) - rng.random((h, w, 3)) * 0.05).astype(np.float32)
    tgt[rng.random((h, w, 3)) < 0.02] = 0.0
    if nan:
        out[rng.random((h, w, 3)) < 0.002] = np.nan
    return out, ipt, tgt


def _check(got, want):
    got = got.cpu().numpy()
    assert got.shape == (2, 4, 5)
    both_nan = np.isnan(got) & np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    for k in (0, 1, 3, 4):                          # pointwise: relative 1e-6
        g, w = got[..., k], want[..., k]
        ok = both_nan[..., k] | (np.abs(g - w) <= 1e-6 * np.abs(w) + 1e-300)
        assert ok.all(), (k, g, w)
    g, w = got[..., 2], want[..., 2]                 # DSSIM: absolute 2e-6
    assert (both_nan[..., 2] | (np.abs(g - w) <= 2e-6)).all(), (g, w)


def _chw(x):
    """The channel-first frame the driver holds, passed to the kernel as a strided (H, W, 3) view."""
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))).to(DEV).permute(1, 2, 0)


@pytest.mark.parametrize("h,w,kind", [(1224, 1224, "plain"), (1000, 563, "plain"), (7, 7, "plain"), (301, 257, "hdr"),
                                      (130, 97, "nan"), (200, 333, "has_hit")])
def test_image_eval_matches_fp64_restatement(h, w, kind):
    from wcmc_amd import ops
    out, ipt, tgt = _frame(h, w, seed=h * 7 + w, hdr=(kind == "hdr"), nan=(kind == "nan"))
    hit = None
    if kind == "has_hit":
        rng = np.random.default_rng(5)
        hit = np.repeat((rng.random((h, w, 1)) < 0.7).astype(np.float32), 3, axis=2)
    got = ops.image_eval(_chw(out), torch.from_numpy(ipt).to(DEV), _chw(tgt),
                         None if hit is None else torch.from_numpy(hit).to(DEV))
    _check(got, evaluate(out, ipt, tgt, hit))


def test_image_eval_is_bitwise_reproducible():
    from wcmc_amd import ops
    out, ipt, tgt = (torch.from_numpy(x).to(DEV) for x in _frame(517, 389, seed=3, hdr=True))
    a = ops.image_eval(out, ipt, tgt)
    b = ops.image_eval(out, ipt, tgt)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_image_eval_rejects_images_below_7x7():
    from wcmc_amd import ops
    from wcmc_amd.support import metrics
    x = torch.ones((6, 9, 3), device=DEV)
    with pytest.raises(ValueError, match="7 x 7"):
        ops.image_eval(x, x, x)
    with pytest.raises(ValueError, match="7 x 7"):
        metrics.SSIM(x, x)


def test_public_metrics_reproduce_the_reference_goldens():
    from wcmc_amd.support import metrics as M
    d = np.load(GOLDEN)
    for n in range(int(d["n_cases"])):
        p = "c%d_" % n
        im, ref = d[p + "im"], d[p + "ref"]
        for name, fn in (("MSE", M.MSE), ("RelMSE", M.RelMSE), ("TRelMSE", M.TRelMSE), ("L1", M.L1), ("RelL1", M.RelL1)):
            got, want = fn(im, ref), float(d[p + name])
            assert isinstance(got, float)
            assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-5 * abs(want), (n, name, got, want)
        got = M.RelMSE(im, ref, eps=1e-2)
        assert abs(got - float(d[p + "RelMSE_eps1e-2"])) <= 1e-5 * abs(float(d[p + "RelMSE_eps1e-2"]))
        full = M.RelMSE(im, ref, reduce=False).cpu().numpy()
        np.testing.assert_allclose(full, d[p + "RelMSE_full"], rtol=1e-5)
        np.testing.assert_allclose(M._tonemap(im).cpu().numpy(), d[p + "tonemap_im"], rtol=1e-6, equal_nan=True)
        # torch input on the device gives the same numbers (NaN-free cases: NaN != NaN)
        if not np.isnan(want):
            assert M.L1(torch.from_numpy(im).to(DEV), torch.from_numpy(ref).to(DEV)) == M.L1(im, ref)


def test_public_ssim_and_tonemaps_match_the_restatement():
    from image_eval_ref import ssim, tonemap
    from wcmc_amd.support import metrics as M
    out, _, tgt = _frame(64, 80, seed=11)
    assert abs(M.SSIM(out, tgt) - (1 - ssim(out, tgt))) <= 2e-6
    assert M.SSIM(tgt, tgt) == pytest.approx(0.0, abs=1e-12)
    with pytest.raises(TypeError):
        M.SSIM(out, tgt, reduce=False)
    np.testing.assert_allclose(M.tonemap(out).cpu().numpy(), tonemap(out), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(M.tonemap(out, kInvGamma=1 / 2.8).cpu().numpy(), tonemap(out, kInvGamma=1 / 2.8),
                               rtol=2e-6, atol=1e-7)


def test_evaluate_frame_returns_the_two_csv_rows():
    from wcmc_amd.support import metrics as M
    out, ipt, tgt = _frame(90, 120, seed=21)
    hit = np.ones_like(out)
    hit[:10] = 0
    a, b = M.evaluate_frame(out, ipt, tgt, hit)
    want = evaluate(out, ipt, tgt, hit)
    assert a.shape == (20,) and b.shape == (20,)
    np.testing.assert_allclose(a, want[0].reshape(20), rtol=1e-6, atol=2e-6)
    np.testing.assert_allclose(b, want[1].reshape(20), rtol=1e-6, atol=2e-6)
