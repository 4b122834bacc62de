"""Regenerate tests/golden/metrics.npz from the reference's support/metrics.py (run by hand, from the repository root):

    python tests/golden/make_golden_metrics.py path/to/reference

It imports the reference's ``support/metrics.py`` with a stub for its ``skimage.metrics`` import (the SSIM is not part of
the fixture: skimage is not installed and its version is not pinned; DESIGN.md section 10 specifies it instead), as
``make_golden.py`` stubs ``kornia``, and stores input triples with the reference's ``MSE``, ``RelMSE`` (reduce True and
False), ``TRelMSE``, ``L1``, ``RelL1`` and ``_tonemap`` outputs.  Only data is written; no reference source travels.

Cases: HDR lognormal values up to 1e3, negatives, zeros in ``ref``, scattered NaNs (cases 1 and 3; they make MSE / L1 /
RelL1 NaN and leave RelMSE finite) and odd sizes.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WCMC_REFERENCE", "")


def import_reference_metrics():
    if not os.path.isfile(os.path.join(REF, "support", "metrics.py")):
        raise SystemExit("usage: make_golden_metrics.py REFERENCE_CHECKOUT (or WCMC_REFERENCE=...)")
    sys.path.insert(0, REF)
    sk = types.ModuleType("skimage")
    skm = types.ModuleType("skimage.metrics")

    def _absent(*a, **k):
        raise NotImplementedError("skimage is not installed; SSIM is not part of the fixture")
    skm.structural_similarity = _absent
    sk.metrics = skm
    sys.modules["skimage"] = sk
    sys.modules["skimage.metrics"] = skm
    from support import metrics
    return metrics


def make_cases():
    rng = np.random.default_rng(20261016)
    cases = []
    for (h, w) in ((7, 7), (13, 29), (64, 48), (101, 37), (33, 65)):
        ref = np.minimum(rng.lognormal(0.0, 2.0, (h, w, 3)), 1e3).astype(np.float32)
        im = (ref * rng.lognormal(0.0, 0.3, (h, w, 3))).astype(np.float32)
        im -= (rng.random((h, w, 3)) < 0.1) * rng.random((h, w, 3)).astype(np.float32) * 2      # negatives
        ref[rng.random((h, w, 3)) < 0.05] = 0.0                                                   # zeros in ref
        if len(cases) in (1, 3):
            im[rng.random((h, w, 3)) < 0.01] = np.nan                                             # scattered NaNs
            ref[rng.random((h, w, 3)) < 0.005] = np.nan
        cases.append((im.astype(np.float32), ref.astype(np.float32)))
    return cases


def main():
    m = import_reference_metrics()
    out = {}
    for n, (im, ref) in enumerate(make_cases()):
        p = "c%d_" % n
        out[p + "im"], out[p + "ref"] = im, ref
        out[p + "MSE"] = np.float64(m.MSE(im, ref))
        out[p + "RelMSE"] = np.float64(m.RelMSE(im, ref))
        out[p + "RelMSE_full"] = m.RelMSE(im, ref, reduce=False)
        out[p + "TRelMSE"] = np.float64(m.TRelMSE(im, ref))
        out[p + "L1"] = np.float64(m.L1(im, ref))
        out[p + "RelL1"] = np.float64(m.RelL1(im, ref))
        out[p + "RelMSE_eps1e-2"] = np.float64(m.RelMSE(im, ref, eps=1e-2))
        out[p + "tonemap_im"] = m._tonemap(im)
    out["n_cases"] = np.int64(len(make_cases()))
    np.savez_compressed(os.path.join(HERE, "metrics.npz"), **out)
    print("wrote", os.path.join(HERE, "metrics.npz"), len(out), "arrays")


if __name__ == "__main__":
    main()
