"""Timing of the structural-similarity loss on the MI355X (one JSON object per line; profiles/dssim_loss_timing.txt) at the
step's shape (N, C, H, W) = (8, 3, 92, 92) and at (8, 3, 128, 128), Reinhard tone map, data range 2.

Arms, all in one process, interleaved (round r runs every arm once, in turn; hipEvents around --inner back-to-back calls on
preallocated buffers, median of --reps such windows per round, the figure is the median over the rounds):

  * hip_fwd          ``wcmc_dssim_loss_fwd`` (partial + finish launch)
  * hip_fwd_bwd      ``wcmc_dssim_loss_fwd`` then ``wcmc_dssim_loss_bwd``
  * torch_fwd_bwd    the fp32 torch-op route (tests/ssim_loss_ref.py: ``F.avg_pool2d`` moments) forward + autograd backward

The HIP forward + backward must beat the torch route.  A training step with ``--dssim_weight`` makes two such calls (diffuse and
specular); the records state them as a share of the benchmarked step (10.66 ms).

    timeout -k 10 300 python scripts/time_dssim_loss.py [--reps 10] [--rounds 5] [--inner 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(8, 3, 92, 92), (8, 3, 128, 128)]
STEP_MS = 10.66


def _median_ms(fn, reps, inner):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts))


def _ab(arms, reps, rounds, inner):
    """{name: [median per round]} with the arms interleaved: round r runs every arm once, in turn."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            meds[k].append(_median_ms(fn, reps, inner))
    return meds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    import ssim_loss_ref as slr
    from wcmc_amd import ops
    from wcmc_amd._lib import check, lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L, st, P = lib(), ops._stream, ops._ptr
    ok = True
    for n, c, h, w in SHAPES:
        x, ref = slr.radiance((n, c, h, w), 1).to(dev), slr.radiance((n, c, h, w), 2).to(dev)
        nbytes = L.wcmc_dssim_loss_workspace_bytes(n, c, h, w)
        ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
        loss, dx, g = torch.empty((), device=dev), torch.empty((n, c, h, w), device=dev), torch.ones((), device=dev)
        xt = x.clone().requires_grad_(True)

        def hip_fwd():
            check(L.wcmc_dssim_loss_fwd(P(x), *x.stride(), P(ref), *ref.stride(), 1, 2.0, P(loss), P(ws), nbytes, n, c, h, w, st()), "fwd")

        def hip_fwd_bwd():
            hip_fwd()
            check(L.wcmc_dssim_loss_bwd(P(x), *x.stride(), P(ref), *ref.stride(), 1, 2.0, P(g), P(dx), n, c, h, w, st()), "bwd")

        def torch_fwd_bwd():
            xt.grad = None
            slr.dssim(xt, ref, "reinhard", 2.0).backward()

        # the timed code computes what the torch route computes
        hip_fwd_bwd()
        torch_fwd_bwd()
        assert abs(loss.item() - slr.dssim(x, ref).item()) <= 4e-6
        assert ((dx - xt.grad).abs().max() / xt.grad.abs().max()).item() <= 1e-4
        meds = _ab({"hip_fwd": hip_fwd, "hip_fwd_bwd": hip_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd}, a.reps, a.rounds, a.inner)
        med = {k: float(np.median(v)) for k, v in meds.items()}
        for k, v in meds.items():
            rec = {"what": k, "shape": [n, c, h, w], "reps": a.reps, "rounds": a.rounds, "inner": a.inner,
                   "median_ms": round(med[k], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            if k == "hip_fwd_bwd":
                rec.update({"torch_over_hip": round(med["torch_fwd_bwd"] / med[k], 2), "hip_beats_torch": bool(med[k] < med["torch_fwd_bwd"]),
                            "two_calls_ms": round(2 * med[k], 4), "two_calls_share_of_%g_ms_step" % STEP_MS: round(2 * med[k] / STEP_MS, 4)})
            print(json.dumps(rec), flush=True)
        ok = ok and med["hip_fwd_bwd"] < med["torch_fwd_bwd"]
    assert ok, "the HIP forward + backward must beat the torch route"


if __name__ == "__main__":
    main()
