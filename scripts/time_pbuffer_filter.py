"""Timing of the P-buffer filter on the MI355X (one JSON object per line; profiles/pbuffer_filter_timing.txt) on a 1280 x 720 frame
with S = 8 samples, C = 3 embedding channels, Cr = 3, R = 10, f = 1: 921,600 pixels x 441 window pairs.

Arms, all in one process, interleaved (round r runs every arm once, in turn; hipEvents around --inner back-to-back calls on
preallocated inputs, median of --reps such windows per round, the figure is the median over the rounds):

  * stats          the statistics launch of ``wcmc_pbuffer_filter`` (passes = 1)
  * filter         the filter launch (passes = 2; the workspace holds the statistics)
  * op             both, as ``ops.pbuffer_filter`` runs them
  * torch_fp32     the fp32 torch route of the same specification on the GPU: shifted planes plus ``avg_pool2d``, tests/rhf_ref.py with
                   dtype float32 -- a reference that nothing here optimises.  CONDITION: the op is faster.

The record of ``filter`` states the rate in window pairs per second and where the time goes by the kernel's arithmetic.

    timeout -k 10 600 python scripts/time_pbuffer_filter.py [--reps 5] [--rounds 5] [--inner 5] [--out profiles/pbuffer_filter_timing.txt]
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

H, W, S, C, CR, R, F = 720, 1280, 8, 3, 3, 10, 1


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pbuffer_filter_timing.txt"))
    a = ap.parse_args()
    from rhf_ref import rhf_ref, scene
    from wcmc_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    img, p = scene(H, W, S, C, CR)
    image, p_buffer = img.to(dev), p.to(dev)
    kw = dict(radius=R, patch_radius=F, bandwidth=1.0, eps=1e-3)
    ws = torch.empty(C * H * W * 2, device=dev)

    def torch_route():
        with torch.no_grad():
            return rhf_ref(image, p_buffer, dtype=torch.float32, **kw)

    # the op computes what the torch route computes (and the timing is of the tested code)
    out, wsum = ops.pbuffer_filter(image, p_buffer, **kw)
    t_out, t_wsum = torch_route()
    err = max(((out - t_out).abs().max() / t_out.abs().max()).item(), ((wsum - t_wsum).abs() / t_wsum).max().item())
    assert err <= 1e-4, err
    frac = float((wsum >= 2).float().mean()), float((wsum <= 0.5 * (2 * R + 1) ** 2).float().mean())
    arms = {"stats": lambda: ops.pbuffer_filter(image, p_buffer, passes=ops.PBF_STATS, workspace=ws, **kw),
            "filter": lambda: ops.pbuffer_filter(image, p_buffer, passes=ops.PBF_FILTER, workspace=ws, **kw),
            "op": lambda: ops.pbuffer_filter(image, p_buffer, workspace=ws, **kw),
            "torch_fp32": torch_route}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            meds[k].append(_median_ms(fn, 2 if k == "torch_fp32" else a.reps, 1 if k == "torch_fp32" else a.inner))
    med = {k: float(np.median(v)) for k, v in meds.items()}
    pairs = float(H) * W * (2 * R + 1) ** 2
    lines = []
    for k, v in meds.items():
        rec = {"what": k, "shape": {"H": H, "W": W, "S": S, "C": C, "Cr": CR, "R": R, "f": F}, "reps": a.reps, "rounds": a.rounds,
               "median_ms": round(med[k], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if k == "stats":
            rec["p_buffer_GB_per_s"] = round(4.0 * S * C * H * W / 1e9 / (med[k] / 1e3), 1)
        if k == "filter":
            dpos = (32 + 2 * F) * (8 + 2 * F) / 256.0
            rec.update({"window_pairs_per_s": round(pairs / (med[k] / 1e3), -6), "input": {"wsum>=2": round(frac[0], 3),
                                                                                             "wsum<=half_window": round(frac[1], 3)},
                        "per_pair": {"reciprocals": round(C * dpos + 1, 2), "exp2": 1, "lds_float2_reads": round(C * dpos, 2),
                                     "lds_float_reads": (2 * F + 1) ** 2, "lds_float_writes": round(dpos, 2),
                                     "lds_byte_reads": round(dpos + 1, 2), "global_loads": CR, "barriers_per_block": 1},
                        "where_the_time_goes": "per window offset a block computes %d deltas (%.2f per output pixel: %d hardware reciprocals each, "
                                               "its own statistics in registers, the partner's one 8-byte LDS read per channel), hands them over "
                                               "through LDS behind one barrier, and every thread box-sums %d of them, takes one reciprocal of the "
                                               "count and one exp2, and multiplies %d image taps loaded from global memory"
                                               % ((32 + 2 * F) * (8 + 2 * F), dpos, C, (2 * F + 1) ** 2, CR)})
        if k == "torch_fp32":
            rec.update({"torch_over_op": round(med[k] / med["op"], 1), "op_beats_torch": bool(med["op"] < med[k])})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert med["op"] < med["torch_fp32"], "the op must beat the torch route of the same specification"


if __name__ == "__main__":
    main()
