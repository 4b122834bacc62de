#!/usr/bin/env python3
"""Measure the multi-count data step on one GPU.

  kernel   one 1024 x 1024 x 8 frame: ``preprocess_kpcn_prefix(raw, 2, 8)`` against what a single-count build does for the same
           seven buffers -- seven times slice, ``.contiguous()`` and ``preprocess_kpcn``.  The two arms alternate in one process;
           warm-up, then the median of ``--reps`` (>= 20) timings each.
  epoch    a generated four-frame directory: one ``PatchLoader(counts=2..8, window=1)`` epoch against seven single-count
           ``PatchLoader`` passes over the same frames; loader only, the batches are dropped.
  capture  one ``capture_validated`` call on the KPCN-Manifold step (what ``--graph`` pays per (window, count)), and the device
           bytes one staged image holds.

Prints one JSON line; ``--out`` also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn_a, fn_b, reps, warmup=3):
    ta, tb = [], []
    for r in range(warmup + reps):
        for fn, acc in ((fn_a, ta), (fn_b, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                acc.append(e0.elapsed_time(e1))
    return statistics.median(ta), statistics.median(tb), min(ta), min(tb)


def time_kernel(size, spp, reps, dev):
    from wcmc_amd import ops
    raw = torch.rand(size, size, spp, 104, device=dev)
    lo, hi = 2, spp
    prefix = lambda: ops.preprocess_kpcn_prefix(raw, lo, hi)                                 # noqa: E731
    seven = lambda: [ops.preprocess_kpcn(raw[:, :, :s].contiguous()) for s in range(lo, hi + 1)]      # noqa: E731
    a, b, amin, bmin = _median_ms(prefix, seven, reps)
    npix, n = size * size, hi - lo + 1
    raw_bytes = npix * spp * 104 * 4
    # prefix pass: raw once, the slabs written by pass 1 and read + written by the finish pass, the workspace pairs written and read
    prefix_bytes = raw_bytes + n * npix * (3 * 44 + 2 * 2) * 4
    # seven passes: each slice is read and written by the copy and read by the kernel; the outputs as above
    seven_bytes = sum(3 * npix * s * 104 * 4 for s in range(lo, hi + 1)) + n * npix * (3 * 44 + 2 * 2) * 4
    return {"frame": [size, size, spp], "counts": [lo, hi], "prefix_ms": round(a, 3), "seven_passes_ms": round(b, 3),
            "prefix_min_ms": round(amin, 3), "seven_passes_min_ms": round(bmin, 3), "ratio": round(b / a, 3),
            "raw_GB": round(raw_bytes / 1e9, 3), "prefix_bytes_GB": round(prefix_bytes / 1e9, 3),
            "seven_bytes_GB": round(seven_bytes / 1e9, 3), "prefix_GBps": round(prefix_bytes / a / 1e6, 1),
            "seven_GBps": round(seven_bytes / b / 1e6, 1), "prefix_raw_only_GBps": round(raw_bytes / a / 1e6, 1)}


def _write_dir(root, n, size, spp):
    rng = np.random.default_rng(0)
    for d in ("gt", "input"):
        os.makedirs(os.path.join(root, "train", d))
    for i in range(n):
        np.save(os.path.join(root, "train", "input", "f%d.npy" % i), rng.random((size, size, spp, 104), dtype=np.float32))
        gt = rng.random((size, size, 9), dtype=np.float32)
        gt[..., :3] += 1.0
        np.save(os.path.join(root, "train", "gt", "f%d.npy" % i), gt)


def time_epoch(size, spp, n_frames, dev):
    from wcmc_amd.support.datasets import DenoiseDirectory, multi_counts
    from wcmc_amd.support.loader import PatchLoader
    out = {}
    with tempfile.TemporaryDirectory() as root:
        _write_dir(root, n_frames, size, spp)
        d = DenoiseDirectory(root, spp, "train", batch_size=8, device=dev, use_llpm_buf=True)
        d.offline_preprocess(llpm=False, kpcn=False)                                         # the probability maps, ahead of time

        def run(loader):
            n = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in loader:
                n += 1
            torch.cuda.synchronize()
            return time.perf_counter() - t0, n

        def multi():
            said = []
            t, n = run(PatchLoader(d.reader, range(len(d)), dev, batch_size=8, use_llpm=True, staged_hook=d.staged_hook,
                                   counts=multi_counts(spp), window=1, report=said.append))
            out["footprint_line"] = said[0] if said else None
            return t, n

        def singles():
            t, n = 0.0, 0
            for s in multi_counts(spp):
                ds = DenoiseDirectory(root, s, "train", batch_size=8, device=dev, use_llpm_buf=True)
                ti, ni = run(PatchLoader(ds.reader, range(len(ds)), dev, batch_size=8, use_llpm=True, staged_hook=ds.staged_hook))
                t, n = t + ti, n + ni
            return t, n

        multi(), singles()                                                                   # warm-up: page cache, allocator, pinned ring
        tm, ts = [], []
        for _ in range(3):
            (a, na), (b, nb) = multi(), singles()
            assert na == nb
            tm.append(a)
            ts.append(b)
    out.update({"frames": n_frames, "frame": [size, size, spp], "batches": na, "multi_epoch_s": round(statistics.median(tm), 3),
                "seven_single_passes_s": round(statistics.median(ts), 3),
                "ratio": round(statistics.median(ts) / statistics.median(tm), 3)})
    return out


def time_capture(dev):
    from wcmc_amd import train_kpcn as tk
    from wcmc_amd.graph import capture_validated
    from wcmc_amd.synthetic import make_batch
    args = tk.check_args(tk.build_parser().parse_args(["--desc", "t", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE",
                                                        "--train_branches", "--not_save", "--save", tempfile.mkdtemp(), "-b", "8"]))
    torch.manual_seed(0)
    itfs, _ = tk.init_model({"dncnn_in_size": 39, "pnet_in_size": 36, "pnet_out_size": 3}, args, torch.device(dev))
    itf = itfs[0]
    itf.to_train_mode()
    res = []
    for s in (2, 8):
        batch = make_batch(8, s, 128, seed=s, device=dev, use_llpm=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step = capture_validated(itf, batch, two_stream=bool(itf.halves_supported()))
        torch.cuda.synchronize()
        res.append({"spp": s, "capture_validated_s": round(time.perf_counter() - t0, 3), "attempts": step.capture_attempts,
                    "replay_ms": step.capture_ms})
        step.close()                                                                         # never two live steps
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epoch_size", type=int, default=256, help="frame edge of the epoch timing's directory")
    ap.add_argument("--skip", nargs="*", default=[], choices=["kernel", "epoch", "capture"])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    res = {}
    if "kernel" not in a.skip:
        res["kernel"] = time_kernel(a.size, a.spp, max(20, a.reps), dev)
    if "epoch" not in a.skip:
        res["epoch"] = time_epoch(a.epoch_size, a.spp, 4, dev)
    if "capture" not in a.skip:
        res["capture"] = time_capture(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
