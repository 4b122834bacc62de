"""Timing of the evaluation path on the MI355X (one JSON object per line; profiles/eval_timing.txt):

  * image_eval   median device time (hipEvents) of ``ops.image_eval`` on one 1224 x 1224 triple (all 40 metrics);
  * stitch_tiles median device time per batch of 8 tiles (92 x 92 radiance + two (8, 3, 128, 128) P-buffers);
  * denoise      wall time of ``evaluate.denoise`` on a synthetic 1280 x 1280 scene at 8 spp (a freshly initialised
                 KPCN-Manifold model; files written to a temp dir first, the first call warms up), next to the wall time
                 of the fp64 numpy restatement of the same frame's 40 metrics on the host (tests/image_eval_ref.py,
                 single-threaded scipy).

    timeout -k 10 900 python scripts/time_eval.py [--reps 50]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _events_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no_denoise", action="store_true")
    a = ap.parse_args()
    from wcmc_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    h = w = 1224
    tgt = np.minimum(rng.lognormal(0, 1.5, (h, w, 3)), 1e3).astype(np.float32)
    out = (tgt * rng.lognormal(0, 0.05, (h, w, 3))).astype(np.float32)
    ipt = (tgt * rng.lognormal(0, 0.5, (h, w, 3))).astype(np.float32)
    hit = np.ones_like(tgt)
    T = [torch.from_numpy(x).to(dev) for x in (out, ipt, tgt, hit)]
    med, lo, hi = _events_ms(lambda: ops.image_eval(*T), a.reps)
    print(json.dumps({"what": "image_eval", "frame": [h, w], "median_ms": round(med, 4), "min_ms": round(lo, 4),
                      "max_ms": round(hi, 4), "reps": a.reps}), flush=True)

    B, S = 8, 8
    H = W = 1280
    rad = torch.randn(B, 3, 92, 92, device=dev)
    pa, pb = torch.randn(B, S, 3, 128, 128, device=dev), torch.randn(B, S, 3, 128, 128, device=dev)
    from wcmc_amd.support.inference import tile_coords
    coords = torch.tensor(tile_coords(H, W)[:B], dtype=torch.int32, device=dev)
    orad = torch.zeros(3, H, W, device=dev)
    opath = {"diffuse": torch.zeros(S, 3, H, W, device=dev), "specular": torch.zeros(S, 3, H, W, device=dev)}
    med, lo, hi = _events_ms(lambda: ops.stitch_tiles(rad, {"diffuse": pa, "specular": pb}, coords, orad, opath), a.reps)
    print(json.dumps({"what": "stitch_tiles", "tiles": B, "spp": S, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                      "max_ms": round(hi, 4), "reps": a.reps}), flush=True)

    if a.no_denoise:
        return
    from image_eval_ref import evaluate as host_eval
    from test_gpu_evaluate import _args, _write_scene           # the test's file layout and flags
    from wcmc_amd import evaluate, train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    with tempfile.TemporaryDirectory() as root:
        _write_scene(root, "big", H, W, seed=7, llpm_spp=(8,), spps=[8])
        save = os.path.join(root, "w")
        args = _args(save)
        torch.manual_seed(0)
        itfs, _ = train_kpcn.init_model({"dncnn_in_size": 39, "pnet_in_size": 36, "pnet_out_size": 3}, args, dev)
        torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, "KPCN_eval_test.pth"))
        walls = []
        frames = {}
        for rep in range(3):
            args = _args(save)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate.denoise(args, os.path.join(root, "KPCN/input"), os.path.join(root, "out"), scenes=["big"], spps=[8],
                             device=dev, frames=frames)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        o, i, t = (x.cpu().numpy() for x in frames[("big", 8)])
        t0 = time.perf_counter()
        host_eval(o, i, t)
        host = time.perf_counter() - t0
    print(json.dumps({"what": "denoise", "frame": [H, W], "spp": 8, "wall_s_per_call": [round(x, 3) for x in walls],
                      "note": "first call includes model build / warm-up", "host_fp64_metrics_s": round(host, 3),
                      "cropped_frame": list(o.shape[:2])}), flush=True)


if __name__ == "__main__":
    main()
