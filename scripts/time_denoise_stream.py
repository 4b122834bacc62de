"""Timing of the streamed upload of ``wcmc_amd.denoise`` against the whole-frame route it replaces, on the MI355X (one JSON object
per line; profiles/denoise_stream_timing.txt).  A synthetic 1280 x 720 frame at 8 samples per pixel is written to disk and read warm
(every arm runs once before anything is timed), the model is a freshly initialised KPCN-Manifold.  One process, alternating rounds:
each round runs every arm once, in turn; the figures are medians over the rounds, next to the spread (max - min) of each arm's rounds.

  * A      the whole-frame route: ``denoise.read_raw`` + ``denoise.upload_raw`` + ``DenoisePreprocessor``, from the file name to the
           buffers being ready (a device synchronise ends the region).
  * B      the streamed route for one frame, from a cold ``FrameStreamer`` (new threads, an empty ring; the pinned memory comes from
           torch's host allocator, warm after the first run) to the buffers being ready, at bands of 16, 64 and 256 MiB.
  * C      four frames in one call through one streamer (``denoise.denoise_file`` per frame: network, finish, files), per frame in
           steady state (frames 2..4), against A followed by the same network / finish / files.
  * peaks  ``max_memory_allocated`` over one run of A and of each B, and the pinned bytes of B's ring.
  * --big  once: 1920 x 1080 at 64 spp (a 55 GB file) through the streamer alone, where the disk and the memory allow it.

    timeout -k 10 900 python scripts/time_denoise_stream.py [--rounds 7] [--big]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, S = 720, 1280, 8
TARGETS = (16 << 20, 64 << 20, 256 << 20)


def _frame_on_disk(fn):
    from data_ref import cmap, make_frame
    x, y = make_frame(H, W, S, seed=0, fill="kpcn", device="cuda:0"), make_frame(H, W, S, seed=1, fill="llpm", device="cuda:0")
    raw = torch.where(torch.isnan(x), y, x)
    del x, y
    raw[..., cmap()["bounce"]][torch.rand((H, W), device="cuda:0") < 0.1] = 0.0
    np.save(fn, raw.cpu().numpy())                                 # (unsanitised: both routes sanitise on the device)


def _spread(v):
    return {"median_s": round(float(np.median(v)), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4),
            "spread_s": round(max(v) - min(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--big", action="store_true", help="only the 1920 x 1080 x 64 spp frame, streamed once")
    ap.add_argument("--tmp", type=str, default=None, help="where the frames are written (default: the system's temporary directory)")
    a = ap.parse_args()
    from wcmc_amd import denoise, train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.datasets import DenoisePreprocessor
    from wcmc_amd.support.staging import FrameStreamer, default_band_rows
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sync = lambda: torch.cuda.synchronize(dev)                     # noqa: E731

    def whole_frame(fn):
        parts, _ = denoise.read_raw(fn)
        raw = denoise.upload_raw(parts, dev)
        pre = DenoisePreprocessor()
        kpcn, llpm = pre._preprocess_kpcn(raw), pre._preprocess_llpm(raw)
        del raw
        sync()
        return kpcn, llpm

    def streamed(fn, target, keep=None):
        frames = FrameStreamer([fn], None, dev, target_bytes=target)
        kpcn, llpm = next(frames)
        sync()
        frames.close()
        if keep is not None:
            keep["ring"] = frames.ring.peak_nbytes
        return kpcn, llpm

    def timed(fn, *args):
        sync()
        t0 = time.perf_counter()
        out = fn(*args)
        return time.perf_counter() - t0, out

    if a.big:
        return big(a, dev)

    with tempfile.TemporaryDirectory(dir=a.tmp) as root:
        fn = os.path.join(root, "frame.npy")
        _frame_on_disk(fn)
        torch.cuda.empty_cache()

        # ---- A against B: the buffers of one frame
        arms = {"A_whole_frame": lambda: whole_frame(fn)}
        for t in TARGETS:
            arms["B_streamed_%dMiB" % (t >> 20)] = (lambda t=t: streamed(fn, t))
        want = None
        for name, arm in arms.items():                             # warm-up of each arm, and the routes agree bit for bit
            got = arm()
            want = want or got
            assert all(torch.equal(g.view(torch.int32), w_.view(torch.int32)) for g, w_ in zip(got, want)), name
        del got, want
        secs = {k: [] for k in arms}
        for _ in range(a.rounds):
            for name, arm in arms.items():
                secs[name].append(timed(arm)[0])
        res = {k: _spread(v) for k, v in secs.items()}
        spread_a = res["A_whole_frame"]["spread_s"]
        for t in TARGETS:
            k = "B_streamed_%dMiB" % (t >> 20)
            res[k]["band_rows"] = default_band_rows(H, W, S, t)
            res[k]["within_A_plus_its_spread"] = bool(res[k]["median_s"] <= res["A_whole_frame"]["median_s"] + spread_a)
        print(json.dumps({"what": "buffers_of_one_frame", "frame": [H, W], "spp": S, "rounds": a.rounds, **res}), flush=True)

        # ---- peaks
        peaks = {}
        for name, arm in arms.items():
            torch.cuda.empty_cache()
            sync()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            keep = {}
            out = streamed(fn, int(name.split("_")[-1][:-3]) << 20, keep) if name.startswith("B") else arm()
            peaks[name] = {"max_memory_allocated_MB": round((torch.cuda.max_memory_allocated() - base) / 1e6, 1),
                           "pinned_ring_MB": round(keep.get("ring", 0) / 1e6, 1)}
            del out
        print(json.dumps({"what": "peaks", "frame": [H, W], "spp": S, "raw_frame_MB": round(H * W * S * 416 / 1e6, 1),
                          "buffers_MB": round(H * W * (44 + 37 * S) * 4 / 1e6, 1), **peaks,
                          "note": "A also holds one pageable host copy of the raw frame; B's host memory is the ring"}), flush=True)

        # ---- C: four frames in one call
        save = os.path.join(root, "w")
        files = [os.path.join(root, "frame_%d.npy" % i) for i in range(4)]
        for f in files:
            os.symlink(fn, f)
        argv = ["--input"] + files + ["--output_dir", os.path.join(root, "out"), "--save", save, "--model_name", "KPCN_timing",
                                      "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--train_branches"]
        args = denoise.build_parser().parse_args(argv)
        os.makedirs(save, exist_ok=True)
        torch.manual_seed(0)
        itfs, _ = train_kpcn.init_model({"dncnn_in_size": 39, "pnet_in_size": 36, "pnet_out_size": 3}, args, dev)
        torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, "KPCN_timing.pth"))
        del itfs
        args = denoise.check_inputs(train_kpcn.check_args(denoise.build_parser().parse_args(argv)))
        itf = denoise.load_interface(args, dev)

        def four_whole():
            per = []
            for f in files:
                t, (kpcn, llpm) = timed(whole_frame, f)
                times = denoise.denoise_buffers(itf, os.path.splitext(os.path.basename(f))[0], kpcn, llpm, args.output_dir, args, t)
                sync()
                per.append(t + times["network"] + times["finish"] + times["write"])
            return per

        def four_streamed():
            frames, per, t0 = FrameStreamer(files, None, dev), [], time.perf_counter()
            try:
                for f in files:
                    denoise.denoise_file(itf, f, args.output_dir, args, dev, frames=frames)
                    sync()
                    per.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
            finally:
                frames.close()
            return per
        four_whole(), four_streamed()                              # warm-up
        rounds = max(3, a.rounds // 2)
        whole, stream = [], []
        for _ in range(rounds):
            whole.append(four_whole())
            stream.append(four_streamed())
        w_tot, s_tot = [sum(p) for p in whole], [sum(p) for p in stream]
        print(json.dumps({"what": "four_frames_in_one_call", "frame": [H, W], "spp": S, "rounds": rounds,
                          "A_four_frames": _spread(w_tot), "C_four_frames": _spread(s_tot),
                          "A_per_frame": _spread([float(np.mean(p)) for p in whole]),
                          "C_first_frame": _spread([p[0] for p in stream]),
                          "C_per_frame_steady_state": _spread([float(np.mean(p[1:])) for p in stream]),
                          "C_over_A": round(float(np.median(s_tot)) / float(np.median(w_tot)), 4)}), flush=True)


def big(a, dev):
    """1920 x 1080 at 64 spp through the streamer, once: the file is written band by band (it never lies in memory here either)."""
    from wcmc_amd.support.staging import FrameStreamer
    h, w, s = 1080, 1920, 64
    nbytes = h * w * s * 416
    root = tempfile.mkdtemp(dir=a.tmp)
    try:
        free_disk = shutil.disk_usage(root).free
        free_mem = os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
        if free_disk < nbytes * 1.05 or free_mem < nbytes * 1.2:
            print(json.dumps({"what": "big_frame", "frame": [h, w], "spp": s, "result": "not measured",
                              "file_GB": round(nbytes / 1e9, 1), "free_disk_GB": round(free_disk / 1e9, 1),
                              "free_memory_GB": round(free_mem / 1e9, 1)}), flush=True)
            return
        fn = os.path.join(root, "big.npy")
        t0 = time.perf_counter()
        out = np.lib.format.open_memmap(fn, mode="w+", dtype=np.float32, shape=(h, w, s, 104))
        tile = np.random.default_rng(0).random((8, w, s, 104), dtype=np.float32)
        for r0 in range(0, h, 8):
            out[r0:r0 + 8] = tile
            if r0 % 120 == 0:
                print("writing the frame: row %d of %d, %.0f s" % (r0, h, time.perf_counter() - t0), file=sys.stderr, flush=True)
        out.flush()
        del out
        t_write = time.perf_counter() - t0
        res = {}
        for run in ("first", "second"):                            # the second reads what the page cache kept
            torch.cuda.empty_cache()
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            frames = FrameStreamer([fn], None, dev)
            kpcn, llpm = next(frames)
            torch.cuda.synchronize(dev)
            t = time.perf_counter() - t0
            frames.close()
            res[run] = {"seconds": round(t, 2), "GB_per_s": round(nbytes / 1e9 / t, 2),
                        "max_memory_allocated_GB": round((torch.cuda.max_memory_allocated() - base) / 1e9, 2),
                        "pinned_ring_MB": round(frames.ring.peak_nbytes / 1e6, 1)}
            del kpcn, llpm
        print(json.dumps({"what": "big_frame", "frame": [h, w], "spp": s, "file_GB": round(nbytes / 1e9, 1),
                          "write_s": round(t_write, 1), "buffers_GB": round(h * w * (44 + 37 * s) * 4 / 1e9, 2), **res}), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
