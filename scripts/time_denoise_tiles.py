"""Timing of wcmc_amd.denoise over tile sizes, pads and feathers on the MI355X, by the method of
scripts/time_denoise.py and scripts/time_self_ensemble.py: every case in ONE process, in interleaved rounds (round r runs every case
once, in turn, after one warm-up run of each), the figures the medians over the rounds beside their min and max.

Per synthetic frame (1280 x 720 and 1920 x 1080 at 8 samples per pixel) and a freshly initialised KPCN-Manifold model, for P in
128, 192, 256, 384, 512 at pad 32 / F 0 and at pad 48 / F 16: tiles, tiles per call (``denoise.tile_batch_size``), the 'network' seconds
of ``support.inference.denoise_frame``, ``torch.cuda.max_memory_allocated`` over the call, and the ratio to the P = 128 / pad 32 row
beside the model ``(P / (P - 2 pad))^2``.  Then ``--self_ensemble`` (all eight codes) at 128 and at the fastest P.  The P = 128 /
pad 32 / F 0 row is the path of profiles/denoise_timing.txt and must agree with its 'network' figure, or the comparison is void.

Seams (``--seams``): the mean absolute step of the denoised radiance across the boundaries of the owned windows over the mean absolute
step between neighbouring pixels elsewhere, with ``--use_llpm_buf``, at F = 0 and F = 16.  The model is untrained.

    timeout -k 10 900 python scripts/time_denoise_tiles.py --commit ID [--rounds 3] [--out profiles/denoise_tiles_timing.txt]
    timeout -k 10 600 python scripts/time_denoise_tiles.py --commit ID --seams [--out profiles/denoise_tiles_seams.txt]
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_denoise_tiles.py --only 384 32 0
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S = 8
FRAMES = [(720, 1280), (1080, 1920)]
TILES = [128, 192, 256, 384, 512]
PADS = [(32, 0), (48, 16)]
PARENT_NETWORK_S = (0.1283, 0.1185)      # profiles/denoise_timing.txt and profiles/self_ensemble_timing.txt: the same path, two sessions


def _frame(h, w, dev):
    from data_ref import cmap, make_frame
    from wcmc_amd import ops
    x, y = make_frame(h, w, S, seed=0, fill="kpcn", device="cuda:0"), make_frame(h, w, S, seed=1, fill="llpm", device="cuda:0")
    raw = torch.where(torch.isnan(x), y, x)
    del x, y
    miss = torch.rand((h, w), device=dev) < 0.1
    raw[..., cmap()["bounce"]][miss] = 0.0
    ops.sanitize_(raw)
    kpcn, llpm = ops.preprocess_kpcn(raw), ops.preprocess_llpm(raw)
    del raw
    torch.cuda.empty_cache()
    return kpcn, llpm


def _model(dev):
    from wcmc_amd import denoise, train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    with tempfile.TemporaryDirectory() as root:
        save = os.path.join(root, "w")
        argv = ["--input", "unused", "--output_dir", "unused", "--save", save, "--model_name", "KPCN_timing", "--use_llpm_buf",
                "--manif_learn", "--manif_loss", "FMSE", "--train_branches"]
        args = denoise.build_parser().parse_args(argv)
        torch.manual_seed(0)
        itfs, _ = train_kpcn.init_model({"dncnn_in_size": 39, "pnet_in_size": 36, "pnet_out_size": 3}, args, dev)
        torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, "KPCN_timing.pth"))
        del itfs
        return denoise.load_interface(train_kpcn.check_args(denoise.build_parser().parse_args(argv)), dev)


def _stat(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timing(a, emit):
    from wcmc_amd import denoise
    from wcmc_amd.support.inference import denoise_frame, frame_tiles
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    itf = _model(dev)
    for h, w in FRAMES:
        kpcn, llpm = _frame(h, w, dev)
        cases = [(p, pad, f) for pad, f in PADS for p in TILES]

        def run(case, codes=(0,)):
            p, pad, f = case
            b = denoise.check_tile_limits(p, pad, S, denoise.tile_batch_size(S, None, p))
            times = {}
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            denoise_frame(itf, kpcn, llpm, True, batch_size=b, patch_size=p, pad_size=pad, blend=f, times=times, ensemble=codes)
            return times["network"], times["tiles"], b, torch.cuda.max_memory_allocated(), base
        for case in cases:                                           # warm-up: every shape's launch plans and allocations
            run(case)
        net = {c: [] for c in cases}
        info = {}
        for _ in range(a.rounds):
            for case in cases:
                n, tiles, b, peak, base = run(case)
                net[case].append(n)
                info[case] = (tiles, b, peak, base)
        ref = float(np.median(net[(128, 32, 0)]))
        spread = (max(net[(128, 32, 0)]) - min(net[(128, 32, 0)])) / ref
        for case in cases:
            p, pad, f = case
            tiles, b, peak, base = info[case]
            assert tiles == len(frame_tiles(h, w, p, pad))
            model = (p / (p - 2.0 * pad)) ** 2 / 4.0
            row = {"what": "tiles", "frame": [h, w], "spp": S, "tile": p, "tile_pad": pad, "blend": f, "tiles": tiles, "tiles_per_call": b,
                   "rounds": a.rounds, "network_s": _stat(net[case]), "over_P128_pad32": round(float(np.median(net[case])) / ref, 4),
                   "model_over_P128_pad32": round(model, 4), "peak_allocated_MiB": round(peak / 2 ** 20, 1),
                   "frame_buffers_MiB": round(base / 2 ** 20, 1)}
            if case == (128, 32, 0):
                row["spread_of_round_medians"] = round(spread, 4)
                if (h, w) == FRAMES[0]:
                    lo, hi = min(PARENT_NETWORK_S), max(PARENT_NETWORK_S)
                    row["parent_network_s"] = list(PARENT_NETWORK_S)
                    row["agrees_with_parent"] = bool(lo * 0.95 <= ref <= hi * 1.05)
            emit(row)
        fastest = min((c for c in cases if c[1:] == (32, 0)), key=lambda c: float(np.median(net[c])))
        ens = {c: [] for c in ((128, 32, 0), fastest)}
        for c in ens:
            run(c, tuple(range(8)))
        for _ in range(a.rounds):
            for c in ens:
                ens[c].append(run(c, tuple(range(8)))[0])
        for c, v in ens.items():
            emit({"what": "self_ensemble, all eight codes", "frame": [h, w], "spp": S, "tile": c[0], "tile_pad": c[1], "blend": c[2],
                  "fastest_tile": c == fastest, "rounds": a.rounds, "network_s": _stat(v),
                  "over_plain_P128": round(float(np.median(v)) / ref, 4)})
        del kpcn, llpm
        torch.cuda.empty_cache()


def only(a):
    """``--only P PAD F``: one warm-up run and five runs of one case on the 1280 x 720 frame, for a `rocprofv3 --kernel-trace --stats`
    run of its own (the kernel that a tile size spends its time in)."""
    from wcmc_amd import denoise
    from wcmc_amd.support.inference import denoise_frame
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    itf = _model(dev)
    kpcn, llpm = _frame(*FRAMES[0], dev)
    p, pad, f = a.only
    for _ in range(6):
        times = {}
        denoise_frame(itf, kpcn, llpm, True, batch_size=denoise.tile_batch_size(S, None, p), patch_size=p, pad_size=pad, blend=f, times=times)
    print(json.dumps({"what": "only", "tile": p, "tile_pad": pad, "blend": f, "network_s_last": round(times["network"], 4)}), flush=True)


def seam_ratio(out, has_hit, table):
    """Mean |step| across the inner boundaries of the owned windows over mean |step| between neighbours elsewhere; steps between
    two hit pixels only (the others hold the noisy input)."""
    img, hit = out.double().cpu().numpy(), has_hit.cpu().numpy() != 0
    res = {}
    for axis, name in ((0, "rows"), (1, "columns")):
        step = np.abs(np.diff(img, axis=axis)).mean(axis=2)
        both = hit[1:] & hit[:-1] if axis == 0 else hit[:, 1:] & hit[:, :-1]
        edges = sorted({r[axis] for r in table if r[axis] > 0})        # i_start / j_start of the tiles that are not first
        seam = np.zeros(step.shape, bool)
        if axis == 0:
            seam[[e - 1 for e in edges], :] = True
        else:
            seam[:, [e - 1 for e in edges]] = True
        res[name] = {"seams": len(edges), "mean_step_across": float(step[seam & both].mean()),
                     "mean_step_elsewhere": float(step[~seam & both].mean()),
                     "ratio": round(float(step[seam & both].mean() / step[~seam & both].mean()), 4)}
    return res


def seams(a, emit):
    from wcmc_amd import denoise
    from wcmc_amd.support.inference import denoise_frame, frame_tiles
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    itf = _model(dev)
    h, w = FRAMES[0]
    kpcn, llpm = _frame(h, w, dev)
    outs = {}
    for p, pad, f in ((128, 32, 0), (128, 48, 0), (128, 48, 16), (256, 32, 0), (256, 48, 0), (256, 48, 16)):
        out, _, has_hit = denoise_frame(itf, kpcn, llpm, True, batch_size=denoise.tile_batch_size(S, None, p), patch_size=p, pad_size=pad,
                                        blend=f)
        emit(dict({"what": "seams", "frame": [h, w], "spp": S, "tile": p, "tile_pad": pad, "blend": f, "model": "untrained KPCN-Manifold"},
                  **seam_ratio(out, has_hit, frame_tiles(h, w, p, pad))))
        outs[(p, pad, f)] = out
    # how far the result depends on the tiling at all (the P-buffer's U-Net sees every tile's zero border): two tilings of one frame
    hit = (has_hit != 0)[..., None].expand_as(out)
    for a_, b_ in (((128, 32, 0), (256, 32, 0)), ((128, 48, 0), (256, 48, 0)), ((256, 48, 0), (256, 48, 16))):
        d = (outs[a_] - outs[b_]).abs()[hit].double()
        emit({"what": "tiling_dependence", "frame": [h, w], "spp": S, "a": list(a_), "b": list(b_), "model": "untrained KPCN-Manifold",
              "mean_abs_difference": float(d.mean()), "max_abs_difference": float(d.max()),
              "mean_abs_value": float(outs[a_].abs()[hit].double().mean())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seams", action="store_true")
    ap.add_argument("--only", type=int, nargs=3, default=None, metavar=("P", "PAD", "F"), help="run one case six times and write no file")
    ap.add_argument("--commit", type=str, default="(no commit given)", help="the commit the tree was measured on (the header line of the file)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.only:
        return only(a)
    out = a.out or os.path.join(ROOT, "profiles", "denoise_tiles_seams.txt" if a.seams else "denoise_tiles_timing.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        if a.seams:
            head = ("# scripts/time_denoise_tiles.py --seams on one MI355X, %s (synthetic 1280 x 720 frame, 8 spp, --use_llpm_buf; the model is "
                    "freshly initialised, NOT trained: nobody has measured this on a trained one)" % a.commit)
        else:
            head = ("# scripts/time_denoise_tiles.py on one MI355X, %s (synthetic frames, 8 spp, freshly initialised KPCN-Manifold model; "
                    "one process, %d interleaved rounds after one warm-up run of every case; network_s: tiles, network, stitching)"
                    % (a.commit, a.rounds))

        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        f.write(head + "\n")
        (seams if a.seams else timing)(a, emit)


if __name__ == "__main__":
    main()
