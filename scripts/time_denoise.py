"""Timing of denoising a render on the MI355X (one JSON object per line; profiles/denoise_timing.txt), on a synthetic
1280 x 720 frame at 8 samples per pixel:

  * assemble     ``ops.assemble_kpcn_tiles`` against ``ops.assemble_kpcn_patches`` (the kernel it restates, plus three target planes)
                 on the same eight in-frame origins, and on a border batch (origins at -32: mirrored reads, differences retaken).
                 Alternating arms: each round times A then B (hipEvents, median of --reps launches); the figures are the medians
                 over the rounds, next to the spread of the existing kernel's own round medians.
  * finish       ``ops.finish_frame`` (without and with the two previews) against the torch expressions it replaces (``full_ipt``
                 and ``has_hit`` as ``FullImageDataset`` computes them, ``torch.where`` as ``evaluate`` does), the same way.
  * denoise      the phases of ``wcmc_amd.denoise`` on the frame written to a temporary directory (a freshly initialised
                 KPCN-Manifold model): upload, preprocess, network, finish; median of --runs runs after one warm-up run, and tiles/s
                 of the network phase.

    timeout -k 10 900 python scripts/time_denoise.py [--reps 30] [--rounds 7] [--runs 4]
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

H, W, S = 720, 1280, 8


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _ab(arms, reps, rounds):
    """{name: [median per round]} with the arms interleaved: round r runs every arm once, in turn."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            meds[k].append(_median_ms(fn, reps))
    return meds


def _summary(meds):
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in meds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--no_denoise", action="store_true")
    a = ap.parse_args()
    from data_ref import cmap, make_frame
    from wcmc_amd import denoise, ops, train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    x, y = make_frame(H, W, S, seed=0, fill="kpcn", device="cuda:0"), make_frame(H, W, S, seed=1, fill="llpm", device="cuda:0")
    raw = torch.where(torch.isnan(x), y, x)
    del x, y
    miss = torch.rand((H, W), device=dev) < 0.1
    raw[..., cmap()["bounce"]][miss] = 0.0
    host_raw = raw.cpu().numpy()                                   # (unsanitised: the command sanitises on the device)
    ops.sanitize_(raw)
    kpcn, llpm = ops.preprocess_kpcn(raw), ops.preprocess_llpm(raw)
    del raw
    gt = torch.zeros((H, W, 9), device=dev)

    # ---- assemble: the same eight in-frame origins through both kernels; then a border batch
    inside = torch.tensor([(0, 0), (64, 64), (128, 320), (300, 700), (592, 1152), (13, 977), (400, 31), (256, 512)],
                          dtype=torch.int32, device=dev)
    border = torch.tensor([(-32, -32), (-32, 544), (-32, 1184), (288, -32), (288, 1184), (624, -32), (624, 544), (624, 1184)],
                          dtype=torch.int32, device=dev)
    ops.check_patch_origins(inside, H, W, 128)
    ops.check_tile_origins(border, H, W, 128, 32)
    meds = _ab({"assemble_kpcn_patches": lambda: ops.assemble_kpcn_patches(kpcn, llpm, gt, inside, 128),
                "assemble_kpcn_tiles": lambda: ops.assemble_kpcn_tiles(kpcn, llpm, inside, 128, 32, check_origins=False),
                "assemble_kpcn_tiles_border": lambda: ops.assemble_kpcn_tiles(kpcn, llpm, border, 128, 32, check_origins=False)}, a.reps, a.rounds)
    old, new = meds["assemble_kpcn_patches"], meds["assemble_kpcn_tiles"]
    spread = (max(old) - min(old)) / float(np.median(old))
    ratio = float(np.median(new)) / float(np.median(old))
    print(json.dumps({"what": "assemble", "tiles": 8, "spp": S, "frame": [H, W], "reps": a.reps, "rounds": a.rounds,
                      **_summary(meds), "tiles_over_patches": round(ratio, 4),
                      "spread_of_patches_round_medians": round(spread, 4), "allowed_ratio": round(1 + max(0.10, spread), 4),
                      "within_bar": bool(ratio <= 1 + max(0.10, spread)),
                      "note": "times include the output allocation of both wrappers; the patches kernel writes three target planes more"}),
          flush=True)

    # ---- finish: the kernel against the torch expressions it replaces
    out_rad = torch.rand((3, H, W), device=dev)

    def torch_finish():
        hit = (llpm[..., 1:].mean(2)[..., 24:25] != 0.0).float()
        has_hit = torch.cat((hit,) * 3, dim=2)
        full_ipt = kpcn[..., :3] * (kpcn[..., 34:37] + 0.00316) + torch.exp(kpcn[..., 10:13]) - 1
        return torch.where(has_hit == 0, full_ipt, out_rad.permute(1, 2, 0))
    meds = _ab({"torch_expressions": torch_finish, "finish_frame": lambda: ops.finish_frame(out_rad, kpcn, llpm),
                "finish_frame_with_previews": lambda: ops.finish_frame(out_rad, kpcn, llpm, preview=True)}, a.reps, a.rounds)
    ratio = float(np.median(meds["finish_frame"])) / float(np.median(meds["torch_expressions"]))
    print(json.dumps({"what": "finish", "spp": S, "frame": [H, W], "reps": a.reps, "rounds": a.rounds, **_summary(meds),
                      "finish_over_torch": round(ratio, 4), "faster": bool(ratio < 1)}), flush=True)
    if a.no_denoise:
        return
    del kpcn, llpm, gt, out_rad

    # ---- the command, phase by phase
    with tempfile.TemporaryDirectory() as root:
        np.save(os.path.join(root, "frame.npy"), host_raw)
        del host_raw
        save = os.path.join(root, "w")
        argv = ["--input", os.path.join(root, "frame.npy"), "--output_dir", os.path.join(root, "out"), "--save", save, "--model_name",
                "KPCN_timing", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--train_branches"]
        args = denoise.build_parser().parse_args(argv)
        torch.manual_seed(0)
        itfs, _ = train_kpcn.init_model({"dncnn_in_size": 39, "pnet_in_size": 36, "pnet_out_size": 3}, args, dev)
        torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, "KPCN_timing.pth"))
        del itfs
        args = denoise.check_inputs(train_kpcn.check_args(denoise.build_parser().parse_args(argv)))
        itf = denoise.load_interface(args, dev)
        runs = [denoise.denoise_file(itf, args.input[0], args.output_dir, args, dev) for _ in range(a.runs + 1)]
    phases = ("upload", "preprocess", "network", "finish", "write")
    med = {p: float(np.median([r[p] for r in runs[1:]])) for p in phases}
    print(json.dumps({"what": "denoise", "frame": [H, W], "spp": S, "tiles": runs[0]["tiles"], "tile_batch": 8, "runs": a.runs,
                      "median_s": {p: round(med[p], 4) for p in phases},
                      "warm_up_run_s": {p: round(runs[0][p], 4) for p in phases},
                      "tiles_per_s": round(runs[0]["tiles"] / med["network"], 1),
                      "for_scale": "profiles/eval_timing.txt: evaluate.denoise takes 0.59 s per call on a 1280 x 1280 frame at 8 spp "
                                   "(361 tiles of which it keeps the inner 72-pixel crop; preprocessed files read from disk)"}),
          flush=True)


if __name__ == "__main__":
    main()
