"""Timing of denoising a render with a sample-based model on the MI355X (one JSON object per line;
profiles/denoise_sample_timing.txt), on a synthetic 1280 x 720 frame at 8 samples per pixel, in the manner of scripts/time_denoise.py:

  * assemble     ``ops.assemble_sample_tiles`` against ``ops.assemble_sample_patches`` (the kernel it restates, plus the target planes)
                 on the same eight in-frame origins, all buffers (use_g_buf, use_sbmc_buf, llpm), and on a border batch (origins at
                 -32: mirrored reads).  Alternating arms: each round times every arm in turn (hipEvents, median of --reps launches);
                 the figures are the medians over the rounds, next to the spread of the existing kernel's own round medians.
                 THE BAR: tiles / patches <= 1.10 on the in-frame origins.
  * finish       ``ops.finish_sample_frame`` (without and with the two previews) against the torch expressions it replaces (``full_ipt``
                 and ``has_hit`` as ``SampleFullImageDataset`` computes them, ``torch.where`` as ``evaluate`` does), the same way.
  * denoise      the phases of ``wcmc_amd.denoise`` on the frame written to a temporary directory, with a freshly initialised SBMC model
                 around ``tests/standins.py: SampleDenoiserStandIn``: upload, preprocess, network, finish; median of --runs runs after one
                 warm-up run.  The network seconds are the stand-in's (a two-layer 3x3 chain) and say nothing about a real denoiser.

    timeout -k 10 900 python scripts/time_denoise_sample.py [--reps 30] [--rounds 7] [--runs 3]
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

from time_denoise import _ab, _summary  # noqa: E402

H, W, S = 720, 1280, 8
BAR = 1.10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no_denoise", action="store_true")
    a = ap.parse_args()
    from data_ref import cmap, make_frame
    from wcmc_amd import denoise, ops, train_kpcn, train_sbmc
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.datasets import dncnn_in_size
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    x, y = make_frame(H, W, S, seed=0, fill="kpcn", device="cuda:0"), make_frame(H, W, S, seed=1, fill="llpm", device="cuda:0")
    raw = torch.where(torch.isnan(x), y, x)
    del x, y
    raw = torch.where(torch.isnan(raw), torch.rand_like(raw), raw)     # (the sbmc-only channels: probabilities, light directions)
    miss = torch.rand((H, W), device=dev) < 0.1
    raw[..., cmap()["bounce"]][miss] = 0.0
    host_raw = None if a.no_denoise else raw.cpu().numpy()            # (unsanitised: the command sanitises on the device)
    ops.sanitize_(raw)
    (sbmc_s, sbmc_p), llpm = ops.preprocess_sbmc(raw), ops.preprocess_llpm(raw)
    del raw
    gt = torch.zeros((H, W, 9), device=dev)

    # ---- assemble: the same eight in-frame origins through both kernels; then a border batch
    inside = torch.tensor([(0, 0), (64, 64), (128, 320), (300, 700), (592, 1152), (13, 977), (400, 31), (256, 512)],
                          dtype=torch.int32, device=dev)
    border = torch.tensor([(-32, -32), (-32, 544), (-32, 1184), (288, -32), (288, 1184), (624, -32), (624, 544), (624, 1184)],
                          dtype=torch.int32, device=dev)
    ops.check_patch_origins(inside, H, W, 128)
    ops.check_tile_origins(border, H, W, 128, 32)
    meds = _ab({"assemble_sample_patches": lambda: ops.assemble_sample_patches(sbmc_s, sbmc_p, llpm, gt, inside, 128, check_origins=False),
                "assemble_sample_tiles": lambda: ops.assemble_sample_tiles(sbmc_s, sbmc_p, llpm, inside, 128, 32, check_origins=False),
                "assemble_sample_tiles_border": lambda: ops.assemble_sample_tiles(sbmc_s, sbmc_p, llpm, border, 128, 32,
                                                                                  check_origins=False)}, a.reps, a.rounds)
    old, new = meds["assemble_sample_patches"], meds["assemble_sample_tiles"]
    ratio = float(np.median(new)) / float(np.median(old))
    print(json.dumps({"what": "assemble", "tiles": 8, "spp": S, "frame": [H, W], "reps": a.reps, "rounds": a.rounds,
                      **_summary(meds), "tiles_over_patches": round(ratio, 4),
                      "spread_of_patches_round_medians": round((max(old) - min(old)) / float(np.median(old)), 4),
                      "bar": BAR, "within_bar": bool(ratio <= BAR),
                      "note": "times include the output allocation of both wrappers; the patches kernel writes the target planes more"}),
          flush=True)

    # ---- finish: the kernel against the torch expressions it replaces
    out_rad = torch.rand((3, H, W), device=dev)

    def torch_finish():
        hit = (llpm[..., 1:].mean(2)[..., 24:25] != 0.0).float()
        has_hit = torch.cat((hit,) * 3, dim=2)
        full_ipt = sbmc_s[..., :3].mean(2)
        return torch.where(has_hit == 0, full_ipt, out_rad.permute(1, 2, 0))
    meds = _ab({"torch_expressions": torch_finish, "finish_sample_frame": lambda: ops.finish_sample_frame(out_rad, sbmc_s, llpm),
                "finish_sample_frame_with_previews": lambda: ops.finish_sample_frame(out_rad, sbmc_s, llpm, preview=True)},
               a.reps, a.rounds)
    ratio = float(np.median(meds["finish_sample_frame"])) / float(np.median(meds["torch_expressions"]))
    print(json.dumps({"what": "finish", "spp": S, "frame": [H, W], "reps": a.reps, "rounds": a.rounds, **_summary(meds),
                      "finish_over_torch": round(ratio, 4), "faster": bool(ratio < 1)}), flush=True)
    if a.no_denoise:
        return
    del sbmc_s, sbmc_p, llpm, gt, out_rad

    # ---- the command, phase by phase
    with tempfile.TemporaryDirectory() as root:
        np.save(os.path.join(root, "frame.npy"), host_raw)
        del host_raw
        save = os.path.join(root, "w")
        argv = ["--input", os.path.join(root, "frame.npy"), "--output_dir", os.path.join(root, "out"), "--save", save, "--model_name",
                "SBMC_timing", "--denoiser", "standins:SampleDenoiserStandIn", "--use_llpm_buf"]
        args = denoise.build_parser().parse_args(argv)
        torch.manual_seed(0)
        sizes = {"dncnn_in_size": dncnn_in_size("sbmc", True, False, True, 0), "pnet_in_size": 36, "pnet_out_size": 0}
        itfs, _ = train_sbmc.init_model(sizes, args, dev)
        ckpt.save_checkpoint(os.path.join(save, "SBMC_timing.pth"), itfs[0], 0, args)
        del itfs
        args = denoise.check_inputs(train_kpcn.check_args(denoise.build_parser().parse_args(argv)))
        itf = denoise.load_interface(args, dev)
        runs = [denoise.denoise_file(itf, args.input[0], args.output_dir, args, dev) for _ in range(a.runs + 1)]
    phases = ("upload", "preprocess", "network", "finish", "write")
    med = {p: float(np.median([r[p] for r in runs[1:]])) for p in phases}
    print(json.dumps({"what": "denoise", "model": "SBMC (g-buffer + llpm, no sbmc buffer) around the two-layer stand-in denoiser",
                      "frame": [H, W], "spp": S, "tiles": runs[0]["tiles"], "tile_batch": 8, "runs": a.runs,
                      "median_s": {p: round(med[p], 4) for p in phases},
                      "warm_up_run_s": {p: round(runs[0][p], 4) for p in phases},
                      "note": "'network' is tiles + PathNet + the stand-in denoiser + stitching: the stand-in's time means nothing for "
                              "a real denoiser; 'preprocess' is 0 by construction (no finish pass: the bands' kernels run inside 'upload')"}),
          flush=True)


if __name__ == "__main__":
    main()
