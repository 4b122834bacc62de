"""Timing of the dihedral self-ensemble of wcmc_amd.denoise on the MI355X (one JSON object per line;
profiles/self_ensemble_timing.txt), on the synthetic 1280 x 720 frame at 8 samples per pixel of
scripts/time_denoise.py and by its method: every arm of a comparison in ONE process, in interleaved rounds (round r runs every arm
once, in turn; hipEvents, median of --reps launches), the figures the medians of the round medians, each ratio next to the spread of
the plain arm's own round medians.

  * kpcn_tiles     ``ops.assemble_kpcn_tiles`` with transform 2, 4, 6 (and 0: the plain call path, the A/A control) against the plain
                   entry point on the same origins: eight in-frame tiles, and the border batch.  Bar: each at most 1.10 x.  Codes 1, 3,
                   5, 7 (origins transposed: those of the turned frame) are recorded without a bar.
  * sample_tiles   the same for ``ops.assemble_sample_tiles``.
  * stitch         ``ops.stitch_tiles_aug`` (an even and an odd code, adding) against ``ops.stitch_tiles`` on one batch.  Recorded.
  * denoise_frame  the 'network' seconds of ``support.inference.denoise_frame`` with all eight codes against the un-ensembled call
                   (a freshly initialised KPCN-Manifold model); the ratio should be about 8.

    timeout -k 10 900 python scripts/time_self_ensemble.py [--reps 20] [--rounds 5] [--frames 3]
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
BAR = 1.10


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


def _report(what, batch, meds, barred, a):
    """One line: every arm's median / min / max of its round medians, its ratio to the 'plain' arm, and for the barred arms the verdict."""
    plain = float(np.median(meds["plain"]))
    spread = (max(meds["plain"]) - min(meds["plain"])) / plain
    arms = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "over_plain": round(float(np.median(v)) / plain, 4)} for k, v in meds.items()}
    for k in barred:
        arms[k]["within_bar"] = bool(arms[k]["over_plain"] <= BAR)
    print(json.dumps({"what": what, "batch": batch, "tiles": 8, "spp": S, "frame": [H, W], "reps": a.reps, "rounds": a.rounds,
                      "bar": BAR if barred else None, "spread_of_plain_round_medians": round(spread, 4), "arms": arms}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=3, help="rounds of the whole-frame comparison")
    a = ap.parse_args()
    from data_ref import cmap, make_frame
    from wcmc_amd import denoise, ops, train_kpcn
    from wcmc_amd.support import checkpoint as ckpt
    from wcmc_amd.support.inference import denoise_frame, frame_tiles
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    x, y = make_frame(H, W, S, seed=0, fill="kpcn", device="cuda:0"), make_frame(H, W, S, seed=1, fill="llpm", device="cuda:0")
    raw = torch.where(torch.isnan(x), y, x)
    del x, y
    miss = torch.rand((H, W), device=dev) < 0.1
    raw[..., cmap()["bounce"]][miss] = 0.0
    ops.sanitize_(raw)
    kpcn, llpm = ops.preprocess_kpcn(raw), ops.preprocess_llpm(raw)
    sbmc_s, sbmc_p = ops.preprocess_sbmc(raw)
    del raw

    inside = torch.tensor([(0, 0), (64, 64), (128, 320), (300, 700), (592, 1152), (13, 977), (400, 31), (256, 512)],
                          dtype=torch.int32, device=dev)
    border = torch.tensor([(-32, -32), (-32, 544), (-32, 1184), (288, -32), (288, 1184), (624, -32), (624, 544), (624, 1184)],
                          dtype=torch.int32, device=dev)
    for name, org in (("in_frame", inside), ("border", border)):
        ops.check_tile_origins(org, H, W, 128, 32)
        turned = org.flip(1).contiguous()                          # the same tiles' origins in the W x H frame of the odd codes
        ops.check_tile_origins(turned, W, H, 128, 32)
        pick = lambda t: turned if t & 1 else org                  # noqa: E731
        arms = {"plain": lambda: ops.assemble_kpcn_tiles(kpcn, llpm, org, 128, 32, check_origins=False)}
        for t in range(8):
            arms["code_%d" % t] = (lambda t=t: ops.assemble_kpcn_tiles(kpcn, llpm, pick(t), 128, 32, check_origins=False, transform=t))
        _report("kpcn_tiles", name, _ab(arms, a.reps, a.rounds), ["code_0", "code_2", "code_4", "code_6"], a)
        arms = {"plain": lambda: ops.assemble_sample_tiles(sbmc_s, sbmc_p, llpm, org, 128, 32, check_origins=False)}
        for t in range(8):
            arms["code_%d" % t] = (lambda t=t: ops.assemble_sample_tiles(sbmc_s, sbmc_p, llpm, pick(t), 128, 32, check_origins=False,
                                                                         transform=t))
        _report("sample_tiles", name, _ab(arms, a.reps, a.rounds), ["code_0", "code_2", "code_4", "code_6"], a)
    del sbmc_s, sbmc_p

    # ---- a freshly initialised KPCN-Manifold model: the shape of its output for the stitch, and the whole frame
    with tempfile.TemporaryDirectory() as root:
        save = os.path.join(root, "w")
        argv = ["--input", "unused", "--output_dir", "unused", "--save", save, "--model_name", "KPCN_timing", "--use_llpm_buf",
                "--manif_learn", "--manif_loss", "FMSE", "--train_branches"]
        args = denoise.build_parser().parse_args(argv)
        torch.manual_seed(0)
        itfs, _ = train_kpcn.init_model({"dncnn_in_size": 39, "pnet_in_size": 36, "pnet_out_size": 3}, args, dev)
        torch.save(ckpt.make_checkpoint(itfs[0], 0, args), os.path.join(save, "KPCN_timing.pth"))
        del itfs
        itf = denoise.load_interface(train_kpcn.check_args(denoise.build_parser().parse_args(argv)), dev)
    itf.to_eval_mode()
    with torch.no_grad():
        out, _ = itf.denoise_batch(ops.assemble_kpcn_tiles(kpcn, llpm, inside, 128, 32, check_origins=False))
    out = out.contiguous()
    table, table_t = frame_tiles(H, W, 128, 32)[:8], frame_tiles(W, H, 128, 32)[:8]
    ops.check_tile_coords(table, H, W, 128)
    ops.check_tile_coords(table_t, W, H, 128)
    coords, coords_t = (torch.tensor(c, dtype=torch.int32, device=dev) for c in (table, table_t))
    out_rad = torch.zeros((3, H, W), device=dev)
    _report("stitch", "first eight tiles, output %d x %d" % tuple(out.shape[2:]),
            _ab({"plain": lambda: ops.stitch_tiles(out, None, coords, out_rad, None, 128),
                 "code_2_add": lambda: ops.stitch_tiles_aug(out, coords, out_rad, 2, True, 128),
                 "code_1_add": lambda: ops.stitch_tiles_aug(out, coords_t, out_rad, 1, True, 128),
                 "code_6_paste": lambda: ops.stitch_tiles_aug(out, coords, out_rad, 6, False, 128)}, a.reps, a.rounds), [], a)
    del out_rad

    # ---- the whole frame: network seconds (tiles, network, stitching), all eight codes against the un-ensembled call
    def network_s(codes):
        times = {}
        denoise_frame(itf, kpcn, llpm, True, batch_size=8, times=times, ensemble=codes)
        return times["network"], times["tiles"]
    for codes in ((0,), tuple(range(8))):
        network_s(codes)                                           # warm-up: both tile tables' shapes have been seen
    plain, full = [], []
    for _ in range(a.frames):
        plain.append(network_s((0,))[0])
        full.append(network_s(tuple(range(8)))[0])
    ratio = float(np.median(full)) / float(np.median(plain))
    print(json.dumps({"what": "denoise_frame", "frame": [H, W], "spp": S, "tile_batch": 8, "rounds": a.frames,
                      "tiles_plain": network_s((0,))[1], "tiles_all_eight": network_s(tuple(range(8)))[1],
                      "network_s_plain": {"median": round(float(np.median(plain)), 4), "min": round(min(plain), 4), "max": round(max(plain), 4)},
                      "network_s_all_eight": {"median": round(float(np.median(full)), 4), "min": round(min(full), 4), "max": round(max(full), 4)},
                      "all_eight_over_plain": round(ratio, 4), "expected": 8, "to_explain_above": round(8 * BAR, 2)}), flush=True)


if __name__ == "__main__":
    main()
