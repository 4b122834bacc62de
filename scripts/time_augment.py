"""Timing of the dihedral patch augmentation on the MI355X (one JSON object per line; profiles/augment_timing.txt).

  * assemble   eight patches of 128 pixels at 8 samples per pixel out of a synthetic 1280 x 720 frame, for both assemblers
               (``ops.assemble_kpcn_patches`` with llpm, ``ops.assemble_sample_patches`` with every buffer): the plain entry point
               against the ``_aug`` entry point with all codes 0, with each row-preserving code (2, 4, 6: the source of an output row
               is a source row) and with each transposing code (1, 3, 5, 7: the source of an output row is a source column).
               Interleaved arms as in scripts/time_denoise.py: each round times every arm once (hipEvents, median of --reps
               launches); the figures are the medians over the rounds, next to the spread of the plain arm's own round medians.
               Bar: codes 0, 2, 4, 6 within 1.10 x of the plain entry point.  The transposing codes are measured, not barred.
  * loader     the step-to-step time of the graphed KPCN-Manifold step fed by ``PatchLoader`` (the set-up of scripts/time_loader.py:
               512 x 512 frames at 8 spp from host memory), ``augment=False`` against ``augment=True`` in interleaved rounds of one
               epoch each.  Bar: the augmented median exceeds the plain median by no more than the plain arm's round-to-round spread.

    timeout -k 10 900 python scripts/time_augment.py [--reps 30] [--rounds 7] [--loader_rounds 5] [--no_loader]
"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from time_denoise import _ab, _summary  # noqa: E402  (scripts/ is sys.path[0])

H, W, S, P = 720, 1280, 8, 128
ROW_CODES, COLUMN_CODES = (2, 4, 6), (1, 3, 5, 7)


def _report(what, meds, reps, rounds):
    plain = meds["plain"]
    base = float(np.median(plain))
    spread = (max(plain) - min(plain)) / base
    ratios = {k: round(float(np.median(v)) / base, 4) for k, v in meds.items() if k != "plain"}
    barred = ["aug_code_0"] + ["aug_code_%d" % t for t in ROW_CODES]
    print(json.dumps({"what": what, "patches": 8, "patch": P, "spp": S, "frame": [H, W], "reps": reps, "rounds": rounds,
                      **_summary(meds), "over_plain": ratios, "spread_of_plain_round_medians": round(spread, 4),
                      "bar_for_codes_0_2_4_6": 1.10, "within_bar": {k: bool(ratios[k] <= 1.10) for k in barred},
                      "transposing_codes": {"aug_code_%d" % t: ratios["aug_code_%d" % t] for t in COLUMN_CODES},
                      "note": "times include the output allocation of the wrapper, the same in every arm"}), flush=True)


def assemble(a):
    from data_ref import make_frame
    from wcmc_amd import ops
    dev = torch.device("cuda", 0)
    x, y = make_frame(H, W, S, seed=0, fill="kpcn", device="cuda:0"), make_frame(H, W, S, seed=1, fill="llpm", device="cuda:0")
    raw = torch.where(torch.isnan(x), y, x)
    del x, y
    ops.sanitize_(raw)
    kpcn, llpm = ops.preprocess_kpcn(raw), ops.preprocess_llpm(raw)
    sbmc_s, sbmc_p = ops.preprocess_sbmc(raw)
    del raw
    gt = torch.rand((H, W, 9), device=dev) + 1.0
    origins = torch.tensor([(0, 0), (64, 64), (128, 320), (300, 700), (592, 1152), (13, 977), (400, 31), (256, 512)],
                           dtype=torch.int32, device=dev)
    ops.check_patch_origins(origins, H, W, P)
    codes = {t: torch.full((8,), t, dtype=torch.int32, device=dev) for t in range(8)}

    arms = {"plain": lambda: ops.assemble_kpcn_patches(kpcn, llpm, gt, origins, P)}
    for t in range(8):
        arms["aug_code_%d" % t] = lambda t=t: ops.assemble_kpcn_patches(kpcn, llpm, gt, origins, P, transforms=codes[t], check_transforms=False)
    _report("assemble_kpcn_patches", _ab(arms, a.reps, a.rounds), a.reps, a.rounds)

    arms = {"plain": lambda: ops.assemble_sample_patches(sbmc_s, sbmc_p, llpm, gt, origins, P, check_origins=False)}
    for t in range(8):
        arms["aug_code_%d" % t] = lambda t=t: ops.assemble_sample_patches(sbmc_s, sbmc_p, llpm, gt, origins, P, check_origins=False,
                                                                          transforms=codes[t])
    _report("assemble_sample_patches", _ab(arms, a.reps, a.rounds), a.reps, a.rounds)


def loader(a):
    import bench
    import make_golden as mg
    from wcmc_amd.graph import GraphedTrainStep
    from wcmc_amd.support.loader import PatchLoader
    dev = torch.device("cuda", 0)
    h = w = 512
    rng = np.random.RandomState(0)
    images = [{"raw": mg.raw_samples(h, w, S, 10 + i), "gt": rng.rand(h, w, 9).astype(np.float32), "prob": None} for i in range(2)]
    n_img = 6
    loaders = {k: PatchLoader(lambda i: images[i % 2], range(n_img), dev, batch_size=8, patch_size=P, augment=k == "augment")
               for k in ("plain", "augment")}
    with contextlib.redirect_stdout(sys.stderr):             # (the interface announces its loss: keep stdout to the JSON lines)
        itf = bench.build_interface(dev, None, rng="device")
    first = next(iter(loaders["plain"]))
    step = GraphedTrainStep(itf, first)

    def epoch(ld):
        """ms per step of one pass; the clock starts when the first batch is there (scripts/time_loader.py)."""
        step.after_enqueue = ld.kick
        it = iter(ld)
        b = next(it)
        torch.cuda.synchronize()
        t0, nb = time.perf_counter(), 0
        while b is not None:
            step(b)
            nb += 1
            b = next(it, None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / nb * 1e3, nb
    for ld in loaders.values():                              # warm-up: pinned allocations, both kernels loaded
        epoch(ld)
    ms = {k: [] for k in loaders}
    for _ in range(a.loader_rounds):
        for k, ld in loaders.items():
            t, nb = epoch(ld)
            ms[k].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = max(ms["plain"]) - min(ms["plain"])
    print(json.dumps({"what": "loader", "frame": [h, w], "spp": S, "images": n_img, "steps_per_epoch": nb, "rounds": a.loader_rounds,
                      "ms_per_step": {k: [round(t, 4) for t in v] for k, v in ms.items()},
                      "median_ms_per_step": {k: round(v, 4) for k, v in med.items()},
                      "augment_minus_plain_ms": round(med["augment"] - med["plain"], 4),
                      "plain_round_to_round_spread_ms": round(spread, 4),
                      "within_bar": bool(med["augment"] - med["plain"] <= spread)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loader_rounds", type=int, default=5)
    ap.add_argument("--no_loader", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    assemble(a)
    torch.cuda.empty_cache()
    if not a.no_loader:
        loader(a)


if __name__ == "__main__":
    main()
