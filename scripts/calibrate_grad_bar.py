"""The per-tensor gradient bars of tests/test_gpu_bench_config.py on more than one draw.

The benchmarked step's parameter gradients are compared per tensor, by relative L2 and 1 - cosine, with two CPU oracles run on the
same weights, batches and pairings: the fp32 oracle (what the reference computes) and the same oracle in fp64 (the yardstick).
This script runs the test's own comparison (``parity_report``) for several seeds (weights, biases, weight_g, batches and pairing
keys all move) in the default arithmetic AND in exact fp32 MFMA, and prints three distances per draw and mode: product vs fp64,
fp32 oracle vs fp64 (the draw's own fp32 sensitivity: no product kernel moves it) and product vs fp32 oracle (the rounds 5-6
column).  For exact fp32 it also prints the worst per-tensor ratio of the product's distance to fp64 over the fp32 oracle's,
for a few floors: the exact-fp32 bar is a small multiple of it.

    python3 scripts/calibrate_grad_bar.py [NSEEDS] [FIRST] [MODES] > profiles/r07_grad_bar_fp64.txt
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

torch.set_num_threads(min(16, os.cpu_count() or 1))
FLOORS = (5e-5, 1e-4, 2e-4, 5e-4)

if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    modes = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    import test_gpu_bench_config as t
    from wcmc_amd import ops
    print("# worst parameter-gradient tensors of the benchmarked step, two steps, weight-normalised PathNets, B=8 128x128 S=8")
    print("# columns: relative L2 (1 - cos) of product vs fp64 oracle | fp32 oracle vs fp64 | product vs fp32 oracle")
    worst = {}
    for mode in (modes or (ops.MODES[0], "fp32")):
        emulate = mode.endswith("+F")                 # rung F: hidden KPCN activations rounded to fp16 (scripts/arith_trajectories.py)
        if emulate:
            sys.path.insert(0, os.path.join(ROOT, "scripts"))
            from arith_trajectories import round_hidden_to_f16
        ops.EMULATE_HIDDEN = round_hidden_to_f16 if emulate else None
        ops.set_precision(mode[:-2] if emulate else mode)
        os.environ["WCMC_PRECISION"] = mode[:-2] if emulate else mode           # (the test asserts the mode it was started in)
        for seed in range(first, first + n):
            t0 = time.time()
            report, fails, _ = t.parity_report("device", True, seed=seed)
            grads = [r for r in report if " grad " in r[0]]
            a = max(grads, key=lambda r: r[4])
            y = max(grads, key=lambda r: r[6])
            o = max(grads, key=lambda r: r[1])
            print("  %-10s seed %d   product vs fp64 %.3e (%.2e)  fp32 oracle vs fp64 %.3e (%.2e)  product vs fp32 oracle %.3e (%.2e)   [%.0f s]"
                  % (mode, seed, a[4], max(r[5] for r in grads), y[6], max(r[7] for r in grads), o[1], max(r[2] for r in grads),
                     time.time() - t0))
            print("      worst vs fp64: %s (fp32 oracle on it %.3e); fp32 oracle's worst: %s; worst vs fp32 oracle: %s" % (a[0], a[6], y[0], o[0]))
            for r in sorted(grads, key=lambda r: -r[4])[1:6]:
                print("      next vs fp64: %.3e  %.2e  (fp32 oracle %.3e)  %s" % (r[4], r[5], r[6], r[0]))
            ratios = []
            for f in FLOORS:
                r = max(grads, key=lambda r: r[4] / max(r[6], f))
                ratios.append("floor %.0e: %.2f (%s)" % (f, r[4] / max(r[6], f), r[0]))
            print("      worst per-tensor ratio product/fp32-oracle distance to fp64, " + "; ".join(ratios))
            print("      default-mode form: worst vs fp64 / max(fp32 oracle's worst, 5e-4) = %.2f" % (a[4] / max(y[6], 5e-4)))
            print("      other failures (losses, outputs, parameter deltas): %d %s" % (len(fails), fails[:2]))
            outs = [r for r in report if " out " in r[0]]
            print("      denoised patches, worst max-norm error against the fp32 oracle %.3e" % max(r[1] for r in outs))
            sys.stdout.flush()
            w = worst.setdefault(mode, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], a[4]), max(w[1], y[6]), max(w[2], o[1])
    for mode, (a, y, o) in worst.items():
        print("# %s over %d seeds: largest relative L2 vs fp64 %.3e, fp32 oracle vs fp64 %.3e, vs fp32 oracle %.3e" % (mode, n, a, y, o))
