"""What the bars of tests/test_gpu_step_tail.py are set from: FeatureMSE / GRS, kernel apply and recombine, forward and
backward, against the CPU oracle in fp64 -- per case the product's distance, the fp32 CPU oracle's distance on the same inputs,
their ratio (over max(fp32 oracle, floor, arithmetic bound)) and the bar the test applies.

Runs the test file's own case functions with the assertions off, so that every figure is printed even where a bar is missed.

    python3 scripts/step_tail_fp64.py > profiles/r08_step_tail_fp64.txt
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

torch.set_num_threads(min(16, os.cpu_count() or 1))

if __name__ == "__main__":
    import test_gpu_step_tail as t
    t.ASSERT = False
    t0 = time.time()
    print("# tests/test_gpu_step_tail.py: distance to the fp64 CPU oracle of the product and of the fp32 CPU oracle, same inputs")
    print("# max-norm relative to the tensor's max (losses: relative; recombine: entry by entry); ratio = product / max(fp32 oracle, floor, bound)")
    print("# K_BAR %g  FLOOR %g  FLOOR_RECOMBINE %g  LSE_ULP %g  cap %g" % (t.K_BAR, t.FLOOR, t.FLOOR_RECOMBINE, t.LSE_ULP, t.CONTRACT))
    for shape in t.FM_SHAPES:
        t.run_feature_mse(shape)
    for shape in t.FM_SHAPES:
        for alpha in t.GRS_ALPHAS:
            t.run_grs(shape, alpha)
    for shape in (t.FM_BIG[0], t.FM_SMALL[1], t.FM_SMALL[3]):
        t.run_grs_overflow(shape)
    t.run_two_live_nodes()
    for name in t.KA_CASES:
        t.run_kernel_apply(name)
    for shape in t.RC_SHAPES:
        t.run_recombine(shape)
    print("#")
    for kernel in ("FeatureMSE", "GRS", "kernel_apply", "recombine"):
        rows = [r for r in t.RECORDS if r[0] == kernel]
        worst = max(rows, key=lambda r: r[3] / r[5])
        far = max(rows, key=lambda r: r[3])
        print("# %-12s %3d figures; largest product distance %.3e (fp32 oracle on it %.3e: %s %s); largest product / bar %.3f = ratio %.2f of %g (%s %s); over the bar: %d"
              % (kernel, len(rows), far[3], far[4], far[1], far[2], worst[3] / worst[5], t.K_BAR * worst[3] / worst[5], t.K_BAR,
                 worst[1], worst[2], sum(1 for r in rows if not r[3] <= r[5])))
    print("# wall time %.0f s, of which the fp64 + fp32 oracles %.0f s (%d host threads)" % (time.time() - t0, t.ORACLE_SECONDS[0], torch.get_num_threads()))
