"""Timing of the kernel-splat op on the MI355X (one JSON object per line; profiles/kernel_splat_timing.txt) at the workload's
shape (N, C, h, w, k) = (8, 3, 128, 128, 21): 231 MB of logits per call.

Arms, all in one process, interleaved (round r runs every arm once, in turn; hipEvents around --inner back-to-back calls of the
C ABI on preallocated buffers, median of --reps such windows per round, the figure is the median over the rounds):

  * logit_max                       ``wcmc_logit_max``
  * splat_shift_fwd_into            ``wcmc_kernel_splat_fwd``, shift mode, accumulate = 1 (a sample of ProgressiveKernelApply)
  * splat_shift_bwd                 ``wcmc_kernel_splat_bwd``, shift mode, g_r and g_w, d_logits and d_data
  * splat_softmax_fwd / _bwd        the same in softmax mode (KernelApply(splat=True))
  * gather_fwd / gather_bwd         the unchanged ``wcmc_kernel_apply_fwd`` / ``_bwd`` at the same shape: it streams the same 441 floats
                                    per pixel, and is the yardstick -- every splat arm is stated as a ratio to it
  * fold_shift_fwd / fold_softmax_fwd   the torch expression of the specification (tests/splat_ref.py in fp32: weights, the
                                    (N, C * 441, h * w) product, ``F.fold``), which the fused forward must beat

For an arm slower than twice the gather, the record says where the time goes from the arithmetic of the kernel: logit bytes,
LDS reads and their FMAs, slab bytes.  The 231 MB of logits are re-read by every arm of every round, so
part of them is served by the 256 MB Infinity Cache: the arms compare with each other, not with a cold-HBM roofline.

    timeout -k 10 600 python scripts/time_kernel_splat.py [--reps 10] [--rounds 5] [--inner 10]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, C, H, W, K = 8, 3, 128, 128, 21


def _median_ms(fn, reps, inner):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts))


def _ab(arms, reps, rounds, inner):
    """{name: [median per round]} with the arms interleaved: round r runs every arm once, in turn."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            meds[k].append(_median_ms(fn, reps, 1 if k.startswith("fold") else inner))
    return meds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    from splat_ref import splat_ref
    from wcmc_amd import ops
    from wcmc_amd._lib import check, lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L, k2 = lib(), K * K
    null = ctypes.c_void_p(0)
    g = torch.Generator().manual_seed(0)
    logits = ops.nhwc_empty(N, k2, H, W, dev)
    logits.copy_((torch.rand((N, k2, H, W), generator=g) * 2 - 1) * 3.0)
    data = ((torch.rand((N, C, H, W), generator=g) * 2 - 1) + 0.5).to(dev)
    g_r, g_w = (torch.rand((N, C, H, W), generator=g) * 2 - 1).to(dev), (torch.rand((N, H, W), generator=g) * 2 - 1).to(dev)
    shift = ops.logit_max(logits)
    sum_r, sum_w = torch.zeros((N, C, H, W), device=dev), torch.zeros((N, H, W), device=dev)
    lse = torch.empty(N * H * W, device=dev)
    ws = torch.empty(L.wcmc_kernel_splat_fwd_workspace_bytes(N, C, H, W, k2) // 4, device=dev)
    lws = torch.empty(L.wcmc_logit_max_workspace_bytes(N) // 4, device=dev)
    lmax = torch.empty(N, device=dev)
    dl, dd = ops.nhwc_empty(N, k2, H, W, dev), torch.empty((N, C, H, W), device=dev)
    out, glse = torch.empty((N, C, H, W), device=dev), torch.empty(N * H * W, device=dev)
    gdd = torch.zeros((N, C, H, W), device=dev)
    st, P, V = ops._stream, ops._ptr, ops._v

    def splat_fwd(mode, acc):
        check(L.wcmc_kernel_splat_fwd(*V(logits), P(data), *data.stride(), P(sum_r), P(sum_w), P(lse), mode,
                                      P(shift) if mode else null, acc, P(ws), ws.numel() * 4, N, C, H, W, k2, st()), "splat_fwd")

    def splat_bwd(mode):
        check(L.wcmc_kernel_splat_bwd(*V(logits), P(data), *data.stride(), P(g_r), *g_r.stride(), P(g_w), *g_w.stride(), P(lse), mode,
                                      P(shift) if mode else null, *V(dl), P(dd), N, C, H, W, k2, st()), "splat_bwd")

    def gather_fwd():
        check(L.wcmc_kernel_apply_fwd(*V(logits), P(data), *data.stride(), P(out), *out.stride(), P(glse), N, C, H, W, K, st()), "ka_fwd")

    def gather_bwd(with_data):
        check(L.wcmc_kernel_apply_bwd(*V(logits), P(data), *data.stride(), P(out), *out.stride(), P(g_r), *g_r.stride(), P(glse),
                                      *V(dl), P(gdd) if with_data else null, N, C, H, W, K, st()), "ka_bwd")

    lg_nchw = logits.contiguous()

    def fold(mode):
        with torch.no_grad():
            return splat_ref(data, lg_nchw, shift if mode else None)

    splat_fwd(0, 0)                 # lse of the softmax mode, read by its backward
    gather_fwd()
    # the fused forward computes what the fold route computes (and the timing is of the tested code)
    for mode in (0, 1):
        splat_fwd(mode, 0)
        fr, fw = fold(mode)
        err = max(((sum_r - fr).abs().max() / fr.abs().max()).item(), ((sum_w - fw).abs().max() / fw.abs().max()).item())
        assert err <= 2e-5, (mode, err)
    splat_fwd(0, 0)
    arms = {"logit_max": lambda: check(L.wcmc_logit_max(*V(logits), P(lmax), P(lws), lws.numel() * 4, N, H, W, k2, st()), "logit_max"),
            "splat_shift_fwd_into": lambda: splat_fwd(1, 1), "splat_shift_bwd": lambda: splat_bwd(1),
            "splat_softmax_fwd": lambda: splat_fwd(0, 0), "splat_softmax_bwd": lambda: splat_bwd(0),
            "gather_fwd": gather_fwd, "gather_bwd": lambda: gather_bwd(False), "gather_bwd_with_d_data": lambda: gather_bwd(True),
            "fold_shift_fwd": lambda: fold(1), "fold_softmax_fwd": lambda: fold(0)}
    meds = _ab(arms, a.reps, a.rounds, a.inner)
    med = {k: float(np.median(v)) for k, v in meds.items()}
    px = N * H * W
    logit_mb = 4.0 * px * k2 / 1e6
    tiles = N * ((H + 7) // 8) * ((W + 15) // 16)
    for k, v in meds.items():
        rec = {"what": k, "shape": [N, C, H, W, K], "reps": a.reps, "rounds": a.rounds, "median_ms": round(med[k], 4),
               "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if k.startswith("splat") or k == "logit_max":
            ref = "gather_bwd_with_d_data" if k.endswith("bwd") else "gather_fwd"
            passes = 2 if k.endswith("bwd") else 1
            rec.update({"gather_arm": ref, "ratio_to_gather": round(med[k] / med[ref], 3),
                        "logit_TB_per_s": round(passes * logit_mb / 1e6 / (med[k] / 1e3), 3)})
            if k.endswith("bwd"):
                rec["ratio_to_gather_bwd_without_d_data"] = round(med[k] / med["gather_bwd"], 3)
            if med[k] > 2 * med[ref]:
                rec["where_the_time_goes"] = (
                    "per call: %.0f MB of logits streamed %s (the gather's whole cost); on top of it, per block and source row, the "
                    "gather phase behind a barrier -- %.0f M live LDS float reads in all (441 per source pixel, one per tap) and about as "
                    "many dead ones (a source column reaches 21 of the tile's 36 destination columns), each a mask and two packed FMAs, and "
                    "as many floats of weights written to LDS first; %.1f MB of slabs written and read back by the second launch (%d tiles "
                    "x %d floats); two blocks per CU (57 KB of LDS each)"
                    % (logit_mb, "and as many bytes of d_logits written" if passes == 2 else "once", px * k2 / 1e6,
                       2 * 4.0 * tiles * (C + 1) * 28 * 36 / 1e6, tiles, (C + 1) * 28 * 36))
        if k.startswith("fold"):
            fused = "splat_shift_fwd_into" if "shift" in k else "splat_softmax_fwd"
            rec.update({"fused_arm": fused, "fold_over_fused": round(med[k] / med[fused], 2), "fused_beats_fold": bool(med[fused] < med[k])})
        print(json.dumps(rec), flush=True)
    assert med["splat_shift_fwd_into"] < med["fold_shift_fwd"] and med["splat_softmax_fwd"] < med["fold_softmax_fwd"], \
        "the fused forward must beat the F.fold route"


if __name__ == "__main__":
    main()
