"""The data-step kernels of the sample-based interfaces (csrc/sbmc_data.hip): time and HBM rate per 1280 x 1280 x 8 frame
(preprocess_sbmc, both forms) and per batch of 8 patches of 128 x 128 x 8 (assemble_sample_patches), next to numpy on the same host.
   python3 scripts/time_sbmc_data.py [OUT.txt]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from wcmc_amd import ops

# registers / LDS of the code objects (gfx950, hipcc -O3 --save-temps: .vgpr_count, and the dynamic LDS the launch asks for)
RESOURCES = ("sb_preprocess_tiled_kernel  25 VGPRs, 35,328 B LDS (128 records x 69 floats), no scratch\n"
             "sb_preprocess_kernel        21 VGPRs, no LDS, no scratch\n"
             "sa_assemble_kernel          45 VGPRs, 33,920 B LDS (32 pixels x 265 floats), no scratch")


def timeit(fn, n=10):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def numpy_preprocess_sbmc(x):
    """The arithmetic of DenoiseDataset._preprocess_sbmc (datasets.py:394-452), for the host's time only."""
    total, diffuse = np.maximum(x[..., 2:5], 0), np.maximum(x[..., 5:8], 0)
    spec = np.log(1 + np.maximum(total - diffuse, 0)) / 10.0
    s = np.concatenate([total, np.log(1 + total) / 10.0, spec, x[..., 0:2], x[..., 8:24]], axis=3)
    bt = x[..., 60:66].astype(np.int16)
    tags = [np.bitwise_and(bt, 1 << k).astype(bool).astype(np.float32) for k in range(5)]
    p = np.concatenate([np.log(np.maximum(x[..., 24:48], 0) + 1e-5) / 30.0, np.clip(x[..., 48:60], -1.0, 1.0)] + tags, axis=3)
    return s, p


lines = []
H = W = 1280
S = 8
raw = torch.rand(H, W, S, 104, device="cuda")
raw[..., 60:66] = torch.randint(0, 32, (H, W, S, 6), device="cuda").float()
n = H * W * S
moved = n * (104 + 27 + 66) * 4                     # whole 416-byte records are fetched; both outputs written once
for name, tiled in (("tiled", True), ("generic", False)):
    t = timeit(lambda: ops.preprocess_sbmc(raw, tiled=tiled))
    lines.append("preprocess_sbmc %-7s %dx%d, %d spp (raw %.2f GB): %9.1f us = %5.0f GB/s" % (name, H, W, S, n * 416 / 1e9, t, moved / t / 1e3))
part = raw[:H // 4, :W // 4].contiguous().cpu().numpy()           # 1/16 of the frame: the whole one needs > 20 GB of host temporaries
t0 = time.perf_counter(); ref_s, ref_p = numpy_preprocess_sbmc(part); c = time.perf_counter() - t0
got_s, got_p = ops.preprocess_sbmc(torch.from_numpy(part).cuda())
err = max(float(np.abs(got_s.cpu().numpy() - ref_s).max()), float(np.abs(got_p.cpu().numpy() - ref_p).max()))
lines.append("   numpy on the host, 320x320x8 (1/16 of the frame): %.1f ms -> x 16 = %.1f s per frame   (max |difference| %.1e)" % (c * 1e3, c * 16, err))
del raw

H = W = 512
B, P = 8, 128
raw = torch.rand(H, W, S, 104, device="cuda")
ss, sp = ops.preprocess_sbmc(raw)
ll = ops.preprocess_llpm(raw)
gt = torch.rand(H, W, 9, device="cuda")
del raw
origins = torch.as_tensor(np.random.RandomState(3).randint(0, H - P + 1, size=(B, 2)).astype(np.int32)).cuda()
hs, hp, hl, hg, ho = ss.cpu().numpy(), sp.cpu().numpy(), ll.cpu().numpy(), gt.cpu().numpy(), origins.cpu().numpy()
for name, g, p, l in (("g + sbmc + llpm (F = 91)", True, True, True), ("lbmc: g + llpm (F = 25)", True, False, True)):
    t = timeit(lambda: ops.assemble_sample_patches(ss, sp, ll if l else None, gt, origins, P, g, p, check_origins=False), n=20)
    f = ops.sample_feature_size(g, p, l)
    read = B * P * P * (S * (27 + (66 if p else 0) + (37 if l else 0)) + 9) * 4
    wrote = B * P * P * (S * (3 + f + (36 if l else 0)) + 3) * 4
    t0 = time.perf_counter()
    for r, c in ho:                                   # what __getitem__ + _transpose + the DataLoader's collation do per patch
        w = (slice(r, r + P), slice(c, c + P))
        feats = [hs[w][..., 3:27]] + ([hp[w]] if p else []) + ([hl[w][..., :1]] if l else [])
        np.ascontiguousarray(hs[w][..., :3].transpose(2, 3, 0, 1)); np.ascontiguousarray(np.concatenate(feats, axis=3).transpose(2, 3, 0, 1))
        np.ascontiguousarray(hl[w][..., 1:].transpose(2, 3, 0, 1)); np.ascontiguousarray(hg[w][..., :3].transpose(2, 0, 1))
    c = time.perf_counter() - t0
    lines.append("assemble_sample_patches %-25s batch of %d, %dx%d, %d spp: %8.1f us = %5.0f GB/s (%.0f MB read, %.0f MB written)   numpy on the host %.1f ms"
                 % (name, B, P, P, S, t, (read + wrote) / t / 1e3, read / 1e6, wrote / 1e6, c * 1e3))
print(RESOURCES)
print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("scripts/time_sbmc_data.py: the kernels of csrc/sbmc_data.hip on one MI355X and numpy on the same host (one process)\n"
                + RESOURCES + "\n" + "\n".join(lines) + "\n")
