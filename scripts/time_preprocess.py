"""Data-step kernels at the benchmark patch size: time, HBM rate, numpy baseline.
   python3 scripts/time_preprocess.py"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
import numpy as np, torch
from wcmc_amd.support.datasets import DenoisePreprocessor
import make_golden as mg
from oracle import datasets as od          # numpy restatement = the CPU baseline ("port")

def timeit(fn, n=20):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3

pre = DenoisePreprocessor()
for h, s in ((128, 8), (512, 8)):
    raw = mg.raw_samples(h, h, s, 5)
    x = torch.from_numpy(raw).cuda()
    nsamp = h * h * s
    t1 = timeit(lambda: pre._preprocess_llpm(x))
    t2 = timeit(lambda: pre._preprocess_kpcn(x))
    rb = nsamp * 104 * 4
    b1 = rb + nsamp * 37 * 4                      # raw records are interleaved: whole 416-byte records are fetched
    b2 = rb + h * h * 44 * 4
    print("%4dx%-4d s=%d  llpm %7.1f us = %5.0f GB/s   kpcn %7.1f us = %5.0f GB/s   (raw %.1f MB)" %
          (h, h, s, t1, b1 / t1 / 1e3, t2, b2 / t2 / 1e3, rb / 1e6))
    if h == 128:
        t0 = time.perf_counter(); od.preprocess_llpm(raw); c1 = time.perf_counter() - t0
        t0 = time.perf_counter(); od.preprocess_kpcn(raw); c2 = time.perf_counter() - t0
        print("   numpy on the host (1 thread): llpm %.1f ms, kpcn %.1f ms" % (c1 * 1e3, c2 * 1e3))

# ---- sampling maps (csrc/sampling_map.hip): kernel time per 1280 x 1280 frame, next to the scipy restatement of the reference's
# gradient_importance_map (support/datasets.py:17-36) on this host.   python3 scripts/time_preprocess.py [OUT.txt]
from scipy.ndimage import gaussian_filter, sobel
from wcmc_amd import ops

def scipy_importance_map(img):
    planes = [img] if img.ndim == 2 else [img[:, :, c] for c in range(img.shape[2])]
    acc = 0
    for p in planes:
        b = gaussian_filter(p, 31)
        gx, gy = sobel(b, axis=0, mode='nearest'), sobel(b, axis=1, mode='nearest')
        acc = acc + gx * gx + gy * gy
    v = np.sqrt(acc)
    return (v - v.min()) / (v.max() - v.min() + 1e-5)

lines = []
H = W = 1280
rng = np.random.RandomState(7)
for name, shape in (("gray", (H, W)), ("rgb", (H, W, 3))):
    img = rng.rand(*shape).astype(np.float32)
    x = torch.from_numpy(img).cuda()
    t = timeit(lambda: ops.importance_map(x), n=10)
    t0 = time.perf_counter(); ref = scipy_importance_map(img); c = time.perf_counter() - t0
    err = float(np.abs(ops.importance_map(x).cpu().numpy() - ref).max())
    lines.append("importance_map %-4s %dx%d: kernels %8.1f us   scipy on the host %8.1f ms   (max |difference| %.1e)"
                 % (name, H, W, t, c * 1e3, err))
S = 8
raw = torch.rand(H, W, S, 104, device="cuda")
raw[..., 60] = torch.randint(0, 20, (H, W, S), device="cuda").float()
gt = torch.rand(H, W, 9, device="cuda") * 4.0
t = timeit(lambda: ops.sampling_prob(raw, gt, 128), n=10)
lines.append("sampling_prob  %dx%d, %d spp (raw %.1f GB on the device): kernels %8.1f us" % (H, W, S, raw.numel() * 4 / 1e9, t))
print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("scripts/time_preprocess.py: the sampling-map kernels per 1280 x 1280 frame (MI355X) and the scipy restatement\n"
                "of gradient_importance_map on the same host (one process, scipy's own threading)\n" + "\n".join(lines) + "\n")
