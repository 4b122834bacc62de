// Sample counts 2..spp from one staged frame.
//
// The reference trains over MSDenoiseDataset (support/datasets.py:1149-1171): one DenoiseDataset per count s = 2..spp, each of
// which reads the first s samples of every frame (:618, :1053-1054, :1091) and runs _preprocess_kpcn (:487-582) on them -- the
// raw frame is read from disk and reduced once per count.  Here the frame is staged once at S = spp samples and
// wcmc_preprocess_kpcn_prefix forms the (h, w, 44) buffer of every count s_lo..s_hi from ONE read of the raw frame.  (A batch at s
// samples out of per-sample buffers that hold S_total is the patch assemblers' own `S_total, s` pair: preprocess.hip, sbmc_data.hip.)
#include "data_step.h"

namespace wcmc {

constexpr int MS_MAX_S = 64;                        // samples per pixel (and so counts) the prefix pass accepts

// pass 1 for every count at once.  A block takes tiles of ppt = 256 / S pixels: thread t reads raw record p0 * S + t (the
// tile's records are consecutive in memory), forms the thirteen per-sample values and leaves them in LDS; then one thread per
// (pixel, count) sums the first s of them in sample order -- mean, then the squared deviations from it, as numpy's mean / var and
// pp_kpcn_stats_kernel do -- and writes that count's sixteen value / variance channels and its workspace pair.  The raw frame is
// read from memory once, whatever the number of counts.  The image maximum of the mean depth is kept per count: block-wide in
// LDS, then one atomicMax per block and count on the slot behind that count's workspace pairs.
template <bool VEC>
__global__ __launch_bounds__(256) void ms_kpcn_prefix_stats_kernel(const float* __restrict__ raw, float* __restrict__ out,
                                                                   float* __restrict__ ws, int64_t npix, int S, int C, int s_lo,
                                                                   int n_counts, PPMap m) {
  __shared__ float vals[256 * KP_NV];               // [record of the tile][value]: odd pitch, conflict-free writes
  __shared__ int smax[MS_MAX_S];
  const int tid = threadIdx.x;
  const int ppt = 256 / S;
  const int64_t ws_stride = 2 * npix + 4, ntiles = (npix + ppt - 1) / ppt;
  if (tid < n_counts) smax[tid] = 0;                // (a non-negative float orders as its bit pattern; 0.0f is 0)
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t p0 = tile * ppt;
    const int npx = (int)min((int64_t)ppt, npix - p0);
    __syncthreads();                                // the last tile's values have been consumed (and smax is initialised)
    if (tid < npx * S) {
      float v[KP_NV];
      pp_kpcn_values<VEC>(raw + (p0 * S + tid) * C, m, v);
#pragma unroll
      for (int c = 0; c < KP_NV; ++c) vals[tid * KP_NV + c] = v[c];
    }
    __syncthreads();
    for (int item = tid; item < npx * n_counts; item += 256) {
      const int pl = item / n_counts, ci = item - pl * n_counts, s = s_lo + ci;
      const float* pv = vals + pl * S * KP_NV;
      const float spp = (float)s;
      float mean[KP_NV], var[KP_NV];
#pragma unroll
      for (int c = 0; c < KP_NV; ++c) mean[c] = 0.f;
      for (int k = 0; k < s; ++k)
#pragma unroll
        for (int c = 0; c < KP_NV; ++c) mean[c] += pv[k * KP_NV + c];
#pragma unroll
      for (int c = 0; c < KP_NV; ++c) { mean[c] = mean[c] / spp; var[c] = 0.f; }
      for (int k = 0; k < s; ++k)
#pragma unroll
        for (int c = 0; c < KP_NV; ++c) { const float d = pv[k * KP_NV + c] - mean[c]; var[c] += d * d; }
#pragma unroll
      for (int c = 0; c < KP_NV; ++c) var[c] = var[c] / spp;
      const int64_t p = p0 + pl;
      pp_kpcn_write_stats(out + ((int64_t)ci * npix + p) * KP_C, ws + ci * ws_stride + 2 * p, mean, var, spp);
      // only the positive part of the maximum matters (datasets.py:517-520 scales when max > 0); fmaxf drops a NaN
      atomicMax(&smax[ci], __float_as_int(fmaxf(mean[3], 0.f)));
    }
  }
  __syncthreads();
  if (tid < n_counts) atomicMax(reinterpret_cast<int*>(ws + tid * ws_stride + 2 * npix), smax[tid]);
}

// pass 2 for every slab: blockIdx.y is the slab, its count s_lo + blockIdx.y
__global__ __launch_bounds__(256) void ms_kpcn_prefix_finish_kernel(float* __restrict__ out, const float* __restrict__ ws, int h,
                                                                    int w, int s_lo) {
  const int64_t npix = (int64_t)h * w;
  pp_kpcn_finish(out + blockIdx.y * npix * KP_C, ws + blockIdx.y * (2 * npix + 4), h, w, s_lo + (int)blockIdx.y);
}

}  // namespace wcmc

using namespace wcmc;

extern "C" size_t wcmc_preprocess_kpcn_prefix_workspace_bytes(int h, int w, int n_counts) {
  if (h <= 0 || w <= 0 || n_counts <= 0) return 0;
  return (size_t)n_counts * ((size_t)2 * h * w + 4) * sizeof(float);
}

extern "C" int wcmc_preprocess_kpcn_prefix(const float* raw, int h, int w, int S, int C, int max_depth, int s_lo, int s_hi,
                                           float* out, void* workspace, size_t workspace_bytes, void* stream) {
  WCMC_REQUIRE(raw && out && workspace && h > 0 && w > 0 && max_depth >= 0 && C >= 38 + 11 * (max_depth + 1), WCMC_ERR_BAD_ARG,
               "preprocess_kpcn_prefix: bad argument");
  WCMC_REQUIRE(1 <= s_lo && s_lo <= s_hi && s_hi <= S && S <= MS_MAX_S, WCMC_ERR_BAD_ARG,
               "preprocess_kpcn_prefix: the counts must satisfy 1 <= s_lo <= s_hi <= S <= 64 (got %d, %d, %d)", s_lo, s_hi, S);
  const int n_counts = s_hi - s_lo + 1;
  WCMC_REQUIRE(workspace_bytes >= wcmc_preprocess_kpcn_prefix_workspace_bytes(h, w, n_counts), WCMC_ERR_WORKSPACE,
               "preprocess_kpcn_prefix: workspace too small");
  const PPMap m = pp_map(max_depth);
  const int64_t npix = (int64_t)h * w;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  for (int ci = 0; ci < n_counts; ++ci)             // one maximum slot per count
    if (hipMemsetAsync(ws + ci * (2 * npix + 4) + 2 * npix, 0, sizeof(float), st) != hipSuccess) {
      set_error("preprocess_kpcn_prefix: memset failed");
      return WCMC_ERR_LAUNCH;
    }
  const int64_t ntiles = ceil_div64(npix, 256 / S);
  const unsigned grid = (unsigned)(ntiles > 4096 ? 4096 : ntiles);
  if (pp_kpcn_vec_ok(raw, C, m))
    hipLaunchKernelGGL(ms_kpcn_prefix_stats_kernel<true>, dim3(grid), dim3(256), 0, st, raw, out, ws, npix, S, C, s_lo, n_counts, m);
  else
    hipLaunchKernelGGL(ms_kpcn_prefix_stats_kernel<false>, dim3(grid), dim3(256), 0, st, raw, out, ws, npix, S, C, s_lo, n_counts, m);
  int rc = check_launch("preprocess_kpcn_prefix(stats)");
  if (rc) return rc;
  hipLaunchKernelGGL(ms_kpcn_prefix_finish_kernel, dim3(pp_grid(npix * KP_C), (unsigned)n_counts), dim3(256), 0, st, out, ws, h, w,
                     s_lo);
  return check_launch("preprocess_kpcn_prefix(finish)");
}
