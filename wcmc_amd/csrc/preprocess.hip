// Per-image preprocessing of raw renderer samples (the step before the KPCN-Manifold path).
//
// Replaces the numpy code of the reference's support/datasets.py:
//   DenoiseDataset._preprocess_llpm :302-361   raw (h,w,s,C) -> (h,w,s,37) path descriptors (log / sqrt transforms)
//   DenoiseDataset._preprocess_kpcn :487-582   raw (h,w,s,C) -> (h,w,44) per-pixel statistics over the spp axis,
//                                              albedo factorisation, log transform, depth normalisation, gradients
//   DenoiseDataset._gradients       :286-300   backward differences with a zero first column / row
// Raw channel map: datasets.py:223-267 (C = 38 + 11 * (MAX_DEPTH + 1) = 104 at MAX_DEPTH = 5).
// All three are streaming, HBM-bound kernels: the raw buffer (416 B per sample) is read once per function.
#include "data_step.h"

namespace wcmc {

// generic form: one thread per (sample, output channel)
__device__ __forceinline__ float pp_llpm_value(const float* r, int c, const PPMap& m, int base) {
  // r: the sample's raw record shifted by `base` channels (0 for a global pointer, m.bounce for the LDS tile)
  if (c < 1) return logf(r[m.pweight - base] + 1e-6f) / 90.0f;
  if (c < 4) return logf(r[m.rwow + c - 1 - base] + 1e-6f) / 30.0f;
  if (c < 7) return logf(r[m.light + c - 4 - base] + 1e-8f) / 10.0f;
  if (c < 7 + 3 * m.d) return logf(r[m.thr + c - 7 - base] + 1e-6f) / 30.0f;
  if (c < 7 + 4 * m.d) return r[m.bounce + c - 7 - 3 * m.d - base] / 19.0f;
  return sqrtf(r[m.rough + c - 7 - 4 * m.d - base]);
}

__global__ __launch_bounds__(256) void pp_llpm_kernel(const float* __restrict__ raw, float* __restrict__ out, int64_t n,
                                                      int C, PPMap m) {
  const int OC = 7 + 5 * m.d;                       // 1 + 3 + 3 + 3d + d + d
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n * OC;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / OC;
    out[idx] = pp_llpm_value(raw + i * C, (int)(idx - i * OC), m, 0);
  }
}

// Tiled form (16-byte aligned records): every channel the function reads lies in [bounce, C) -- 44 of the 104
// channels at MAX_DEPTH 5.  A block stages that range of 256 consecutive samples in LDS with 16-byte loads
// (176-byte runs per record; the first 240 bytes of a record are never requested), then writes the 256 x 37
// outputs as one contiguous run.
__global__ __launch_bounds__(256) void pp_llpm_tiled_kernel(const float* __restrict__ raw, float* __restrict__ out,
                                                            int64_t n, int C, PPMap m) {
  extern __shared__ __attribute__((aligned(16))) float pp_tile[];
  const int W4 = (C - m.bounce) / 4;                // float4 per record (11)
  const int LD = W4 * 4 + 1;                        // odd row pitch: conflict-free column reads
  const int OC = 7 + 5 * m.d;
  for (int64_t s0 = (int64_t)blockIdx.x * 256; s0 < n; s0 += (int64_t)gridDim.x * 256) {
    const int cnt = (int)min((int64_t)256, n - s0);
    for (int t = threadIdx.x; t < cnt * W4; t += 256) {
      const int j = t / W4, q = t - j * W4;
      const float4 v = *reinterpret_cast<const float4*>(raw + (s0 + j) * C + m.bounce + q * 4);
      float* d = pp_tile + j * LD + q * 4;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < cnt * OC; t += 256) {
      const int j = t / OC, c = t - j * OC;
      out[s0 * OC + t] = pp_llpm_value(pp_tile + j * LD, c, m, m.bounce);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void pp_gradients_kernel(const float* __restrict__ buf, float* __restrict__ out, int h,
                                                           int w, int c) {
  const int64_t total = (int64_t)h * w * c;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(idx % c);
    const int64_t p = idx / c;
    const int x = (int)(p % w), y = (int)(p / w);
    const float v = buf[idx];
    out[p * 2 * c + ch] = x > 0 ? v - buf[idx - c] : 0.f;
    out[p * 2 * c + c + ch] = y > 0 ? v - buf[idx - (int64_t)w * c] : 0.f;
  }
}

// mean and population variance over the s samples of one raw channel group (numpy .mean(2) / .var(2))
template <int NC, class F>
__device__ __forceinline__ void pp_mean_var(const float* __restrict__ px, int s, int C, F f, float* mean, float* var) {
  float sum[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) sum[c] = 0.f;
  for (int k = 0; k < s; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) sum[c] += f(px + (int64_t)k * C, c);
#pragma unroll
  for (int c = 0; c < NC; ++c) { mean[c] = sum[c] / (float)s; sum[c] = 0.f; }
  for (int k = 0; k < s; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) { const float d = f(px + (int64_t)k * C, c) - mean[c]; sum[c] += d * d; }
#pragma unroll
  for (int c = 0; c < NC; ++c) var[c] = sum[c] / (float)s;
}

// pass 1: everything that needs only the pixel's own samples; depth stays raw in the workspace
__global__ __launch_bounds__(256) void pp_kpcn_stats_kernel(const float* __restrict__ raw, float* __restrict__ out,
                                                            float* __restrict__ ws, int* __restrict__ maxslot, int64_t npix,
                                                            int s, int C, PPMap m) {
  // raw / out / ws start at the first of the npix pixels this launch covers (a whole frame or a band of its rows); maxslot is the
  // frame's maximum slot, wherever the band lies
  const float eps = 0.00316f;
  float bmax = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const float* px = raw + p * s * C;
    float* o = out + p * KP_C;
    float mean[3], var[3];
    const float spp = (float)s;
    pp_mean_var<3>(px, s, C, [&](const float* r, int c) { return r[m.normal + c]; }, mean, var);
    o[KP_NORM + 0] = mean[0]; o[KP_NORM + 1] = mean[1]; o[KP_NORM + 2] = mean[2];
    o[KP_NORM + 3] = ((var[0] + var[1] + var[2]) / 3.0f) / spp;
    float dm[1], dv[1];
    pp_mean_var<1>(px, s, C, [&](const float* r, int) { return r[m.depth]; }, dm, dv);
    ws[2 * p] = dm[0]; ws[2 * p + 1] = dv[0];
    bmax = fmaxf(bmax, dm[0]);
    float alb[3];
    pp_mean_var<3>(px, s, C, [&](const float* r, int c) { return r[m.albedo + c]; }, alb, var);
    o[KP_ALB + 0] = alb[0]; o[KP_ALB + 1] = alb[1]; o[KP_ALB + 2] = alb[2];
    o[KP_ALB + 3] = ((var[0] + var[1] + var[2]) / 3.0f) / spp;
    const float a0 = alb[0] + eps, a1 = alb[1] + eps, a2 = alb[2] + eps;
    const float albedo_sqr = (a0 * a0 + a1 * a1 + a2 * a2) / 3.0f;
    pp_mean_var<3>(px, s, C, [&](const float* r, int c) { return fmaxf(r[m.diffuse + c], 0.f); }, mean, var);
    const float diffuse_v = ((var[0] + var[1] + var[2]) / 3.0f) / spp;
    o[KP_DIFF + 0] = mean[0] / a0; o[KP_DIFF + 1] = mean[1] / a1; o[KP_DIFF + 2] = mean[2] / a2;
    o[KP_DIFF + 3] = diffuse_v / albedo_sqr;
    pp_mean_var<3>(px, s, C,
                   [&](const float* r, int c) {
                     return fmaxf(fmaxf(r[m.radiance + c], 0.f) - fmaxf(r[m.diffuse + c], 0.f), 0.f);
                   },
                   mean, var);
    const float specular_v = ((var[0] + var[1] + var[2]) / 3.0f) / spp;
    const float s0 = 1.0f + mean[0], s1 = 1.0f + mean[1], s2 = 1.0f + mean[2];
    const float specular_sqr = (s0 * s0 + s1 * s1 + s2 * s2) / 3.0f;
    o[KP_SPEC + 0] = logf(s0); o[KP_SPEC + 1] = logf(s1); o[KP_SPEC + 2] = logf(s2);
    o[KP_SPEC + 3] = specular_v / specular_sqr;
  }
  // image maximum of the mean depth (only its positive part matters: datasets.py:517-520 scales when max > 0)
  bmax = fmaxf(bmax, __shfl_xor(bmax, 32, 64));
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(maxslot, __float_as_int(bmax));
}

// pass 1, one lane per (pixel, sample) for power-of-two spp <= 64: the s lanes of a pixel sit side by side, so a
// wave reads 64 consecutive raw records (26 KB of contiguous memory) and the statistics are xor-shuffle trees
// (the per-pixel form above walks each pixel's records from a single lane, 3.3 KB apart across the wave).
template <bool VEC>
__global__ __launch_bounds__(256) void pp_kpcn_stats_lanes_kernel(const float* __restrict__ raw, float* __restrict__ out,
                                                                  float* __restrict__ ws, int* __restrict__ maxslot,
                                                                  int64_t npix, int s, int C, PPMap m) {
  const float spp = (float)s;
  const int ppw = 64 / s;                                       // pixels per wave
  const int lane = threadIdx.x & 63, k = lane & (s - 1), pl = lane / s;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  float bmax = 0.f;
  for (int64_t p0 = wave * ppw; p0 < npix; p0 += nwaves * ppw) {
    const int64_t p = p0 + pl;
    const bool ok = p < npix;
    const float* r = raw + ((ok ? p : npix - 1) * s + k) * C;
    float v[13];               // normal(3) depth(1) albedo(3) diffuse+(3) specular+(3)
    pp_kpcn_values<VEC>(r, m, v);
    float mean[13], var[13];
#pragma unroll
    for (int c = 0; c < 13; ++c) {
      float a = v[c];
      for (int o = 1; o < s; o <<= 1) a += __shfl_xor(a, o, 64);
      mean[c] = a / spp;
      const float d = v[c] - mean[c];
      float q = d * d;
      for (int o = 1; o < s; o <<= 1) q += __shfl_xor(q, o, 64);
      var[c] = q / spp;
    }
    if (ok && k == 0) {
      pp_kpcn_write_stats(out + p * KP_C, ws + 2 * p, mean, var, spp);
      bmax = fmaxf(bmax, mean[3]);
    }
  }
  bmax = fmaxf(bmax, __shfl_xor(bmax, 32, 64));
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, off, 64));
  if (lane == 0) atomicMax(maxslot, __float_as_int(bmax));
}

// pass 2 (data_step.h: pp_kpcn_finish)
__global__ __launch_bounds__(256) void pp_kpcn_finish_kernel(float* __restrict__ out, const float* __restrict__ ws, int h,
                                                             int w, int s) {
  pp_kpcn_finish(out, ws, h, w, s);
}

}  // namespace wcmc

using namespace wcmc;

extern "C" int wcmc_preprocess_llpm(const float* raw, int64_t nsamples, int C, int max_depth, float* out, void* stream) {
  WCMC_REQUIRE(raw && out && nsamples > 0 && max_depth >= 0 && C >= 38 + 11 * (max_depth + 1), WCMC_ERR_BAD_ARG,
               "preprocess_llpm: bad argument (raw needs >= 38 + 11*(max_depth+1) channels)");
  const PPMap m = pp_map(max_depth);
  if (C % 4 == 0 && m.bounce % 4 == 0 && aligned16(raw)) {
    const size_t lds = (size_t)256 * (C - m.bounce + 1) * sizeof(float);
    const int64_t blocks = ceil_div64(nsamples, 256);
    hipLaunchKernelGGL(pp_llpm_tiled_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), lds,
                       (hipStream_t)stream, raw, out, nsamples, C, m);
  } else {
    hipLaunchKernelGGL(pp_llpm_kernel, dim3(pp_grid(nsamples * (7 + 5 * m.d))), dim3(256), 0, (hipStream_t)stream, raw,
                       out, nsamples, C, m);
  }
  return check_launch("preprocess_llpm");
}

extern "C" int wcmc_gradients(const float* buf, int h, int w, int c, float* out, void* stream) {
  WCMC_REQUIRE(buf && out && h > 0 && w > 0 && c > 0, WCMC_ERR_BAD_ARG, "gradients: bad argument");
  hipLaunchKernelGGL(pp_gradients_kernel, dim3(pp_grid((int64_t)h * w * c)), dim3(256), 0, (hipStream_t)stream, buf, out, h,
                     w, c);
  return check_launch("gradients");
}

extern "C" size_t wcmc_preprocess_kpcn_workspace_bytes(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return ((size_t)2 * h * w + 4) * sizeof(float);
}

// The frame in row bands (support/staging.py): begin zeroes the maximum slot, rows runs pass 1 on the band's rows -- everything pass 1
// writes is the pixel's own, and the maximum is an atomic on one slot, so any partition of the rows gives the whole frame's bits --
// and end runs pass 2, the only place where pixels meet (the maximum and the backward differences).
static int pp_kpcn_frame_args(const char* who, const void* out, const void* workspace, size_t workspace_bytes, int h, int w) {
  WCMC_REQUIRE(out && workspace, WCMC_ERR_BAD_ARG, "%s: null pointer", who);
  WCMC_REQUIRE(h > 0 && w > 0, WCMC_ERR_BAD_ARG, "%s: the frame (%d x %d) must be positive", who, h, w);
  WCMC_REQUIRE(workspace_bytes >= wcmc_preprocess_kpcn_workspace_bytes(h, w), WCMC_ERR_WORKSPACE,
               "%s: workspace too small (%zu bytes, the %d x %d frame needs %zu)", who, workspace_bytes, h, w,
               wcmc_preprocess_kpcn_workspace_bytes(h, w));
  return WCMC_OK;
}

extern "C" int wcmc_preprocess_kpcn_begin(void* workspace, size_t workspace_bytes, int h, int w, void* stream) {
  int rc = pp_kpcn_frame_args("preprocess_kpcn_begin", workspace, workspace, workspace_bytes, h, w);
  if (rc) return rc;
  if (hipMemsetAsync((float*)workspace + 2 * (int64_t)h * w, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) {
    set_error("preprocess_kpcn_begin: memset failed");
    return WCMC_ERR_LAUNCH;
  }
  return WCMC_OK;
}

extern "C" int wcmc_preprocess_kpcn_rows(const float* raw_band, int h, int w, int row0, int rows, int s, int C, int max_depth,
                                         float* out, void* workspace, size_t workspace_bytes, void* stream) {
  WCMC_REQUIRE(raw_band, WCMC_ERR_BAD_ARG, "preprocess_kpcn_rows: null pointer");
  int rc = pp_kpcn_frame_args("preprocess_kpcn_rows", out, workspace, workspace_bytes, h, w);
  if (rc) return rc;
  WCMC_REQUIRE(s > 0 && max_depth >= 0 && C >= 38 + 11 * (max_depth + 1), WCMC_ERR_BAD_ARG,
               "preprocess_kpcn_rows: bad argument (s = %d, raw needs >= 38 + 11*(max_depth+1) channels, got %d)", s, C);
  WCMC_REQUIRE(row0 >= 0 && rows >= 1 && rows <= h - row0, WCMC_ERR_BAD_ARG,
               "preprocess_kpcn_rows: rows [%d, %d + %d) are not rows of the %d-row frame", row0, row0, rows, h);
  const PPMap m = pp_map(max_depth);
  const int64_t npix = (int64_t)rows * w, p0 = (int64_t)row0 * w;
  float* ws = (float*)workspace;
  int* maxslot = reinterpret_cast<int*>(ws + 2 * (int64_t)h * w);
  float* o = out + p0 * KP_C;
  float* wsb = ws + 2 * p0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = pp_kpcn_vec_ok(raw_band, C, m);
  if (s <= 64 && (s & (s - 1)) == 0 && vec)
    hipLaunchKernelGGL(pp_kpcn_stats_lanes_kernel<true>, dim3(pp_grid(npix * s)), dim3(256), 0, st, raw_band, o, wsb, maxslot, npix, s, C, m);
  else if (s <= 64 && (s & (s - 1)) == 0)
    hipLaunchKernelGGL(pp_kpcn_stats_lanes_kernel<false>, dim3(pp_grid(npix * s)), dim3(256), 0, st, raw_band, o, wsb, maxslot, npix, s, C, m);
  else
    hipLaunchKernelGGL(pp_kpcn_stats_kernel, dim3(pp_grid(npix)), dim3(256), 0, st, raw_band, o, wsb, maxslot, npix, s, C, m);
  return check_launch("preprocess_kpcn_rows(stats)");
}

extern "C" int wcmc_preprocess_kpcn_end(float* out, void* workspace, size_t workspace_bytes, int h, int w, int s, void* stream) {
  int rc = pp_kpcn_frame_args("preprocess_kpcn_end", out, workspace, workspace_bytes, h, w);
  if (rc) return rc;
  WCMC_REQUIRE(s > 0, WCMC_ERR_BAD_ARG, "preprocess_kpcn_end: s = %d must be positive", s);
  hipLaunchKernelGGL(pp_kpcn_finish_kernel, dim3(pp_grid((int64_t)h * w * KP_C)), dim3(256), 0, (hipStream_t)stream, out,
                     (const float*)workspace, h, w, s);
  return check_launch("preprocess_kpcn_end(finish)");
}

extern "C" int wcmc_preprocess_kpcn(const float* raw, int h, int w, int s, int C, int max_depth, float* out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  WCMC_REQUIRE(raw && out && workspace && h > 0 && w > 0 && s > 0 && max_depth >= 0 && C >= 38 + 11 * (max_depth + 1),
               WCMC_ERR_BAD_ARG, "preprocess_kpcn: bad argument");
  WCMC_REQUIRE(workspace_bytes >= wcmc_preprocess_kpcn_workspace_bytes(h, w), WCMC_ERR_WORKSPACE,
               "preprocess_kpcn: workspace too small");
  // the whole frame as one band: the same memset, the same two launches with the same grids as before the band entry points
  int rc = wcmc_preprocess_kpcn_begin(workspace, workspace_bytes, h, w, stream);
  if (rc) return rc;
  rc = wcmc_preprocess_kpcn_rows(raw, h, w, 0, h, s, C, max_depth, out, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return wcmc_preprocess_kpcn_end(out, workspace, workspace_bytes, h, w, s, stream);
}

// ------------------------------------------------------------------ patch batch assembly (datasets.py:1026-1146)
// What DenoiseDataset.__getitem__ + _sample_patches + _transpose do per patch on the loader's CPU worker, for the
// KPCN base model: crop a P x P window out of the preprocessed per-image buffers and lay the batch dictionary's
// tensors out channel-first --
//   kpcn_diffuse_in  = [kpcn 0:10, kpcn 20:44 (, mean_s llpm[..., 0])]       34 (+1) channels      :1080,1099-1103
//   kpcn_specular_in = [kpcn 10:44 (, mean_s llpm[..., 0])]                  34 (+1)               :1081,1104-1107
//   kpcn_diffuse_buffer = kpcn 0:3, kpcn_specular_buffer = kpcn 10:13, kpcn_albedo = kpcn 34:37 + 0.00316  :1082-1084
//   paths = llpm[..., 1:37] as (S, 36, P, P)                                                       :1110
//   target_total = gt 0:3, target_diffuse = gt 3:6 / (gt 6:9 + 0.00316), target_specular = log(1 + total - diffuse)  :1117-1126
// One thread per (patch, y, x): every output plane is written as coalesced rows, the inputs are read once.
namespace wcmc {
struct PatchOut {
  float *din, *sin, *dbuf, *sbuf, *alb, *paths, *tdif, *tspec, *ttot;
};
// AUG (a transforms table is given): output pixel (y, x) of patch b takes the window position patch_map gives for
// the code transforms[b] -- the destination is untouched, only the source index is permuted, and a source is still one whole
// 176-byte record plus its S * 148 bytes of llpm.  The backward differences are those of the transformed frame: taken again
// from the stored value channels against the source of output (y, x - 1) / (y - 1, x) -- thirteen floats of one more record each,
// one step outside the window at x = 0 / y = 0 -- and 0.f where that source lies outside the frame.  Where the source steps as
// the stored difference did (+1 column for dx, +1 row for dy) the stored one is that very subtraction and is kept.
template <bool AUG>
__global__ __launch_bounds__(256) void pp_assemble_kpcn_kernel(const float* __restrict__ kpcn, const float* __restrict__ llpm,
                                                               const float* __restrict__ gt, const int* __restrict__ origins,
                                                               const int* __restrict__ transforms, PatchOut o, int B, int H, int W,
                                                               int S, int Sn, int P) {
  // S: samples per pixel of llpm; Sn <= S: the first Sn of them go to the batch
  const int64_t total = (int64_t)B * P * P;
  const int cin = llpm ? 35 : 34;
  const int64_t plane = (int64_t)P * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % P), y = (int)((i / P) % P), b = (int)(i / plane);
    PatchMap pm{y, x, 0, 1, 1, 0};
    if (AUG) pm = patch_map(transforms[b], y, x, P);
    const int r = origins[2 * b] + pm.sy, c = origins[2 * b + 1] + pm.sx;     // (row, column) of the image
    const int64_t pix = (int64_t)r * W + c;
    const float* k = kpcn + pix * 44;
    float v[KP_C];                                                            // AUG: the record, its differences retaken
    if (AUG) {
#pragma unroll
      for (int ch = 0; ch < KP_C; ++ch) v[ch] = k[ch];
      if (pm.xc != 1) {
        const int nr = r - pm.xr, nc = c - pm.xc;
        const bool in = nr >= 0 && nr < H && nc >= 0 && nc < W;               // (clamped before use, 0 selected afterwards)
        const float* kn = kpcn + ((int64_t)min(max(nr, 0), H - 1) * W + min(max(nc, 0), W - 1)) * KP_C;
#pragma unroll
        for (int g = 0; g < KP_NV; ++g) {
          const float d = v[ft_grad_src(g)] - kn[ft_grad_src(g)];
          v[ft_grad_dst(g, false)] = in ? d : 0.f;
        }
      }
      if (pm.yr != 1) {
        const int nr = r - pm.yr, nc = c - pm.yc;
        const bool in = nr >= 0 && nr < H && nc >= 0 && nc < W;
        const float* kn = kpcn + ((int64_t)min(max(nr, 0), H - 1) * W + min(max(nc, 0), W - 1)) * KP_C;
#pragma unroll
        for (int g = 0; g < KP_NV; ++g) {
          const float d = v[ft_grad_src(g)] - kn[ft_grad_src(g)];
          v[ft_grad_dst(g, true)] = in ? d : 0.f;
        }
      }
    }
    auto kv = [&](int ch) { return AUG ? v[ch] : k[ch]; };
    const int64_t po = (int64_t)y * P + x;
    float* din = o.din + (int64_t)b * cin * plane + po;
    float* sin = o.sin + (int64_t)b * cin * plane + po;
    for (int ch = 0; ch < 10; ++ch) din[ch * plane] = kv(ch);
    for (int ch = 20; ch < 44; ++ch) din[(ch - 10) * plane] = kv(ch);
    for (int ch = 10; ch < 44; ++ch) sin[(ch - 10) * plane] = kv(ch);
    for (int ch = 0; ch < 3; ++ch) {
      o.dbuf[((int64_t)b * 3 + ch) * plane + po] = kv(ch);
      o.sbuf[((int64_t)b * 3 + ch) * plane + po] = kv(10 + ch);
      o.alb[((int64_t)b * 3 + ch) * plane + po] = kv(34 + ch) + 0.00316f;
    }
    if (llpm) {
      const float* l = llpm + pix * S * 37;
      float pw = 0.f;
      for (int s = 0; s < Sn; ++s) {
        pw += l[s * 37];
        float* pp = o.paths + (((int64_t)b * Sn + s) * 36) * plane + po;
        for (int ch = 0; ch < 36; ++ch) pp[ch * plane] = l[s * 37 + 1 + ch];
      }
      pw /= (float)Sn;
      din[34 * plane] = pw;
      sin[34 * plane] = pw;
    }
    const float* g = gt + pix * 9;
    for (int ch = 0; ch < 3; ++ch) {
      const float tot = g[ch], dif = g[3 + ch], alb = g[6 + ch];
      o.ttot[((int64_t)b * 3 + ch) * plane + po] = tot;
      o.tdif[((int64_t)b * 3 + ch) * plane + po] = dif / (alb + 0.00316f);
      o.tspec[((int64_t)b * 3 + ch) * plane + po] = logf(1.f + tot - dif);
    }
  }
}

}  // namespace wcmc

extern "C" int wcmc_assemble_kpcn_patches(const float* kpcn, const float* llpm, const float* gt, const int* origins,
                                          const int* transforms, int B, int H, int W, int S_total, int s, int P, float* diffuse_in,
                                          float* specular_in, float* diffuse_buffer, float* specular_buffer, float* albedo,
                                          float* paths, float* target_diffuse, float* target_specular, float* target_total,
                                          void* stream) {
  WCMC_REQUIRE(kpcn && gt && origins && diffuse_in && specular_in && diffuse_buffer && specular_buffer && albedo && target_diffuse &&
                   target_specular && target_total,
               WCMC_ERR_BAD_ARG, "assemble_kpcn_patches: null pointer");
  WCMC_REQUIRE(B > 0 && H > 0 && W > 0 && P > 0, WCMC_ERR_BAD_ARG, "assemble_kpcn_patches: B, H, W, P must be positive");
  WCMC_REQUIRE(P <= H && P <= W, WCMC_ERR_BAD_ARG, "assemble_kpcn_patches: a %d-pixel patch does not fit the %d x %d frame", P, H, W);
  // (the sample counts are read with llpm alone: without it S_total = s = 0 is a plain batch)
  WCMC_REQUIRE(!llpm || (1 <= s && s <= S_total), WCMC_ERR_BAD_ARG,
               "assemble_kpcn_patches: the prefix must satisfy 1 <= s <= S_total (got %d of %d)", s, S_total);
  WCMC_REQUIRE(!llpm || paths, WCMC_ERR_BAD_ARG, "assemble_kpcn_patches: llpm given without a paths output");
  PatchOut o{diffuse_in, specular_in, diffuse_buffer, specular_buffer, albedo, paths, target_diffuse, target_specular,
             target_total};
  const int64_t total = (int64_t)B * P * P;
  const unsigned grid = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
  if (transforms)
    hipLaunchKernelGGL(pp_assemble_kpcn_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, kpcn, llpm, gt, origins,
                       transforms, o, B, H, W, S_total, s, P);
  else
    hipLaunchKernelGGL(pp_assemble_kpcn_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, kpcn, llpm, gt, origins,
                       transforms, o, B, H, W, S_total, s, P);
  return check_launch("assemble_kpcn_patches");
}
