// What the data-step translation units share (preprocess.hip, multi_spp.hip, sbmc_data.hip, frame_tiles.hip): the raw channel map, the layout of
// the 44-channel KPCN buffer, the per-sample values and per-pixel closing arithmetic of _preprocess_kpcn, the finish pass, the
// mirror map and the dihedral maps of the assembly kernels.
#pragma once
#include "common.h"

namespace wcmc {

struct PPMap { int radiance, diffuse, bounce, albedo, normal, depth, pweight, rwow, light, thr, rough, d; };

static PPMap pp_map(int max_depth) {
  const int d = max_depth + 1;
  PPMap m;
  m.radiance = 2; m.diffuse = 5; m.bounce = 24 + d * 6; m.albedo = 24 + d * 7; m.normal = 27 + d * 7;
  m.depth = 30 + d * 7; m.pweight = 31 + d * 7; m.rwow = 32 + d * 7; m.light = 35 + d * 7;
  m.thr = 38 + d * 7; m.rough = 38 + d * 10; m.d = d;
  return m;
}

// 16-byte aligned records with radiance / diffuse at 2 / 5 and albedo, normal, depth side by side from a channel a with a even and
// a + 2 a multiple of 4: what the float2 / float4 loads of pp_kpcn_values<true> need
static bool pp_kpcn_vec_ok(const float* raw, int C, const PPMap& m) {
  return C % 4 == 0 && aligned16(raw) && m.radiance == 2 && m.diffuse == 5 && m.albedo % 2 == 0 && (m.albedo + 2) % 4 == 0 &&
         m.normal == m.albedo + 3 && m.depth == m.albedo + 6;
}

// output channel offsets of the 44-channel KPCN buffer
constexpr int KP_DIFF = 0, KP_SPEC = 10, KP_NORM = 20, KP_DEPTH = 30, KP_ALB = 34, KP_C = 44;
constexpr int KP_NV = 13;                           // per-sample values behind the statistics

// The thirteen values of one raw record whose mean and variance over the samples _preprocess_kpcn takes (datasets.py:505-543):
// v = normal(3) depth(1) albedo(3) max(diffuse, 0)(3) max(max(radiance, 0) - max(diffuse, 0), 0)(3)
template <bool VEC>
__device__ __forceinline__ void pp_kpcn_values(const float* __restrict__ r, const PPMap& m, float* v) {
  float in[13];                // radiance(3) diffuse(3) albedo(3) normal(3) depth(1)
  if (VEC) {
    const float2 a = *reinterpret_cast<const float2*>(r + 2), b = *reinterpret_cast<const float2*>(r + 4),
                 c2 = *reinterpret_cast<const float2*>(r + 6), d2 = *reinterpret_cast<const float2*>(r + m.albedo);
    const float4 e = *reinterpret_cast<const float4*>(r + m.albedo + 2);
    in[0] = a.x; in[1] = a.y; in[2] = b.x; in[3] = b.y; in[4] = c2.x; in[5] = c2.y;
    in[6] = d2.x; in[7] = d2.y; in[8] = e.x; in[9] = e.y; in[10] = e.z; in[11] = e.w; in[12] = r[m.depth];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      in[c] = r[m.radiance + c]; in[3 + c] = r[m.diffuse + c]; in[6 + c] = r[m.albedo + c]; in[9 + c] = r[m.normal + c];
    }
    in[12] = r[m.depth];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c] = in[9 + c];
    v[4 + c] = in[6 + c];
    const float df = fmaxf(in[3 + c], 0.f);
    v[7 + c] = df;
    v[10 + c] = fmaxf(fmaxf(in[c], 0.f) - df, 0.f);
  }
  v[3] = in[12];
}

// One pixel's sixteen value / variance channels from the means and population variances of its thirteen values over spp samples
// (datasets.py:545-582 up to the depth normalisation); the raw mean depth and its variance go to the workspace pair wsp.
__device__ __forceinline__ void pp_kpcn_write_stats(float* __restrict__ o, float* __restrict__ wsp, const float* mean,
                                                    const float* var, float spp) {
  const float eps = 0.00316f;
  o[KP_NORM + 0] = mean[0]; o[KP_NORM + 1] = mean[1]; o[KP_NORM + 2] = mean[2];
  o[KP_NORM + 3] = ((var[0] + var[1] + var[2]) / 3.0f) / spp;
  wsp[0] = mean[3]; wsp[1] = var[3];
  o[KP_ALB + 0] = mean[4]; o[KP_ALB + 1] = mean[5]; o[KP_ALB + 2] = mean[6];
  o[KP_ALB + 3] = ((var[4] + var[5] + var[6]) / 3.0f) / spp;
  const float a0 = mean[4] + eps, a1 = mean[5] + eps, a2 = mean[6] + eps;
  const float albedo_sqr = (a0 * a0 + a1 * a1 + a2 * a2) / 3.0f;
  o[KP_DIFF + 0] = mean[7] / a0; o[KP_DIFF + 1] = mean[8] / a1; o[KP_DIFF + 2] = mean[9] / a2;
  o[KP_DIFF + 3] = (((var[7] + var[8] + var[9]) / 3.0f) / spp) / albedo_sqr;
  const float s0 = 1.0f + mean[10], s1 = 1.0f + mean[11], s2 = 1.0f + mean[12];
  const float specular_sqr = (s0 * s0 + s1 * s1 + s2 * s2) / 3.0f;
  o[KP_SPEC + 0] = logf(s0); o[KP_SPEC + 1] = logf(s1); o[KP_SPEC + 2] = logf(s2);
  o[KP_SPEC + 3] = (((var[10] + var[11] + var[12]) / 3.0f) / spp) / specular_sqr;
}

// pass 2 of _preprocess_kpcn on one (h, w, 44) buffer: depth normalisation by the image maximum ws[2 * npix] (when it is positive)
// + clip, and the backward differences of the five feature groups.  One thread per (pixel, output channel): a wave touches
// consecutive floats of the 176-byte pixel records.  ws: [mean depth, depth variance] per pixel, then the maximum.
__device__ __forceinline__ void pp_kpcn_finish(float* __restrict__ out, const float* __restrict__ ws, int h, int w, int s) {
  const int64_t npix = (int64_t)h * w;
  const float maxd = ws[2 * npix];
  auto depth_of = [&](int64_t p) {
    float d = ws[2 * p];
    if (maxd > 0.f) d = d / maxd;
    // np.clip keeps a NaN (an overflowed mean over an overflowed maximum is Inf / Inf); fminf(fmaxf()) would turn it into 0
    return d < 0.f ? 0.f : (d > 1.f ? 1.f : d);
  };
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < npix * KP_C;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = idx / KP_C;
    const int c = (int)(idx - p * KP_C);
    const int x = (int)(p % w), y = (int)(p / w);
    if (c >= KP_DEPTH && c < KP_ALB) {
      float v;
      if (c == KP_DEPTH) v = depth_of(p);
      else if (c == KP_DEPTH + 1) { v = ws[2 * p + 1]; if (maxd > 0.f) v = v / (maxd * maxd * (float)s); }
      else if (c == KP_DEPTH + 2) v = x > 0 ? depth_of(p) - depth_of(p - 1) : 0.f;
      else v = y > 0 ? depth_of(p) - depth_of(p - w) : 0.f;
      out[idx] = v;
      continue;
    }
    const int g0 = c < KP_SPEC ? KP_DIFF : c < KP_NORM ? KP_SPEC : c < KP_DEPTH ? KP_NORM : KP_ALB;
    const int j = c - g0;
    if (j < 4) continue;                                  // values and variance: final since pass 1
    const int src = g0 + (j < 7 ? j - 4 : j - 7);
    const float v = out[p * KP_C + src];
    if (j < 7) out[idx] = x > 0 ? v - out[(p - 1) * KP_C + src] : 0.f;
    else out[idx] = y > 0 ? v - out[(p - w) * KP_C + src] : 0.f;
  }
}

static unsigned pp_grid(int64_t work) {
  const int64_t b = ceil_div64(work, 256);
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// The mirror map of the tiles of a frame of any size (frame_tiles.hip, sbmc_data.hip): source index of position i in [-n, 2n) of a
// line of n entries: d c b a | a b c d | d c b a (one reflection; pad < n).  The clamp costs two instructions and keeps a table the
// host check let through from reading outside the buffers.
__device__ __forceinline__ int ft_mirror(int i, int n) {
  const int m = i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i);
  return min(max(m, 0), n - 1);
}

// value channel behind the g-th backward difference of a direction: diffuse, specular, normal (3 each), depth (1), albedo (3)
__device__ __forceinline__ int ft_grad_src(int g) { return g < 3 ? KP_DIFF + g : g < 6 ? KP_SPEC + g - 3 : g < 9 ? KP_NORM + g - 6 :
                                                           g < 10 ? KP_DEPTH : KP_ALB + g - 10; }
// where that difference is stored: dx at value + 4 (depth: + 2), dy at value + 7 (depth: + 3)
__device__ __forceinline__ int ft_grad_dst(int g, bool dy) {
  const int src = ft_grad_src(g);
  return src == KP_DEPTH ? src + (dy ? 3 : 2) : src + (dy ? 7 : 4);
}

// Dihedral patch transforms: code t in 0..7 is T_t(a) = rot90(fliplr(a) if t & 4 else a, k = t & 3) on a
// P x P window.  The map output (y, x) -> window position (sy, sx) is affine: (sy, sx) at this output pixel, and the steps
// (xr, xc) / (yr, yc) the source takes when the output moves one pixel along x / along y.  The code is masked to 0..7 (the host
// checks the table; the mask keeps a bad one inside the window).
struct PatchMap { int sy, sx, xr, xc, yr, yc; };
__device__ __forceinline__ PatchMap patch_map(int t, int y, int x, int P) {
  const int k = t & 3, q = P - 1;
  PatchMap m;
  m.sy = k == 0 ? y : k == 1 ? x : k == 2 ? q - y : q - x;
  m.sx = k == 0 ? x : k == 1 ? q - y : k == 2 ? q - x : y;
  m.xr = k == 1 ? 1 : k == 3 ? -1 : 0;  m.xc = k == 0 ? 1 : k == 2 ? -1 : 0;
  m.yr = k == 0 ? 1 : k == 2 ? -1 : 0;  m.yc = k == 1 ? -1 : k == 3 ? 1 : 0;
  if (t & 4) { m.sx = q - m.sx; m.xc = -m.xc; m.yc = -m.yc; }
  return m;
}

// Whole-frame dihedral transforms (the self-ensemble of wcmc_amd.denoise): patch_map with the H x W frame's
// own two sizes in place of P.  T_t of the frame is H x W for even t and W x H for odd t; (y, x) is a position INSIDE the transformed
// frame (mirrored already), and the result the source pixel of the stored H x W buffers.  The code is masked to 0..7; the result is
// clamped, so a position the host check let through cannot lead outside the buffers.
struct FramePos { int sy, sx; };
__device__ __forceinline__ FramePos frame_map(int t, int y, int x, int H, int W) {
  const int k = t & 3;
  FramePos m;
  m.sy = k == 0 ? y : k == 1 ? x : k == 2 ? H - 1 - y : H - 1 - x;
  m.sx = k == 0 ? x : k == 1 ? W - 1 - y : k == 2 ? W - 1 - x : y;
  if (t & 4) m.sx = W - 1 - m.sx;
  m.sy = min(max(m.sy, 0), H - 1);
  m.sx = min(max(m.sx, 0), W - 1);
  return m;
}

}  // namespace wcmc
