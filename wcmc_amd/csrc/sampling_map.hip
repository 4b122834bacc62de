// Patch-sampling probability maps of the training data step: the reference's gradient_importance_map
// (support/datasets.py:17-36) and the `_prob_imp` block of DenoiseDataset._offline_preprocess (:697-715), plus the
// NaN / Inf rule of :623-624 in place.
//
// importance map of C (1 or 3) planes of an H x W image:
//   1. scipy.ndimage.gaussian_filter(x, 31): a separable 249-tap Gaussian (radius int(4 * 31 + 0.5) = 124), axis 0 first,
//      boundary mode 'reflect' (d c b a | a b c d | d c b a, period 2n: correct for images smaller than the radius), the
//      result rounded to fp32 between the passes.  One kernel per pass (sm_gauss_kernel<ALONG_X>): a block stages
//      SM_TA + 2 * 124 positions along the filtered axis x SM_TB lines in LDS and every thread accumulates 16 outputs in
//      fp64 in scipy's order (ni_filters.c, symmetric branch: centre tap, then the pairs from the outermost inwards), so
//      the blurred planes carry the rounding of scipy's own and the Sobel differences of near-equal neighbours do not
//      amplify a different summation error;
//   2. sobel(axis 0) and sobel(axis 1) with mode 'nearest' ([-1 0 1] along the axis, [1 2 1] across, each stage rounded
//      to fp32 as scipy does for fp32 input), the root of the sum of squares over the planes in fp32, and the block's
//      min / max (sm_sobel_kernel);
//   3. a one-block finish over the blocks' min / max (sm_minmax_finish_kernel), then (v - min) / (max - min + 1e-5).
// sampling_prob adds the per-pixel planes in front (sm_planes_kernel: tone-mapped sRGB luminance of the target, the
// sample mean of the normal, the material term of the bounce-0 type bits) and the combination behind (crop, block sums
// in fp64, a one-block finish in a fixed order, the division).  No atomics anywhere: every result is bitwise reproducible.
#include "common.h"

#include <math.h>
#include <mutex>

namespace wcmc {

constexpr int SM_SIGMA = 31;
constexpr int SM_R = 124;                            // int(4.0 * 31 + 0.5)
constexpr int SM_TA = 128;                           // outputs along the filtered axis per block
constexpr int SM_TB = 32;                            // lines across it per block
constexpr int SM_EXT = SM_TA + 2 * SM_R;             // staged positions along the axis
constexpr int SM_PITCH = SM_TB + 1;                  // odd pitch: lanes over either coordinate hit distinct banks
constexpr int SM_THREADS = 256;
constexpr int SM_PER_THREAD = SM_TA * SM_TB / SM_THREADS;      // 16
constexpr int SM_SW = 32, SM_SH = 8;                 // sobel / pointwise tile (SM_SW * SM_SH == SM_THREADS)

struct SmWeights { double w[SM_R + 1]; };            // w[d]: the normalised tap at distance d (symmetric)

// scipy's 'reflect' (numpy.pad's 'symmetric') source index of position i of a line of n entries, any i
__host__ __device__ __forceinline__ int sm_reflect(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// One pass of the Gaussian over C planes.  src: element (y, x, c) at src[y * sy + x * sx + c * sc]; dst: planar [C][H][W].
template <bool ALONG_X>
__global__ __launch_bounds__(SM_THREADS) void sm_gauss_kernel(const float* __restrict__ src, int64_t sy, int64_t sx, int64_t sc,
                                                              float* __restrict__ dst, int H, int W, SmWeights wt) {
  __shared__ float tile[SM_EXT * SM_PITCH];
  const int tid = threadIdx.x;
  const int na = ALONG_X ? W : H, nb = ALONG_X ? H : W;
  const int a0 = blockIdx.x * SM_TA, b0 = blockIdx.y * SM_TB;
  const float* plane = src + (int64_t)blockIdx.z * sc;
  for (int e = tid; e < SM_EXT * SM_TB; e += SM_THREADS) {
    // consecutive threads walk x: the filtered axis in the row pass, the lines in the column pass
    const int ae = ALONG_X ? e % SM_EXT : e / SM_TB;
    const int b = ALONG_X ? e / SM_EXT : e % SM_TB;
    const int ai = sm_reflect(a0 - SM_R + ae, na), bi = b0 + b;
    float v = 0.f;
    if (bi < nb) v = ALONG_X ? plane[(int64_t)bi * sy + (int64_t)ai * sx] : plane[(int64_t)ai * sy + (int64_t)bi * sx];
    tile[ae * SM_PITCH + b] = v;
  }
  __syncthreads();
  // output k of this thread: lanes walk x again
  const int ar = ALONG_X ? tid % SM_TA : tid / SM_TB;
  const int br = ALONG_X ? tid / SM_TA : tid % SM_TB;
  constexpr int AS = ALONG_X ? 0 : SM_THREADS / SM_TB;          // step of a between a thread's outputs
  constexpr int BS = ALONG_X ? SM_THREADS / SM_TA : 0;          // step of b
  double acc[SM_PER_THREAD];
  const float* ctr[SM_PER_THREAD];
#pragma unroll
  for (int k = 0; k < SM_PER_THREAD; ++k) {
    ctr[k] = tile + (ar + k * AS + SM_R) * SM_PITCH + (br + k * BS);
    acc[k] = (double)ctr[k][0] * wt.w[0];
  }
  for (int d = SM_R; d >= 1; --d) {
    const double w = wt.w[d];
#pragma unroll
    for (int k = 0; k < SM_PER_THREAD; ++k)
      acc[k] += ((double)ctr[k][-d * SM_PITCH] + (double)ctr[k][d * SM_PITCH]) * w;
  }
  float* out = dst + (int64_t)blockIdx.z * H * W;
#pragma unroll
  for (int k = 0; k < SM_PER_THREAD; ++k) {
    const int a = a0 + ar + k * AS, b = b0 + br + k * BS;
    if (a < na && b < nb) out[ALONG_X ? (int64_t)b * W + a : (int64_t)a * W + b] = (float)acc[k];
  }
}

// NaN-propagating min / max (numpy.min / numpy.max)
__device__ __forceinline__ float sm_min(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ float sm_max(float m, float v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ void sm_block_minmax(float mn, float mx, float* red, float* out_mn, float* out_mx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = sm_min(mn, __shfl_xor(mn, o, 64));
    mx = sm_max(mx, __shfl_xor(mx, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave] = mn; red[4 + wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = red[0], b = red[4];
#pragma unroll
    for (int w = 1; w < SM_THREADS / 64; ++w) { a = sm_min(a, red[w]); b = sm_max(b, red[4 + w]); }
    *out_mn = a;
    *out_mx = b;
  }
}

// blur: planar [C][H][W].  mag (H, W) and the block's min / max -> mm[blk], mm[nblk + blk].
__global__ __launch_bounds__(SM_THREADS) void sm_sobel_kernel(const float* __restrict__ blur, int C, int H, int W,
                                                              float* __restrict__ mag, float* __restrict__ mm) {
  __shared__ float red[8];
  const int x = blockIdx.x * SM_SW + threadIdx.x % SM_SW, y = blockIdx.y * SM_SH + threadIdx.x / SM_SW;
  const int nblk = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  if (x < W && y < H) {
    const int ys[3] = {max(y - 1, 0), y, min(y + 1, H - 1)}, xs[3] = {max(x - 1, 0), x, min(x + 1, W - 1)};
    float sum = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* p = blur + (int64_t)c * H * W;
      // d0[i]: the axis-0 difference at (y, xs[i]); d1[i]: the axis-1 difference at (ys[i], x); both rounded to fp32
      float d0[3], d1[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int xx = xs[i], yy = ys[i];
        d0[i] = (float)((double)p[(int64_t)min(y + 1, H - 1) * W + xx] - (double)p[(int64_t)max(y - 1, 0) * W + xx]);
        d1[i] = (float)((double)p[(int64_t)yy * W + min(x + 1, W - 1)] - (double)p[(int64_t)yy * W + max(x - 1, 0)]);
      }
      const float gx = (float)((double)d0[1] * 2.0 + ((double)d0[0] + (double)d0[2]));
      const float gy = (float)((double)d1[1] * 2.0 + ((double)d1[0] + (double)d1[2]));
      sum = c == 0 ? gx * gx + gy * gy : (sum + gx * gx) + gy * gy;
    }
    const float v = sqrtf(sum);
    mag[(int64_t)y * W + x] = v;
    mn = mx = v;
  }
  sm_block_minmax(mn, mx, red, mm + blk, mm + nblk + blk);
}

__global__ __launch_bounds__(SM_THREADS) void sm_minmax_finish_kernel(const float* __restrict__ mm, int nblk,
                                                                      float* __restrict__ result) {
  __shared__ float red[8];
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < nblk; i += SM_THREADS) { mn = sm_min(mn, mm[i]); mx = sm_max(mx, mm[nblk + i]); }
  sm_block_minmax(mn, mx, red, result, result + 1);
}

__device__ __forceinline__ float sm_normalised(float v, const float* mm) {
  return (v - mm[0]) / ((mm[1] - mm[0]) + 1e-5f);
}

__global__ __launch_bounds__(SM_THREADS) void sm_normalise_kernel(const float* __restrict__ mag, const float* __restrict__ mm,
                                                                  int64_t n, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SM_THREADS)
    out[i] = sm_normalised(mag[i], mm);
}

// ---------------------------------------------------------------------------------------------- sampling_prob
// Per pixel: lum (H, W), normal planar [3][H][W], mat (H, W).
__global__ __launch_bounds__(SM_THREADS) void sm_planes_kernel(const float* __restrict__ raw, const float* __restrict__ gt, int64_t npix,
                                                               int S, int C, int ch_normal, int ch_bounce, float* __restrict__ lum,
                                                               float* __restrict__ normal, float* __restrict__ mat) {
  const int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= npix) return;
  // LinearToSrgb(ToneMap(gt[..., :3], 1.5)) (support/utils.py:44-57), then the luminance of the result
  const float* g = gt + i * 9;
  const float l = (0.2126f * g[0] + 0.7152f * g[1]) + 0.0722f * g[2];
  const float den = 1.0f + l / 1.5f;
  float t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = powf(g[c] / den, (float)(1.0 / 2.2));
    t[c] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);            // numpy's clip: NaN passes through
  }
  lum[i] = (0.2126f * t[0] + 0.7152f * t[1]) + 0.0722f * t[2];
  float n[3] = {0.f, 0.f, 0.f}, dif = 0.f, glo = 0.f, spe = 0.f;
  const float* r = raw + i * (int64_t)S * C;
  for (int s = 0; s < S; ++s, r += C) {
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] += r[ch_normal + c];
    const float b = r[ch_bounce];
    const int bits = (b > -32768.f && b < 32768.f) ? (int)b : 0;      // astype(int16); a sanitised 1e38 carries no bits
    dif += (bits & 4) ? 1.f : 0.f;
    glo += (bits & 8) ? 1.f : 0.f;
    spe += (bits & 16) ? 1.f : 0.f;
  }
  const float fs = (float)S;
#pragma unroll
  for (int c = 0; c < 3; ++c) normal[(int64_t)c * npix + i] = (n[c] / fs) * 0.5f + 0.5f;
  mat[i] = ((dif / fs + (glo / fs) * 4.f) + (spe / fs) * 2.f) / 7.f;
}

// prob = 0.3 d_lum + 0.2 d_norm + 0.5 mat on the crop [top, top + ho) x [top, top + wo); the block's sum in fp64 -> part[blk]
__global__ __launch_bounds__(SM_THREADS) void sm_combine_kernel(const float* __restrict__ mag_l, const float* __restrict__ mm_l,
                                                                const float* __restrict__ mag_n, const float* __restrict__ mm_n,
                                                                const float* __restrict__ mat, int W, int top, int ho, int wo,
                                                                float* __restrict__ out, double* __restrict__ part) {
  __shared__ double red[SM_THREADS / 64];
  const int x = blockIdx.x * SM_SW + threadIdx.x % SM_SW, y = blockIdx.y * SM_SH + threadIdx.x / SM_SW;
  double v = 0.0;
  if (x < wo && y < ho) {
    const int64_t i = (int64_t)(y + top) * W + (x + top);
    const float p = (0.3f * sm_normalised(mag_l[i], mm_l) + 0.2f * sm_normalised(mag_n[i], mm_n)) + 0.5f * mat[i];
    out[(int64_t)y * wo + x] = p;
    v = (double)p;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one block: the blocks' sums in a fixed order (thread-strided, a fixed xor tree, the waves in order) -> *total
__global__ __launch_bounds__(SM_THREADS) void sm_sum_finish_kernel(const double* __restrict__ part, int nblk, float* __restrict__ total) {
  __shared__ double red[SM_THREADS / 64];
  double v = 0.0;
  for (int i = threadIdx.x; i < nblk; i += SM_THREADS) v += part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *total = (float)(((red[0] + red[1]) + red[2]) + red[3]);        // numpy.sum of fp32 returns fp32
}

__global__ __launch_bounds__(SM_THREADS) void sm_divide_kernel(float* __restrict__ out, int64_t n, const float* __restrict__ total) {
  const float den = *total + 1e-5f;
  for (int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SM_THREADS) out[i] = out[i] / den;
}

__global__ __launch_bounds__(SM_THREADS) void sm_sanitize_kernel(float* __restrict__ x, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SM_THREADS) {
    const float v = x[i];
    if (!(v < 1.0e38f)) x[i] = 1.0e38f;              // NaN, +Inf and >= 1e38 fail the comparison ...
    else if (v == -INFINITY) x[i] = 1.0e38f;         // ... and -Inf is not finite either (datasets.py:623)
  }
}

}  // namespace wcmc

using namespace wcmc;

// scipy.ndimage._filters._gaussian_kernel1d(31, 0, 124) in fp64, once per process
static const SmWeights& sm_weights() {
  static SmWeights wt;
  static std::once_flag once;
  std::call_once(once, [] {
    const double sigma2 = (double)SM_SIGMA * SM_SIGMA;
    double phi[2 * SM_R + 1], sum = 0.0;
    for (int i = -SM_R; i <= SM_R; ++i) phi[i + SM_R] = exp(-0.5 / sigma2 * ((double)i * i));
    for (int i = 0; i < 2 * SM_R + 1; ++i) sum += phi[i];
    for (int d = 0; d <= SM_R; ++d) wt.w[d] = phi[SM_R + d] / sum;
  });
  return wt;
}

static inline size_t sm_align(size_t n) { return (n + 255) / 256 * 256; }
static inline int sm_tiles(int H, int W) { return ((W + SM_SW - 1) / SM_SW) * ((H + SM_SH - 1) / SM_SH); }
static inline bool sm_size_ok(int H, int W) { return H >= 1 && W >= 1 && H <= 32768 && W <= 32768; }

// workspace of one importance map: two sets of C blurred planes, the magnitude, the blocks' min / max, the result pair
struct SmLayout { size_t blur_a, blur_b, mag, mm, res, end; };
static SmLayout sm_layout(size_t base, int H, int W, int C) {
  SmLayout l;
  const size_t plane = sm_align((size_t)H * W * sizeof(float));
  l.blur_a = base;
  l.blur_b = l.blur_a + plane * C;
  l.mag = l.blur_b + plane * C;
  l.mm = l.mag + plane;
  l.res = l.mm + sm_align((size_t)2 * sm_tiles(H, W) * sizeof(float));
  l.end = l.res + 256;
  return l;
}

// src (y, x, c) at src[y * sy + x * sx + c * sc] -> magnitude at ws + l.mag, min / max at ws + l.res
static int sm_run_map(const float* src, int64_t sy, int64_t sx, int64_t sc, int C, int H, int W, char* ws, const SmLayout& l,
                      hipStream_t st) {
  const SmWeights& wt = sm_weights();
  float* a = (float*)(ws + l.blur_a);
  float* b = (float*)(ws + l.blur_b);
  // (the C planes of a / b lie densely at stride H * W inside their padded regions)
  hipLaunchKernelGGL(sm_gauss_kernel<false>, dim3((H + SM_TA - 1) / SM_TA, (W + SM_TB - 1) / SM_TB, C), dim3(SM_THREADS), 0, st, src,
                     sy, sx, sc, a, H, W, wt);
  int rc = check_launch("importance_map(gauss axis 0)");
  if (rc) return rc;
  hipLaunchKernelGGL(sm_gauss_kernel<true>, dim3((W + SM_TA - 1) / SM_TA, (H + SM_TB - 1) / SM_TB, C), dim3(SM_THREADS), 0, st,
                     (const float*)a, (int64_t)W, (int64_t)1, (int64_t)H * W, b, H, W, wt);
  rc = check_launch("importance_map(gauss axis 1)");
  if (rc) return rc;
  const dim3 grid((W + SM_SW - 1) / SM_SW, (H + SM_SH - 1) / SM_SH);
  hipLaunchKernelGGL(sm_sobel_kernel, grid, dim3(SM_THREADS), 0, st, (const float*)b, C, H, W, (float*)(ws + l.mag),
                     (float*)(ws + l.mm));
  rc = check_launch("importance_map(sobel)");
  if (rc) return rc;
  hipLaunchKernelGGL(sm_minmax_finish_kernel, dim3(1), dim3(SM_THREADS), 0, st, (const float*)(ws + l.mm), sm_tiles(H, W),
                     (float*)(ws + l.res));
  return check_launch("importance_map(min / max)");
}

static inline unsigned sm_flat_grid(int64_t n) {
  const int64_t b = (n + SM_THREADS - 1) / SM_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

extern "C" int wcmc_reflect_index(int i, int n) { return n >= 1 ? sm_reflect(i, n) : -1; }

extern "C" size_t wcmc_importance_map_workspace_bytes(int H, int W, int C) {
  if (!sm_size_ok(H, W) || (C != 1 && C != 3)) return 0;
  return sm_layout(0, H, W, C).end;
}

extern "C" int wcmc_importance_map(const float* img, int H, int W, int C, float* out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  WCMC_REQUIRE(img && out && workspace, WCMC_ERR_BAD_ARG, "importance_map: null pointer");
  WCMC_REQUIRE(C == 1 || C == 3, WCMC_ERR_BAD_ARG, "importance_map: the image must be gray (1 channel) or rgb (3), got %d", C);
  WCMC_REQUIRE(sm_size_ok(H, W), WCMC_ERR_BAD_ARG, "importance_map: bad image size %d x %d", H, W);
  WCMC_REQUIRE(workspace_bytes >= wcmc_importance_map_workspace_bytes(H, W, C), WCMC_ERR_WORKSPACE,
               "importance_map: workspace too small (%zu < %zu bytes)", workspace_bytes, wcmc_importance_map_workspace_bytes(H, W, C));
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const SmLayout l = sm_layout(0, H, W, C);
  int rc = sm_run_map(img, (int64_t)W * C, C, 1, C, H, W, ws, l, st);
  if (rc) return rc;
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(sm_normalise_kernel, dim3(sm_flat_grid(n)), dim3(SM_THREADS), 0, st, (const float*)(ws + l.mag),
                     (const float*)(ws + l.res), n, out);
  return check_launch("importance_map(normalise)");
}

// workspace of sampling_prob: lum, normal x 3, mat planes; one gray and one rgb importance-map workspace; the block sums; the total
struct SpLayout { size_t lum, normal, mat; SmLayout gray, rgb; size_t part, total, end; };
static SpLayout sp_layout(int H, int W, int P) {
  SpLayout l;
  const size_t plane = sm_align((size_t)H * W * sizeof(float));
  l.lum = 0;
  l.normal = plane;
  l.mat = 4 * plane;
  l.gray = sm_layout(5 * plane, H, W, 1);
  l.rgb = sm_layout(l.gray.end, H, W, 3);
  l.part = l.rgb.end;
  l.total = l.part + sm_align((size_t)sm_tiles(H - P, W - P) * sizeof(double));
  l.end = l.total + 256;
  return l;
}

extern "C" size_t wcmc_sampling_prob_workspace_bytes(int H, int W, int patch) {
  if (!sm_size_ok(H, W) || patch < 1 || H <= patch || W <= patch) return 0;
  return sp_layout(H, W, patch).end;
}

extern "C" int wcmc_sampling_prob(const float* raw, const float* gt, int H, int W, int S, int C, int max_depth, int patch,
                                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
  WCMC_REQUIRE(raw && gt && out && workspace, WCMC_ERR_BAD_ARG, "sampling_prob: null pointer");
  WCMC_REQUIRE(sm_size_ok(H, W) && S >= 1 && max_depth >= 0, WCMC_ERR_BAD_ARG, "sampling_prob: bad size (H %d, W %d, S %d, max_depth %d)",
               H, W, S, max_depth);
  WCMC_REQUIRE(C >= 38 + 11 * (max_depth + 1), WCMC_ERR_BAD_ARG, "sampling_prob: %d raw channels, need %d for max_depth %d", C,
               38 + 11 * (max_depth + 1), max_depth);
  WCMC_REQUIRE(patch >= 1 && H > patch && W > patch, WCMC_ERR_BAD_ARG,
               "sampling_prob: the image (%d x %d) must be larger than the patch (%d) in both dimensions", H, W, patch);
  WCMC_REQUIRE(workspace_bytes >= wcmc_sampling_prob_workspace_bytes(H, W, patch), WCMC_ERR_WORKSPACE,
               "sampling_prob: workspace too small (%zu < %zu bytes)", workspace_bytes, wcmc_sampling_prob_workspace_bytes(H, W, patch));
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const SpLayout l = sp_layout(H, W, patch);
  const int64_t npix = (int64_t)H * W;
  float* lum = (float*)(ws + l.lum);
  float* normal = (float*)(ws + l.normal);
  float* mat = (float*)(ws + l.mat);
  // idx_g['normal'] = [17, 20); idx_sbmc['bounce_types'] starts at 24 + 6 * (max_depth + 1), bounce 0 first (datasets.py:232-255)
  hipLaunchKernelGGL(sm_planes_kernel, dim3((unsigned)((npix + SM_THREADS - 1) / SM_THREADS)), dim3(SM_THREADS), 0, st, raw, gt, npix, S,
                     C, 17, 24 + 6 * (max_depth + 1), lum, normal, mat);
  int rc = check_launch("sampling_prob(planes)");
  if (rc) return rc;
  rc = sm_run_map(lum, W, 1, 0, 1, H, W, ws, l.gray, st);
  if (rc) return rc;
  rc = sm_run_map(normal, W, 1, npix, 3, H, W, ws, l.rgb, st);
  if (rc) return rc;
  const int ho = H - patch, wo = W - patch;
  const dim3 grid((wo + SM_SW - 1) / SM_SW, (ho + SM_SH - 1) / SM_SH);
  hipLaunchKernelGGL(sm_combine_kernel, grid, dim3(SM_THREADS), 0, st, (const float*)(ws + l.gray.mag), (const float*)(ws + l.gray.res),
                     (const float*)(ws + l.rgb.mag), (const float*)(ws + l.rgb.res), (const float*)mat, W, patch / 2, ho, wo, out,
                     (double*)(ws + l.part));
  rc = check_launch("sampling_prob(combine)");
  if (rc) return rc;
  hipLaunchKernelGGL(sm_sum_finish_kernel, dim3(1), dim3(SM_THREADS), 0, st, (const double*)(ws + l.part), (int)(grid.x * grid.y),
                     (float*)(ws + l.total));
  rc = check_launch("sampling_prob(sum)");
  if (rc) return rc;
  hipLaunchKernelGGL(sm_divide_kernel, dim3(sm_flat_grid((int64_t)ho * wo)), dim3(SM_THREADS), 0, st, out, (int64_t)ho * wo,
                     (const float*)(ws + l.total));
  return check_launch("sampling_prob(divide)");
}

extern "C" int wcmc_sanitize(float* x, int64_t n, void* stream) {
  WCMC_REQUIRE((x || n == 0) && n >= 0, WCMC_ERR_BAD_ARG, "sanitize: null pointer or negative count");   // (an empty tensor has no storage)
  if (n == 0) return WCMC_OK;
  hipLaunchKernelGGL(sm_sanitize_kernel, dim3(sm_flat_grid(n)), dim3(SM_THREADS), 0, (hipStream_t)stream, x, n);
  return check_launch("sanitize");
}
