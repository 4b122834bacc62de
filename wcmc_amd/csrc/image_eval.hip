// Full-frame evaluation of a denoised image (the image metrics of the reference's test_models.py:234-251 and
// support/metrics.py) and the tile stitch of its inference loop (test_models.py:49-101).
//
// image_eval: the 40 numbers of one (scene, spp) cell -- 5 metrics (RelMSE, RelL1, DSSIM, L1, MSE) x 4 tone maps
// (linear, _tonemap, tonemap gamma 1/2.2, tonemap gamma 1/2.8) x 2 comparisons (out vs tgt, ipt vs tgt) -- in one launch
// plus a one-block finish.  Everything after the fp32 load is fp64: the tone maps, the pointwise terms and the SSIM
// window moments (a 7x7 window of HDR values near 1e3 loses its variance in fp32 E[x^2] - E[x]^2).
//
// Each block owns a TW x TH tile of pixels and stages the tile plus a 3-pixel halo of out / ipt / tgt in LDS once
// (fp32, has_hit composite applied on load).  Then, per tone map and channel: tone-map the staged region into fp64
// LDS planes (and add the pointwise terms of the owned pixels), take horizontal 7-tap sums of the eight moments
// (a, b, r, aa, bb, rr, ar, br; a = out, b = ipt, r = tgt), then vertical 7-tap sums and the SSIM map of both comparisons
// at every owned pixel of the interior (3 pixels in from every edge).  Each block writes its 48 partial sums; the finish
// block adds them in a fixed order.  No floating-point atomics: the result is bitwise reproducible.
//
// stitch_tiles: one launch per batch pastes every tile's owned window into the full-frame radiance and P-buffers --
// the per-tile slice copies of test_models.inference, with the 'replicate' padding of the network output folded into
// the source index.  A copy: bit-identical to the slice assignments.
#include "common.h"

namespace wcmc {

constexpr int IE_TW = 32, IE_TH = 8, IE_HALO = 3;
constexpr int IE_RW = IE_TW + 2 * IE_HALO, IE_RH = IE_TH + 2 * IE_HALO, IE_RN = IE_RW * IE_RH;   // staged region
constexpr int IE_NQ = 48;          // partial sums per block: [cmp 2][tonemap 4][RelMSE, count, RelL1, L1, MSE, SSIM]
constexpr int IE_THREADS = 256;

struct IeImage { const float* p; int64_t sh, sw, sc; };

// numpy's clip: NaN passes through (fmax / fmin would drop it)
__device__ __forceinline__ double ie_clip_lo0(double x) { return x < 0.0 ? 0.0 : x; }
__device__ __forceinline__ double ie_clip_hi1(double x) { return x > 1.0 ? 1.0 : x; }

// tone map t of channel ch of a pixel (c0, c1, c2):
//   0 linear, 1 _tonemap (metrics.py:24-27), 2 / 3 tonemap with gamma 1/2.2 / 1/2.8 on the pixel's own luminance
//   (test_models.py:24-34)
__device__ __forceinline__ double ie_tonemap(int t, const double* c, int ch) {
  if (t == 0) return c[ch];
  if (t == 1) { const double x = ie_clip_lo0(c[ch]); return x / (1.0 + x); }
  const double lum = 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2];
  const double v = ie_clip_lo0(c[ch] / (1.0 + lum / 1.5));
  return ie_clip_hi1(pow(v, t == 2 ? 1.0 / 2.2 : 1.0 / 2.8));
}

// fixed-order block sum of `v` over IE_THREADS threads; every thread gets the result
__device__ __forceinline__ double ie_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();                       // `red` may still be read by the previous call
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < IE_THREADS / 64; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(IE_THREADS) void ie_partial_kernel(IeImage out, IeImage ipt, IeImage tgt, IeImage hit,
                                                                int H, int W, double eps, double* __restrict__ ws) {
  __shared__ float raw[9][IE_RN];                   // [image 3][channel 3] fp32 staged region
  __shared__ double tm[3][IE_RN];                   // one tone-mapped channel of a, b, r
  __shared__ double hs[8][IE_RH][IE_TW];            // horizontal 7-tap sums of the eight moments
  __shared__ double red[IE_THREADS / 64];
  const int tid = threadIdx.x;
  const int ty0 = blockIdx.y * IE_TH, tx0 = blockIdx.x * IE_TW;
  const int nblk = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;

  // stage: region pixel (ry, rx) is image pixel (ty0 - 3 + ry, tx0 - 3 + rx); outside the image it is 0 (read by no
  // owned output)
  for (int e = tid; e < 9 * IE_RN; e += IE_THREADS) {
    const int plane = e / IE_RN, q = e - plane * IE_RN;
    const int img = plane / 3, ch = plane - img * 3;
    const int ry = q / IE_RW, rx = q - ry * IE_RW;
    const int y = ty0 - IE_HALO + ry, x = tx0 - IE_HALO + rx;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      if (img == 0) {
        v = out.p[y * out.sh + x * out.sw + ch * out.sc];
        if (hit.p && hit.p[y * hit.sh + x * hit.sw + ch * hit.sc] == 0.f)     // test_models.py:231-232
          v = ipt.p[y * ipt.sh + x * ipt.sw + ch * ipt.sc];
      } else {
        const IeImage& im = img == 1 ? ipt : tgt;
        v = im.p[y * im.sh + x * im.sw + ch * im.sc];
      }
    }
    raw[plane][q] = v;
  }

  for (int t = 0; t < 4; ++t) {
    // [cmp][RelMSE, count, RelL1, L1, MSE, SSIM]
    double acc[2][6];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[c][k] = 0.0;
    for (int ch = 0; ch < 3; ++ch) {
      __syncthreads();                             // staging done / the previous channel's horizontal pass has read tm
      for (int q = tid; q < IE_RN; q += IE_THREADS) {
        double v[3];
#pragma unroll
        for (int img = 0; img < 3; ++img) {
          const double c[3] = {(double)raw[img * 3 + 0][q], (double)raw[img * 3 + 1][q], (double)raw[img * 3 + 2][q]};
          v[img] = ie_tonemap(t, c, ch);
          tm[img][q] = v[img];
        }
        const int ry = q / IE_RW, rx = q - ry * IE_RW;
        const int y = ty0 - IE_HALO + ry, x = tx0 - IE_HALO + rx;
        const bool own = ry >= IE_HALO && ry < IE_HALO + IE_TH && rx >= IE_HALO && rx < IE_HALO + IE_TW && y < H && x < W;
        if (own) {
          const double r = v[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const double d = v[c] - r;
            const double rel = d * d / (r * r + eps);
            if (rel == rel) { acc[c][0] += rel; acc[c][1] += 1.0; }        // metrics.py:52-53: NaN entries dropped
            acc[c][2] += fabs(d) / (fabs(r) + eps);
            acc[c][3] += fabs(d);
            acc[c][4] += d * d;
          }
        }
      }
      __syncthreads();
      for (int e = tid; e < IE_RH * IE_TW; e += IE_THREADS) {
        const int ry = e / IE_TW, ox = e - ry * IE_TW;
        const double* pa = &tm[0][ry * IE_RW + ox];
        const double* pb = &tm[1][ry * IE_RW + ox];
        const double* pr = &tm[2][ry * IE_RW + ox];
        double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          const double a = pa[k], b = pb[k], r = pr[k];
          s[0] += a; s[1] += b; s[2] += r; s[3] += a * a; s[4] += b * b; s[5] += r * r; s[6] += a * r; s[7] += b * r;
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) hs[m][ry][ox] = s[m];
      }
      __syncthreads();
      {
        const int oy = tid / IE_TW, ox = tid - oy * IE_TW;          // IE_THREADS == IE_TW * IE_TH: one owned pixel each
        const int y = ty0 + oy, x = tx0 + ox;
        if (y >= IE_HALO && y < H - IE_HALO && x >= IE_HALO && x < W - IE_HALO) {
          double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
          for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int m = 0; m < 8; ++m) s[m] += hs[m][oy + k][ox];
          // skimage structural_similarity (< 0.21): data_range 2, K1 0.01, K2 0.03, sample covariance 49/48
          const double inv = 1.0 / 49.0, cov = 49.0 / 48.0;
          const double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0);
          const double ur = s[2] * inv, vr = cov * (s[5] * inv - ur * ur);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const double ux = s[c] * inv;
            const double vx = cov * (s[3 + c] * inv - ux * ux);
            const double vxr = cov * (s[6 + c] * inv - ux * ur);
            const double A1 = 2.0 * ux * ur + C1, A2 = 2.0 * vxr + C2;
            const double B1 = ux * ux + ur * ur + C1, B2 = vx + vr + C2;
            acc[c][5] += (A1 * A2) / (B1 * B2);
          }
        }
      }
    }
    // one tone map's 12 block sums -> ws[q][blk], q = (cmp * 4 + t) * 6 + k
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const double s = ie_block_sum(acc[c][k], red);
        if (tid == 0) ws[(int64_t)((c * 4 + t) * 6 + k) * nblk + blk] = s;
      }
  }
}

// one block: every quantity summed over the blocks in a fixed order (lane-strided, then a fixed xor tree), then the 40
// results [cmp][t][RelMSE, RelL1, DSSIM, L1, MSE]
__global__ __launch_bounds__(IE_THREADS) void ie_finish_kernel(const double* __restrict__ ws, int nblk, int H, int W,
                                                               double* __restrict__ result) {
  __shared__ double tot[IE_NQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = wave; q < IE_NQ; q += IE_THREADS / 64) {
    double s = 0.0;
    for (int i = lane; i < nblk; i += 64) s += ws[(int64_t)q * nblk + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) tot[q] = s;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int ct = threadIdx.x;                     // cmp * 4 + t
    const double* p = tot + ct * 6;
    const double n = 3.0 * (double)H * (double)W;
    const double ns = 3.0 * (double)(H - 2 * IE_HALO) * (double)(W - 2 * IE_HALO);
    double* r = result + ct * 5;
    r[0] = p[0] / p[1];                             // 0 / 0 = NaN when every entry was NaN
    r[1] = p[2] / n;
    r[2] = 1.0 - p[5] / ns;
    r[3] = p[3] / n;
    r[4] = p[4] / n;
  }
}

// ------------------------------------------------------------------ tile stitch
struct StitchArgs {
  const float* rad; int64_t rsb, rsc, rsh, rsw;     // (B, 3, ho, wo) network output
  const float* pb[2]; float* opb[2];                // (B, S, C, P, P) tile P-buffers -> (S, C, H, W), nullable
  const int* coords;                                // (B, 6): i_start, j_start, i_end, j_end, i, j
  float* orad;                                      // (3, H, W)
  int ho, wo, S, C, P, H, W;
};

__global__ __launch_bounds__(256) void ie_stitch_kernel(StitchArgs a) {
  const int b = blockIdx.y;
  const int* cd = a.coords + 6 * b;
  const int i0 = cd[0], j0 = cd[1], i1 = cd[2], j1 = cd[3], ib = cd[4], jb = cd[5];
  // a window outside the frame or the tile is skipped (the wrapper validates the table on the host before upload)
  if (i0 < 0 || j0 < 0 || i1 > a.H || j1 > a.W || i0 >= i1 || j0 >= j1 || i0 < ib || j0 < jb || i1 > ib + a.P ||
      j1 > jb + a.P)
    return;
  const int wh = i1 - i0, ww = j1 - j0;
  const int64_t win = (int64_t)wh * ww;
  const int top = (a.P - a.ho) / 2, left = (a.P - a.wo) / 2;      // F.pad(..., (pad_w//2, ., pad_h//2, .), 'replicate')
  const int64_t hw = (int64_t)a.H * a.W, pp = (int64_t)a.P * a.P;
  const int npb = (a.pb[0] ? 1 : 0) + (a.pb[1] ? 1 : 0);
  const int64_t total = win * (3 + (int64_t)npb * a.S * a.C);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t plane = e / win, q = e - plane * win;
    const int dy = (int)(q / ww), dx = (int)(q - (int64_t)(q / ww) * ww);
    const int y = i0 + dy, x = j0 + dx;             // frame pixel
    const int ty = y - ib, tx = x - jb;             // tile pixel
    if (plane < 3) {
      const int sy = min(max(ty - top, 0), a.ho - 1), sx = min(max(tx - left, 0), a.wo - 1);
      a.orad[plane * hw + (int64_t)y * a.W + x] = a.rad[b * a.rsb + plane * a.rsc + sy * a.rsh + sx * a.rsw];
    } else {
      const int64_t sc = plane - 3, per = (int64_t)a.S * a.C;
      const int which = (sc >= per || !a.pb[0]) ? 1 : 0;
      const int64_t k = sc >= per ? sc - per : sc;  // s * C + c
      a.opb[which][k * hw + (int64_t)y * a.W + x] = a.pb[which][((int64_t)b * per + k) * pp + (int64_t)ty * a.P + tx];
    }
  }
}

}  // namespace wcmc

using namespace wcmc;

static int ie_blocks(int H, int W, int* gx, int* gy) {
  *gx = (W + IE_TW - 1) / IE_TW;
  *gy = (H + IE_TH - 1) / IE_TH;
  return *gx * *gy;
}

extern "C" size_t wcmc_image_eval_workspace_bytes(int H, int W) {
  if (H < 7 || W < 7 || H > 65535 * IE_TH) return 0;
  int gx, gy;
  return (size_t)ie_blocks(H, W, &gx, &gy) * IE_NQ * sizeof(double);
}

extern "C" int wcmc_image_eval(const float* out, int64_t osh, int64_t osw, int64_t osc, const float* ipt, int64_t ish,
                               int64_t isw, int64_t isc, const float* tgt, int64_t tsh, int64_t tsw, int64_t tsc,
                               const float* has_hit, int64_t hsh, int64_t hsw, int64_t hsc, int H, int W, double eps,
                               double* result, void* workspace, size_t workspace_bytes, void* stream) {
  WCMC_REQUIRE(out && ipt && tgt && result && workspace, WCMC_ERR_BAD_ARG, "image_eval: null pointer");
  WCMC_REQUIRE(H >= 7 && W >= 7, WCMC_ERR_BAD_ARG, "image_eval: the image is %d x %d; SSIM's 7x7 window needs at least 7 x 7",
               H, W);
  WCMC_REQUIRE(H <= 65535 * IE_TH, WCMC_ERR_BAD_ARG, "image_eval: H = %d is too large", H);
  WCMC_REQUIRE(eps > 0.0, WCMC_ERR_BAD_ARG, "image_eval: eps must be positive");
  WCMC_REQUIRE(workspace_bytes >= wcmc_image_eval_workspace_bytes(H, W), WCMC_ERR_WORKSPACE,
               "image_eval: workspace too small (%zu < %zu bytes)", workspace_bytes, wcmc_image_eval_workspace_bytes(H, W));
  int gx, gy;
  const int nblk = ie_blocks(H, W, &gx, &gy);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ie_partial_kernel, dim3(gx, gy), dim3(IE_THREADS), 0, st, IeImage{out, osh, osw, osc},
                     IeImage{ipt, ish, isw, isc}, IeImage{tgt, tsh, tsw, tsc}, IeImage{has_hit, hsh, hsw, hsc}, H, W, eps,
                     (double*)workspace);
  int rc = check_launch("image_eval(partial)");
  if (rc) return rc;
  hipLaunchKernelGGL(ie_finish_kernel, dim3(1), dim3(IE_THREADS), 0, st, (const double*)workspace, nblk, H, W, result);
  return check_launch("image_eval(finish)");
}

extern "C" int wcmc_stitch_tiles(const float* rad, int64_t rsb, int64_t rsc, int64_t rsh, int64_t rsw, int ho, int wo,
                                 const float* pbuf_a, const float* pbuf_b, int S, int C, int P, const int* coords, int B,
                                 int H, int W, float* out_rad, float* out_pbuf_a, float* out_pbuf_b, void* stream) {
  WCMC_REQUIRE(rad && coords && out_rad && B > 0 && H > 0 && W > 0 && P > 0, WCMC_ERR_BAD_ARG,
               "stitch_tiles: bad argument (null pointer or non-positive size)");
  WCMC_REQUIRE((ho == P && wo == P) || (ho > 0 && wo > 0 && ho < P && wo < P), WCMC_ERR_BAD_ARG,
               "stitch_tiles: the %d x %d network output must be P x P or smaller in both dimensions (P = %d)", ho, wo, P);
  WCMC_REQUIRE(!pbuf_a == !out_pbuf_a && !pbuf_b == !out_pbuf_b, WCMC_ERR_BAD_ARG,
               "stitch_tiles: a P-buffer needs both its tile and its frame pointer");
  WCMC_REQUIRE(!(pbuf_a || pbuf_b) || (S > 0 && C > 0), WCMC_ERR_BAD_ARG, "stitch_tiles: P-buffers need S > 0 and C > 0");
  WCMC_REQUIRE(B <= 65535, WCMC_ERR_BAD_ARG, "stitch_tiles: at most 65535 tiles per launch");
  StitchArgs a{rad, rsb, rsc, rsh, rsw, {pbuf_a, pbuf_b}, {out_pbuf_a, out_pbuf_b}, coords, out_rad, ho, wo, S, C, P, H, W};
  const int64_t per_tile = (int64_t)P * P * (3 + 2 * (int64_t)(S > 0 ? S : 0) * (C > 0 ? C : 0));
  const int64_t bx = (per_tile + 255) / 256;
  hipLaunchKernelGGL(ie_stitch_kernel, dim3((unsigned)(bx < 1024 ? bx : 1024), B), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("stitch_tiles");
}
