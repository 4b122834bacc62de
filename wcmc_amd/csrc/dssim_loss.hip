// A structural-similarity image loss for training: loss = 1 - mean SSIM over every 7x7 window of every plane of an
// (N,C,H,W) pair, forward and backward (the SSIM is that of image_eval.hip / section 10 with an
// optional Reinhard tone map in front and a settable data range).
//
// Everything after the fp32 load is fp64, as in ie_partial_kernel: the tone map, the five window moments, the SSIM map,
// the per-window gradient coefficients and their box sums.  A window of linear radiance near 1e3 loses its variance in
// fp32 E[x^2] - E[x]^2, and the backward's box(a) + T(x) box(b) + T(y) box(c) cancels in the same way (a holds
// -b * mx - c * my): fp32 coefficient planes would put that cancellation into the gradient.
//
// forward : one block per DS_TW x DS_TH tile of WINDOWS of one plane.  It stages the (DS_TW + 6) x (DS_TH + 6) pixels
//           those windows read (tone map applied on load, fp64 LDS planes), takes horizontal then vertical 7-tap sums of
//           x, y, xx, yy, xy, and writes the block's sum of S.  A one-block finish adds the partial sums in a fixed order
//           and writes the 0-d fp32 loss.
// backward: one block per DS_TW x DS_TH tile of PIXELS of one plane.  A pixel lies in the windows whose top-left corner is
//           up to 6 pixels above / left of it, so the block recomputes the coefficients (a, b, c) of the
//           (DS_TW + 6) x (DS_TH + 6) windows around its tile from a 6-pixel halo of the inputs (zero for a window that
//           does not fit the image), then takes the horizontal and the vertical 7-tap sums of the three planes: a gather,
//           no scatter and no atomics.  Nothing is handed from the forward to the backward but the inputs themselves.
// No floating-point atomics anywhere: value and gradient are bitwise reproducible.
#include "common.h"

namespace wcmc {

constexpr int DS_TW = 32, DS_TH = 8, DS_THREADS = 256;
constexpr int DS_WIN = 7, DS_EXT = DS_WIN - 1;                  // a window's extent beyond its top-left pixel
static_assert(DS_TW * DS_TH == DS_THREADS, "one owned window / pixel per thread");

struct DsImage { const float* p; int64_t sn, sc, sh, sw; };

// tonemap 0: none; 1: Reinhard of the clamped value (NaN passes through, as in ie_tonemap)
__device__ __forceinline__ double ds_tonemap(int tonemap, double v) {
  if (tonemap == 0) return v;
  const double c = v < 0.0 ? 0.0 : v;
  return c / (1.0 + c);
}

// d T(v) / d v: what autograd gives for clamp(min = 0) followed by c / (1 + c)
__device__ __forceinline__ double ds_tonemap_grad(int tonemap, double v) {
  if (tonemap == 0) return 1.0;
  if (!(v >= 0.0)) return 0.0;
  const double q = 1.0 / (1.0 + v);
  return q * q;
}

// The SSIM of one window from its five 49-term sums s = {x, y, xx, yy, xy}; with `coef`, also the coefficients of
// d S / d (tone-mapped x_i) = (a + b * x_i + c * y_i) / 49.
template <bool COEF>
__device__ __forceinline__ double ds_window(const double* s, double C1, double C2, double* coef) {
  const double inv = 1.0 / 49.0, cov = 49.0 / 48.0;
  const double mx = s[0] * inv, my = s[1] * inv;
  const double vx = cov * (s[2] * inv - mx * mx), vy = cov * (s[3] * inv - my * my), vxy = cov * (s[4] * inv - mx * my);
  const double A1 = 2.0 * mx * my + C1, A2 = 2.0 * vxy + C2;
  const double B1 = mx * mx + my * my + C1, B2 = vx + vy + C2;
  const double D = B1 * B2;
  const double S = (A1 * A2) / D;
  if (COEF) {
    const double dmu = 2.0 * my * A2 / D - 2.0 * mx * S / B1;
    const double dvx = -S / B2, dvxy = 2.0 * A1 / D;
    coef[0] = dmu - 2.0 * cov * dvx * mx - cov * dvxy * my;
    coef[1] = 2.0 * cov * dvx;
    coef[2] = cov * dvxy;
  }
  return S;
}

__global__ __launch_bounds__(DS_THREADS) void ds_fwd_kernel(DsImage x, DsImage r, int C, int H, int W, int tonemap,
                                                            double C1, double C2, double* __restrict__ ws) {
  constexpr int RW = DS_TW + DS_EXT, RH = DS_TH + DS_EXT, RN = RW * RH;     // staged pixels
  __shared__ double tm[2][RN];                      // tone-mapped x, ref
  __shared__ double hs[5][RH][DS_TW];               // horizontal 7-tap sums of the five moments
  __shared__ double red[DS_THREADS / 64];
  const int tid = threadIdx.x;
  const int n = blockIdx.z / C, c = blockIdx.z - n * C;
  const int wy0 = blockIdx.y * DS_TH, wx0 = blockIdx.x * DS_TW;             // top-left corner of the tile's first window
  const float* xp = x.p + n * x.sn + c * x.sc;
  const float* rp = r.p + n * r.sn + c * r.sc;

  // region pixel (ry, rx) is image pixel (wy0 + ry, wx0 + rx); past the image it is 0 (read by no owned window)
  for (int q = tid; q < RN; q += DS_THREADS) {
    const int ry = q / RW, rx = q - ry * RW;
    const int y = wy0 + ry, xx = wx0 + rx;
    double a = 0.0, b = 0.0;
    if (y < H && xx < W) {
      a = ds_tonemap(tonemap, (double)xp[y * x.sh + xx * x.sw]);
      b = ds_tonemap(tonemap, (double)rp[y * r.sh + xx * r.sw]);
    }
    tm[0][q] = a;
    tm[1][q] = b;
  }
  __syncthreads();
  for (int e = tid; e < RH * DS_TW; e += DS_THREADS) {
    const int ry = e / DS_TW, ox = e - ry * DS_TW;
    const double* pa = &tm[0][ry * RW + ox];
    const double* pb = &tm[1][ry * RW + ox];
    double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < DS_WIN; ++k) {
      const double a = pa[k], b = pb[k];
      s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
    }
#pragma unroll
    for (int m = 0; m < 5; ++m) hs[m][ry][ox] = s[m];
  }
  __syncthreads();
  double v = 0.0;
  {
    const int oy = tid / DS_TW, ox = tid - oy * DS_TW;
    if (wy0 + oy < H - DS_EXT && wx0 + ox < W - DS_EXT) {
      double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < DS_WIN; ++k)
#pragma unroll
        for (int m = 0; m < 5; ++m) s[m] += hs[m][oy + k][ox];
      v = ds_window<false>(s, C1, C2, nullptr);
    }
  }
  // fixed-order block sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < DS_THREADS / 64; ++w) s += red[w];
    ws[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
  }
}

// one block: the partial sums added in a fixed order (thread-strided, a fixed xor tree, the waves in order)
__global__ __launch_bounds__(DS_THREADS) void ds_finish_kernel(const double* __restrict__ ws, int64_t nblk, double n_windows,
                                                               float* __restrict__ loss) {
  __shared__ double red[DS_THREADS / 64];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < nblk; i += DS_THREADS) s += ws[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < DS_THREADS / 64; ++w) t += red[w];
    *loss = (float)(1.0 - t / n_windows);
  }
}

__global__ __launch_bounds__(DS_THREADS) void ds_bwd_kernel(DsImage x, DsImage r, int C, int H, int W, int tonemap,
                                                            double C1, double C2, const float* __restrict__ grad_loss,
                                                            double scale, float* __restrict__ dx) {
  constexpr int CW = DS_TW + DS_EXT, CH = DS_TH + DS_EXT;                   // windows whose coefficients the tile gathers
  constexpr int RW = CW + DS_EXT, RH = CH + DS_EXT, RN = RW * RH;           // pixels those windows read
  __shared__ double tm[2][RN];                      // tone-mapped x, ref
  __shared__ double hbuf[5 * RH * CW];              // hs[5][RH][CW]: horizontal moment sums; then hc[3][CH][DS_TW]
  __shared__ double cf[3][CH][CW];                  // a, b, c per window
  static_assert(3 * CH * DS_TW <= 5 * RH * CW, "hc fits where hs lay");
  const int tid = threadIdx.x;
  const int n = blockIdx.z / C, c = blockIdx.z - n * C;
  const int py0 = blockIdx.y * DS_TH, px0 = blockIdx.x * DS_TW;             // first owned pixel
  const float* xp = x.p + n * x.sn + c * x.sc;
  const float* rp = r.p + n * r.sn + c * r.sc;

  // region pixel (ry, rx) is image pixel (py0 - 6 + ry, px0 - 6 + rx); outside the image it is 0 (read only by windows that
  // do not fit the image, whose coefficients are set to 0 below)
  for (int q = tid; q < RN; q += DS_THREADS) {
    const int ry = q / RW, rx = q - ry * RW;
    const int y = py0 - DS_EXT + ry, xx = px0 - DS_EXT + rx;
    double a = 0.0, b = 0.0;
    if (y >= 0 && y < H && xx >= 0 && xx < W) {
      a = ds_tonemap(tonemap, (double)xp[y * x.sh + xx * x.sw]);
      b = ds_tonemap(tonemap, (double)rp[y * r.sh + xx * r.sw]);
    }
    tm[0][q] = a;
    tm[1][q] = b;
  }
  __syncthreads();
  for (int e = tid; e < RH * CW; e += DS_THREADS) {
    const int ry = e / CW, cx = e - ry * CW;
    const double* pa = &tm[0][ry * RW + cx];
    const double* pb = &tm[1][ry * RW + cx];
    double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < DS_WIN; ++k) {
      const double a = pa[k], b = pb[k];
      s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
    }
#pragma unroll
    for (int m = 0; m < 5; ++m) hbuf[m * RH * CW + e] = s[m];
  }
  __syncthreads();
  // window (cy, cx) of the region has its top-left corner at image pixel (py0 - 6 + cy, px0 - 6 + cx)
  for (int e = tid; e < CH * CW; e += DS_THREADS) {
    const int cy = e / CW, cx = e - cy * CW;
    const int wy = py0 - DS_EXT + cy, wx = px0 - DS_EXT + cx;
    double co[3] = {0.0, 0.0, 0.0};
    if (wy >= 0 && wy < H - DS_EXT && wx >= 0 && wx < W - DS_EXT) {
      double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < DS_WIN; ++k)
#pragma unroll
        for (int m = 0; m < 5; ++m) s[m] += hbuf[m * RH * CW + (cy + k) * CW + cx];
      ds_window<true>(s, C1, C2, co);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) cf[j][cy][cx] = co[j];
  }
  __syncthreads();                                   // cf complete; hs has been read for the last time
  // pixel column px0 + ox lies in the windows of region columns ox .. ox + 6
  for (int e = tid; e < CH * DS_TW; e += DS_THREADS) {
    const int cy = e / DS_TW, ox = e - cy * DS_TW;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double* p = &cf[j][cy][ox];
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < DS_WIN; ++k) s += p[k];
      hbuf[j * CH * DS_TW + e] = s;
    }
  }
  __syncthreads();
  {
    const int oy = tid / DS_TW, ox = tid - oy * DS_TW;
    const int y = py0 + oy, xx = px0 + ox;
    if (y < H && xx < W) {
      double box[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < DS_WIN; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) box[j] += hbuf[j * CH * DS_TW + (oy + k) * DS_TW + ox];
      const int q = (oy + DS_EXT) * RW + ox + DS_EXT;
      const double dT = ds_tonemap_grad(tonemap, (double)xp[y * x.sh + xx * x.sw]);
      const double g = (double)*grad_loss * scale;
      dx[((int64_t)blockIdx.z * H + y) * W + xx] = (float)(g * (box[0] + tm[0][q] * box[1] + tm[1][q] * box[2]) * dT);
    }
  }
}

}  // namespace wcmc

using namespace wcmc;

static int64_t ds_fwd_blocks(int N, int C, int H, int W, int* gx, int* gy) {
  *gx = (W - DS_EXT + DS_TW - 1) / DS_TW;
  *gy = (H - DS_EXT + DS_TH - 1) / DS_TH;
  return (int64_t)*gx * *gy * N * C;
}

// the shapes the launches take: a 7x7 window fits, and the planes / tile rows fit a grid's z / y extent
static bool ds_shape_ok(int N, int C, int H, int W) {
  return N > 0 && C > 0 && H >= DS_WIN && W >= DS_WIN && (int64_t)N * C <= 65535 && (H + DS_TH - 1) / DS_TH <= 65535;
}

extern "C" size_t wcmc_dssim_loss_workspace_bytes(int N, int C, int H, int W) {
  if (!ds_shape_ok(N, C, H, W)) return 0;
  int gx, gy;
  return (size_t)ds_fwd_blocks(N, C, H, W, &gx, &gy) * sizeof(double);
}

static int ds_check(const char* who, const void* x, const void* ref, int tonemap, double data_range, int N, int C, int H, int W) {
  WCMC_REQUIRE(x && ref, WCMC_ERR_BAD_ARG, "%s: null pointer", who);
  WCMC_REQUIRE(N > 0 && C > 0, WCMC_ERR_BAD_ARG, "%s: N = %d, C = %d must be positive", who, N, C);
  WCMC_REQUIRE(H >= DS_WIN && W >= DS_WIN, WCMC_ERR_BAD_ARG, "%s: the image is %d x %d; the 7x7 window needs at least 7 x 7", who,
               H, W);
  WCMC_REQUIRE(ds_shape_ok(N, C, H, W), WCMC_ERR_BAD_ARG, "%s: N * C = %lld planes (at most 65535) or H = %d is too large", who,
               (long long)N * C, H);
  WCMC_REQUIRE(tonemap == 0 || tonemap == 1, WCMC_ERR_BAD_ARG, "%s: unknown tone map %d (0 none, 1 reinhard)", who, tonemap);
  WCMC_REQUIRE(data_range > 0.0, WCMC_ERR_BAD_ARG, "%s: data_range must be positive", who);
  return WCMC_OK;
}

extern "C" int wcmc_dssim_loss_fwd(const float* x, int64_t xsn, int64_t xsc, int64_t xsh, int64_t xsw, const float* ref,
                                   int64_t rsn, int64_t rsc, int64_t rsh, int64_t rsw, int tonemap, double data_range,
                                   float* loss, void* workspace, size_t workspace_bytes, int N, int C, int H, int W,
                                   void* stream) {
  int rc = ds_check("dssim_loss_fwd", x, ref, tonemap, data_range, N, C, H, W);
  if (rc) return rc;
  WCMC_REQUIRE(loss && workspace, WCMC_ERR_BAD_ARG, "dssim_loss_fwd: null pointer");
  const size_t need = wcmc_dssim_loss_workspace_bytes(N, C, H, W);
  WCMC_REQUIRE(workspace_bytes >= need, WCMC_ERR_WORKSPACE, "dssim_loss_fwd: workspace too small (%zu < %zu bytes)",
               workspace_bytes, need);
  int gx, gy;
  const int64_t nblk = ds_fwd_blocks(N, C, H, W, &gx, &gy);
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  const double n_windows = (double)N * C * (double)(H - DS_EXT) * (double)(W - DS_EXT);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ds_fwd_kernel, dim3(gx, gy, N * C), dim3(DS_THREADS), 0, st, DsImage{x, xsn, xsc, xsh, xsw},
                     DsImage{ref, rsn, rsc, rsh, rsw}, C, H, W, tonemap, C1, C2, (double*)workspace);
  rc = check_launch("dssim_loss_fwd(partial)");
  if (rc) return rc;
  hipLaunchKernelGGL(ds_finish_kernel, dim3(1), dim3(DS_THREADS), 0, st, (const double*)workspace, nblk, n_windows, loss);
  return check_launch("dssim_loss_fwd(finish)");
}

extern "C" int wcmc_dssim_loss_bwd(const float* x, int64_t xsn, int64_t xsc, int64_t xsh, int64_t xsw, const float* ref,
                                   int64_t rsn, int64_t rsc, int64_t rsh, int64_t rsw, int tonemap, double data_range,
                                   const float* grad_loss, float* dx, int N, int C, int H, int W, void* stream) {
  int rc = ds_check("dssim_loss_bwd", x, ref, tonemap, data_range, N, C, H, W);
  if (rc) return rc;
  WCMC_REQUIRE(grad_loss && dx, WCMC_ERR_BAD_ARG, "dssim_loss_bwd: null pointer");
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  const double n_windows = (double)N * C * (double)(H - DS_EXT) * (double)(W - DS_EXT);
  hipLaunchKernelGGL(ds_bwd_kernel, dim3((W + DS_TW - 1) / DS_TW, (H + DS_TH - 1) / DS_TH, N * C), dim3(DS_THREADS), 0,
                     (hipStream_t)stream, DsImage{x, xsn, xsc, xsh, xsw}, DsImage{ref, rsn, rsc, rsh, rsw}, C, H, W, tonemap, C1,
                     C2, grad_loss, -1.0 / (49.0 * n_windows), dx);
  return check_launch("dssim_loss_bwd");
}
