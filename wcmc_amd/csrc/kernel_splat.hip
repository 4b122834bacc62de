// Kernel splatting: every SOURCE pixel q sends w[q, t] * data[q] to the destination q + off(t), t over its k x k taps.
//
// Replaces sbmc.modules.KernelApply(softmax=True, splat=True) and the per-sample step of sbmc.modules.ProgressiveKernelApply
// (upstream: the Halide ops Scatter2Gather + KernelWeighting), which sbmc.Multisteps runs once per sample.  Specification:
// DESIGN.md section 18; fp64 restatement: tests/splat_ref.py.
//
// Forward (source-owned tiles, no atomics): a 256-thread block owns 16 x 8 source pixels and walks them row by row.  For the 16
// pixels of a row, 16 lanes own one pixel exactly as in kernel_apply.hip: each lane loads the 16-byte vectors j, j + 16, ... of
// the pixel's tap row (a wave instruction reads 4 x 256 contiguous bytes), keeps its <= 28 logits in registers one row ahead of
// the arithmetic, and writes the pixel's WEIGHTS to LDS ([16][444] floats, double-buffered).  Behind one barrier per row the
// roles turn: every thread owns four of the block's (8 + 2r) x (16 + 2r) DESTINATIONS, with their C + 1 sums in registers, and
// gathers from the row's weights -- for source column sx the weight of tap (hy - sy, hx - sx), consecutive lanes reading
// consecutive floats -- times the source's radiance (an LDS broadcast).  LDS float adds were the first form of this kernel and
// ran at 0.3 lanes per clock (24 x the gather's time); this form has none.  The block stores its tile of sums to a workspace slab
// with plain coalesced stores; a second launch sums, per destination pixel, the <= 4 x 3 slabs that cover it in tile order (on
// top of the previous sums when accumulating).  Every sum has a fixed order: the forward is bitwise reproducible.
//
// Backward: both gradients are gathers around the source pixel, so the kernel has the structure of the gather's forward: the
// zero-extended halo of (g_r, g_w) sits in LDS, the weights are recomputed from the logits (softmax mode: from the saved
// log-sum-exp), the thread group that owns q writes its 441 d_logits coalesced and d_data[q] as one per-pixel sum.  No atomics:
// the backward is bitwise reproducible.
#include <math.h>

#include "common.h"

namespace wcmc {

constexpr int SP_TW = 16, SP_TH = 8;      // source pixels per block: 4 waves x 8 quads of 4 x-neighbours
constexpr int SP_CELLS = 4;               // destinations per thread: 256 * 4 >= (8 + 20) * (16 + 20)
constexpr int SP_MAXV = 7;                // float4 per lane: 16 * 7 * 4 = 448 >= 441 taps
constexpr float SP_NEG = -1.0e30f;        // logit of a tap slot beyond k*k: exp2() of it is exactly 0
constexpr float SP_LOG2E = 1.4426950408889634f;
constexpr int LM_BLOCKS = 64;             // partial maxima per image
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct SPParams {
  const float* logits; int64_t lsn, lsh, lsw;
  const float* data; int64_t dsn, dsc, dsh, dsw;
  float* sum_r; float* sum_w;                             // fwd: (N,C,h,w) and (N,h,w), contiguous
  float* ws;                                              // fwd: [N][tiles][C + 1][hrows][hcols] slabs
  const float* g_r; int64_t gsn, gsc, gsh, gsw;           // bwd, may be null
  const float* g_w; int64_t wsn, wsh, wsw;                // bwd, may be null
  float* lse;                                             // softmax mode: fwd writes (may be null), bwd reads
  const float* shift;                                     // shift mode: (N,)
  float* dlogits; int64_t qsn, qsh, qsw;                  // bwd
  float* ddata;                                           // bwd, (N,C,h,w) contiguous, may be null
  int N, C, h, w, k, r, taps, nvec, hcols, hrows, hs, mode;
};

__device__ __forceinline__ float sp_group_sum(float v) {       // over the 16 lanes that own a pixel, fixed order
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}
__device__ __forceinline__ float sp_group_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 16));
  return v;
}

// this lane's vectors of one pixel's tap row; slots beyond k*k become SP_NEG so that the arithmetic needs no per-tap predicate
__device__ __forceinline__ void sp_load_quad(const SPParams& p, int n, int y, int x, int j, int taps, int nvec, float4* lv) {
  const bool valid = y < p.h && x < p.w;
  const float* lrow = p.logits + (int64_t)n * p.lsn + (int64_t)y * p.lsh + (int64_t)x * p.lsw;
#pragma unroll
  for (int i = 0; i < SP_MAXV; ++i) {
    const int vi = j + 16 * i;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid && vi < nvec) v = *reinterpret_cast<const float4*>(lrow + 4 * vi);
    const int t = 4 * vi;
    if (t + 0 >= taps) v.x = SP_NEG;
    if (t + 1 >= taps) v.y = SP_NEG;
    if (t + 2 >= taps) v.z = SP_NEG;
    if (t + 3 >= taps) v.w = SP_NEG;
    lv[i] = v;
  }
}

// KS > 0: compile-time kernel size (LDS offsets become immediates); KS == 0: runtime p.k.
// CT > 0: compile-time channel count; CT == 0: runtime p.C (<= 4).
template <int KS, int CT>
__global__ __launch_bounds__(256, KS > 0 ? 2 : 1) void kernel_splat_fwd_kernel(SPParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];       // 2 x [16][P] weights of a source row, 2 x [16] radiance
  const int C = CT > 0 ? CT : p.C;
  const int kk = KS > 0 ? KS : p.k;
  const int taps = KS > 0 ? KS * KS : p.taps;
  const int nvec = (taps + 3) / 4;
  const int P = 4 * nvec;                                 // floats per source pixel in LDS
  float4* const dsm = reinterpret_cast<float4*>(smem + 2 * SP_TW * P);      // {1, c0, c1, c2} per source pixel: two FMA operand pairs
  float* const d3sm = smem + 2 * SP_TW * P + 2 * SP_TW * 4;                // c3 (C == 4)

  const int tiles_x = (p.w + SP_TW - 1) / SP_TW;
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * SP_TH, tx0 = (blockIdx.x % tiles_x) * SP_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15;
  const int px = 4 * wave + (lane >> 4);                  // this lane group's source pixel in the row
  const int x = tx0 + px;
  static_assert(SP_TW == 16, "a row of the tile is one pixel quad per wave");

  // this thread's destinations (hy, hx) of the tile's halo, and per destination the source columns that reach it
  const int cells = p.hrows * p.hcols;
  int chy[SP_CELLS], chx[SP_CELLS];
  unsigned cmask[SP_CELLS];
  f32x2 a01[SP_CELLS], a23[SP_CELLS];                     // {sum_w, c0}, {c1, c2}: one packed FMA each per weight
  float a4[SP_CELLS];                                     // c3 (C == 4)
#pragma unroll
  for (int m = 0; m < SP_CELLS; ++m) {
    const int id = threadIdx.x + 256 * m;
    chy[m] = id < cells ? id / p.hcols : -(1 << 20);      // (beyond the tile: no source row reaches it)
    chx[m] = id < cells ? id % p.hcols : 0;
    cmask[m] = 0u;
#pragma unroll
    for (int sx = 0; sx < SP_TW; ++sx)
      if ((unsigned)(chx[m] - sx) < (unsigned)kk) cmask[m] |= 1u << sx;
    a01[m] = f32x2{0.f, 0.f}; a23[m] = f32x2{0.f, 0.f}; a4[m] = 0.f;
  }
  const float sh = p.mode == WCMC_SPLAT_SHIFT ? p.shift[n] : 0.f;

  float4 lvA[SP_MAXV], lvB[SP_MAXV];
  sp_load_quad(p, n, ty0, x, j, taps, nvec, lvA);

  // one source row: `lv` holds its logits, the next row's go into `nxt` first
  auto step = [&](int sy, float4* lv, float4* nxt) {
    if (sy + 1 < SP_TH) sp_load_quad(p, n, ty0 + sy + 1, x, j, taps, nvec, nxt);
    const int y = ty0 + sy;
    const bool valid = y < p.h && x < p.w;                // uniform across the 16-lane group
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
      const float* dp = p.data + (int64_t)n * p.dsn + (int64_t)y * p.dsh + (int64_t)x * p.dsw;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) d[c] = dp[(int64_t)c * p.dsc];
    }
    float m = sh, scale = 1.f;
    if (p.mode == WCMC_SPLAT_SOFTMAX) {
      m = SP_NEG;
#pragma unroll
      for (int i = 0; i < SP_MAXV; ++i) m = fmaxf(fmaxf(m, fmaxf(lv[i].x, lv[i].y)), fmaxf(lv[i].z, lv[i].w));
      m = sp_group_max(m);
    }
    // w = exp(l - m): the difference first, so that the rounding of a large shift does not enter the exponent
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SP_MAXV; ++i) {
      float* l = reinterpret_cast<float*>(&lv[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        l[e] = __builtin_amdgcn_exp2f((l[e] - m) * SP_LOG2E);
        s += l[e];
      }
    }
    if (p.mode == WCMC_SPLAT_SOFTMAX) {
      s = sp_group_sum(s);
      scale = 1.f / s;
      if (valid && j == 0 && p.lse) p.lse[((int64_t)n * p.h + y) * p.w + x] = m + __logf(s);
    }
    // the row's weights and radiance to LDS (a pixel outside the image sends nothing)
    float* const wb = smem + (sy & 1) * (SP_TW * P);
#pragma unroll
    for (int i = 0; i < SP_MAXV; ++i) {
      const int vi = j + 16 * i;
      if (vi < nvec)
        *reinterpret_cast<float4*>(wb + px * P + 4 * vi) =
            valid ? make_float4(lv[i].x * scale, lv[i].y * scale, lv[i].z * scale, lv[i].w * scale) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (j == 0) {
      dsm[(sy & 1) * SP_TW + px] = make_float4(1.f, d[0], d[1], d[2]);
      if (C == 4) d3sm[(sy & 1) * SP_TW + px] = d[3];
    }
    // One barrier per row: the weights written above are read below, and the buffer written two rows later is this one --
    // behind the next row's barrier, which no thread passes before every thread has left this row's reads.
    __syncthreads();
    // destination (hy, hx) takes tap (hy - sy, hx - sx) of source column sx: index sx * P + (hy - sy) * k + hx - sx.  The index
    // stays inside the buffer for every sx when the row reaches the destination (0 <= hy - sy < k), so the read is
    // unconditional and the VALUE is masked: bit sx of cmask, sign-extended, ANDed onto the float (a dead read becomes +0).
    const float4* const dp = dsm + (sy & 1) * SP_TW;
#pragma unroll
    for (int mm = 0; mm < SP_CELLS; ++mm) {
      const int dyi = chy[mm] - sy;
      if ((unsigned)dyi < (unsigned)kk) {                 // (a wave's 64 destinations span two or three rows: mostly uniform)
        const float* const wp = wb + dyi * kk + chx[mm];
#pragma unroll 4                                          // (all 16 at once put 16 + 64 registers of reads in flight)
        for (int sx = 0; sx < SP_TW; ++sx) {
          const float4 dv = dp[sx];
          const unsigned keep = (unsigned)__builtin_amdgcn_sbfe((int)cmask[mm], sx, 1);        // bit sx -> 0 or ~0
          const float wt = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, wp[sx * (P - 1)]) & keep);
          const f32x2 w2 = {wt, wt};
          a01[mm] = __builtin_elementwise_fma(w2, f32x2{dv.x, dv.y}, a01[mm]);                  // (fma(w, 1, s) = s + w exactly)
          a23[mm] = __builtin_elementwise_fma(w2, f32x2{dv.z, dv.w}, a23[mm]);
          if (C == 4) a4[mm] = fmaf(wt, d3sm[(sy & 1) * SP_TW + sx], a4[mm]);
        }
      }
    }
  };
  static_assert(SP_TH % 2 == 0, "the row loop is unrolled by two");
#pragma unroll 1
  for (int sy = 0; sy < SP_TH; sy += 2) {
    step(sy, lvA, lvB);
    step(sy + 1, lvB, lvA);
  }

  // the block's tile of sums to its slab: [C + 1][hrows * hcols], consecutive lanes on consecutive floats
  float* slab = p.ws + ((int64_t)n * gridDim.x + blockIdx.x) * (C + 1) * cells;
#pragma unroll
  for (int mm = 0; mm < SP_CELLS; ++mm) {
    const int id = threadIdx.x + 256 * mm;
    if (id < cells) {
      const float av[5] = {a01[mm].x, a01[mm].y, a23[mm].x, a23[mm].y, a4[mm]};
#pragma unroll
      for (int c = 0; c < 5; ++c)
        if (c <= C) slab[c * cells + id] = av[c];
    }
  }
}

// One thread per destination pixel: the slabs of the tiles whose halo covers it, in tile order, on top of the previous sums
// when accumulating.
__global__ __launch_bounds__(256) void kernel_splat_combine_kernel(SPParams p, int accumulate) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.h * p.w) return;
  const int n = blockIdx.y, y = idx / p.w, x = idx - y * p.w;
  const int tiles_x = (p.w + SP_TW - 1) / SP_TW, tiles_y = (p.h + SP_TH - 1) / SP_TH;
  const int cells = p.hrows * p.hcols;
  // tile row ty covers destination rows [ty * SP_TH - r, ty * SP_TH + SP_TH - 1 + r]
  const int ty_lo = (max(0, y - p.r - SP_TH + 1) + SP_TH - 1) / SP_TH, ty_hi = min(tiles_y - 1, (y + p.r) / SP_TH);
  const int tx_lo = (max(0, x - p.r - SP_TW + 1) + SP_TW - 1) / SP_TW, tx_hi = min(tiles_x - 1, (x + p.r) / SP_TW);
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  float* ow = p.sum_w + ((int64_t)n * p.h + y) * p.w + x;
  float* orr = p.sum_r + ((int64_t)n * p.C * p.h + y) * p.w + x;
  const int64_t cs = (int64_t)p.h * p.w;
  if (accumulate) {
    acc[0] = *ow;
    for (int c = 0; c < p.C; ++c) acc[c + 1] = orr[c * cs];
  }
  for (int ty = ty_lo; ty <= ty_hi; ++ty)
    for (int tx = tx_lo; tx <= tx_hi; ++tx) {
      const int hy = y - ty * SP_TH + p.r, hx = x - tx * SP_TW + p.r;
      const float* slab = p.ws + ((int64_t)n * tiles_x * tiles_y + ty * tiles_x + tx) * (p.C + 1) * cells + hy * p.hcols + hx;
      for (int pl = 0; pl <= p.C; ++pl) acc[pl] += slab[pl * cells];
    }
  *ow = acc[0];
  for (int c = 0; c < p.C; ++c) orr[c * cs] = acc[c + 1];
}

// C4: four channels, g_w in a plane of its own; else the halo pixel is {g0, g1, g2, g_w}
template <int KS, bool C4>
__global__ __launch_bounds__(256, KS > 0 ? 2 : 1) void kernel_splat_bwd_kernel(SPParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int kk = KS > 0 ? KS : p.k;
  const int taps = KS > 0 ? KS * KS : p.taps;
  const int nvec = (taps + 3) / 4;
  const int hs = p.hs, plane = p.hrows * hs;
  float4* halo = reinterpret_cast<float4*>(smem);
  float* halow = smem + 4 * plane;                         // C4 only

  const int tiles_x = (p.w + SP_TW - 1) / SP_TW;
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * SP_TH, tx0 = (blockIdx.x % tiles_x) * SP_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, j = lane & 15;
  constexpr int NIT = SP_TW * SP_TH / 16;
  auto pixel = [&](int it, int& ty, int& tx) {
    const int pi = wave * (NIT * 4) + it * 4 + q;
    ty = pi / SP_TW; tx = pi % SP_TW;
  };

  float4 lvA[SP_MAXV], lvB[SP_MAXV];
  {
    int ty, tx;
    pixel(0, ty, tx);
    sp_load_quad(p, n, ty0 + ty, tx0 + tx, j, taps, nvec, lvA);
  }
  // the zero-extended halo of the incoming gradients (an absent gradient is zero)
  for (int i = threadIdx.x; i < p.hrows * p.hcols; i += blockDim.x) {
    const int hy = i / p.hcols, hx = i - hy * p.hcols;
    const int y = ty0 + hy - p.r, x = tx0 + hx - p.r;
    float g[4] = {0.f, 0.f, 0.f, 0.f}, gw = 0.f;
    if ((unsigned)y < (unsigned)p.h && (unsigned)x < (unsigned)p.w) {
      if (p.g_r) {
        const float* gp = p.g_r + (int64_t)n * p.gsn + (int64_t)y * p.gsh + (int64_t)x * p.gsw;
        for (int c = 0; c < p.C; ++c) g[c] = gp[(int64_t)c * p.gsc];
      }
      if (p.g_w) gw = p.g_w[(int64_t)n * p.wsn + (int64_t)y * p.wsh + (int64_t)x * p.wsw];
    }
    halo[hy * hs + hx] = make_float4(g[0], g[1], g[2], C4 ? g[3] : gw);
    if (C4) halow[hy * hs + hx] = gw;
  }

  int toff[SP_MAXV][4];                                    // halo index of each tap's destination, relative to the source
#pragma unroll
  for (int i = 0; i < SP_MAXV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int t = 4 * (j + 16 * i) + e;
      const int dy = t / kk, dx = t - dy * kk;
      toff[i][e] = t < taps ? dy * hs + dx : 0;            // (slot beyond k*k: its weight is 0)
    }
  const float sh = p.mode == WCMC_SPLAT_SHIFT ? p.shift[n] : 0.f;
  __syncthreads();

  // one pixel quad: `lv` holds its logits, the next quad's go into `nxt` first.  The loop below is unrolled by two only (the
  // buffers swap): unrolled over all eight quads the compiler keeps several quads' loads live, past 256 registers.
  auto step = [&](int it, float4* lv, float4* nxt) {
    if (it + 1 < NIT) {
      int ty, tx;
      pixel(it + 1, ty, tx);
      sp_load_quad(p, n, ty0 + ty, tx0 + tx, j, taps, nvec, nxt);
    }
    int ty, tx;
    pixel(it, ty, tx);
    const int y = ty0 + ty, x = tx0 + tx;
    const bool valid = y < p.h && x < p.w;                 // uniform across the 16-lane group
    const int64_t pix = ((int64_t)n * p.h + y) * p.w + x;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    float m = sh;
    if (valid) {
      const float* dp = p.data + (int64_t)n * p.dsn + (int64_t)y * p.dsh + (int64_t)x * p.dsw;
      for (int c = 0; c < p.C; ++c) d[c] = dp[(int64_t)c * p.dsc];
      if (p.mode == WCMC_SPLAT_SOFTMAX) m = p.lse[pix];
    }
    const int hb = ty * hs + tx;
    // pass 1: w_t (kept in place of the logit), w_t * G_t, and the sums over the taps
    float wg[SP_MAXV][4];
    float S = 0.f, dd0 = 0.f, dd1 = 0.f, dd2 = 0.f, dd3 = 0.f;
#pragma unroll
    for (int i = 0; i < SP_MAXV; ++i) {
      float* l = reinterpret_cast<float*>(&lv[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float wt = __builtin_amdgcn_exp2f((l[e] - m) * SP_LOG2E);
        const float4 g = halo[hb + toff[i][e]];
        float G;
        if (C4) G = fmaf(d[0], g.x, fmaf(d[1], g.y, fmaf(d[2], g.z, fmaf(d[3], g.w, halow[hb + toff[i][e]]))));
        else G = fmaf(d[0], g.x, fmaf(d[1], g.y, fmaf(d[2], g.z, g.w)));
        l[e] = wt;
        wg[i][e] = wt * G;
        S += wg[i][e];
        dd0 = fmaf(wt, g.x, dd0); dd1 = fmaf(wt, g.y, dd1); dd2 = fmaf(wt, g.z, dd2);
        if (C4) dd3 = fmaf(wt, g.w, dd3);
      }
    }
    if (p.mode == WCMC_SPLAT_SOFTMAX) S = sp_group_sum(S);
    else S = 0.f;
    if (p.ddata) {
      dd0 = sp_group_sum(dd0); dd1 = sp_group_sum(dd1); dd2 = sp_group_sum(dd2);
      if (C4) dd3 = sp_group_sum(dd3);
      if (valid && j == 0) {
        const float dv[4] = {dd0, dd1, dd2, dd3};
        for (int c = 0; c < p.C; ++c) p.ddata[(((int64_t)n * p.C + c) * p.h + y) * p.w + x] = dv[c];
      }
    }
    // pass 2: d l_t = w_t * (G_t - S), S = 0 in shift mode
    if (valid) {
      float* qrow = p.dlogits + (int64_t)n * p.qsn + (int64_t)y * p.qsh + (int64_t)x * p.qsw;
#pragma unroll
      for (int i = 0; i < SP_MAXV; ++i) {
        const float* l = reinterpret_cast<const float*>(&lv[i]);
        const int vi = j + 16 * i;
        if (vi < nvec)
          *reinterpret_cast<float4*>(qrow + 4 * vi) = make_float4(wg[i][0] - l[0] * S, wg[i][1] - l[1] * S,
                                                                  wg[i][2] - l[2] * S, wg[i][3] - l[3] * S);
      }
    }
  };
  static_assert(NIT % 2 == 0, "the quad loop is unrolled by two");
#pragma unroll 1
  for (int it = 0; it < NIT; it += 2) {
    step(it, lvA, lvB);
    step(it + 1, lvB, lvA);
  }
}

// ------------------------------------------------------------------ per-image maximum of the logits
// torch.amax semantics: a NaN operand wins.  max is exact, so any fixed order gives the same bits; the order here is fixed.
__device__ __forceinline__ float lm_nanmax(float a, float b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }

__global__ __launch_bounds__(256) void logit_max_partial_kernel(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw,
                                                                float* partial, int h, int w, int taps) {
  const int n = blockIdx.y, b = blockIdx.x;
  const int grp = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int nvec = (taps + 3) / 4, npix = h * w;
  float m = -INFINITY;
  for (int pix = b * 16 + grp; pix < npix; pix += LM_BLOCKS * 16) {
    const int y = pix / w, x = pix - y * w;
    const float* lrow = logits + (int64_t)n * lsn + (int64_t)y * lsh + (int64_t)x * lsw;
    for (int vi = j; vi < nvec; vi += 16) {
      const float4 v = *reinterpret_cast<const float4*>(lrow + 4 * vi);
      const int t = 4 * vi;
      m = lm_nanmax(m, v.x);                                // (4 * vi < taps always)
      if (t + 1 < taps) m = lm_nanmax(m, v.y);
      if (t + 2 < taps) m = lm_nanmax(m, v.z);
      if (t + 3 < taps) m = lm_nanmax(m, v.w);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = lm_nanmax(m, __shfl_xor(m, o, 64));
  __shared__ float wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) partial[n * LM_BLOCKS + b] = lm_nanmax(lm_nanmax(wm[0], wm[1]), lm_nanmax(wm[2], wm[3]));
}

__global__ __launch_bounds__(64) void logit_max_finish_kernel(const float* partial, float* out) {
  float m = partial[blockIdx.x * LM_BLOCKS + threadIdx.x];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = lm_nanmax(m, __shfl_xor(m, o, 64));
  if (threadIdx.x == 0) out[blockIdx.x] = m;
}
static_assert(LM_BLOCKS == 64, "the finish kernel reads one partial maximum per lane");

static int sp_fill(SPParams& p, const char* who, int N, int C, int h, int w, int k2, int mode, const float* shift) {
  const int k = (int)lround(sqrt((double)(k2 > 0 ? k2 : 0)));
  WCMC_REQUIRE(k2 > 0 && k * k == k2, WCMC_ERR_BAD_ARG, "%s: k2 = %d is not a square", who, k2);
  WCMC_REQUIRE((k & 1) && k <= 21, WCMC_ERR_BAD_ARG, "%s: k = %d must be odd and at most 21", who, k);
  static_assert((SP_TH + 20) * (SP_TW + 20) <= 256 * SP_CELLS, "every destination of a k = 21 tile has a thread");
  WCMC_REQUIRE(C >= 1 && C <= 4, WCMC_ERR_BAD_ARG, "%s: C = %d channels (1..4 are supported)", who, C);
  WCMC_REQUIRE(N > 0 && N <= 65535 && h > 0 && w > 0 && (int64_t)h * w < (1ll << 30), WCMC_ERR_BAD_ARG,
               "%s: unsupported shape (N=%d h=%d w=%d)", who, N, h, w);
  WCMC_REQUIRE(mode == WCMC_SPLAT_SOFTMAX || mode == WCMC_SPLAT_SHIFT, WCMC_ERR_BAD_ARG, "%s: unknown mode %d", who, mode);
  WCMC_REQUIRE(mode != WCMC_SPLAT_SHIFT || shift, WCMC_ERR_BAD_ARG, "%s: shift mode needs a shift pointer", who);
  p.N = N; p.C = C; p.h = h; p.w = w; p.k = k; p.r = k / 2; p.taps = k2; p.nvec = (k2 + 3) / 4;
  p.hcols = SP_TW + k - 1; p.hrows = SP_TH + k - 1;
  p.hs = p.hcols | 1;                                                        // odd row stride: rows shift the LDS banks
  p.mode = mode; p.shift = shift;
  return 0;
}
static dim3 sp_grid(int N, int h, int w) {
  return dim3((unsigned)(((h + SP_TH - 1) / SP_TH) * ((w + SP_TW - 1) / SP_TW)), (unsigned)N);
}

}  // namespace wcmc

using namespace wcmc;

static size_t sp_ws_bytes(int N, int C, int h, int w, int k) {
  const size_t tiles = (size_t)((h + SP_TH - 1) / SP_TH) * ((w + SP_TW - 1) / SP_TW);
  return (size_t)N * tiles * (C + 1) * (SP_TH + k - 1) * (SP_TW + k - 1) * sizeof(float);
}

extern "C" size_t wcmc_kernel_splat_fwd_workspace_bytes(int N, int C, int h, int w, int k2) {
  SPParams p = {};
  if (sp_fill(p, "kernel_splat_fwd_workspace_bytes", N, C, h, w, k2, WCMC_SPLAT_SOFTMAX, nullptr)) return 0;
  return sp_ws_bytes(N, C, h, w, p.k);
}

extern "C" int wcmc_kernel_splat_fwd(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw, const float* data,
                                     int64_t dsn, int64_t dsc, int64_t dsh, int64_t dsw, float* sum_r, float* sum_w,
                                     float* lse, int mode, const float* shift, int accumulate, void* workspace,
                                     size_t workspace_bytes, int N, int C, int h, int w, int k2, void* stream) {
  SPParams p = {};
  if (int rc = sp_fill(p, "kernel_splat_fwd", N, C, h, w, k2, mode, shift)) return rc;
  WCMC_REQUIRE(data && sum_r && sum_w && workspace, WCMC_ERR_BAD_ARG, "kernel_splat_fwd: null pointer");
  WCMC_REQUIRE(nhwc_view_ok(logits, lsn, lsh, lsw, k2), WCMC_ERR_ALIGNMENT,
               "kernel_splat_fwd: logits violate the NHWC-view contract");
  WCMC_REQUIRE(workspace_bytes >= sp_ws_bytes(N, C, h, w, p.k), WCMC_ERR_WORKSPACE,
               "kernel_splat_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, sp_ws_bytes(N, C, h, w, p.k));
  p.logits = logits; p.lsn = lsn; p.lsh = lsh; p.lsw = lsw;
  p.data = data; p.dsn = dsn; p.dsc = dsc; p.dsh = dsh; p.dsw = dsw;
  p.sum_r = sum_r; p.sum_w = sum_w; p.lse = lse; p.ws = static_cast<float*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)(2 * SP_TW * 4 * p.nvec + 2 * SP_TW * 4 + 2 * SP_TW) * sizeof(float);       // 57,472 B at k = 21
  if (p.k == 21 && C == 3) hipLaunchKernelGGL((kernel_splat_fwd_kernel<21, 3>), sp_grid(N, h, w), dim3(256), lds, st, p);
  else hipLaunchKernelGGL((kernel_splat_fwd_kernel<0, 0>), sp_grid(N, h, w), dim3(256), lds, st, p);
  if (int rc = check_launch("kernel_splat_fwd")) return rc;
  hipLaunchKernelGGL(kernel_splat_combine_kernel, dim3((unsigned)((h * w + 255) / 256), (unsigned)N), dim3(256), 0, st, p,
                     accumulate ? 1 : 0);
  return check_launch("kernel_splat_fwd(combine)");
}

extern "C" int wcmc_kernel_splat_bwd(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw, const float* data,
                                     int64_t dsn, int64_t dsc, int64_t dsh, int64_t dsw, const float* g_r, int64_t gsn,
                                     int64_t gsc, int64_t gsh, int64_t gsw, const float* g_w, int64_t wsn, int64_t wsh,
                                     int64_t wsw, const float* lse, int mode, const float* shift, float* d_logits,
                                     int64_t qsn, int64_t qsh, int64_t qsw, float* d_data, int N, int C, int h, int w,
                                     int k2, void* stream) {
  SPParams p = {};
  if (int rc = sp_fill(p, "kernel_splat_bwd", N, C, h, w, k2, mode, shift)) return rc;
  WCMC_REQUIRE(data && (g_r || g_w), WCMC_ERR_BAD_ARG, "kernel_splat_bwd: null pointer (data, or both gradients)");
  WCMC_REQUIRE(mode != WCMC_SPLAT_SOFTMAX || lse, WCMC_ERR_BAD_ARG, "kernel_splat_bwd: softmax mode needs the saved lse");
  WCMC_REQUIRE(nhwc_view_ok(logits, lsn, lsh, lsw, k2) && nhwc_view_ok(d_logits, qsn, qsh, qsw, k2), WCMC_ERR_ALIGNMENT,
               "kernel_splat_bwd: logits/d_logits violate the NHWC-view contract");
  p.logits = logits; p.lsn = lsn; p.lsh = lsh; p.lsw = lsw;
  p.data = data; p.dsn = dsn; p.dsc = dsc; p.dsh = dsh; p.dsw = dsw;
  p.g_r = g_r; p.gsn = gsn; p.gsc = gsc; p.gsh = gsh; p.gsw = gsw;
  p.g_w = g_w; p.wsn = wsn; p.wsh = wsh; p.wsw = wsw;
  p.lse = const_cast<float*>(lse);
  p.dlogits = d_logits; p.qsn = qsn; p.qsh = qsh; p.qsw = qsw; p.ddata = d_data;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)(C == 4 ? 5 : 4) * p.hrows * p.hs * sizeof(float);
  if (p.k == 21 && C <= 3) hipLaunchKernelGGL((kernel_splat_bwd_kernel<21, false>), sp_grid(N, h, w), dim3(256), lds, st, p);
  else if (C <= 3) hipLaunchKernelGGL((kernel_splat_bwd_kernel<0, false>), sp_grid(N, h, w), dim3(256), lds, st, p);
  else hipLaunchKernelGGL((kernel_splat_bwd_kernel<0, true>), sp_grid(N, h, w), dim3(256), lds, st, p);
  return check_launch("kernel_splat_bwd");
}

extern "C" size_t wcmc_logit_max_workspace_bytes(int N) { return N > 0 ? (size_t)N * LM_BLOCKS * sizeof(float) : 0; }

extern "C" int wcmc_logit_max(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw, float* out, void* workspace,
                              size_t workspace_bytes, int N, int h, int w, int k2, void* stream) {
  WCMC_REQUIRE(N > 0 && N <= 65535 && h > 0 && w > 0 && (int64_t)h * w < (1ll << 30) && k2 > 0, WCMC_ERR_BAD_ARG,
               "logit_max: unsupported shape (N=%d h=%d w=%d k2=%d)", N, h, w, k2);
  WCMC_REQUIRE(out && workspace, WCMC_ERR_BAD_ARG, "logit_max: null pointer");
  WCMC_REQUIRE(nhwc_view_ok(logits, lsn, lsh, lsw, k2), WCMC_ERR_ALIGNMENT, "logit_max: logits violate the NHWC-view contract");
  WCMC_REQUIRE(workspace_bytes >= wcmc_logit_max_workspace_bytes(N), WCMC_ERR_WORKSPACE,
               "logit_max: workspace of %zu bytes, %zu needed", workspace_bytes, wcmc_logit_max_workspace_bytes(N));
  hipStream_t st = (hipStream_t)stream;
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(logit_max_partial_kernel, dim3(LM_BLOCKS, (unsigned)N), dim3(256), 0, st, logits, lsn, lsh, lsw, partial, h,
                     w, k2);
  if (int rc = check_launch("logit_max")) return rc;
  hipLaunchKernelGGL(logit_max_finish_kernel, dim3((unsigned)N), dim3(64), 0, st, partial, out);
  return check_launch("logit_max");
}
