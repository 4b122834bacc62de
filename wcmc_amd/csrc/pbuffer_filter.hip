// Filter a frame by its P-buffer: non-local means whose patch distance is taken between the per-pixel statistics of the path
// embedding (Ray Histogram Fusion with the learned manifold in place of the colour histograms).  Forward only.
// Specification: DESIGN.md section 19; fp64 restatement: tests/rhf_ref.py.
//
//   mu[c,p] = (1/S) sum_s P[s,c,p],  v[c,p] = (1/S^2) sum_s (P[s,c,p] - mu[c,p])^2
//   delta(p,q) = (1/C) sum_c (mu[c,p] - mu[c,q])^2 / (eps + v[c,p] + v[c,q])
//   D(p,q) = mean over |oy|,|ox| <= f, with p + o and q + o inside the image, of delta(p + o, q + o)
//   w(p,q) = exp(-D(p,q) / b^2) for q = p + (dy,dx) inside the image (and mask[q] != 0), |dy|,|dx| <= R
//   wsum[p] = sum_q w(p,q),  out[p,:] = sum_q w(p,q) image[q,:] / wsum[p]       (q in tap order, dy major)
//
// Two launches.  The statistics pass reads the P-buffer once and writes {mu, v} pairs, [C][H][W] float2, to the workspace.  The
// filter kernel gives a 256-thread block 32 x 8 output pixels.  The pairs of the tile and its (R + f) halo sit in LDS ([C][rows][cols]
// float2: consecutive lanes read consecutive 8-byte words) beside one byte per position that says "outside the image", "inside and
// masked" or "inside".  The block then walks the (2R + 1)^2 window offsets.  For one offset d, delta(p', p' + d) is needed at the
// (32 + 2f) x (8 + 2f) positions p' of the tile and its f halo, and each is shared by up to (2f + 1)^2 patch sums: the threads compute
// these deltas ONCE (one or two positions per thread at f = 1; a pair with an end outside the image is written as -1, delta itself is
// never negative), hand them over through a double-buffered LDS tile behind ONE barrier per offset, and every thread box-sums the
// (2f + 1)^2 neighbours of its own pixel, counting the ones that exist.  Per window pair that is C hardware reciprocals * 1.33
// instead of * 9, and (2f + 1)^2 + 1.33 * C LDS reads.  The thread's own statistics stay in registers where C is a compile-time
// constant.  Image taps are plain global loads (a wave reads one row segment; they hit the L1).  No atomics, fixed order: the result
// is bitwise reproducible.  A tile whose whole halo lies inside an unmasked image walks without the flags (same operations, same
// order, same bits; a fifth faster).  A P-buffer too wide for LDS (C * positions * 8 bytes above PF_LDS_MAX) takes the same kernel with the
// pairs read from the workspace through the caches.
#include <math.h>

#include <type_traits>

#include "common.h"

namespace wcmc {

constexpr int PF_TW = 32, PF_TH = 8;          // output pixels per block, one per thread
constexpr int PF_MAXR = 10, PF_MAXF = 3, PF_MAXC = 32, PF_MAXCR = 4;
constexpr int PF_MAXNP = 3;                   // delta positions per thread: (32 + 6) * (8 + 6) = 532 <= 3 * 256
constexpr size_t PF_LDS_MAX = 128 << 10;      // of the CU's 160 KiB
static_assert((PF_TW + 2 * PF_MAXF) * (PF_TH + 2 * PF_MAXF) <= PF_MAXNP * PF_TW * PF_TH, "every delta position has a thread");

struct PFParams {
  const float* img; int64_t ish, isw, isc;
  const float* pb; int64_t pss, psc, psh, psw;
  const void* mask; int mask_bytes;           // (H, W) contiguous; 1: uint8 / bool, 4: fp32; null: every pixel counts
  float* out; float* wsum;                    // (H, W, Cr) and (H, W), contiguous
  float2* stats;                              // workspace: [C][H][W] {mu, v}
  int H, W, S, C, Cr, R, f;
  float eps, kexp, inv_c;                     // kexp = -log2(e) / b^2
};

__global__ __launch_bounds__(256) void pbuffer_stats_kernel(PFParams p) {
  const int64_t plane = (int64_t)p.H * p.W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= plane * p.C) return;
  const int c = (int)(idx / plane);
  const int pix = (int)(idx - (int64_t)c * plane);
  const int y = pix / p.W, x = pix - y * p.W;
  const float* src = p.pb + (int64_t)c * p.psc + (int64_t)y * p.psh + (int64_t)x * p.psw;
  float s = 0.f;
  for (int k = 0; k < p.S; ++k) s += src[(int64_t)k * p.pss];
  const float mu = s / (float)p.S;
  float q = 0.f;
  for (int k = 0; k < p.S; ++k) {              // (the second read of the S values comes from the caches)
    const float d = src[(int64_t)k * p.pss] - mu;
    q += d * d;
  }
  p.stats[idx] = make_float2(mu, q / ((float)p.S * (float)p.S));
}

// RT, FT >= 0: compile-time radii; CT > 0: compile-time channel count (the thread's own statistics stay in registers);
// LDS: the pairs of the halo are LDS-resident, else read from the workspace.
template <int RT, int FT, int CT, bool LDS>
__global__ __launch_bounds__(256) void pbuffer_filter_kernel(PFParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int R = RT >= 0 ? RT : p.R, f = FT >= 0 ? FT : p.f, C = CT > 0 ? CT : p.C;
  const int HF = R + f;
  const int HS = PF_TW + 2 * HF, NPOS = (PF_TH + 2 * HF) * HS;       // the halo: row stride, positions
  const int DW = PF_TW + 2 * f, ND = DW * (PF_TH + 2 * f);           // the delta tile
  constexpr int NP = FT >= 0 ? ((PF_TW + 2 * FT) * (PF_TH + 2 * FT) + 255) / 256 : PF_MAXNP;
  constexpr int CR = CT > 0 ? CT : 1;
  float2* const st = reinterpret_cast<float2*>(smem);                 // [C][NPOS] (LDS only)
  float* const delta = smem + (LDS ? 2 * C * NPOS : 0);               // [2][ND]
  unsigned char* const flags = reinterpret_cast<unsigned char*>(delta + 2 * ND);        // [NPOS]: 0 outside, 1 masked, 2 inside

  const int tiles_x = (p.W + PF_TW - 1) / PF_TW;
  const int y0 = (blockIdx.x / tiles_x) * PF_TH, x0 = (blockIdx.x % tiles_x) * PF_TW;
  const int tid = threadIdx.x, tx = tid & (PF_TW - 1), ty = tid / PF_TW;
  const int64_t plane = (int64_t)p.H * p.W;

  for (int i = tid; i < NPOS; i += 256) {
    const int hy = i / HS, hx = i - hy * HS;
    const int y = y0 - HF + hy, x = x0 - HF + hx;
    const bool in = (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
    unsigned char fl = in ? 2 : 0;
    if (in && p.mask) {
      const int64_t mi = (int64_t)y * p.W + x;
      const bool m = p.mask_bytes == 4 ? static_cast<const float*>(p.mask)[mi] != 0.f
                                       : static_cast<const unsigned char*>(p.mask)[mi] != 0;
      fl = m ? 2 : 1;
    }
    flags[i] = fl;
    if (LDS)
      for (int c = 0; c < C; ++c)
        st[c * NPOS + i] = in ? p.stats[c * plane + (int64_t)y * p.W + x] : make_float2(0.f, 0.f);
  }
  __syncthreads();

  // {mu, v} of channel c at halo position i, which lies inside the image (its coordinates: (gy, gx))
  auto stat = [&](int c, int i, int gy, int gx) -> float2 {
    if (LDS) return st[c * NPOS + i];
    return p.stats[c * plane + (int64_t)gy * p.W + gx];
  };

  // this thread's delta positions p': halo index and frame coordinates of p' - (R, R), the corner its q' start from
  int dbase[NP], dgy[NP], dgx[NP];
  bool pin[NP];
  float pmu[NP][CR], pev[NP][CR];                                     // CT > 0: mu and eps + v of p'
#pragma unroll
  for (int n = 0; n < NP; ++n) {
    const int i = tid + 256 * n;
    const int iy = i / DW, ix = i - iy * DW;
    dbase[n] = i < ND ? iy * HS + ix : -1;
    dgy[n] = y0 - f + iy - R; dgx[n] = x0 - f + ix - R;
    pin[n] = i < ND && flags[dbase[n] + R * HS + R] != 0;
#pragma unroll
    for (int c = 0; c < CR; ++c) {
      pmu[n][c] = 0.f; pev[n][c] = 0.f;
      if (CT > 0 && pin[n]) {
        const float2 a = stat(c, dbase[n] + R * HS + R, dgy[n] + R, dgx[n] + R);
        pmu[n][c] = a.x; pev[n][c] = p.eps + a.y;
      }
    }
  }

  const int y = y0 + ty, x = x0 + tx;
  const bool p_in = y < p.H && x < p.W;
  const bool p_ok = flags[(ty + HF) * HS + tx + HF] == 2;
  const int qbase = (ty + f) * HS + tx + f;                           // halo index of q at the window's corner
  const int side = 2 * R + 1, box = 2 * f + 1;
  float acc[PF_MAXCR] = {0.f, 0.f, 0.f, 0.f}, ws = 0.f;
  int buf = 0;

  // A tile whose whole halo lies inside an unmasked image needs no flag: every pair exists, every patch holds box^2 deltas.  INSIDE
  // is that case at compile time; it computes the same operations in the same order on the same values as the flagged walk
  // (cnt is box^2 there too), so a pixel's bits do not depend on which walk its tile took.
  const bool inside = !p.mask && y0 >= HF && x0 >= HF && y0 + PF_TH + HF <= p.H && x0 + PF_TW + HF <= p.W;      // block-uniform
  const float rbox = __builtin_amdgcn_rcpf((float)(box * box));
  auto walk = [&](auto inside_tag) {
    constexpr bool INSIDE = decltype(inside_tag)::value;
#pragma unroll 1
    for (int dyi = 0; dyi < side; ++dyi) {
#pragma unroll 1
      for (int dxi = 0; dxi < side; ++dxi) {
        float* const dl = delta + buf * ND;
        buf ^= 1;
        const int off = dyi * HS + dxi;
#pragma unroll
        for (int n = 0; n < NP; ++n) {
          if (dbase[n] < 0) continue;
          float d = -1.f;                                             // a pair with an end outside the image
          const int qi = dbase[n] + off;
          if (INSIDE || (pin[n] && flags[qi] != 0)) {
            float s = 0.f;
            if (CT > 0) {
#pragma unroll
              for (int c = 0; c < CR; ++c) {
                const float2 b = stat(c, qi, dgy[n] + dyi, dgx[n] + dxi);
                const float df = pmu[n][c] - b.x;
                s += (df * df) * __builtin_amdgcn_rcpf(pev[n][c] + b.y);
              }
            } else {
              for (int c = 0; c < C; ++c) {
                const float2 a = stat(c, dbase[n] + R * HS + R, dgy[n] + R, dgx[n] + R);
                const float2 b = stat(c, qi, dgy[n] + dyi, dgx[n] + dxi);
                const float df = a.x - b.x;
                s += (df * df) * __builtin_amdgcn_rcpf((p.eps + a.y) + b.y);
              }
            }
            d = s * p.inv_c;
          }
          dl[tid + 256 * n] = d;
        }
        // One barrier per offset: the deltas written above are read below, and the buffer written two offsets later is this one --
        // behind the next offset's barrier, which no thread passes before every thread has left this offset's reads.
        __syncthreads();
        if (INSIDE || (p_ok && flags[qbase + off] == 2)) {
          float sum = 0.f, cnt = 0.f;
          const float* const dp = dl + ty * DW + tx;
          auto take = [&](int oy, int ox) {
            const float d = dp[oy * DW + ox];
            if (INSIDE) sum += d;
            else if (!(d < 0.f)) { sum += d; cnt += 1.f; }            // (a NaN delta counts: it poisons the pixels that read it)
          };
          if (FT >= 0) {
            constexpr int BOX = FT >= 0 ? 2 * FT + 1 : 1;
#pragma unroll
            for (int oy = 0; oy < BOX; ++oy)
#pragma unroll
              for (int ox = 0; ox < BOX; ++ox) take(oy, ox);
          } else {
            for (int oy = 0; oy < box; ++oy)
              for (int ox = 0; ox < box; ++ox) take(oy, ox);
          }
          const float w = __builtin_amdgcn_exp2f(sum * (INSIDE ? rbox : __builtin_amdgcn_rcpf(cnt)) * p.kexp);
          ws += w;
          const float* ip = p.img + (int64_t)(y + dyi - R) * p.ish + (int64_t)(x + dxi - R) * p.isw;
#pragma unroll
          for (int c = 0; c < PF_MAXCR; ++c)
            if (c < p.Cr) acc[c] = fmaf(w, ip[(int64_t)c * p.isc], acc[c]);
        }
      }
    }
  };
  if (inside) walk(std::true_type{});
  else walk(std::false_type{});

  if (!p_in) return;
  const int64_t pix = (int64_t)y * p.W + x;
  const float* ip = p.img + (int64_t)y * p.ish + (int64_t)x * p.isw;
  p.wsum[pix] = p_ok ? ws : 0.f;
#pragma unroll
  for (int c = 0; c < PF_MAXCR; ++c)
    if (c < p.Cr) p.out[pix * p.Cr + c] = p_ok ? acc[c] / ws : ip[(int64_t)c * p.isc];
}

static size_t pf_lds_bytes(int C, int R, int f, bool lds) {
  const size_t npos = (size_t)(PF_TH + 2 * (R + f)) * (PF_TW + 2 * (R + f));
  const size_t nd = (size_t)(PF_TW + 2 * f) * (PF_TH + 2 * f);
  return (lds ? (size_t)C * npos * sizeof(float2) : 0) + 2 * nd * sizeof(float) + (npos + 15) / 16 * 16;
}

template <int RT, int FT, int CT, bool LDS>
static int pf_launch(const PFParams& p, size_t lds, hipStream_t st) {
  static LdsAttr attr;
  const void* fn = reinterpret_cast<const void*>(&pbuffer_filter_kernel<RT, FT, CT, LDS>);
  if (lds > (48u << 10) && set_max_lds(fn, lds, attr) != hipSuccess) return WCMC_ERR_LAUNCH;
  const unsigned tiles = (unsigned)(((p.H + PF_TH - 1) / PF_TH) * ((p.W + PF_TW - 1) / PF_TW));
  hipLaunchKernelGGL((pbuffer_filter_kernel<RT, FT, CT, LDS>), dim3(tiles), dim3(256), lds, st, p);
  return check_launch("pbuffer_filter");
}

}  // namespace wcmc

using namespace wcmc;

extern "C" size_t wcmc_pbuffer_filter_workspace_bytes(int S, int C, int H, int W) {
  if (S < 1 || C < 1 || C > PF_MAXC || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 30)) return 0;
  return (size_t)C * H * W * sizeof(float2);
}

extern "C" int wcmc_pbuffer_filter(const float* image, int64_t ish, int64_t isw, int64_t isc, const float* p_buffer, int64_t pss,
                                   int64_t psc, int64_t psh, int64_t psw, const void* mask, int mask_bytes, float* out,
                                   float* wsum, void* workspace, size_t workspace_bytes, int H, int W, int S, int C, int Cr,
                                   int R, int f, float bandwidth, float eps, int passes, void* stream) {
  WCMC_REQUIRE(R >= 0 && R <= PF_MAXR && f >= 0 && f <= PF_MAXF, WCMC_ERR_BAD_ARG,
               "pbuffer_filter: radius %d, patch_radius %d (0..%d and 0..%d are supported)", R, f, PF_MAXR, PF_MAXF);
  WCMC_REQUIRE(C >= 1 && C <= PF_MAXC && Cr >= 1 && Cr <= PF_MAXCR, WCMC_ERR_BAD_ARG,
               "pbuffer_filter: C = %d embedding channels, Cr = %d image channels (1..%d and 1..%d are supported)", C, Cr, PF_MAXC,
               PF_MAXCR);
  WCMC_REQUIRE(S >= 1, WCMC_ERR_BAD_ARG, "pbuffer_filter: S = %d samples (at least 1)", S);
  WCMC_REQUIRE(bandwidth > 0.f && eps > 0.f, WCMC_ERR_BAD_ARG, "pbuffer_filter: bandwidth %g and eps %g must be positive",
               (double)bandwidth, (double)eps);
  WCMC_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30), WCMC_ERR_BAD_ARG, "pbuffer_filter: unsupported shape (H=%d W=%d)",
               H, W);
  WCMC_REQUIRE(passes >= 1 && passes <= 3, WCMC_ERR_BAD_ARG, "pbuffer_filter: passes = %d (1: statistics, 2: filter, 3: both)", passes);
  WCMC_REQUIRE(image && p_buffer && out && wsum && workspace, WCMC_ERR_BAD_ARG, "pbuffer_filter: null pointer");
  WCMC_REQUIRE(!mask || mask_bytes == 1 || mask_bytes == 4, WCMC_ERR_BAD_ARG,
               "pbuffer_filter: mask elements of %d bytes (1: uint8 / bool, 4: fp32)", mask_bytes);
  const size_t need = wcmc_pbuffer_filter_workspace_bytes(S, C, H, W);
  WCMC_REQUIRE(workspace_bytes >= need, WCMC_ERR_WORKSPACE, "pbuffer_filter: workspace of %zu bytes, %zu needed", workspace_bytes,
               need);
  PFParams p = {};
  p.img = image; p.ish = ish; p.isw = isw; p.isc = isc;
  p.pb = p_buffer; p.pss = pss; p.psc = psc; p.psh = psh; p.psw = psw;
  p.mask = mask; p.mask_bytes = mask_bytes; p.out = out; p.wsum = wsum; p.stats = static_cast<float2*>(workspace);
  p.H = H; p.W = W; p.S = S; p.C = C; p.Cr = Cr; p.R = R; p.f = f;
  p.eps = eps; p.inv_c = 1.f / (float)C;
  p.kexp = (float)(-1.4426950408889634 / ((double)bandwidth * (double)bandwidth));
  hipStream_t st = (hipStream_t)stream;
  if (passes & 1) {
    const int64_t total = (int64_t)C * H * W;
    hipLaunchKernelGGL(pbuffer_stats_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p);
    if (int rc = check_launch("pbuffer_filter(statistics)")) return rc;
  }
  if (!(passes & 2)) return 0;
  // THE launch plan: the default window with three embedding channels; else the runtime instance, LDS-resident while it fits
  const bool lds = pf_lds_bytes(C, R, f, true) <= PF_LDS_MAX;
  const size_t bytes = pf_lds_bytes(C, R, f, lds);
  if (R == 10 && f == 1 && C == 3) return pf_launch<10, 1, 3, true>(p, bytes, st);
  if (lds) return pf_launch<-1, -1, 0, true>(p, bytes, st);
  return pf_launch<-1, -1, 0, false>(p, bytes, st);
}
