// What the split-bf16 ("bf16x3") convolution units share: conv_bf16x3.hip (its header comment describes the operand split and the
// tensor / weight layouts; it holds the glue kernels, the plans and every C entry) and one unit per GEMM kernel family --
// bf16x3_igemm.hip, bf16x3_halo.hip, bf16x3_halo64.hip, bf16x3_halo3.hip, bf16x3_pw.hip, bf16x3_wgrad.hip.  Every kernel template is
// instantiated in exactly ONE unit: a family is launched through its launch entry declared at the end of this
// header, never by naming its kernel from another unit.
#pragma once
#include "common.h"

namespace wcmc {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u16 f2bf(float x) { return __builtin_bit_cast(u16, (__bf16)x); }
__device__ __forceinline__ float bf2f(u16 h) { return __builtin_bit_cast(float, (unsigned)h << 16); }
__device__ __forceinline__ void split1(float x, u16& hi, u16& lo) {
  hi = f2bf(x);
  lo = f2bf(x - bf2f(hi));
}

typedef _Float16 xf16x8 __attribute__((ext_vector_type(8)));

constexpr int XBM = 128;   // pixels per block
constexpr int XKC = 32;    // k per LDS stage = one MFMA k-step
constexpr int XROW = 32;   // bf16 per LDS row
constexpr unsigned XOOB = 0x80000000u;   // byte offset beyond any buffer (num_records < 2 GiB)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// bit e = (bf16 number e of the vector is > 0): the activation-derivative predicate of act_gate on a hi plane.
// A bf16 is positive iff it is positive as an int16; per dword (two of them): max(., 0) of both halves in one packed instruction,
// "half != 0" as bit 15 of half + 0x7fff (no carry between the halves: a clamped half is at most 0x7fff) -- four vector
// instructions per pair where the test half by half took ten (the gate masks cost 3 of a U-Net layer's 37 us, profiles/r06_unet_halo3.txt).
typedef short xs16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned positive_pair(unsigned w) {          // bit 0: low half > 0, bit 16: high half > 0
  const xs16x2 z = {0, 0};
  const xs16x2 c = __builtin_elementwise_max(__builtin_bit_cast(xs16x2, w), z);
  return ((__builtin_bit_cast(unsigned, c) + 0x7fff7fffu) >> 15) & 0x00010001u;
}
__device__ __forceinline__ unsigned char positive_mask8(const u32x4 v) {
  // pairs e = 0..3 -> bits 2e (low half) and 2e + 1 (high half)
  const unsigned x = positive_pair(v[0]) | (positive_pair(v[1]) << 2) | (positive_pair(v[2]) << 4) | (positive_pair(v[3]) << 6);
  return (unsigned char)((x | (x >> 15)) & 0xffu);
}

// Epilogue of one accumulator quad (4 consecutive couts of one pixel): bias, activation, pixel validity, gate, split --
// as packed conversions and selects.  Couts past Cout need no test: their packed weights and their bias (out-of-range
// buffer load) are zeros, and every activation maps 0 to +0.
typedef __bf16 xbf16x2 __attribute__((ext_vector_type(2)));
typedef float xf32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void x_split2(float a, float b, unsigned& hi2, unsigned& lo2) {
  const xf32x2 v = {a, b};
  hi2 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, xbf16x2));
  const xf32x2 back = {__builtin_bit_cast(float, hi2 << 16), __builtin_bit_cast(float, hi2 & 0xffff0000u)};
  lo2 = __builtin_bit_cast(unsigned, __builtin_convertvector(v - back, xbf16x2));
}
// activation as selects (bit-identical to act_apply, no branches inside an unrolled epilogue)
struct XAct { float ns; bool zero; };
__device__ __forceinline__ XAct x_act(int act, float slope) {
  return XAct{act == WCMC_ACT_LEAKY_RELU ? slope : 1.f, act == WCMC_ACT_RELU};
}
__device__ __forceinline__ float x_act_apply(float v, XAct a) { return v > 0.f ? v : (a.zero ? 0.f : v * a.ns); }

// gate kinds of x_epi_quad: 0 none, 1 split gate tensor (hi plane of 4 values in g2), 2 bit mask (byte in g2.x)
__device__ __forceinline__ void x_epi_quad(const f32x4 a4, const float (&b)[4], bool ok, XAct ak, int gkind, u32x2 g2, int co,
                                           float gate_off, float (&v)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = a4[e] + b[e];
    const float neg = ak.zero ? 0.f : t * ak.ns;
    const float r = t > 0.f ? t : neg;
    v[e] = ok ? r : 0.f;
  }
  if (gkind == 1) {
    const unsigned g[4] = {g2.x << 16, g2.x & 0xffff0000u, g2.y << 16, g2.y & 0xffff0000u};
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __builtin_bit_cast(float, g[e]) > 0.f ? v[e] : v[e] * gate_off;
  } else if (gkind == 2) {
    const unsigned bits = g2.x >> (co & 7);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((bits >> e) & 1u) ? v[e] : v[e] * gate_off;
  }
}

struct XIgemmParams {
  const u16* x; int N, H, W, Cin, Cpi;
  const u16* wp; const float* bias;
  float* yf; int64_t ysn, ysh, ysw;       // fp32 NHWC view output (or null)
  u16* ys; int Cpo;                       // split dense output (or null)
  int Ho, Wo, Cout;
  const u16* gate; int gate_act; float gate_slope;   // split dense, geometry of y
  const unsigned char* gate_mask;         // alternative to gate: 1 bit per element, [pixel][Cpo/8] (what mask_out wrote)
  unsigned char* mask_out;                // optional with ys: bit = (hi plane of the result > 0), [pixel][Cpo/8]
  int ks, pad, act; float slope;
  int Kp, Kt, Np;
  int64_t M;
  unsigned x_bytes, wp_bytes;
  float* colsum;                          // optional [G][Np] per-tile column sums of the split output
  int G;                                  // rows of colsum (tiles past the kernel's own are zero-filled)
  int CS, nslabs, SPS, PXS, tilesX, tilesY;   // halo kernel: channel slab, stages per slab, halo pixel stride
  int CSl, SPSl;                              // ... of the last slab
  int rows16;                                 // conv_halo64, PT = 4 instance: tile rows [0, rows16) are 16 pixels high, the rest 12 (launch_xhalo64; set there)
  int stripX, stripY;                         // ... and a strip of stripX TRANSPOSED tile columns of 12 pixels (16 rows high, stripY of them) right of the tilesX columns of 16
  int ap;                                     // planes of x multiplied: 2 = hi + lo, 1 = hi only (two MFMAs per product)
  int wplanes;                                // planes of the weights multiplied: 2, or 1 with ap == 1 (ONE MFMA per product; conv_halo64 only)
  int f16;                                    // with ap == wplanes == 1: x is ONE fp16 plane [pixel][Cpi], the pack's hi rows are fp16
  unsigned y_bytes, m_bytes;                  // pointwise kernel: extents of the output and of the 1-bit masks
  // pointwise kernel, optional tail layer (a second 1x1 conv of <= 4 couts applied to the tile while it is in LDS)
  const u16* wp2; const float* bias2; float* y2; int64_t y2sn, y2sh, y2sw;
  int Cout2, act2, Kt2; float slope2; unsigned wp2_bytes, y2_bytes;
};

// Parameter blocks of the weight-gradient kernels (bf16x3_wgrad.hip; wcmc_conv2d_wgrad_bf16x3 fills them): one tap per block ...
struct XWgradParams {
  const u16* x; int N, H, W, Cin, Cpi;
  const u16* dy; int Ho, Wo, Cout, Cpo;
  int ks, pad;
  float* slabs; int S; int64_t M, pix_per_split;
  int Np, Cq, coBlocks, ciBlocks;
  unsigned x_bytes, dy_bytes;
  int xps, yps;                     // pixel stride (bytes) of x / dy: 4 * Cp for a split tensor, 2 * Cp for a single bf16 plane
};
// ... and one filter row per block
struct XWRowsParams {
  const u16* x; int N, H, W, Cpi;
  const u16* dy; int Ho, Wo, Cpo;
  int pad;
  float* slabs; int S, rps, R;
  float* dbg;                       // clock-probe build only
  int prio;                         // rows8: iteration (of 14 per stage) at which waves 0-3 hand the priority to waves 4-7; 0 = off
  int Np, Cq, coBlocks, ciBlocks;
  unsigned x_bytes, dy_bytes;
  int xps, yps;                     // pixel stride (bytes) of x / dy: 4 * Cp for a split tensor, 2 * Cp for a single bf16 plane
};
// LDS row stride (u16) of a CH-channel tile: bytes = odd multiple of 32 (conflict-free transposing reads);
// the pad vectors of a row are filled by DMA lanes with an out-of-range source (zeros).
constexpr int xwr_stride(int ch) { return ((ch / 16) | 1) * 16; }
// dynamic LDS of the filter-row instance <ks, tm, nw, pl> (as xwr_lds_bytes of bf16x3_wgrad.hip): x_plan_wgrad sizes its splits by it
static size_t xwr_lds_bytes_rt(int ks, int tm, int nw, int pl = 2) {
  const int nvec = pl * 64 * (xwr_stride(tm * 16) / 8) + pl * (64 + ks - 1) * (xwr_stride(nw * 16) / 8);
  const int ni = (nvec + nw * 64 - 1) / (nw * 64);
  const size_t stage = (size_t)2 * ni * nw * 64 * 16, red = (size_t)tm * 16 * (nw * 16 + 4) * sizeof(float);
  return stage > red ? stage : red;
}

// Workgroup barrier for kernels that keep LDS-DMA in flight across it: __syncthreads() carries a release fence,
// for which hipcc waits for EVERY outstanding LDS-DMA (vmcnt(0)); the rings of those kernels order their DMA by explicit counts.
__device__ __forceinline__ void pw_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

int x_env_on(const char* name);           // conv_bf16x3.hip: switch is ON unless the variable starts with '0' (debug build only: ab_env)

// ------------------------------------------------------------------ launch plans and launch entries, one pair per family (its own unit defines it)
// A plan function decides WHICH kernel instance a launch runs and its geometry: host arithmetic on the parameters (and, in the debug
// build, the A/B switches, read per call) -- no HIP runtime call, so the launch-plan queries (wcmc_conv2d_launch_plan_bf16x3,
// wcmc_conv2d_wgrad_launch_plan_bf16x3) ask the same code without a device.  A launcher runs the instance its plan names, or fails.
// The fields that are template arguments are spelled as the kernel's: a kernel name is printed from them.
// nt = x_pick_nt(p.Np / 16): cout tiles per block, one of {7, 4, 2, 1}
struct XIgemmPlan { int nt, padded, dbuf; };                                    // conv_igemm_bf16x3_kernel<nt, padded, dbuf, 0>
struct XHaloPlan { int nt, th, nb, ap, tilesY; size_t lds; };                   // conv_halo_bf16x3_kernel<nt, th, 16, 0, nb, ap>
struct XHalo64Plan { int nt, nb, pt, pxst, ap, wp, f16;                         // conv_halo64_bf16x3_kernel<nt, nb, pt, 0, pxst, ap, wp, f16>
                     int tilesX, tilesY, rows16, stripX, stripY; size_t lds; }; // ... and what the launch writes into its copy of the parameters
struct XHalo3Plan { int ap, spt; };                                             // conv_halo3_bf16x3_kernel<ap, spt, 2, 0>
struct XPwPlan { int ntw, u; };                                                 // conv_pw_bf16x3_kernel<ntw, u, split output, 0>
struct XWRowsPlan { int ks, tm, nw, pl, rows8, xe; };                           // conv_wgrad_rows_bf16x3_kernel<ks, tm, nw, 0, pl> | rows8: conv_wgrad_rows8_bf16x3_kernel<0, xe, pl>
// bf16x3_igemm.hip: plans without a halo (p.PXS == 0)
XIgemmPlan x_plan_igemm(int nt, const XIgemmParams& p);
int launch_xigemm(const XIgemmPlan& g, const XIgemmParams& p, hipStream_t stream);
// bf16x3_halo.hip: halo plans (p.PXS != 0) but those of the 64-pixel 5x5 kernel (x_halo_is64); x_plan_halo fails where the tile does not fit in LDS
bool x_halo_is64(const XIgemmParams& p);
int x_plan_halo(int nt, const XIgemmParams& p, XHaloPlan* h);
int launch_xhalo(const XHaloPlan& h, const XIgemmParams& p, hipStream_t stream);
// bf16x3_halo64.hip
XHalo64Plan x_plan_halo64(int nt, const XIgemmParams& p);
int launch_xhalo64(const XHalo64Plan& h, const XIgemmParams& p, hipStream_t stream);
// bf16x3_halo3.hip: the 3x3 plans of conv_halo3_bf16x3_kernel
bool x_halo3_ok(const XIgemmParams& p);
XHalo3Plan x_plan_halo3(const XIgemmParams& p);
int launch_xhalo3(const XHalo3Plan& h, const XIgemmParams& p, hipStream_t stream);
// bf16x3_pw.hip: x_plan_pw picks the pointwise instance (ntw waves, u 16-byte units per pixel) or says no; launch_xpw sets p.y_bytes / p.m_bytes
bool x_plan_pw(const XIgemmParams& p, XPwPlan* w);
int launch_xpw(XIgemmParams& p, const XPwPlan& w, hipStream_t stream);
int launch_xpw_pair(int kind, const XIgemmParams& p, hipStream_t stream);      // kind = x_pair_kind(...): 1..3, the fused two-layer instances
// bf16x3_wgrad.hip; planes: 2 = three MFMAs per product, 1 = the hi planes only
int launch_xwgrad(int tm, int planes, const XWgradParams& p, hipStream_t stream);                            // tm = XWgradPlan::TM: 7 or 4
XWRowsPlan x_plan_wgrad_rows(int ks, int tm, int nw, int planes);                                            // (tm, nw) = XWgradPlan::rTM, rNW
int launch_xwgrad_rows(const XWRowsPlan& r, const XWRowsParams& p, hipStream_t stream);

}  // namespace wcmc
