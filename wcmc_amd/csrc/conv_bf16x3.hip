// Split-bf16 ("bf16x3") convolution forward / data-gradient / weight-gradient for gfx950.
//
// Same GEMM views as conv.hip, but every fp32 operand x is carried as two bf16 planes
//   hi = bf16(x), lo = bf16(x - hi)          (x = hi + lo to ~2^-17 relative)
// and a product is evaluated as hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation (the dropped lo*lo term is ~2^-18 relative).  bf16 x bf16 products are exact in
// fp32, so the only roundings are the operand split and the fp32 accumulate: 3 MFMAs at 16x the fp32
// MFMA rate = 5.3x the fp32-MFMA throughput at close to fp32 accuracy (measured in
// tests/test_gpu_ops.py).  Replaces the same reference expressions as conv.hip (torch.nn.Conv2d
// inside sbmc.modules.ConvChain; cuDNN with TF32 on the reference's hardware).
//
// Split tensor layout (chain-internal, dense): u16 [N][H][W][2][Cp], Cp = round_up(C, 8);
// plane 0 = hi, plane 1 = lo; pad channels are ZERO (producers guarantee it), so loaders need no
// channel masks.  Packed weights: u16 wp[Np][2][Kt], k = tap*Kp + c, Kp = round_up(kchan, 8),
// Kt = round_up(taps*Kp, 32), Np = round_up(rows, 16).
//
// This unit holds what is not a GEMM kernel family: the split / cat / pack glue kernels, the plans and every C entry.  Each
// family (igemm, halo, halo64, halo3, pw, wgrad) has its own bf16x3_<family>.hip and is reached through its launch entries
// in bf16x3_common.h.
#include <stdlib.h>

#include "bf16x3_common.h"
#include "conv_common.h"

namespace wcmc {

// ------------------------------------------------------------------ fp32 NHWC view -> split
// Optional gate (post != nullptr): out = split(x * act'(post)), the output-activation backward of a chain
// (wcmc_act_backward) folded into the split of its upstream gradient -- one pass over dy instead of two.
__global__ void split_kernel(const float* __restrict__ x, int64_t xsn, int64_t xsh, int64_t xsw,
                             u16* __restrict__ out, int H, int W, int C, int Cp, int64_t total,
                             const float* __restrict__ post = nullptr, int64_t psn = 0, int64_t psh = 0, int64_t psw = 0,
                             int act = 0, float slope = 0.f) {
  const int V = Cp / 8;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const NhwvIndex ix_ = decode_nhwv(idx, total, H, W, V);
    const int v = ix_.v, xx = ix_.x, y = ix_.y, n = ix_.n;
    const float* src = x + n * xsn + y * xsh + xx * xsw + v * 8;
    float f[8];
    const int c0 = v * 8;
    if (c0 + 8 <= C) {
      const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = (c0 + e < C) ? src[e] : 0.f;
    }
    if (post) {
      const float* ps = post + n * psn + y * psh + xx * psw + c0;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c0 + e < C) f[e] *= act_gate(ps[e], act, slope);
    }
    u16 hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) split1(f[e], hi[e], lo[e]);
    u16* o = out + (((int64_t)n * H + y) * W + xx) * 2 * Cp + c0;
    *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(hi);
    *reinterpret_cast<uint4*>(o + Cp) = *reinterpret_cast<const uint4*>(lo);
  }
}

// ------------------------------------------------------------------ split -> one fp16 plane
// x = hi + lo of a split tensor, rounded once to fp16 (11 bits; saturating at +-65504): the A operand of the one-MFMA fp16 forward
// of an un-gated output layer ("bf16x321h" mode).  [N*H*W][Cp] halfs, Cp = round_up(C, 8).
__device__ __forceinline__ u16 f2h_sat(float v) {
  v = v > 65504.f ? 65504.f : (v < -65504.f ? -65504.f : v);
  return __builtin_bit_cast(u16, (_Float16)v);
}
__global__ __launch_bounds__(256) void split_to_f16_kernel(const u16* __restrict__ xs, u16* __restrict__ out, int Cp, int64_t total) {
  const int V = Cp / 8;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int v = (int)(idx % V); const int64_t px = idx / V;
    const uint4 h = *reinterpret_cast<const uint4*>(xs + px * 2 * Cp + v * 8), l = *reinterpret_cast<const uint4*>(xs + px * 2 * Cp + Cp + v * 8);
    const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
    u16 o[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = __builtin_bit_cast(float, hw[e] << 16) + __builtin_bit_cast(float, lw[e] << 16);
      const float b = __builtin_bit_cast(float, hw[e] & 0xffff0000u) + __builtin_bit_cast(float, lw[e] & 0xffff0000u);
      o[2 * e] = f2h_sat(a); o[2 * e + 1] = f2h_sat(b);
    }
    *reinterpret_cast<uint4*>(out + px * Cp + v * 8) = *reinterpret_cast<const uint4*>(o);
  }
}

// ------------------------------------------------------------------ strided (N,C,H,W) -> split
// The per-sample path descriptors arrive channel-first (`paths` (B,S,36,H,W), support/networks.py:31-33) and are only
// ever read as the embedding chain's split input: transpose and split in one pass (64 pixels of one image row x all
// channels through LDS) instead of a channel-last fp32 copy that is then split (0.3 GB less traffic per step).
__global__ __launch_bounds__(256) void nchw_split_kernel(const float* __restrict__ src, int64_t ssn, int64_t ssc, int64_t ssh,
                                                         int64_t ssw, u16* __restrict__ out, int C, int Cp, int H, int W) {
  __shared__ float tile[64][65];                    // [channel][pixel]
  const int xt = blockIdx.x * 64, y = blockIdx.y % H, n = blockIdx.y / H;
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  for (int c = grp; c < Cp; c += 4) {
    const int x = xt + lane;
    tile[c][lane] = (c < C && x < W) ? src[(int64_t)n * ssn + (int64_t)c * ssc + (int64_t)y * ssh + (int64_t)x * ssw] : 0.f;
  }
  __syncthreads();
  const int V = Cp / 8;
  for (int i = threadIdx.x; i < 64 * V; i += 256) {
    const int px = i / V, v = i - px * V, x = xt + px;
    if (x >= W) continue;
    u16 hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) split1(tile[v * 8 + e][px], hi[e], lo[e]);
    u16* o = out + (((int64_t)n * H + y) * W + x) * 2 * Cp + v * 8;
    *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(hi);
    *reinterpret_cast<uint4*>(o + Cp) = *reinterpret_cast<const uint4*>(lo);
  }
}

// ------------------------------------------------------------------ cat([flat, repeat_S(prop)], 1) -> split
// support/networks.py:39-40 feeding the `final` ConvChain: the 128-channel concatenation of the per-sample
// embedding (B*S images) and the spp-broadcast U-Net output (B images) is written once, directly as the
// chain's split-bf16 input (separately: copy 268 MB + broadcast 268 MB into an fp32 tensor, then read its
// 537 MB and write 537 MB of split planes).  One thread = 8 channels of one pixel.
// up != 0 (U-Net skip concatenation, Autoencoder of sbmc.modules): `flat` is the level below at (H/2, W/2) and is
// upsampled on the fly -- bilinear x2, align_corners=False, the same four taps and the same fma chain as
// upsample2_fwd_kernel (elementwise.hip), so the result equals upsample + concatenation bit for bit.
__global__ void cat_broadcast_split_kernel(const float* __restrict__ flat, int64_t fsn, int64_t fsh, int64_t fsw,
                                           const float* __restrict__ prop, int64_t psn, int64_t psh, int64_t psw,
                                           u16* __restrict__ out, int S, int H, int W, int C1, int C2, int Cp,
                                           int64_t total, int up = 0) {
  const int V = Cp / 8;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const NhwvIndex ix_ = decode_nhwv(idx, total, H, W, V);
    const int v = ix_.v, xx = ix_.x, y = ix_.y, n = ix_.n;
    const int c0 = v * 8;
    float f[8];
    if (c0 < C1 && up) {
      const int hh = H >> 1, wh = W >> 1, iy = y >> 1, ix = xx >> 1;
      const int ny = (y & 1) ? min(iy + 1, hh - 1) : max(iy - 1, 0);
      const int nx = (xx & 1) ? min(ix + 1, wh - 1) : max(ix - 1, 0);
      const float* b0 = flat + n * fsn + c0;
      const float* p00 = b0 + iy * fsh + ix * fsw;
      const float* p01 = b0 + iy * fsh + nx * fsw;
      const float* p10 = b0 + ny * fsh + ix * fsw;
      const float* p11 = b0 + ny * fsh + nx * fsw;
      __attribute__((aligned(16))) float t00[8], t01[8], t10[8], t11[8];      // (two 16-byte loads per tap; the same fma chain per element)
      *reinterpret_cast<float4*>(t00) = *reinterpret_cast<const float4*>(p00); *reinterpret_cast<float4*>(t00 + 4) = *reinterpret_cast<const float4*>(p00 + 4);
      *reinterpret_cast<float4*>(t01) = *reinterpret_cast<const float4*>(p01); *reinterpret_cast<float4*>(t01 + 4) = *reinterpret_cast<const float4*>(p01 + 4);
      *reinterpret_cast<float4*>(t10) = *reinterpret_cast<const float4*>(p10); *reinterpret_cast<float4*>(t10 + 4) = *reinterpret_cast<const float4*>(p10 + 4);
      *reinterpret_cast<float4*>(t11) = *reinterpret_cast<const float4*>(p11); *reinterpret_cast<float4*>(t11 + 4) = *reinterpret_cast<const float4*>(p11 + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float r = 0.5625f * t00[e];
        r = fmaf(0.1875f, t01[e], r);
        r = fmaf(0.1875f, t10[e], r);
        r = fmaf(0.0625f, t11[e], r);
        f[e] = r;
      }
    } else if (c0 < C1) {                            // C1 % 8 == 0: a vector never straddles the two sources
      const float* src = flat + n * fsn + y * fsh + xx * fsw + c0;
      const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
      const float* src = prop + (n / S) * psn + y * psh + xx * psw + (c0 - C1);
      if (c0 - C1 + 8 <= C2) {
        const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (c0 - C1 + e < C2) ? src[e] : 0.f;
      }
    }
    u16 hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) split1(f[e], hi[e], lo[e]);
    u16* o = out + (((int64_t)n * H + y) * W + xx) * 2 * Cp + c0;
    *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(hi);
    *reinterpret_cast<uint4*>(o + Cp) = *reinterpret_cast<const uint4*>(lo);
  }
}

// ------------------------------------------------------------------ split(g + repeat_S(gm) * scale)
// Gradient of the embedding chain's output (support/networks.py:35-40): the per-sample gradient from the
// concatenation plus the spp-broadcast gradient of the mean, written once as the split dy of the chain's
// backward (separately: broadcast into 268 MB, an elementwise add over 3 x 268 MB, then the split pass).
// g may be null (only the mean path carries gradient).  One thread = 8 channels of one pixel.
__global__ void add_broadcast_split_kernel(const float* __restrict__ g, int64_t gsn, int64_t gsh, int64_t gsw,
                                           const float* __restrict__ gm, int64_t msn, int64_t msh, int64_t msw,
                                           float scale, u16* __restrict__ out, int S, int H, int W, int C, int Cp,
                                           int64_t total) {
  const int V = Cp / 8;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const NhwvIndex ix_ = decode_nhwv(idx, total, H, W, V);
    const int v = ix_.v, xx = ix_.x, y = ix_.y, n = ix_.n;
    const int c0 = v * 8;
    float f[8];
    if (c0 + 8 <= C) {                               // whole vector: two 16-byte loads per operand
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
      if (g) {
        const float* q = g + n * gsn + y * gsh + xx * gsw + c0;
        const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
      }
      if (gm) {
        const float* q = gm + (n / S) * msn + y * msh + xx * msw + c0;
        const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
        f[0] += a.x * scale; f[1] += a.y * scale; f[2] += a.z * scale; f[3] += a.w * scale;
        f[4] += b.x * scale; f[5] += b.y * scale; f[6] += b.z * scale; f[7] += b.w * scale;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float a = 0.f;
        if (c0 + e < C) {
          if (g) a = g[n * gsn + y * gsh + xx * gsw + c0 + e];
          if (gm) a += gm[(n / S) * msn + y * msh + xx * msw + c0 + e] * scale;
        }
        f[e] = a;
      }
    }
    u16 hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) split1(f[e], hi[e], lo[e]);
    u16* o = out + (((int64_t)n * H + y) * W + xx) * 2 * Cp + c0;
    *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(hi);
    *reinterpret_cast<uint4*>(o + Cp) = *reinterpret_cast<const uint4*>(lo);
  }
}

// ------------------------------------------------------------------ the gradient entering a chain's backward -> split + column sums
// out = split((dy [+ repeat_S(gm) * scale]) [* act'(post)]) -- what split_kernel / add_broadcast_split_kernel produce for the
// LAST layer of a chain -- and, in the same pass, the per-block column sums of the result in the layout the GEMM epilogues
// leave ([row][Np] + trailer word = rows written): the layer's bias gradient is then finished by its weight gradient's
// slab-reduction launch (wcmc_conv2d_wgrad_bf16x3, dy_colsum_partial) instead of a column-sum pass that re-reads the split
// tensor (268 MB for a PathNet embedding) plus a finish launch.  One thread = one 8-channel vector of every PL-th pixel of
// the block's range; fixed-order LDS tree over the pixel lanes: bitwise reproducible.
__global__ __launch_bounds__(256) void split_dy_colsum_kernel(const float* __restrict__ dy, int64_t dsn, int64_t dsh, int64_t dsw,
                                                              const float* __restrict__ post, int64_t psn, int64_t psh, int64_t psw,
                                                              int act, float slope, const float* __restrict__ gm, int64_t msn,
                                                              int64_t msh, int64_t msw, int S, float scale, u16* __restrict__ out,
                                                              int H, int W, int C, int Cp, int64_t M, int64_t per_block,
                                                              float* __restrict__ partial, int Np, int Gmax) {
  extern __shared__ __attribute__((aligned(16))) float smem[];      // [PL][V][8]
  const int V = Cp / 8, PL = 256 / V;
  const int v = threadIdx.x % V, pl = threadIdx.x / V;
  const int64_t p0 = (int64_t)blockIdx.x * per_block, p1 = min(M, p0 + per_block);
  const int c0 = v * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (pl < PL) {
    // pixel cursor (n, y, xx) of q, advanced by PL per iteration (the first version divided the 64-bit pixel index three
    // times per pixel: the kernel ran at 1.7 TB/s on its address arithmetic)
    int xx, y, n;
    { const int64_t q0 = p0 + pl; xx = (int)(q0 % W); const int64_t t = q0 / W; y = (int)(t % H); n = (int)(t / H); }
    for (int64_t q = p0 + pl; q < p1; q += PL, xx += PL) {
      while (xx >= W) { xx -= W; if (++y == H) { y = 0; ++n; } }
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
      const bool whole = c0 + 8 <= C;
      if (dy) {
        const float* src = dy + n * dsn + y * dsh + xx * dsw + c0;
        if (whole) {
          const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
          f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) if (c0 + e < C) f[e] = src[e];
        }
      }
      if (gm) {
        const float* src = gm + (n / S) * msn + y * msh + xx * msw + c0;
        if (whole) {
          const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
          f[0] += a.x * scale; f[1] += a.y * scale; f[2] += a.z * scale; f[3] += a.w * scale;
          f[4] += b.x * scale; f[5] += b.y * scale; f[6] += b.z * scale; f[7] += b.w * scale;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) if (c0 + e < C) f[e] += src[e] * scale;
        }
      }
      if (post) {
        const float* ps = post + n * psn + y * psh + xx * psw + c0;
        if (whole) {
          const float4 a = *reinterpret_cast<const float4*>(ps), b = *reinterpret_cast<const float4*>(ps + 4);
          const float g[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] *= act_gate(g[e], act, slope);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (c0 + e < C) f[e] *= act_gate(ps[e], act, slope);
        }
      }
      u16 hi[8], lo[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        split1(f[e], hi[e], lo[e]);
        acc[e] += bf2f(hi[e]) + bf2f(lo[e]);          // (the sum of what the GEMMs will see, as colsum_split_kernel)
      }
      u16* o = out + q * 2 * Cp + c0;
      *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(hi);
      *reinterpret_cast<uint4*>(o + Cp) = *reinterpret_cast<const uint4*>(lo);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) smem[(pl * V + v) * 8 + e] = acc[e];
  }
  __syncthreads();
  if (pl == 0) {
    for (int q = 1; q < PL; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += smem[(q * V + v) * 8 + e];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (c0 + e < Np) partial[(int64_t)blockIdx.x * Np + c0 + e] = (c0 + e < C) ? acc[e] : 0.f;
  }
  // (Np - Cp can be 8: the columns past the last vector)
  if (threadIdx.x < Np - Cp) partial[(int64_t)blockIdx.x * Np + Cp + threadIdx.x] = 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int*>(partial)[(int64_t)Gmax * Np] = (int)gridDim.x;
}

// K order of the packed weights: k = slab*Ks + tap*cs + cl, channel = slab*CS + cl (cs = CS, or CSl in the last slab).  The streaming
// kernel uses one slab of all (padded) channels (CS = Kp, Ks = Kt); the halo kernel cuts the channels into
// slabs of CS <= 64 that fit in LDS with their halo (x_plan_k below decides, from (kchan, ks) alone).
__global__ void pack_weight_split_kernel(const float* __restrict__ w, u16* __restrict__ wp, int Cout, int Cin,
                                         int ks, int mode, int rows, int Np, int CS, int Ks, int Kt, int nslabs, int CSl, int f16) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)Np * Kt) return;
  const int n = (int)(idx / Kt), k = (int)(idx - (int64_t)n * Kt);
  int slab = k / Ks;
  if (slab > nslabs - 1) slab = nslabs - 1;                 // (the last slab's Ks may be the smaller one)
  const int kk = k - slab * Ks;
  const int cs = slab == nslabs - 1 ? CSl : CS;
  const int tap = kk / cs, cl = kk - tap * cs;
  const int c = slab * CS + cl;
  const int taps = ks * ks;
  const int kchan = mode == 0 ? Cin : Cout;
  float v = 0.f;
  if (n < rows && tap < taps && c < kchan) {
    if (mode == 0) v = w[((int64_t)n * Cin + c) * taps + tap];
    else           v = w[((int64_t)c * Cin + n) * taps + (taps - 1 - tap)];
  }
  u16 hi, lo;
  split1(v, hi, lo);
  if (f16) { hi = f2h_sat(v); lo = 0; }          // (mode 4: ONE fp16 plane in the hi rows; the lo rows are never read)
  wp[((int64_t)n * 2) * Kt + k] = hi;
  wp[((int64_t)n * 2 + 1) * Kt + k] = lo;
}

int x_env_on(const char* name) {           // switch is ON unless the variable starts with '0' (debug build only: ab_env)
  const char* e = ab_env(name);
  return (e && e[0] == '0') ? 0 : 1;
}
struct XKPlan { bool halo; int Kp, CS, nslabs, Ks, Kt, PXS, CSl, Ksl, ap; };     // CSl / Ksl: the last (narrower) slab
static int x_pick_nt(int tiles);
// conv_halo64_bf16x3_kernel, last slab of at most FOUR real channels (KPCN's 100 = 6 x 16 + 4 = 3 x 32 + 4): its k order is four
// channels per tap, EIGHT taps per 32-k stage -- 4 stages for the 25 taps instead of the 7 of an 8-channel slab (four taps per stage,
// half of every k-group zeros): 85 -> 82 stages in the forward, 82 -> 79 in the data gradient (-3.6 % MFMAs).  CSl = 4 is the K ORDER
// only: the halo still holds the slab as 8-channel units (one 16-byte DMA granule per plane); a lane's k-group is two 8-byte reads
// from two neighbouring taps.  (WCMC_HALO64_L4=0, debug build: the 8-channel order.)
static bool x_last4(int kchan, int CS, int nslabs) {
  const int left = kchan - (nslabs - 1) * CS;
  return nslabs >= 2 && left >= 1 && left <= 4 && x_env_on("WCMC_HALO64_L4");
}
// ap_req: planes of the A operand (the pixels) the caller wants multiplied -- 2 = hi + lo (three MFMAs per product), 1 = hi only
// (two: W_lo*A_hi + W_hi*A_hi; the data gradient of the "bf16x321" mode).  q.ap is what the plan grants: 1 only where a
// kernel instance for it exists (rows = the GEMM's output channels pick the instance), else the three-term plan.  The K
// order of the packed weights follows the plan, so packing and launch must ask with the same (kchan, ks, ap_req, rows).
static XKPlan x_plan_k(int kchan, int ks, int ap_req = 2, int rows = 0) {
  // (debug build: A/B switches are read per call, so that a script can flip them in one process)
  const int enable = x_env_on("WCMC_IGEMM_HALO");
  XKPlan q;
  q.ap = 2;
  q.Kp = round_up(kchan, 8);
  q.halo = enable && ks >= 3 && ks <= 5 && q.Kp >= 32;
  // (rows: seven cout tiles per block -- the KPCN layers -- or ONE: the first layer's data gradient restricted to the 8 input
  // channels whose gradient is read, ops.conv_chain)
  const int nt_rows = rows > 0 ? x_pick_nt(round_up(rows, 16) / 16) : 0;
  if (ap_req == 1 && q.halo && ks == 5 && x_env_on("WCMC_HALO64") && (nt_rows == 7 || nt_rows == 1) &&
      q.Kp % 32 != 24 && x_env_on("WCMC_DGRAD_AP1")) {
    // conv_halo64_bf16x3_kernel<7, 3, PT, 0, 80, 1>: the halo holds the hi plane only, so a pixel's 80 bytes carry 32 channels
    // instead of 16 -- half the slabs (104 channels = 32 + 32 + 32 + 8: K = 3 x 800 + 224 = 2624 of 2500 useful, three halo
    // reloads per tile instead of six), one tap per 32-k stage (four in the 8-channel slab)
    q.ap = 1;
    q.nslabs = (q.Kp + 31) / 32;
    q.CS = 32; q.CSl = q.Kp - (q.nslabs - 1) * 32;            // 8, 16 or 32
    if (x_last4(kchan, q.CS, q.nslabs)) q.CSl = 4;            // (see x_last4)
    q.PXS = 80;
    q.Ks = round_up(ks * ks * q.CS, 32); q.Ksl = round_up(ks * ks * q.CSl, 32);
    q.Kt = (q.nslabs - 1) * q.Ks + q.Ksl;
    return q;
  }
  if (ap_req == 1 && q.halo && ks == 3 && rows > 0 && x_pick_nt(round_up(rows, 16) / 16) >= 4 && x_env_on("WCMC_DGRAD_AP1")) {
    // conv_halo_bf16x3_kernel<4 | 7, .., AP = 1> (the U-Net's 3x3 data gradients): hi plane only, so a slab holds up to 128 channels
    // in the strides the two-plane plan uses for 64 -- half the halo reloads (and a 224-byte halo for the 64-channel layers)
    q.ap = 1;
    q.nslabs = (q.Kp + 127) / 128;
    q.CS = round_up((q.Kp + q.nslabs - 1) / q.nslabs, 8);
    q.PXS = q.CS <= 112 ? 224 : 288;          // 16 B x (14 or 2 mod 16): conflict-free b128 reads, as below
    q.Ks = round_up(ks * ks * q.CS, 32);
    q.CSl = q.Kp - (q.nslabs - 1) * q.CS;
    if (q.CSl < 32) q.CSl = q.CS;
    q.Ksl = round_up(ks * ks * q.CSl, 32);
    q.Kt = (q.nslabs - 1) * q.Ks + q.Ksl;
    return q;
  }
  if (q.halo && ks == 5 && x_env_on("WCMC_HALO64")) {
    // conv_halo64_bf16x3_kernel: slabs of 16 channels (the last one 8 or 16), halo pixel stride 80 B, two taps per stage
    // (5x5 only: on the U-Net's 3x3 layers it wins 4 % at 128^2 and loses 30-70 % on the 64^2 / 32^2 levels, whose 16x16
    // tilings leave most CUs with one workgroup -- scripts/time_unet_layers.py)
    if (q.Kp >= 256 && q.Kp % 32 == 0 && x_env_on("WCMC_HALO64_CS32")) {
      // many input channels (the 441-cout layer's data gradient: 448): 32-channel slabs, one tap per stage -- half the
      // halo reloads and no padded taps (14 x 800 k instead of 28 x 416); the 160-byte halo only fits the 12x16 tile
      // beside a second workgroup, with two weight stages (launch_xhalo64)
      q.nslabs = q.Kp / 32;
      q.CS = q.CSl = 32;
      q.PXS = 160;
      q.Ks = q.Ksl = round_up(ks * ks * 32, 32);
      q.Kt = q.nslabs * q.Ks;
      return q;
    }
    q.nslabs = (q.Kp + 15) / 16;
    q.CS = 16; q.CSl = q.Kp - (q.nslabs - 1) * 16;
    if (x_last4(kchan, q.CS, q.nslabs)) q.CSl = 4;
    // halo pixel stride 80 B (5 slots of 16 B: hi 0-1, lo 2-3, one of pad).  The ds_read_b128 of the pixel fragments are
    // 2-way bank conflicts with it (PMC: 23-26 % of the LDS cycles; the four 16-lane groups of a b128 read take k-groups 0
    // and 1 of different pixel columns together and 5 f, 5 f' + 1 meet mod 16); 96 B is conflict-free for the 16-channel
    // slabs and measured 0.7 % SLOWER (3.120 vs 3.097 ms per branch: the LDS pipe is not what the loop waits for, and the
    // halo grows by a fifth); the switch for that A/B is gone (round 3)
    q.PXS = 80;
    q.Ks = round_up(ks * ks * q.CS, 32); q.Ksl = round_up(ks * ks * q.CSl, 32);
    q.Kt = (q.nslabs - 1) * q.Ks + q.Ksl;
    return q;
  }
  const int th8 = x_env_on("WCMC_HALO_TH8_5X5");   // =0: A/B switch back to 16x16 tiles with 56/48-channel slabs
  if (q.halo && th8 && ks == 5 && (q.Kp % 32 == 0 || q.Kp % 32 == 8)) {
    // slabs of 32 channels, the last one 32 or 40: halo pixel stride 160 B (10 units = 2 mod 4), 38 KB for a 12x20 halo
    q.nslabs = q.Kp / 32;
    q.CS = 32; q.CSl = q.Kp - (q.nslabs - 1) * 32;
    q.PXS = 160;
    q.Ks = round_up(ks * ks * q.CS, 32); q.Ksl = round_up(ks * ks * q.CSl, 32);
    q.Kt = (q.nslabs - 1) * q.Ks + q.Ksl;
    return q;
  }
  if (q.halo) {
    q.nslabs = (q.Kp + 63) / 64;
    q.CS = round_up((q.Kp + q.nslabs - 1) / q.nslabs, 8);
    q.PXS = q.CS <= 56 ? 224 : 288;           // halo pixel stride: 16 B x (2 or 14 mod 16) -> conflict-free b128 reads
    q.Ks = round_up(ks * ks * q.CS, 32);
    // the last slab holds what is left (104 channels = 56 + 48: 1408 + 1216 k instead of 2 x 1408); the lane's
    // tap stepping assumes at most one wrap per 32-k stage, so a slab narrower than 32 channels is padded instead
    q.CSl = q.Kp - (q.nslabs - 1) * q.CS;
    if (q.CSl < 32) q.CSl = q.CS;
    q.Ksl = round_up(ks * ks * q.CSl, 32);
  } else {
    q.nslabs = 1; q.CS = q.Kp; q.PXS = 0;
    q.Ks = round_up(ks * ks * q.Kp, 32);
    q.CSl = q.CS; q.Ksl = q.Ks;
  }
  q.Kt = (q.nslabs - 1) * q.Ks + q.Ksl;
  return q;
}
// All weights of a chain, both orientations, in ONE launch: a table of up to 20 (layer, mode) entries by value; a block
// finds its entry by its block range and runs pack_weight_split_kernel's body on it.  (114 packing launches of ~4 us per
// step become 16.)
constexpr int XPACK_MAX = 32;      // (2.3 KB of kernel arguments: the fifteen U-Net layers of a PathNet, both orientations, in one launch)
struct XPackEntry { const float* w; u16* wp; int Cout, Cin, mode, rows, Np, CS, Ks, Kt, nslabs, CSl; unsigned block0; int f16; };
struct XPackTable { XPackEntry e[XPACK_MAX]; int n, ks; };
__global__ __launch_bounds__(256) void pack_weight_split_multi_kernel(XPackTable t) {
  int k = 0;
#pragma unroll 1
  for (int i = 1; i < t.n; ++i)
    if (blockIdx.x >= t.e[i].block0) k = i;
  const XPackEntry& q = t.e[k];
  const int64_t idx = (int64_t)(blockIdx.x - q.block0) * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)q.Np * q.Kt) return;
  const int n = (int)(idx / q.Kt), kk0 = (int)(idx - (int64_t)n * q.Kt);
  int slab = kk0 / q.Ks;
  if (slab > q.nslabs - 1) slab = q.nslabs - 1;
  const int kk = kk0 - slab * q.Ks;
  const int cs = slab == q.nslabs - 1 ? q.CSl : q.CS;
  const int tap = kk / cs, cl = kk - tap * cs;
  const int c = slab * q.CS + cl;
  const int taps = t.ks * t.ks;
  const int kchan = q.mode == 0 ? q.Cin : q.Cout;
  float v = 0.f;
  if (n < q.rows && tap < taps && c < kchan) {
    if (q.mode == 0) v = q.w[((int64_t)n * q.Cin + c) * taps + tap];
    else             v = q.w[((int64_t)c * q.Cin + n) * taps + (taps - 1 - tap)];
  }
  u16 hi, lo;
  split1(v, hi, lo);
  if (q.f16) { hi = f2h_sat(v); lo = 0; }
  q.wp[((int64_t)n * 2) * q.Kt + kk0] = hi;
  q.wp[((int64_t)n * 2 + 1) * q.Kt + kk0] = lo;
}

// rows of the per-tile column-sum buffer: enough for either kernel's tiling of (N, Ho, Wo)
static int x_colsum_rows(int N, int Ho, int Wo) {
  const int64_t gl = ceil_div64((int64_t)N * Ho * Wo, 128);
  const int64_t gh = (int64_t)N * ((Ho + 7) / 8) * ((Wo + 15) / 16);      // 8x16 halo tiles (16x16: fewer)
  return (int)(gl > gh ? gl : gh);
}

// bias gradient from a split tensor: partial[g][c] = sum over the block's pixels of hi + lo.
// One thread = 8 channels (two 16-byte loads per pixel), 256/V pixel lanes, LDS tree across them.
__global__ __launch_bounds__(256) void colsum_split_kernel(const u16* __restrict__ dy, int Cp, int C, int64_t M,
                                                            int64_t per_block, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float smem[];      // [PL][V][8]
  const int V = Cp / 8;                      // <= 256 (C <= 2048)
  const int PL = 256 / V;
  const int v = threadIdx.x % V, pl = threadIdx.x / V;
  const int64_t p0 = (int64_t)blockIdx.x * per_block, p1 = min(M, p0 + per_block);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (pl < PL) {
    for (int64_t q = p0 + pl; q < p1; q += PL) {
      const u16* r = dy + q * 2 * Cp + v * 8;
      const uint4 h = *reinterpret_cast<const uint4*>(r), l = *reinterpret_cast<const uint4*>(r + Cp);
      const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[2 * e] += __builtin_bit_cast(float, hw[e] << 16) + __builtin_bit_cast(float, lw[e] << 16);
        acc[2 * e + 1] += __builtin_bit_cast(float, hw[e] & 0xffff0000u) + __builtin_bit_cast(float, lw[e] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) smem[(pl * V + v) * 8 + e] = acc[e];
  }
  __syncthreads();
  if (pl == 0) {
    for (int q = 1; q < PL; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += smem[(q * V + v) * 8 + e];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (v * 8 + e < C) partial[(int64_t)blockIdx.x * C + v * 8 + e] = acc[e];
  }
}

static int x_pick_nt(int tiles) {
  const int cand[4] = {7, 4, 2, 1};
  int best = 1, best_cost = 1 << 30;
  for (int i = 0; i < 4; ++i) {
    const int nt = cand[i];
    const int cost = ((tiles + nt - 1) / nt) * (nt + 2);
    if (cost < best_cost) { best_cost = cost; best = nt; }
  }
  return best;
}

struct XWgradPlan { int rows, rps, R, rTM, rNW; int TM, coBlocks, ciBlocks, S, Np, Cq, G; int64_t pix_per_split, per_block; size_t slab_elems, bytes; };
// terms: bf16 MFMAs per product of the launch (3 | 1).  The one-plane instances need half the LDS per stage, so two of the
// four-wave filter-row blocks share a CU where the two-plane ones run alone: twice the splits for those layers (the
// U-Net's 64-channel levels: 28 -> 23 us, 192 -> 64: 72 -> 47 us; scripts/time_wgrad_unet.py) -- one wave per SIMD cannot hide
// its own DMA issue and barriers.  The slab layout follows the plan: the launch and its reduction ask with the same `terms`.
static XWgradPlan x_plan_wgrad(int N, int Ho, int Wo, int Cout, int Cin, int ks, int terms = 3) {
  XWgradPlan pl;
  pl.Np = round_up(Cout, 16); pl.Cq = round_up(Cin, 16);
  const int coT = pl.Np / 16, ciT = pl.Cq / 16;
  pl.TM = (coT % 7 == 0) ? 7 : 4;
  pl.coBlocks = (coT + pl.TM - 1) / pl.TM;
  pl.ciBlocks = (ciT + 3) / 4;
  const int64_t M = (int64_t)N * Ho * Wo;
  const int taps = ks * ks;
  const int rows_on = x_env_on("WCMC_WGRAD_ROWS");   // =0: A/B switch back to the one-tap-per-block kernel
  // filter-row kernel: (KS, TM, NW) instances below; TM / NW must divide the tile counts
  pl.R = N * Ho; pl.rps = 0; pl.rows = 0; pl.rTM = pl.rNW = 0;
  if (rows_on && (ks == 5 || ks == 3 || (ks == 1 && x_env_on("WCMC_WGRAD_ROWS_1X1"))) && (int64_t)N * Ho >= 64) {
    // measured against the one-tap kernel (scripts/profile_layers.py): the 5x5 layers gain 1.9-2.7x; of the
    // 3x3 U-Net layers only those with >= 256 input channels gain (a filter row is 3 taps of reuse, not 5)
    int tm = 0, nw = 0;
    if (ks == 5) { tm = coT % 7 == 0 ? 7 : 0; nw = ciT % 7 == 0 ? 7 : ciT == 3 ? 3 : 0; }
    else if (ks == 1) {
      // the PathNet 1x1 layers: pure streaming (two operands read once); the stage ring of this kernel fills by LDS-DMA
      // while the previous stage multiplies, the one-tap kernel stages through registers between two barriers
      // (measured, scripts/time_wgrad_1x1.py: 128 -> 128 gains, 220 -> 184 us = 5.8 TB/s; 64 -> 64 is even and the narrow
      // layers 36 -> 64 and 128 -> 3 lose 10-14 %: they stay on the one-tap kernel, which already streams them at 5.6-5.9 TB/s)
      if (coT == 8 && ciT == 8) { tm = 8; nw = 8; }
    }
    else if (ks == 3) {
      // (with the fill overlapped -- see the kernel -- the filter-row kernel also wins on the 128-channel levels: 128 -> 128 at
      // 64^2 57 -> 36 us, 128 -> 256 at 32^2 32 -> 26; the 64-channel layers are even; WCMC_WGRAD_ROWS_3X3=0: A/B switch back
      // to >= 256 input channels only -- scripts/time_wgrad_unet.py)
      const int wide = x_env_on("WCMC_WGRAD_ROWS_3X3");
      const char* e44 = ab_env("WCMC_WGRAD_44");          // (debug build) 1: 4 x 4 channel tiles per block everywhere
      if (coT % 8 == 0 && ciT % 8 == 0 && (ciT >= 16 || wide) && !(e44 && e44[0] == '1')) { tm = 8; nw = 8; }
      else if (wide && coT % 4 == 0 && ciT % 4 == 0) { tm = 4; nw = 4; }
    }
    if (tm && nw) {
      pl.rows = 1; pl.rTM = tm; pl.rNW = nw;
      pl.coBlocks = coT / tm; pl.ciBlocks = ciT / nw;
      // one block per (unit, filter row); the ks blocks of a unit share an XCD (32 CUs x resident blocks
      // per CU): at most that many per XCD keeps the launch to one round
      const size_t lds = xwr_lds_bytes_rt(ks, tm, nw, terms == 1 ? 1 : 2);
      int wpc = (int)((160 * 1024) / lds);
      int wcap = nw <= 4 ? 2 : 1;                     // as the kernel's __launch_bounds__
      { const char* e = ab_env("WCMC_WGRAD_WCAP"); if (e && nw <= 4) wcap = atoi(e); }      // (debug build: scripts/time_wgrad_unet.py)
      int sdiv = 1;
      { const char* e = ab_env("WCMC_WGRAD_SDIV"); if (e) sdiv = atoi(e); }                 // (debug build: fewer, longer splits)
      if (wpc > wcap) wpc = wcap;
      if (wpc < 1) wpc = 1;
      int S = 8 * ((32 * wpc) / ks) / (pl.coBlocks * pl.ciBlocks) / sdiv;
      if (S > pl.R / 4) S = pl.R / 4;                 // at least 4 rows per block
      if (S < 1) S = 1;
      pl.rps = (pl.R + S - 1) / S;
      pl.S = (pl.R + pl.rps - 1) / pl.rps;
      pl.pix_per_split = 0;
    }
  }
  const int64_t tiles = (int64_t)taps * pl.coBlocks * pl.ciBlocks;
  // ~2 waves of 512 co-resident blocks for the multi-tap convs; one wave for the HBM-bound 1x1 layers,
  // whose slab traffic (S x Np x Cq floats, written and re-read) otherwise rivals the operand stream
  int64_t S = (ks == 1 ? 512 : 1024) / tiles;
  const int64_t maxS = M / 512 > 0 ? M / 512 : 1;     // >= 8 stages of 64 pixels per block
  if (S > maxS) S = maxS;
  if (S < 1) S = 1;
  if (!pl.rows) {
    pl.pix_per_split = ceil_div64(ceil_div64(M, S), 64) * 64;
    pl.S = (int)ceil_div64(M, pl.pix_per_split);
  }
  pl.slab_elems = (size_t)pl.S * taps * pl.Np * pl.Cq;
  pl.G = (int)(M / 64 > 0 ? (M / 64 < 1024 ? M / 64 : 1024) : 1);
  pl.per_block = ceil_div64(M, pl.G);
  pl.G = (int)ceil_div64(M, pl.per_block);
  pl.bytes = (pl.slab_elems + (size_t)pl.G * Cout) * sizeof(float);
  return pl;
}

}  // namespace wcmc

using namespace wcmc;

extern "C" size_t wcmc_split_elems(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return (size_t)N * H * W * 2 * round_up(C, 8);
}

extern "C" int wcmc_split_bf16(const float* x, int64_t xsn, int64_t xsh, int64_t xsw, void* out, int N, int H, int W,
                               int C, void* stream) {
  WCMC_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && out, WCMC_ERR_BAD_ARG, "split_bf16: bad argument");
  WCMC_REQUIRE(nhwc_view_ok(x, xsn, xsh, xsw, C) && aligned16(out), WCMC_ERR_ALIGNMENT,
               "split_bf16: x violates the NHWC-view contract (or out unaligned)");
  const int Cp = round_up(C, 8);
  const int64_t total = (int64_t)N * H * W * (Cp / 8);
  const int64_t blocks = ceil_div64(total, 256);
  hipLaunchKernelGGL(split_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                     x, xsn, xsh, xsw, (u16*)out, H, W, C, Cp, total, (const float*)nullptr, (int64_t)0, (int64_t)0,
                     (int64_t)0, 0, 0.f);
  return check_launch("split_bf16");
}

extern "C" int wcmc_split_gated_bf16(const float* dy, int64_t xsn, int64_t xsh, int64_t xsw, const float* post, int64_t psn,
                                     int64_t psh, int64_t psw, int act, float slope, void* out, int N, int H, int W, int C,
                                     void* stream) {
  WCMC_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && out, WCMC_ERR_BAD_ARG, "split_gated_bf16: bad argument");
  WCMC_REQUIRE(nhwc_view_ok(dy, xsn, xsh, xsw, C) && nhwc_view_ok(post, psn, psh, psw, C) && aligned16(out),
               WCMC_ERR_ALIGNMENT, "split_gated_bf16: dy / post violate the NHWC-view contract (or out unaligned)");
  const int Cp = round_up(C, 8);
  const int64_t total = (int64_t)N * H * W * (Cp / 8);
  const int64_t blocks = ceil_div64(total, 256);
  hipLaunchKernelGGL(split_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                     dy, xsn, xsh, xsw, (u16*)out, H, W, C, Cp, total, post, psn, psh, psw, act, slope);
  return check_launch("split_gated_bf16");
}

extern "C" int wcmc_split_from_nchw(const float* src, int64_t ssn, int64_t ssc, int64_t ssh, int64_t ssw, void* out_split,
                                    int N, int C, int H, int W, void* stream) {
  WCMC_REQUIRE(src && out_split && N > 0 && C > 0 && C <= 64 && H > 0 && W > 0, WCMC_ERR_BAD_ARG,
               "split_from_nchw: bad argument (at most 64 channels)");
  WCMC_REQUIRE(aligned16(out_split), WCMC_ERR_ALIGNMENT, "split_from_nchw: out must be 16-byte aligned");
  WCMC_REQUIRE((int64_t)N * H <= 65535, WCMC_ERR_BAD_ARG, "split_from_nchw: N*H > 65535");
  hipLaunchKernelGGL(nchw_split_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)(N * H)), dim3(256), 0,
                     (hipStream_t)stream, src, ssn, ssc, ssh, ssw, (u16*)out_split, C, round_up(C, 8), H, W);
  return check_launch("split_from_nchw");
}

extern "C" int wcmc_cat_broadcast_split(const float* flat, int64_t fsn, int64_t fsh, int64_t fsw, const float* prop,
                                       int64_t psn, int64_t psh, int64_t psw, void* out_split, int B, int S, int H,
                                       int W, int C1, int C2, void* stream) {
  WCMC_REQUIRE(flat && prop && out_split && B > 0 && S > 0 && H > 0 && W > 0 && C1 > 0 && C2 > 0, WCMC_ERR_BAD_ARG,
               "cat_broadcast_split: bad argument");
  WCMC_REQUIRE(C1 % 8 == 0, WCMC_ERR_BAD_ARG, "cat_broadcast_split: the first operand needs a multiple of 8 channels");
  WCMC_REQUIRE(nhwc_view_ok(flat, fsn, fsh, fsw, C1) && nhwc_view_ok(prop, psn, psh, psw, C2) && aligned16(out_split),
               WCMC_ERR_ALIGNMENT, "cat_broadcast_split: a view violates the NHWC-view contract");
  const int Cp = round_up(C1 + C2, 8);
  const int64_t total = (int64_t)B * S * H * W * (Cp / 8);
  const int64_t blocks = ceil_div64(total, 256);
  hipLaunchKernelGGL(cat_broadcast_split_kernel, dim3((unsigned)(blocks > 65535 ? 65535 : blocks)), dim3(256), 0,
                     (hipStream_t)stream, flat, fsn, fsh, fsw, prop, psn, psh, psw, (u16*)out_split, S, H, W, C1, C2, Cp,
                     total, 0);
  return check_launch("cat_broadcast_split");
}

extern "C" int wcmc_cat_upsample_split(const float* deep, int64_t dsn, int64_t dsh, int64_t dsw, const float* skip,
                                       int64_t ssn, int64_t ssh, int64_t ssw, void* out_split, int N, int H, int W, int C1,
                                       int C2, void* stream) {
  WCMC_REQUIRE(deep && skip && out_split && N > 0 && H > 1 && W > 1 && (H % 2) == 0 && (W % 2) == 0 && C1 > 0 && C2 > 0,
               WCMC_ERR_BAD_ARG, "cat_upsample_split: bad argument (H and W are the fine, even, geometry)");
  WCMC_REQUIRE(C1 % 8 == 0, WCMC_ERR_BAD_ARG, "cat_upsample_split: the upsampled operand needs a multiple of 8 channels");
  WCMC_REQUIRE(nhwc_view_ok(deep, dsn, dsh, dsw, C1) && nhwc_view_ok(skip, ssn, ssh, ssw, C2) && aligned16(out_split),
               WCMC_ERR_ALIGNMENT, "cat_upsample_split: a view violates the NHWC-view contract");
  const int Cp = round_up(C1 + C2, 8);
  const int64_t total = (int64_t)N * H * W * (Cp / 8);
  const int64_t blocks = ceil_div64(total, 256);
  hipLaunchKernelGGL(cat_broadcast_split_kernel, dim3((unsigned)(blocks > 65535 ? 65535 : blocks)), dim3(256), 0,
                     (hipStream_t)stream, deep, dsn, dsh, dsw, skip, ssn, ssh, ssw, (u16*)out_split, 1, H, W, C1, C2, Cp,
                     total, 1);
  return check_launch("cat_upsample_split");
}

extern "C" int wcmc_add_broadcast_split(const float* g, int64_t gsn, int64_t gsh, int64_t gsw, const float* gm,
                                       int64_t msn, int64_t msh, int64_t msw, float scale, void* out_split, int B,
                                       int S, int H, int W, int C, void* stream) {
  WCMC_REQUIRE((g || gm) && out_split && B > 0 && S > 0 && H > 0 && W > 0 && C > 0, WCMC_ERR_BAD_ARG,
               "add_broadcast_split: bad argument");
  WCMC_REQUIRE((!g || nhwc_view_ok(g, gsn, gsh, gsw, C)) && (!gm || nhwc_view_ok(gm, msn, msh, msw, C)) &&
                   aligned16(out_split),
               WCMC_ERR_ALIGNMENT, "add_broadcast_split: a view violates the NHWC-view contract");
  const int Cp = round_up(C, 8);
  const int64_t total = (int64_t)B * S * H * W * (Cp / 8);
  const int64_t blocks = ceil_div64(total, 256);
  hipLaunchKernelGGL(add_broadcast_split_kernel, dim3((unsigned)(blocks > 65535 ? 65535 : blocks)), dim3(256), 0,
                     (hipStream_t)stream, g, gsn, gsh, gsw, gm, msn, msh, msw, scale, (u16*)out_split, S, H, W, C, Cp,
                     total);
  return check_launch("add_broadcast_split");
}

extern "C" int wcmc_split_dy_colsum_bf16(const float* dy, int64_t dsn, int64_t dsh, int64_t dsw, const float* post, int64_t psn,
                                         int64_t psh, int64_t psw, int act, float slope, const float* gm, int64_t msn,
                                         int64_t msh, int64_t msw, int S, float scale, void* out_split, float* colsum_partial,
                                         int N, int H, int W, int C, void* stream) {
  WCMC_REQUIRE((dy || gm) && out_split && colsum_partial && N > 0 && S > 0 && H > 0 && W > 0 && C > 0 && C <= 2048,
               WCMC_ERR_BAD_ARG, "split_dy_colsum_bf16: bad argument");
  WCMC_REQUIRE(!gm || N % S == 0, WCMC_ERR_BAD_ARG, "split_dy_colsum_bf16: N must be a multiple of S");
  WCMC_REQUIRE((!dy || nhwc_view_ok(dy, dsn, dsh, dsw, C)) && (!post || nhwc_view_ok(post, psn, psh, psw, C)) &&
                   (!gm || nhwc_view_ok(gm, msn, msh, msw, C)) && aligned16(out_split),
               WCMC_ERR_ALIGNMENT, "split_dy_colsum_bf16: a view violates the NHWC-view contract (or out unaligned)");
  const int Cp = round_up(C, 8), Np = round_up(C, 16);
  const int64_t M = (int64_t)N * H * W;
  const int Gmax = x_colsum_rows(N, H, W);
  int blocks = Gmax < 1024 ? Gmax : 1024;
  const int64_t per_block = ceil_div64(M, blocks);
  blocks = (int)ceil_div64(M, per_block);
  hipLaunchKernelGGL(split_dy_colsum_kernel, dim3((unsigned)blocks), dim3(256), (size_t)256 * 8 * sizeof(float),
                     (hipStream_t)stream, dy, dsn, dsh, dsw, post, psn, psh, psw, act, slope, gm, msn, msh, msw, S, scale,
                     (u16*)out_split, H, W, C, Cp, M, per_block, colsum_partial, Np, Gmax);
  return check_launch("split_dy_colsum_bf16");
}

// mode of a packed weight: 0 = forward orientation, 1 = data-gradient orientation (flipped taps, channels swapped), 2 = the
// data-gradient orientation in the K order of a TWO-term launch (terms = 2 of wcmc_conv2d_igemm_bf16x3: x hi plane only)
// 3 = the FORWARD orientation in the K order of a two- / one-term launch (terms <= 2 of a forward launch: the un-gated output layers
// of the "bf16x321o" mode)
// 4 = mode 3 with the weights rounded ONCE to fp16 in the hi rows (wcmc_conv2d_out_f16; the lo rows are zero and never read)
static inline int x_mode_ap(int mode) { return mode >= 2 ? 1 : 2; }
static inline bool x_mode_fwd(int mode) { return mode == 0 || mode == 3 || mode == 4; }
extern "C" size_t wcmc_conv2d_packed_elems_bf16x3(int rows, int kchan, int ks, int mode) {
  if (rows <= 0 || kchan <= 0 || ks <= 0 || mode < 0 || mode > 4) return 0;
  return (size_t)round_up(rows, 16) * 2 * x_plan_k(kchan, ks, x_mode_ap(mode), rows).Kt;
}

extern "C" int wcmc_conv2d_pack_weight_bf16x3(const float* w, void* wp, int Cout, int Cin, int ks, int mode,
                                              void* stream) {
  WCMC_REQUIRE(w && wp && Cout > 0 && Cin > 0 && ks > 0 && mode >= 0 && mode <= 4, WCMC_ERR_BAD_ARG,
               "conv2d_pack_weight_bf16x3: bad argument");
  const int rows = x_mode_fwd(mode) ? Cout : Cin, kchan = x_mode_fwd(mode) ? Cin : Cout;
  const int Np = round_up(rows, 16);
  const XKPlan q = x_plan_k(kchan, ks, x_mode_ap(mode), rows);
  const int64_t total = (int64_t)Np * q.Kt;
  hipLaunchKernelGGL(pack_weight_split_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0,
                     (hipStream_t)stream, w, (u16*)wp, Cout, Cin, ks, x_mode_fwd(mode) ? 0 : 1, rows, Np, q.CS, q.Ks, q.Kt, q.nslabs, q.CSl, mode == 4 ? 1 : 0);
  return check_launch("conv2d_pack_weight_bf16x3");
}

extern "C" int wcmc_conv2d_pack_chain_bf16x3(int n_entries, const float* const* w, void* const* wp, const int* Cout,
                                             const int* Cin, const int* mode, int ks, void* stream) {
  WCMC_REQUIRE(n_entries > 0 && n_entries <= XPACK_MAX && w && wp && Cout && Cin && mode && ks > 0, WCMC_ERR_BAD_ARG,
               "conv2d_pack_chain_bf16x3: bad argument (at most %d entries)", XPACK_MAX);
  XPackTable t;
  t.n = n_entries; t.ks = ks;
  unsigned blocks = 0;
  for (int i = 0; i < n_entries; ++i) {
    WCMC_REQUIRE(w[i] && wp[i] && Cout[i] > 0 && Cin[i] > 0 && mode[i] >= 0 && mode[i] <= 4, WCMC_ERR_BAD_ARG,
                 "conv2d_pack_chain_bf16x3: bad entry %d", i);
    XPackEntry& e = t.e[i];
    e.w = w[i]; e.wp = (u16*)wp[i]; e.Cout = Cout[i]; e.Cin = Cin[i]; e.mode = x_mode_fwd(mode[i]) ? 0 : 1;      // (the kernel knows orientations only)
    e.f16 = mode[i] == 4 ? 1 : 0;
    e.rows = x_mode_fwd(mode[i]) ? Cout[i] : Cin[i];
    const int kchan = x_mode_fwd(mode[i]) ? Cin[i] : Cout[i];
    e.Np = round_up(e.rows, 16);
    const XKPlan q = x_plan_k(kchan, ks, x_mode_ap(mode[i]), e.rows);
    e.CS = q.CS; e.Ks = q.Ks; e.Kt = q.Kt; e.nslabs = q.nslabs; e.CSl = q.CSl;
    e.block0 = blocks;
    blocks += (unsigned)ceil_div64((int64_t)e.Np * q.Kt, 256);
  }
  hipLaunchKernelGGL(pack_weight_split_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, t);
  return check_launch("conv2d_pack_chain_bf16x3");
}

extern "C" int wcmc_conv2d_wgrad_reduce_multi(int n, void* const* workspace, float* const* dw, float* const* db,
                                              const float* const* dy_colsum_partial, const int* N, const int* Ho, const int* Wo,
                                              const int* Cout, const int* Cin, const int* ks, int terms, void* stream) {
  WCMC_REQUIRE(n > 0 && n <= WRM_MAX && workspace && dw && db && dy_colsum_partial && N && Ho && Wo && Cout && Cin && ks &&
               (terms == 1 || terms == 3), WCMC_ERR_BAD_ARG, "conv2d_wgrad_reduce_multi: bad argument (1..%d layers)", WRM_MAX);
  WRMTable t;
  t.n = n;
  unsigned blocks = 0;
  size_t lds = 0;
  for (int i = 0; i < n; ++i) {
    WCMC_REQUIRE(workspace[i] && dw[i] && N[i] > 0 && Ho[i] > 0 && Wo[i] > 0 && Cout[i] > 0 && Cin[i] > 0 && ks[i] > 0 && ks[i] <= 7,
                 WCMC_ERR_BAD_ARG, "conv2d_wgrad_reduce_multi: bad layer %d", i);
    WCMC_REQUIRE(!db[i] || dy_colsum_partial[i], WCMC_ERR_BAD_ARG,
                 "conv2d_wgrad_reduce_multi: layer %d wants a bias gradient without the column sums of dy", i);
    const XWgradPlan pl = x_plan_wgrad(N[i], Ho[i], Wo[i], Cout[i], Cin[i], ks[i], terms);
    WRMEntry& e = t.e[i];
    const bool fuse_db = db[i] != nullptr;
    e.slabs = (const float*)workspace[i]; e.dw = dw[i]; e.cs_partial = fuse_db ? dy_colsum_partial[i] : nullptr; e.db = db[i];
    e.S = pl.S; e.taps = ks[i] * ks[i]; e.Cout = Cout[i]; e.Cin = Cin[i]; e.Np = pl.Np; e.Cq = pl.Cq;
    e.cs_gmax = x_colsum_rows(N[i], Ho[i], Wo[i]); e.cs_ld = round_up(Cout[i], 16);
    e.gx = (Cin[i] + WR_CI - 1) / WR_CI;
    e.block0 = blocks;
    blocks += (unsigned)e.gx * (unsigned)(Cout[i] + (fuse_db ? (Cout[i] + 63) / 64 : 0));
    size_t l = (size_t)WR_CI * (e.taps + 1) * sizeof(float) + 256 * sizeof(float);
    if (fuse_db && l < (size_t)16 * 64 * sizeof(float)) l = (size_t)16 * 64 * sizeof(float);
    if (l > lds) lds = l;
  }
  hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3(blocks), dim3(256), lds, (hipStream_t)stream, t);
  return check_launch("conv2d_wgrad_reduce_multi");
}

// ---- the fp16 one-MFMA forward of an un-gated 5x5 output layer ("bf16x321h" mode; profiles/r04_forward_ladder.txt, table "last", rung E)
static bool x_out_f16_plan(int Cin, int Cout, int ks, XKPlan* q) {
  if (ks != 5 || Cin <= 0 || Cout <= 0) return false;
  *q = x_plan_k(Cin, ks, 1, Cout);
  return q->ap == 1 && q->halo && q->PXS == 80 && x_pick_nt(round_up(Cout, 16) / 16) == 7;
}
extern "C" int wcmc_conv2d_out_f16_supported(int Cin, int Cout, int ks) {
  XKPlan q;
  return x_out_f16_plan(Cin, Cout, ks, &q) ? 1 : 0;
}
extern "C" size_t wcmc_split_to_f16_elems(int N, int H, int W, int C) {
  return (N > 0 && H > 0 && W > 0 && C > 0) ? (size_t)N * H * W * round_up(C, 8) : 0;
}
extern "C" int wcmc_split_to_f16(const void* x_split, int N, int H, int W, int C, void* out_f16, void* stream) {
  WCMC_REQUIRE(x_split && out_f16 && N > 0 && H > 0 && W > 0 && C > 0, WCMC_ERR_BAD_ARG, "split_to_f16: bad argument");
  WCMC_REQUIRE(aligned16(x_split) && aligned16(out_f16), WCMC_ERR_ALIGNMENT, "split_to_f16: buffers must be 16-byte aligned");
  const int Cp = round_up(C, 8);
  const int64_t total = (int64_t)N * H * W * (Cp / 8);
  const int64_t blocks = ceil_div64(total, 256);
  hipLaunchKernelGGL(split_to_f16_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                     (const u16*)x_split, (u16*)out_f16, Cp, total);
  return check_launch("split_to_f16");
}

// ---- one decision path for the GEMM launches: shape -> parameters -> plan -> launch.  The launch-plan query runs the first three.
// The scalar half of the entries' argument checks and every field of p that follows from the shape (the pointers are the entry's).
// gated: a gate, a gate mask or a mask output is asked for; f16: the wcmc_conv2d_out_f16 launch (one fp16 plane, terms = 1).
static int x_igemm_shape(XIgemmParams& p, const char* who, int N, int H, int W, int Cin, int Cout, int ks, int pad, int terms,
                         bool split_out, int64_t ysn, int64_t ysh, int64_t ysw, bool gated, bool f16) {
  WCMC_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && ks > 0 && pad >= 0, WCMC_ERR_BAD_ARG, "%s: bad argument", who);
  WCMC_REQUIRE(terms >= 1 && terms <= 3, WCMC_ERR_BAD_ARG,
               "%s: terms must be 3, 2 (x hi plane only; wp packed with mode 2 / 3) or 1 (hi planes of x and W only)", who);
  const int Ho = H + 2 * pad - ks + 1, Wo = W + 2 * pad - ks + 1;
  WCMC_REQUIRE(Ho > 0 && Wo > 0, WCMC_ERR_BAD_ARG, "%s: empty output", who);
  WCMC_REQUIRE(!gated || split_out, WCMC_ERR_BAD_ARG, "%s: a gate / a mask requires the split output geometry", who);
  XKPlan q;
  if (f16)
    WCMC_REQUIRE(x_out_f16_plan(Cin, Cout, ks, &q), WCMC_ERR_BAD_ARG,
                 "%s: no fp16 instance for this shape (ask wcmc_conv2d_out_f16_supported; 5x5, cout blocks of seven tiles)", who);
  else
    q = x_plan_k(Cin, ks, terms <= 2 ? 1 : 2, Cout);
  p = XIgemmParams{};
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cpi = round_up(Cin, 8);
  p.ysn = ysn; p.ysh = ysh; p.ysw = ysw;
  p.Cpo = split_out ? round_up(Cout, 8) : round_up(Cout, 4);
  p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
  p.ks = ks; p.pad = pad;
  p.ap = f16 ? 1 : q.ap;
  // one term: where the plan grants the hi-plane instance of the 64-pixel 5x5 kernel (the only one with a one-plane weight path);
  // anywhere else the launch multiplies what the plan's instance multiplies (two or three terms) -- more exact, never less
  p.wplanes = (f16 || (terms == 1 && q.ap == 1 && ks == 5 && q.PXS == 80 && x_pick_nt(round_up(Cout, 16) / 16) == 7)) ? 1 : 2;
  p.f16 = f16 ? 1 : 0;
  p.Kp = p.Cpi; p.Kt = q.Kt; p.Np = round_up(Cout, 16);
  p.CS = q.CS; p.nslabs = q.nslabs; p.SPS = q.Ks / 32; p.PXS = q.halo ? q.PXS : 0;
  p.CSl = q.CSl; p.SPSl = q.Ksl / 32;
  p.tilesY = (Ho + 15) / 16; p.tilesX = (Wo + 15) / 16;
  p.G = x_colsum_rows(N, Ho, Wo);
  p.M = (int64_t)N * Ho * Wo;
  const size_t xb = (f16 ? (size_t)N * H * W * p.Cpi : wcmc_split_elems(N, H, W, Cin)) * sizeof(u16), wb = (size_t)p.Np * 2 * p.Kt * sizeof(u16);
  WCMC_REQUIRE(xb < 0x7ff00000u && wb < 0x7ff00000u, WCMC_ERR_BAD_ARG, "%s: operand larger than 2 GiB (split the batch)", who);
  // (the halo kernels push the weight-DMA offsets of stages past the end out of range by adding 2^30: see dma_b)
  WCMC_REQUIRE(!q.halo || wb < 0x40000000u, WCMC_ERR_BAD_ARG, "%s: packed weights of 1 GiB or more", who);
  p.x_bytes = (unsigned)xb; p.wp_bytes = (unsigned)wb;
  return 0;
}
// Which family runs the launch and that family's plan (bf16x3_common.h).  Reads of p only: which output and whether a gate tensor
// is given are asked of the pointers being null or not.
struct XConvPlan {
  enum { PW, HALO3, IGEMM, HALO, HALO64 } family;
  XPwPlan pw; XHalo3Plan h3; XIgemmPlan ig; XHaloPlan halo; XHalo64Plan h64;
};
static int x_plan_conv(const XIgemmParams& p, XConvPlan* c) {
  const int nt = x_pick_nt(p.Np / 16);
  if (x_plan_pw(p, &c->pw)) c->family = XConvPlan::PW;
  else if (x_halo3_ok(p)) { c->family = XConvPlan::HALO3; c->h3 = x_plan_halo3(p); }
  else if (!p.PXS) { c->family = XConvPlan::IGEMM; c->ig = x_plan_igemm(nt, p); }
  else if (x_halo_is64(p)) { c->family = XConvPlan::HALO64; c->h64 = x_plan_halo64(nt, p); }
  else { c->family = XConvPlan::HALO; return x_plan_halo(nt, p, &c->halo); }
  return 0;
}
static int x_launch_conv(const XConvPlan& c, XIgemmParams& p, hipStream_t st) {
  switch (c.family) {
    case XConvPlan::PW: return launch_xpw(p, c.pw, st);
    case XConvPlan::HALO3: return launch_xhalo3(c.h3, p, st);
    case XConvPlan::IGEMM: return launch_xigemm(c.ig, p, st);
    case XConvPlan::HALO64: return launch_xhalo64(c.h64, p, st);
    default: return launch_xhalo(c.halo, p, st);
  }
}
// Profiler class (the vocabulary of bench.py: a class that names ONE kernel instance there is given to that instance only, every
// other kernel is "conv_igemm") and the kernel as rocprofv3 prints it, every template argument written out.
static int x_name_conv(const XConvPlan& c, const XIgemmParams& p, char* cls, char* kernel, size_t len) {      // returns the longer string's length
  const char* k = "conv_igemm";
  int kn = 0, cn = 0;
  switch (c.family) {
    case XConvPlan::PW:
      k = "conv_pw";
      kn = snprintf(kernel, len, "conv_pw_bf16x3_kernel<%d, %d, %s, 0>", c.pw.ntw, c.pw.u, p.ys ? "true" : "false");
      break;
    case XConvPlan::HALO3:
      k = c.h3.ap == 2 ? "conv_halo3" : "conv_halo3_x2";
      kn = snprintf(kernel, len, "conv_halo3_bf16x3_kernel<%d, %d, 2, 0>", c.h3.ap, c.h3.spt);
      break;
    case XConvPlan::IGEMM:
      kn = snprintf(kernel, len, "conv_igemm_bf16x3_kernel<%d, %s, %s, 0>", c.ig.nt, c.ig.padded ? "true" : "false", c.ig.dbuf ? "true" : "false");
      break;
    case XConvPlan::HALO:
      if (c.halo.nt == 7 && c.halo.th == 8 && c.halo.ap == 2) k = "conv_halo7";
      kn = snprintf(kernel, len, "conv_halo_bf16x3_kernel<%d, %d, 16, 0, %d, %d>", c.halo.nt, c.halo.th, c.halo.nb, c.halo.ap);
      break;
    case XConvPlan::HALO64: {
      const XHalo64Plan& h = c.h64;
      if (h.nt == 7 && h.nb == 2 && h.pt == 3 && h.pxst == 160) k = "conv_halo64_cs32";
      else if (h.nt == 7 && h.nb == 3 && h.pxst == 80) {
        cn = snprintf(cls, len, "conv_halo64_pt%d%s", h.pt, h.f16 ? "_h1" : h.wp == 1 ? "_x1" : h.ap == 1 ? "_x2" : "");
        k = nullptr;
      }
      kn = snprintf(kernel, len, "conv_halo64_bf16x3_kernel<%d, %d, %d, 0, %d, %d, %d, %d>", h.nt, h.nb, h.pt, h.pxst, h.ap, h.wp, h.f16);
      break;
    }
  }
  if (k) cn = snprintf(cls, len, "%s", k);
  return cn > kn ? cn : kn;
}

extern "C" int wcmc_conv2d_launch_plan_bf16x3(int N, int H, int W, int Cin, int Cout, int ks, int pad, int terms, int split_out,
                                              int64_t ysn, int64_t ysh, int64_t ysw, int gate_tensor, int out_f16,
                                              char* cls, char* kernel, size_t len) {
  const char* who = "conv2d_launch_plan_bf16x3";
  WCMC_REQUIRE(cls && kernel && len > 0, WCMC_ERR_BAD_ARG, "%s: bad argument", who);
  WCMC_REQUIRE(!out_f16 || (!split_out && !gate_tensor), WCMC_ERR_BAD_ARG, "%s: the fp16 launch writes an fp32 view, un-gated", who);
  XIgemmParams p;
  if (const int rc = x_igemm_shape(p, who, N, H, W, Cin, Cout, ks, pad, out_f16 ? 1 : terms, split_out != 0, ysn, ysh, ysw,
                                   gate_tensor != 0, out_f16 != 0)) return rc;
  static const u16 given = 0;              // (never read: the plans ask only whether a pointer is null)
  if (split_out) p.ys = const_cast<u16*>(&given); else p.yf = reinterpret_cast<float*>(const_cast<u16*>(&given));
  if (gate_tensor) p.gate = &given;
  XConvPlan c;
  if (const int rc = x_plan_conv(p, &c)) return rc;
  WCMC_REQUIRE((size_t)x_name_conv(c, p, cls, kernel, len) < len, WCMC_ERR_BAD_ARG, "%s: buffers of %zu bytes are too short", who, len);
  return 0;
}

extern "C" int wcmc_conv2d_igemm_bf16x3(const void* x_split, int N, int H, int W, int Cin, const void* wp,
                                        const float* bias, float* y, int64_t ysn, int64_t ysh, int64_t ysw,
                                        void* y_split, int Cout, int ks, int pad, int act, float slope,
                                        const void* gate_split, int gate_act, float gate_slope,
                                        float* colsum_partial, const void* gate_mask, void* mask_out,
                                        int terms, void* stream) {
  const char* who = "conv2d_igemm_bf16x3";
  WCMC_REQUIRE(x_split && wp, WCMC_ERR_BAD_ARG, "%s: bad argument", who);
  WCMC_REQUIRE(!colsum_partial || y_split, WCMC_ERR_BAD_ARG,
               "conv2d_igemm_bf16x3: column sums are produced with the split output only");
  WCMC_REQUIRE((y != nullptr) != (y_split != nullptr), WCMC_ERR_BAD_ARG,
               "conv2d_igemm_bf16x3: exactly one of y (fp32 view) and y_split must be given");
  XIgemmParams p;
  if (const int rc = x_igemm_shape(p, who, N, H, W, Cin, Cout, ks, pad, terms, y_split != nullptr, ysn, ysh, ysw,
                                   gate_split || gate_mask || mask_out, false)) return rc;
  WCMC_REQUIRE(aligned16(x_split) && aligned16(wp) && (!y_split || aligned16(y_split)) &&
                   (!gate_split || aligned16(gate_split)),
               WCMC_ERR_ALIGNMENT, "conv2d_igemm_bf16x3: split buffers must be 16-byte aligned");
  WCMC_REQUIRE(!y || nhwc_view_ok(y, ysn, ysh, ysw, Cout), WCMC_ERR_ALIGNMENT,
               "conv2d_igemm_bf16x3: y violates the NHWC-view contract");
  WCMC_REQUIRE(!(gate_split && gate_mask), WCMC_ERR_BAD_ARG, "conv2d_igemm_bf16x3: gate_split and gate_mask are exclusive");
  p.x = (const u16*)x_split; p.wp = (const u16*)wp; p.bias = bias;
  p.yf = y; p.ys = (u16*)y_split;
  p.gate = (const u16*)gate_split; p.gate_act = gate_act; p.gate_slope = gate_slope;
  p.gate_mask = (const unsigned char*)gate_mask; p.mask_out = (unsigned char*)mask_out;
  p.act = act; p.slope = slope;
  p.colsum = colsum_partial;
#ifdef WCMC_DEBUG_BUILD
  {  // timing-only experiments (guide section 7: zero-record descriptors drop one operand's traffic)
    static int dbg = -1;
    if (dbg < 0) { const char* e = ab_env("WCMC_DEBUG_DROP"); dbg = e ? atoi(e) : 0; }
    if (dbg & 1) p.x_bytes = 0;
    if (dbg & 2) p.wp_bytes = 0;
  }
#endif
  XConvPlan c;
  if (const int rc = x_plan_conv(p, &c)) return rc;
  return x_launch_conv(c, p, (hipStream_t)stream);
}

extern "C" int wcmc_conv2d_out_f16(const void* x_f16, int N, int H, int W, int Cin, const void* wp_f16, const float* bias, float* y,
                                   int64_t ysn, int64_t ysh, int64_t ysw, int Cout, int ks, int pad, void* stream) {
  const char* who = "conv2d_out_f16";
  WCMC_REQUIRE(x_f16 && wp_f16 && y, WCMC_ERR_BAD_ARG, "%s: bad argument", who);
  XIgemmParams p;
  if (const int rc = x_igemm_shape(p, who, N, H, W, Cin, Cout, ks, pad, 1, false, ysn, ysh, ysw, false, true)) return rc;
  WCMC_REQUIRE(aligned16(x_f16) && aligned16(wp_f16) && nhwc_view_ok(y, ysn, ysh, ysw, Cout), WCMC_ERR_ALIGNMENT,
               "conv2d_out_f16: unaligned operand or y violates the NHWC-view contract");
  p.x = (const u16*)x_f16; p.wp = (const u16*)wp_f16; p.bias = bias; p.yf = y;
  p.gate_act = WCMC_ACT_LINEAR; p.act = WCMC_ACT_LINEAR;
  XConvPlan c;
  if (const int rc = x_plan_conv(p, &c)) return rc;
  return x_launch_conv(c, p, (hipStream_t)stream);
}

static bool x_pair_enabled() {
  const char* e = ab_env("WCMC_IGEMM_PW");
  const char* t = ab_env("WCMC_PW_TAIL");       // WCMC_PW_TAIL=0: A/B switch back to two launches
  return !(e && e[0] == '0') && !(t && t[0] == '0');
}
// fused instances: (input units, couts of the first layer, tail kind)
static int x_pair_kind(int Cin, int Cout1, int Cout2) {
  const int cpi = round_up(Cin, 8);
  if (cpi == 128 && Cout1 == 128 && Cout2 >= 1 && Cout2 <= 4) return 1;     // PathNet.final forward: 128 -> 128 -> 3
  if (cpi == 8 && Cout1 == 128 && Cout2 == 128) return 2;                    // its data gradient: 3 -> 128 -> 128
  if (cpi == 64 && Cout1 == 64 && Cout2 == 64) return 3;                     // PathNet.embedding forward: 64 -> 64 -> 64
  return 0;
}

extern "C" int wcmc_conv1x1_pair_supported(int Cin, int Cout1, int Cout2) {
  return x_pair_enabled() && x_pair_kind(Cin, Cout1, Cout2) != 0;
}

extern "C" int wcmc_conv1x1_pair_bf16x3(const void* x_split, int N, int H, int W, int Cin, const void* wp1,
                                        const float* bias1, int Cout1, int act1, float slope1, void* y1_split,
                                        void* mask1, const void* gate_mask1, int gate_act1, float gate_slope1,
                                        float* colsum1, const void* wp2, const float* bias2, int Cout2, int act2,
                                        float slope2, float* y2, int64_t y2sn, int64_t y2sh, int64_t y2sw, void* stream) {
  WCMC_REQUIRE(N > 0 && H > 0 && W > 0 && x_split && wp1 && wp2 && y1_split && y2, WCMC_ERR_BAD_ARG,
               "conv1x1_pair_bf16x3: bad argument");
  const int kind = x_pair_enabled() ? x_pair_kind(Cin, Cout1, Cout2) : 0;
  WCMC_REQUIRE(kind != 0, WCMC_ERR_BAD_ARG, "conv1x1_pair_bf16x3: no fused instance for %d -> %d -> %d channels", Cin,
               Cout1, Cout2);
  WCMC_REQUIRE(aligned16(x_split) && aligned16(wp1) && aligned16(wp2) && aligned16(y1_split), WCMC_ERR_ALIGNMENT,
               "conv1x1_pair_bf16x3: split buffers must be 16-byte aligned");
  WCMC_REQUIRE(nhwc_view_ok(y2, y2sn, y2sh, y2sw, Cout2), WCMC_ERR_ALIGNMENT, "conv1x1_pair_bf16x3: y2 violates the NHWC-view contract");
  XIgemmParams p;
  p.x = (const u16*)x_split; p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cpi = round_up(Cin, 8);
  p.wp = (const u16*)wp1; p.bias = bias1;
  p.yf = nullptr; p.ysn = p.ysh = p.ysw = 0;
  p.ys = (u16*)y1_split; p.Cpo = round_up(Cout1, 8);
  p.Ho = H; p.Wo = W; p.Cout = Cout1;
  p.gate = nullptr; p.gate_act = gate_act1; p.gate_slope = gate_slope1; p.gate_mask = (const unsigned char*)gate_mask1;
  p.mask_out = (unsigned char*)mask1;
  p.ks = 1; p.pad = 0; p.act = act1; p.slope = slope1;
  p.Kp = p.Cpi; p.Kt = round_up(p.Cpi, 32); p.Np = round_up(Cout1, 16);
  p.CS = p.Kp; p.nslabs = 1; p.SPS = p.Kt / 32; p.PXS = 0; p.CSl = p.CS; p.SPSl = p.SPS; p.ap = 2; p.wplanes = 2; p.f16 = 0;
  p.tilesY = p.tilesX = 0; p.G = x_colsum_rows(N, H, W); p.colsum = colsum1;
  p.M = (int64_t)N * H * W;
  const int cp2 = round_up(Cout2, 4);
  const int64_t xb = p.M * 4 * p.Cpi, yb = p.M * 4 * p.Np;
  const int64_t y2b = ((int64_t)(N - 1) * y2sn + (int64_t)(H - 1) * y2sh + (int64_t)(W - 1) * y2sw + cp2) * 4;
  WCMC_REQUIRE(xb < 0x7ff00000LL && yb < 0x7ff00000LL && y2b < 0x7ff00000LL && y2sn >= 0 && y2sh >= 0 && y2sw >= cp2,
               WCMC_ERR_BAD_ARG, "conv1x1_pair_bf16x3: operand larger than 2 GiB (split the batch)");
  p.x_bytes = (unsigned)xb; p.wp_bytes = (unsigned)((size_t)p.Np * 2 * p.Kt * sizeof(u16));
  p.y_bytes = (unsigned)yb; p.m_bytes = (unsigned)(p.M * (p.Np / 8));
  p.wp2 = (const u16*)wp2; p.bias2 = bias2; p.y2 = y2; p.y2sn = y2sn; p.y2sh = y2sh; p.y2sw = y2sw;
  p.Cout2 = Cout2; p.act2 = act2; p.slope2 = slope2; p.Kt2 = p.Np;
  p.wp2_bytes = (unsigned)((size_t)round_up(Cout2, 16) * 2 * p.Kt2 * sizeof(u16)); p.y2_bytes = (unsigned)y2b;
  hipStream_t st = (hipStream_t)stream;
  return launch_xpw_pair(kind, p, st);
}

extern "C" size_t wcmc_conv2d_igemm_colsum_elems(int N, int Ho, int Wo, int Cout) {
  if (N <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0) return 0;
  return (size_t)x_colsum_rows(N, Ho, Wo) * round_up(Cout, 16) + 4;      // + trailer: rows the producing launch wrote
}

extern "C" int wcmc_colsum_finish(const float* partial, int N, int Ho, int Wo, int Cout, float* db, void* stream) {
  WCMC_REQUIRE(partial && db && N > 0 && Ho > 0 && Wo > 0 && Cout > 0, WCMC_ERR_BAD_ARG, "colsum_finish: bad argument");
  const int G = x_colsum_rows(N, Ho, Wo), Np = round_up(Cout, 16);
  // partial rows are Np wide: reduce the first Cout columns of each
  hipLaunchKernelGGL(colsum_final_strided_kernel, dim3((unsigned)((Cout + 63) / 64)), dim3(1024), 0,
                     (hipStream_t)stream, partial, G, Np, Cout, db);
  return check_launch("colsum_finish");
}

extern "C" size_t wcmc_conv2d_wgrad_bf16x3_workspace_bytes(int N, int Ho, int Wo, int Cout, int Cin, int ks) {
  if (N <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0 || Cin <= 0 || ks <= 0) return 0;
  const size_t b3 = x_plan_wgrad(N, Ho, Wo, Cout, Cin, ks, 3).bytes, b1 = x_plan_wgrad(N, Ho, Wo, Cout, Cin, ks, 1).bytes;
  return b3 > b1 ? b3 : b1;                              // (enough for either number of terms)
}

// The scalar half of wcmc_conv2d_wgrad_bf16x3's argument checks, the plan and every field of p that follows from the shape
// (shared with the launch-plan query; the pointers are the entry's).
static int x_wgrad_shape(XWgradParams& p, XWgradPlan& pl, const char* who, int N, int H, int W, int Cin, int Cout, int ks, int pad, int terms) {
  WCMC_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && ks > 0 && pad >= 0, WCMC_ERR_BAD_ARG, "%s: bad argument", who);
  WCMC_REQUIRE(terms == 3 || terms == 1, WCMC_ERR_BAD_ARG, "%s: terms must be 3 (hi*hi + hi*lo + lo*hi) or 1 (the hi planes only)", who);
  const int Ho = H + 2 * pad - ks + 1, Wo = W + 2 * pad - ks + 1;
  WCMC_REQUIRE(Ho > 0 && Wo > 0, WCMC_ERR_BAD_ARG, "%s: empty output", who);
  pl = x_plan_wgrad(N, Ho, Wo, Cout, Cin, ks, terms);
  p = XWgradParams{};
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cpi = round_up(Cin, 8);
  p.Ho = Ho; p.Wo = Wo; p.Cout = Cout; p.Cpo = round_up(Cout, 8);
  p.ks = ks; p.pad = pad; p.S = pl.S; p.M = (int64_t)N * Ho * Wo;
  p.pix_per_split = pl.pix_per_split; p.Np = pl.Np; p.Cq = pl.Cq; p.coBlocks = pl.coBlocks; p.ciBlocks = pl.ciBlocks;
  const size_t xb = wcmc_split_elems(N, H, W, Cin) * sizeof(u16), yb = wcmc_split_elems(N, Ho, Wo, Cout) * sizeof(u16);
  WCMC_REQUIRE(xb < 0x7ff00000u && yb < 0x7ff00000u, WCMC_ERR_BAD_ARG, "%s: operand larger than 2 GiB (split the batch)", who);
  p.x_bytes = (unsigned)xb; p.dy_bytes = (unsigned)yb;
  p.xps = 4 * p.Cpi; p.yps = 4 * p.Cpo;
  return 0;
}

// The GEMM launch of wcmc_conv2d_wgrad_bf16x3 (phases 0 and 1): "conv_wgrad_rows" is the 5x5 filter-row kernel of seven by seven
// channel tiles (either wave count), "conv_wgrad" every other kernel.
extern "C" int wcmc_conv2d_wgrad_launch_plan_bf16x3(int N, int H, int W, int Cin, int Cout, int ks, int pad, int terms,
                                                    char* cls, char* kernel, size_t len) {
  const char* who = "conv2d_wgrad_launch_plan_bf16x3";
  WCMC_REQUIRE(cls && kernel && len > 0, WCMC_ERR_BAD_ARG, "%s: bad argument", who);
  XWgradParams p;
  XWgradPlan pl;
  if (const int rc = x_wgrad_shape(p, pl, who, N, H, W, Cin, Cout, ks, pad, terms)) return rc;
  const XWRowsPlan r = x_plan_wgrad_rows(ks, pl.rTM, pl.rNW, terms == 1 ? 1 : 2);
  const int cn = snprintf(cls, len, "%s", (pl.rows && ks == 5 && pl.rTM == 7 && pl.rNW == 7) ? "conv_wgrad_rows" : "conv_wgrad");
  const int kn = pl.rows && r.rows8 ? snprintf(kernel, len, "conv_wgrad_rows8_bf16x3_kernel<0, %d, %d>", r.xe, r.pl)
                 : pl.rows ? snprintf(kernel, len, "conv_wgrad_rows_bf16x3_kernel<%d, %d, %d, 0, %d>", r.ks, r.tm, r.nw, r.pl)
                           : snprintf(kernel, len, "conv_wgrad_bf16x3_kernel<%d, %d>", pl.TM, r.pl);
  WCMC_REQUIRE((size_t)(cn > kn ? cn : kn) < len, WCMC_ERR_BAD_ARG, "%s: buffers of %zu bytes are too short", who, len);
  return 0;
}

extern "C" int wcmc_conv2d_wgrad_bf16x3(const void* x_split, int N, int H, int W, int Cin, const void* dy_split,
                                        int Cout, int ks, int pad, float* dw, float* db, void* workspace,
                                        size_t workspace_bytes, int phase, const float* dy_colsum_partial, int terms,
                                        void* stream) {
  const char* who = "conv2d_wgrad_bf16x3";
  WCMC_REQUIRE(dw && workspace && x_split && dy_split, WCMC_ERR_BAD_ARG, "%s: bad argument", who);
  XWgradParams p;
  XWgradPlan pl;
  if (const int rc = x_wgrad_shape(p, pl, who, N, H, W, Cin, Cout, ks, pad, terms)) return rc;
  const int Ho = p.Ho, Wo = p.Wo;
  WCMC_REQUIRE(aligned16(x_split) && aligned16(dy_split), WCMC_ERR_ALIGNMENT,
               "conv2d_wgrad_bf16x3: split buffers must be 16-byte aligned");
  WCMC_REQUIRE(workspace_bytes >= pl.bytes && aligned16(workspace), WCMC_ERR_WORKSPACE,
               "conv2d_wgrad_bf16x3: workspace %zu < %zu bytes (or unaligned)", workspace_bytes, pl.bytes);
  WCMC_REQUIRE(phase >= 0 && phase <= 2, WCMC_ERR_BAD_ARG, "conv2d_wgrad_bf16x3: phase must be 0, 1 or 2");
  hipStream_t st = (hipStream_t)stream;
  p.x = (const u16*)x_split; p.dy = (const u16*)dy_split; p.slabs = (float*)workspace;
  int rc = 0;
  if (phase != 2 && pl.rows) {
    XWRowsParams q;
    q.x = p.x; q.N = N; q.H = H; q.W = W; q.Cpi = p.Cpi; q.dy = p.dy; q.Ho = Ho; q.Wo = Wo; q.Cpo = p.Cpo;
    q.dbg = (float*)workspace + pl.slab_elems;
    { const char* e = ab_env("WCMC_WGRAD_ROWS8_PRIO"); q.prio = e ? atoi(e) : 8; if (q.prio < 0 || q.prio > 13) q.prio = 0; }   // (scripts/time_wgrad_rows8.py: 6-8 of 14 best)
    q.pad = pad; q.slabs = p.slabs; q.S = pl.S; q.rps = pl.rps; q.R = pl.R; q.Np = pl.Np; q.Cq = pl.Cq;
    q.coBlocks = pl.coBlocks; q.ciBlocks = pl.ciBlocks; q.x_bytes = p.x_bytes; q.dy_bytes = p.dy_bytes;
    q.xps = p.xps; q.yps = p.yps;
    rc = launch_xwgrad_rows(x_plan_wgrad_rows(ks, pl.rTM, pl.rNW, terms == 1 ? 1 : 2), q, st);
  } else if (phase != 2) {
    rc = launch_xwgrad(pl.TM, terms == 1 ? 1 : 2, p, st);
  }
  if (rc || phase == 1) return rc;
  // the slab reduction; with the column sums of dy at hand its launch also finishes the bias gradient (extra grid rows)
  const bool fuse_db = db && dy_colsum_partial;
  const int cs_rows = fuse_db ? (Cout + 63) / 64 : 0;
  size_t red_lds = (size_t)WR_CI * (ks * ks + 1) * sizeof(float) + 256 * sizeof(float);   // (+ the group sums of the few-tap path)
  if (fuse_db && red_lds < (size_t)16 * 64 * sizeof(float)) red_lds = (size_t)16 * 64 * sizeof(float);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((Cin + WR_CI - 1) / WR_CI), (unsigned)(Cout + cs_rows)), dim3(256),
                     red_lds, st, p.slabs, dw, pl.S, ks * ks, Cout, Cin, pl.Np, pl.Cq, fuse_db ? dy_colsum_partial : nullptr,
                     x_colsum_rows(N, Ho, Wo), round_up(Cout, 16), db);
  rc = check_launch("conv2d_wgrad_bf16x3_reduce");
  if (rc || !db || fuse_db) return rc;
  float* partial = (float*)workspace + pl.slab_elems;
  WCMC_REQUIRE(p.Cpo / 8 <= 256, WCMC_ERR_BAD_ARG, "conv2d_wgrad_bf16x3: Cout > 2048 unsupported");
  hipLaunchKernelGGL(colsum_split_kernel, dim3((unsigned)pl.G), dim3(256), (size_t)256 * 8 * sizeof(float), st, p.dy,
                     p.Cpo, Cout, p.M, pl.per_block, partial);
  hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)((Cout + 63) / 64)), dim3(1024), 0, st, partial, pl.G, Cout,
                     db);
  return check_launch("conv2d_bias_grad_bf16x3");
}
