// Split-bf16 convolution, weight gradients: one tap per block (conv_wgrad_bf16x3_kernel) and one filter row per block
// (conv_wgrad_rows_bf16x3_kernel, conv_wgrad_rows8_bf16x3_kernel).  Their parameter blocks are in bf16x3_common.h.
#include "bf16x3_common.h"

namespace wcmc {

// ------------------------------------------------------------------ weight gradient
// D[co][ci] (per tap) = sum_pix dy[pix][co] * x[pix+tap][ci]; both operands are read with the
// transposing LDS load (ds_read_b64_tr_b16): the tiles sit in LDS as [pixel][channel] exactly as
// they come from HBM, and a lane receives 4 consecutive PIXELS (= MFMA k) of its channel column.
// Block = 64-pixel stage x (TM*16 couts) x 64 cins; waves: 2 (pixel halves = MFMA k-steps) x 2 (cin halves).
// PMC profile of the first version: 36 % L2 hit rate and 2.7 GB fetched per launch -- the 50 blocks
// that share a pixel range (25 taps x 2 cin blocks) ran on different XCDs at different times.  The
// 1-D grid is therefore remapped so that one XCD runs the (tap, tile) blocks of a pixel split back to
// back (speed only), rows of the LDS tiles are an odd multiple of 32 B and the k -> pixel assignment
// of the transposing reads is {4g..4g+3, 16+4g..16+4g+3} (conflict-free, identical for both operands).
constexpr int xw_stride(int ch) { return ((ch / 16) & 1) ? ch : ch + 16; }   // bf16 elements; bytes = odd * 32

// PL = planes multiplied: 2 = hi + lo of both operands, three MFMAs per product (yl*xh + yh*xl + yh*xh); 1 = the hi planes
// only, ONE MFMA per product (the round-3 precision ladder, profiles/r03_precision_ladder.txt: rounding dy and x to bf16 is
// independent from pixel to pixel and averages out over the pixel sum -- the gradients of the benchmarked step move from
// 1.09e-3 to 1.14e-3 of the fp32 oracle's in relative L2).  Half the stage bytes, half the fragment reads, a third of the MFMAs.
template <int TM, int PL = 2>
__global__ __launch_bounds__(256, 2) void conv_wgrad_bf16x3_kernel(XWgradParams p) {
  constexpr int PK = 64;
  constexpr int YC = TM * 16, XC = 64;
  constexpr int SA = xw_stride(YC), SB = xw_stride(XC);
  constexpr int YV = YC / 8, XV = XC / 8;          // 16-byte vectors per plane per pixel
  constexpr int TOTV = PL * YV + PL * XV;
  constexpr int NV = (TOTV + 3) / 4;               // vectors per thread (4 threads share a pixel)
  extern __shared__ __attribute__((aligned(16))) u16 smem16[];
  u16* Ys = smem16;                        // [PL][PK][SA]
  u16* Xs = smem16 + PL * PK * SA;         // [PL][PK][SB]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (a scalar: wave-uniform tests and LDS-DMA destinations stay scalar code)
  // block -> (split, tap, tile): XCD x (= blockIdx & 7) owns splits s = x, x+8, ...; its consecutive
  // blocks sweep the taps and tiles of one split.
  const int taps = p.ks * p.ks;
  const int per_split = taps * p.coBlocks * p.ciBlocks;
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int s = (local / per_split) * 8 + xcd;
  if (s >= p.S) return;
  const int within = local - (local / per_split) * per_split;
  const int tap = within % taps, tileid = within / taps;
  const int cob = tileid / p.ciBlocks, cib = tileid - cob * p.ciBlocks;
  const int co0 = cob * YC, ci0 = cib * XC;
  const int tdy = tap / p.ks - p.pad, tdx = tap % p.ks - p.pad;
  // waves: 2 (pixel halves = MFMA k-steps) x 2 (cout halves); every wave covers the 4 cin tiles, so a
  // stage costs it 8 + 2*MT transposing fragment loads for 12*MT MFMAs (was 36 for 42).
  constexpr int MT = (TM + 1) / 2;                 // cout tiles per wave (the second half may hold one less)
  const int wk = wave >> 1, wm = wave & 1;
  const int tm_valid = min(MT, max(0, min(TM, (p.Np - co0) / 16) - wm * MT));
  const int tn_valid = min(4, max(0, (p.Cq - ci0) / 16));
  const int64_t pstart = (int64_t)s * p.pix_per_split;
  const int64_t pend = min(p.M, pstart + p.pix_per_split);
  const int nstages = (int)((pend - pstart + PK - 1) / PK);

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, (int)p.dy_bytes, 0x00020000);

  // loader: thread -> pixel tid/4 of the stage, vectors (tid&3) + 4*j; per-vector constant parts
  const int lpx = tid >> 2, lv0 = tid & 3;
  unsigned voff[NV]; int lds_off[NV]; bool isy[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lv0 + 4 * j;
    if (v < PL * YV) {
      const int plane = v >= YV, vec = v - plane * YV;
      const int co = co0 + vec * 8;
      isy[j] = true;
      voff[j] = co < p.Cpo ? (unsigned)((plane * p.Cpo + co) * 2) : XOOB;
      lds_off[j] = (plane * PK + lpx) * SA + vec * 8;
    } else if (v < TOTV) {
      const int u = v - PL * YV;
      const int plane = u >= XV, vec = u - plane * XV;
      const int ci = ci0 + vec * 8;
      isy[j] = false;
      voff[j] = ci < p.Cpi ? (unsigned)((plane * p.Cpi + ci) * 2) : XOOB;
      lds_off[j] = PL * PK * SA + (plane * PK + lpx) * SB + vec * 8;
    } else {                               // (TOTV not a multiple of 4: this thread has one vector less)
      isy[j] = true; voff[j] = XOOB; lds_off[j] = -1;
    }
  }
  int cn, coy, cox; int64_t cp = pstart + lpx;
  {
    const int64_t hw = (int64_t)p.Ho * p.Wo;
    cn = (int)(cp / hw);
    const int r = (int)(cp - (int64_t)cn * hw);
    coy = r / p.Wo; cox = r - coy * p.Wo;
  }
  u32x4 rv[NV];
  auto load_stage = [&]() {
    const bool pv = cp < pend;
    const int iy = coy + tdy, ix = cox + tdx;
    const bool xv = pv && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    const unsigned yb = pv ? (unsigned)((((int64_t)cn * p.Ho + coy) * p.Wo + cox) * p.yps) : XOOB;
    const unsigned xb = xv ? (unsigned)((((int64_t)cn * p.H + iy) * p.W + ix) * p.xps) : XOOB;
#pragma unroll
    for (int j = 0; j < NV; ++j)
      rv[j] = isy[j] ? __builtin_amdgcn_raw_buffer_load_b128(yr, (yb | voff[j]) >= XOOB ? XOOB : yb + voff[j], 0, 0)
                     : __builtin_amdgcn_raw_buffer_load_b128(xr, (xb | voff[j]) >= XOOB ? XOOB : xb + voff[j], 0, 0);
    cp += PK; cox += PK;
    while (cox >= p.Wo) { cox -= p.Wo; if (++coy == p.Ho) { coy = 0; ++cn; } }
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int j = 0; j < NV; ++j)
      if (TOTV % 4 == 0 || lds_off[j] >= 0) *reinterpret_cast<u32x4*>(smem16 + lds_off[j]) = rv[j];
  };

  f32x4 acc[MT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // transposing read: lane (group g = lane>>4, i = lane&15, q = i>>2, pp = i&3) addresses pixel row
  // 4g + q (first read) / 16 + 4g + q (second read) and channels 4pp..4pp+3 of a 16-channel tile;
  // it receives channel i of those 4 pixels.  Both MFMA operands use the same pixel order.
  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const int prow0 = wk * 32 + 4 * g + tq;
  auto tr_read = [&](const u16* base, int stride, int col0, bf16x8& out) {
    const u16* a0 = base + prow0 * stride + col0 + 4 * tp;
    const s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (s16x4 __attribute__((address_space(3)))*)(a0));
    const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (s16x4 __attribute__((address_space(3)))*)(a0 + 16 * stride));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 cat = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
    out = __builtin_bit_cast(bf16x8, cat);
  };

  if (nstages > 0) load_stage();
  for (int st = 0; st < nstages; ++st) {
    __syncthreads();                 // every wave is done reading the previous stage
    store_stage();
    __syncthreads();
    if (st + 1 < nstages) load_stage();
    bf16x8 xh[4], xl[PL == 2 ? 4 : 1], yh[MT], yl[PL == 2 ? MT : 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tr_read(Xs, SB, j * 16, xh[j]);
      if constexpr (PL == 2) tr_read(Xs + PK * SB, SB, j * 16, xl[j]);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      tr_read(Ys, SA, (wm * MT + i) * 16, yh[i]);            // (a tile past TM reads the X region: unused)
      if constexpr (PL == 2) tr_read(Ys + PK * SA, SA, (wm * MT + i) * 16, yl[i]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      if (i < tm_valid) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < tn_valid) {
            if constexpr (PL == 2) {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yl[i], xh[j], acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh[i], xl[j], acc[i][j], 0, 0, 0);
            }
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh[i], xh[j], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- ordered sum of the two k-halves through LDS, then one coalesced slab write
  constexpr int RS = XC + 4;
  float* red = reinterpret_cast<float*>(smem16);         // [YC][RS] floats
  const int fcol = lane & 15, fq = (lane >> 4) * 4;
  for (int h = 0; h < 2; ++h) {
    if (wk == h) {
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (wm * MT + i < TM) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* q = red + ((wm * MT + i) * 16 + fq + r) * RS + j * 16 + fcol;
              *q = (h == 0 ? 0.f : *q) + acc[i][j][r];
            }
        }
      }
    }
    __syncthreads();
  }
  float* slab = p.slabs + ((int64_t)s * taps + tap) * p.Np * p.Cq;
  for (int idx = tid; idx < YC * (XC / 4); idx += 256) {
    const int r = idx / (XC / 4), c = (idx - r * (XC / 4)) * 4;
    if (co0 + r < p.Np && ci0 + c < p.Cq)
      *reinterpret_cast<float4*>(slab + (int64_t)(co0 + r) * p.Cq + ci0 + c) =
          *reinterpret_cast<const float4*>(red + r * RS + c);
  }
}


// ------------------------------------------------------------------ weight gradient, one filter row per block
// The kernel above runs one tap per block: every 64-pixel stage (44 KB of dy and x) feeds 168 MFMAs, i.e.
// 65 B per clock and CU from L2 -- the load path, not the matrix pipe, sets its pace (120-150 TF/s).
// Here a block owns a whole filter ROW (KS taps) of one 112-cout block and keeps all KS x 7 x 7
// accumulator tiles in registers (wave w = cin tile w: KS x 7 tiles = 140 VGPRs at KS = 5): a stage is
// 64 pixels of one output row, dy [64][112] and the x row segment [64 + KS - 1][112] (both planes),
// and feeds 2 x KS x 49 x 3 = 1470 MFMAs -- 8.6 B per clock.  The KS taps read the same x rows at shifted
// pixel offsets (the transposing LDS read addresses pixel rows per lane, so any shift is free), dy
// fragments are shared by all taps.  Stages are filled by LDS-DMA (buffer_load ... lds, no staging
// registers) into two buffers; one barrier per stage of ~3400 MFMA cycles per wave.
// KS = filter size, TM = cout tiles (16) per block, NW = waves = cin tiles per block.
// Transposing LDS reads the compiler does not see as LDS reads.  Behind an LDS-DMA hipcc orders every LDS read it knows of
// with s_waitcnt vmcnt(0) (it cannot tell the stage being filled from the stage being read inside one dynamic array): the
// first version of the kernel below therefore waited for stage st+1 to LAND before it multiplied stage st -- no overlap of
// the fill with the MFMAs at all.  The pair (rows prow, prow + 16 of one 16-channel tile) is issued without a wait;
// xwr_frag() orders it (lgkmcnt) and assembles the MFMA operand -- any register copy the compiler adds sits behind the wait.
struct XwrRaw { u32x2 a, b; };
template <int OFF2>
__device__ __forceinline__ void xwr_tr_issue(unsigned addr, XwrRaw& r) {
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%3" : "=&v"(r.a), "=&v"(r.b) : "v"(addr), "n"(OFF2));
}
__device__ __forceinline__ bf16x8 xwr_cat(const XwrRaw& r) {
  const u32x4 c = {r.a[0], r.a[1], r.b[0], r.b[1]};
  return __builtin_bit_cast(bf16x8, c);
}

template <int OFF1, int OFF2>
__device__ __forceinline__ void xwr_tr_issue_at(unsigned addr, XwrRaw& r) {
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"
               : "=&v"(r.a), "=&v"(r.b) : "v"(addr), "n"(OFF1), "n"(OFF2));
}

// loops whose index must be a constant expression (immediate offsets of the transposing reads: an address that is a register
// plus a constant costs a vector addition per read as a plain unrolled loop, and these kernels are bound by vector issue)
template <class F, int... I>
__device__ __forceinline__ void xstatic_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void xstatic_for(F&& f) { xstatic_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{}); }

// PL: planes multiplied (see conv_wgrad_bf16x3_kernel): 2 = [Yh | Yl | Xh | Xl] stages, three MFMAs per product; 1 = [Yh | Xh], one.
template <int KS, int TM, int NW, int DBG = 0, int PL = 2>
__global__ __launch_bounds__(NW * 64, (NW <= 4 ? 2 : 1)) void conv_wgrad_rows_bf16x3_kernel(XWRowsParams p) {
  constexpr int CHY = TM * 16, CHX = NW * 16, PK = 64, XR = PK + KS - 1;
  constexpr int SY = xwr_stride(CHY), SX = xwr_stride(CHX);
  constexpr int VY = SY / 8, VX = SX / 8;                   // 16-byte vectors per row and plane (with pad)
  constexpr int YV = PK * VY, XV = XR * VX;
  constexpr int NVEC = PL * YV + PL * XV;
  constexpr int NI = (NVEC + NW * 64 - 1) / (NW * 64);      // LDS-DMA instructions per wave and stage
  constexpr int BUF = NI * NW * 64 * 8;                     // u16 per buffer (whole instructions)
  extern __shared__ __attribute__((aligned(16))) u16 smem16[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // unit = (split, cout block, cin block); its KS filter-row blocks run side by side on one XCD
  // (blockIdx & 7) and share the unit's dy rows and x rows in that XCD's L2.  The plan keeps the units of
  // an XCD within its 32 CUs: one round.
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int unit = (local / KS) * 8 + xcd;
  const int upb = p.coBlocks * p.ciBlocks;
  if (unit >= p.S * upb) return;
  const int trow = local % KS;
  const int s = unit / upb, ub = unit - s * upb;
  const int cob = ub / p.ciBlocks, cib = ub - cob * p.ciBlocks;
  const int co0 = cob * CHY, ci0 = cib * CHX;
  const int r0 = s * p.rps, r1 = min(p.R, r0 + p.rps);
  const int nch = (p.Wo + PK - 1) / PK;
  const int nrows = r1 - r0;
  const int nst = nrows * nch;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, (int)p.dy_bytes, 0x00020000);

  // ---- stage fill: the buffer is one linear run of 16-byte vectors [Yh | Yl | Xh | Xl];
  // instruction i of wave w writes vectors (i*NW + w)*64 + lane (lane-linear destination), the per-lane
  // SOURCE picks the pixel / plane / channel; invalid sources use an out-of-range offset and land as zeros.
  // What a lane fetches for instruction i is the same in every stage up to the stage's base address and
  // edge tests: one packed word per instruction -- bits 0..19 byte offset / 2 relative to the stage's first
  // pixel, 20..26 pixel row of the tile, 27 operand (1 = x), 28 never valid (row pad, tail of the buffer).
  // What a lane fetches for instruction i is the same in every stage up to the stage's base address and its edge tests:
  // relv = byte offset relative to the stage's first pixel, rowv = pixel row of the tile (127: never valid -- row pad,
  // tail of the buffer, channel past the tensor).
  unsigned relv[NI]; int rowv[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int v = (i * NW + wave) * 64 + lane;
    unsigned rel = 0; int rw = 127;
    if (v < PL * YV) {
      const int plane = v >= YV, vv = v - plane * YV;
      const int row = vv / VY, vec = vv - row * VY;
      const int co = co0 + vec * 8;
      if (vec * 8 < CHY && co < p.Cpo) { rel = (unsigned)(row * p.yps + plane * 2 * p.Cpo + co * 2); rw = row; }
    } else if (v < NVEC) {
      const int u = v - PL * YV;
      const int plane = u >= XV, uu = u - plane * XV;
      const int row = uu / VX, vec = uu - row * VX;
      const int ci = ci0 + vec * 8;
      if (vec * 8 < CHX && ci < p.Cpi) { rel = (unsigned)(row * p.xps + plane * 2 * p.Cpi + ci * 2); rw = row; }
    }
    relv[i] = rel; rowv[i] = rw;
  }
  // per-stage scalars of the fill (issue_prep) and one DMA instruction of it (issue_one, four vector instructions and no
  // branch): the instructions of stage st+1 are spread over the MFMA stream of stage st (stamps of the first version,
  // which issued them in one burst after the barrier: 1500-1950 of 10500 cycles per stage, the matrix pipe idle)
  unsigned f_ybase = 0, f_xbase = 0, f_yn = 0, f_xn = 0; int f_xlo = 0, f_buf = 0;
  // Row order skewed by the filter row: at step j the KS blocks of a unit read the SAME x row r0 + j and dy rows one
  // step apart -- stage st is chunk st % nch of row r0 + (st / nch - trow) mod nrows.  The stages are prepared in order,
  // so the cursor advances by increments (the divisions of the first version cost 500-850 cycles per stage).
  int f_c = 0, f_rs = nrows > 0 ? (nrows - trow % nrows) % nrows : 0, f_n, f_oy;
  const int f_n0 = r0 / p.Ho, f_oy0 = r0 - f_n0 * p.Ho;
  { const int r = r0 + f_rs; f_n = r / p.Ho; f_oy = r - f_n * p.Ho; }
  auto issue_prep = [&](int buf) {
    const int ox0 = f_c * PK;
    const int iy = f_oy + trow - p.pad;
    const bool rowok = (unsigned)iy < (unsigned)p.H;
    f_ybase = (unsigned)(((f_n * p.Ho + f_oy) * p.Wo + ox0) * p.yps);
    f_xbase = (unsigned)(((f_n * p.H + iy) * p.W + ox0 - p.pad) * p.xps);       // may wrap: only used when valid
    f_yn = (unsigned)max(0, p.Wo - ox0);               // dy rows [0, yn) exist
    f_xlo = p.pad - ox0;                               // x rows [xlo, xlo + xn) are inside the image
    f_xn = rowok ? (unsigned)p.W : 0u;
    f_buf = buf;
    if (++f_c == nch) {                                // the cursor of the following stage
      f_c = 0;
      if (++f_rs == nrows) { f_rs = 0; f_n = f_n0; f_oy = f_oy0; }
      else if (++f_oy == p.Ho) { f_oy = 0; ++f_n; }
    }
  };
  auto issue_one = [&](int i) {
    if ((i + 1) * NW * 64 > NVEC && (i * NW + wave) * 64 >= NVEC) return;   // (the tail of the last instruction row: nothing to fetch)
    // PL*YV is a multiple of 64: a wave-instruction is all dy or all x (wave-uniform choice of descriptor and base)
    const bool isx = (PL * VY) % NW == 0 ? i >= (PL * VY) / NW : (i * NW + wave) * 64 >= PL * YV;
    const unsigned base = isx ? f_xbase : f_ybase, cnt = isx ? f_xn : f_yn;
    const int lo = isx ? f_xlo : 0;
    const unsigned off = (unsigned)(rowv[i] - lo) < cnt ? base + relv[i] : XOOB;
    __attribute__((address_space(3))) void* dst =
        (__attribute__((address_space(3))) void*)(smem16 + f_buf * BUF + (i * NW + wave) * 512);
    if (!isx) __builtin_amdgcn_raw_ptr_buffer_load_lds(yr, dst, 16, off, 0, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, dst, 16, off, 0, 0, 0);
  };
  auto issue = [&](int buf) {
    issue_prep(buf);
#pragma unroll
    for (int i = 0; i < NI; ++i) issue_one(i);
  };

  f32x4 acc[KS][TM];
#pragma unroll
  for (int t = 0; t < KS; ++t)
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // transposing read (see conv_wgrad_bf16x3_kernel): lane addresses pixel row 4g + q (+16) and channels
  // 4pp..4pp+3 of a 16-channel tile and receives channel (lane & 15) of pixels {4g..4g+3, 16+4g..16+4g+3}
  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) u16*)smem16);

  unsigned long long tc0 = 0, tr0 = 0;
  if (DBG & 4) { tc0 = __builtin_amdgcn_s_memtime(); tr0 = __builtin_amdgcn_s_memrealtime(); }
  // DBG & 16 (scripts/timeline_wgrad.py): wall-clock stamps (100 MHz) of entry / loop start / loop end / exit and the
  // shader-clock cycles of the stage loop spent waiting (DMA + barrier), issuing the next stage and multiplying
  unsigned long long rt[4] = {0, 0, 0, 0}, cyc[3] = {0, 0, 0}, tprev = 0;
  auto rts = [&](int i) {
    if (DBG & 16) {
      unsigned long long t;
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      rt[i] = t;
    }
  };
  auto cst = [&](int i) {
    if (DBG & 16) {
      unsigned long long t;
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      if (i >= 0) cyc[i] += t - tprev;
      tprev = t;
    }
  };
  rts(0);
  if (nst > 0) issue(0);
  rts(1);
  cst(-1);
  for (int st = 0; st < nst; ++st) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's share of stage st has landed
    __syncthreads();                                      // ... everyone's; and everyone is done with stage st-1
    cst(0);
    const bool fill = st + 1 < nst && !((DBG & 2) && st > 0);
    cst(1);
    // byte addresses of this lane's first fragment row in the four planes of the stage
    const int prow0 = 4 * g + tq;
    const unsigned aYh = lds0 + (unsigned)(((st & 1) * BUF + prow0 * SY + 4 * tp) * 2);
    const unsigned aXh = lds0 + (unsigned)(((st & 1) * BUF + PL * PK * SY + prow0 * SX + wave * 16 + 4 * tp) * 2);
    const int c = st % nch;
    const int nk = (min(PK, p.Wo - c * PK) + 31) / 32;    // 32-pixel MFMA k-steps with any valid pixel (1 or 2)
    // Software pipeline inside the wave (the first version read a k-step's fragments, waited, multiplied: a wave alone on
    // its SIMD kept the matrix pipe 61 % busy): the x fragments of all KS taps stay in registers for a k-step and are
    // replaced tap by tap during its last cout tile; the dy fragments are double-buffered one cout tile ahead.  The
    // order of the MFMAs on every accumulator is unchanged (bit-identical results).
    XwrRaw rxh[KS], rxl[KS], ryh[2], ryl[2];
    constexpr int XLOB = XR * SX * 2, YLOB = PK * SY * 2;   // lo planes; every read below = aXh / aYh + an immediate
    xstatic_for<KS>([&](auto T_) {
      constexpr int t = decltype(T_)::value;
      xwr_tr_issue_at<t * SX * 2, t * SX * 2 + 16 * SX * 2>(aXh, rxh[t]);
      if constexpr (PL == 2) xwr_tr_issue_at<XLOB + t * SX * 2, XLOB + t * SX * 2 + 16 * SX * 2>(aXh, rxl[t]);
    });
    xwr_tr_issue_at<0, 16 * SY * 2>(aYh, ryh[0]);
    if constexpr (PL == 2) xwr_tr_issue_at<YLOB, YLOB + 16 * SY * 2>(aYh, ryl[0]);
    bf16x8 xh[KS], xl[KS];
    xstatic_for<2>([&](auto K_) {
      constexpr int kk = decltype(K_)::value;
      if (kk < nk) {
        xstatic_for<TM>([&](auto I_) {
          constexpr int i = decltype(I_)::value;
          constexpr int cur = (kk * TM + i) & 1, nxt = cur ^ 1;
          // everything issued so far has landed (the reads of this iteration were issued one iteration ago)
          if constexpr (PL == 1) {                     // (the lo registers do not exist in this instance)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ryh[cur].a), "+v"(ryh[cur].b));
            if (i == 0) {
#pragma unroll
              for (int t = 0; t < KS; ++t) {
                asm volatile("" : "+v"(rxh[t].a), "+v"(rxh[t].b));
                xh[t] = xwr_cat(rxh[t]);
              }
            }
          } else if (DBG & 8) {                        // (timing only: no wait for the fragments)
            asm volatile("" : "+v"(ryh[cur].a), "+v"(ryh[cur].b), "+v"(ryl[cur].a), "+v"(ryl[cur].b));
            if (i == 0) {
#pragma unroll
              for (int t = 0; t < KS; ++t) { xh[t] = xwr_cat(rxh[t]); xl[t] = xwr_cat(rxl[t]); }
            }
          } else if (i == 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ryh[cur].a), "+v"(ryh[cur].b), "+v"(ryl[cur].a), "+v"(ryl[cur].b));
#pragma unroll
            for (int t = 0; t < KS; ++t) {
              asm volatile("" : "+v"(rxh[t].a), "+v"(rxh[t].b), "+v"(rxl[t].a), "+v"(rxl[t].b));
              xh[t] = xwr_cat(rxh[t]); xl[t] = xwr_cat(rxl[t]);
            }
          } else {
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ryh[cur].a), "+v"(ryh[cur].b), "+v"(ryl[cur].a), "+v"(ryl[cur].b));
          }
          bf16x8 yh = xwr_cat(ryh[cur]), yl = yh;
          if constexpr (PL == 2) yl = xwr_cat(ryl[cur]);
          if constexpr (i + 1 < TM) {
            constexpr int O = (kk * 32 * SY + (i + 1) * 16) * 2;
            xwr_tr_issue_at<O, O + 16 * SY * 2>(aYh, ryh[nxt]);
            if constexpr (PL == 2) xwr_tr_issue_at<YLOB + O, YLOB + O + 16 * SY * 2>(aYh, ryl[nxt]);
          } else if (kk + 1 < nk) {
            constexpr int O = (kk + 1) * 32 * SY * 2;
            xwr_tr_issue_at<O, O + 16 * SY * 2>(aYh, ryh[nxt]);
            if constexpr (PL == 2) xwr_tr_issue_at<YLOB + O, YLOB + O + 16 * SY * 2>(aYh, ryl[nxt]);
          }
          __builtin_amdgcn_sched_barrier(0);             // (the prefetch leaves before the MFMAs, not among them)
          xstatic_for<KS>([&](auto T_) {
            constexpr int t = decltype(T_)::value;
            if (DBG & 1) { asm volatile("" ::"v"(yl), "v"(yh), "v"(xh[t]), "v"(xl[t])); }
            else {
              if constexpr (PL == 2) {
                acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yl, xh[t], acc[t][i], 0, 0, 0);
                acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, xl[t], acc[t][i], 0, 0, 0);
              }
              acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, xh[t], acc[t][i], 0, 0, 0);
            }
            if (i == TM - 1 && kk + 1 < nk) {             // this tap's fragments of the next k-step
              constexpr int O = ((kk + 1) * 32 + t) * SX * 2;
              xwr_tr_issue_at<O, O + 16 * SX * 2>(aXh, rxh[t]);
              if constexpr (PL == 2) xwr_tr_issue_at<XLOB + O, XLOB + O + 16 * SX * 2>(aXh, rxl[t]);
            }
          });
          // (the next stage's scalars are worked out behind the first MFMAs of the stage, not at the barrier where all
          // waves of the block would do it at the same moment with the matrix pipe empty)
          if (fill && kk * TM + i == 0) issue_prep((st + 1) & 1);
          if (fill && kk * TM + i < NI) issue_one(kk * TM + i);
          __builtin_amdgcn_sched_barrier(0);
        });
      }
    });
    if (fill) {                                          // what the MFMA stream had no slot for (one k-step, or NI > 2 TM)
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (i >= nk * TM) issue_one(i);
    }
    cst(2);
  }
  rts(2);

  if (DBG & 4) {     // clock probe: shader-clock ticks and 100 MHz ticks over the main loop
    const unsigned long long tc1 = __builtin_amdgcn_s_memtime(), tr1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(p.dbg) + (int64_t)blockIdx.x * 4;
      o[0] = tc1 - tc0; o[1] = tr1 - tr0; o[2] = (unsigned long long)nst;
    }
  }
  // ---- slab write: lane holds D[co = 4*(lane>>4) + r][ci = 16*wave + (lane & 15)] of each tile.  The tile
  // goes through LDS and leaves as whole 16-byte vectors, CHX*4-byte row segments (direct stores are
  // 64-byte fragments of 128-byte lines: 0.4 TB/s measured).
  __syncthreads();
  constexpr int RS = CHX + 4;
  float* red = reinterpret_cast<float*>(smem16);           // [CHY][RS]
  const int fcol = lane & 15, fq = (lane >> 4) * 4;
#pragma unroll
  for (int t = 0; t < KS; ++t) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(i * 16 + fq + r) * RS + wave * 16 + fcol] = acc[t][i][r];
    __syncthreads();
    float* slab = p.slabs + (((int64_t)s * KS * KS + trow * KS + t) * p.Np + co0) * p.Cq + ci0;
    for (int idx = tid; idx < CHY * (CHX / 4); idx += NW * 64) {
      const int row = idx / (CHX / 4), v = idx - row * (CHX / 4);
      if (co0 + row < p.Np && ci0 + v * 4 < p.Cq)
        *reinterpret_cast<float4*>(slab + (int64_t)row * p.Cq + v * 4) = *reinterpret_cast<const float4*>(red + row * RS + v * 4);
    }
    __syncthreads();
  }
  if (DBG & 16) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    rts(3);
    if (lane == 0) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(p.dbg) + ((int64_t)blockIdx.x * NW + wave) * 8;
      for (int i = 0; i < 4; ++i) o[i] = rt[i];
      for (int i = 0; i < 3; ++i) o[4 + i] = cyc[i];
      o[7] = (unsigned long long)nst;
    }
  }
}

// The KPCN instance (5x5, 7 x 7 channel tiles) of the filter-row kernel on EIGHT waves.  conv_wgrad_rows_bf16x3_kernel
// <5, 7, 7> gives wave w the input-channel tile w: seven waves on four SIMDs, 105 MFMAs per wave and k-step -- three SIMDs
// carry two waves (210 MFMAs per k-step), the fourth one (scripts/timeline_wgrad.py: waves 0-3 wait 3100 of 9060 cycles
// per stage for waves 4-6).  Here the 245 accumulator tiles (5 taps x 7 cin tiles x 7 cout tiles) are dealt evenly:
// (tap, cin tile) pair q = 7 tap + ci, wave w owns pairs 4w .. 4w+3 with all seven cout tiles (28 tiles) and, of the
// three pairs left over (tap 4, cin tiles 4..6), the cout tile w (wave 7 multiplies wave 0's again and drops it: no
// branch in the MFMA stream) -- 93 MFMAs per wave and k-step, 186 per SIMD.  Stage layout, fill, slab layout and the
// order of the MFMAs on every accumulator are those of the seven-wave kernel: the slabs are bit-identical.
template <int DBG = 0, int XE = 1, int PL = 2>
__global__ __launch_bounds__(512, 1) void conv_wgrad_rows8_bf16x3_kernel(XWRowsParams p) {
#define XWR8_READ(O1, O2, ADDR, REG) do { if (DBG & 32) { asm volatile("" : "+v"((REG).a), "+v"((REG).b)); } else xwr_tr_issue_at<O1, O2>(ADDR, REG); } while (0)
  constexpr int KS = 5, TM = 7, NCI = 7, NW = 8, NS = 4, NE = 3;
  constexpr int CHY = TM * 16, CHX = NCI * 16, PK = 64, XR = PK + KS - 1;
  constexpr int SY = xwr_stride(CHY), SX = xwr_stride(CHX);
  constexpr int VY = SY / 8, VX = SX / 8;
  constexpr int YV = PK * VY, XV = XR * VX;
  constexpr int NVEC = PL * YV + PL * XV;                   // PL = 1: [Yh | Xh] stages, one MFMA per product (see conv_wgrad_bf16x3_kernel)
  constexpr int NI = (NVEC + NW * 64 - 1) / (NW * 64);
  constexpr int BUF = NI * NW * 64 * 8;
  constexpr int XLO = XR * SX * 2;                          // byte offset of the lo plane of x (and below: of dy)
  constexpr int YLO = PK * SY * 2;
  extern __shared__ __attribute__((aligned(16))) u16 smem16[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int unit = (local / KS) * 8 + xcd;
  const int upb = p.coBlocks * p.ciBlocks;
  if (unit >= p.S * upb) return;
  const int trow = local % KS;
  const int s = unit / upb, ub = unit - s * upb;
  const int cob = ub / p.ciBlocks, cib = ub - cob * p.ciBlocks;
  const int co0 = cob * CHY, ci0 = cib * CHX;
  const int r0 = s * p.rps, r1 = min(p.R, r0 + p.rps);
  const int nch = (p.Wo + PK - 1) / PK;
  const int nrows = r1 - r0;
  const int nst = nrows * nch;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, (int)p.dy_bytes, 0x00020000);

  // ---- stage fill: as conv_wgrad_rows_bf16x3_kernel (one linear run of 16-byte vectors [Yh | Yl | Xh | Xl])
  unsigned relv[NI]; int rowv[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int v = (i * NW + wave) * 64 + lane;
    unsigned rel = 0; int rw = 127;
    if (v < PL * YV) {
      const int plane = v >= YV, vv = v - plane * YV;
      const int row = vv / VY, vec = vv - row * VY;
      const int co = co0 + vec * 8;
      if (vec * 8 < CHY && co < p.Cpo) { rel = (unsigned)(row * p.yps + plane * 2 * p.Cpo + co * 2); rw = row; }
    } else if (v < NVEC) {
      const int u = v - PL * YV;
      const int plane = u >= XV, uu = u - plane * XV;
      const int row = uu / VX, vec = uu - row * VX;
      const int ci = ci0 + vec * 8;
      if (vec * 8 < CHX && ci < p.Cpi) { rel = (unsigned)(row * p.xps + plane * 2 * p.Cpi + ci * 2); rw = row; }
    }
    relv[i] = rel; rowv[i] = rw;
  }
  unsigned f_ybase = 0, f_xbase = 0, f_yn = 0, f_xn = 0; int f_xlo = 0, f_buf = 0;
  int f_c = 0, f_rs = nrows > 0 ? (nrows - trow % nrows) % nrows : 0, f_n, f_oy;
  const int f_n0 = r0 / p.Ho, f_oy0 = r0 - f_n0 * p.Ho;
  { const int r = r0 + f_rs; f_n = r / p.Ho; f_oy = r - f_n * p.Ho; }
  auto issue_prep = [&](int buf) {
    const int ox0 = f_c * PK;
    const int iy = f_oy + trow - p.pad;
    const bool rowok = (unsigned)iy < (unsigned)p.H;
    f_ybase = (unsigned)(((f_n * p.Ho + f_oy) * p.Wo + ox0) * p.yps);
    f_xbase = (unsigned)(((f_n * p.H + iy) * p.W + ox0 - p.pad) * p.xps);       // may wrap: only used when valid
    f_yn = (unsigned)max(0, p.Wo - ox0);
    f_xlo = p.pad - ox0;
    f_xn = rowok ? (unsigned)p.W : 0u;
    f_buf = buf;
    if (++f_c == nch) {
      f_c = 0;
      if (++f_rs == nrows) { f_rs = 0; f_n = f_n0; f_oy = f_oy0; }
      else if (++f_oy == p.Ho) { f_oy = 0; ++f_n; }
    }
  };
  auto issue_one = [&](int i) {
    // the last instruction row is mostly past the stage's 3696 vectors: six of the eight waves have nothing to fetch there
    // (an LDS-DMA instruction holds the SIMD's vector issue for 60-100 cycles whether or not its lanes are in range)
    if ((i + 1) * NW * 64 > NVEC && (i * NW + wave) * 64 >= NVEC) return;
    // 2*YV is a multiple of 64: a wave-instruction is all dy or all x; only one instruction row straddles the two (written
    // out so that the others are compile-time choices and not wave-uniform masks kept in spilled scalar registers)
    const bool isx = (i * NW + NW - 1) * 64 < PL * YV ? false : i * NW * 64 >= PL * YV ? true : (i * NW + wave) * 64 >= PL * YV;
    const unsigned base = isx ? f_xbase : f_ybase, cnt = isx ? f_xn : f_yn;
    const int lo = isx ? f_xlo : 0;
    const unsigned off = (unsigned)(rowv[i] - lo) < cnt ? base + relv[i] : XOOB;
    __attribute__((address_space(3))) void* dst =
        (__attribute__((address_space(3))) void*)(smem16 + f_buf * BUF + (i * NW + wave) * 512);
    if (!isx) __builtin_amdgcn_raw_ptr_buffer_load_lds(yr, dst, 16, off, 0, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, dst, 16, off, 0, 0, 0);
  };

  // this wave's pairs: byte offset of the pair's fragment column (tap row + cin tile) inside an x plane, and the
  // cout tile of loop slot i (rotated by the wave: slot 0 is the tile of the wave's three extra accumulators)
  int xoff[NS], ycol[TM];
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    const int pr = NS * wave + q, pt = pr / NCI, pc = pr - pt * NCI;
    xoff[q] = (pt * SX + pc * 16) * 2;
  }
  // XE = 1 (shipped; WCMC_WGRAD_ROWS8_XE=0 for the A/B): the 21 left-over tiles are dealt as ONE pair per wave x 2..4
  // consecutive cout tiles -- pair 32: waves 0-2 (cout tiles {0,1}, {2,3}, {4,5,6}), pair 33: waves 3-5 alike, pair 34: waves
  // 6, 7 ({0,1,2}, {3,4,5,6}); 4 / 5 / 6 / 6 extra tiles per SIMD (waves w, w + 4) -- so that a wave reads ONE extra x
  // fragment per k-step instead of three (48 instead of 56 transposing reads per 90-96 MFMAs; the kernel is bound by the
  // issue of its non-MFMA instructions: profiles/HISTORY.md 6.1).  The extras sit in loop slots 0 .. nex-1 (slots 2, 3 behind a
  // wave-uniform test); XE = 0: three pairs x cout tile `wave` in slot 0, wave 7 multiplies wave 0's again and drops them.
  const int er = wave % 3;
  const int epair = XE ? (wave < 6 ? wave / 3 : 2) : 0;
  const int ebase = XE ? (wave < 6 ? 2 * er : wave == 6 ? 0 : 3) : wave;
  const int nex = XE ? (wave < 6 ? (er == 2 ? 3 : 2) : wave == 6 ? 3 : 4) : 1;
#pragma unroll
  for (int i = 0; i < TM; ++i) ycol[i] = (ebase + i) % TM;
  constexpr int ETAP = KS - 1, ECI0 = NCI - NE;              // the left-over pairs: tap 4, cin tiles 4..6
  constexpr int NA = XE ? 4 : NE, NF = XE ? 1 : NE;          // extra accumulators / extra x fragments per wave
  const int exoff = (ETAP * SX + (ECI0 + epair) * 16) * 2;   // (XE) byte offset of the wave's extra pair inside an x plane

  f32x4 acc[NS][TM], ace[NA];
#pragma unroll
  for (int q = 0; q < NS; ++q)
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[q][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < NA; ++e) ace[e] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) u16*)smem16);

  unsigned long long rt[4] = {0, 0, 0, 0}, cyc[3] = {0, 0, 0}, tprev = 0;
  auto rts = [&](int i) {
    if (DBG & 16) {
      unsigned long long t;
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      rt[i] = t;
    }
  };
  auto cst = [&](int i) {
    if (DBG & 16) {
      unsigned long long t;
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      if (i >= 0) cyc[i] += t - tprev;
      tprev = t;
    }
  };
  rts(0);
  if (nst > 0) {
    issue_prep(0);
#pragma unroll
    for (int i = 0; i < NI; ++i) issue_one(i);
  }
  rts(1);
  cst(-1);
  // The stage loop is unrolled by two so that the buffer of a stage is a compile-time choice: this lane's fragment
  // addresses in either buffer (7 dy cout tiles, 4 + 1 x slots) are worked out ONCE and every transposing read is an
  // address register plus an immediate -- the loop had ~30 address additions per stage and wave, and it is bound by the
  // issue of exactly such instructions (profiles/HISTORY.md 6.1).
  unsigned ayv[2][TM], axv[2][NS], aEv[2], aXv[2];
  {
    const int prow0 = 4 * g + tq;
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      const unsigned by = lds0 + (unsigned)((bb * BUF + prow0 * SY + 4 * tp) * 2);
      const unsigned bx = lds0 + (unsigned)((bb * BUF + PL * PK * SY + prow0 * SX + 4 * tp) * 2);
#pragma unroll
      for (int i = 0; i < TM; ++i) { ayv[bb][i] = by + (unsigned)(ycol[i] * 32); asm volatile("" : "+v"(ayv[bb][i])); }
#pragma unroll
      for (int q = 0; q < NS; ++q) { axv[bb][q] = bx + (unsigned)xoff[q]; asm volatile("" : "+v"(axv[bb][q])); }
      aEv[bb] = bx + (unsigned)exoff; asm volatile("" : "+v"(aEv[bb]));
      aXv[bb] = bx; asm volatile("" : "+v"(aXv[bb]));
    }
  }
  auto stage = [&](const int st, auto PAR) __attribute__((always_inline)) {
    constexpr int par = decltype(PAR)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cst(0);
    const bool fill = st + 1 < nst && !((DBG & 2) && st > 0);   // (DBG: timing-only ablations, wrong results -- 1 no MFMA, 2 no fills after the first, 8 no fragment waits, 32 no fragment reads)
    cst(1);
    // Two waves share a SIMD (w and w + 4) and of two ready waves the older one issues: waves 0-3 ran ahead and then
    // waited ~2800 of 8200 cycles per stage at the barrier while waves 4-7 finished alone, a lone wave keeping the matrix
    // pipe ~60 % busy against ~86 % for a pair (scripts/timeline_wgrad.py).  Waves 0-3 take priority 2 for the first
    // p.prio iterations of the stage and 0 afterwards, waves 4-7 stay at 1: both reach the barrier together.
    if (p.prio) { if (wave < 4) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(1); }
    const unsigned aX = aXv[par];
    const unsigned (&ax)[NS] = axv[par];
    const unsigned (&ayp)[TM] = ayv[par];
    const int c = st % nch;
    const int nk = (min(PK, p.Wo - c * PK) + 31) / 32;
    XwrRaw rxh[NS], rxl[NS], reh[NF], rel_[NF], ryh[2], ryl[2];
    const unsigned aE = aEv[par];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      XWR8_READ(0, 16 * SX * 2, ax[q], rxh[q]);
      if constexpr (PL == 2) XWR8_READ(XLO, XLO + 16 * SX * 2, ax[q], rxl[q]);
    }
    if (XE) {
      XWR8_READ(0, 16 * SX * 2, aE, reh[0]);
      if constexpr (PL == 2) XWR8_READ(XLO, XLO + 16 * SX * 2, aE, rel_[0]);
    } else {
#pragma unroll
      for (int e = 0; e < NF; ++e) {
        XWR8_READ(0, 16 * SX * 2, aX + (unsigned)((ETAP * SX + (ECI0 + e) * 16) * 2), reh[e]);
        if constexpr (PL == 2) XWR8_READ(XLO, XLO + 16 * SX * 2, aX + (unsigned)((ETAP * SX + (ECI0 + e) * 16) * 2), rel_[e]);
      }
    }
    XWR8_READ(0, 16 * SY * 2, ayp[0], ryh[0]);
    if constexpr (PL == 2) XWR8_READ(YLO, YLO + 16 * SY * 2, ayp[0], ryl[0]);
    bf16x8 xh[NS], xl[NS], eh[NF], el[NF];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (kk < nk) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int cur = (kk * TM + i) & 1, nxt = cur ^ 1;
          if (kk * TM + i > 0 && p.prio == kk * TM + i && wave < 4) __builtin_amdgcn_s_setprio(0);
          if constexpr (PL == 1) {                        // (the lo registers do not exist in this instance)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ryh[cur].a), "+v"(ryh[cur].b));
            if (i == 0) {
#pragma unroll
              for (int q = 0; q < NS; ++q) { asm volatile("" : "+v"(rxh[q].a), "+v"(rxh[q].b)); xh[q] = xwr_cat(rxh[q]); }
#pragma unroll
              for (int e = 0; e < NF; ++e) { asm volatile("" : "+v"(reh[e].a), "+v"(reh[e].b)); eh[e] = xwr_cat(reh[e]); }
            }
          } else {
          if (DBG & 8) { asm volatile("" : "+v"(ryh[cur].a), "+v"(ryh[cur].b), "+v"(ryl[cur].a), "+v"(ryl[cur].b)); }
          else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ryh[cur].a), "+v"(ryh[cur].b), "+v"(ryl[cur].a), "+v"(ryl[cur].b));
          if (i == 0) {
#pragma unroll
            for (int q = 0; q < NS; ++q) {
              asm volatile("" : "+v"(rxh[q].a), "+v"(rxh[q].b), "+v"(rxl[q].a), "+v"(rxl[q].b));
              xh[q] = xwr_cat(rxh[q]); xl[q] = xwr_cat(rxl[q]);
            }
#pragma unroll
            for (int e = 0; e < NF; ++e) {
              asm volatile("" : "+v"(reh[e].a), "+v"(reh[e].b), "+v"(rel_[e].a), "+v"(rel_[e].b));
              eh[e] = xwr_cat(reh[e]); el[e] = xwr_cat(rel_[e]);
            }
          }
          }
          bf16x8 yh = xwr_cat(ryh[cur]), yl = yh;
          if constexpr (PL == 2) yl = xwr_cat(ryl[cur]);
          constexpr int KY = 32 * SY * 2;                 // the second k-step of the dy planes
          if (i + 1 < TM) {
            if (kk == 0) {
              XWR8_READ(0, 16 * SY * 2, ayp[i + 1 < TM ? i + 1 : 0], ryh[nxt]);
              if constexpr (PL == 2) XWR8_READ(YLO, YLO + 16 * SY * 2, ayp[i + 1 < TM ? i + 1 : 0], ryl[nxt]);
            } else {
              XWR8_READ(KY, KY + 16 * SY * 2, ayp[i + 1 < TM ? i + 1 : 0], ryh[nxt]);
              if constexpr (PL == 2) XWR8_READ(KY + YLO, KY + YLO + 16 * SY * 2, ayp[i + 1 < TM ? i + 1 : 0], ryl[nxt]);
            }
          } else if (kk + 1 < nk) {
            XWR8_READ(KY, KY + 16 * SY * 2, ayp[0], ryh[nxt]);
            if constexpr (PL == 2) XWR8_READ(KY + YLO, KY + YLO + 16 * SY * 2, ayp[0], ryl[nxt]);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (XE) {                                       // the left-over pair of this wave: cout tiles ycol[0 .. nex-1]
            if (i < 4) {
              if (i < 2 || i < nex) {
                if (DBG & 1) { asm volatile("" ::"v"(yl), "v"(yh), "v"(eh[0]), "v"(el[0])); }
                else {
                  if constexpr (PL == 2) {
                    ace[i < NA ? i : 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yl, eh[0], ace[i < NA ? i : 0], 0, 0, 0);
                    ace[i < NA ? i : 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, el[0], ace[i < NA ? i : 0], 0, 0, 0);
                  }
                  ace[i < NA ? i : 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, eh[0], ace[i < NA ? i : 0], 0, 0, 0);
                }
              }
              if (i == 3 && kk + 1 < nk) {
                constexpr int K1 = 32 * SX * 2;
                XWR8_READ(K1, K1 + 16 * SX * 2, aE, reh[0]);
                if constexpr (PL == 2) XWR8_READ(K1 + XLO, K1 + XLO + 16 * SX * 2, aE, rel_[0]);
              }
            }
          } else if (i == 0) {                            // the left-over pairs: cout tile ycol[0] = wave
#pragma unroll
            for (int e = 0; e < NF; ++e) {
              if (DBG & 1) { asm volatile("" ::"v"(yl), "v"(yh), "v"(eh[e]), "v"(el[e])); }
              else {
                if constexpr (PL == 2) {
                  ace[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yl, eh[e], ace[e], 0, 0, 0);
                  ace[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, el[e], ace[e], 0, 0, 0);
                }
                ace[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, eh[e], ace[e], 0, 0, 0);
              }
              if (kk + 1 < nk) {
                const unsigned ae = aX + (unsigned)((((kk + 1) * 32 + ETAP) * SX + (ECI0 + e) * 16) * 2);
                XWR8_READ(0, 16 * SX * 2, ae, reh[e]);
                if constexpr (PL == 2) XWR8_READ(XLO, XLO + 16 * SX * 2, ae, rel_[e]);
              }
            }
          }
#pragma unroll
          for (int q = 0; q < NS; ++q) {
            if (DBG & 1) { asm volatile("" ::"v"(yl), "v"(yh), "v"(xh[q]), "v"(xl[q])); }
            else {
              if constexpr (PL == 2) {
                acc[q][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yl, xh[q], acc[q][i], 0, 0, 0);
                acc[q][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, xl[q], acc[q][i], 0, 0, 0);
              }
              acc[q][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, xh[q], acc[q][i], 0, 0, 0);
            }
            if (i == TM - 1 && kk + 1 < nk) {
              constexpr int K1 = 32 * SX * 2;              // (kk + 1 < nk <= 2: the second k-step)
              XWR8_READ(K1, K1 + 16 * SX * 2, ax[q], rxh[q]);
              if constexpr (PL == 2) XWR8_READ(K1 + XLO, K1 + XLO + 16 * SX * 2, ax[q], rxl[q]);
            }
          }
          // (the next stage's scalars are worked out here, behind the first MFMAs of the stage, not at the barrier where
          // both waves of every SIMD would do it at the same moment with the matrix pipe empty)
          if (fill && kk * TM + i == 0) issue_prep(par ^ 1);
          if (fill && kk * TM + i < NI) issue_one(kk * TM + i);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (fill) {
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (i >= nk * TM) issue_one(i);
    }
    cst(2);
  };
  for (int st = 0; st < nst; st += 2) {
    stage(st, std::integral_constant<int, 0>{});
    if (st + 1 < nst) stage(st + 1, std::integral_constant<int, 1>{});
  }
  rts(2);

  // ---- slab write, tap by tap through LDS (as the seven-wave kernel): the wave stages the tiles of its pairs of this tap
  __syncthreads();
  constexpr int RS = CHX + 4;
  float* red = reinterpret_cast<float*>(smem16);           // [CHY][RS]
  const int fcol = lane & 15, fq = (lane >> 4) * 4;
  int etap[NS], eci[NS];                                   // (recomputed: not kept live through the stage loop)
#pragma unroll
  for (int q = 0; q < NS; ++q) { const int pr = NS * wave + q; etap[q] = pr / NCI; eci[q] = pr - etap[q] * NCI; }
#pragma unroll
  for (int t = 0; t < KS; ++t) {
#pragma unroll
    for (int q = 0; q < NS; ++q)
      if (etap[q] == t) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) red[(ycol[i] * 16 + fq + r) * RS + eci[q] * 16 + fcol] = acc[q][i][r];
      }
    if (XE) {
      if (t == ETAP) {
#pragma unroll
        for (int j = 0; j < NA; ++j)
          if (j < nex) {
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(ycol[j] * 16 + fq + r) * RS + (ECI0 + epair) * 16 + fcol] = ace[j][r];
          }
      }
    } else if (t == ETAP && wave < TM) {
#pragma unroll
      for (int e = 0; e < NF; ++e)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 16 + fq + r) * RS + (ECI0 + e) * 16 + fcol] = ace[e][r];
    }
    __syncthreads();
    float* slab = p.slabs + (((int64_t)s * KS * KS + trow * KS + t) * p.Np + co0) * p.Cq + ci0;
    for (int idx = tid; idx < CHY * (CHX / 4); idx += NW * 64) {
      const int row = idx / (CHX / 4), v = idx - row * (CHX / 4);
      if (co0 + row < p.Np && ci0 + v * 4 < p.Cq)
        *reinterpret_cast<float4*>(slab + (int64_t)row * p.Cq + v * 4) = *reinterpret_cast<const float4*>(red + row * RS + v * 4);
    }
    __syncthreads();
  }
  if (DBG & 16) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    rts(3);
    if (lane == 0) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(p.dbg) + ((int64_t)blockIdx.x * NW + wave) * 8;
      for (int i = 0; i < 4; ++i) o[i] = rt[i];
      for (int i = 0; i < 3; ++i) o[4 + i] = cyc[i];
      o[7] = (unsigned long long)nst;
    }
  }
}
#undef XWR8_READ

template <int KS, int TM, int NW, int PL = 2>
static constexpr size_t xwr_lds_bytes() {
  constexpr int NVEC = PL * 64 * (xwr_stride(TM * 16) / 8) + PL * (64 + KS - 1) * (xwr_stride(NW * 16) / 8);
  constexpr int NI = (NVEC + NW * 64 - 1) / (NW * 64);
  constexpr size_t stage = (size_t)2 * NI * NW * 64 * 16;
  constexpr size_t red = (size_t)TM * 16 * (NW * 16 + 4) * sizeof(float);
  return stage > red ? stage : red;
}

template <int KS, int TM, int NW, int PL = 2>
static int launch_xwgrad_rows(const XWRowsPlan& r, const XWRowsParams& q, hipStream_t st) {
  constexpr size_t lds = xwr_lds_bytes<KS, TM, NW, PL>();
  const dim3 grid((unsigned)(((q.S * q.coBlocks * q.ciBlocks + 7) / 8) * 8 * KS));
  if (KS == 5 && TM == 7 && NW == 7 && r.rows8) {
    // two stages of NI = 8 (PL = 1: 4) instructions x 8 waves x 1 KB (> the 52 KB staging tile of the slab write)
    constexpr size_t lds8 = (size_t)2 * ((PL * (64 * 14 + 68 * 14) + 511) / 512) * 512 * 16;
    if (PL == 1) {
      static LdsAttr attr81_set;
      if (set_max_lds(reinterpret_cast<const void*>(&conv_wgrad_rows8_bf16x3_kernel<0, 1, 1>), (size_t)lds8, attr81_set) != hipSuccess) return WCMC_ERR_LAUNCH;
      hipLaunchKernelGGL((conv_wgrad_rows8_bf16x3_kernel<0, 1, 1>), grid, dim3(512), lds8, st, q);
      return check_launch("conv2d_wgrad_bf16x3(rows8, one plane)");
    }
    static LdsAttr attr8_set, attr80_set;
#ifdef WCMC_DEBUG_BUILD
    { const char* e = ab_env("WCMC_DEBUG_ABLATE");
      const int ab = e ? atoi(e) : 0;
      auto kfn = ab == 16 ? &conv_wgrad_rows8_bf16x3_kernel<16> : ab == 1 ? &conv_wgrad_rows8_bf16x3_kernel<1> : ab == 2 ? &conv_wgrad_rows8_bf16x3_kernel<2>
                 : ab == 3 ? &conv_wgrad_rows8_bf16x3_kernel<3> : ab == 8 ? &conv_wgrad_rows8_bf16x3_kernel<8> : ab == 32 ? &conv_wgrad_rows8_bf16x3_kernel<32>
                 : ab == 34 ? &conv_wgrad_rows8_bf16x3_kernel<34> : ab == 35 ? &conv_wgrad_rows8_bf16x3_kernel<35> : nullptr;
      if (kfn) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds8);
        hipLaunchKernelGGL(kfn, grid, dim3(512), lds8, st, q);
        return check_launch("conv2d_wgrad_bf16x3(rows8 ablation / stamps)");
      } }
#endif
    if (set_max_lds(reinterpret_cast<const void*>(&conv_wgrad_rows8_bf16x3_kernel<0, 1>), (size_t)lds8, attr8_set) != hipSuccess) return WCMC_ERR_LAUNCH;
    if (set_max_lds(reinterpret_cast<const void*>(&conv_wgrad_rows8_bf16x3_kernel<0, 0>), (size_t)lds8, attr80_set) != hipSuccess) return WCMC_ERR_LAUNCH;
    if (r.xe) hipLaunchKernelGGL((conv_wgrad_rows8_bf16x3_kernel<0, 1>), grid, dim3(512), lds8, st, q);
    else hipLaunchKernelGGL((conv_wgrad_rows8_bf16x3_kernel<0, 0>), grid, dim3(512), lds8, st, q);
    return check_launch("conv2d_wgrad_bf16x3(rows8)");
  }
#ifdef WCMC_DEBUG_BUILD        // `make debug` only: timing-only instances that compute WRONG results are not in the release library
  if (KS == 5 && TM == 7 && NW == 7 && PL == 2) {
    int ab;                             // WCMC_DEBUG_ABLATE: timing-only builds (1 = no MFMA, 2 = no stage fills, 4 = clock probe)
    { const char* e = ab_env("WCMC_DEBUG_ABLATE"); ab = e ? atoi(e) : 0; }
    if (ab == 1 || ab == 2 || ab == 3 || ab == 4 || ab == 8 || ab == 16) {
      auto kfn = ab == 16 ? &conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 16> : ab == 1 ? &conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 1> : ab == 2 ? &conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 2>
                 : ab == 3 ? &conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 3> : ab == 4 ? &conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 4>
                 : &conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 8>;
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kfn, grid, dim3(448), lds, st, q);
      return check_launch("conv2d_wgrad_bf16x3(rows ablation)");
    }
  }
#endif
  static LdsAttr attr_set;
  if (set_max_lds(reinterpret_cast<const void*>(&conv_wgrad_rows_bf16x3_kernel<KS, TM, NW, 0, PL>), (size_t)lds, attr_set) != hipSuccess) return WCMC_ERR_LAUNCH;
  hipLaunchKernelGGL((conv_wgrad_rows_bf16x3_kernel<KS, TM, NW, 0, PL>), grid, dim3(NW * 64), lds, st, q);
  return check_launch("conv2d_wgrad_bf16x3(rows)");
}
// ks, tm, nw: the filter-row instance of x_plan_wgrad (rTM, rNW); planes: 1 = the hi planes only
XWRowsPlan x_plan_wgrad_rows(int ks, int tm, int nw, int planes) {
  XWRowsPlan r;
  r.ks = ks; r.tm = tm; r.nw = nw; r.pl = planes == 1 ? 1 : 2;
  // The eight-wave kernel for the two-plane (three-term) launches, the seven-wave one for the one-plane launches of the default
  // mode: there the seven waves are faster alone (0.311 against 0.295 of the bf16 peak in the eager profile) and beside the other
  // half of the step (+0.9 % per step, round 4).  WCMC_WGRAD_ROWS8=1 / 0: eight / seven waves for both.
  const char* r8e = ab_env("WCMC_WGRAD_ROWS8");
  r.rows8 = (ks == 5 && tm == 7 && nw == 7 && (r8e ? r8e[0] != '0' : r.pl == 2)) ? 1 : 0;
  r.xe = (r.rows8 && (r.pl == 1 || x_env_on("WCMC_WGRAD_ROWS8_XE"))) ? 1 : 0;      // (the one-plane eight-wave instance exists with XE = 1 only)
  return r;
}
int launch_xwgrad_rows(const XWRowsPlan& r, const XWRowsParams& q, hipStream_t st) {
  int rc = 0;
  const int key = (r.pl == 1 ? 1000 : 0) + r.ks * 100 + r.tm * 10 + r.nw;
  switch (key) {
    case 577: rc = launch_xwgrad_rows<5, 7, 7>(r, q, st); break;
    case 573: rc = launch_xwgrad_rows<5, 7, 3>(r, q, st); break;
    case 388: rc = launch_xwgrad_rows<3, 8, 8>(r, q, st); break;
    case 344: rc = launch_xwgrad_rows<3, 4, 4>(r, q, st); break;
    case 188: rc = launch_xwgrad_rows<1, 8, 8>(r, q, st); break;
    case 1577: rc = launch_xwgrad_rows<5, 7, 7, 1>(r, q, st); break;
    case 1573: rc = launch_xwgrad_rows<5, 7, 3, 1>(r, q, st); break;
    case 1388: rc = launch_xwgrad_rows<3, 8, 8, 1>(r, q, st); break;
    case 1344: rc = launch_xwgrad_rows<3, 4, 4, 1>(r, q, st); break;
    case 1188: rc = launch_xwgrad_rows<1, 8, 8, 1>(r, q, st); break;
    default: WCMC_REQUIRE(false, WCMC_ERR_BAD_ARG, "conv2d_wgrad_bf16x3: no filter-row instance for the plan");
  }
  return rc;
}

template <int TM, int PL = 2>
static int launch_xwgrad(const XWgradParams& p, hipStream_t stream) {
  constexpr size_t lds_stage = (size_t)PL * 64 * (xw_stride(TM * 16) + xw_stride(64)) * sizeof(u16);
  constexpr size_t lds_red = (size_t)TM * 16 * (64 + 4) * sizeof(float);
  constexpr size_t lds = lds_stage > lds_red ? lds_stage : lds_red;
  const int per_split = p.ks * p.ks * p.coBlocks * p.ciBlocks;
  const dim3 grid((unsigned)(((p.S + 7) / 8) * 8 * per_split));
  hipLaunchKernelGGL((conv_wgrad_bf16x3_kernel<TM, PL>), grid, dim3(256), lds, stream, p);
  return check_launch("conv2d_wgrad_bf16x3");
}
int launch_xwgrad(int tm, int planes, const XWgradParams& p, hipStream_t st) {      // tm: 7 or 4 cout tiles per block
  if (planes == 1) return tm == 7 ? launch_xwgrad<7, 1>(p, st) : launch_xwgrad<4, 1>(p, st);
  return tm == 7 ? launch_xwgrad<7>(p, st) : launch_xwgrad<4>(p, st);
}

}  // namespace wcmc
