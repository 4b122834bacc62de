// Split-bf16 convolution, the KPCN 5x5 layers: halo-resident, 64 pixels per wave (conv_halo64_bf16x3_kernel).
#include "bf16x3_common.h"

namespace wcmc {

// ------------------------------------------------------------------ implicit GEMM, halo-resident, 64 pixels per wave
// Interleaved timing ablations of conv_halo_bf16x3_kernel (scripts/time_halo_abl.py, 175 us): without the weight stream of the
// stage loop 156, without fragment reads 160, without both 135 -- per 32-k stage a workgroup of 128 pixels moves 86 KB
// through LDS (14 KB of weights in, the same 14 KB out again to EACH of its four waves, 16 KB of pixels) for 168 MFMAs
// and waits for a weight stage that was requested only one stage earlier.  This variant halves the LDS traffic and the
// weight stream per MFMA: a wave owns FOUR pixel tiles (64 pixels x all NT*16 couts: 22 KB of fragments for 12*NT MFMAs),
// a workgroup is four waves on a 16x16 tile, and two workgroups still share a CU (independent stage barriers) because
// the channel slab is thinner: 16 channels (the last one 8 or 16), pixel stride 80 B, 32 KB for the 20x20 halo.  A 32-k
// stage is then TWO filter taps x 16 channels (four taps x 8 in an 8-channel slab): k-group kg of the lanes reads tap
// 2s + (kg >> 1); taps past ks*ks are slab padding (zero weights) and read the tile's first pixel.
// Wave w owns tile rows w, w+4, w+8, w+12 (a tile that hangs over the image edge idles every wave equally).
// PXST: the halo pixel stride as a compile-time constant (80 or 160; 0 = p.PXS, the WCMC_HALO64_PXS experiments) -- with it the
// pixel tiles of a wave sit at immediate offsets of ONE address register per stage (the kernel is launched for ks == 5 only).
// AP: planes of the pixel operand that are multiplied -- 2: W_lo*A_hi + W_hi*A_lo + W_hi*A_hi; 1: the hi plane only (W_lo*A_hi +
// W_hi*A_hi: the data gradient of the "bf16x321" mode, whose A operand is dy) -- the halo then holds no lo plane and a
// pixel's PXS bytes carry twice the channels (x_plan_k).
// WP: planes of the WEIGHTS that are multiplied -- 2: both; 1 (with AP = 1 only): W_hi*A_hi alone, ONE bf16 MFMA per product -- the
// forward of an un-gated OUTPUT layer in the "bf16x321o" mode (the KPCN chains' 100 -> 441 logits: no ReLU behind it, so the
// rounding flips no gate; profiles/r04_forward_ladder.txt, table "last").  The lo plane of the pack is neither fetched nor read.
// F16 (with AP = 1, WP = 1): the operands are ONE fp16 plane each -- x as [pixel][Cpi] halfs (wcmc_split_to_f16), the weights' hi rows
// as fp16 (pack mode 4) -- multiplied by v_mfma_f32_16x16x32_f16: 11 bits per operand instead of bf16's 8 at the same MFMA count
// (the "bf16x321h" mode's output layers; same data movement as the bf16 one-term instance, half the halo bytes per channel pair).
template <int NT, int NB, int PT = 4, int DBG = 0, int PXST = 0, int AP = 2, int WP = 2, int F16 = 0>
__global__ __launch_bounds__(256, 2) void conv_halo64_bf16x3_kernel(XIgemmParams p0) {
  static_assert(WP == 2 || AP == 1, "one weight plane only together with one pixel plane");
  static_assert(!F16 || (AP == 1 && WP == 1), "fp16 operands: one plane each");
  XIgemmParams p = p0;
  if (PXST) { p.PXS = PXST; p.ks = 5; }
  constexpr int BN = NT * 16, TH = 4 * PT, TW = 16, NTHR = 256, NWV = 4;
  constexpr int NG = (PT + 1) / 2;             // epilogue groups of two pixel tiles per wave (128 pixels of staging)
  extern __shared__ __attribute__((aligned(16))) u16 smem16[];
  constexpr int B_LO = BN * XROW + 32, B_ELEMS = 2 * BN * XROW + 64;
  const int HWd = TW + p.ks - 1, HHt = TH + p.ks - 1, HP = HWd * HHt;     // (a 12-row workgroup of the PT = 4 instance keeps the 16-row layout)
  char* const halo = reinterpret_cast<char*>(smem16);
  u16* const bsm = smem16 + ((HP * p.PXS + 127) & ~127) / 2;

  // (wave as a SCALAR: the weight ring's LDS destinations, the group tests and the wait counts become scalar code -- as a
  // vector value they cost ~10 vector instructions and 4 v_readfirstlane per stage in a loop bound by vector issue)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // DBG (debug library, timing only, WRONG results): 1 no MFMA, 2 no weight DMA in the stage loop, 4 one halo per tile,
  // 8 no fragment reads, 32 no epilogue; 64 = wall-clock stamps (scripts/timeline_halo.py)
  unsigned long long st_rt[7] = {0, 0, 0, 0, 0, 0, 0};
  auto rstamp = [&](int i) {
    if (DBG & 64) {
      unsigned long long t;
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      st_rt[i] = t;
    }
  };
  rstamp(0);
  int tile;
  {
    const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int nmain = p.tilesX * p.tilesY;
  const int tpi = nmain + (PT == 4 ? p.stripX * p.stripY : 0);
  const int img = tile / tpi, trem0 = tile - img * tpi;
  // Transposed strip (PT = 4 instance): where 16 does not divide the output WIDTH either, the launcher covers it with tilesX columns
  // of 16 (these tiles) and stripX columns of 12 whose workgroups hold their halo TRANSPOSED in LDS -- LDS row = image column, LDS
  // column = image row: 16 image rows x 12 image columns look exactly like a 12-row tile to the stage loop (same pitch, same pixel
  // tile distance, same bank pattern); only the halo fill (which pixel goes where), the LDS offset of a filter tap (dx rows, dy
  // columns) and the epilogue's pixel coordinates know.  A pixel's products are summed in the same order in either orientation.
  const bool tr = PT == 4 && trem0 >= nmain;
  const int trem = tr ? trem0 - nmain : trem0;
  // Mixed tile heights (PT = 4 instance): the launcher covers Ho EXACTLY with rows16 tile rows of 16 pixels followed by tile rows of
  // 12 where it can (100 = 4 x 16 + 3 x 12: 100 rows of MFMAs instead of 108 or 112) -- a 12-row workgroup stages a 16-row halo and
  // skips its fourth pixel tile (ptc, wave-uniform).
  const int tcols = tr ? p.stripX : p.tilesX;
  const int trow = trem / tcols;
  const int ptc = tr ? 3 : (PT == 4 && trow >= p.rows16) ? 3 : PT;
  const int oy0 = tr ? trow * 16 : PT == 4 ? (trow < p.rows16 ? trow * 16 : p.rows16 * 16 + (trow - p.rows16) * 12) : trow * TH;
  const int ox0 = tr ? p.tilesX * TW + (trem - trow * tcols) * 12 : (trem - trow * tcols) * TW;
  const int n0 = blockIdx.y * BN;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, (int)p.wp_bytes, 0x00020000);
  const int pixb = (F16 ? 2 : 4) * p.Cpi;                // bytes per pixel of x: two bf16 planes, or one fp16 plane

  // ---- halo: [pixel][hi cs][lo cs] at stride PXS, one linear run of 16-byte vectors filled by LDS-DMA
  const int VP = p.PXS / 16;
  const int hvecs = HWd * (4 * ptc + p.ks - 1) * VP;      // (the rows this workgroup's pixel tiles reach)
  const float invVP = 1.0f / (float)VP, invHW = 1.0f / (float)HWd;
  // With the stride a template constant the per-lane source offsets of the halo's 16-byte vectors are worked out ONCE, for a
  // regular slab and for the last (narrower) one; a slab's fill is then one addition per instruction (+ slab * CS * 2, a
  // scalar).  Decoding them again for every slab cost ~25 vector instructions per vector, ~800 cycles of vector issue per
  // wave in front of the MFMAs of each slab's last stage (the "six halo reloads per tile: 4 %" of the ablations).
  constexpr int NHV = PXST ? (((TH + 4) * (TW + 4) * (PXST / 16) + 63) / 64 + NWV - 1) / NWV : 0;
  const int CSlh = p.CSl < 8 ? 8 : p.CSl;      // channels per plane the halo holds of the last slab (CSl = 4: a K order, x_last4)
  unsigned hoff[NHV ? NHV : 1], hoffl[NHV ? NHV : 1];
  if (PXST) {
#pragma unroll
    for (int kq = 0; kq < NHV; ++kq) {
      const int v = (wave + NWV * kq) * 64 + lane;
      hoff[kq] = XOOB; hoffl[kq] = XOOB;
      if (v < hvecs) {
        const int px = (int)(((float)v + 0.5f) * invVP), part = v - px * VP;     // exact: v < 2^13
        const int hy = (int)(((float)px + 0.5f) * invHW), hx = px - hy * HWd;
        const int iy = oy0 - p.pad + (tr ? hx : hy), ix = ox0 - p.pad + (tr ? hy : hx);       // (transposed: LDS row = image column)
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
          const unsigned pbase = (unsigned)(((img * p.H + iy) * p.W + ix) * pixb);
          if (AP == 1) {                             // hi plane only: part = 16-byte unit of the slab's channels
            if (part < p.CS / 8 && (p.nslabs - 2) * p.CS + part * 8 < p.Cpi) hoff[kq] = pbase + (unsigned)(part * 16);
            if (part < CSlh / 8 && (p.nslabs - 1) * p.CS + part * 8 < p.Cpi) hoffl[kq] = pbase + (unsigned)(part * 16);
          } else {
          {
            const int V = p.CS / 4, plane = part >= (V >> 1), vec = part - plane * (V >> 1);
            // (channel test against the widest regular slab, nslabs - 2: it then holds for every regular slab)
            if (part < V && (p.nslabs - 2) * p.CS + vec * 8 < p.Cpi) hoff[kq] = pbase + (unsigned)(plane * 2 * p.Cpi + vec * 16);
          }
          {
            const int V = CSlh / 4, plane = part >= (V >> 1), vec = part - plane * (V >> 1);
            if (part < V && (p.nslabs - 1) * p.CS + vec * 8 < p.Cpi) hoffl[kq] = pbase + (unsigned)(plane * 2 * p.Cpi + vec * 16);
          }
          }
        }
      }
    }
  }
  auto dma_halo = [&](int slab) {
    if (PXST) {
      const unsigned so = (unsigned)(slab * p.CS * 2);
      const bool lastslab = slab == p.nslabs - 1;
#pragma unroll
      for (int kq = 0; kq < NHV; ++kq) {
        const int ii = wave + NWV * kq;
        if (ii * 64 < hvecs) {
          const unsigned off = (lastslab ? hoffl[kq] : hoff[kq]) + so;     // (invalid: 2^31 + a few hundred: out of range)
          if (ii * 64 + lane < hvecs)                                      // (the tail of the last instruction would land in the weight ring)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (__attribute__((address_space(3))) void*)(halo + ii * 1024), 16, off, 0, 0, 0);
        }
      }
      return;
    }
    const int V = (slab == p.nslabs - 1 ? CSlh : p.CS) / (AP == 1 ? 8 : 4);      // data vectors per halo pixel (AP planes x cs/8)
    for (int ii = wave; ii * 64 < hvecs; ii += NWV) {
      const int v = ii * 64 + lane;
      if (v < hvecs) {
        const int px = (int)(((float)v + 0.5f) * invVP), part = v - px * VP;     // exact: v < 2^13
        const int hy = (int)(((float)px + 0.5f) * invHW), hx = px - hy * HWd;
        const int iy = oy0 - p.pad + (tr ? hx : hy), ix = ox0 - p.pad + (tr ? hy : hx);
        const int plane = AP == 1 ? 0 : part >= (V >> 1), vec = part - plane * (V >> 1);
        const int ch = slab * p.CS + vec * 8;
        unsigned off = XOOB;
        if (part < V && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W && ch < p.Cpi)
          off = (unsigned)(((img * p.H + iy) * p.W + ix) * pixb + plane * 2 * p.Cpi + ch * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (__attribute__((address_space(3))) void*)(halo + ii * 1024), 16, off, 0, 0, 0);
      }
    }
  };

  // ---- weights: LDS-DMA ring of NB stages, as in conv_halo_bf16x3_kernel (row group = 16 cout rows x 64 B per plane)
  const int nstages = p.Kt / XKC;
  constexpr int NGMAX = (NT + NWV - 1) / NWV;
  const int ngroups = wave < NT ? (NT - wave + NWV - 1) / NWV : 0;       // wave-uniform
  unsigned dbase[NGMAX], dbase2[NGMAX];                  // hi / lo plane of this lane's 16 bytes of a stage's row group
#pragma unroll
  for (int q = 0; q < NGMAX; ++q) {
    const int drow = 16 * (wave + q * NWV) + (lane >> 2);
    const int dvq = (lane & 3) ^ ((drow >> 1) & 3);
    dbase[q] = (q < ngroups && n0 + drow < p.Np) ? (unsigned)(((n0 + drow) * 2 * p.Kt + dvq * 8) * 2) : XOOB;
    dbase2[q] = dbase[q] >= XOOB ? XOOB : dbase[q] + (unsigned)(p.Kt * 2);
  }
  auto dma_b = [&](int g, int buf) {
    // one addition per instruction: the stage's byte offset is a scalar; stages past the end add 2^30 instead, which puts
    // valid rows (< 2^30: the packed weights are a few MB) and invalid ones (2^31) alike beyond the buffer without wrapping
    const unsigned sg = g < nstages ? (unsigned)(g * XKC * 2) : 0x40000000u;
#pragma unroll
    for (int q = 0; q < NGMAX; ++q) {
      if (q < ngroups) {
        const unsigned off = dbase[q] + sg;
        const unsigned off2 = dbase2[q] + sg;
        u16* d = bsm + buf * B_ELEMS + 16 * (wave + q * NWV) * XROW;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (__attribute__((address_space(3))) void*)d, 16, off, 0, 0, 0);
        if (WP == 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (__attribute__((address_space(3))) void*)(d + B_LO), 16, off2, 0, 0, 0);
      }
    }
  };

  f32x4 acc[NT][PT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < PT; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- fragments: lane = pixel column (lane & 15) of its four tile rows, k group kg = lane >> 4 (8 k each)
  const int frow = lane & 15, kg = lane >> 4;
  const int fslot = (kg ^ ((frow >> 1) & 3)) * 8;
  const int abase0 = (wave * HWd + frow) * p.PXS, dA = NWV * HWd * p.PXS;   // tile row i of the wave: + i * dA (a constant with PXST)
  // this lane's (tap, channel) of the stage whose A fragments are read next
  int cs_cur, sps_cur, lo_off, tps, coff, tdx, tdy;
  bool cs4 = false;                                      // (wave-uniform) the slab being read is in the four-channel K order (x_last4)
  // The LDS offset of the lane's tap is carried along instead of being worked out from (tdy, tdx) every stage: one filter column is
  // sMx bytes away, one filter row sMy -- a pixel and a halo row in a regular workgroup, the other way round in a transposed one (the
  // tap (dy, dx) is then dx LDS rows and dy LDS columns away) -- so the orientation costs the stage loop nothing.
  const int sMx = tr ? HWd * p.PXS : p.PXS, sMy = tr ? p.PXS : HWd * p.PXS;
  int toff = 0, dstep = 0;                               // toff: (tdy, tdx) as bytes + coff; dstep: one stage's taps in x
  const int wrapc = sMy - p.ks * sMx;                    // ... and what a wrap into the next filter row adds
  auto slab_begin = [&](int slab) {
    cs_cur = slab == p.nslabs - 1 ? p.CSl : p.CS;
    sps_cur = slab == p.nslabs - 1 ? p.SPSl : (p.SPS & 0xff);
    cs4 = cs_cur == 4;
    lo_off = (cs4 ? 8 : cs_cur) * 2;
    tps = 32 / cs_cur;                                   // taps per stage: 1 (32 channels), 2 (16), 4 (8) or 8 (4)
    coff = cs4 ? 0 : ((kg * 8) & (cs_cur - 1)) * 2;
    tdy = 0; tdx = cs_cur == 32 ? 0 : cs_cur == 16 ? (kg >> 1) : cs4 ? 2 * kg : kg;        // (cs4: the FIRST of the lane's two taps)
    if (tdx >= p.ks) { tdx -= p.ks; ++tdy; }             // (cs4, kg = 3: tap 6)
    toff = tdy * sMy + tdx * sMx + coff;
    dstep = tps * sMx;
  };
  bf16x8 ah[PT], al[PT], wh[NT], wl[NT];
  auto a_off = [&]() { return tdy < p.ks ? toff : coff; };          // (taps past ks * ks are slab padding: zero weights, any pixel)
  // (cs4) the lane's second tap: the next one in the filter's raster order
  auto a_off2 = [&]() {
    const bool wrap = tdx + 1 >= p.ks;
    const int y = tdy + (wrap ? 1 : 0);
    return y < p.ks ? toff + sMx + (wrap ? wrapc : 0) : 0;
  };
  auto a_advance = [&]() {
    tdx += tps; toff += dstep;
    if (tdx >= p.ks) { tdx -= p.ks; ++tdy; toff += wrapc; }
    if (cs4 && tdx >= p.ks) { tdx -= p.ks; ++tdy; toff += wrapc; }      // (eight taps ahead: up to two rows of five)
  };
  auto read_a1 = [&](int i, int aoff, int aoff2) {
    const char* pa = halo + abase0 + aoff;
    if (cs4) {                                            // two taps x four channels: 8 bytes each
      const char* pb = halo + abase0 + aoff2;
      const u32x2 a0 = *reinterpret_cast<const u32x2*>(pa + i * dA), a1 = *reinterpret_cast<const u32x2*>(pb + i * dA);
      ah[i] = __builtin_bit_cast(bf16x8, u32x4{a0.x, a0.y, a1.x, a1.y});
      if (AP == 2) {
        const u32x2 l0 = *reinterpret_cast<const u32x2*>(pa + lo_off + i * dA), l1 = *reinterpret_cast<const u32x2*>(pb + lo_off + i * dA);
        al[i] = __builtin_bit_cast(bf16x8, u32x4{l0.x, l0.y, l1.x, l1.y});
      }
      return;
    }
    ah[i] = *reinterpret_cast<const bf16x8*>(pa + i * dA);
    if (AP == 2) al[i] = *reinterpret_cast<const bf16x8*>(pa + lo_off + i * dA);
  };
  const u16* const bfrag = bsm + frow * XROW + fslot;
  auto read_b = [&](int buf, int j) {
    wh[j] = *reinterpret_cast<const bf16x8*>(bfrag + buf * B_ELEMS + j * 16 * XROW);
    if (WP == 2) wl[j] = *reinterpret_cast<const bf16x8*>(bfrag + buf * B_ELEMS + B_LO + j * 16 * XROW);
  };

#pragma unroll
  for (int b = 0; b < NB; ++b) dma_b(b, b);
  dma_halo(0);
  slab_begin(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  {
    const int aoff = a_off(), aoff2 = cs4 ? a_off2() : 0;
#pragma unroll
    for (int i = 0; i < PT; ++i)
      if (i < ptc) read_a1(i, aoff, aoff2);
    a_advance();
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) read_b(0, j);
  int s_in = 0, slab = 0, bcur = 0;
  const int wgpar = (blockIdx.x >> 8) & 1;
  const bool prio_on = p.SPS & 0x100;          // (set by the launcher)
  rstamp(1);
  for (int g = 0; g < nstages; ++g) {
    const int b1 = bcur + 1 == NB ? 0 : bcur + 1;      // buffer of stage g+1; stage g's fragments are in registers
    if (NGMAX == 1 || ngroups < 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WP * (NB - 2)) : "memory");       // (WP DMA instructions per row group)
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * WP * (NB - 2)) : "memory");
    pw_barrier();                                // stage g+1 has landed for everyone; everyone has read stage g's fragments
    // The two workgroups of a CU are dispatched one after the other (local block indices l and l + 32 of an XCD) and the
    // instruction arbiter prefers the older wave: stamps showed the first one through its stage loop in 114 us and the
    // second in 158, the last 40 us alone on the CU.  Alternating the priority stage by stage shares the matrix pipe.
    if (prio_on) { if ((g ^ wgpar) & 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
    if (!(DBG & 2)) dma_b(g + NB, bcur);
    bcur = b1;
    const bool last_of_slab = (s_in + 1 == sps_cur);
    if (last_of_slab && slab + 1 < p.nslabs && !(DBG & 4)) dma_halo(slab + 1);      // (no wave reads the halo during a slab's last stage)
    const int aoff = a_off(), aoff2 = cs4 ? a_off2() : 0;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
      for (int i = 0; i < PT; ++i) {
        if (i >= ptc) continue;                    // (PT = 4 instance on a 12-row tile: wave-uniform)
        if (!(DBG & 1)) {
          if (WP == 2) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], ah[i], acc[j][i], 0, 0, 0);   // small terms first
          if (AP == 2) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], al[i], acc[j][i], 0, 0, 0);
          if (F16) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(xf16x8, wh[j]), __builtin_bit_cast(xf16x8, ah[i]), acc[j][i], 0, 0, 0);
          else acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], ah[i], acc[j][i], 0, 0, 0);
        }
        // the pixel tile's fragments of stage g+1 replace it as soon as its last MFMAs of this stage have issued
        if (j == NT - 1 && !last_of_slab && !(DBG & 8)) read_a1(i, aoff, aoff2);
      }
      if (!(DBG & 8)) read_b(b1, j);             // stage g+1, same cout tile, into the registers just consumed
      __builtin_amdgcn_sched_barrier(0);
    }
    if (!last_of_slab) {
      a_advance();
      ++s_in;
    } else {                                     // slab boundary: the next A fragments come from the next halo
      s_in = 0;
      ++slab;
      slab_begin(slab < p.nslabs ? slab : p.nslabs - 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the new halo (and of the weight ring)
      __syncthreads();
      const int a2 = a_off(), a22 = cs4 ? a_off2() : 0;
#pragma unroll
      for (int i = 0; i < PT; ++i)
        if (i < ptc) read_a1(i, a2, a22);
      a_advance();
    }
  }
  __builtin_amdgcn_s_setprio(0);
  rstamp(2);
  if ((DBG & 32) && !(DBG & 64)) {                     // timing only: no epilogue (one store keeps the accumulators alive)
    float keep = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < PT; ++i) keep += acc[j][i][0] + acc[j][i][1] + acc[j][i][2] + acc[j][i][3];
    if (keep == 12345.678f && p.ys) p.ys[0] = 1;
    return;
  }
  // ---- epilogue operands (one batch of unconditional buffer loads, issued before the drain)
  const int fq = kg * 4;
  float bv[NT][4];
  {
    const __amdgpu_buffer_rsrc_t brs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(p.bias ? (const void*)p.bias : (const void*)p.wp), 0, p.bias ? p.Cout * 4 : 0, 0x00020000);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        bv[j][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(brs, (n0 + j * 16 + fq + e) * 4, 0, 0));
  }
  const bool use_gate = p.ys && p.gate, use_mask = p.ys && !p.gate && p.gate_mask && p.gate_act != WCMC_ACT_LINEAR;
  u32x2 gv[PT][NT];                            // split gate: 4 hi-plane bf16 per quad; bit mask: one byte in .x
  bool okp[PT]; int64_t mp[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int oy = tr ? oy0 + frow : oy0 + wave + NWV * i, ox = tr ? ox0 + wave + NWV * i : ox0 + frow;
    okp[i] = i < ptc && oy < p.Ho && ox < p.Wo;
    mp[i] = ((int64_t)img * p.Ho + oy) * p.Wo + ox;
  }
  if (use_gate) {
    const int64_t gbytes = (int64_t)p.N * p.Ho * p.Wo * 4 * p.Cpo;
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void*)p.gate, 0, (int)(gbytes < 0x7fffffff ? gbytes : 0x7fffffff), 0x00020000);
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 16 + fq;
        gv[i][j] = __builtin_amdgcn_raw_buffer_load_b64(grs, (okp[i] && co < p.Cpo) ? (unsigned)((mp[i] * 2 * p.Cpo + co) * 2) : XOOB, 0, 0);
      }
  } else if (use_mask) {
    const int64_t mbytes = (int64_t)p.N * p.Ho * p.Wo * (p.Cpo >> 3);
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.gate_mask, 0, (int)mbytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 16 + fq;
        gv[i][j].x = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(mrs, (okp[i] && co < p.Cpo) ? (unsigned)(mp[i] * (p.Cpo >> 3) + (co >> 3)) : XOOB, 0, 0);
      }
  }
  const XAct ak = x_act(p.act, p.slope);
  const float gate_off = p.gate_act == WCMC_ACT_RELU ? 0.f : p.gate_act == WCMC_ACT_LEAKY_RELU ? p.gate_slope : 1.f;
  const int gkind = use_gate ? 1 : use_mask ? 2 : 0;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the (zero) weight stages past the end have landed:
  __syncthreads();                                     // LDS is free for the epilogue staging
  rstamp(3);

  // ---- epilogue in two halves of 128 pixels (the staging tile of 256 split pixels would not fit beside a second
  // workgroup): half h = pixel tiles 2h, 2h+1 of every wave; staging row pr = 32 * wave + 16 * (i & 1) + column
  auto pix_of = [&](int h, int pr, int& oy, int& ox) {
    const int i = 2 * h + ((pr >> 4) & 1);             // (PT odd: the last group holds one pixel tile)
    if (tr) { oy = oy0 + (pr & 15); ox = ox0 + (pr >> 5) + NWV * i; }
    else { oy = oy0 + (pr >> 5) + NWV * i; ox = ox0 + (pr & 15); }
    return i < ptc && oy < p.Ho && ox < p.Wo;
  };
  if (p.ys) {
    constexpr int OLD = 2 * BN + 8;
    u16* so = smem16;
    constexpr int CW = BN <= 16 ? 16 : BN <= 32 ? 32 : BN <= 64 ? 64 : 128, RG = NTHR / CW;
    const int cc = tid % CW, rg = tid / CW;
    float csum = 0.f;
#pragma unroll
    for (int h = 0; h < NG; ++h) {
      if (h) __syncthreads();                            // the first half has left the staging tile
#pragma unroll
      for (int il = 0; il < 2; ++il) {
        const int pr = wave * 32 + il * 16 + frow;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int co = n0 + j * 16 + fq;
          unsigned h01 = 0, l01 = 0, h23 = 0, l23 = 0;
          if (2 * h + il < PT) {                           // (else: zeros, the column sums run over all 128 rows)
            constexpr int dummy = 0; (void)dummy;
            float v[4];
            const int ti = 2 * h + il < PT ? 2 * h + il : 0;
            x_epi_quad(acc[j][ti], bv[j], okp[ti], ak, gkind, gv[ti][j], co, gate_off, v);
            x_split2(v[0], v[1], h01, l01);
            x_split2(v[2], v[3], h23, l23);
          }
          *reinterpret_cast<uint2*>(so + pr * OLD + j * 16 + fq) = make_uint2(h01, h23);
          *reinterpret_cast<uint2*>(so + pr * OLD + BN + j * 16 + fq) = make_uint2(l01, l23);
        }
      }
      __syncthreads();
      if (h == 0) rstamp(4);
      constexpr int VPP = BN / 8;
      for (int v = tid; v < 128 * 2 * VPP; v += NTHR) {
        const int pr = v / (2 * VPP), q = v - pr * (2 * VPP);
        const int plane = q >= VPP, vec = q - plane * VPP;
        const int co = n0 + vec * 8;
        int oy, ox;
        if (pix_of(h, pr, oy, ox) && co < p.Cpo) {
          const int64_t m = ((int64_t)img * p.Ho + oy) * p.Wo + ox;
          const u32x4 hv = *reinterpret_cast<const u32x4*>(so + pr * OLD + plane * BN + vec * 8);
          *reinterpret_cast<u32x4*>(p.ys + m * 2 * p.Cpo + plane * p.Cpo + co) = hv;
          if (p.mask_out && plane == 0) p.mask_out[m * (p.Cpo >> 3) + (co >> 3)] = positive_mask8(hv);
        }
      }
      if (h == 0) rstamp(5);
      if (p.colsum && cc < BN)
        for (int r = rg; r < 128; r += RG) csum += bf2f(so[r * OLD + cc]) + bf2f(so[r * OLD + BN + cc]);
    }
    if (p.colsum && !(DBG & 64)) {
      __syncthreads();
      float* red = reinterpret_cast<float*>(so);
      if (rg > 0 && cc < BN) red[(rg - 1) * BN + cc] = csum;
      __syncthreads();
      if (rg == 0 && cc < BN && n0 + cc < p.Np) {
        for (int q = 0; q < RG - 1; ++q) csum += red[q * BN + cc];
        p.colsum[(int64_t)tile * p.Np + n0 + cc] = csum;
        // trailer: the number of rows this launch wrote (the finish kernel reads no further)
        if (tile == 0 && n0 + cc == 0) reinterpret_cast<int*>(p.colsum)[(int64_t)p.G * p.Np] = (int)gridDim.x;
      }
    }
  } else {
    constexpr int OLD = BN + 4;
    float* so = reinterpret_cast<float*>(smem16);
#pragma unroll
    for (int h = 0; h < NG; ++h) {
      if (h) __syncthreads();
#pragma unroll
      for (int il = 0; il < 2; ++il) {
        const int pr = wave * 32 + il * 16 + frow;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int co = n0 + j * 16 + fq;
          const f32x4 a4 = acc[j][2 * h + il < PT ? 2 * h + il : 0];
          float v[4];
          x_epi_quad(a4, bv[j], true, ak, 0, u32x2{0u, 0u}, co, 1.f, v);
          *reinterpret_cast<float4*>(so + pr * OLD + j * 16 + fq) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
      __syncthreads();
      constexpr int VPP = BN / 4;
      for (int v = tid; v < 128 * VPP; v += NTHR) {
        const int pr = v / VPP, vec = v - pr * VPP;
        const int co = n0 + vec * 4;
        int oy, ox;
        if (pix_of(h, pr, oy, ox) && co < p.Cpo)
          *reinterpret_cast<float4*>(p.yf + (int64_t)img * p.ysn + (int64_t)oy * p.ysh + (int64_t)ox * p.ysw + co) =
              *reinterpret_cast<const float4*>(so + pr * OLD + vec * 4);
      }
    }
  }
  if (DBG & 64) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the stores have left)
    rstamp(6);
    if (lane == 0) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(p.colsum) + ((int64_t)tile * NWV + wave) * 14;
      for (int i = 0; i < 7; ++i) o[6 + i] = st_rt[i];
      unsigned hw, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      o[13] = hw | ((unsigned long long)xcc << 32);
    }
  }
}

static size_t xh64_halo_bytes(int th, const XIgemmParams& p) { return (size_t)(((th + p.ks - 1) * (16 + p.ks - 1) * p.PXS + 127) & ~127); }
static size_t xh64_bstage_bytes(int nt) { return (size_t)(2 * nt * 16 * XROW + 64) * sizeof(u16); }      // one weight stage

XHalo64Plan x_plan_halo64(int nt, const XIgemmParams& p) {
  XHalo64Plan h;
  h.nt = nt;
  // Tile height 16 (four pixel tiles per wave) or 12 (three): 512 workgroups are resident (two per CU), a launch takes
  // ceil(workgroups / 512) rounds of a time proportional to the tile height.  The KPCN layers of 100..108 output rows
  // are 392 tiles of 16x16 (one round, a quarter of the slots empty) but 504 of 12x16 (one round of 3/4 the length).
  const int gy = (p.Np / 16 + nt - 1) / nt;
  auto rounds = [&](int th) { return ((int64_t)p.N * p.tilesX * ((p.Ho + th - 1) / th) * gy + 511) / 512 * th; };
  bool pt3 = p.PXS == 160 || (x_env_on("WCMC_HALO64_PT3") && rounds(12) < rounds(16));     // (32-channel slabs: 12x16 only)
  // 16 does not divide Ho (KPCN: 124, 120, 116, 108, 104, 100, 92 rows): a tile rows of 16 followed by b of 12 cover it EXACTLY -- the
  // 16-row instance, whose workgroups of the last b tile rows skip their fourth pixel tile (p.rows16).  Smallest b: as many workgroups
  // as the 16-row tiling and no padded rows (3-7 % fewer MFMAs than the better pure tiling where 12 does not divide Ho either; where
  // it does -- 120, 108 -- the same MFMAs in fewer, taller workgroups: less weight streaming per pixel).  ALONE such a launch is slower
  // (one round of 16-row workgroups where the 12-row tiling ran a shorter round: +2 % per branch); the captured two-stream step is
  // faster by 1.8 %, every one of the seven heights contributing (profiles/r06_step_ab.txt).  Where 16 divides Ho
  // the rule above stands (96 rows: 288 workgroups of 16 rows are slower than 384 of 12, in the step too).
  // Debug build, WCMC_HALO64_MIX: 0 = pure tilings, 1 = mix only where 12 does not divide Ho either; WCMC_HALO64_NOMIX=<Ho>: one
  // height keeps its pure tiling (the per-height A/B).
  h.rows16 = 1 << 20; h.stripX = h.stripY = 0; h.tilesX = p.tilesX;
  const char* mixe = ab_env("WCMC_HALO64_MIX");
  const bool mix12 = !(mixe && mixe[0] == '1');
  const char* nomix = ab_env("WCMC_HALO64_NOMIX");
  if (p.PXS != 160 && p.Ho % 16 != 0 && (p.Ho % 12 != 0 || mix12) && x_env_on("WCMC_HALO64_MIX") && !(nomix && atoi(nomix) == p.Ho)) {
    for (int b = 1; 12 * b < p.Ho; ++b)
      if ((p.Ho - 12 * b) % 16 == 0) { h.rows16 = (p.Ho - 12 * b) / 16; pt3 = false; break; }
  }
  const bool mixed = h.rows16 != (1 << 20);
  const int th = pt3 ? 12 : 16;
  h.tilesY = mixed ? h.rows16 + (p.Ho - 16 * h.rows16) / 12 : (p.Ho + th - 1) / th;
  const size_t halo = xh64_halo_bytes(th, p), bstage = xh64_bstage_bytes(nt);
  const size_t out = p.ys ? (size_t)128 * (2 * nt * 16 + 8) * sizeof(u16) : (size_t)128 * (nt * 16 + 4) * sizeof(float);
  // three weight stages where two workgroups still fit a CU (80 KB each), else two
  const char* nbe = ab_env("WCMC_HALO_NB");
  h.nb = (p.ap == 1 || (!(nbe && nbe[0] == '2') && halo + 3 * bstage <= 80 * 1024)) ? 3 : 2;
  h.pt = pt3 ? 3 : 4;
  // The width likewise: where 16 does not divide Wo, a tile columns of 16 + b columns of 12 cover it exactly; the b columns are a
  // strip of workgroups that hold their halo transposed (see the kernel: 16 image rows x 12 image columns each, 16-row tile rows) --
  // the 16-row instance only.  (WCMC_HALO64_STRIP=0, debug build: 16-wide tiles throughout.)
  if (!pt3 && p.ks == 5 && p.Wo % 16 != 0 && p.Wo % 4 == 0 && x_env_on("WCMC_HALO64_STRIP")) {
    for (int b = 1; b <= 3; ++b)
      if (12 * b < p.Wo && (p.Wo - 12 * b) % 16 == 0) { h.stripX = b; h.tilesX = (p.Wo - 12 * b) / 16; h.stripY = (p.Ho + 15) / 16; break; }
  }
  const size_t main_ = halo + h.nb * bstage;
  h.lds = main_ > out ? main_ : out;
  // which instance: the hi-plane ones exist for three weight stages and seven cout tiles (one MFMA per product: wp = 1, fp16 operands:
  // f16) or seven / one (two MFMAs: ap = 1; x_plan_k grants ap = 1 with PXS = 80, ks = 5 only); the halo pixel stride is a template
  // constant for the two shipped values (nb = 3: 16-channel slabs, 80 B; nb = 2 with 12x16 tiles: 32-channel slabs, 160 B), anything
  // else (WCMC_HALO_NB experiments) reads it from the params (pxst = 0)
  const bool hi = h.nb == 3 && p.ap == 1;
  h.wp = (hi && nt == 7 && p.wplanes == 1) ? 1 : 2;      // "bf16x321o" output layers
  h.f16 = (h.wp == 1 && p.f16) ? 1 : 0;                  // "bf16x321h" output layers
  h.ap = (hi && (nt == 7 || nt == 1)) ? 1 : 2;
  h.pxst = h.ap == 1 ? 80 : (p.ks == 5 && p.PXS == 80 && h.nb == 3) ? 80 : (p.ks == 5 && p.PXS == 160 && h.nb == 2 && pt3) ? 160 : 0;
  return h;
}

template <int NT, int NB, int PT, int PXST, int AP = 2, int WP = 2, int F16 = 0>
static int launch_xhalo64c(const XHalo64Plan& h, const XIgemmParams& p, hipStream_t stream) {
  WCMC_REQUIRE(h.nt == NT && h.nb == NB && h.pt == PT && h.pxst == PXST && h.ap == AP && h.wp == WP && h.f16 == F16, WCMC_ERR_LAUNCH,
               "conv2d_igemm_bf16x3(halo, 64 pixels per wave): no instance for the plan");
  static LdsAttr attr;
  if (set_max_lds(reinterpret_cast<const void*>(&conv_halo64_bf16x3_kernel<NT, NB, PT, 0, PXST, AP, WP, F16>), h.lds, attr) != hipSuccess) return WCMC_ERR_LAUNCH;
  const dim3 grid((unsigned)(p.N * (p.tilesX * p.tilesY + (PT == 4 ? p.stripX * p.stripY : 0))), (unsigned)((p.Np / 16 + NT - 1) / NT));
  hipLaunchKernelGGL((conv_halo64_bf16x3_kernel<NT, NB, PT, 0, PXST, AP, WP, F16>), grid, dim3(256), h.lds, stream, p);
  return check_launch("conv2d_igemm_bf16x3(halo, 64 pixels per wave)");
}
template <int NT, int NB, int PT>
static int launch_xhalo64b(const XHalo64Plan& h, const XIgemmParams& p, hipStream_t stream) {
  if constexpr (NT == 7 && NB == 3) {
    if (h.f16) return launch_xhalo64c<NT, NB, PT, 80, 1, 1, 1>(h, p, stream);
    if (h.wp == 1) return launch_xhalo64c<NT, NB, PT, 80, 1, 1>(h, p, stream);
  }
  if constexpr ((NT == 7 || NT == 1) && NB == 3) {
    if (h.ap == 1) return launch_xhalo64c<NT, NB, PT, 80, 1>(h, p, stream);
  }
  if (h.pxst == 80) return launch_xhalo64c<NT, NB, PT, NB == 3 ? 80 : 0>(h, p, stream);
  if (h.pxst == 160) return launch_xhalo64c<NT, NB, PT, (NB == 2 && PT == 3) ? 160 : 0>(h, p, stream);
  return launch_xhalo64c<NT, NB, PT, 0>(h, p, stream);
}
template <int NT>
static int launch_xhalo64(const XHalo64Plan& h, const XIgemmParams& p0, hipStream_t stream) {
  XIgemmParams p = p0;
  p.SPS |= 0x100;     // alternate the priority of a CU's two workgroups stage by stage (measured neutral on the launch time, kept: it evens the two workgroups' finish times; its A/B switch is gone)
  p.rows16 = h.rows16; p.tilesY = h.tilesY; p.stripX = p.stripY = 0;
#ifdef WCMC_DEBUG_BUILD
  if (NT == 7 && h.pt == 4 && p.PXS == 80 && p.ks == 5) {
    const char* e = ab_env("WCMC_DEBUG_ABLATE");
    const int ab = e ? atoi(e) : 0;
    if (ab) {
      auto kfn = ab == 1 ? &conv_halo64_bf16x3_kernel<7, 3, 4, 1, 80> : ab == 2 ? &conv_halo64_bf16x3_kernel<7, 3, 4, 2, 80>
                 : ab == 4 ? &conv_halo64_bf16x3_kernel<7, 3, 4, 4, 80> : ab == 8 ? &conv_halo64_bf16x3_kernel<7, 3, 4, 8, 80>
                 : ab == 10 ? &conv_halo64_bf16x3_kernel<7, 3, 4, 10, 80> : ab == 14 ? &conv_halo64_bf16x3_kernel<7, 3, 4, 14, 80>
                 : ab == 32 ? &conv_halo64_bf16x3_kernel<7, 3, 4, 32, 80> : ab == 46 ? &conv_halo64_bf16x3_kernel<7, 3, 4, 46, 80>
                 : &conv_halo64_bf16x3_kernel<7, 3, 4, 64, 80>;
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      const dim3 grid((unsigned)(p.N * p.tilesX * p.tilesY), (unsigned)((p.Np / 16 + NT - 1) / NT));
      hipLaunchKernelGGL(kfn, grid, dim3(256), xh64_halo_bytes(16, p) + 3 * xh64_bstage_bytes(NT), stream, p);
      return check_launch("conv2d_igemm_bf16x3(halo64, debug)");
    }
  }
#endif
  p.tilesX = h.tilesX; p.stripX = h.stripX; p.stripY = h.stripY;
  if (h.pt == 3) return h.nb == 3 ? launch_xhalo64b<NT, 3, 3>(h, p, stream) : launch_xhalo64b<NT, 2, 3>(h, p, stream);
  return h.nb == 3 ? launch_xhalo64b<NT, 3, 4>(h, p, stream) : launch_xhalo64b<NT, 2, 4>(h, p, stream);
}
int launch_xhalo64(const XHalo64Plan& h, const XIgemmParams& p, hipStream_t stream) {
  switch (h.nt) {
    case 7: return launch_xhalo64<7>(h, p, stream);
    case 4: return launch_xhalo64<4>(h, p, stream);
    case 2: return launch_xhalo64<2>(h, p, stream);
    default: return launch_xhalo64<1>(h, p, stream);
  }
}

}  // namespace wcmc
