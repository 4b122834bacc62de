// Split-bf16 convolution, ks 3..5: halo-resident implicit GEMM on 16x16 / 8x16 pixel tiles (conv_halo_bf16x3_kernel).
#include "bf16x3_common.h"

namespace wcmc {

// ------------------------------------------------------------------ implicit GEMM, halo-resident (ks 3..5)
// Stamps of the streaming kernel (bf16x3_igemm.hip; scripts/stamp_igemm.py): per 32-k stage a wave spends 830 cycles
// issuing its 8 buffer loads and 540 storing them to LDS, against 770 issuing MFMAs -- the L1/TA path and
// L2 bandwidth (23 B/clk/CU sustained), not the matrix pipe, set the pace, and 53 % of those bytes are
// the A operand re-read once per filter tap.  This kernel keeps the input pixels of a 16x16 output
// tile with their (ks-1) halo resident in LDS for one channel slab (CS <= 64 channels, both planes) and
// reads every tap's A fragments from there with shifted addresses; only the weights stream (14 KB per
// stage for 256 pixels instead of 30 KB for 128).  512 threads = 8 waves, each 32 pixels (two tile rows)
// x all NT*16 couts; one workgroup per CU (LDS: halo 90-115 KB + two weight stages).
// K order: slab-major (pack_weight_split_kernel); stages never straddle slabs (Ks % 32 == 0).
template <int NT, int TH, int TW, int DBG = 0, int NB = 3, int AP = 2>       // AP: see conv_halo64_bf16x3_kernel
__global__ __launch_bounds__(TH * TW * 2, (TH * TW <= 128 ? 2 : 1)) void conv_halo_bf16x3_kernel(XIgemmParams p) {
  constexpr int BN = NT * 16;
  constexpr int TPX = TH * TW, NTHR = TPX * 2, NWV = NTHR / 64;   // one wave per 32 pixels (two MFMA pixel tiles)
  constexpr int TPR = TW / 16;                 // MFMA pixel tiles per tile row
  static_assert(TPX % 32 == 0 && TW % 16 == 0, "a wave = 2 pixel tiles of 16");
  constexpr int STW = BN * 4 >= NWV * 14 * 8 ? NWV : 1;    // (stamp builds: waves with a record in the tile's colsum row)
  extern __shared__ __attribute__((aligned(16))) u16 smem16[];
  constexpr int B_LO = BN * XROW + 32, B_ELEMS = 2 * BN * XROW + 64;
  const int HWd = TW + p.ks - 1, HHt = TH + p.ks - 1, HP = HWd * HHt;
  char* const halo = reinterpret_cast<char*>(smem16);
  u16* const bsm = smem16 + ((HP * p.PXS + 127) & ~127) / 2;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (a scalar: wave-uniform tests and LDS-DMA destinations stay scalar code)
  int tile;
  {
    const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int tpi = p.tilesX * p.tilesY;
  const int img = tile / tpi, trem = tile - img * tpi;
  const int oy0 = (trem / p.tilesX) * TH, ox0 = (trem % p.tilesX) * TW;
  const int n0 = blockIdx.y * BN;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, (int)p.wp_bytes, 0x00020000);
  const int pixb = 4 * p.Cpi;

  // ---- halo: [pixel][hi CS][lo CS] at stride PXS; out-of-image pixels and channels >= Cpi read zeros.
  // Filled by LDS-DMA as one linear run of 16-byte vectors (PXS / 16 per pixel, the last ones pad): wave
  // instruction ii writes vectors [64 ii, 64 ii + 64), the per-lane source picks pixel / plane / channel.
  int cs_cur = p.nslabs == 1 ? p.CSl : p.CS;   // channels of the slab being multiplied (the last one may be narrower)
  int sps_cur = p.nslabs == 1 ? p.SPSl : p.SPS;
  const int VP = p.PXS / 16;                   // vectors per halo pixel with pad
  const int hvecs = HP * VP;
  const float invVP = 1.0f / (float)VP, invHW = 1.0f / (float)HWd;
  auto dma_halo = [&](int slab) {
    const int V = (slab == p.nslabs - 1 ? p.CSl : p.CS) / (AP == 1 ? 8 : 4);      // data vectors per halo pixel (AP planes x cs/8)
    for (int ii = wave; ii * 64 < hvecs; ii += NTHR / 64) {
      const int v = ii * 64 + lane;
      if (v < hvecs) {
        const int px = (int)(((float)v + 0.5f) * invVP), part = v - px * VP;     // exact: v < 2^13
        const int hy = (int)(((float)px + 0.5f) * invHW), hx = px - hy * HWd;
        const int iy = oy0 - p.pad + hy, ix = ox0 - p.pad + hx;
        const int plane = AP == 1 ? 0 : part >= (V >> 1), vec = part - plane * (V >> 1);
        const int ch = slab * p.CS + vec * 8;
        unsigned off = XOOB;
        if (part < V && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W && ch < p.Cpi)
          off = (unsigned)(((img * p.H + iy) * p.W + ix) * pixb + plane * 2 * p.Cpi + ch * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (__attribute__((address_space(3))) void*)(halo + ii * 1024), 16, off, 0, 0, 0);
      }
    }
  };

  // ---- weights: LDS-DMA (buffer_load ... lds), no staging registers and no ds_write pass.  One wave
  // instruction fills 16 cout rows x 64 B of one plane (1 KB, lane-linear destination: row 16*wave + lane/4,
  // 16-byte slot lane%4); the XOR swizzle of the slot goes on the per-lane SOURCE column.
  const int nstages = p.Kt / XKC;
  // row group = 16 cout rows; wave w fills groups w, w + NWV, ... (one each with 8 waves; up to two with 4)
  constexpr int NGMAX = (NT + NWV - 1) / NWV;
  const int ngroups = wave < NT ? (NT - wave + NWV - 1) / NWV : 0;       // wave-uniform
  unsigned dbase[NGMAX], dbase2[NGMAX];
#pragma unroll
  for (int q = 0; q < NGMAX; ++q) {
    const int drow = 16 * (wave + q * NWV) + (lane >> 2);
    const int dvq = (lane & 3) ^ ((drow >> 1) & 3);
    dbase[q] = (q < ngroups && n0 + drow < p.Np) ? (unsigned)(((n0 + drow) * 2 * p.Kt + dvq * 8) * 2) : XOOB;
    dbase2[q] = dbase[q] >= XOOB ? XOOB : dbase[q] + (unsigned)(p.Kt * 2);
  }
  // one row group (hi + lo plane: two wave instructions) of stage g's weights; one addition per instruction (the stage's
  // byte offset is a scalar; stages past the end add 2^30: valid rows -- the packed weights are a few MB -- and invalid
  // ones (2^31) alike land beyond the buffer, without wrapping)
  auto dma_b_group = [&](int g, int buf, int q) {
    if (q < ngroups) {
      const unsigned sg = g < nstages ? (unsigned)(g * XKC * 2) : 0x40000000u;
      const unsigned off = dbase[q] + sg;
      const unsigned off2 = dbase2[q] + sg;
      u16* d = bsm + buf * B_ELEMS + 16 * (wave + q * NWV) * XROW;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (__attribute__((address_space(3))) void*)d, 16, off, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (__attribute__((address_space(3))) void*)(d + B_LO), 16, off2, 0, 0, 0);
    }
  };
  auto dma_b = [&](int g, int buf) {
#pragma unroll
    for (int q = 0; q < NGMAX; ++q) dma_b_group(g, buf, q);
  };

  f32x4 acc[NT][2];
#pragma unroll
  for (int j = 0; j < NT; ++j) { acc[j][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  unsigned long long st_prev = 0, st_acc[6] = {0, 0, 0, 0, 0, 0}, st_rt[7] = {0, 0, 0, 0, 0, 0, 0};
  auto rstamp = [&](int i) {                   // (stamp builds) wall clock, 100 MHz: kernel entry / loop start / loop end / exit
    if (DBG & 64) {
      unsigned long long t;
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      st_rt[i] = t;
    }
  };
  rstamp(0);
  auto stamp = [&](int i) {
    if (DBG & 64) {
      unsigned long long t;
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      if (i >= 0) st_acc[i] += t - st_prev;
      st_prev = t;
    }
  };

  // ---- fragments: lane = pixel (lane & 15) of a 16-pixel row segment, k group kg = lane >> 4 (8 k each)
  const int frow = lane & 15, kg = lane >> 4;
  const int fslot = (kg ^ ((frow >> 1) & 3)) * 8;
  int abase[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pt = wave * 2 + i;
    abase[i] = ((pt / TPR) * HWd + (pt % TPR) * 16 + frow) * p.PXS;
  }
  int cl = kg * 8, tdx = 0, tdy = 0, aoff = cl * 2;      // this lane's (channel, tap) inside the slab
  int lo_off = cs_cur * 2;
  // Software pipeline inside every wave (stamps of the first version: all eight waves read fragments,
  // then all multiply -- 53 % MFMA issue occupancy; a two-group ping-pong did no better): the fragments of
  // stage g+1 are read WHILE the MFMAs of stage g issue, cout tile by cout tile into the registers the
  // tile's MFMAs have just consumed, so no wave ever waits for LDS with an idle matrix pipe.  NB weight
  // buffers: while stage g multiplies (its fragments are in registers), stage g+1 is read from its buffer and
  // the DMAs of stages g+2 .. g+NB-1 are in flight or landed (one stage of latency cover was not enough: stamps
  // showed 400 of 2340 cycles per stage waiting for the weights); each wave waits for its own share of stage
  // g+1 with a counted vmcnt before the stage barrier (no fence: a release fence would drain every DMA).
  bf16x8 ah[2], al[2], wh[NT], wl[NT];
  auto read_a = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ah[i] = *reinterpret_cast<const bf16x8*>(halo + abase[i] + aoff);
      if (AP == 2) al[i] = *reinterpret_cast<const bf16x8*>(halo + abase[i] + aoff + lo_off);
    }
    // the following stage's tap / channel of this lane (CS >= 32: at most one wrap); taps past ks*ks (slab
    // padding, zero weights) read the tile's first pixels
    cl += XKC;
    if (cl >= cs_cur) { cl -= cs_cur; if (++tdx == p.ks) { tdx = 0; ++tdy; } }
    aoff = tdy < p.ks ? (int)__umul24(__umul24((unsigned)tdy, (unsigned)HWd) + (unsigned)tdx, (unsigned)p.PXS) + cl * 2 : 0;
  };
  const u16* const bfrag = bsm + frow * XROW + fslot;
  auto read_b = [&](int buf, int j) {
    wh[j] = *reinterpret_cast<const bf16x8*>(bfrag + buf * B_ELEMS + j * 16 * XROW);
    wl[j] = *reinterpret_cast<const bf16x8*>(bfrag + buf * B_ELEMS + B_LO + j * 16 * XROW);
  };

#pragma unroll
  for (int b = 0; b < NB; ++b) dma_b(b, b);
  dma_halo(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  read_a();
#pragma unroll
  for (int j = 0; j < NT; ++j) read_b(0, j);
  int s_in = 0, slab = 0, bcur = 0;
  rstamp(1);
  stamp(-1);
  for (int g = 0; g < nstages; ++g) {
    const int b1 = bcur + 1 == NB ? 0 : bcur + 1;      // buffer of stage g+1; stage g's fragments are in registers
    // this wave's share of stage g+1 has landed; the NB-2 stages behind it (two DMA instructions each) stay in flight
    if (NGMAX == 1 || ngroups < 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NB - 2)) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (NB - 2)) : "memory");
    stamp(4);                                    // (stamp builds: slot 4 = the wait for this wave's own weight DMA)
    if (!(DBG & 16)) pw_barrier();               // ... everyone's; and everyone has read stage g's fragments
    stamp(0);
    if (!(DBG & 2)) dma_b(g + NB, bcur);           // (DBG & 2, timing only: no weight stream inside the loop)
    bcur = b1;
    stamp(5);                                    // weight DMA issued
    const bool last_of_slab = (s_in + 1 == sps_cur);
    // the fragments of a slab's last stage are in registers and the barrier above retired every read of the
    // halo: the next slab's halo lands while this stage multiplies
    if (last_of_slab && slab + 1 < p.nslabs && !(DBG & 4)) dma_halo(slab + 1);      // (DBG & 4, timing only: one halo per tile)
    stamp(1);
    // A fragments of stage g+1: with two workgroups per CU (8x16 tiles) they replace a pixel tile's registers as soon as its
    // last MFMAs of this stage have issued (LATE; reading them into a second register set during the first cout tile and
    // copying costs 8 v_mov_b64 per stage in a loop of 24 MFMAs that is bound by vector issue: 64 -> 64 at 128^2 43.3 -> 41.9
    // us); with ONE workgroup per CU (16x16 tiles, all eight waves in step) the early read hides the LDS latency that
    // nothing else covers there and stays (128 -> 128 at 64^2: 37 us early, 39-40 late).
    constexpr bool LATE = TH * TW <= 128;
    bf16x8 ahn[2], aln[2];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (!(DBG & 1)) {
          acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], ah[i], acc[j][i], 0, 0, 0);   // small terms first
          if (AP == 2) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], al[i], acc[j][i], 0, 0, 0);
          acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], ah[i], acc[j][i], 0, 0, 0);
        }
        if (LATE && j == NT - 1 && !last_of_slab && !(DBG & 8)) {
          ah[i] = *reinterpret_cast<const bf16x8*>(halo + abase[i] + aoff);
          if (AP == 2) al[i] = *reinterpret_cast<const bf16x8*>(halo + abase[i] + aoff + lo_off);
        }
      }
      if (!(DBG & 8)) read_b(b1, j);             // stage g+1, same cout tile, into the registers just consumed
      if (!LATE && j == 0 && !last_of_slab && !(DBG & 8)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          ahn[i] = *reinterpret_cast<const bf16x8*>(halo + abase[i] + aoff);
          if (AP == 2) aln[i] = *reinterpret_cast<const bf16x8*>(halo + abase[i] + aoff + lo_off);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    stamp(2);
    if (!last_of_slab) {
      if (!LATE) {
#pragma unroll
        for (int i = 0; i < 2; ++i) { ah[i] = ahn[i]; if (AP == 2) al[i] = aln[i]; }
      }
      cl += XKC;
      if (cl >= cs_cur) { cl -= cs_cur; if (++tdx == p.ks) { tdx = 0; ++tdy; } }
      aoff = tdy < p.ks ? (int)__umul24(__umul24((unsigned)tdy, (unsigned)HWd) + (unsigned)tdx, (unsigned)p.PXS) + cl * 2 : 0;
      ++s_in;
    } else {                                     // slab boundary: the next A fragments come from the next halo
      s_in = 0;
      ++slab;
      if (slab == p.nslabs - 1) { cs_cur = p.CSl; sps_cur = p.SPSl; lo_off = cs_cur * 2; }
      cl = kg * 8; tdx = 0; tdy = 0; aoff = cl * 2;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the new halo (and of stage g+2)
      __syncthreads();
      read_a();
    }
    stamp(3);                                // tail of the stage (slab boundaries included: halo wait + barrier + re-read)
  }
  // ---- epilogue operands: the bias of this lane's couts and the gate of its (pixel, cout) quads, as ONE batch of
  // unconditional buffer loads (out of range -> 0) issued before the drain.  (The first version loaded them one by one
  // inside the per-element branches: 56 global loads, each with its own full wait -- 11-12 us of a ~105 us tile.)
  const int fq = kg * 4;
  auto pix_of = [&](int pr, int& oy, int& ox) {
    const int pt = pr >> 4;
    oy = oy0 + pt / TPR; ox = ox0 + (pt % TPR) * 16 + (pr & 15);
    return oy < p.Ho && ox < p.Wo;
  };
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
  u32x2 gv[2][NT];                             // split gate: 4 hi-plane bf16 per quad; bit mask: one byte in .x
  bool okp[2]; int64_t mp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int oy, ox;
    okp[i] = pix_of(wave * 32 + i * 16 + frow, oy, ox);
    mp[i] = ((int64_t)img * p.Ho + oy) * p.Wo + ox;
  }
  if (use_gate) {
    const int64_t gbytes = (int64_t)p.N * p.Ho * p.Wo * 4 * p.Cpo;
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void*)p.gate, 0, (int)(gbytes < 0x7fffffff ? gbytes : 0x7fffffff), 0x00020000);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 16 + fq;
        gv[i][j] = __builtin_amdgcn_raw_buffer_load_b64(grs, (okp[i] && co < p.Cpo) ? (unsigned)((mp[i] * 2 * p.Cpo + co) * 2) : XOOB, 0, 0);
      }
  } else if (use_mask) {
    const int64_t mbytes = (int64_t)p.N * p.Ho * p.Wo * (p.Cpo >> 3);
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.gate_mask, 0, (int)mbytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 16 + fq;
        gv[i][j].x = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(mrs, (okp[i] && co < p.Cpo) ? (unsigned)(mp[i] * (p.Cpo >> 3) + (co >> 3)) : XOOB, 0, 0);
      }
  }
  const XAct ak = x_act(p.act, p.slope);
  const float gate_off = p.gate_act == WCMC_ACT_RELU ? 0.f : p.gate_act == WCMC_ACT_LEAKY_RELU ? p.gate_slope : 1.f;
  const int gkind = use_gate ? 1 : use_mask ? 2 : 0;
  rstamp(2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the (zero) weight stages past the end have landed:
  __syncthreads();                                     // LDS is free for the epilogue staging
  rstamp(3);
  if ((DBG & 32) && !(DBG & 64)) {                     // timing only: no epilogue (one store keeps the accumulators alive)
    float keep = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) keep += (acc[j][0][0] + acc[j][0][1] + acc[j][0][2] + acc[j][0][3]) +
                                         (acc[j][1][0] + acc[j][1][1] + acc[j][1][2] + acc[j][1][3]);
    if (keep == 12345.678f && p.ys) p.ys[0] = 1;
    return;
  }
  if (DBG & 64) {
    if (lane == 0 && wave < STW) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(p.colsum) + ((int64_t)tile * STW + wave) * 14;
      for (int i = 0; i < 6; ++i) o[i] = st_acc[i];
      for (int i = 0; i < 3; ++i) o[6 + i] = st_rt[i];
      unsigned hw;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      unsigned xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      o[13] = hw | ((unsigned long long)xcc << 32);
    }
  }

  // ---- epilogue (as the streaming kernel; pixels of the tile outside the image are written as zeros to LDS
  // and skipped on the way out).  Tile-local pixel pr = 16 * pixel-tile + column.
  if (p.ys) {
    constexpr int OLD = 2 * BN + 8;
    u16* so = smem16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pr = wave * 32 + i * 16 + frow;
      const bool ok = okp[i];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 16 + fq;
        float v[4];
        // (gate: the hi-plane predicate from the split tensor, or from the bit mask the producing launch left)
        x_epi_quad(acc[j][i], bv[j], ok, ak, gkind, gv[i][j], co, gate_off, v);
        unsigned h01, l01, h23, l23;
        x_split2(v[0], v[1], h01, l01);
        x_split2(v[2], v[3], h23, l23);
        *reinterpret_cast<uint2*>(so + pr * OLD + j * 16 + fq) = make_uint2(h01, h23);
        *reinterpret_cast<uint2*>(so + pr * OLD + BN + j * 16 + fq) = make_uint2(l01, l23);
      }
    }
    __syncthreads();
    rstamp(4);
    constexpr int VPP = BN / 8;
    for (int v = tid; v < TPX * 2 * VPP; v += NTHR) {
      const int pr = v / (2 * VPP), q = v - pr * (2 * VPP);
      const int plane = q >= VPP, vec = q - plane * VPP;
      const int co = n0 + vec * 8;
      int oy, ox;
      if (pix_of(pr, oy, ox) && co < p.Cpo) {
        const int64_t m = ((int64_t)img * p.Ho + oy) * p.Wo + ox;
        const u32x4 hv = *reinterpret_cast<const u32x4*>(so + pr * OLD + plane * BN + vec * 8);
        *reinterpret_cast<u32x4*>(p.ys + m * 2 * p.Cpo + plane * p.Cpo + co) = hv;
        if (p.mask_out && plane == 0) p.mask_out[m * (p.Cpo >> 3) + (co >> 3)] = positive_mask8(hv);
      }
    }
    rstamp(5);
    if (!(DBG & 64) && p.colsum) {
      constexpr int CW = BN <= 16 ? 16 : BN <= 32 ? 32 : BN <= 64 ? 64 : 128, RG = NTHR / CW;
      float* red = reinterpret_cast<float*>(so + TPX * OLD);
      const int c = tid % CW, rg = tid / CW;
      float a = 0.f;
      if (c < BN)
        for (int r = rg; r < TPX; r += RG) a += bf2f(so[r * OLD + c]) + bf2f(so[r * OLD + BN + c]);
      if (rg > 0 && c < BN) red[(rg - 1) * BN + c] = a;
      __syncthreads();
      if (rg == 0 && c < BN && n0 + c < p.Np) {
        for (int q = 0; q < RG - 1; ++q) a += red[q * BN + c];
        p.colsum[(int64_t)tile * p.Np + n0 + c] = a;
        // trailer: the number of rows this launch wrote (the finish kernel reads no further)
        if (tile == 0 && n0 + c == 0) reinterpret_cast<int*>(p.colsum)[(int64_t)p.G * p.Np] = (int)gridDim.x;
      }
    }
  } else {
    constexpr int OLD = BN + 4;
    float* so = reinterpret_cast<float*>(smem16);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pr = wave * 32 + i * 16 + frow;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 16 + fq;
        float v[4];
        x_epi_quad(acc[j][i], bv[j], true, ak, 0, u32x2{0u, 0u}, co, 1.f, v);
        *reinterpret_cast<float4*>(so + pr * OLD + j * 16 + fq) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    __syncthreads();
    constexpr int VPP = BN / 4;
    for (int v = tid; v < TPX * VPP; v += NTHR) {
      const int pr = v / VPP, vec = v - pr * VPP;
      const int co = n0 + vec * 4;
      int oy, ox;
      if (pix_of(pr, oy, ox) && co < p.Cpo)
        *reinterpret_cast<float4*>(p.yf + (int64_t)img * p.ysn + (int64_t)oy * p.ysh + (int64_t)ox * p.ysw + co) =
            *reinterpret_cast<const float4*>(so + pr * OLD + vec * 4);
    }
  }
  if (DBG & 64) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the stores have left)
    rstamp(6);
    if (lane == 0 && wave < STW) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(p.colsum) + ((int64_t)tile * STW + wave) * 14;
      for (int i = 3; i < 7; ++i) o[6 + i] = st_rt[i];
    }
  }
}

}  // namespace wcmc

using namespace wcmc;

static size_t xh_bstage_bytes(int nt) { return (size_t)(2 * nt * 16 * XROW + 64) * sizeof(u16); }      // one weight stage
namespace wcmc {
// halo plans of the 64-pixel 5x5 kernel (bf16x3_halo64.hip)
bool x_halo_is64(const XIgemmParams& p) {
  return (p.CS == 16 || p.ap == 1 ||
          (p.CS == 32 && p.PXS == 160 && p.CSl == 32 && p.Kp >= 256 && x_env_on("WCMC_HALO64") && x_env_on("WCMC_HALO64_CS32"))) &&
         p.ks == 5;
}
int x_plan_halo(int nt, const XIgemmParams& p, XHaloPlan* h) {
  constexpr int TH = 16, TW = 16;
  const int HP = (TH + p.ks - 1) * (TW + p.ks - 1);
  const size_t halo = (size_t)((HP * p.PXS + 127) & ~127), bstage = xh_bstage_bytes(nt);
  const size_t lds_out = p.ys ? (size_t)256 * (2 * nt * 16 + 8) * sizeof(u16) + (size_t)32 * nt * 16 * sizeof(float)
                              : (size_t)256 * (nt * 16 + 4) * sizeof(float);
  // three weight stages (two stages of DMA latency cover) where LDS allows, else two
  const char* nbe = ab_env("WCMC_HALO_NB");
  const int nbmax = (nbe && nbe[0] == '2') ? 2 : 3;
  const int nb = (nbmax >= 3 && halo + 3 * bstage <= 160 * 1024) ? 3 : 2;
  const size_t lds_main = halo + nb * bstage;
  const size_t lds = lds_main > lds_out ? lds_main : lds_out;
  WCMC_REQUIRE(lds <= 160 * 1024, WCMC_ERR_BAD_ARG, "conv2d_igemm_bf16x3: halo tile does not fit in LDS");
  h->nt = nt;
  h->ap = ((nt == 4 || nt == 7) && p.ap == 1) ? 1 : 2;      // (x_plan_k grants ap = 1 to this kernel for ks = 3 and nt = 4 or 7 only)
  // ... and for any launch whose 16x16 tiling has fewer workgroups than the chip has CUs (the deepest U-Net level: 32 tiles
  // x 4 cout blocks), where half-size tiles simply fill the machine (<= 4 cout tiles: one wave per weight row group pair)
  const int64_t blocks16 = (int64_t)p.N * p.tilesX * p.tilesY * ((p.Np / 16 + nt - 1) / nt);
  // ... and, measured (scripts/time_unet_layers.py), where the 16x16 tiling is two or more rounds (the 128^2 level: 512
  // tiles): two 128-pixel workgroups per CU with their own stage barriers instead of one of 256 -- 46.8 -> 43.5 us
  const bool underfilled = nt <= 4 && (blocks16 < 256 || blocks16 >= 512) && p.Ho >= 16;
  if ((p.PXS == 160 && p.ks == 5) || underfilled) {
    // WCMC_HALO_TH8_5X5 plan (32-channel slabs): 8x16-pixel tiles, four waves, TWO workgroups per CU -- their stage
    // barriers are independent, so the non-MFMA phases of one hide behind the MFMAs of the other
    constexpr int TH8 = 8;
    const size_t halo8 = (size_t)(((TH8 + p.ks - 1) * (TW + p.ks - 1) * p.PXS + 127) & ~127);
    const size_t out8 = p.ys ? (size_t)TH8 * TW * (2 * nt * 16 + 8) * sizeof(u16) + (size_t)32 * nt * 16 * sizeof(float)
                             : (size_t)TH8 * TW * (nt * 16 + 4) * sizeof(float);
    // (three weight stages, which still fit beside the second workgroup for <= 4 cout tiles, measured no faster on the
    // U-Net's 3x3 layers, nor five in the 16x16 tiling: wall-clock stamps show 15 us in the stage loop of 64 -> 64 at
    // 128^2 for 7 us of MFMAs, but the DMA is not what the stages wait for -- scripts/timeline_halo.py --unet)
    const size_t main8 = halo8 + 2 * bstage;
    h->th = TH8; h->nb = 2; h->tilesY = (p.Ho + TH8 - 1) / TH8; h->lds = main8 > out8 ? main8 : out8;
  } else {
    h->th = TH; h->nb = nb; h->tilesY = p.tilesY; h->lds = lds;
  }
  return 0;
}
}  // namespace wcmc

template <int NT, int TH, int NB, int AP = 2>
static int launch_xhalo2(const XHaloPlan& h, const XIgemmParams& p, hipStream_t stream) {
  constexpr int TW = 16;
  WCMC_REQUIRE(h.nt == NT && h.th == TH && h.nb == NB && h.ap == AP, WCMC_ERR_LAUNCH, "conv2d_igemm_bf16x3(halo): no instance for the plan");
  static LdsAttr attr;
  if (set_max_lds(reinterpret_cast<const void*>(&conv_halo_bf16x3_kernel<NT, TH, TW, 0, NB, AP>), h.lds, attr) != hipSuccess) return WCMC_ERR_LAUNCH;
  XIgemmParams q = p;
  q.tilesY = h.tilesY;
  const dim3 grid((unsigned)(q.N * q.tilesX * q.tilesY), (unsigned)((q.Np / 16 + NT - 1) / NT));
  hipLaunchKernelGGL((conv_halo_bf16x3_kernel<NT, TH, TW, 0, NB, AP>), grid, dim3(TH * TW * 2), h.lds, stream, q);
  return check_launch(TH == 16 ? "conv2d_igemm_bf16x3(halo)" : AP == 1 ? "conv2d_igemm_bf16x3(halo, 8x16, x hi plane)" : "conv2d_igemm_bf16x3(halo, 8x16)");
}
template <int NT>
static int launch_xhalo(const XHaloPlan& h, const XIgemmParams& p, hipStream_t stream) {
#ifdef WCMC_DEBUG_BUILD
  constexpr int TW = 16;
  const size_t bstage = xh_bstage_bytes(NT);
  if (NT == 7 && p.PXS == 160 && p.ks == 5) {
    int ab;                             // (read per call: scripts interleave the modes inside one process)
    { const char* e = ab_env("WCMC_DEBUG_ABLATE"); ab = e ? atoi(e) : 0; }
    if (ab == 1 || ab == 2 || ab == 4 || ab == 8 || ab == 16 || ab == 10 || ab == 26 || ab == 18 || ab == 27 || ab == 31 || ab == 59 || ab == 63 || ab == 32) {
      // timing only (WRONG results): 1 = no MFMA, 2 = no weight DMA in the stage loop, 8 = no fragment reads, 16 = no stage
      // barrier, 4 = one halo per tile (no slab reloads), 32 = no epilogue; sums combine (27 = empty stage loop)
      constexpr int TH8 = 8;
      XIgemmParams q = p;
      q.tilesY = (p.Ho + TH8 - 1) / TH8;
      const size_t halo8 = (size_t)(((TH8 + p.ks - 1) * (TW + p.ks - 1) * p.PXS + 127) & ~127);
      const dim3 grid((unsigned)(q.N * q.tilesX * q.tilesY), (unsigned)((q.Np / 16 + NT - 1) / NT));
      auto kfn = ab == 4 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 4, 2> : ab == 1 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 1, 2> : ab == 2 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 2, 2>
                 : ab == 8 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 8, 2> : ab == 16 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 16, 2>
                 : ab == 10 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 10, 2> : ab == 18 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 18, 2>
                 : ab == 27 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 27, 2> : ab == 31 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 31, 2>
                 : ab == 59 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 59, 2> : ab == 63 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 63, 2>
                 : ab == 32 ? &conv_halo_bf16x3_kernel<7, TH8, TW, 32, 2>
                 : &conv_halo_bf16x3_kernel<7, TH8, TW, 26, 2>;
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      hipLaunchKernelGGL(kfn, grid, dim3(TH8 * TW * 2), halo8 + 2 * bstage, stream, q);
      return check_launch("conv2d_igemm_bf16x3(halo 8x16, ablation)");
    }
    if (ab == 64) {      // stamp build of the shipped 8x16 tiling (scripts/stamp_igemm.py)
      constexpr int TH8 = 8;
      XIgemmParams q = p;
      q.tilesY = (p.Ho + TH8 - 1) / TH8;
      const size_t halo8 = (size_t)(((TH8 + p.ks - 1) * (TW + p.ks - 1) * p.PXS + 127) & ~127);
      const dim3 grid((unsigned)(q.N * q.tilesX * q.tilesY), (unsigned)((q.Np / 16 + NT - 1) / NT));
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo_bf16x3_kernel<7, TH8, TW, 64, 2>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      hipLaunchKernelGGL((conv_halo_bf16x3_kernel<7, TH8, TW, 64, 2>), grid, dim3(TH8 * TW * 2), halo8 + 2 * bstage, stream, q);
      return check_launch("conv2d_igemm_bf16x3(halo 8x16, stamps)");
    }
  }
  if (NT == 4 && p.ks == 3) {        // wall-clock stamps of the U-Net 3x3 launches, 8x16 tiling (scripts/timeline_halo.py --unet)
    const char* e = ab_env("WCMC_DEBUG_ABLATE");
    if (e && atoi(e) == 64) {
      constexpr int TH8 = 8;
      XIgemmParams q = p;
      q.tilesY = (p.Ho + TH8 - 1) / TH8;
      const size_t halo8 = (size_t)(((TH8 + p.ks - 1) * (TW + p.ks - 1) * p.PXS + 127) & ~127);
      const size_t out8 = (size_t)TH8 * TW * (2 * NT * 16 + 8) * sizeof(u16) + (size_t)32 * NT * 16 * sizeof(float);
      const size_t main8 = halo8 + 2 * bstage;
      const dim3 grid((unsigned)(q.N * q.tilesX * q.tilesY), (unsigned)((q.Np / 16 + NT - 1) / NT));
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo_bf16x3_kernel<4, TH8, TW, 64, 2>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      hipLaunchKernelGGL((conv_halo_bf16x3_kernel<4, TH8, TW, 64, 2>), grid, dim3(TH8 * TW * 2), main8 > out8 ? main8 : out8, stream, q);
      return check_launch("conv2d_igemm_bf16x3(halo 8x16 3x3, stamps)");
    }
  }
#endif
  if constexpr (NT == 4 || NT == 7) {
    if (h.ap == 1) return h.th == 8 ? launch_xhalo2<NT, 8, 2, 1>(h, p, stream) : h.nb == 3 ? launch_xhalo2<NT, 16, 3, 1>(h, p, stream) : launch_xhalo2<NT, 16, 2, 1>(h, p, stream);
  }
  return h.th == 8 ? launch_xhalo2<NT, 8, 2>(h, p, stream) : h.nb == 3 ? launch_xhalo2<NT, 16, 3>(h, p, stream) : launch_xhalo2<NT, 16, 2>(h, p, stream);
}
namespace wcmc {
int launch_xhalo(const XHaloPlan& h, const XIgemmParams& p, hipStream_t stream) {
  switch (h.nt) {
    case 7: return ::launch_xhalo<7>(h, p, stream);
    case 4: return ::launch_xhalo<4>(h, p, stream);
    case 2: return ::launch_xhalo<2>(h, p, stream);
    default: return ::launch_xhalo<1>(h, p, stream);
  }
}
}  // namespace wcmc
