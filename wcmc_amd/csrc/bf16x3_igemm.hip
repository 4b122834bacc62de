// Split-bf16 convolution, streaming implicit GEMM (conv_igemm_bf16x3_kernel): the layers without a halo plan (x_plan_k).
#include "bf16x3_common.h"

namespace wcmc {

// ------------------------------------------------------------------ implicit GEMM (fwd + dgrad)
// PMC profile of the first version (profiles/): 97 % L2 hits, but 3.3 VALU + 1.5 SALU per MFMA, half of
// the LDS cycles bank conflicts, 37 % of wave time parked on vmcnt/barrier.  Hence:
//   * operand loads are buffer loads: out-of-image taps / rows past the tensor use an out-of-range
//     offset and the hardware returns zeros (no branches, no zero-fill moves, 32-bit offsets);
//   * LDS rows are 64 B (one 32-k stage of one plane) with the 16-byte slot XOR-swizzled by
//     (row >> 1) & 3 and the lo plane shifted by 64 B: ds_read_b128 and ds_write_b128 conflict-free;
//   * the register prefetch runs TWO stages ahead of the MFMAs.

// DBUF: two LDS stage buffers and one barrier per stage (2 workgroups per CU), or one buffer and two
// barriers per stage (3 workgroups per CU = 3 waves per SIMD to cover the barriers and LDS latency).
// DBG (timing-only ablations, results are wrong): 1 = no MFMA, 2 = no LDS stores, 8 = no LDS fragment
// reads, 16 = no barriers.  DBG = 0 is the product kernel.
template <int NT, bool PADDED, bool DBUF, int DBG = 0>
__global__ __launch_bounds__(256, DBUF ? 2 : 3) void conv_igemm_bf16x3_kernel(XIgemmParams p) {
  constexpr int BN = NT * 16;
  constexpr int NJ = (BN + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) u16 smem16[];
  // per buffer (u16 units): A hi [XBM][32], A lo at +XBM*32+32 (64 B shift), then B hi / B lo likewise
  constexpr int A_LO = XBM * XROW + 32, A_ELEMS = 2 * XBM * XROW + 64;
  constexpr int B_LO = BN * XROW + 32, B_ELEMS = 2 * BN * XROW + 64;
  constexpr int BUF = A_ELEMS + B_ELEMS;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (a scalar: wave-uniform tests and LDS-DMA destinations stay scalar code)
  // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (private 4 MB L2 each), so
  // give each XCD one contiguous run of pixel tiles (speed only, any placement is correct).
  int tile;
  {
    const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int64_t m0 = (int64_t)tile * XBM;
  const int n0 = blockIdx.y * BN;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, (int)p.wp_bytes, 0x00020000);

  // loader mapping: 8 consecutive threads = one row's 2 planes x 4 vectors of 8 bf16
  const int vq = tid & 3, pl = (tid >> 2) & 1, prow = tid >> 3;
  unsigned abase[4]; int aiy[4], aix[4];
  const int64_t HoWo = (int64_t)p.Ho * p.Wo;
  const int pixb = 4 * p.Cpi;                           // bytes per input pixel (2 planes of bf16)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t m = m0 + prow + 32 * j;
    if (m < p.M) {
      const int n = (int)(m / HoWo);
      const int r = (int)(m - (int64_t)n * HoWo);
      const int oy = r / p.Wo, ox = r - oy * p.Wo;
      aiy[j] = oy - p.pad; aix[j] = ox - p.pad;
      abase[j] = (unsigned)((((int64_t)n * p.H + aiy[j]) * p.W + aix[j]) * pixb + pl * 2 * p.Cpi);
    } else {
      aiy[j] = -(1 << 28); aix[j] = -(1 << 28); abase[j] = XOOB;      // stays out of range for every tap
    }
  }
  unsigned wbase[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int nrow = prow + 32 * j;
    wbase[j] = (nrow < BN && n0 + nrow < p.Np) ? (unsigned)((((n0 + nrow) * 2 + pl) * p.Kt + vq * 8) * 2) : XOOB;
  }
  int ci = vq * 8, tdy = 0, tdx = 0;
  while (ci >= p.Kp) { ci -= p.Kp; if (++tdx == p.ks) { tdx = 0; ++tdy; } }
  const int nchunks = p.Kt / XKC;

  auto load_chunk = [&](int c, u32x4* ra, u32x4* rb) {
    // taps past ks*ks fall outside the tensor (or hit zero weights): no tap predicate needed.
    // Stages past the end (the K loop is run in pairs) load nothing: out-of-range offsets.
    const unsigned kill = c < nchunks ? 0u : XOOB;
    const unsigned toff = (unsigned)((tdy * p.W + tdx) * pixb + ci * 2) | kill;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned off = abase[j] + toff;
      if (PADDED) {
        const int iy = aiy[j] + tdy, ix = aix[j] + tdx;
        off = ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) ? off : XOOB;
      }
      if (DBG & 4) ra[j] = u32x4{off, 0u, 0u, 0u};             // ablation: no A-operand load instruction at all
      else ra[j] = __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (DBG & 32) rb[j] = u32x4{wbase[j], 0u, 0u, 0u};       // ablation: no B-operand load instruction
      else rb[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, (wbase[j] + (unsigned)(c * XKC * 2)) | kill, 0, 0);
    }
    ci += XKC;
    while (ci >= p.Kp) { ci -= p.Kp; if (++tdx == p.ks) { tdx = 0; ++tdy; } }
  };
  const int wslot = (vq ^ ((prow >> 1) & 3)) * 8;       // swizzled 16-byte slot of this thread's vector
  auto store_chunk = [&](int buf, const u32x4* ra, const u32x4* rb) {
    if (DBG & 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(ra[j]));
#pragma unroll
      for (int j = 0; j < NJ; ++j) asm volatile("" ::"v"(rb[j]));
      return;
    }
    u16* a = smem16 + buf * BUF + pl * A_LO + wslot;
    u16* b = smem16 + buf * BUF + A_ELEMS + pl * B_LO + wslot;
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x4*>(a + (prow + 32 * j) * XROW) = ra[j];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int nrow = prow + 32 * j;
      if (nrow < BN) *reinterpret_cast<u32x4*>(b + nrow * XROW) = rb[j];
    }
  };

  f32x4 acc[NT][2];
#pragma unroll
  for (int j = 0; j < NT; ++j) { acc[j][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  // DBG & 64: in-kernel stamps (s_memtime) accumulate per-phase cycles of every wave into p.colsum
  // reinterpreted as u64 [tile][wave][8] (diagnostic build: read the shares, not the run time).
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

  const int frow = lane & 15;
  const int fslot = ((lane >> 4) ^ ((frow >> 1) & 3)) * 8;   // MFMA 16x16x32: lane holds k = 8*(lane>>4) .. +7
  auto compute = [&](int buf) {
    const u16* a = smem16 + buf * BUF + (wave * 32 + frow) * XROW + fslot;
    const u16* b = smem16 + buf * BUF + A_ELEMS + frow * XROW + fslot;
    // every fragment read of the stage is issued before the first MFMA (hipcc otherwise emits
    // read -> lgkmcnt(0) -> 6 MFMAs per cout tile and exposes the LDS latency seven times per stage)
    bf16x8 ah[2], al[2], wh[NT], wl[NT];
    if (DBG & 8) {
      const bf16x8 z = __builtin_bit_cast(bf16x8, u32x4{(unsigned)lane, 0u, 0u, 0u});
#pragma unroll
      for (int i = 0; i < 2; ++i) { ah[i] = z; al[i] = z; }
#pragma unroll
      for (int j = 0; j < NT; ++j) { wh[j] = z; wl[j] = z; }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = *reinterpret_cast<const bf16x8*>(a + i * 16 * XROW);
        al[i] = *reinterpret_cast<const bf16x8*>(a + A_LO + i * 16 * XROW);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        wh[j] = *reinterpret_cast<const bf16x8*>(b + j * 16 * XROW);
        wl[j] = *reinterpret_cast<const bf16x8*>(b + B_LO + j * 16 * XROW);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    stamp(1);                                // fragment reads issued and returned
    if (DBG & 1) {
#pragma unroll
      for (int i = 0; i < 2; ++i) { asm volatile("" ::"v"(ah[i])); asm volatile("" ::"v"(al[i])); }
#pragma unroll
      for (int j = 0; j < NT; ++j) { asm volatile("" ::"v"(wh[j])); asm volatile("" ::"v"(wl[j])); }
      return;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], ah[i], acc[j][i], 0, 0, 0);   // small terms first
        acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], al[i], acc[j][i], 0, 0, 0);
        acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], ah[i], acc[j][i], 0, 0, 0);
      }
    }
  };

  // prologue: stage 0 in LDS, stage 1 in flight in the second register set
  u32x4 ra0[4], rb0[NJ], ra1[4], rb1[NJ];
  load_chunk(0, ra0, rb0);
  load_chunk(1, ra1, rb1);
  store_chunk(0, ra0, rb0);
  __syncthreads();
  if (DBUF) {
    // Straight-line body, two stages per trip (a stage past the end multiplies zeros): no branch
    // between a load and its use, so hipcc's vmcnt bookkeeping keeps both register sets in flight.
    stamp(-1);
    for (int c = 0; c < nchunks; c += 2) {
      load_chunk(c + 2, ra0, rb0);          // set 0 is free; set 1 holds stage c+1
      stamp(0);                             // global loads issued
      compute(0);                           // stage c from LDS buffer 0
      stamp(2);                             // MFMAs issued
      store_chunk(1, ra1, rb1);
      stamp(3);                             // vmcnt wait + LDS stores
      if (!(DBG & 16)) __syncthreads();
      stamp(4);                             // barrier
      load_chunk(c + 3, ra1, rb1);          // set 1 is free; set 0 holds stage c+2
      stamp(0);
      compute(1);                           // stage c+1 from LDS buffer 1
      stamp(2);
      store_chunk(0, ra0, rb0);
      stamp(3);
      if (!(DBG & 16)) __syncthreads();
      stamp(4);
    }
    if (DBG & 64) {
      if (lane == 0) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(p.colsum) + ((int64_t)tile * 4 + wave) * 8;
        for (int i = 0; i < 5; ++i) o[i] = st_acc[i];
        o[5] = st_prev; o[6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_ID
      }
    }
  } else {
    for (int c = 0; c < nchunks; c += 2) {
      if (c + 2 < nchunks) load_chunk(c + 2, ra0, rb0);
      compute(0);
      __syncthreads();                                   // every wave has read stage c
      if (c + 1 >= nchunks) break;
      store_chunk(0, ra1, rb1);
      __syncthreads();
      if (c + 3 < nchunks) load_chunk(c + 3, ra1, rb1);
      compute(0);
      __syncthreads();
      if (c + 2 < nchunks) { store_chunk(0, ra0, rb0); __syncthreads(); }
    }
  }

  // ---- epilogue: lane holds couts n0 + j*16 + 4*(lane>>4) + {0..3} of pixel (lane&15).
  // Bias / activation / gate in registers, then the tile goes through LDS (free after the last
  // barrier) so that HBM sees whole 16-byte-per-lane contiguous rows instead of 8-byte fragments.
  const int fq = (lane >> 4) * 4;
  if (p.ys) {
    constexpr int OLD = 2 * BN + 8;                      // bf16 per LDS pixel row: [hi BN][lo BN] + pad
    u16* so = smem16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pr = wave * 32 + i * 16 + frow;
      const int64_t m = m0 + pr;
      const u16* gp = (p.gate && m < p.M) ? p.gate + (int64_t)m * 2 * p.Cpo : nullptr;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 16 + fq;
        float v[4] = {acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (co + e < p.Cout) {
            if (p.bias) v[e] += p.bias[co + e];
            v[e] = act_apply(v[e], p.act, p.slope);
          } else {
            v[e] = 0.f;
          }
        }
        if (gp && co < p.Cpo) {
          const uint2 g2 = *reinterpret_cast<const uint2*>(gp + co);
          const u16 g[4] = {(u16)(g2.x & 0xffff), (u16)(g2.x >> 16), (u16)(g2.y & 0xffff), (u16)(g2.y >> 16)};
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= act_gate(bf2f(g[e]), p.gate_act, p.gate_slope);
        }
        else if (p.gate_mask && m < p.M && co < p.Cpo && p.gate_act != WCMC_ACT_LINEAR) {
          // the same predicate (hi plane > 0) from the bit mask the producing launch left: 1/16 of the bytes
          const unsigned bits = (unsigned)p.gate_mask[m * (p.Cpo >> 3) + (co >> 3)] >> (co & 7);
          const float off = p.gate_act == WCMC_ACT_LEAKY_RELU ? p.gate_slope : 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= ((bits >> e) & 1u) ? 1.f : off;
        }
        u16 hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) split1(v[e], hi[e], lo[e]);
        *reinterpret_cast<uint2*>(so + pr * OLD + j * 16 + fq) =
            make_uint2((unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16));
        *reinterpret_cast<uint2*>(so + pr * OLD + BN + j * 16 + fq) =
            make_uint2((unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16));
      }
    }
    __syncthreads();
    constexpr int VPP = BN / 8;                          // 16-byte vectors per plane per pixel
    for (int v = tid; v < XBM * 2 * VPP; v += 256) {
      const int pr = v / (2 * VPP), q = v - pr * (2 * VPP);
      const int plane = q >= VPP, vec = q - plane * VPP;
      const int64_t m = m0 + pr;
      const int co = n0 + vec * 8;
      if (m < p.M && co < p.Cpo) {
        const u32x4 hv = *reinterpret_cast<const u32x4*>(so + pr * OLD + plane * BN + vec * 8);
        *reinterpret_cast<u32x4*>(p.ys + (int64_t)m * 2 * p.Cpo + plane * p.Cpo + co) = hv;
        if (p.mask_out && plane == 0) p.mask_out[m * (p.Cpo >> 3) + (co >> 3)] = positive_mask8(hv);
      }
    }
    if (!(DBG & 64) && p.colsum) {
      // bias gradient of the consumer layer for free: column sums of this tile (hi + lo) while it is in LDS;
      // RG row groups per column, combined through LDS in a fixed order
      constexpr int CW = BN <= 16 ? 16 : BN <= 32 ? 32 : BN <= 64 ? 64 : 128, RG = 256 / CW;
      float* red = reinterpret_cast<float*>(so + XBM * OLD);
      const int c = tid % CW, rg = tid / CW;
      const int rows = (int)min((int64_t)XBM, p.M - m0);
      float a = 0.f;
      if (c < BN)
        for (int r = rg; r < rows; r += RG) a += bf2f(so[r * OLD + c]) + bf2f(so[r * OLD + BN + c]);
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
    constexpr int OLD = BN + 4;                          // floats per LDS pixel row
    float* so = reinterpret_cast<float*>(smem16);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pr = wave * 32 + i * 16 + frow;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 16 + fq;
        float v[4] = {acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (co + e < p.Cout) {
            if (p.bias) v[e] += p.bias[co + e];
            v[e] = act_apply(v[e], p.act, p.slope);
          } else {
            v[e] = 0.f;
          }
        }
        *reinterpret_cast<float4*>(so + pr * OLD + j * 16 + fq) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    __syncthreads();
    constexpr int VPP = BN / 4;                          // float4 per pixel
    for (int v = tid; v < XBM * VPP; v += 256) {
      const int pr = v / VPP, vec = v - pr * VPP;
      const int64_t m = m0 + pr;
      const int co = n0 + vec * 4;
      if (m < p.M && co < p.Cpo) {                       // Cpo = round_up(Cout, 4) here
        const int n = (int)(m / HoWo);
        const int r = (int)(m - (int64_t)n * HoWo);
        const int oy = r / p.Wo, ox = r - oy * p.Wo;
        *reinterpret_cast<float4*>(p.yf + (int64_t)n * p.ysn + (int64_t)oy * p.ysh + (int64_t)ox * p.ysw + co) =
            *reinterpret_cast<const float4*>(so + pr * OLD + vec * 4);
      }
    }
  }
}

template <int NT, bool PADDED, bool DBUF>
static int launch_xigemm3(const XIgemmParams& p, hipStream_t stream) {
  const size_t lds_stage = (size_t)(DBUF ? 2 : 1) * (2 * XBM * XROW + 64 + 2 * NT * 16 * XROW + 64) * sizeof(u16);
  const size_t lds_out = (size_t)XBM * (2 * NT * 16 + 8) * sizeof(u16) + (size_t)16 * NT * 16 * sizeof(float);   // epilogue staging tile + column-sum partials
  const size_t lds = lds_stage > lds_out ? lds_stage : lds_out;
  static LdsAttr attr_set;
  if (set_max_lds(reinterpret_cast<const void*>(&conv_igemm_bf16x3_kernel<NT, PADDED, DBUF>), (size_t)lds, attr_set) != hipSuccess) return WCMC_ERR_LAUNCH;
  const dim3 grid((unsigned)ceil_div64(p.M, XBM), (unsigned)((p.Np / 16 + NT - 1) / NT));
  hipLaunchKernelGGL((conv_igemm_bf16x3_kernel<NT, PADDED, DBUF>), grid, dim3(256), lds, stream, p);
  return check_launch("conv2d_igemm_bf16x3");
}
#ifdef WCMC_DEBUG_BUILD
template <int DBG>
static int launch_xigemm_dbg(const XIgemmParams& p, hipStream_t stream) {
  const size_t lds = (size_t)2 * (2 * XBM * XROW + 64 + 2 * 7 * 16 * XROW + 64) * sizeof(u16);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_bf16x3_kernel<7, false, true, DBG>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const dim3 grid((unsigned)ceil_div64(p.M, XBM), (unsigned)((p.Np / 16 + 6) / 7));
  hipLaunchKernelGGL((conv_igemm_bf16x3_kernel<7, false, true, DBG>), grid, dim3(256), lds, stream, p);
  return check_launch("conv2d_igemm_bf16x3(ablation)");
}
#endif
template <int NT, bool PADDED>
static int launch_xigemm2(const XIgemmPlan& g, const XIgemmParams& p, hipStream_t stream) {
#ifdef WCMC_DEBUG_BUILD
  if (NT == 7 && !PADDED) {       // WCMC_DEBUG_ABLATE=<mask>: timing-only ablation builds of the 5x5 forward GEMM
    static int ab = -1;
    if (ab < 0) { const char* e = ab_env("WCMC_DEBUG_ABLATE"); ab = e ? atoi(e) : 0; }
    switch (ab) {
      case 1: return launch_xigemm_dbg<1>(p, stream);
      case 2: return launch_xigemm_dbg<2>(p, stream);
      case 8: return launch_xigemm_dbg<8>(p, stream);
      case 16: return launch_xigemm_dbg<16>(p, stream);
      case 10: return launch_xigemm_dbg<10>(p, stream);
      case 26: return launch_xigemm_dbg<26>(p, stream);
      case 4: return launch_xigemm_dbg<4>(p, stream);
      case 32: return launch_xigemm_dbg<32>(p, stream);
      case 36: return launch_xigemm_dbg<36>(p, stream);
      case 62: return launch_xigemm_dbg<62>(p, stream);
      case 64: return launch_xigemm_dbg<64>(p, stream);
      default: break;
    }
  }
#endif
  return g.dbuf ? launch_xigemm3<NT, PADDED, true>(p, stream) : launch_xigemm3<NT, PADDED, false>(p, stream);
}

template <int NT>
static int launch_xigemm(const XIgemmPlan& g, const XIgemmParams& p, hipStream_t stream) {
  return g.padded ? launch_xigemm2<NT, true>(g, p, stream) : launch_xigemm2<NT, false>(g, p, stream);
}
XIgemmPlan x_plan_igemm(int nt, const XIgemmParams& p) {
  return XIgemmPlan{nt, p.pad > 0 ? 1 : 0, x_env_on("WCMC_IGEMM_DBUF")};      // WCMC_IGEMM_DBUF=0 (debug build): A/B switch to the single buffer
}
int launch_xigemm(const XIgemmPlan& g, const XIgemmParams& p, hipStream_t stream) {
  switch (g.nt) {
    case 7: return launch_xigemm<7>(g, p, stream);
    case 4: return launch_xigemm<4>(g, p, stream);
    case 2: return launch_xigemm<2>(g, p, stream);
    default: return launch_xigemm<1>(g, p, stream);
  }
}

}  // namespace wcmc
