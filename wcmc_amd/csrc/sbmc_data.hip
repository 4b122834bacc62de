// The data step of the sample-based denoisers (SBMC / LBMC interfaces): the per-sample buffers and their patch batches.
//
// Replaces the numpy code of the reference's support/datasets.py:
//   DenoiseDataset._preprocess_sbmc :363-485   raw (h,w,s,C) -> sbmc_s (h,w,s,27) and sbmc_p (h,w,s,11*(MAX_DEPTH+1) = 66)
//   DenoiseDataset.__getitem__      :1045-1073, 1086-1118 + _transpose :760-791
//                                              crop, channel selection and the (y,x,s,c) -> (s,c,y,x) transpose of a patch
// Raw channel map: datasets.py:223-267.  Both are streaming, HBM-bound kernels: nothing is read twice.
#include "data_step.h"

namespace wcmc {

constexpr int SB_S = 27;                    // total(3) log total(3) log specular(3) subpixel(2) g-buffer(16)
constexpr int SB_TILE = 128;                // records staged per block iteration of the tiled form

// raw channels of _preprocess_sbmc (datasets.py:229-255): subpixel 0:2, radiance 2:5, diffuse 5:8, g-buffer 8:24,
// probabilities 24:24+4d, light directions 24+4d:24+6d, bounce types 24+6d:24+7d  (d = MAX_DEPTH + 1)
__device__ __forceinline__ float sb_s_value(const float* r, int c) {
  if (c < 3) return fmaxf(r[2 + c], 0.f);                                            // :394-397
  if (c < 6) return logf(1.f + fmaxf(r[2 + c - 3], 0.f)) / 10.0f;                    // :442
  if (c < 9) {                                                                       // :399-406
    const float t = fmaxf(r[2 + c - 6], 0.f), df = fmaxf(r[5 + c - 6], 0.f);
    return logf(1.f + fmaxf(t - df, 0.f)) / 10.0f;
  }
  if (c < 11) return r[c - 9];                                                       // :408-410
  return r[8 + c - 11];                                                              // :412-415
}

__device__ __forceinline__ float sb_p_value(const float* r, int c, int d) {
  if (c < 4 * d) return logf(fmaxf(r[24 + c], 0.f) + 1e-5f) / 30.0f;                 // :417-420
  if (c < 6 * d) return fminf(fmaxf(r[24 + c], -1.0f), 1.0f);                        // :422-425
  const int k = (c - 6 * d) / d, b = (c - 6 * d) - k * d;                            // plane k (bit k), bounce b  :427-438
  const float v = r[24 + 6 * d + b];
  // astype(np.int16): truncation toward zero; a value with no int16 counterpart has no tags (wcmc_hip.h)
  const int code = (v > -32769.0f && v < 32768.0f) ? (int)v : 0;
  return (code >> k) & 1 ? 1.0f : 0.0f;
}

// generic form: one thread per output element of either buffer
__global__ __launch_bounds__(256) void sb_preprocess_kernel(const float* __restrict__ raw, float* __restrict__ out_s,
                                                            float* __restrict__ out_p, int64_t n, int C, int d) {
  const int PC = 11 * d, OC = SB_S + PC;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n * OC;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / OC;
    const int c = (int)(idx - i * OC);
    if (c < SB_S) out_s[i * SB_S + c] = sb_s_value(raw + i * C, c);
    else out_p[i * PC + c - SB_S] = sb_p_value(raw + i * C, c - SB_S, d);
  }
}

// Tiled form (16-byte aligned records), after pp_llpm_tiled_kernel: the function reads channels [0, 24 + 7d) -- 66 of 104 at
// MAX_DEPTH 5.  A block stages that range (rounded up to whole float4: 272-byte runs) of 128 consecutive records in LDS with 16-byte
// loads, then writes the 128 x 27 and the 128 x 66 outputs as one contiguous run each.
__global__ __launch_bounds__(256) void sb_preprocess_tiled_kernel(const float* __restrict__ raw, float* __restrict__ out_s,
                                                                  float* __restrict__ out_p, int64_t n, int C, int d) {
  extern __shared__ __attribute__((aligned(16))) float sb_tile[];
  const int W4 = (24 + 7 * d + 3) / 4;              // float4 per record (17); the host checks 4 * W4 <= C
  const int LD = W4 * 4 + 1;                        // odd row pitch: conflict-free column reads
  const int PC = 11 * d;
  for (int64_t s0 = (int64_t)blockIdx.x * SB_TILE; s0 < n; s0 += (int64_t)gridDim.x * SB_TILE) {
    const int cnt = (int)min((int64_t)SB_TILE, n - s0);
    for (int t = threadIdx.x; t < cnt * W4; t += 256) {
      const int j = t / W4, q = t - j * W4;
      const float4 v = *reinterpret_cast<const float4*>(raw + (s0 + j) * C + q * 4);
      float* dst = sb_tile + j * LD + q * 4;
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < cnt * SB_S; t += 256) {
      const int j = t / SB_S;
      out_s[s0 * SB_S + t] = sb_s_value(sb_tile + j * LD, t - j * SB_S);
    }
    for (int t = threadIdx.x; t < cnt * PC; t += 256) {
      const int j = t / PC;
      out_p[s0 * PC + t] = sb_p_value(sb_tile + j * LD, t - j * PC, d);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ sample-based patch batches (datasets.py:1045-1118)
// Work unit: (source buffer, patch b, patch row y, chunk of 32 pixels along x, chunk of up to 4 samples).  The unit's source is
// 32 runs of (samples x channels) consecutive floats, one per pixel (one single run when the chunk holds every sample): global
// reads run along c into an LDS tile with an odd pixel pitch; the tile is then read along x, so every (sample, channel) row of the
// outputs is written as one 128-byte segment.
constexpr int SA_XT = 32, SA_SC = 4;
constexpr int SA_CP = 66, SA_CL = 37, SA_CG = 9;

struct SampleSrc { const float* p; int C, S, Sp, nout; int64_t first; };  // S: samples taken, of the Sp each pixel holds; first: index of the source's first work unit
struct SampleBatch {
  SampleSrc src[4];                                                      // sbmc_s, sbmc_p, llpm, gt (nout = 0: not read)
  float *rad, *feat, *paths, *tgt;
  int F, ng;                                                             // feature channels; those taken from sbmc_s (24 or 3)
};

__device__ __forceinline__ float* sa_dst(const SampleBatch& a, int k, int b, int s, int S, int ch, int64_t plane) {
  const int64_t bs = (int64_t)b * S + s;
  if (k == 0) return ch < 3 ? a.rad + (bs * 3 + ch) * plane : a.feat + (bs * a.F + ch - 3) * plane;
  if (k == 1) return a.feat + (bs * a.F + a.ng + ch) * plane;
  if (k == 2) return ch == 0 ? a.feat + (bs * a.F + a.F - 1) * plane : a.paths + (bs * 36 + ch - 1) * plane;
  return a.tgt + ((int64_t)b * 3 + ch) * plane;
}

// AUG (a transforms table is given): the unit's 32 output pixels (y, x0 + px) take the window positions patch_map
// gives for the code transforms[b].  The map is affine, so the 32 source runs are `step` floats apart -- one pixel pitch forwards
// or backwards along a source row, or a whole source row up or down for the transposing codes -- instead of one pitch; every
// channel is a copy, and the LDS tile and the writes are the plain form's.
template <bool AUG>
__global__ __launch_bounds__(256) void sa_assemble_kernel(SampleBatch a, const int* __restrict__ origins,
                                                          const int* __restrict__ transforms, int64_t units, int B, int H, int W,
                                                          int S, int P) {
  extern __shared__ __attribute__((aligned(16))) float sa_tile[];
  const int nxc = (P + SA_XT - 1) / SA_XT;
  const int64_t plane = (int64_t)P * P;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    int k = 3;
    while (k > 0 && (a.src[k].nout == 0 || u < a.src[k].first)) --k;
    const SampleSrc sr = a.src[k];
    int64_t t = u - sr.first;
    const int nsc = (sr.S + SA_SC - 1) / SA_SC;
    const int sc = (int)(t % nsc); t /= nsc;
    const int xc = (int)(t % nxc); t /= nxc;
    const int y = (int)(t % P), b = (int)(t / P);
    const int x0 = xc * SA_XT, xcnt = min(SA_XT, P - x0);
    const int s0 = sc * SA_SC, scnt = min(SA_SC, sr.S - s0);
    // (the host checks the origins; the clamp keeps a bad one from reading outside the image)
    PatchMap pm{y, x0, 0, 1, 1, 0};
    if (AUG) pm = patch_map(transforms[b], y, x0, P);
    const int r = min(max(origins[2 * b], 0), H - P) + pm.sy, c = min(max(origins[2 * b + 1], 0), W - P) + pm.sx;
    const int run = scnt * sr.C, LD = (SA_SC * sr.C) | 1;
    const int64_t pitch = (int64_t)sr.Sp * sr.C;
    const float* base = sr.p + ((int64_t)r * W + c) * pitch + (int64_t)s0 * sr.C;
    if (AUG) {
      const int64_t step = ((int64_t)pm.xr * W + pm.xc) * pitch;             // from the source of (y, x) to that of (y, x + 1)
      for (int f = threadIdx.x; f < xcnt * run; f += 256) {
        const int px = f / run, e = f - px * run;
        sa_tile[px * LD + e] = base[px * step + e];
      }
    } else {
      for (int f = threadIdx.x; f < xcnt * run; f += 256) {
        const int px = f / run, e = f - px * run;
        sa_tile[px * LD + e] = base[px * pitch + e];
      }
    }
    __syncthreads();
    const int rows = scnt * sr.nout;
    for (int o = threadIdx.x; o < rows * SA_XT; o += 256) {
      const int x = o & (SA_XT - 1), row = o / SA_XT;
      if (x < xcnt) {
        const int sl = row / sr.nout, ch = row - sl * sr.nout;
        sa_dst(a, k, b, s0 + sl, sr.S, ch, plane)[(int64_t)y * P + x0 + x] = sa_tile[x * LD + sl * sr.C + ch];
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ sample-based tiles of the mirror-extended frame (wcmc_amd.denoise)
// sa_assemble_kernel with other addressing: the tile's origin is in frame coordinates and may lie up to `pad` pixels outside, the
// source row is m(r) and each of the chunk's 32 pixels has its own source column m(c + px) (ft_mirror: a chunk that straddles a
// frame edge runs backwards on the far side of it).  All three buffers are per sample, so a mirrored position is a copy of its
// image's record -- nothing is recomputed -- and there is no gt source.  LDS tile and write pattern as above; the reads run along c
// too, a pixel per half-wave.
// AUG (a code t in 1..7): the whole launch reads the frame through one dihedral transform `code`.
// Origins and mirror are those of the TRANSFORMED frame (Ht x Wt: W x H for odd codes) and frame_map gives each of the chunk's 32
// pixels its source record: along a source row for even codes, down a source column for odd ones.  Every channel is a copy; the
// LDS tile and the writes are unchanged.
template <bool AUG>
__global__ __launch_bounds__(256) void sa_assemble_tiles_kernel(SampleBatch a, const int* __restrict__ origins, int64_t units, int H,
                                                                int W, int P, int code) {
  extern __shared__ __attribute__((aligned(16))) float sa_tile[];
  const int nxc = (P + SA_XT - 1) / SA_XT;
  const int64_t plane = (int64_t)P * P;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    int k = 2;
    while (k > 0 && (a.src[k].nout == 0 || u < a.src[k].first)) --k;
    const SampleSrc sr = a.src[k];
    int64_t t = u - sr.first;
    const int nsc = (sr.S + SA_SC - 1) / SA_SC;
    const int sc = (int)(t % nsc); t /= nsc;
    const int xc = (int)(t % nxc); t /= nxc;
    const int y = (int)(t % P), b = (int)(t / P);
    const int x0 = xc * SA_XT, xcnt = min(SA_XT, P - x0);
    const int s0 = sc * SA_SC, scnt = min(SA_SC, sr.S - s0);
    // (the host checks the origins; ft_mirror's clamp keeps a bad one from reading outside the buffers)
    const int Ht = AUG && (code & 1) ? W : H, Wt = AUG && (code & 1) ? H : W; // the transformed frame's sizes
    const int r = ft_mirror(origins[2 * b] + y, Ht), c = origins[2 * b + 1] + x0;
    const int run = scnt * sr.C, LD = (SA_SC * sr.C) | 1;
    const int64_t pitch = (int64_t)sr.Sp * sr.C;
    const float* base = sr.p + (AUG ? 0 : (int64_t)r * W * pitch) + (int64_t)s0 * sr.C;
    // eight pixels at a time, 32 lanes along each pixel's run (128-byte segments): the source column is mirrored once per pixel,
    // not once per float, and no index is divided
    for (int px = threadIdx.x >> 5; px < xcnt; px += 8) {
      const float* src;
      if (AUG) {
        const FramePos sp = frame_map(code, r, ft_mirror(c + px, Wt), H, W);
        src = base + ((int64_t)sp.sy * W + sp.sx) * pitch;
      } else {
        src = base + ft_mirror(c + px, W) * pitch;
      }
      float* dst = sa_tile + px * LD;
#pragma unroll 4
      for (int e = threadIdx.x & 31; e < run; e += 32) dst[e] = src[e];
    }
    __syncthreads();
    const int rows = scnt * sr.nout;
    for (int o = threadIdx.x; o < rows * SA_XT; o += 256) {
      const int x = o & (SA_XT - 1), row = o / SA_XT;
      if (x < xcnt) {
        const int sl = row / sr.nout, ch = row - sl * sr.nout;
        sa_dst(a, k, b, s0 + sl, sr.S, ch, plane)[(int64_t)y * P + x0 + x] = sa_tile[x * LD + sl * sr.C + ch];
      }
    }
    __syncthreads();
  }
}

}  // namespace wcmc

using namespace wcmc;

// The sources and the work units of a launch of either assembly kernel.  The per-sample buffers hold S_total samples per pixel, the
// outputs the first s of them; gt (patches only) is the fourth source, and without it neither its slot nor target_image is read.
static SampleBatch sa_batch(const float* sbmc_s, const float* sbmc_p, const float* llpm, const float* gt, int B, int S_total, int s,
                            int P, int use_g_buf, int use_sbmc_buf, float* radiance, float* features, float* paths,
                            float* target_image, int64_t* units_out) {
  SampleBatch a;
  a.rad = radiance; a.feat = features; a.paths = paths; a.tgt = target_image;
  a.ng = use_g_buf ? 24 : 3;
  a.F = a.ng + (use_sbmc_buf ? SA_CP : 0) + (llpm ? 1 : 0);
  a.src[0] = SampleSrc{sbmc_s, SB_S, s, S_total, 3 + a.ng, 0};
  a.src[1] = SampleSrc{sbmc_p, SA_CP, s, S_total, use_sbmc_buf ? SA_CP : 0, 0};
  a.src[2] = SampleSrc{llpm, SA_CL, s, S_total, llpm ? SA_CL : 0, 0};
  a.src[3] = SampleSrc{gt, SA_CG, 1, 1, gt ? 3 : 0, 0};
  const int64_t rows = (int64_t)B * P * ((P + SA_XT - 1) / SA_XT);
  int64_t units = 0;
  for (int k = 0; k < (gt ? 4 : 3); ++k) {
    a.src[k].first = units;
    if (a.src[k].nout > 0) units += rows * ((a.src[k].S + SA_SC - 1) / SA_SC);
  }
  *units_out = units;
  return a;
}

constexpr size_t SA_LDS = (size_t)SA_XT * ((SA_SC * SA_CP) | 1) * sizeof(float);   // the widest source's tile

extern "C" int wcmc_assemble_sample_tiles(const float* sbmc_s, const float* sbmc_p, const float* llpm, const int* origins, int B,
                                          int H, int W, int S, int P, int pad, int t, int use_g_buf, int use_sbmc_buf,
                                          float* radiance, float* features, float* paths, void* stream) {
  WCMC_REQUIRE(t >= 0 && t <= 7, WCMC_ERR_BAD_ARG, "assemble_sample_tiles: the transform code must lie in 0..7 (got %d)", t);
  WCMC_REQUIRE(sbmc_s && origins && radiance && features, WCMC_ERR_BAD_ARG, "assemble_sample_tiles: null pointer");
  WCMC_REQUIRE(!use_sbmc_buf || sbmc_p, WCMC_ERR_BAD_ARG, "assemble_sample_tiles: use_sbmc_buf needs sbmc_p");
  WCMC_REQUIRE(!llpm || paths, WCMC_ERR_BAD_ARG, "assemble_sample_tiles: llpm needs a paths output");
  WCMC_REQUIRE(B > 0 && H > 0 && W > 0 && P > 0 && pad >= 0, WCMC_ERR_BAD_ARG,
               "assemble_sample_tiles: B, H, W, P must be positive and pad non-negative");
  WCMC_REQUIRE(S > 0, WCMC_ERR_BAD_ARG, "assemble_sample_tiles: S must be positive (got %d)", S);
  const int Ht = t & 1 ? W : H, Wt = t & 1 ? H : W;
  WCMC_REQUIRE(pad < Ht && pad < Wt, WCMC_ERR_BAD_ARG,
               "assemble_sample_tiles: pad = %d must be smaller than the transformed %d x %d frame (one reflection)", pad, Ht, Wt);
  WCMC_REQUIRE(P > 2 * pad, WCMC_ERR_BAD_ARG, "assemble_sample_tiles: a %d-pixel tile has no interior inside a pad of %d", P, pad);
  WCMC_REQUIRE(P <= Ht + 2 * pad && P <= Wt + 2 * pad, WCMC_ERR_BAD_ARG,
               "assemble_sample_tiles: a %d-pixel tile does not fit the transformed %d x %d frame extended by %d", P, Ht, Wt, pad);
  int64_t units;
  const SampleBatch a = sa_batch(sbmc_s, sbmc_p, llpm, nullptr, B, S, S, P, use_g_buf, use_sbmc_buf, radiance, features, paths, nullptr,
                                 &units);
  const dim3 grid((unsigned)(units > 65535 ? 65535 : units));
  if (t)
    hipLaunchKernelGGL(sa_assemble_tiles_kernel<true>, grid, dim3(256), SA_LDS, (hipStream_t)stream, a, origins, units, H, W, P, t);
  else
    hipLaunchKernelGGL(sa_assemble_tiles_kernel<false>, grid, dim3(256), SA_LDS, (hipStream_t)stream, a, origins, units, H, W, P, 0);
  return check_launch("assemble_sample_tiles");
}

extern "C" int wcmc_preprocess_sbmc(const float* raw, int64_t nsamples, int C, int max_depth, float* out_s, float* out_p,
                                    int tiled, void* stream) {
  WCMC_REQUIRE(raw && out_s && out_p && nsamples > 0 && max_depth >= 0 && C >= 38 + 11 * (max_depth + 1), WCMC_ERR_BAD_ARG,
               "preprocess_sbmc: bad argument (raw needs >= 38 + 11*(max_depth+1) channels)");
  const int d = max_depth + 1;
  const int W4 = (24 + 7 * d + 3) / 4;
  const size_t lds = (size_t)SB_TILE * (W4 * 4 + 1) * sizeof(float);
  const bool can_tile = C % 4 == 0 && 4 * W4 <= C && aligned16(raw) && lds <= 64 * 1024;
  WCMC_REQUIRE(tiled <= 0 || can_tile, WCMC_ERR_BAD_ARG,
               "preprocess_sbmc: the tiled form needs 16-byte aligned records (C a multiple of 4, aligned base) and max_depth <= 16");
  if (tiled != 0 && can_tile) {
    const int64_t blocks = ceil_div64(nsamples, SB_TILE);
    hipLaunchKernelGGL(sb_preprocess_tiled_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), lds,
                       (hipStream_t)stream, raw, out_s, out_p, nsamples, C, d);
  } else {
    hipLaunchKernelGGL(sb_preprocess_kernel, dim3(pp_grid(nsamples * (SB_S + 11 * d))), dim3(256), 0, (hipStream_t)stream, raw,
                       out_s, out_p, nsamples, C, d);
  }
  return check_launch("preprocess_sbmc");
}

extern "C" int wcmc_assemble_sample_patches(const float* sbmc_s, const float* sbmc_p, const float* llpm, const float* gt,
                                            const int* origins, const int* transforms, int B, int H, int W, int S_total, int s,
                                            int P, int use_g_buf, int use_sbmc_buf, float* radiance, float* features, float* paths,
                                            float* target_image, void* stream) {
  WCMC_REQUIRE(sbmc_s && gt && origins && radiance && features && target_image, WCMC_ERR_BAD_ARG,
               "assemble_sample_patches: null pointer");
  WCMC_REQUIRE(!use_sbmc_buf || sbmc_p, WCMC_ERR_BAD_ARG, "assemble_sample_patches: use_sbmc_buf needs sbmc_p");
  WCMC_REQUIRE(B > 0 && H > 0 && W > 0 && P > 0, WCMC_ERR_BAD_ARG, "assemble_sample_patches: B, H, W, P must be positive");
  WCMC_REQUIRE(P <= H && P <= W, WCMC_ERR_BAD_ARG, "assemble_sample_patches: a %d-pixel patch does not fit the %d x %d frame", P, H,
               W);
  WCMC_REQUIRE(1 <= s && s <= S_total, WCMC_ERR_BAD_ARG,
               "assemble_sample_patches: the prefix must satisfy 1 <= s <= S_total (got %d of %d)", s, S_total);
  WCMC_REQUIRE(!llpm || paths, WCMC_ERR_BAD_ARG, "assemble_sample_patches: llpm given without a paths output");
  int64_t units;
  const SampleBatch a = sa_batch(sbmc_s, sbmc_p, llpm, gt, B, S_total, s, P, use_g_buf, use_sbmc_buf, radiance, features, paths,
                                 target_image, &units);
  const dim3 grid((unsigned)(units > 65535 ? 65535 : units));
  if (transforms)
    hipLaunchKernelGGL(sa_assemble_kernel<true>, grid, dim3(256), SA_LDS, (hipStream_t)stream, a, origins, transforms, units, B, H, W, s,
                       P);
  else
    hipLaunchKernelGGL(sa_assemble_kernel<false>, grid, dim3(256), SA_LDS, (hipStream_t)stream, a, origins, transforms, units, B, H, W,
                       s, P);
  return check_launch("assemble_sample_patches");
}

