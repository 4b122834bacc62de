// Denoising a render of any size (wcmc_amd.denoise; DESIGN.md "Denoising a render"): the two kernels around the network.
//
//   wcmc_assemble_kpcn_tiles  the inference batch for tiles whose origins may lie up to `pad` pixels outside the frame.  The frame is
//                             taken as extended by `pad` pixels on every side by mirror reflection with the edge repeated (numpy
//                             'symmetric', scipy 'reflect': wcmc_reflect_index), but the extension is never stored: a position
//                             outside reads the record of its mirror image, and the backward differences of the 44-channel buffer
//                             (data_step.h: pp_kpcn_finish) are taken again from the stored values wherever a neighbour lies across
//                             the edge.  Bit for bit what preprocessing the padded raw frame and wcmc_assemble_kpcn_patches give.
//   wcmc_finish_frame         one pass over the stitched frame: the noisy input, the has-hit mask, the composite and 8-bit previews.
// The dihedral self-ensemble adds the way through a whole-frame transform and back:
//   wcmc_assemble_kpcn_tiles, t > 0   the same batch of the frame as if the RAW frame had been flipped / turned before preprocessing.
//   wcmc_stitch_tiles_aug             pastes or adds the owned windows of the transformed frame's tiles into the frame in source orientation.
// Feathered seams:
//   wcmc_stitch_tiles_blend       adds w * v and w of one batch of tiles, each on its owned window widened by F pixels, under a code t.
//   wcmc_blend_finish             out = acc / wsum, or out += acc / wsum: a pass normalised by its own weight sum.
#include "data_step.h"

namespace wcmc {

struct TileOut {
  float *din, *sin, *dbuf, *sbuf, *alb, *paths;
};

// (ft_grad_src / ft_grad_dst, the channels of the backward differences, are in data_step.h: the augmented patch assembler uses them too)
// One thread per (tile, y, x), as pp_assemble_kpcn_kernel: every output plane is written as coalesced rows, each record is read once
// (a second record's thirteen values only where a difference crosses the frame's edge: the outer `pad` ring of border tiles).
// AUG (a code t in 1..7): the whole launch reads the frame through one dihedral transform t.  The origins
// and the mirror are those of the TRANSFORMED frame (Ht x Wt: W x H for odd t), frame_map then gives the source record, and each of the
// 26 differences is value[src(p)] - value[src(p - e)] with e one step along the transformed frame's x / y.  Where that neighbour's
// source is the stored one (one column / row before the source) the stored difference is that very subtraction and is kept; elsewhere
// thirteen floats of the neighbour's record are read.  AUG = false is the plain kernel: its body is the one it had.
template <bool VEC, bool AUG>
__global__ __launch_bounds__(256) void ft_assemble_tiles_kernel(const float* __restrict__ kpcn, const float* __restrict__ llpm,
                                                                const int* __restrict__ origins, TileOut o, int B, int H, int W,
                                                                int S, int P, int pad, int t) {
  const int64_t total = (int64_t)B * P * P;
  const int cin = llpm ? 35 : 34;
  const int64_t plane = (int64_t)P * P;
  const int Ht = AUG && (t & 1) ? W : H, Wt = AUG && (t & 1) ? H : W;         // the transformed frame's sizes
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % P), y = (int)((i / P) % P), b = (int)(i / plane);
    const int r = origins[2 * b] + y, c = origins[2 * b + 1] + x;             // (row, column) of the frame; may lie outside
    const int mr = ft_mirror(r, Ht), mc = ft_mirror(c, Wt);
    FramePos sp{mr, mc};
    if (AUG) sp = frame_map(t, mr, mc, H, W);
    const int64_t pix = (int64_t)sp.sy * W + sp.sx;
    const float* k = kpcn + pix * KP_C;
    float v[KP_C];
    if (VEC) {
#pragma unroll
      for (int q = 0; q < KP_C / 4; ++q) {
        const float4 f = *reinterpret_cast<const float4*>(k + 4 * q);
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < KP_C; ++ch) v[ch] = k[ch];
    }
    if (AUG) {
      {
        const bool first = c + pad <= 0;
        const FramePos n = frame_map(t, mr, ft_mirror(c - 1, Wt), H, W);      // source of the left neighbour in the transformed frame
        if (first || n.sy != sp.sy || n.sx != sp.sx - 1) {
          const float* kl = kpcn + ((int64_t)n.sy * W + n.sx) * KP_C;
#pragma unroll
          for (int g = 0; g < KP_NV; ++g) v[ft_grad_dst(g, false)] = first ? 0.f : v[ft_grad_src(g)] - kl[ft_grad_src(g)];
        }
      }
      {
        const bool first = r + pad <= 0;
        const FramePos n = frame_map(t, ft_mirror(r - 1, Ht), mc, H, W);      // ... of the upper neighbour
        if (first || n.sx != sp.sx || n.sy != sp.sy - 1) {
          const float* ku = kpcn + ((int64_t)n.sy * W + n.sx) * KP_C;
#pragma unroll
          for (int g = 0; g < KP_NV; ++g) v[ft_grad_dst(g, true)] = first ? 0.f : v[ft_grad_src(g)] - ku[ft_grad_src(g)];
        }
      }
    } else {
      // The stored difference is that of the extended frame only where both operands are in-frame neighbours (1 <= c < W); elsewhere
      // it is value[m(r), m(c)] - value[m(r), m(c - 1)], and 0 in the extended frame's first column / row (frame position -pad).
      if (c < 1 || c >= W) {
        const bool first = c + pad <= 0;
        const float* kl = kpcn + ((int64_t)mr * W + ft_mirror(c - 1, W)) * KP_C;
#pragma unroll
        for (int g = 0; g < KP_NV; ++g) v[ft_grad_dst(g, false)] = first ? 0.f : v[ft_grad_src(g)] - kl[ft_grad_src(g)];
      }
      if (r < 1 || r >= H) {
        const bool first = r + pad <= 0;
        const float* ku = kpcn + ((int64_t)ft_mirror(r - 1, H) * W + mc) * KP_C;
#pragma unroll
        for (int g = 0; g < KP_NV; ++g) v[ft_grad_dst(g, true)] = first ? 0.f : v[ft_grad_src(g)] - ku[ft_grad_src(g)];
      }
    }
    const int64_t po = (int64_t)y * P + x;
    float* din = o.din + (int64_t)b * cin * plane + po;
    float* sin = o.sin + (int64_t)b * cin * plane + po;
#pragma unroll
    for (int ch = 0; ch < 10; ++ch) din[ch * plane] = v[ch];
#pragma unroll
    for (int ch = 20; ch < 44; ++ch) din[(ch - 10) * plane] = v[ch];
#pragma unroll
    for (int ch = 10; ch < 44; ++ch) sin[(ch - 10) * plane] = v[ch];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      o.dbuf[((int64_t)b * 3 + ch) * plane + po] = v[ch];
      o.sbuf[((int64_t)b * 3 + ch) * plane + po] = v[10 + ch];
      o.alb[((int64_t)b * 3 + ch) * plane + po] = v[34 + ch] + 0.00316f;
    }
    if (llpm) {
      const float* l = llpm + pix * S * 37;
      float pw = 0.f;
      for (int s = 0; s < S; ++s) {
        pw += l[s * 37];
        float* pp = o.paths + (((int64_t)b * S + s) * 36) * plane + po;
        for (int ch = 0; ch < 36; ++ch) pp[ch * plane] = l[s * 37 + 1 + ch];
      }
      pw /= (float)S;
      din[34 * plane] = pw;
      sin[34 * plane] = pw;
    }
  }
}

// tonemap of test_models.py:24-34 at its default gamma on the image's own luminance, then round(255 * .) (half to even, as np.round)
__device__ __forceinline__ void ft_preview(const float* rgb, uint8_t* dst) {
  const float lum = 0.2126f * rgb[0] + 0.7152f * rgb[1] + 0.0722f * rgb[2];
  const float den = 1.f + lum / 1.5f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float t = fmaxf(rgb[ch] / den, 0.f);                  // (fmaxf / fminf: a NaN becomes 0, a defined 8-bit value)
    t = fminf(fmaxf(powf(t, 1.0f / 2.2f), 0.f), 1.f);
    dst[ch] = (uint8_t)rintf(255.f * t);
  }
}

// One thread per pixel.  llpm: one float per sample (descriptor 24 of `paths`: the bounce type of the first bounce).
__global__ __launch_bounds__(256) void ft_finish_frame_kernel(const float* __restrict__ out_rad, const float* __restrict__ kpcn,
                                                              const float* __restrict__ llpm, int64_t npix, int S,
                                                              float* __restrict__ out, float* __restrict__ ipt,
                                                              float* __restrict__ has_hit, uint8_t* __restrict__ prev_out,
                                                              uint8_t* __restrict__ prev_ipt) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const float* k = kpcn + p * KP_C;
    const float* l = llpm + p * S * 37 + 25;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += l[s * 37];
    const bool hit = sum / (float)S != 0.f;
    float in[3], res[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      in[ch] = k[KP_DIFF + ch] * (k[KP_ALB + ch] + 0.00316f) + expf(k[KP_SPEC + ch]) - 1.f;
      res[ch] = hit ? out_rad[ch * npix + p] : in[ch];
      ipt[p * 3 + ch] = in[ch];
      out[p * 3 + ch] = res[ch];
    }
    has_hit[p] = hit ? 1.f : 0.f;
    if (prev_out) ft_preview(res, prev_out + p * 3);
    if (prev_ipt) ft_preview(in, prev_ipt + p * 3);
  }
}

// The closing pass of the sample-based models.  One thread per pixel: the noisy input is the mean over the samples of the first
// three channels of sbmc_s (max(total, 0); datasets.py:1248), summed in sample order; has_hit as above.
__global__ __launch_bounds__(256) void ft_finish_sample_frame_kernel(const float* __restrict__ out_rad, const float* __restrict__ sbmc_s,
                                                                     const float* __restrict__ llpm, int64_t npix, int S,
                                                                     float* __restrict__ out, float* __restrict__ ipt,
                                                                     float* __restrict__ has_hit, uint8_t* __restrict__ prev_out,
                                                                     uint8_t* __restrict__ prev_ipt) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const float* r = sbmc_s + p * S * 27;
    const float* l = llpm + p * S * 37 + 25;
    float sum = 0.f, acc[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      sum += l[s * 37];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] += r[s * 27 + ch];
    }
    const bool hit = sum / (float)S != 0.f;
    float in[3], res[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      in[ch] = acc[ch] / (float)S;
      res[ch] = hit ? out_rad[ch * npix + p] : in[ch];
      ipt[p * 3 + ch] = in[ch];
      out[p * 3 + ch] = res[ch];
    }
    has_hit[p] = hit ? 1.f : 0.f;
    if (prev_out) ft_preview(res, prev_out + p * 3);
    if (prev_ipt) ft_preview(in, prev_ipt + p * 3);
  }
}

// The way back of the self-ensemble: ie_stitch_kernel's radiance half for tiles of the frame TRANSFORMED by
// code t, written to (or added to) the frame in SOURCE orientation.  coords: the (B, 6) table of the transformed Ht x Wt frame.  One
// thread per (channel, owned pixel): the reads run along the network output's rows; the writes run along source rows for even t
// and down source columns for odd t.  The owned windows partition the frame and frame_map is a bijection, so every element of
// out_rad is touched by one thread of one launch of a pass: `out + v` needs no atomic and is the same bits on every run.
struct StitchAugArgs {
  const float* rad; int64_t rsb, rsc, rsh, rsw;     // (B, 3, ho, wo) network output
  const int* coords;                                // (B, 6): i_start, j_start, i_end, j_end, i, j of the transformed frame
  float* orad;                                      // (3, H, W), source orientation
  int ho, wo, P, H, W, t;
};

template <bool ACC>
__global__ __launch_bounds__(256) void ft_stitch_aug_kernel(StitchAugArgs a) {
  const int b = blockIdx.y;
  const int* cd = a.coords + 6 * b;
  const int i0 = cd[0], j0 = cd[1], i1 = cd[2], j1 = cd[3], ib = cd[4], jb = cd[5];
  const int Ht = a.t & 1 ? a.W : a.H, Wt = a.t & 1 ? a.H : a.W;
  // a window outside the transformed frame or the tile is skipped (the wrapper validates the table on the host before upload)
  if (i0 < 0 || j0 < 0 || i1 > Ht || j1 > Wt || i0 >= i1 || j0 >= j1 || i0 < ib || j0 < jb || i1 > ib + a.P || j1 > jb + a.P)
    return;
  const int wh = i1 - i0, ww = j1 - j0;
  const int64_t win = (int64_t)wh * ww;
  const int top = (a.P - a.ho) / 2, left = (a.P - a.wo) / 2;      // the 'replicate' padding of ie_stitch_kernel
  const int64_t hw = (int64_t)a.H * a.W;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 3 * win; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t plane = e / win, q = e - plane * win;
    const int dy = (int)(q / ww), dx = (int)(q - (int64_t)dy * ww);
    const int y = i0 + dy, x = j0 + dx;                           // pixel of the transformed frame
    const int sy = min(max(y - ib - top, 0), a.ho - 1), sx = min(max(x - jb - left, 0), a.wo - 1);
    const float v = a.rad[b * a.rsb + plane * a.rsc + sy * a.rsh + sx * a.rsw];
    const FramePos p = frame_map(a.t, y, x, a.H, a.W);
    float* dst = a.orad + plane * hw + (int64_t)p.sy * a.W + p.sx;
    *dst = ACC ? *dst + v : v;
  }
}

// The feathered stitch: every tile of the batch adds w * v and w on [i_start - F, i_end + F) x [j_start - F,
// j_end + F) of the (transformed) frame, clipped to it.  One thread owns a destination pixel for the whole launch and walks the
// batch's tiles in table order, so the fp32 sums are those of the table order whatever the batches are, with no atomic; launches
// follow one another on one stream.  Every thread first takes the bounding box of the batch's ranges (B uniform reads of the table)
// and the grid strides over that box alone: a batch is a few tiles of a frame of many.
struct StitchBlendArgs {
  const float* rad; int64_t rsb, rsc, rsh, rsw;     // (B, 3, ho, wo) network output
  const int* coords;                                // (B, 6) rows of the transformed frame's table
  float *acc, *wsum;                                // (3, H, W), (H, W): source orientation
  int ho, wo, P, B, H, W, t, F;
};

// a table row that ie_stitch_kernel would skip is skipped here too
__device__ __forceinline__ bool ft_row_ok(const int* cd, int Ht, int Wt, int P) {
  const int i0 = cd[0], j0 = cd[1], i1 = cd[2], j1 = cd[3], ib = cd[4], jb = cd[5];
  return !(i0 < 0 || j0 < 0 || i1 > Ht || j1 > Wt || i0 >= i1 || j0 >= j1 || i0 < ib || j0 < jb || i1 > ib + P || j1 > jb + P);
}

// u(x) = L(x) * R(x) of section 22 along an axis of length n for the owned interval [a, b), inside [a - F, b + F) and F > 0.  The
// numerators are odd integers over 4F: exact in fp64, so the 2-D weight is rounded once, on its way to fp32.
__device__ __forceinline__ double ft_feather(int x, int a, int b, int n, int F) {
  const double den = 4.0 * F;
  const double l = a == 0 ? 1.0 : fmin(fmax((double)(2 * (x - a + F) + 1) / den, 0.0), 1.0);
  const double r = b == n ? 1.0 : fmin(fmax((double)(2 * (b + F - x) - 1) / den, 0.0), 1.0);
  return l * r;
}

__global__ __launch_bounds__(256) void ft_stitch_blend_kernel(StitchBlendArgs a) {
  const int Ht = a.t & 1 ? a.W : a.H, Wt = a.t & 1 ? a.H : a.W;
  int y0 = Ht, y1 = 0, x0 = Wt, x1 = 0;
  for (int b = 0; b < a.B; ++b) {
    const int* cd = a.coords + 6 * b;
    if (!ft_row_ok(cd, Ht, Wt, a.P)) continue;
    y0 = min(y0, max(cd[0] - a.F, 0)); y1 = max(y1, min(cd[2] + a.F, Ht));
    x0 = min(x0, max(cd[1] - a.F, 0)); x1 = max(x1, min(cd[3] + a.F, Wt));
  }
  if (y0 >= y1 || x0 >= x1) return;
  const int bw = x1 - x0;
  const int64_t box = (int64_t)(y1 - y0) * bw, hw = (int64_t)a.H * a.W;
  const int top = (a.P - a.ho) / 2, left = (a.P - a.wo) / 2;      // the 'replicate' padding of ie_stitch_kernel
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < box; e += (int64_t)gridDim.x * blockDim.x) {
    const int y = y0 + (int)(e / bw), x = x0 + (int)(e % bw);     // pixel of the transformed frame
    float s[3] = {0.f, 0.f, 0.f}, sw = 0.f;
    bool any = false;
    const FramePos p = frame_map(a.t, y, x, a.H, a.W);
    const int64_t dst = (int64_t)p.sy * a.W + p.sx;
    for (int b = 0; b < a.B; ++b) {
      const int* cd = a.coords + 6 * b;
      if (!ft_row_ok(cd, Ht, Wt, a.P)) continue;
      const int i0 = cd[0], j0 = cd[1], i1 = cd[2], j1 = cd[3], ib = cd[4], jb = cd[5];
      if (y < i0 - a.F || y >= i1 + a.F || x < j0 - a.F || x >= j1 + a.F) continue;
      const float w = a.F == 0 ? 1.f : (float)(ft_feather(y, i0, i1, Ht, a.F) * ft_feather(x, j0, j1, Wt, a.F));
      const int sy = min(max(y - ib - top, 0), a.ho - 1), sx = min(max(x - jb - left, 0), a.wo - 1);
      const float* v = a.rad + b * a.rsb + sy * a.rsh + sx * a.rsw;
      if (!any) {                                                 // the sums of earlier launches: read once, where a tile contributes
        any = true;
        sw = a.wsum[dst];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) s[ch] = a.acc[ch * hw + dst];
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) s[ch] = s[ch] + w * v[ch * a.rsc];
      sw = sw + w;
    }
    if (any) {
      a.wsum[dst] = sw;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) a.acc[ch * hw + dst] = s[ch];
    }
  }
}

// out = acc / wsum, or out + acc / wsum: the pass of one transform code, normalised by its own weight sum
template <bool ACC>
__global__ __launch_bounds__(256) void ft_blend_finish_kernel(const float* __restrict__ acc, const float* __restrict__ wsum, int64_t npix,
                                                              float* __restrict__ out) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const float w = wsum[p];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float q = acc[ch * npix + p] / w;
      out[ch * npix + p] = ACC ? out[ch * npix + p] + q : q;
    }
  }
}

}  // namespace wcmc

using namespace wcmc;

extern "C" int wcmc_stitch_tiles_blend(const float* rad, int64_t rsb, int64_t rsc, int64_t rsh, int64_t rsw, int ho, int wo, int P,
                                       int pad, const int* coords, int B, int t, int H, int W, int F, float* acc, float* wsum,
                                       void* stream) {
  WCMC_REQUIRE(t >= 0 && t <= 7, WCMC_ERR_BAD_ARG, "stitch_tiles_blend: the transform code must lie in 0..7 (got %d)", t);
  WCMC_REQUIRE(rad && coords && acc && wsum, WCMC_ERR_BAD_ARG, "stitch_tiles_blend: null pointer");
  WCMC_REQUIRE(B > 0 && H > 0 && W > 0 && P > 0, WCMC_ERR_BAD_ARG, "stitch_tiles_blend: B, H, W, P must be positive");
  WCMC_REQUIRE((ho == P && wo == P) || (ho > 0 && wo > 0 && ho < P && wo < P), WCMC_ERR_BAD_ARG,
               "stitch_tiles_blend: the %d x %d network output must be P x P or smaller in both dimensions (P = %d)", ho, wo, P);
  WCMC_REQUIRE(F >= 0, WCMC_ERR_BAD_ARG, "stitch_tiles_blend: the feather half-width must not be negative (got %d)", F);
  WCMC_REQUIRE(F <= P, WCMC_ERR_BAD_ARG, "stitch_tiles_blend: a feather half-width of %d is wider than the %d-pixel tile", F, P);
  if (pad >= 0) {                                                 // (a negative pad: the caller vouches for the table)
    WCMC_REQUIRE(P > 2 * pad, WCMC_ERR_BAD_ARG, "stitch_tiles_blend: a %d-pixel tile has no interior inside a pad of %d", P, pad);
    WCMC_REQUIRE(2 * F <= P - 2 * pad, WCMC_ERR_BAD_ARG,
                 "stitch_tiles_blend: the two ramps of 2 * %d pixels are longer than the %d-pixel interior of a tile (P %d - 2 * pad %d)",
                 F, P - 2 * pad, P, pad);
    const int inset = (P - ho + 1) / 2 > (P - wo + 1) / 2 ? (P - ho + 1) / 2 : (P - wo + 1) / 2;
    WCMC_REQUIRE(F <= pad - inset, WCMC_ERR_BAD_ARG,
                 "stitch_tiles_blend: a feather of %d pixels beyond a pad of %d reaches the %d replicated pixels of the %d x %d output",
                 F, pad, inset, ho, wo);
  }
  WCMC_REQUIRE(B <= 65535, WCMC_ERR_BAD_ARG, "stitch_tiles_blend: at most 65535 tiles per launch");
  StitchBlendArgs a{rad, rsb, rsc, rsh, rsw, coords, acc, wsum, ho, wo, P, B, H, W, t, F};
  int64_t work = (int64_t)B * P * P;                              // every range lies inside its tile: the box is seldom larger
  if (work > (int64_t)H * W) work = (int64_t)H * W;
  hipLaunchKernelGGL(ft_stitch_blend_kernel, dim3(pp_grid(work)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("stitch_tiles_blend");
}

extern "C" int wcmc_blend_finish(const float* acc, const float* wsum, int H, int W, int accumulate, float* out_rad, void* stream) {
  WCMC_REQUIRE(acc && wsum && out_rad, WCMC_ERR_BAD_ARG, "blend_finish: null pointer");
  WCMC_REQUIRE(H > 0 && W > 0, WCMC_ERR_BAD_ARG, "blend_finish: H and W must be positive (got %d, %d)", H, W);
  WCMC_REQUIRE(accumulate == 0 || accumulate == 1, WCMC_ERR_BAD_ARG, "blend_finish: accumulate must be 0 or 1 (got %d)", accumulate);
  const int64_t npix = (int64_t)H * W;
  if (accumulate)
    hipLaunchKernelGGL(ft_blend_finish_kernel<true>, dim3(pp_grid(npix)), dim3(256), 0, (hipStream_t)stream, acc, wsum, npix, out_rad);
  else
    hipLaunchKernelGGL(ft_blend_finish_kernel<false>, dim3(pp_grid(npix)), dim3(256), 0, (hipStream_t)stream, acc, wsum, npix, out_rad);
  return check_launch("blend_finish");
}

extern "C" int wcmc_finish_sample_frame(const float* out_rad, const float* sbmc_s, const float* llpm, int H, int W, int S,
                                        float* out, float* ipt, float* has_hit, unsigned char* preview_out,
                                        unsigned char* preview_ipt, void* stream) {
  WCMC_REQUIRE(out_rad && sbmc_s && llpm && out && ipt && has_hit, WCMC_ERR_BAD_ARG, "finish_sample_frame: null pointer");
  WCMC_REQUIRE(H > 0 && W > 0 && S > 0, WCMC_ERR_BAD_ARG, "finish_sample_frame: H, W and S must be positive (got %d, %d, %d)", H, W,
               S);
  const int64_t npix = (int64_t)H * W;
  hipLaunchKernelGGL(ft_finish_sample_frame_kernel, dim3(pp_grid(npix)), dim3(256), 0, (hipStream_t)stream, out_rad, sbmc_s, llpm, npix,
                     S, out, ipt, has_hit, preview_out, preview_ipt);
  return check_launch("finish_sample_frame");
}

extern "C" int wcmc_assemble_kpcn_tiles(const float* kpcn, const float* llpm, const int* origins, int B, int H, int W, int S, int P,
                                        int pad, int t, float* diffuse_in, float* specular_in, float* diffuse_buffer,
                                        float* specular_buffer, float* albedo, float* paths, void* stream) {
  WCMC_REQUIRE(t >= 0 && t <= 7, WCMC_ERR_BAD_ARG, "assemble_kpcn_tiles: the transform code must lie in 0..7 (got %d)", t);
  WCMC_REQUIRE(kpcn && origins && diffuse_in && specular_in && diffuse_buffer && specular_buffer && albedo, WCMC_ERR_BAD_ARG,
               "assemble_kpcn_tiles: null pointer");
  WCMC_REQUIRE(!llpm || (paths && S > 0), WCMC_ERR_BAD_ARG, "assemble_kpcn_tiles: llpm needs a paths output and S > 0");
  WCMC_REQUIRE(B > 0 && H > 0 && W > 0 && P > 0 && pad >= 0, WCMC_ERR_BAD_ARG,
               "assemble_kpcn_tiles: B, H, W, P must be positive and pad non-negative");
  const int Ht = t & 1 ? W : H, Wt = t & 1 ? H : W;
  WCMC_REQUIRE(pad < Ht && pad < Wt, WCMC_ERR_BAD_ARG,
               "assemble_kpcn_tiles: pad = %d must be smaller than the transformed %d x %d frame (one reflection)", pad, Ht, Wt);
  WCMC_REQUIRE(P > 2 * pad, WCMC_ERR_BAD_ARG, "assemble_kpcn_tiles: a %d-pixel tile has no interior inside a pad of %d", P, pad);
  WCMC_REQUIRE(P <= Ht + 2 * pad && P <= Wt + 2 * pad, WCMC_ERR_BAD_ARG,
               "assemble_kpcn_tiles: a %d-pixel tile does not fit the transformed %d x %d frame extended by %d", P, Ht, Wt, pad);
  TileOut o{diffuse_in, specular_in, diffuse_buffer, specular_buffer, albedo, paths};
  const int64_t total = (int64_t)B * P * P;
  const dim3 grid((unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535));
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = aligned16(kpcn);
  if (vec && t)
    hipLaunchKernelGGL((ft_assemble_tiles_kernel<true, true>), grid, dim3(256), 0, st, kpcn, llpm, origins, o, B, H, W, S, P, pad, t);
  else if (t)
    hipLaunchKernelGGL((ft_assemble_tiles_kernel<false, true>), grid, dim3(256), 0, st, kpcn, llpm, origins, o, B, H, W, S, P, pad, t);
  else if (vec)
    hipLaunchKernelGGL((ft_assemble_tiles_kernel<true, false>), grid, dim3(256), 0, st, kpcn, llpm, origins, o, B, H, W, S, P, pad, 0);
  else
    hipLaunchKernelGGL((ft_assemble_tiles_kernel<false, false>), grid, dim3(256), 0, st, kpcn, llpm, origins, o, B, H, W, S, P, pad, 0);
  return check_launch("assemble_kpcn_tiles");
}

extern "C" int wcmc_stitch_tiles_aug(const float* rad, int64_t rsb, int64_t rsc, int64_t rsh, int64_t rsw, int ho, int wo, int P,
                                     const int* coords, int B, int t, int H, int W, int accumulate, float* out_rad, void* stream) {
  WCMC_REQUIRE(t >= 0 && t <= 7, WCMC_ERR_BAD_ARG, "stitch_tiles_aug: the transform code must lie in 0..7 (got %d)", t);
  WCMC_REQUIRE(rad && coords && out_rad, WCMC_ERR_BAD_ARG, "stitch_tiles_aug: null pointer");
  WCMC_REQUIRE(B > 0 && H > 0 && W > 0 && P > 0, WCMC_ERR_BAD_ARG, "stitch_tiles_aug: B, H, W, P must be positive");
  WCMC_REQUIRE((ho == P && wo == P) || (ho > 0 && wo > 0 && ho < P && wo < P), WCMC_ERR_BAD_ARG,
               "stitch_tiles_aug: the %d x %d network output must be P x P or smaller in both dimensions (P = %d)", ho, wo, P);
  WCMC_REQUIRE(accumulate == 0 || accumulate == 1, WCMC_ERR_BAD_ARG, "stitch_tiles_aug: accumulate must be 0 or 1 (got %d)",
               accumulate);
  WCMC_REQUIRE(B <= 65535, WCMC_ERR_BAD_ARG, "stitch_tiles_aug: at most 65535 tiles per launch");
  StitchAugArgs a{rad, rsb, rsc, rsh, rsw, coords, out_rad, ho, wo, P, H, W, t};
  const int64_t bx = ((int64_t)P * P * 3 + 255) / 256;
  if (accumulate)
    hipLaunchKernelGGL(ft_stitch_aug_kernel<true>, dim3((unsigned)(bx < 1024 ? bx : 1024), B), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ft_stitch_aug_kernel<false>, dim3((unsigned)(bx < 1024 ? bx : 1024), B), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("stitch_tiles_aug");
}

extern "C" int wcmc_finish_frame(const float* out_rad, const float* kpcn, const float* llpm, int H, int W, int S, float* out,
                                 float* ipt, float* has_hit, unsigned char* preview_out, unsigned char* preview_ipt, void* stream) {
  WCMC_REQUIRE(out_rad && kpcn && llpm && out && ipt && has_hit, WCMC_ERR_BAD_ARG, "finish_frame: null pointer");
  WCMC_REQUIRE(H > 0 && W > 0 && S > 0, WCMC_ERR_BAD_ARG, "finish_frame: H, W and S must be positive (got %d, %d, %d)", H, W, S);
  const int64_t npix = (int64_t)H * W;
  hipLaunchKernelGGL(ft_finish_frame_kernel, dim3(pp_grid(npix)), dim3(256), 0, (hipStream_t)stream, out_rad, kpcn, llpm, npix, S, out,
                     ipt, has_hit, preview_out, preview_ipt);
  return check_launch("finish_frame");
}
