/*
 * wcmc_hip.h -- C ABI of libwcmc_hip.so, the MI355X (gfx950) hot path of the
 * KPCN-Manifold training step (Mephisto405/WCMC).
 *
 * The reference is pure Python on PyTorch; the arithmetic of its hot path lives
 * in torch.nn / cuDNN and in the external `sbmc` package's Halide ops.  There is
 * no FFI in the reference for this path, so each entry point below names the
 * reference EXPRESSION it replaces (file:line under the reference tree) and is
 * what a ctypes binding under support/ would bind.
 *
 * Conventions
 *   - All tensors are fp32 device memory owned by the caller (PyTorch).  The
 *     library never allocates, frees or retains a pointer past return.
 *   - "NHWC view" = (ptr, N, H, W, C, sn, sh, sw): element (n,y,x,c) lives at
 *     ptr[n*sn + y*sh + x*sw + c]; the channel stride is 1.  ptr must be 16-byte
 *     aligned, sn/sh/sw multiples of 4, and sw >= round_up(C, 4) so that a 16-byte
 *     access that starts at a channel multiple of 4 stays inside the pixel.
 *     Slices of wider buffers (concat targets, cropped images) are expressed by
 *     the strides.
 *   - Every call only enqueues work on `stream` (a hipStream_t) and returns; no
 *     host synchronisation, no global mutable state except a thread-local error
 *     string.
 *   - Return value: 0 on success, a negative wcmc_status on failure;
 *     wcmc_last_error() then describes it.  Nothing aborts or throws.
 */
#ifndef WCMC_HIP_H
#define WCMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WCMC_ABI_VERSION 4     /* 2: `terms` of the GEMM entry points, packing mode 2 (round 3); round 4 widened the value ranges only (terms = 1, mode 3)
                                * 3: the four batch assemblers take `transforms, S_total, s` / `t`: the _prefix and _aug names are gone
                                * 4: the fused PathNet chains take `x_split, x_nchw, strides` / `h_hi` / `out, h_hi`: the _nchw, _save and _saved names are gone */

enum wcmc_status {
  WCMC_OK = 0,
  WCMC_ERR_BAD_ARG = -1,     /* null pointer, negative size, unsupported shape */
  WCMC_ERR_ALIGNMENT = -2,   /* pointer or stride violates the NHWC-view contract */
  WCMC_ERR_WORKSPACE = -3,   /* workspace too small */
  WCMC_ERR_LAUNCH = -4       /* hipGetLastError() after a launch */
};

enum wcmc_act { WCMC_ACT_LINEAR = 0, WCMC_ACT_RELU = 1, WCMC_ACT_LEAKY_RELU = 2 };

int wcmc_abi_version(void);
const char* wcmc_last_error(void);

/* ---------------------------------------------------------------- layout helpers
 * Strided copies between the reference's NCHW tensors (batch dict entries,
 * support/datasets.py:1080-1126) and NHWC views.  src element (n,c,y,x) at
 * src[n*ssn + c*ssc + y*ssh + x*ssw]. */
int wcmc_to_nhwc(const float* src, int64_t ssn, int64_t ssc, int64_t ssh, int64_t ssw,
                 float* dst, int64_t dsn, int64_t dsh, int64_t dsw,
                 int N, int C, int H, int W, void* stream);
int wcmc_from_nhwc(const float* src, int64_t ssn, int64_t ssh, int64_t ssw,
                   float* dst, int64_t dsn, int64_t dsc, int64_t dsh, int64_t dsw,
                   int N, int C, int H, int W, void* stream);

/* ---------------------------------------------------------------- convolution
 * Replaces torch.nn.Conv2d forward/backward inside sbmc.modules.ConvChain
 * (call sites support/networks.py:18-24, train_kpcn.py:213) -- the cuDNN calls
 * enabled at train_kpcn.py:349.
 *
 * Packed weights: wp[n][k], n in [0, Np), k in [0, Kt); k = tap*Kp + ci with
 * tap = ky*ks + kx, Kp = round_up(Cin,4), Kt = round_up(ks*ks*Kp, 32),
 * Np = round_up(Cout,16); padding entries are zero.
 *   mode 0 (forward operand):  wp[co][tap*Kp+ci] = w[co][ci][ky][kx]
 *   mode 1 (data-gradient operand, rows are INPUT channels):
 *                              wp[ci][tap'*Kp'+co] = w[co][ci][ks-1-ky'][ks-1-kx'],
 *                              Kp' = round_up(Cout,4), Np' = round_up(Cin,16)
 */
size_t wcmc_conv2d_packed_elems(int rows, int kchan, int ks);
int wcmc_conv2d_pack_weight(const float* w_oihw, float* wp, int Cout, int Cin, int ks, int mode,
                            void* stream);

/* y = act(conv(x, wp) + bias) [* gate'].  Implicit GEMM on fp32 MFMA.
 *   x: NHWC view (N,H,W,Cin); y: NHWC view (N,Ho,Wo,Cout), Ho = H + 2*pad - ks + 1.
 *   bias: [Cout] or NULL.  act/slope: wcmc_act applied to the result.
 *   gate (optional NHWC view with y's geometry): if non-NULL the result is
 *   multiplied by d act_gate / d pre-activation evaluated from the POST-activation
 *   value stored in gate (1 if gate>0 else gate_slope; gate_act = RELU uses slope 0).
 *   That is the fused ReLU backward used when this call computes a data gradient.
 */
int wcmc_conv2d_igemm(const float* x, int64_t xsn, int64_t xsh, int64_t xsw,
                      int N, int H, int W, int Cin,
                      const float* wp, const float* bias,
                      float* y, int64_t ysn, int64_t ysh, int64_t ysw, int Cout,
                      int ks, int pad, int act, float slope,
                      const float* gate, int64_t gsn, int64_t gsh, int64_t gsw,
                      int gate_act, float gate_slope, void* stream);

/* Weight gradient dW[co][ci][ky][kx] = sum_{n,y,x} dy[n,y,x,co] * x[n,y+ky-pad,x+kx-pad,ci]
 * (+ bias gradient db[co] = sum dy) written in the parameter's own OIHW layout.
 * Two launches inside: split-K partial slabs into `workspace`, then a fixed-order
 * reduction (bitwise reproducible).  db may be NULL. */
size_t wcmc_conv2d_wgrad_workspace_bytes(int N, int Ho, int Wo, int Cout, int Cin, int ks);
int wcmc_conv2d_wgrad(const float* x, int64_t xsn, int64_t xsh, int64_t xsw,
                      int N, int H, int W, int Cin,
                      const float* dy, int64_t dsn, int64_t dsh, int64_t dsw, int Cout,
                      int ks, int pad, float* dw_oihw, float* db,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Strided channel-first (N,C,H,W) fp32 -> dense split tensor in one pass (element strides; C <= 64): the per-sample
 * path descriptors `paths` (support/networks.py:31-33) are only read as the embedding chain's split input. */
int wcmc_split_from_nchw(const float* src, int64_t ssn, int64_t ssc, int64_t ssh, int64_t ssw, void* out_split, int N,
                         int C, int H, int W, void* stream);

/* ---------------------------------------------------------------- split-bf16 ("bf16x3") convolution
 * Same reference expressions as above (torch.nn.Conv2d fwd/bwd in sbmc.modules.ConvChain), computed
 * with every fp32 operand carried as two bf16 planes hi = bf16(x), lo = bf16(x - hi) and each product
 * as hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32 accumulation (~2^-17 relative per operand;
 * 5.3x the fp32-MFMA rate).  Chain-internal "split tensors" are dense u16 [N][H][W][2][Cp],
 * Cp = round_up(C,8), plane 0 = hi, plane 1 = lo, pad channels zero.  Packed weights:
 * u16 wp[Np][2][Kt], k = tap*round_up(kchan,8) + c, Kt = round_up(ks*ks*Kp, 32), Np = round_up(rows,16);
 * `mode` as for wcmc_conv2d_pack_weight. */
size_t wcmc_split_elems(int N, int H, int W, int C);
int wcmc_split_bf16(const float* x, int64_t xsn, int64_t xsh, int64_t xsw, void* out_split,
                    int N, int H, int W, int C, void* stream);
/* split(dy * act'(post)): the backward of a chain's output activation (wcmc_act_backward) folded into the split of
 * the upstream gradient; dy and post are fp32 NHWC views of the same geometry. */
int wcmc_split_gated_bf16(const float* dy, int64_t dsn, int64_t dsh, int64_t dsw, const float* post, int64_t psn,
                          int64_t psh, int64_t psw, int act, float slope, void* out_split, int N, int H, int W, int C,
                          void* stream);
/* cat([flat (B*S,C1,H,W), repeat_S(prop (B,C2,H,W))], 1) (support/networks.py:39-40) written directly as a
 * split tensor of B*S images with C1 + C2 channels; C1 % 8 == 0. */
int wcmc_cat_broadcast_split(const float* flat, int64_t fsn, int64_t fsh, int64_t fsw,
                             const float* prop, int64_t psn, int64_t psh, int64_t psw,
                             void* out_split, int B, int S, int H, int W, int C1, int C2, void* stream);
/* U-Net skip concatenation (sbmc.modules.Autoencoder: cat([upsample_x2(deeper), skip], 1) feeding a level's right
 * ConvChain): the bilinear upsampling (align_corners=False, as wcmc_upsample2_fwd) is evaluated on the fly and the
 * concatenation is written once, directly as the chain's split input.  deep: (N, C1, H/2, W/2), skip: (N, C2, H, W),
 * C1 % 8 == 0; the result equals wcmc_upsample2_fwd + wcmc_cat_broadcast_split(S = 1) bit for bit. */
int wcmc_cat_upsample_split(const float* deep, int64_t dsn, int64_t dsh, int64_t dsw, const float* skip, int64_t ssn,
                            int64_t ssh, int64_t ssw, void* out_split, int N, int H, int W, int C1, int C2,
                            void* stream);

/* split(g (B*S,C,H,W) + repeat_S(gm (B,C,H,W)) * scale): the gradient of a chain output that feeds both the
 * concatenation and the spp mean (support/networks.py:35-40), as the split dy of the chain's backward.  Either
 * gradient may be null. */
int wcmc_add_broadcast_split(const float* g, int64_t gsn, int64_t gsh, int64_t gsw,
                             const float* gm, int64_t msn, int64_t msh, int64_t msw, float scale,
                             void* out_split, int B, int S, int H, int W, int C, void* stream);
/* The gradient that ENTERS a chain's backward, split, with the column sums of the result (= the last layer's bias
 * gradient, `interfaces.py:237-238` -> `nn.Conv2d` backward) in the same pass:
 *   out = split((dy [+ repeat_S(gm) * scale]) [* act'(post)])      -- dy or gm may be null, post may be null --
 * i.e. wcmc_split_bf16 / wcmc_split_gated_bf16 / wcmc_add_broadcast_split, plus colsum_partial in the layout of
 * wcmc_conv2d_igemm_bf16x3's column sums (wcmc_conv2d_igemm_colsum_elems floats), to be handed to
 * wcmc_conv2d_wgrad_bf16x3 as dy_colsum_partial.  N = B * S images when gm (B images) is given. */
int wcmc_split_dy_colsum_bf16(const float* dy, int64_t dsn, int64_t dsh, int64_t dsw,
                              const float* post, int64_t psn, int64_t psh, int64_t psw, int act, float slope,
                              const float* gm, int64_t msn, int64_t msh, int64_t msw, int S, float scale,
                              void* out_split, float* colsum_partial, int N, int H, int W, int C, void* stream);
/* mode: 0 = forward orientation (rows = Cout, k over Cin x taps); 1 = data-gradient orientation (rows = Cin, k over
 * Cout x flipped taps) for a three-term launch; 2 = the same orientation in the K order of a TWO-term launch
 * (wcmc_conv2d_igemm_bf16x3 with terms = 2: the channel slabs are twice as wide, see there); 3 = the FORWARD orientation in
 * that K order (a forward launch with terms = 2 or 1: round 4, the un-gated output layers of the "bf16x321o" mode); 4 = mode 3
 * with the weights rounded once to fp16 in the hi rows (wcmc_conv2d_out_f16). */
size_t wcmc_conv2d_packed_elems_bf16x3(int rows, int kchan, int ks, int mode);
int wcmc_conv2d_pack_weight_bf16x3(const float* w_oihw, void* wp, int Cout, int Cin, int ks, int mode,
                                   void* stream);
/* The same for up to 32 (layer, mode) pairs (one chain, or the chains of one U-Net) in ONE launch: w[i] OIHW (Cout[i], Cin[i], ks, ks) ->
 * wp[i] (wcmc_conv2d_packed_elems_bf16x3(rows, kchan, ks, mode) u16 each), mode[i] as above; host arrays of n_entries items. */
int wcmc_conv2d_pack_chain_bf16x3(int n_entries, const float* const* w, void* const* wp, const int* Cout,
                                  const int* Cin, const int* mode, int ks, void* stream);
/* Exactly one of y (fp32 NHWC view) and y_split (dense split tensor) receives the result.
 * gate_split (optional, geometry of the output, requires y_split): fused activation-derivative
 * mask evaluated from the hi plane of the post-activation tensor.
 * mask_out (optional, with y_split): uint8 [N*Ho*Wo][round_up(Cout,8)/8], bit c%8 of byte c/8 = (hi plane of
 * output channel c > 0) -- the same predicate at 1/16 of the bytes; gate_mask (optional, instead of gate_split):
 * such a mask of a tensor with the output's geometry.
 * terms: bf16 MFMAs per product -- 3 = W_lo*x_hi + W_hi*x_lo + W_hi*x_hi (the forward); 2 = W_lo*x_hi + W_hi*x_hi, i.e.
 * x rounded to its hi plane (8 mantissa bits), W exact to 16 -- the data gradient of the default mode, whose x operand is
 * dy (wp then packed with mode 2).  Where no two-term kernel instance exists for the shape the launch runs three terms
 * (the packing of mode 2 follows the same rule, so the pair stays consistent).  Replaces the data gradient of
 * `nn.Conv2d` under cuDNN (train_kpcn.py:349; TF32 by default on the reference's hardware: 10 bits on BOTH operands).
 * 1 = W_hi*x_hi only (8 bits on both operands; wp packed with mode 3; round 4): the forward of a 5x5 layer whose output no
 * activation gates -- sbmc.KPCN's kernel-predicting output layers (call site support/interfaces.py:203-204) -- where a
 * rounding cannot flip a ReLU unit; granted where the hi-plane instance of the 64-pixel 5x5 kernel exists (cout blocks of
 * seven tiles, input channels not 24 mod 32), anywhere else the launch runs the plan's two or three terms. */
int wcmc_conv2d_igemm_bf16x3(const void* x_split, int N, int H, int W, int Cin,
                             const void* wp, const float* bias,
                             float* y, int64_t ysn, int64_t ysh, int64_t ysw, void* y_split, int Cout,
                             int ks, int pad, int act, float slope,
                             const void* gate_split, int gate_act, float gate_slope,
                             float* colsum_partial, const void* gate_mask, void* mask_out, int terms, void* stream);
/* Round 4: the forward of an un-gated 5x5 OUTPUT layer with ONE fp16 MFMA per product (the "bf16x321h" mode; sbmc.KPCN's
 * kernel-predicting output layers, call site support/interfaces.py:203-204).  Both operands are rounded ONCE to fp16 (11 bits;
 * the reference's own cuDNN path rounds both to TF32's 10, train_kpcn.py:349): x by wcmc_split_to_f16 (split tensor ->
 * [N*H*W][round_up(C,8)] halfs, saturating), the weights by wcmc_conv2d_pack_weight_bf16x3 with mode 4.  No activation follows
 * the layer, so no ReLU gate can flip (profiles/r04_forward_ladder.txt: every HIDDEN layer needs >= 16-bit operands).
 * wcmc_conv2d_out_f16_supported: 5x5, cout blocks of seven tiles, input channels not 24 mod 32 (the hi-plane instance of the
 * 64-pixel kernel); y = conv(x, W) + bias as an fp32 NHWC view, linear. */
int wcmc_conv2d_out_f16_supported(int Cin, int Cout, int ks);
size_t wcmc_split_to_f16_elems(int N, int H, int W, int C);
int wcmc_split_to_f16(const void* x_split, int N, int H, int W, int C, void* out_f16, void* stream);
int wcmc_conv2d_out_f16(const void* x_f16, int N, int H, int W, int Cin, const void* wp_f16, const float* bias, float* y,
                        int64_t ysn, int64_t ysh, int64_t ysw, int Cout, int ks, int pad, void* stream);
/* colsum_partial (optional, with y_split): [wcmc_conv2d_igemm_colsum_elems] floats that receive the
 * per-pixel-tile column sums of the result -- the bias gradient of the layer that consumes this
 * data gradient, finished by wcmc_colsum_finish (saves a pass over dy per layer).  The buffer ends with a trailer
 * word: the number of rows the producing launch wrote, which is all wcmc_colsum_finish reads. */
/* Two 1x1 layers in one launch (sbmc.modules.ConvChain with ksize 1: the last two layers of PathNet.final and of
 * PathNet.embedding, support/networks.py:22-27,33-41, and the data gradient of the former): y1 = gate * act1(W1 x + b1)
 * is written as a split tensor -- with its 1-bit mask (mask1) on the forward, gated by gate_mask1 and with column
 * sums (colsum1, see below) on the backward, exactly as wcmc_conv2d_igemm_bf16x3 would -- and y2 = act2(W2 y1 + b2)
 * (fp32 NHWC view) is computed from the tile while it is on chip, so the hidden tensor is not re-read by a second
 * launch.  wcmc_conv1x1_pair_supported says whether a fused instance exists for the channel counts (else: two
 * wcmc_conv2d_igemm_bf16x3 launches, same results bit for bit).  wp1 / wp2: wcmc_conv2d_pack_weight_bf16x3. */
int wcmc_conv1x1_pair_supported(int Cin, int Cout1, int Cout2);
int wcmc_conv1x1_pair_bf16x3(const void* x_split, int N, int H, int W, int Cin, const void* wp1, const float* bias1,
                             int Cout1, int act1, float slope1, void* y1_split, void* mask1, const void* gate_mask1,
                             int gate_act1, float gate_slope1, float* colsum1, const void* wp2, const float* bias2,
                             int Cout2, int act2, float slope2, float* y2, int64_t y2sn, int64_t y2sh, int64_t y2sw,
                             void* stream);
/* ---------------------------------------------------------------- PathNet.embedding, fused (support/networks.py:33-36)
 * y = ConvChain(Cin -> 64 -> 64 -> 64, ksize 1, ReLU, ReLU, linear)(x) over M = B*S*H*W pixels as ONE launch per direction:
 * the hidden activations never leave the chip (forward) and are recomputed from x (backward).
 *   x_split   split tensor [M][2][round_up(Cin, 8)] (wcmc_split_from_nchw / wcmc_split_bf16)
 *   wp0..wp2  forward packs (wcmc_conv2d_pack_weight_bf16x3, mode 0), wt1 / wt2 data-gradient packs (mode 1) of layers 1, 2
 *   y         fp32 [M][64] (an NHWC tensor of 64 channels); bit-identical to three wcmc_conv2d_igemm_bf16x3 launches
 *   backward  dy = gy (fp32, pixel stride gy_pixel_stride floats; may be null) + repeat_S(gm) * gm_scale (gm: fp32 over
 *             M / S pixels, B images of HW pixels; may be null) -- the gradient of `y` and of its spp mean
 *             (support/networks.py:35-36) -- and dw / db of the three layers (OIHW, ks = 1) in the default mode's arithmetic
 *             (data gradients dy_hi x (W_hi + W_lo), weight gradients hi x hi); no gradient for x.  Fixed summation order:
 *             bitwise reproducible. */
int wcmc_embed3_supported(int Cin, int C1, int C2, int C3);
size_t wcmc_embed3_bwd_workspace_bytes(void);
int wcmc_embed3_fwd(const void* x_split, int64_t M, int Cin, const void* wp0, const float* b0, const void* wp1,
                    const float* b1, const void* wp2, const float* b2, float* y, void* stream);
/* The same forward with the spp mean of y leaving in the same launch (support/networks.py:35-36: y.view(B, S, ...).mean(1)):
 * y_mean fp32 [M / S][64], the sums formed s ascending in fp32 and multiplied by 1 / S -- bit-identical to wcmc_spp_reduce on
 * the stored y, which is then not read again.  M = B * S * HW with HW % 64 == 0 (wcmc_embed3_mean_supported).
 * wcmc_embed3_mean_fwd and wcmc_embed3_bwd take x in one of two forms; EXACTLY ONE of x_split / x_nchw is non-null (both, or
 * neither: WCMC_ERR_BAD_ARG, before anything else):
 *   x_split  the split tensor, as in wcmc_embed3_fwd; the two strides are ignored.
 *   x_nchw   x WHERE IT LIES: fp32, channel-first -- N = M / HW samples of Cin channel planes of HW floats, sample / channel
 *            stride x_sample_stride / x_channel_stride floats (a slice of a larger buffer in N and C is fine), each H x W plane
 *            contiguous -- instead of its split copy (`paths` arrives channel-first, support/networks.py:31-33, and this chain is
 *            its only reader: the split copy was a pass over memory of its own).  The kernels load a tile's Cin rows of 64 pixels
 *            and split them with wcmc_split_from_nchw's arithmetic on the way into the LDS tile, so y, y_mean and the six gradients
 *            equal those of the x_split form BIT FOR BIT.  wcmc_embed3_nchw_supported (host only, no device needed): Cin <= 64,
 *            H * W % 64 == 0 (a 64-pixel tile lies in one sample), sw == 1 and sh == W (a contiguous plane), sc >= H * W; anything
 *            else takes the split copy.  x_nchw needs 4-byte alignment only. */
int wcmc_embed3_mean_supported(int S, int64_t HW);
int wcmc_embed3_nchw_supported(int Cin, int64_t N, int64_t H, int64_t W, int64_t sn, int64_t sc, int64_t sh, int64_t sw);
int wcmc_embed3_mean_fwd(const void* x_split, const float* x_nchw, int64_t x_sample_stride, int64_t x_channel_stride, int64_t M,
                         int Cin, const void* wp0, const float* b0, const void* wp1, const float* b1, const void* wp2,
                         const float* b2, float* y, float* y_mean, int S, int64_t HW, void* stream);
int wcmc_embed3_bwd(const void* x_split, const float* x_nchw, int64_t x_sample_stride, int64_t x_channel_stride, int64_t M,
                    int Cin, const void* wp0, const float* b0, const void* wp1, const float* b1, const void* wt1,
                    const void* wt2, const float* gy, int gy_pixel_stride, const float* gm, int gm_pixel_stride, int S,
                    int64_t HW, float gm_scale, float* dw0, float* db0, float* dw1, float* db1, float* dw2, float* db2,
                    void* workspace, size_t workspace_bytes, void* stream);
/* ---------------------------------------------------------------- PathNet.final, fused (support/networks.py:39-42)
 * out = ConvChain(128 -> 128 -> outc <= 8, ksize 1, ReLU, ReLU)(cat([y, repeat_S(prop)], 1)): y fp32 over M = B*S*HW pixels
 * (64 channels, pixel stride y_pixel_stride floats), prop fp32 over B*HW pixels (64 channels), out / gout fp32 [M][os] with
 * os = 4 for outc <= 4, else 8 (an NHWC view of outc channels; round 4: up to eight, the reference's --pnet_out_size 6 runs,
 * train_kpcn.py:209-212); HW % 64 == 0.  The concatenation is never written.  The backward writes dy [M][64] and dprop [B*HW][64]
 * (the sum over the S samples) and the weight / bias gradients (OIHW, ks = 1) in the default mode's arithmetic.  Forward
 * bit-identical to wcmc_cat_broadcast_split + wcmc_conv1x1_pair_bf16x3.
 *   wp0 / wp1  forward packs (mode 0) of the two layers, wt0 / wt1 their data-gradient packs (mode 1).
 * All the backward uses of the hidden activation is its bf16 hi plane (ReLU gate, one-term dW1), all it uses of out is its sign.
 * It either recomputes both or reads them from the forward:
 *   wcmc_final2_fwd  h_hi null: nothing but out is written.  h_hi non-null: also writes h_hi, a dense bf16 plane [M][128] (256 B
 *                    per pixel); out is bit for bit the same.
 *   wcmc_final2_bwd  out and h_hi both null: recomputes the hidden activation and out from y and prop.  Both non-null: reads that
 *                    h_hi, and out as the forward wrote it (read only): no recomputation (58 instead of 118 MFMAs per 64-pixel
 *                    tile and wave), all eight results bit for bit the same.  Exactly one of them null: WCMC_ERR_BAD_ARG.
 * Errors before any launch, after those of the other arguments: out without h_hi or h_hi without out in the backward
 * WCMC_ERR_BAD_ARG, an h_hi / out that is not 16-byte aligned WCMC_ERR_ALIGNMENT (the output of the forward, null or misaligned:
 * WCMC_ERR_BAD_ARG), then a short workspace WCMC_ERR_WORKSPACE (wcmc_final2_bwd_workspace_bytes() serves both forms). */
int wcmc_final2_supported(int C1, int C2, int Chid, int outc, int64_t HW);
size_t wcmc_final2_bwd_workspace_bytes(void);
int wcmc_final2_fwd(const float* y, int y_pixel_stride, const float* prop, int prop_pixel_stride, int B, int S, int64_t HW,
                    const void* wp0, const float* b0, const void* wp1, const float* b1, int outc, float* out, void* h_hi,
                    void* stream);
int wcmc_final2_bwd(const float* y, int y_pixel_stride, const float* prop, int prop_pixel_stride, int B, int S, int64_t HW,
                    const void* wp0, const float* b0, const void* wp1, const float* b1, int outc, const void* wt0,
                    const void* wt1, const float* gout, const float* out, const void* h_hi, float* dy, float* dprop,
                    float* dw0, float* db0, float* dw1, float* db1, void* workspace, size_t workspace_bytes, void* stream);
size_t wcmc_conv2d_igemm_colsum_elems(int N, int Ho, int Wo, int Cout);
int wcmc_colsum_finish(const float* partial, int N, int Ho, int Wo, int Cout, float* db, void* stream);
/* Which kernel a launch WOULD run, from the code that launches, without touching the device (no GPU needed).  Each writes two
 * NUL-terminated strings into caller buffers of `len` bytes and returns 0: cls = the profiler class (conv_pw | conv_halo3[_x2] |
 * conv_halo64_pt3|pt4[_x2|_x1|_h1] | conv_halo64_cs32 | conv_halo7 | conv_igemm; conv_wgrad_rows | conv_wgrad -- a class that
 * stands for ONE kernel instance is given to that instance only, any other kernel gets conv_igemm / conv_wgrad) and kernel = the
 * instance as rocprofv3 prints it without "wcmc::", every template argument written out.  Arguments the launch would refuse (and
 * buffers too short) return the launch's error code, message in wcmc_last_error -- those that can be told from these scalars: the
 * launch also refuses an fp32 output with a gate MASK or a mask output, and misaligned or missing buffers, which the query is not
 * told about.  (Both launches check the shape first: of several bad arguments, WCMC_ERR_BAD_ARG for the shape is the one reported,
 * before WCMC_ERR_ALIGNMENT and WCMC_ERR_WORKSPACE.)  The debug library follows its A/B switches.
 * wcmc_conv2d_launch_plan_bf16x3: wcmc_conv2d_igemm_bf16x3 (split_out: y_split given, else y with the strides ysn / ysh / ysw;
 * gate_tensor: gate_split given) or, with out_f16 != 0, wcmc_conv2d_out_f16.  wcmc_conv2d_wgrad_launch_plan_bf16x3: the GEMM
 * launch (phase 0 or 1) of wcmc_conv2d_wgrad_bf16x3. */
int wcmc_conv2d_launch_plan_bf16x3(int N, int H, int W, int Cin, int Cout, int ks, int pad, int terms, int split_out,
                                   int64_t ysn, int64_t ysh, int64_t ysw, int gate_tensor, int out_f16,
                                   char* cls, char* kernel, size_t len);
int wcmc_conv2d_wgrad_launch_plan_bf16x3(int N, int H, int W, int Cin, int Cout, int ks, int pad, int terms,
                                         char* cls, char* kernel, size_t len);
size_t wcmc_conv2d_wgrad_bf16x3_workspace_bytes(int N, int Ho, int Wo, int Cout, int Cin, int ks);
/* phase: 0 = everything; 1 = the split-K GEMM into the workspace only; 2 = the slab reduction and
 * bias gradient only (1 then 2 == 0; lets a profiler bracket the GEMM launch alone).
 * dy_colsum_partial (optional): the per-tile column sums of dy that the launch which PRODUCED dy left
 * (wcmc_conv2d_igemm_bf16x3 / wcmc_conv1x1_pair_bf16x3 colsum output, wcmc_conv2d_igemm_colsum_elems floats): the bias
 * gradient db is then finished from them by extra blocks of the slab-reduction launch -- same sums, same order as
 * wcmc_colsum_finish, bit for bit -- instead of a column-sum pass over dy plus a finish launch.
 * terms: bf16 MFMAs per product -- 3 = dy_lo*x_hi + dy_hi*x_lo + dy_hi*x_hi; 1 = dy_hi*x_hi only (the lo planes are not
 * read: half the operand bytes).  The reference's counterpart is cuDNN's weight gradient under
 * `torch.backends.cudnn.allow_tf32` (train_kpcn.py:349 leaves the default, TF32 = 10 mantissa bits per operand). */
/* Phase 2 of up to 32 wcmc_conv2d_wgrad_bf16x3 calls in ONE launch: layer i's split-K slabs (workspace[i], filled by a phase-1
 * call with the same N, Ho, Wo, Cout, Cin, ks and terms) are summed into dw[i], and db[i] (optional) is finished from
 * dy_colsum_partial[i] (required with db[i]).  Bit-identical to the per-layer phase 2.  The U-Net's fifteen weight gradients per
 * PathNet and backward pass are reduced by one launch at the end of the chain walk instead of fifteen between its GEMMs. */
int wcmc_conv2d_wgrad_reduce_multi(int n, void* const* workspace, float* const* dw, float* const* db,
                                   const float* const* dy_colsum_partial, const int* N, const int* Ho, const int* Wo,
                                   const int* Cout, const int* Cin, const int* ks, int terms, void* stream);
int wcmc_conv2d_wgrad_bf16x3(const void* x_split, int N, int H, int W, int Cin,
                             const void* dy_split, int Cout, int ks, int pad, float* dw, float* db,
                             void* workspace, size_t workspace_bytes, int phase, const float* dy_colsum_partial,
                             int terms, void* stream);

/* dx = dy * act'(y) from the post-activation value y (NHWC views of equal geometry). */
int wcmc_act_backward(const float* dy, int64_t dsn, int64_t dsh, int64_t dsw,
                      const float* y, int64_t ysn, int64_t ysh, int64_t ysw,
                      float* dx, int64_t xsn, int64_t xsh, int64_t xsw,
                      int N, int H, int W, int C, int act, float slope, void* stream);

/* ---------------------------------------------------------------- kernel apply
 * Replaces sbmc.modules.KernelApply(softmax=True, splat=False) inside sbmc.KPCN
 * (call site support/interfaces.py:203-204; upstream a Halide op).
 *   logits: NHWC view (N,h,w,k*k) -- tap t = (dy+r)*k + (dx+r), r = k/2.
 *   data/out: (N,C,h,w) with arbitrary element strides (sn,sc,sh,sw), C <= 4.
 *   out[n,c,y,x] = sum_t softmax_t(logits[n,y,x,:]) * data0[n,c,y+dy,x+dx],
 *   data0 = data zero-extended outside [0,h)x[0,w).
 *   lse: [N*h*w] per-pixel log-sum-exp saved for the backward (may be NULL).
 */
int wcmc_kernel_apply_fwd(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw,
                          const float* data, int64_t dsn, int64_t dsc, int64_t dsh, int64_t dsw,
                          float* out, int64_t osn, int64_t osc, int64_t osh, int64_t osw,
                          float* lse, int N, int C, int h, int w, int k, void* stream);
/* d_logits (NHWC view, same geometry as logits) from grad_out; d_data (N,C,h,w
 * contiguous, accumulated with atomics, must be zeroed by the caller) may be NULL. */
int wcmc_kernel_apply_bwd(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw,
                          const float* data, int64_t dsn, int64_t dsc, int64_t dsh, int64_t dsw,
                          const float* out, int64_t osn, int64_t osc, int64_t osh, int64_t osw,
                          const float* grad_out, int64_t gsn, int64_t gsc, int64_t gsh, int64_t gsw,
                          const float* lse,
                          float* d_logits, int64_t qsn, int64_t qsh, int64_t qsw,
                          float* d_data, int N, int C, int h, int w, int k, void* stream);

/* ---------------------------------------------------------------- kernel splat
 * Replaces sbmc.modules.KernelApply(softmax=True, splat=True) and the per-sample step of
 * sbmc.modules.ProgressiveKernelApply(splat=True) inside sbmc.Multisteps (upstream: the Halide
 * ops Scatter2Gather + KernelWeighting).  Specification: DESIGN.md section 18.
 *   logits: NHWC view (N,h,w,k2), k2 = k*k, k odd, k <= 21 -- tap t = (dy+r)*k + (dx+r), r = k/2.
 *   data: (N,C,h,w) with arbitrary element strides (sn,sc,sh,sw), C <= 4.
 *   A source pixel q sends tap t to the destination q + (dy,dx); destinations outside the image are dropped:
 *     sum_r[n,c,p] (+)= sum over (q,t), q + off(t) = p, of w[n,q,t] * data[n,c,q],   sum_w[n,p] (+)= the same sum of w,
 *     w[n,q,t] = exp(logits[n,q,t] - m) * s
 *       mode WCMC_SPLAT_SOFTMAX: m = max_t logits[n,q,:], s = 1 / sum_t exp(logits[n,q,t] - m); lse [N*h*w] receives the
 *                                per-source log-sum-exp for the backward (may be NULL);
 *       mode WCMC_SPLAT_SHIFT:   m = shift[n] (device, (N,)), s = 1.
 *   sum_r (N,C,h,w) and sum_w (N,h,w) are contiguous; accumulate = 0 overwrites them, else they are added into.
 *   Two launches and no atomics: every sum has a fixed order, the results are bitwise reproducible.
 *   workspace: wcmc_kernel_splat_fwd_workspace_bytes(N, C, h, w, k2) bytes (0 for an unsupported shape).
 */
enum wcmc_splat_mode { WCMC_SPLAT_SOFTMAX = 0, WCMC_SPLAT_SHIFT = 1 };
size_t wcmc_kernel_splat_fwd_workspace_bytes(int N, int C, int h, int w, int k2);
int wcmc_kernel_splat_fwd(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw,
                          const float* data, int64_t dsn, int64_t dsc, int64_t dsh, int64_t dsw,
                          float* sum_r, float* sum_w, float* lse, int mode, const float* shift,
                          int accumulate, void* workspace, size_t workspace_bytes,
                          int N, int C, int h, int w, int k2, void* stream);
/* G[q,t] = sum_c data[c,q] * g_r[c,q+off(t)] + g_w[q+off(t)] (0 outside); either of g_r (N,C,h,w strided) and g_w
 * (N,h,w strided) may be NULL, not both.
 *   d_data[c,q]   = sum_t w[q,t] * g_r[c,q+off(t)]           ((N,C,h,w) contiguous, written, may be NULL)
 *   d_logits[q,t] = w * G (shift mode),  w * (G - sum_u w[q,u] G[q,u]) (softmax mode; lse as the forward wrote it)
 * Both are gathers around the source pixel: no atomics, bitwise reproducible. */
int wcmc_kernel_splat_bwd(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw,
                          const float* data, int64_t dsn, int64_t dsc, int64_t dsh, int64_t dsw,
                          const float* g_r, int64_t gsn, int64_t gsc, int64_t gsh, int64_t gsw,
                          const float* g_w, int64_t wsn, int64_t wsh, int64_t wsw,
                          const float* lse, int mode, const float* shift,
                          float* d_logits, int64_t qsn, int64_t qsh, int64_t qsw,
                          float* d_data, int N, int C, int h, int w, int k2, void* stream);
/* out[n] = max over (t,y,x) of logits[n] (``kernels.amax(dim=(1, 2, 3))``: a NaN logit gives NaN), the running shift of
 * ProgressiveKernelApply.  Two launches in a fixed order; workspace: wcmc_logit_max_workspace_bytes(N). */
size_t wcmc_logit_max_workspace_bytes(int N);
int wcmc_logit_max(const float* logits, int64_t lsn, int64_t lsh, int64_t lsw, float* out,
                   void* workspace, size_t workspace_bytes, int N, int h, int w, int k2, void* stream);

/* Tail of sbmc.KPCN.forward (result keys consumed at support/interfaces.py:207-211):
 *   radiance = albedo * r_diffuse + exp(r_specular) - 1.
 * Inputs (N,C,H,W) with arbitrary element strides; out / grad_out / d_* contiguous (N,C,H,W). */
int wcmc_recombine_fwd(const float* albedo, int64_t asn, int64_t asc, int64_t ash, int64_t asw,
                       const float* r_diffuse, int64_t dsn, int64_t dsc, int64_t dsh, int64_t dsw,
                       const float* r_specular, int64_t ssn, int64_t ssc, int64_t ssh, int64_t ssw,
                       float* out, int N, int C, int H, int W, void* stream);
int wcmc_recombine_bwd(const float* grad_out,
                       const float* albedo, int64_t asn, int64_t asc, int64_t ash, int64_t asw,
                       const float* r_specular, int64_t ssn, int64_t ssc, int64_t ssh, int64_t ssw,
                       float* d_diffuse, float* d_specular, int N, int C, int H, int W, void* stream);

/* Image losses on the (N,C,H,W) outputs: torch.nn.L1Loss (train_kpcn.py:299-304; applied at
 * support/interfaces.py:213-249) and RelativeMSE (support/losses.py:245-264: 0.5 * mean((x - ref)^2 / (ref^2 + eps))) of
 * one pair in one pass; either output may be null.  Both tensors with arbitrary element strides.  Deterministic
 * (fixed-order two-level sum).  wcmc_l1_mean_bwd: dx = grad_loss[0] * sign(x - ref) / (N*C*H*W), contiguous (N,C,H,W). */
size_t wcmc_image_loss_workspace_bytes(void);
int wcmc_image_loss_fwd(const float* x, int64_t xsn, int64_t xsc, int64_t xsh, int64_t xsw,
                        const float* ref, int64_t rsn, int64_t rsc, int64_t rsh, int64_t rsw, float eps,
                        float* l1_mean, float* relative_mse, void* workspace, size_t workspace_bytes,
                        int N, int C, int H, int W, void* stream);
int wcmc_l1_mean_bwd(const float* x, int64_t xsn, int64_t xsc, int64_t xsh, int64_t xsw,
                     const float* ref, int64_t rsn, int64_t rsc, int64_t rsh, int64_t rsw,
                     const float* grad_loss, float* dx, int N, int C, int H, int W, void* stream);

/* ---------------------------------------------------------------- U-Net glue
 * F.max_pool2d(x,2,2) / F.interpolate(x, scale_factor=2, 'bilinear',
 * align_corners=False) inside sbmc.modules.Autoencoder (support/networks.py:20-22). */
int wcmc_maxpool2_fwd(const float* x, int64_t xsn, int64_t xsh, int64_t xsw,
                      float* y, int64_t ysn, int64_t ysh, int64_t ysw,
                      int N, int H, int W, int C, void* stream);
/* dx[n,2y+i,2x+j] = dy[n,y,x] where x[...] is the (first) maximum of its window, else 0. */
/* dx = maxpool2's gradient + add: the pooled tensor also feeds a skip connection, whose gradient `add` (fp32 NHWC view of x's
 * geometry) is summed in by the same pass (the sum autograd would form with one more elementwise launch). */
int wcmc_maxpool2_bwd_add(const float* x, int64_t xsn, int64_t xsh, int64_t xsw, const float* dy, int64_t dsn, int64_t dsh,
                          int64_t dsw, const float* add, int64_t asn, int64_t ash, int64_t asw, float* dx, int64_t gsn,
                          int64_t gsh, int64_t gsw, int N, int H, int W, int C, void* stream);
int wcmc_maxpool2_bwd(const float* x, int64_t xsn, int64_t xsh, int64_t xsw,
                      const float* dy, int64_t dsn, int64_t dsh, int64_t dsw,
                      float* dx, int64_t gsn, int64_t gsh, int64_t gsw,
                      int N, int H, int W, int C, void* stream);
/* (N,H,W,C) -> (N,2H,2W,C) */
int wcmc_upsample2_fwd(const float* x, int64_t xsn, int64_t xsh, int64_t xsw,
                       float* y, int64_t ysn, int64_t ysh, int64_t ysw,
                       int N, int H, int W, int C, void* stream);
/* dy (N,2H,2W,C) -> dx (N,H,W,C) (gather form of the transposed interpolation) */
int wcmc_upsample2_bwd(const float* dy, int64_t dsn, int64_t dsh, int64_t dsw,
                       float* dx, int64_t xsn, int64_t xsh, int64_t xsw,
                       int N, int H, int W, int C, void* stream);

/* ---------------------------------------------------------------- PathNet glue
 * support/networks.py:35-36 (`flat.mean(1)`) and :39-40 (`repeat` + `cat`).
 * x holds B*S images, y holds B images (image b*S+s belongs to patch b).
 *   reduce:    y[b] = scale * sum_s x[b*S+s]
 *   broadcast: y[b*S+s] = (accumulate ? y[b*S+s] : 0) + scale * x[b]            */
int wcmc_spp_reduce(const float* x, int64_t xsn, int64_t xsh, int64_t xsw,
                    float* y, int64_t ysn, int64_t ysh, int64_t ysw,
                    int B, int S, int H, int W, int C, float scale, void* stream);
int wcmc_spp_broadcast(const float* x, int64_t xsn, int64_t xsh, int64_t xsw,
                       float* y, int64_t ysn, int64_t ysh, int64_t ysw,
                       int B, int S, int H, int W, int C, float scale, int accumulate,
                       void* stream);

/* Per-sample feature assembly of the sample-based denoisers (SBMCInterface / LBMCInterface,
 * support/interfaces.py:394-403, :797-806): out (B, S, C + Cp + 1, H, W, contiguous) =
 * cat([features (B,S,C,H,W), P (B,S,Cp,H,W), repeat_S(P.var(1).mean(1, keepdims) / S)], 2); element strides for the
 * two inputs.  The variance channel carries no gradient (.detach() in the reference): the backward is two slices. */
int wcmc_sample_cat_fwd(const float* feat, int64_t fsb, int64_t fss, int64_t fsc, int64_t fsh, int64_t fsw,
                        const float* p, int64_t psb, int64_t pss, int64_t psc, int64_t psh, int64_t psw, float* out,
                        int B, int S, int C, int Cp, int H, int W, void* stream);

/* ---------------------------------------------------------------- P-buffer statistics
 * support/interfaces.py:165-176: builds the KPCN input
 *   out = cat([base, mean_s P, (var_s P (unbiased)).mean_c / S], channel)
 * base: (B,Cb,H,W) strided NCHW-style tensor; P: (B,S,Cp,H,W) strided;
 * out: NHWC view (B,H,W,Cb+Cp+1).  The backward of the mean term is
 *   dP[b,s,c,y,x] = g[b,y,x,Cb+c] / S   (the variance term is detached, :165).   */
int wcmc_pbuffer_cat_fwd(const float* base, int64_t bsn, int64_t bsc, int64_t bsh, int64_t bsw,
                         const float* p, int64_t psb, int64_t pss, int64_t psc, int64_t psh,
                         int64_t psw,
                         float* out, int64_t osn, int64_t osh, int64_t osw,
                         int B, int S, int Cb, int Cp, int H, int W, void* stream);
int wcmc_pbuffer_cat_bwd(const float* g, int64_t gsn, int64_t gsh, int64_t gsw,
                         float* dp, int64_t psb, int64_t pss, int64_t psc, int64_t psh,
                         int64_t psw,
                         int B, int S, int Cb, int Cp, int H, int W, void* stream);

/* ---------------------------------------------------------------- FeatureMSE
 * support/losses.py:33-61,63-65,82-113 (path-disentangling loss, color='rgb').
 * p: (B,S,C,h,w) strided view (already cropped), C <= 8; ref: (B,3,h,w) strided
 * (NOT yet tonemapped).  idx_patch: permutation of S*h*w (int64, device);
 * idx_batch: permutation of B*S*h*w or NULL for non_local=False.
 * workspace layout is private; loss is a single float.  The forward leaves in the
 * workspace what the backward needs (tonemapped ref, displacements, inverse
 * permutations), so the same workspace must be passed to the backward.          */
size_t wcmc_feature_mse_workspace_bytes(int B, int S, int C, int h, int w);
int wcmc_feature_mse_fwd(const float* p, int64_t psb, int64_t pss, int64_t psc, int64_t psh,
                         int64_t psw,
                         const float* ref, int64_t rsb, int64_t rsc, int64_t rsh, int64_t rsw,
                         const int64_t* idx_patch, const int64_t* idx_batch,
                         float* loss, void* workspace, size_t workspace_bytes,
                         int B, int S, int C, int h, int w, void* stream);
/* dp: contiguous (B,S,C,h,w); grad_scale: device pointer to the upstream scalar gradient. */
int wcmc_feature_mse_bwd(const float* p, int64_t psb, int64_t pss, int64_t psc, int64_t psh,
                         int64_t psw,
                         const int64_t* idx_patch, const int64_t* idx_batch,
                         const float* grad_scale, float* dp,
                         void* workspace, size_t workspace_bytes,
                         int B, int S, int C, int h, int w, void* stream);

/* GlobalRelativeSimilarityLoss (support/losses.py:116-211, `--manif_loss GRS`): same pairings and
 * displacements, loss = (logsumexp(alpha*[d_p, d_b, -d_p, -d_b, 0]) - log(1 + 4N)) / sqrt(alpha).
 * Same workspace (wcmc_feature_mse_workspace_bytes) and calling convention as FeatureMSE. */
int wcmc_grs_fwd(const float* p, int64_t psb, int64_t pss, int64_t psc, int64_t psh, int64_t psw,
                 const float* ref, int64_t rsb, int64_t rsc, int64_t rsh, int64_t rsw,
                 const int64_t* idx_patch, const int64_t* idx_batch, float alpha,
                 float* loss, void* workspace, size_t workspace_bytes,
                 int B, int S, int C, int h, int w, void* stream);
int wcmc_grs_bwd(const float* p, int64_t psb, int64_t pss, int64_t psc, int64_t psh, int64_t psw,
                 const int64_t* idx_patch, const int64_t* idx_batch,
                 const float* grad_scale, float* dp,
                 void* workspace, size_t workspace_bytes,
                 int B, int S, int C, int h, int w, void* stream);

/* A pseudo-random permutation of [0, n) as int64 indices, keyed by `seed` (6-round Feistel network, cycle-walked):
 * the `rng='device'` source of the FeatureMSE / GRS pairings instead of the sort behind torch.randperm.  The
 * reference draws its pairings with torch.randperm on the CPU generator (support/losses.py:35,50). */
int wcmc_random_permutation(int64_t* out, int64_t n, uint64_t seed, void* stream);
/* The same bijection keyed from DEVICE memory, for a launch captured into the step's hipGraph (a by-value seed is frozen at capture):
 * state = {seed, step counter} (two uint64), key = wcmc_permutation_key(seed, counter, slot) (host mirror of the device arithmetic:
 * wcmc_random_permutation_dev(out, n, state, slot) == wcmc_random_permutation(out, n, wcmc_permutation_key(state[0], state[1], slot))).
 * wcmc_step_counter_advance: state[1] += 1, once per step, ahead of the step's draws (losses.py:35,50 draws fresh pairings per call).
 * slot in [0, 8): the step's draws (diffuse patch / batch, specular patch / batch). */
uint64_t wcmc_permutation_key(uint64_t seed, uint64_t counter, int slot);
int wcmc_random_permutation_dev(int64_t* out, int64_t n, const uint64_t* state, int slot, void* stream);
int wcmc_step_counter_advance(uint64_t* state, void* stream);

/* ---------------------------------------------------------------- image losses of the sample-based interfaces
 * support/losses.py:267-320, built at train_lbmc.py:164-170 / train_sbmc.py (SMAPE: LBMC; Tonemapped*: SBMC).  Strided (N,C,H,W)
 * operands like wcmc_image_loss_fwd; one pass + a one-block finish in a fixed order (bitwise reproducible); workspace of
 * wcmc_image_loss_workspace_bytes().  T = Reinhard tone map of the clamped image (losses.py:234-242).
 *   kind 0  SMAPE                  mean |x - ref| / (eps + |x| + |ref|)   (the denominator carries no gradient, losses.py:279-282)
 *   kind 1  TonemappedMSE          0.5 * mean (T(x) - T(ref))^2
 *   kind 2  TonemappedRelativeMSE  0.5 * mean (T(x) - T(ref))^2 / (T(ref)^2 + eps)
 * bwd: dx (contiguous (N,C,H,W)) = *grad_loss * d loss / d x. */
int wcmc_image_loss2_fwd(int kind, const float* x, int64_t xsn, int64_t xsc, int64_t xsh, int64_t xsw, const float* ref,
                         int64_t rsn, int64_t rsc, int64_t rsh, int64_t rsw, float eps, float* loss, void* workspace,
                         size_t workspace_bytes, int N, int C, int H, int W, void* stream);
int wcmc_image_loss2_bwd(int kind, const float* x, int64_t xsn, int64_t xsc, int64_t xsh, int64_t xsw, const float* ref,
                         int64_t rsn, int64_t rsc, int64_t rsh, int64_t rsw, float eps, const float* grad_loss, float* dx,
                         int N, int C, int H, int W, void* stream);
/* torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) (support/interfaces.py:454-458, 826-833: 1000 for SBMC, 250 for LBMC)
 * over up to 96 gradient tensors in three launches: norm_and_coef[0] = the total 2-norm BEFORE clipping (what the reference prints),
 * norm_and_coef[1] = min(1, max_norm / (norm + 1e-6)); the gradients are scaled in place when the factor is below one. */
size_t wcmc_grad_norm_clip_workspace_bytes(int n_tensors, const int64_t* numel);
int wcmc_grad_norm_clip(int n_tensors, float* const* grads, const int64_t* numel, float max_norm, float* norm_and_coef,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- weight normalisation
 * sbmc.modules.ConvChain wraps every nn.Conv2d in torch.nn.utils.weight_norm unless its caller passes weight_norm=False;
 * support/networks.py:18-24 (PathNet's embedding / propagation / final chains) does not, sbmc.KPCN does.  Parameters per
 * layer: weight_g (Cout,1,1,1), weight_v (Cout,Cin,k,k);  weight = weight_g * weight_v / ||weight_v||, norm over (Cin,k,k)
 * per output channel (torch._weight_norm, dim 0).
 *
 * Both entries take ALL layers of a model in one launch (n_layers <= 32): tables of n_layers device pointers, rows[l] = Cout,
 * row_len[l] = Cin*k*k.  v / w / dw / dv are dense [rows][row_len] fp32 (16-byte aligned when row_len % 4 == 0);
 * g / norm / dg are [rows].
 *   fwd: w = v * (g / ||v||), norm = ||v||                                  (torch._weight_norm)
 *   bwd: dg = <dw, v> / norm;  dv = (g / norm) * (dw - v * <dw, v> / norm^2)   (torch._weight_norm_interface_backward) */
int wcmc_weight_norm_fwd(int n_layers, const float* const* v, const float* const* g, float* const* w,
                         float* const* norm, const int* rows, const int* row_len, void* stream);
int wcmc_weight_norm_bwd(int n_layers, const float* const* dw, const float* const* v, const float* const* g,
                         const float* const* norm, float* const* dv, float* const* dg, const int* rows,
                         const int* row_len, void* stream);

/* ---------------------------------------------------------------- clip + Adam
 * support/interfaces.py:260-261 (clip_grad_value_) + :269-271 (Adam.step,
 * train_kpcn.py:274-277: default betas/eps, no weight decay, no amsgrad) fused
 * over one flat parameter buffer.  grad is clamped IN PLACE (the reference leaves
 * clipped .grad behind), then m,v,param are updated.  step is the 1-based count. */
/* guard (optional device float): when *guard == 0 the launch is a no-op (the host raises the
 * reference's non-finite-loss error, interfaces.py:254-257, without having to sync before enqueuing). */
int wcmc_clip_adam(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float clip, double lr, double beta1, double beta2, double eps, int step,
                   float grad_scale, const float* guard, void* stream);
/* The same launch with its per-step scalars read from DEVICE memory, for a launch captured into the step's hipGraph (whose
 * by-value arguments are frozen at capture): hyper7 = the seven floats wcmc_clip_adam_hyper (host-side, no GPU call)
 * derives from (lr, betas, eps, step) exactly as wcmc_clip_adam does -- same arithmetic, bit-identical update.  The host
 * refreshes the buffer before every replay (`optim.param_groups[0]['lr']` may have changed: train_kpcn.py:279-296). */
void wcmc_clip_adam_hyper(double lr, double beta1, double beta2, double eps, int step, float* out7);
int wcmc_clip_adam_dev(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float clip,
                       float grad_scale, const float* hyper7, const float* guard, void* stream);
/* The head of the step's captured tail in one launch: losses = n (<= 16) device pointers to the 0-d loss scalars of loss_dict.
 * flags[i] = isfinite(loss_i) (the reference's check, support/interfaces.py:254-257), flags[n] = guard = all finite AND *ok;
 * *ok <- guard (a non-finite step keeps the steps enqueued behind it from updating until the host has raised the error and reset
 * *ok to 1); sums[i] += loss_i when the guard holds (the running sums of interfaces.py:263-267).  flags + n is what
 * wcmc_clip_adam_dev takes as its guard. */
int wcmc_step_guard(const float* const* losses, int n, float* ok, float* sums, float* flags, void* stream);
/* The same in two halves for several ranks (the reference's nn.DataParallel, train_kpcn.py:256-271, sees one process; here every rank
 * checks its own losses and all must agree): `local` writes flags[0..n) and this rank's 1 - (all finite AND *ok) into flag_slot -- the
 * float behind the first gradient bucket, summed over the ranks by the bucket's all-reduce; `global` reads the summed slot: guard =
 * (slot == 0) -> flags[n], *ok, and sums[i] += loss_i under the guard. */
int wcmc_step_guard_local(const float* const* losses, int n, const float* ok, float* flags, float* flag_slot, void* stream);
int wcmc_step_guard_global(const float* const* losses, int n, const float* flag_slot, float* ok, float* sums, float* flags, void* stream);

/* ---------------------------------------------------------------- per-image preprocessing (data step before the path)
 * support/datasets.py: DenoiseDataset._preprocess_llpm :302-361, ._preprocess_kpcn :487-582,
 * ._gradients :286-300; raw channel map :223-267 (C >= 38 + 11*(max_depth+1); the reference's MAX_DEPTH is 5,
 * C = 104).  Dense, contiguous fp32 device buffers in the reference's numpy layouts:
 *   raw (h, w, s, C);  llpm out (h, w, s, 7 + 5*(max_depth+1)) = 37;  kpcn out (h, w, 44);
 *   gradients: buf (h, w, c) -> out (h, w, 2c) = [d/dx (c), d/dy (c)], zero first column / row. */
int wcmc_preprocess_llpm(const float* raw, int64_t nsamples /* h*w*s */, int C, int max_depth, float* out,
                         void* stream);
size_t wcmc_preprocess_kpcn_workspace_bytes(int h, int w);
int wcmc_preprocess_kpcn(const float* raw, int h, int w, int s, int C, int max_depth, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);
int wcmc_gradients(const float* buf, int h, int w, int c, float* out, void* stream);
/* wcmc_preprocess_kpcn in row bands (support/staging.py streams a frame that never lies whole on the device): `out` (h, w, 44) and the
 * workspace (wcmc_preprocess_kpcn_workspace_bytes(h, w): [mean depth, depth variance] per pixel, then the image maximum of the mean
 * depth) belong to the whole frame.  _begin zeroes the maximum slot; _rows runs pass 1 (the per-pixel statistics; the maximum by an
 * atomic on that slot) on frame rows [row0, row0 + rows) from raw_band (rows, w, s, C), choosing among the three statistics kernels
 * by the band's own alignment; _end runs pass 2 (depth normalisation, backward differences) over the frame once every row has been
 * through _rows.  Any partition of [0, h) gives wcmc_preprocess_kpcn's result bit for bit; wcmc_preprocess_kpcn is
 * _begin + _rows(0, h) + _end.  All on one stream, or ordered by the caller.  Null pointers and rows outside the frame (row0 < 0,
 * rows < 1, row0 + rows > h) are WCMC_ERR_BAD_ARG, a short workspace WCMC_ERR_WORKSPACE, before any launch. */
int wcmc_preprocess_kpcn_begin(void* workspace, size_t workspace_bytes, int h, int w, void* stream);
int wcmc_preprocess_kpcn_rows(const float* raw_band, int h, int w, int row0, int rows, int s, int C, int max_depth, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);
int wcmc_preprocess_kpcn_end(float* out, void* workspace, size_t workspace_bytes, int h, int w, int s, void* stream);

/* Batch assembly for the KPCN base model (DenoiseDataset.__getitem__ + _sample_patches + _transpose,
 * support/datasets.py:795-840,1026-1146): crops B windows of P x P pixels at origins[b] = (row, column) out of the
 * per-image buffers kpcn (H, W, 44), llpm (H, W, S, 37; null without --use_llpm_buf) and gt (H, W, 9) and writes the
 * batch dictionary's tensors channel-first and contiguous: diffuse_in / specular_in (B, 34 [+1], P, P), the two
 * 3-channel radiance buffers, albedo + 0.00316, paths (B, S, 36, P, P), and the three targets
 * (total, diffuse / (albedo + 0.00316), log(1 + total - diffuse)).  origins: device int32 [B][2], windows in bounds.
 * S_total, s (sample counts 2..spp from one staged frame, MSDenoiseDataset :1149-1171): llpm holds S_total samples per pixel and the
 *   batch takes the first s, 1 <= s <= S_total -- what `llpm[:, :, :s]` feeds __getitem__ (:1045-1118).  paths has s samples; the
 *   path-weight channel of the two inputs is the mean over the first s, summed in sample order (:1099-1107).  Neither is read
 *   without llpm (0, 0 will do).
 * transforms (dihedral patch augmentation): null, or B device ints, one code per patch.  Code t in 0..7 is
 *   T_t(a) = rot90(fliplr(a) if t & 4 else a, k = t & 3) (numpy's rot90 and fliplr on the row and column axes); 0 is the identity,
 *   and the eight codes are the dihedral group of the square -- what the reference's _random_rot(_random_flip(.))
 *   (support/datasets.py:718-758) reaches, every element by two of its sixteen draws.  origins keep their meaning: they name a
 *   P x P window of the source frame, and batch entry b is T_t[b] of that window, as if the whole frame had been transformed
 *   before preprocessing:
 *     - every per-pixel channel (values and variances of the five KPCN groups, depth and its variance, path weight, paths, the three
 *       buffers, albedo, the three targets) is that of the source pixel;
 *     - the x- and y-differences of the diffuse, specular, normal and albedo values and of the depth are taken again from the stored
 *       value channels: dx_out(y, x) = val(src(y, x)) - val(src(y, x - 1)), dy_out(y, x) = val(src(y, x)) - val(src(y - 1, x)), one
 *       fp32 subtraction of two stored floats, where src is the same affine map (at x = 0 / y = 0: one step outside the window), and
 *       exactly 0.f where that neighbour lies outside the frame (the transformed frame's first column / row, as _gradients);
 *     - direction-valued channels (normals) are copied, not re-expressed: the reference's functions do the same.
 *   A null table and a table of zeros give the same batch bit for bit (the null table launches the kernel without the map).  The
 *   codes are data: the host checks them (ops.check_patch_transforms) and the kernels mask them to t & 7, so a bad table cannot read
 *   outside the buffers.
 * WCMC_ERR_BAD_ARG before any launch: a null pointer other than llpm, transforms and paths; a non-positive size; P > H or P > W;
 *   with llpm, s outside 1..S_total or no paths. */
int wcmc_assemble_kpcn_patches(const float* kpcn, const float* llpm, const float* gt, const int* origins, const int* transforms,
                               int B, int H, int W, int S_total, int s, int P, float* diffuse_in, float* specular_in,
                               float* diffuse_buffer, float* specular_buffer, float* albedo, float* paths,
                               float* target_diffuse, float* target_specular, float* target_total, void* stream);

/* ---------------------------------------------------------------- patch-sampling probability maps
 * support/datasets.py: gradient_importance_map :17-36 and the `_prob_imp` block of DenoiseDataset._offline_preprocess
 * :697-715 (with LinearToSrgb(ToneMap(., 1.5)), support/utils.py:44-57); the NaN / Inf rule of :623-624.  Dense,
 * contiguous fp32 device buffers in the reference's numpy layouts.  No atomics: every result is bitwise reproducible.
 *
 * wcmc_reflect_index: the source index of position i (any int) of a line of n >= 1 entries under scipy's boundary mode
 *   'reflect' (d c b a | a b c d | d c b a, period 2n; numpy.pad's 'symmetric') -- the map the Gaussian passes use.  Host only.
 * wcmc_importance_map: img (H, W, C), C = 1 or 3 -> out (H, W):
 *   per channel scipy.ndimage.gaussian_filter(x, 31) (249 taps per axis, axis 0 first, mode 'reflect', fp64 accumulation in
 *   scipy's order, rounded to fp32 between the passes), sobel along both axes with mode 'nearest', the root of the sum of squares
 *   over the channels, then (v - min) / (max - min + 1e-5).
 * wcmc_sampling_prob: raw (H, W, S, C >= 38 + 11*(max_depth+1)), gt (H, W, 9), both sanitised -> out (H - patch, W - patch):
 *   prob = 0.3 * importance_map(lum) + 0.2 * importance_map(normal) + 0.5 * mat, cropped by patch/2 at the top / left and
 *   patch - patch/2 at the bottom / right, divided by (sum + 1e-5).  lum: luminance (0.2126, 0.7152, 0.0722) of
 *   LinearToSrgb(ToneMap(gt[..., :3], 1.5)); normal: sample mean of raw channels 17..19 (idx_g['normal'], :232-248; the s-buffer's
 *   columns 20:23 of _preprocess_sbmc, :363-485) * 0.5 + 0.5; mat = (diffuse + 4 glossy + 2 specular) / 7 from the sample means of
 *   bits 2, 3, 4 of raw channel 24 + 6*(max_depth+1) (idx_sbmc['bounce_types'] :249-255, bounce 0: the p-buffer's columns 48, 54, 60).
 *   H and W must exceed patch.
 * wcmc_sanitize: x[i] <- 1e38 where x[i] is NaN, +-Inf or >= 1e38 (:623-624), in place; n = 0 is no work
 *   and no error (x may then be null: an empty tensor has no storage). */
int wcmc_reflect_index(int i, int n);
size_t wcmc_importance_map_workspace_bytes(int H, int W, int C);
int wcmc_importance_map(const float* img, int H, int W, int C, float* out, void* workspace, size_t workspace_bytes,
                        void* stream);
size_t wcmc_sampling_prob_workspace_bytes(int H, int W, int patch);
int wcmc_sampling_prob(const float* raw, const float* gt, int H, int W, int S, int C, int max_depth, int patch, float* out,
                       void* workspace, size_t workspace_bytes, void* stream);
int wcmc_sanitize(float* x, int64_t n, void* stream);

/* ---------------------------------------------------------------- the data step of the sample-based denoisers (csrc/sbmc_data.hip)
 * wcmc_preprocess_sbmc: DenoiseDataset._preprocess_sbmc (support/datasets.py:363-485; channel order and arithmetic :394-452).
 *   raw (h, w, s, C >= 38 + 11*(max_depth+1)), sanitised -> out_s (h, w, s, 27) and out_p (h, w, s, 11*(max_depth+1)) = 66:
 *   out_s = [max(total, 0) (3), log(1 + max(total, 0)) / 10 (3), log(1 + max(max(total, 0) - max(diffuse, 0), 0)) / 10 (3),
 *            subpixel = raw 0:2, raw 8:24 verbatim (albedo / normal at first and at first non-specular bounce, depths, visibility, hasHit)]
 *   out_p = [log(max(prob, 0) + 1e-5) / 30 (4d), clip(light_directions, -1, 1) (2d), then the five tag planes of bits 0..4 of the
 *            bounce type, plane-major: is_reflection x d, is_transmission x d, is_diffuse x d, is_glossy x d, is_specular x d]
 *   The bounce code is the float truncated toward zero, as astype(np.int16) does for a value that int16 holds; a code outside
 *   [-32768, 32767] -- the 1e38 that sanitising leaves -- gives all five flags 0 (numpy's result for such a cast is whatever the
 *   host's conversion instruction leaves: undefined in C).
 *   tiled: -1 picks the form (LDS-staged for 16-byte aligned records, else one thread per element), 0 / 1 force the generic / the
 *   tiled form (1 is an error where the tiled form does not apply); the two forms are bit-identical.
 * wcmc_assemble_sample_patches: the sample-based batch of DenoiseDataset.__getitem__ (:1045-1073, 1086-1118) after _transpose
 *   (:760-791), for B windows of P x P pixels at origins[b] = (row, column) (device int32 [B][2], windows in bounds) of one image:
 *   sbmc_s (H, W, S_total, 27), sbmc_p (H, W, S_total, 66; may be null without use_sbmc_buf), llpm (H, W, S_total, 37) or null,
 *   gt (H, W, 9); the batch takes the first s samples of each, 1 <= s <= S_total (the `[:, :, :s]` slices of MSDenoiseDataset) ->
 *     radiance (B, s, 3, P, P) = sbmc_s 0:3
 *     features (B, s, F, P, P) = [sbmc_s 3:27 if use_g_buf else sbmc_s 3:6] ++ [sbmc_p if use_sbmc_buf] ++ [llpm 0:1 if llpm]
 *                                F = 24 | 3, + 66, + 1
 *     paths    (B, s, 36, P, P) = llpm 1:37 (only with llpm)
 *     target_image (B, 3, P, P) = gt 0:3
 *   transforms: null, or one dihedral code per patch as wcmc_assemble_kpcn_patches takes them; every channel is per sample, so every
 *   one is a copy of the source pixel's (subpixel and light directions included: not re-expressed), and a null table and a table of
 *   zeros give the same batch.  One launch; copies only (bit-exact).
 *   WCMC_ERR_BAD_ARG before any launch: a null pointer other than sbmc_p, llpm, transforms and paths; a non-positive size; P > H or
 *   P > W; s outside 1..S_total; llpm without paths; use_sbmc_buf without sbmc_p. */
int wcmc_preprocess_sbmc(const float* raw, int64_t nsamples /* h*w*s */, int C, int max_depth, float* out_s, float* out_p,
                         int tiled, void* stream);
int wcmc_assemble_sample_patches(const float* sbmc_s, const float* sbmc_p, const float* llpm, const float* gt,
                                 const int* origins, const int* transforms, int B, int H, int W, int S_total, int s, int P,
                                 int use_g_buf, int use_sbmc_buf, float* radiance, float* features, float* paths,
                                 float* target_image, void* stream);

/* ---------------------------------------------------------------- sample counts 2..spp from one staged frame (csrc/multi_spp.hip)
 * The reference trains over MSDenoiseDataset (support/datasets.py:1149-1171): one DenoiseDataset per count s = 2..spp, each reading
 * the first s samples of every frame (:618, :1053-1054, :1091).  Here every count comes out of ONE staged frame.
 * wcmc_preprocess_kpcn_prefix: replaces `_preprocess_kpcn(sample[:, :, :s])` (:487-582) for s = s_lo..s_hi, 1 <= s_lo <= s_hi <=
 *   S <= 64.  raw (h, w, S, C) as for wcmc_preprocess_kpcn -> out (s_hi - s_lo + 1, h, w, 44): slab s - s_lo is what
 *   wcmc_preprocess_kpcn returns for the contiguous first s samples -- mean and population variance over the prefix (:505-543), the
 *   divisions by that s, the depth normalised by that prefix's own image maximum, the gradients of that slab.  Sums run in sample
 *   order (numpy's; wcmc_preprocess_kpcn's for a count that is no power of two), so a power-of-two count may differ from
 *   wcmc_preprocess_kpcn's shuffle tree in the last place.  raw is read from memory once.
 * The batches of a count come from the two patch assemblers above: their S_total / s pair takes the first s of the staged samples. */
size_t wcmc_preprocess_kpcn_prefix_workspace_bytes(int h, int w, int n_counts);
int wcmc_preprocess_kpcn_prefix(const float* raw, int h, int w, int S, int C, int max_depth, int s_lo, int s_hi, float* out,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- full-frame evaluation
 * The image metrics of the reference's evaluation script (test_models.py:234-251, support/metrics.py) for one
 * (scene, spp) cell.  out / ipt / tgt: fp32 (H, W, 3) images, element (y, x, c) at p[y*sh + x*sw + c*sc] (any int64
 * strides: the channel-first frame is passed as a view); has_hit: the same form, or null.  When given, out is replaced
 * by ipt wherever has_hit == 0 (test_models.py:231-232) on load.
 * result: 40 fp64 device values [cmp][t][k] -- cmp 0 = out vs tgt, 1 = ipt vs tgt; tone map t in (linear, _tonemap,
 * tonemap gamma 1/2.2, tonemap gamma 1/2.8), each image on its own luminance; metric k in (RelMSE, RelL1, DSSIM, L1, MSE):
 *   MSE = mean (a-r)^2, L1 = mean |a-r|, RelL1 = mean |a-r| / (|r| + eps),
 *   RelMSE = mean over the non-NaN entries of (a-r)^2 / (r^2 + eps) (NaN when all are NaN),
 *   DSSIM = 1 - SSIM: 7x7 uniform window, K1 0.01, K2 0.03, sample covariance (49/48), data_range 2, fp64, the SSIM map
 *   averaged over the interior cropped by 3 pixels and over the channels (skimage.metrics.structural_similarity with
 *   multichannel=True before 0.21, as specified in DESIGN.md).
 * H, W >= 7.  Two launches (blocks' partial sums, then a one-block finish in a fixed order): bitwise reproducible. */
size_t wcmc_image_eval_workspace_bytes(int H, int W);
int wcmc_image_eval(const float* out, int64_t osh, int64_t osw, int64_t osc, const float* ipt, int64_t ish, int64_t isw,
                    int64_t isc, const float* tgt, int64_t tsh, int64_t tsw, int64_t tsc, const float* has_hit, int64_t hsh,
                    int64_t hsw, int64_t hsc, int H, int W, double eps, double* result, void* workspace,
                    size_t workspace_bytes, void* stream);
/* The tile loop of test_models.inference (test_models.py:75-89) for one batch of B tiles: for every tile b with
 * coords[b] = (i_start, j_start, i_end, j_end, i, j) (device int32 (B, 6)), copy its owned window
 * [i_start:i_end, j_start:j_end] of
 *   the radiance: rad (B, 3, ho, wo) with strides (rsb, rsc, rsh, rsw), 'replicate'-padded back to P x P
 *     (F.pad(out, (pw//2, pw-pw//2, ph//2, ph-ph//2)), test_models.py:66-70) -> out_rad (3, H, W) contiguous;
 *   up to two P-buffers: pbuf (B, S, C, P, P) contiguous -> out_pbuf (S, C, H, W) contiguous (null: none).
 * ho == wo == P (no padding) or both smaller than P.  Windows outside the frame or the tile are skipped. */
int wcmc_stitch_tiles(const float* rad, int64_t rsb, int64_t rsc, int64_t rsh, int64_t rsw, int ho, int wo,
                      const float* pbuf_a, const float* pbuf_b, int S, int C, int P, const int* coords, int B, int H, int W,
                      float* out_rad, float* out_pbuf_a, float* out_pbuf_b, void* stream);

/* ---------------------------------------------------------------- denoising a render of any size (csrc/frame_tiles.hip)
 * Inference on a frame with no ground truth and no divisibility condition (wcmc_amd.denoise, DESIGN.md "Denoising a render").
 * The frame is taken as extended by `pad` pixels on every side by mirror reflection with the edge repeated -- numpy.pad's
 * 'symmetric', the map of the reflect-index entry point above -- and tiled at stride P - 2*pad; every tile owns pixels of its
 * [pad, P - pad) interior only, so nothing but what the network computed from real or mirrored data reaches the image.
 * assemble_kpcn_tiles: the batch of the KPCN base model without targets, for B tiles of P x P pixels at origins[b] = (row, column)
 *   in FRAME coordinates, -pad <= origin <= dim + pad - P (device int32 [B][2]; the caller checks them on the host), out of
 *   kpcn (H, W, 44) and llpm (H, W, S, 37; null without --use_llpm_buf): diffuse_in / specular_in (B, 34 [+1], P, P), the two
 *   3-channel radiance buffers, albedo + 0.00316 and paths (B, S, 36, P, P), laid out as the patch-assembly entry point lays them
 *   out.  The extended frame is never stored: a position outside reads its mirror image's record, and each of the 26 backward
 *   differences is taken again as value[m(r), m(c)] - value[m(r), m(c - 1)] (rows likewise; 0 at frame position -pad) wherever its two
 *   operands are not in-frame neighbours.  Bit for bit what preprocessing numpy.pad(raw, pad, 'symmetric') and assembling patches at
 *   origins + pad give.  0 <= pad < min(H, W), P > 2*pad, P <= min(H, W) + 2*pad.
 *   t (dihedral self-ensemble): 0, or a code 1..7 for the tiles of the frame AS IF the raw frame had been
 *   transformed by T_t before preprocessing.  T_t(a) = rot90(fliplr(a) if t & 4 else a, k = t & 3) on the row and column axes, as
 *   the patch assemblers' codes; the transformed frame is H x W for even t and W x H for odd t, and its pixel (y, x) is source pixel
 *   (sy, sx) = (y, x), (x, W-1-y), (H-1-y, W-1-x), (H-1-x, y) for k = 0..3, then sx = W-1-sx if t & 4.  One code per launch; H and W
 *   are always the SOURCE buffers' sizes; origins are in the TRANSFORMED frame's coordinates, and the pad and P conditions hold
 *   against its sizes.  The mirror is that of the transformed frame, then the map above: copied channels are the source record's
 *   (direction-valued ones are not re-expressed); each of the 26 differences is value[src(p)] - value[src(p - e)], e one step along
 *   the transformed frame's x / y, one fp32 subtraction (also of a record with itself), and exactly 0 at the transformed extended
 *   frame's first column / row.  Bit for bit t = 0 on the buffers preprocessed from the host-transformed raw frame.  t outside 0..7
 *   is refused on the host and masked in the kernels; every mirrored and mapped index is clamped before use.
 * finish_frame: one pass over the frame after stitching.  out_rad (3, H, W), kpcn (H, W, 44), llpm (H, W, S, 37) ->
 *   ipt (H, W, 3) = kpcn[0:3] * (kpcn[34:37] + 0.00316) + exp(kpcn[10:13]) - 1   (datasets.py:1234)
 *   has_hit (H, W) = 1.0 where (sum over the S samples, in sample order, of llpm[..., 25]) / S != 0, else 0.0   (:1407-1414)
 *   out (H, W, 3) = has_hit ? out_rad : ipt   (test_models.py:231-232)
 *   preview_out / preview_ipt (H, W, 3) uint8, each optional (null: not written): round(255 * clip(tonemap(.), 0, 1)) of out / ipt
 *   with tonemap of test_models.py:24-34 at gamma 1/2.2 on the image's own luminance, rounding half to even; NaN gives 0. */
int wcmc_assemble_kpcn_tiles(const float* kpcn, const float* llpm, const int* origins, int B, int H, int W, int S, int P, int pad,
                             int t, float* diffuse_in, float* specular_in, float* diffuse_buffer, float* specular_buffer,
                             float* albedo, float* paths, void* stream);
int wcmc_finish_frame(const float* out_rad, const float* kpcn, const float* llpm, int H, int W, int S, float* out, float* ipt,
                      float* has_hit, unsigned char* preview_out, unsigned char* preview_ipt, void* stream);

/* ---------------------------------------------------------------- the same for the sample-based models (SBMC / LBMC interfaces)
 * assemble_sample_tiles (csrc/sbmc_data.hip): the sample-based batch without gt and without target_image, for B tiles of P x P
 *   pixels at origins[b] = (row, column) in FRAME coordinates, -pad <= origin <= dim + pad - P (device int32 [B][2]; the caller
 *   checks them on the host, the kernel clamps the mirrored index), out of sbmc_s (H, W, S, 27), sbmc_p (H, W, S, 66; may be null
 *   without use_sbmc_buf) and llpm (H, W, S, 37) or null: radiance (B, S, 3, P, P), features (B, S, F, P, P) and, with llpm, paths
 *   (B, S, 36, P, P), channel for channel as the sample-patch entry point above lays them out (F = 24 | 3, + 66, + 1).  Every buffer
 *   is per sample, so a position outside the frame is a copy of its mirror image's record: bit for bit what preprocessing
 *   numpy.pad(raw, pad, 'symmetric') and assembling sample patches at origins + pad give.  One launch; copies only.
 *   S > 0, 0 <= pad < min(H, W), P > 2*pad, P <= min(H, W) + 2*pad.  t: as assemble_kpcn_tiles takes it -- the frame is read through
 *   the mirror of the transformed frame and then the same map, the conditions hold against the transformed sizes; copies only.
 * finish_sample_frame (csrc/frame_tiles.hip): finish_frame with the noisy input of the sample-based models,
 *   ipt (H, W, 3) = (sum over the S samples, in sample order, of sbmc_s[..., 0:3]) / S   (datasets.py:1248)
 *   has_hit, out and the two optional previews as finish_frame. */
int wcmc_assemble_sample_tiles(const float* sbmc_s, const float* sbmc_p, const float* llpm, const int* origins, int B, int H, int W,
                               int S, int P, int pad, int t, int use_g_buf, int use_sbmc_buf, float* radiance, float* features,
                               float* paths, void* stream);
int wcmc_finish_sample_frame(const float* out_rad, const float* sbmc_s, const float* llpm, int H, int W, int S, float* out,
                             float* ipt, float* has_hit, unsigned char* preview_out, unsigned char* preview_ipt, void* stream);

/* ---------------------------------------------------------------- dihedral self-ensemble of a frame
 * The way back of a pass whose tiles were assembled under a code t (assemble_kpcn_tiles / assemble_sample_tiles above: the code, the
 * transformed frame's sizes and the source map (sy, sx) of its pixel (y, x) are defined there).  coords are in the TRANSFORMED
 * frame's coordinates; t outside 0..7 is refused on the host and masked in the kernel.
 * stitch_tiles_aug: for every tile b with coords[b] = (i_start, j_start, i_end, j_end, i, j) of the transformed frame's table (device
 *   int32 (B, 6)) and every pixel (y, x) of its owned window, v = rad (B, 3, ho, wo) 'replicate'-padded back to P x P as stitch_tiles
 *   does it, and out_rad[:, sy, sx] = v (accumulate = 0) or out_rad[:, sy, sx] + v (accumulate = 1); out_rad (3, H, W) contiguous, in
 *   SOURCE orientation.  The owned windows partition the frame, so a launch set touches every element once: no atomics, and passes
 *   that follow one another on one stream give a bit-defined sum.  No P-buffers (those are the identity pass's). */
int wcmc_stitch_tiles_aug(const float* rad, int64_t rsb, int64_t rsc, int64_t rsh, int64_t rsw, int ho, int wo, int P,
                          const int* coords, int B, int t, int H, int W, int accumulate, float* out_rad, void* stream);

/* The feathered stitch: radiance blended across the seams of the owned windows.
 * stitch_tiles_blend: for every tile b of the batch, in table order, and every pixel (y, x) of [i_start - F, i_end + F) x
 *   [j_start - F, j_end + F) clipped to the frame transformed by code t (t = 0: the frame itself), acc[:, sy, sx] += w * v and
 *   wsum[sy, sx] += w; v is read as stitch_tiles_aug reads it, (sy, sx) is the pixel's source, and w = u_rows(y) * u_cols(x) with
 *   u(x) = L(x) * R(x), L = 1 where i_start == 0, else clamp((x - i_start + F + 0.5) / (2F), 0, 1), R = 1 where i_end is the axis'
 *   length, else clamp((i_end + F - x - 0.5) / (2F), 0, 1); F = 0: w = 1 on the owned window.  acc (3, H, W) and wsum (H, W) are
 *   contiguous fp32 in SOURCE orientation and zero before the first batch of a pass.  One thread owns a destination pixel and adds the
 *   batch's tiles in order: no atomics, and the sums do not depend on how the table is cut into batches.  pad: the pad of the table,
 *   or negative where the caller vouches for it; with a pad, 2F <= P - 2 pad (at most three tiles meet on an axis) and
 *   F <= pad - max((P - ho + 1) / 2, (P - wo + 1) / 2) (no replicated pixel carries weight) are required.
 * blend_finish: out_rad (3, H, W) = acc / wsum (accumulate = 0) or out_rad + acc / wsum (accumulate = 1). */
int wcmc_stitch_tiles_blend(const float* rad, int64_t rsb, int64_t rsc, int64_t rsh, int64_t rsw, int ho, int wo, int P, int pad,
                            const int* coords, int B, int t, int H, int W, int F, float* acc, float* wsum, void* stream);
int wcmc_blend_finish(const float* acc, const float* wsum, int H, int W, int accumulate, float* out_rad, void* stream);

/* ---------------------------------------------------------------- filtering a frame by its P-buffer (csrc/pbuffer_filter.hip)
 * Non-local means whose patch distance is taken between the per-pixel statistics of the path embedding (Ray Histogram Fusion with
 * the learned manifold in place of the colour histograms).  The build's own specification: DESIGN.md section 19.
 *   image (H,W,Cr), element (y,x,c) at image[y*ish + x*isw + c*isc], Cr <= 4; p_buffer (S,C,H,W), element (s,c,y,x) at
 *   p_buffer[s*pss + c*psc + y*psh + x*psw], S >= 1, 1 <= C <= 32; mask (H,W) contiguous or NULL, mask_bytes = 1 (uint8 / bool)
 *   or 4 (fp32), a pixel counts where its element is not zero.
 *     mu[c,p] = (1/S) sum_s P[s,c,p],   v[c,p] = (1/S^2) sum_s (P[s,c,p] - mu[c,p])^2            (sample order, fp32)
 *     delta(p,q) = (1/C) sum_c (mu[c,p] - mu[c,q])^2 / (eps + v[c,p] + v[c,q])
 *     D(p,q) = mean of delta(p+o, q+o) over |oy|,|ox| <= f with p+o and q+o inside the image
 *     w(p,q) = exp(-D(p,q) / bandwidth^2), q = p + (dy,dx), |dy|,|dx| <= R, q inside the image and mask[q] != 0; else 0
 *     wsum[p] = sum_q w(p,q);  out[p,:] = sum_q w(p,q) image[q,:] / wsum[p]   (q in tap order, dy major: bitwise reproducible)
 *     where mask[p] == 0: out[p,:] = image[p,:], wsum[p] = 0.
 *   out (H,W,Cr) and wsum (H,W) are contiguous.  0 <= R <= 10, 0 <= f <= 3, bandwidth > 0, eps > 0.  A non-finite P-buffer
 *   value poisons the pixels whose windows and patches read it, and no others.
 *   workspace: wcmc_pbuffer_filter_workspace_bytes(S, C, H, W) bytes (0 for an unsupported shape); it receives {mu, v}.
 *   passes: 1 the statistics launch alone, 2 the filter launch alone (the workspace holds the statistics), 3 both. */
size_t wcmc_pbuffer_filter_workspace_bytes(int S, int C, int H, int W);
int wcmc_pbuffer_filter(const float* image, int64_t ish, int64_t isw, int64_t isc,
                        const float* p_buffer, int64_t pss, int64_t psc, int64_t psh, int64_t psw,
                        const void* mask, int mask_bytes, float* out, float* wsum, void* workspace, size_t workspace_bytes,
                        int H, int W, int S, int C, int Cr, int R, int f, float bandwidth, float eps, int passes, void* stream);

/* ---------------------------------------------------------------- structural-similarity training loss (csrc/dssim_loss.hip)
 * loss = 1 - mean SSIM over every 7x7 window of every plane of a strided fp32 (N,C,H,W) pair; the build's own specification:
 * DESIGN.md section 23 (the SSIM of section 10 / wcmc_image_eval: uniform window at valid positions, K1 0.01, K2 0.03, sample
 * covariance 49/48, C1 = (K1 R)^2, C2 = (K2 R)^2 with R = data_range > 0).  Element (n,c,y,x) of x is x[n*xsn + c*xsc + y*xsh + x*xsw].
 *   tonemap 0  none
 *   tonemap 1  reinhard: T(v) = max(v, 0) / (1 + max(v, 0)) on both images (metrics._tonemap); T'(v) = 1 / (1 + v)^2 for v >= 0, else 0
 * With tonemap 1, data_range 2, N = 1, C = 3 the loss is the `_tonemap` DSSIM of wcmc_image_eval.  H, W >= 7, N * C <= 65535.
 * Every moment, the SSIM map and the gradient's box sums are fp64; partial sums are added in a fixed order by a one-block finish (no
 * atomics: loss and dx are bitwise reproducible).  Non-finite inputs are not filtered: a NaN pixel gives a NaN loss.
 *   fwd: *loss (fp32, device) <- the loss.  workspace: wcmc_dssim_loss_workspace_bytes(N, C, H, W) bytes (0 for a refused shape).
 *   bwd: dx (contiguous (N,C,H,W)) = *grad_loss * d loss / d x; ref carries no gradient.  The backward recomputes the per-window
 *        coefficients from the inputs: nothing but x and ref passes from fwd to bwd. */
size_t wcmc_dssim_loss_workspace_bytes(int N, int C, int H, int W);
int wcmc_dssim_loss_fwd(const float* x, int64_t xsn, int64_t xsc, int64_t xsh, int64_t xsw, const float* ref, int64_t rsn,
                        int64_t rsc, int64_t rsh, int64_t rsw, int tonemap, double data_range, float* loss, void* workspace,
                        size_t workspace_bytes, int N, int C, int H, int W, void* stream);
int wcmc_dssim_loss_bwd(const float* x, int64_t xsn, int64_t xsc, int64_t xsh, int64_t xsw, const float* ref, int64_t rsn,
                        int64_t rsc, int64_t rsh, int64_t rsw, int tonemap, double data_range, const float* grad_loss, float* dx,
                        int N, int C, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WCMC_HIP_H */
