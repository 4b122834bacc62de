"""Autograd wrappers over the C ABI of ``libwcmc_hip.so``.

Tensors between ops are *NHWC views*: logically (N,C,H,W) torch tensors whose
channel stride is 1 and whose pixel stride is padded to a multiple of 4 floats
(``nhwc_empty``).  Slices / crops / concat targets stay views; every kernel takes
explicit strides.  PyTorch here is device memory, streams and autograd plumbing
only -- all arithmetic of the hot path runs in the HIP library.  Nothing in this
package has a CPU path: a tensor that is not on ``cuda`` raises.

One module per concern, named after the translation unit of ``csrc/`` it wraps where there is one; every name of every module
is re-exported here, so ``wcmc_amd.ops.<name>`` is the spelling for callers.  This file launches nothing.  It holds the names
that code OUTSIDE the package assigns (``ops.USE_SIDE_STREAM = False``, ``monkeypatch.setattr(ops, "FUSE_EMBED", ...)``): the
modules read them here, as ``_sw.<NAME>``, at the moment a function runs -- never ``from . import <NAME>``, which would leave a
module with a copy of its own that such an assignment does not reach (tests/test_cpu_host.py holds that).
"""
import os

import torch  # noqa: F401      (``ops.torch``, ``ops.weakref``, ``ops.check``, ``ops.lib``: names the one-file module had, kept)
import weakref  # noqa: F401

from .._lib import check, lib  # noqa: F401

# Arithmetic of the conv GEMMs (all HIP paths; WCMC_PRECISION):
#   "bf16x321h" (default) "bf16x321" with ONE fp16 MFMA per product (fp16(x) x fp16(W): 11 bits each, the last hidden activation
#                         converted once by wcmc_split_to_f16) in the forward of a chain's un-gated OUTPUT layer where the library
#                         has the instance (5x5, linear output: the KPCN chains' 100 -> 441 logits, 30 % of the KPCN forward's
#                         FLOPs): +2.8 % step throughput, denoised patches within 1.6e-5 of the oracle's (north star: 1e-3).  Opt-in
#                         in round 4 because its worst gradient tensor sat at 1.41e-3 against 1.20e-3 for "bf16x321" and a bar of
#                         2e-3; round 5 measured what that bar was worth: the same comparison moves from 1.20e-3 to 1.96e-3 when the
#                         WEIGHTS are re-drawn, in "bf16x321" as in exact fp32 (profiles/r05_grad_bar_calibration.txt), and
#                         "bf16x321h" sits at 2.00e-3 on that draw -- the draw decides, not this rung.  Its 200-step training
#                         trajectory lies inside the spread of fp32 runs that start one ulp apart (profiles/r05_arith_trajectories.txt:
#                         validation 0.45 % from fp32 against a spread of 0.69 %, last-50 rmse 0.04 % against 0.56 %)
#   "bf16x321o" (opt-in)  "bf16x321" with ONE MFMA per product (x_hi x W_hi) in the forward of a chain's un-gated OUTPUT layer
#                         where the library has the instance (5x5, linear output: the KPCN chains' 100 -> 441 logits, 30 % of the
#                         KPCN forward's FLOPs).  The forward precision ladder (profiles/r04_forward_ladder.txt) shows why only
#                         there: rounding a HIDDEN layer's operands below 16 bits flips ReLU gates and moves the parameter
#                         gradients past their parity bars (no rung holds), an output layer has no gate behind it -- measured
#                         on the benchmarked step: denoised patches 1.1e-4, loss scalars 8e-6, gradients 1.61e-3; its trajectory's
#                         validation error ends 1.3 % from fp32, outside the fp32 spread: opt-in
#   "bf16x321"            split-bf16 operands (hi + lo planes, fp32 accumulate; conv_bf16x3.hip) with the number of bf16 MFMAs
#                         per product chosen per GEMM role by the measured precision ladder (profiles/r03_precision_ladder.txt):
#                         forward 3 (hi*hi + hi*lo + lo*hi), data gradient 2 (dy_hi x (W_hi + W_lo)), weight gradient 1
#                         (dy_hi x x_hi) -- rounding dy and x to bf16 is independent from pixel to pixel and averages out over
#                         the pixel sums, a rounded W would not; outputs and losses are those of "bf16x3" bit for bit (the
#                         default of rounds 3-4)
#   "bf16x3"              three MFMAs per product in every role (rounds 1-2)
#   "fp32"                exact fp32 MFMA (conv.hip)
MODES = ("bf16x321h", "bf16x321", "bf16x321o", "bf16x3", "fp32")


# ---------------------------------------------------------------------------------------------------------------- switches
# Every name below is assigned from outside (bench.py, graph.py, tests, scripts/) and read by the modules as ``_sw.<NAME>``.
# The environment variables are read once, here.
PRECISION = os.environ.get("WCMC_PRECISION", MODES[0])         # one of MODES; change it with set_precision()
assert PRECISION in MODES, PRECISION


def _side_stream_default(mode):
    """Weight-gradient GEMMs on a stream of their own beside the data-gradient GEMMs?  Not since both branch losses share one
    autograd engine run (round 4): the two halves of the backward already overlap on two streams, and a third chain that forks
    and joins per layer loses in every mode -- default mode 11.68 -> 13.2 ms (``profiles/r04_schedule.txt``), ``bf16x3``
    17.0 -> 18.55 ms, exact fp32 62.5 -> 69.3 ms (same box, ``scripts/time_step_env.py``).  Rounds 2-3, with the halves'
    backward passes in series, had it on for the three-term and fp32 modes (even / +1.5 % there).  WCMC_SIDE_STREAM=1 turns it on."""
    return os.environ.get("WCMC_SIDE_STREAM") == "1"


USE_SIDE_STREAM = _side_stream_default(PRECISION)      # weight-gradient GEMMs beside the data-gradient GEMMs: by mode (see above; streams.py)

# the specular half of the step on a second stream (streams.py: branch_stream, on_branch)
USE_BRANCH_STREAM = os.environ.get("WCMC_BRANCH_STREAM", "1") != "0"   # +1.8 % at B=8 (331 -> 337 patches/s, same box, 3 alternations)

# PathNet.embedding as one launch per direction (csrc/pathnet_fused.hip): hidden activations stay on chip in the forward and
# are recomputed in the backward.  Default mode only (its backward arithmetic is built in); WCMC_FUSE_EMBED=0: A/B switch.
FUSE_EMBED = os.environ.get("WCMC_FUSE_EMBED", "1") != "0"

# The fused embedding reads the channel-first `paths` where it lies (wcmc_embed3_*_nchw) instead of a split copy made by a pass of
# its own in front of the step (pathnet_fused.py: embed_in_place); same results bit for bit.  WCMC_EMBED_IN_PLACE=0: A/B switch.
EMBED_IN_PLACE = os.environ.get("WCMC_EMBED_IN_PLACE", "1") != "0"

# WCMC_FUSE_FINAL=0: A/B switch back to concatenation + fused layer pair (csrc/pathnet_fused.hip; default mode only)
FUSE_FINAL = os.environ.get("WCMC_FUSE_FINAL", "1") != "0"

# The fused final chain's forward hands the hi plane of its hidden activation (bf16, 256 B per pixel) and its output to the backward
# (h_hi / out of wcmc_final2_fwd / _bwd) instead of the backward recomputing both (null pointers there): same results bit for bit, 60 of
# 118 MFMAs per tile and wave fewer, +268 MB live per PathNet between forward and backward at the benchmark shape.  False: recompute.
SAVE_FINAL_HIDDEN = True

# (weight-gradient, data-gradient) MFMAs per product of the chains with a given filter size, where they differ from the mode's:
# the rung table of the backward GEMMs (profiles/r06_grad_rungs.txt; empty = the mode's rungs everywhere)
TERMS_BY_KS = {}

# Emulation hook (scripts/arith_trajectories.py only; None in the product): a callable (split tensor, dims, ksize) -> split tensor applied
# to every HIDDEN activation a split-bf16 chain has just written -- "what if this layer's output were rounded to fp16?" measured on
# training trajectories before any kernel is written.
EMULATE_HIDDEN = None

# Test hook: when a list, every chain forward appends its post-activation layer outputs (used by the
# parity tests to count ReLU sign flips against the oracle; a flipped unit changes gradients by ~1e-3).
DEBUG_ACTS = None

# Slabs of a weight gradient above this size are reduced right behind their GEMM, never deferred (grads.py: deferred slab reductions)
DEFER_MAX_BYTES = 24 << 20

# ---- state the package rebinds itself (set_profiler; deferred_wgrad_reduce): kept here for the same reason -- one binding, read as _sw.<NAME>
_PROFILER = None            # bench.py's per-launch profiler, or None (_base.py: set_profiler, _Timed)
_DEFERRED = None            # None, or {stream id: (stream, [entries])} while a scope is open


# ---------------------------------------------------------------------------------------------------------------- mode helpers
def reduced_backward(mode=None):
    """True in the modes whose backward GEMMs run on two / one MFMAs per product."""
    return (PRECISION if mode is None else mode) in ("bf16x321h", "bf16x321o", "bf16x321")


def set_precision(mode):
    global PRECISION, USE_SIDE_STREAM
    assert mode in MODES, mode
    PRECISION = mode
    USE_SIDE_STREAM = _side_stream_default(mode)


def split_path():
    """True when the conv chains run on the split-bf16 GEMMs (either bf16 mode)."""
    return PRECISION != "fp32"


def wgrad_terms():
    return 1 if reduced_backward() else 3


def dgrad_terms():
    return 2 if reduced_backward() else 3


def chain_terms(ks, cin=None):
    """cin: input channels of the chain's first layer -- a key (ks, cin) singles out one chain (PathNet.embedding: (1, 36), final: (1, 128))."""
    return TERMS_BY_KS.get((ks, cin), TERMS_BY_KS.get(ks, (wgrad_terms(), dgrad_terms())))


def out_layer_terms(ks, act):
    """bf16 MFMAs per product in the FORWARD of a chain's output layer: 1 in the "bf16x321o" mode for a linear (un-gated) 5x5
    output layer -- the shape the library's one-term instance and the measurement behind it cover -- else 3."""
    if PRECISION == "bf16x321h" and ks == 5 and act == "linear":
        return "h"                                              # one fp16 MFMA where wcmc_conv2d_out_f16_supported (decided per shape)
    if not (PRECISION == "bf16x321o" and ks == 5 and act == "linear"):
        return 3
    return 1


# ---------------------------------------------------------------------------------------------------------------- the modules
# Every name each module defines, in dependency order.  (The modules reach the names above through ``_sw``, inside functions only.)
from ._base import (ACT, LEAKY_SLOPE, set_profiler, _Timed, _ptr, _stream, _need_cuda, nhwc_empty, is_nhwc_view, _v,  # noqa: E402,F401
                    to_nhwc_raw, from_nhwc_raw, _ToNHWC, as_nhwc, _as_nhwc_nograd, conv_launch_plan, wgrad_launch_plan, _timed_conv)
from .streams import (_SIDE_STREAMS, _side_stream, _BRANCH_STREAMS, branch_stream, _step_streams, fork_all_streams,  # noqa: E402,F401
                      join_all_streams, _STREAM_PAIRS, _spin_ms, concurrent_stream_pair, on_branch)
from .conv_fp32 import (_pack, conv2d_raw, conv2d_wgrad_raw, act_backward_raw, _ConvChain)  # noqa: E402,F401
from .grads import (_GRAD_SINK, register_grad_sinks, release_grad_sinks, _sink_ex, _sink, _param_ptr, _flushed_by_consumer,  # noqa: E402,F401
                    _WeightNormMulti, WEIGHT_NORM_MAX_LAYERS, weight_norm_multi, deferred_wgrad_reduce, flush_wgrad_reduce,
                    _on_side_stream, _reduce_multi)
from .elementwise import (_MaxPool2, _MaxPool2Skip, maxpool2_skip, _Upsample2, maxpool2, upsample2, _CatChannels, cat_channels,  # noqa: E402,F401
                          _SppMean, spp_mean, _CatBroadcast, cat_broadcast, _PBufferCat, pbuffer_cat, _SampleCat,
                          sample_features_cat)
from .conv_split import (_split_empty, split_raw, split_from_nchw_raw, presplit_shared, split_gated_raw, split_dy_colsum_raw,  # noqa: E402,F401
                         unsplit_debug, _dgrad_mode, _pack_x, _fwd_pack_mode, PACK_MAX_ENTRIES, _pack_chains_x, _pack_chain_x,
                         _chain_out_terms, conv2d_x_raw, conv2d_out_f16_raw, conv1x1_pair_x_raw, colsum_finish_raw,
                         conv2d_wgrad_x_raw, _chainx_forward, _chainx_backward, _ConvChainX, _split_shared, _ChainSppMeanX,
                         _CatBroadcastChainX, _CatUpsampleChainX, conv_chain)
from .pathnet_fused import (_dense_pixel_stride, _EmbedSppMeanFusedX, _FinalFusedX, cat_upsample_chain, _UNFUSED_NOTED,  # noqa: E402,F401
                            _note_unfused, conv_chain_spp_mean, cat_broadcast_chain, embed_in_place, embed_in_place_supported,
                            _reads_in_place)
from .image import (_KernelApply, kernel_apply, chain_kernel_apply, _Recombine, recombine, _image_loss_raw, _L1Mean, l1_mean,  # noqa: E402,F401
                    image_metrics, relative_mse, LOSS2_KINDS, _ImageLoss2, image_loss2, DSSIM_TONEMAPS, dssim_loss_supported,
                    _DssimLoss, dssim_loss, image_eval)
from .splat import (SPLAT_SOFTMAX, SPLAT_SHIFT, _splat_dims, _KernelSplat, kernel_splat, logit_max)  # noqa: E402,F401
from .filter import (PBF_STATS, PBF_FILTER, PBF_MAX_RADIUS, PBF_MAX_PATCH_RADIUS, PBF_MAX_CHANNELS,  # noqa: E402,F401
                     PBF_MAX_IMAGE_CHANNELS, _pbuffer_filter_check, pbuffer_filter)
from .manifold import (_FeatureMSE, _GRS, grs_loss, feature_mse)  # noqa: E402,F401
from .optim import (clip_grad_norm_, clip_adam_, clip_adam_hyper, clip_adam_dev_, step_guard_, step_guard_local_,  # noqa: E402,F401
                    step_guard_global_)
from .data import (_need_dense, preprocess_llpm, preprocess_kpcn, assemble_kpcn_patches, gradients, reflect_index,  # noqa: E402,F401
                   preprocess_kpcn_begin, preprocess_kpcn_rows, preprocess_kpcn_end,
                   importance_map, sampling_prob, sanitize_, random_permutation, random_permutation_dev, step_counter_advance,
                   permutation_key, check_tile_coords, stitch_tiles, preprocess_sbmc, check_patch_origins, sample_feature_size,
                   assemble_sample_patches, preprocess_kpcn_prefix, check_tile_origins, assemble_kpcn_tiles, finish_frame,
                   assemble_sample_tiles, finish_sample_frame, check_patch_transforms, check_frame_transforms, stitch_tiles_aug,
                   stitch_tiles_blend, blend_finish)
