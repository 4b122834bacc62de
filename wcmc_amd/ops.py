"""Autograd wrappers over the C ABI of ``libwcmc_hip.so``.

Tensors between ops are *NHWC views*: logically (N,C,H,W) torch tensors whose
channel stride is 1 and whose pixel stride is padded to a multiple of 4 floats
(``nhwc_empty``).  Slices / crops / concat targets stay views; every kernel takes
explicit strides.  PyTorch here is device memory, streams and autograd plumbing
only -- all arithmetic of the hot path runs in the HIP library.  Nothing in this
file has a CPU path: a tensor that is not on ``cuda`` raises.
"""
import ctypes
import math
import os

import torch

from ._lib import check, lib

ACT = {"linear": 0, "relu": 1, "leaky_relu": 2}
LEAKY_SLOPE = 0.01

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
PRECISION = os.environ.get("WCMC_PRECISION", MODES[0])
assert PRECISION in MODES, PRECISION


def reduced_backward(mode=None):
    """True in the modes whose backward GEMMs run on two / one MFMAs per product."""
    return (PRECISION if mode is None else mode) in ("bf16x321h", "bf16x321o", "bf16x321")


def _side_stream_default(mode):
    """Weight-gradient GEMMs on a stream of their own beside the data-gradient GEMMs?  Not since both branch losses share one
    autograd engine run (round 4): the two halves of the backward already overlap on two streams, and a third chain that forks
    and joins per layer loses in every mode -- default mode 11.68 -> 13.2 ms (``profiles/r04_schedule.txt``), ``bf16x3``
    17.0 -> 18.55 ms, exact fp32 62.5 -> 69.3 ms (same box, ``scripts/time_step_env.py``).  Rounds 2-3, with the halves'
    backward passes in series, had it on for the three-term and fp32 modes (even / +1.5 % there).  WCMC_SIDE_STREAM=1 turns it on."""
    return os.environ.get("WCMC_SIDE_STREAM") == "1"


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


# (weight-gradient, data-gradient) MFMAs per product of the chains with a given filter size, where they differ from the mode's:
# the rung table of the backward GEMMs (profiles/r06_grad_rungs.txt; empty = the mode's rungs everywhere)
TERMS_BY_KS = {}


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

# Optional per-launch timing (bench.py): HIP events recorded on the launch stream around an op.
_PROFILER = None


def set_profiler(prof):
    """prof: object with .add(name, work, unit, ev_start, ev_end) or None to disable."""
    global _PROFILER
    _PROFILER = prof


class _Timed:
    def __init__(self, name, work, unit):
        self.args = (name, work, unit)

    def __enter__(self):
        if _PROFILER is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _PROFILER is not None:
            self.e1.record()
            _PROFILER.add(*self.args, self.e0, self.e1)
        return False


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("wcmc_amd ops run on the MI355X only (got a %s tensor); "
                               "there is no CPU path" % t.device)
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("wcmc_amd ops are fp32 (got %s)" % t.dtype)


def nhwc_empty(n, c, h, w, device, zero=False):
    """(n,c,h,w) tensor backed by an [n][h][w][round_up(c,4)] buffer."""
    cp = (c + 3) // 4 * 4
    mk = torch.zeros if zero else torch.empty
    return mk((n, h, w, cp), device=device, dtype=torch.float32).permute(0, 3, 1, 2)[:, :c]


def is_nhwc_view(t):
    if t.dim() != 4 or t.stride(1) != 1:
        return False
    sn, _, sh, sw = t.stride()
    return (t.data_ptr() % 16 == 0 and sn % 4 == 0 and sh % 4 == 0 and sw % 4 == 0
            and sw >= (t.shape[1] + 3) // 4 * 4)


def _v(t):
    """(ptr, sn, sh, sw) of an NHWC view."""
    return _ptr(t), t.stride(0), t.stride(2), t.stride(3)


def to_nhwc_raw(x):
    """Strided (N,C,H,W) -> fresh NHWC view (no autograd)."""
    n, c, h, w = x.shape
    out = nhwc_empty(n, c, h, w, x.device)
    check(lib().wcmc_to_nhwc(_ptr(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3),
                             *_v(out), n, c, h, w, _stream()), "to_nhwc")
    return out


def from_nhwc_raw(x):
    """NHWC view -> contiguous NCHW (no autograd)."""
    n, c, h, w = x.shape
    out = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
    check(lib().wcmc_from_nhwc(*_v(x), _ptr(out), out.stride(0), out.stride(1), out.stride(2),
                               out.stride(3), n, c, h, w, _stream()), "from_nhwc")
    return out


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return to_nhwc_raw(x)

    @staticmethod
    def backward(ctx, g):
        return from_nhwc_raw(g) if is_nhwc_view(g) else g


def as_nhwc(x):
    _need_cuda(x)
    return x if is_nhwc_view(x) else _ToNHWC.apply(x)


def _as_nhwc_nograd(g):
    return g if is_nhwc_view(g) else to_nhwc_raw(g)


# ------------------------------------------------------------------------ conv chain
def _pack(weight, mode):
    cout, cin, ks, _ = weight.shape
    rows, kch = (cout, cin) if mode == 0 else (cin, cout)
    n = lib().wcmc_conv2d_packed_elems(rows, kch, ks)
    wp = torch.empty(n, device=weight.device, dtype=torch.float32)
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    check(lib().wcmc_conv2d_pack_weight(_ptr(w), _ptr(wp), cout, cin, ks, mode, _stream()), "pack_weight")
    return wp


def conv2d_raw(x, wp, bias, cout, ks, pad, act, gate=None, gate_act="linear", out=None):
    """One implicit-GEMM launch: out = act(conv(x) + bias) [* act'(gate)]."""
    n, cin, h, w = x.shape
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    if out is None:
        out = nhwc_empty(n, cout, ho, wo, x.device)
    g = _v(gate) if gate is not None else (_ptr(None), 0, 0, 0)
    # algorithmic FLOPs: 2 * pixels * Cout * Cin * ks^2 of the (smaller) valid-conv side
    pix = min(ho * wo, h * w)
    with _Timed(_igemm_class(cin, cout, ks), 2.0 * n * pix * cout * cin * ks * ks, "flop"):
        check(lib().wcmc_conv2d_igemm(*_v(x), n, h, w, cin, _ptr(wp), _ptr(bias), *_v(out), cout, ks, pad,
                                      ACT[act], LEAKY_SLOPE, *g, ACT[gate_act], LEAKY_SLOPE, _stream()),
              "conv2d_igemm")
    return out


def conv2d_wgrad_raw(x, dy, ks, pad, weight_shape, want_bias=True):
    n, cin, h, w = x.shape
    cout, ho, wo = dy.shape[1], dy.shape[2], dy.shape[3]
    nbytes = lib().wcmc_conv2d_wgrad_workspace_bytes(n, ho, wo, cout, cin, ks)
    ws = torch.empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32)
    dw = torch.empty(weight_shape, device=x.device, dtype=torch.float32)
    db = torch.empty(cout, device=x.device, dtype=torch.float32) if want_bias else None
    with _Timed("conv_wgrad", 2.0 * n * ho * wo * cout * cin * ks * ks, "flop"):
        check(lib().wcmc_conv2d_wgrad(*_v(x), n, h, w, cin, *_v(dy), cout, ks, pad, _ptr(dw), _ptr(db),
                                      _ptr(ws), ws.numel() * 4, _stream()), "conv2d_wgrad")
    return dw, db


def act_backward_raw(dy, y, act):
    n, c, h, w = y.shape
    dx = nhwc_empty(n, c, h, w, y.device)
    check(lib().wcmc_act_backward(*_v(dy), *_v(y), *_v(dx), n, h, w, c, ACT[act], LEAKY_SLOPE, _stream()),
          "act_backward")
    return dx


# Emulation hook (scripts/arith_trajectories.py only; None in the product): a callable (split tensor, dims, ksize) -> split tensor applied
# to every HIDDEN activation a split-bf16 chain has just written -- "what if this layer's output were rounded to fp16?" measured on
# training trajectories before any kernel is written.
EMULATE_HIDDEN = None

# Test hook: when a list, every chain forward appends its post-activation layer outputs (used by the
# parity tests to count ReLU sign flips against the oracle; a flipped unit changes gradients by ~1e-3).
DEBUG_ACTS = None

_SIDE_STREAMS = {}
USE_SIDE_STREAM = _side_stream_default(PRECISION)      # weight-gradient GEMMs beside the data-gradient GEMMs: by mode (see above)


def _side_stream(device, of=None):
    """The weight-gradient stream that belongs to stream `of` (default: the CURRENT stream), or None when
    weight gradients should stay on that stream.

    The forked specular branch keeps its weight gradients on its own stream: hipStreamEndCapture (ROCm
    7.0) recurses without end when two forked (non-origin) streams of a capture wait on each other
    (each wait registers the waiter as a child of the other), so only the step's origin stream forks
    and joins a weight-gradient stream."""
    if not USE_SIDE_STREAM:
        return None
    of = torch.cuda.current_stream(device) if of is None else of
    br = _BRANCH_STREAMS.get((device.type, device.index))
    if br is not None and br.cuda_stream == of.cuda_stream:
        return None
    key = (device.type, device.index, of.cuda_stream)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


# Branch-level concurrency: the diffuse and specular halves of the step (PathNet backbones, KPCN conv
# stacks + kernel apply, their losses and backward passes) are independent until the optimiser.
# Running the specular half on a second stream lets its kernels fill the CUs that the tail of a
# diffuse launch leaves idle (a conv launch is a whole number of 512-workgroup waves); autograd
# replays each half's backward on the stream its forward ran on.
USE_BRANCH_STREAM = os.environ.get("WCMC_BRANCH_STREAM", "1") != "0"   # +1.8 % at B=8 (331 -> 337 patches/s, same box, 3 alternations)
_BRANCH_STREAMS = {}


def branch_stream(device):
    key = (device.type, device.index)
    if key not in _BRANCH_STREAMS:
        _BRANCH_STREAMS[key] = torch.cuda.Stream(device=device)
    return _BRANCH_STREAMS[key]


def _step_streams(device):
    """The streams one step forks work onto from the current stream."""
    device = torch.device(device)
    cur = torch.cuda.current_stream(device)
    out = [_side_stream(device, cur)]
    if USE_BRANCH_STREAM:
        out.append(branch_stream(device))
    return cur, [s for s in out if s is not None and s.cuda_stream != cur.cuda_stream]


def fork_all_streams(device):
    """Fork every stream the step uses directly from the current stream (under HIP stream capture: make
    them first-level children of the capturing stream before anything else touches them)."""
    if torch.device(device).type != "cuda":
        return
    cur, streams = _step_streams(device)
    for s in streams:
        s.wait_stream(cur)


def join_all_streams(device):
    """Make the current stream wait for every stream the step forked work onto (a stream capture must
    not end with forked work outstanding)."""
    if torch.device(device).type != "cuda":
        return
    cur, streams = _step_streams(device)
    for s in streams:
        cur.wait_stream(s)


# Two streams overlap on the GPU only when the HIP runtime has mapped them onto DIFFERENT hardware queues; it deals its (few) queues
# out to streams as they are created, so two freshly made streams may share one and then run strictly one after the other -- the
# "lottery" of rounds 3-4 (a captured step whose halves ran in series: 13.4 instead of 11.7 ms, decided at stream creation and stable
# for the life of the streams).  ``concurrent_stream_pair`` makes streams until two of them demonstrably run a pair of spin kernels
# side by side, once per device and process; the two-stream step replays its halves on that pair.
_STREAM_PAIRS = {}


def _spin_ms(streams, cycles):
    cur = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for s in streams:
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
    for s in streams:
        cur.wait_stream(s)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def concurrent_stream_pair(device, tries=8):
    """Two side streams of `device` that run concurrently (probed with spin kernels), cached per device; ``.probe`` on the returned
    tuple's first stream holds what was measured (ms of one spin kernel, of the accepted pair, streams tried)."""
    device = torch.device(device)
    key = (device.type, device.index)
    if key in _STREAM_PAIRS:
        return _STREAM_PAIRS[key]
    with torch.cuda.device(device):
        first = torch.cuda.Stream(device=device)
        if not hasattr(torch.cuda, "_sleep"):                # (no spin kernel to probe with: two fresh streams, unprobed)
            pair = (first, torch.cuda.Stream(device=device))
            pair[0].probe = {"spin_ms": None, "pair_ms": None, "streams_tried": 2, "concurrent": None}
            _STREAM_PAIRS[key] = pair
            return pair
        cycles = 200000
        one = _spin_ms([first], cycles)
        one = _spin_ms([first], cycles)                      # (second run: without first-launch costs)
        if one < 0.2:                                        # aim at ~0.3 ms per spin: long against launch latencies
            cycles = int(cycles * 0.3 / max(one, 1e-3))
            one = _spin_ms([first], cycles)
        pool, best = [first], None
        for _ in range(tries):
            cand = torch.cuda.Stream(device=device)
            for other in pool:
                t = min(_spin_ms([other, cand], cycles), _spin_ms([other, cand], cycles))
                if best is None or t < best[0]:
                    best = (t, other, cand)
                if t < 1.4 * one:
                    break
            pool.append(cand)
            if best[0] < 1.4 * one:
                break
    pair = (best[1], best[2])
    pair[0].probe = {"spin_ms": round(one, 4), "pair_ms": round(best[0], 4), "streams_tried": len(pool), "concurrent": bool(best[0] < 1.4 * one)}
    _STREAM_PAIRS[key] = pair
    return pair


class on_branch:
    """``with on_branch(device) as br: y = f(x)`` runs f on the branch stream after everything enqueued
    so far on the current stream; ``br.join(y, ...)`` makes the current stream wait for it."""

    def __init__(self, device):
        self.enabled = USE_BRANCH_STREAM and torch.device(device).type == "cuda"
        if self.enabled:
            self.main = torch.cuda.current_stream(device)
            self.stream = branch_stream(torch.device(device))
            self.ctx = torch.cuda.stream(self.stream)

    def __enter__(self):
        if self.enabled:
            self.stream.wait_stream(self.main)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.enabled:
            self.ctx.__exit__(*exc)
        return False

    def join(self, *tensors):
        if self.enabled:
            self.main.wait_stream(self.stream)
            for t in tensors:
                if isinstance(t, torch.Tensor):
                    t.record_stream(self.main)


class _ConvChain(torch.autograd.Function):
    """A whole ``sbmc.modules.ConvChain`` as one autograd node.

    spec = (ksize, pad, [act per layer]).  params = w0, b0, w1, b1, ...
    The backward fuses each hidden ReLU mask into the epilogue of the data-gradient
    GEMM that produces the masked tensor, and puts the weight-gradient GEMM of layer l
    on a second HIP stream: it only depends on (x_l, dy_l), so it fills the CUs that the
    tail of the data-gradient launch of the same layer leaves idle (a launch is a whole
    number of 512-block waves on 256 CUs).
    """

    @staticmethod
    def forward(ctx, x, spec, *params):
        ks, pad, acts = spec
        _need_cuda(x, *params)
        nl = len(acts)
        xs = [x]
        for l in range(nl):
            w, b = params[2 * l], params[2 * l + 1]
            if w.shape[1] != xs[-1].shape[1]:
                raise RuntimeError("conv chain layer %d: weight expects %d input channels, got a tensor with %d"
                                   % (l, w.shape[1], xs[-1].shape[1]))
            wp = _pack(w, 0)
            xs.append(conv2d_raw(xs[-1], wp, b.detach(), w.shape[0], ks, pad, acts[l]))
        ctx.spec = spec
        ctx.save_for_backward(*xs, *[params[2 * l] for l in range(nl)])
        if DEBUG_ACTS is not None:
            DEBUG_ACTS.extend(t for t, a in zip(xs[1:], acts) if a != "linear")
        return xs[-1]

    @staticmethod
    def backward(ctx, dy):
        ks, pad, acts = ctx.spec
        nl = len(acts)
        saved = ctx.saved_tensors
        xs, ws = saved[:nl + 1], saved[nl + 1:]
        dy = _as_nhwc_nograd(dy)
        if acts[-1] != "linear":
            dy = act_backward_raw(dy, xs[nl], acts[-1])
        grads = [None] * (2 * nl)
        dx = None
        main = torch.cuda.current_stream()
        side = _side_stream(dy.device)
        keep = []                       # every dy stays allocated until the side stream has joined
        for l in range(nl - 1, -1, -1):
            w = ws[l]
            if side is not None:
                side.wait_stream(main)                      # dy_l is ready
                with torch.cuda.stream(side):
                    dw, db = conv2d_wgrad_raw(xs[l], dy, ks, pad, w.shape)
                dw.record_stream(main)
                db.record_stream(main)
                keep.append(dy)
            else:
                dw, db = conv2d_wgrad_raw(xs[l], dy, ks, pad, w.shape)
            grads[2 * l], grads[2 * l + 1] = dw, db
            if l > 0 or ctx.needs_input_grad[0]:
                wpt = _pack(w, 1)
                gate = xs[l] if l > 0 else None
                gate_act = acts[l - 1] if l > 0 else "linear"
                dy = conv2d_raw(dy, wpt, None, w.shape[1], ks, ks - 1 - pad, "linear",
                                gate=gate, gate_act=gate_act)
                dx = dy
        if side is not None:
            main.wait_stream(side)      # join: grads are visible to (and memory reuse ordered after) main
        del keep
        return (dx if ctx.needs_input_grad[0] else None, None, *grads)


# ---- gradient sinks --------------------------------------------------------------------------
# FusedClipAdam keeps one flat gradient bucket per model (the RCCL message, the clip + Adam kernel's input).  Autograd hands a
# parameter's gradient to it as whatever tensor the backward returns -- so the weight-gradient kernels write their result
# STRAIGHT INTO the parameter's slice of the bucket and return that view: AccumulateGrad adopts it (p.grad was None) and the
# optimiser's gather (three multi-tensor copies, 60 us per step) has nothing left to move.  A parameter whose .grad is already
# set (a second backward without zero_grad) gets a fresh tensor instead, which autograd accumulates as usual -- and so does the
# SECOND producer of a parameter's gradient inside one engine run (a chain applied to two inputs: AccumulateGrad runs after
# both, so a second hand-out of the same view would have the later node overwrite the earlier one's result and the engine sum
# two aliases): a sink is out while the tensor that was handed out is alive -- in the engine's buffers until AccumulateGrad
# has run, in ``p.grad`` afterwards, gone after ``zero_grad()`` -- or until ``release_grad_sinks`` (the optimiser's gather).
import weakref

_GRAD_SINK = {}


def register_grad_sinks(params, views):
    for p, v in zip(params, views):
        _GRAD_SINK[p.data_ptr()] = [weakref.ref(p), weakref.ref(v), None]


def release_grad_sinks(params):
    """End of an accumulation window: the gradients of `params` have been consumed (or dropped); their sinks may be handed out again."""
    for p in params:
        e = _GRAD_SINK.get(p.data_ptr())
        if e is not None:
            e[2] = None


def _sink_ex(param_ptr, shape, device):
    """(tensor, is_bucket_view): the bucket view a gradient of `shape` for the parameter at `param_ptr` may be written into, or a
    fresh tensor.  A bucket view is handed out only for a parameter that requires a gradient and has none yet (AccumulateGrad will
    adopt the tensor), and its memory belongs to the optimiser: it outlives the step."""
    e = _GRAD_SINK.get(param_ptr)
    if e is not None:
        p, v = e[0](), e[1]()
        if p is None or v is None or p.data_ptr() != param_ptr:
            del _GRAD_SINK[param_ptr]
        elif (p.grad is None and p.requires_grad and (e[2] is None or e[2]() is None) and tuple(v.shape) == tuple(shape)
              and v.device == device):
            out = v.detach()                    # (a new tensor object on the same memory: AccumulateGrad may adopt it)
            e[2] = weakref.ref(out)
            return out, True
    return torch.empty(shape, device=device, dtype=torch.float32), False


def _sink(param_ptr, shape, device):
    return _sink_ex(param_ptr, shape, device)[0]


def _param_ptr(t):
    return t.data_ptr() if isinstance(t, torch.nn.Parameter) else 0


def _flushed_by_consumer(w):
    """True when the gradient of weight `w` is read by a node that flushes the deferred slab reductions first: `w` is an output
    of ``_WeightNormMulti`` itself (defined below; looked up when called)."""
    return isinstance(w.grad_fn, _WeightNormMulti._backward_cls)


# ---- weight normalisation ------------------------------------------------------------------
class _WeightNormMulti(torch.autograd.Function):
    """``w_l = g_l * v_l / ||v_l||`` for ALL weight-normalised layers of a model as one node: one launch forms every effective
    weight before the model's first chain (``wcmc_weight_norm_fwd``), one launch turns every chain's weight gradient into
    (dg, dv) once the last of them has arrived (``wcmc_weight_norm_bwd``), written straight into the optimiser's bucket.
    Arguments g0, v0, g1, v1, ...; returns (w0, w1, ...)."""

    @staticmethod
    def forward(ctx, *gv):
        n = len(gv) // 2
        gs, vs = gv[0::2], gv[1::2]
        _need_cuda(*gv)
        ctx.set_materialize_grads(False)            # (a layer no chain used arrives as None, not as a tensor of zeros)
        dev = vs[0].device
        rows = [v.shape[0] for v in vs]
        lens = [v[0].numel() for v in vs]
        vc = [v.detach() if v.is_contiguous() else v.detach().contiguous() for v in vs]
        gc = [g.detach().reshape(-1) if g.is_contiguous() else g.detach().contiguous().reshape(-1) for g in gs]
        # one block for all effective weights (each on a 256-byte boundary) and one for the norms
        offs, off = [], 0
        for v in vc:
            offs.append(off)
            off += (v.numel() + 63) // 64 * 64
        flat = torch.empty(off, device=dev, dtype=torch.float32)
        ws = [flat[o:o + v.numel()].view(v.shape) for o, v in zip(offs, vc)]
        noffs = [sum(rows[:i]) for i in range(n)]
        norms = torch.empty(sum(rows), device=dev, dtype=torch.float32)
        nv = [norms[o:o + r] for o, r in zip(noffs, rows)]
        ap, ai = ctypes.c_void_p * n, ctypes.c_int * n
        check(lib().wcmc_weight_norm_fwd(n, ap(*[t.data_ptr() for t in vc]), ap(*[t.data_ptr() for t in gc]),
                                         ap(*[t.data_ptr() for t in ws]), ap(*[t.data_ptr() for t in nv]),
                                         ai(*rows), ai(*lens), _stream()), "weight_norm_fwd")
        ctx.geom = (rows, lens, noffs)
        ctx.sinks = [(_param_ptr(g), _param_ptr(v)) for g, v in zip(gs, vs)]
        ctx.save_for_backward(norms, *gc, *vc)
        return tuple(ws)

    @staticmethod
    def backward(ctx, *dws):
        rows, lens, noffs = ctx.geom
        n = len(rows)
        flush_wgrad_reduce()                    # (deferred slab reductions of this stream: the dw this node is about to read)
        saved = ctx.saved_tensors
        norms, gc, vc = saved[0], saved[1:1 + n], saved[1 + n:]
        dev = norms.device
        live = [l for l in range(n) if dws[l] is not None]      # (a layer no chain used this step has no gradient: None, as torch)
        grads = [None] * (2 * n)
        if not live:
            return tuple(grads)
        dw, dv, dg = [], [], []
        for l in live:
            d = dws[l]
            dw.append(d if d.is_contiguous() else d.contiguous())
            gp, vp = ctx.sinks[l]
            dg.append(_sink(gp, (rows[l], 1, 1, 1), dev))
            dv.append(_sink(vp, vc[l].shape, dev))
            grads[2 * l], grads[2 * l + 1] = dg[-1], dv[-1]
        m = len(live)
        ap, ai = ctypes.c_void_p * m, ctypes.c_int * m
        check(lib().wcmc_weight_norm_bwd(m, ap(*[t.data_ptr() for t in dw]), ap(*[vc[l].data_ptr() for l in live]),
                                         ap(*[gc[l].data_ptr() for l in live]),
                                         ap(*[norms[noffs[l]:].data_ptr() for l in live]), ap(*[t.data_ptr() for t in dv]),
                                         ap(*[t.data_ptr() for t in dg]), ai(*[rows[l] for l in live]),
                                         ai(*[lens[l] for l in live]), _stream()), "weight_norm_bwd")
        return tuple(grads)


WEIGHT_NORM_MAX_LAYERS = 32


def weight_norm_multi(gs, vs):
    """[w_l] of ``torch.nn.utils.weight_norm``'s parametrisation for the layers (g_l, v_l), <= 32 of them per launch."""
    out = []
    for i in range(0, len(gs), WEIGHT_NORM_MAX_LAYERS):
        gv = []
        for g, v in zip(gs[i:i + WEIGHT_NORM_MAX_LAYERS], vs[i:i + WEIGHT_NORM_MAX_LAYERS]):
            gv += [g, v]
        out += list(_WeightNormMulti.apply(*gv))
    return out


# ---- split-bf16 chain ----------------------------------------------------------------------
def _split_empty(n, c, h, w, device):
    return torch.empty(lib().wcmc_split_elems(n, h, w, c), device=device, dtype=torch.int16)


def split_raw(x):
    """fp32 NHWC view -> dense split tensor (int16 storage of [N][H][W][2][round_up(C,8)] bf16)."""
    n, c, h, w = x.shape
    out = _split_empty(n, c, h, w, x.device)
    check(lib().wcmc_split_bf16(*_v(x), _ptr(out), n, h, w, c, _stream()), "split_bf16")
    return out


def split_from_nchw_raw(x):
    """Strided channel-first (N,C,H,W) fp32 -> split tensor in one pass (wcmc_split_from_nchw; C <= 64)."""
    n, c, h, w = x.shape
    out = _split_empty(n, c, h, w, x.device)
    check(lib().wcmc_split_from_nchw(_ptr(x), *x.stride(), _ptr(out), n, c, h, w, _stream()), "split_from_nchw")
    return out


def presplit_shared(x):
    """Attach the split form of the channel-first tensor `x` to it so that ``conv_chain_spp_mean(x, ...)`` consumes it
    directly -- on ANY stream that was forked after this call (the two PathNets embed the same `paths`, the second one on
    the forked specular stream: the split is made once, before the fork).  Returns x."""
    _need_cuda(x)
    x._wcmc_split = ((x._version, None), split_from_nchw_raw(x))
    return x


def split_gated_raw(dy, post, act):
    """split(dy * act'(post)) in one pass (wcmc_split_gated_bf16): act_backward_raw + split_raw."""
    n, c, h, w = dy.shape
    out = _split_empty(n, c, h, w, dy.device)
    check(lib().wcmc_split_gated_bf16(*_v(dy), *_v(post), ACT[act], LEAKY_SLOPE, _ptr(out), n, h, w, c, _stream()),
          "split_gated_bf16")
    return out


def split_dy_colsum_raw(dims, dy=None, post=None, act="linear", gm=None, s=1, scale=1.0):
    """``split((dy [+ repeat_S(gm) * scale]) [* act'(post)])`` and the per-block column sums of the result in one pass
    (wcmc_split_dy_colsum_bf16): the split gradient entering a chain's backward plus its last layer's bias-gradient
    partials.  dims = (N, C, H, W) of the result."""
    n, c, h, w = dims
    dev = (dy if dy is not None else gm).device
    out = _split_empty(n, c, h, w, dev)
    part = torch.empty(lib().wcmc_conv2d_igemm_colsum_elems(n, h, w, c), device=dev, dtype=torch.float32)
    z = (_ptr(None), 0, 0, 0)
    check(lib().wcmc_split_dy_colsum_bf16(*(_v(dy) if dy is not None else z), *(_v(post) if post is not None else z), ACT[act],
                                          LEAKY_SLOPE, *(_v(gm) if gm is not None else z), s, float(scale), _ptr(out), _ptr(part),
                                          n, h, w, c, _stream()), "split_dy_colsum_bf16")
    return out, part


def unsplit_debug(t, n, c, h, w):
    """split tensor -> fp32 (N,C,H,W) with torch ops; test / debug only."""
    cp = (c + 7) // 8 * 8
    v = t.view(torch.bfloat16).view(n, h, w, 2, cp).float()
    return (v[:, :, :, 0] + v[:, :, :, 1])[..., :c].permute(0, 3, 1, 2)


def _dgrad_mode(terms=None):
    """Packing mode of the data-gradient weights: 1 = three-term launch, 2 = the K order of a two-term launch (x hi plane only)."""
    return 2 if (dgrad_terms() if terms is None else terms) == 2 else 1


def _pack_x(weight, mode):
    """mode 0: forward orientation; 1 / 2: the data-gradient orientation for a three- / two-term launch (_dgrad_mode); 3: the
    forward orientation in the K order of a two- / one-term launch (an output layer of the "bf16x321o" mode)."""
    cout, cin, ks, _ = weight.shape
    rows, kch = (cout, cin) if mode in (0, 3, 4) else (cin, cout)
    wp = torch.empty(lib().wcmc_conv2d_packed_elems_bf16x3(rows, kch, ks, mode), device=weight.device, dtype=torch.int16)
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    check(lib().wcmc_conv2d_pack_weight_bf16x3(_ptr(w), _ptr(wp), cout, cin, ks, mode, _stream()),
          "pack_weight_bf16x3")
    return wp


# One packing launch per chain (all layers, both orientations: wcmc_conv2d_pack_chain_bf16x3) instead of two per layer:
# 114 launches per step become 16 (bit-identical to per-layer packing, which chains of more than 10 layers still take).


def _fwd_pack_mode(out_terms):
    """Packing mode of an output layer's forward weights: 0 (three terms), 3 (hi-plane K order: two / one bf16 term), 4 (fp16)."""
    return 4 if out_terms == "h" else 0 if out_terms == 3 else 3


PACK_MAX_ENTRIES = 32       # (layer, orientation) pairs per wcmc_conv2d_pack_chain_bf16x3 launch


def _pack_chains_x(chains, ks):
    """chains: [(weights, out_terms)] of filter size ks -> per chain [(wp_mode0, wp_mode1, (mode0, mode1))] per layer, ALL packed by
    ONE launch.  out_terms < 3: that chain's LAST layer's forward pack is made in the K order of a hi-plane launch (mode 3 / 4)."""
    assert sum(2 * len(w) for w, _ in chains) <= PACK_MAX_ENTRIES
    dev = chains[0][0][0].device
    ws, outs, couts, cins, modes, keep, res = [], [], [], [], [], [], []
    for weights, out_terms in chains:
        n = len(weights)
        dmode = _dgrad_mode(chain_terms(ks, weights[0].shape[1])[1])
        per = []
        for li, wt in enumerate(weights):
            w = wt.detach()
            if not w.is_contiguous():
                w = w.contiguous()
            keep.append(w)
            cout, cin = w.shape[0], w.shape[1]
            pair = []
            for mode in (_fwd_pack_mode(out_terms) if li == n - 1 else 0, dmode):
                rows, kch = (cout, cin) if mode in (0, 3, 4) else (cin, cout)
                wp = torch.empty(lib().wcmc_conv2d_packed_elems_bf16x3(rows, kch, ks, mode), device=dev, dtype=torch.int16)
                ws.append(w.data_ptr()); outs.append(wp.data_ptr()); couts.append(cout); cins.append(cin); modes.append(mode)
                pair.append(wp)
            per.append((pair[0], pair[1], (_fwd_pack_mode(out_terms) if li == n - 1 else 0, dmode)))
        res.append(per)
    m = len(ws)
    arr_p, arr_i = ctypes.c_void_p * m, ctypes.c_int * m
    check(lib().wcmc_conv2d_pack_chain_bf16x3(m, arr_p(*ws), arr_p(*outs), arr_i(*couts), arr_i(*cins), arr_i(*modes), ks,
                                              _stream()), "conv2d_pack_chain_bf16x3")
    return res


def _pack_chain_x(weights, ks, out_terms=3):
    """[(wp_mode0, wp_mode1)] of the OIHW weights of one chain, packed by ONE launch."""
    return [(a, b) for a, b, _ in _pack_chains_x([(weights, out_terms)], ks)[0]]


def _chain_out_terms(ks, act_last, cin_last, cout_last, pair):
    """MFMAs per product of a chain's output layer's forward (3, 1, or "h": one fp16 MFMA), as _chainx_forward decides it."""
    oterms = 3 if pair else out_layer_terms(ks, act_last)
    if oterms == "h" and not lib().wcmc_conv2d_out_f16_supported(cin_last, cout_last, ks):
        oterms = 3
    return oterms


def _igemm_class(cin, cout, ks, dims=None, terms=3):
    """Profiler class of a split-bf16 GEMM launch = the kernel the library's plan picks for it
    (csrc/conv_bf16x3.hip: x_plan_k, x_pick_nt; csrc/bf16x3_pw.hip: x_plan_pw; csrc/bf16x3_halo3.hip: x_halo3_ok; csrc/bf16x3_halo64.hip: launch_xhalo64), so that a class average is one kernel's average.
    dims = (n, ho, wo) of the output selects between the two tile heights of the 5x5 kernel; terms = 2 (the data gradient of
    the default mode) runs the AP = 1 instances where the plan grants them: classes with the suffix "_x2"; terms = 1 (the output
    layers' forward of the default mode): "_x1"."""
    tiles = (cout + 15) // 16
    nt = min((7, 4, 2, 1), key=lambda t: (-(-tiles // t)) * (t + 2))
    halo = 3 <= ks <= 5 and (cin + 7) // 8 * 8 >= 32
    if ks == 1 and ((cin + 7) // 8 * 8, cout) in ((64, 64), (40, 64), (128, 128), (8, 128)):
        return "conv_pw"                    # x_plan_pw: the persistent pointwise kernel (HBM-bound class)
    if halo and ks == 3 and (cout + 15) // 16 * 16 % 64 == 0:
        # conv_halo3_bf16x3_kernel (x_halo3_ok): the U-Net's 3x3 layers -- slabs of exactly 64 channels (three terms) or of 64 / 128
        # channels of the hi plane (two terms: "_x2")
        kp3 = (cin + 7) // 8 * 8
        if terms >= 3 and kp3 % 64 == 0:
            return "conv_halo3"
        if terms <= 2 and (kp3 == 64 or kp3 % 128 == 0):
            return "conv_halo3_x2"
    if not (halo and nt == 7 and ks == 5):
        return "conv_igemm"
    if dims is None:
        return "conv_halo7"                 # (the fp32 path's 5x5 class)
    n, ho, wo = dims                        # conv_halo64_bf16x3_kernel<7, NB, PT>: 16x16 tiles (PT = 4; also the mixed 16 / 12 heights) or 12x16 (PT = 3)
    kp = (cin + 7) // 8 * 8
    x2 = terms <= 2 and kp % 32 != 24      # x_plan_k grants ap = 1 (32-channel slabs, 80 B)
    x1 = x2 and terms == 1              # ... and the one-plane weight path: <7, 3, PT, 0, 80, 1, 1>, suffix "_x1"
    if not x2 and kp >= 256 and kp % 32 == 0:
        return "conv_halo64_cs32"           # 32-channel slabs: <7, 2, 3> (two weight stages, 12x16 tiles)
    gy = -(-tiles // nt)
    rounds = lambda th: -(-(n * (-(-wo // 16)) * (-(-ho // th)) * gy) // 512) * th
    pt3 = rounds(12) < rounds(16)
    # round 6: where 16 does not divide ho but a rows of 16 + b >= 1 rows of 12 cover it exactly, the 16-row instance runs (mixed tile heights)
    if ho % 16 != 0 and any((ho - 12 * b) % 16 == 0 for b in range(1, (ho - 1) // 12 + 1)):
        pt3 = False
    return ("conv_halo64_pt3" if pt3 else "conv_halo64_pt4") + ("_x1" if x1 else "_x2" if x2 else "")


def _wgrad_class(n, ho, cin, cout, ks):
    rows = ks == 5 and (cin + 15) // 16 == 7 and ((cout + 15) // 16) % 7 == 0 and n * ho >= 64
    return "conv_wgrad_rows" if rows else "conv_wgrad"


def conv2d_x_raw(xs, dims, wp, bias, cout, ks, pad, act, out_split, gate=None, gate_act="linear", colsum=False,
                 gate_mask=None, mask_out=False, terms=3, out=None):
    """One split-bf16 implicit-GEMM launch.  xs: split tensor of dims (n,cin,h,w).
    terms: bf16 MFMAs per product -- 3, 2 = the hi plane of xs only (wp packed with mode 2: the data gradient of the
    "bf16x321" modes, whose xs is dy; or mode 3: a forward launch), 1 = the hi planes of xs and wp only (mode 3: the un-gated
    output layer of the "bf16x321o" mode).
    Returns a split tensor when out_split else an fp32 NHWC view; with colsum=True also the per-tile
    column sums of the result (the consumer layer's bias gradient, see colsum_finish_raw); with mask_out=True
    also the (hi plane > 0) bit mask of the result, which a later launch can take as gate_mask instead of
    re-reading the tensor as gate."""
    n, cin, h, w = dims
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    dev = xs.device
    if out_split:
        ysp, yf, yv = _split_empty(n, cout, ho, wo, dev), None, (_ptr(None), 0, 0, 0)
    else:
        # (out: an fp32 NHWC view of (n, cout, ho, wo) to write into -- e.g. a channel slice of a wider tensor)
        yf = nhwc_empty(n, cout, ho, wo, dev) if out is None else out
        assert tuple(yf.shape) == (n, cout, ho, wo)
        ysp, yv = None, _v(yf)
    pix = min(ho * wo, h * w)
    part = None
    if colsum:
        part = torch.empty(lib().wcmc_conv2d_igemm_colsum_elems(n, ho, wo, cout), device=dev, dtype=torch.float32)
    mask = None
    if mask_out:
        mask = torch.empty(n * ho * wo * ((cout + 7) // 8), device=dev, dtype=torch.uint8)
    cls = _igemm_class(cin, cout, ks, (n, ho, wo), terms) if pad == 0 or ks > 1 else "conv_igemm"
    if cls == "conv_pw":    # algorithmic bytes: the split input and the split / fp32 output, 4 B per channel and pixel
        work = (4.0 * n * pix * ((cin + 7) // 8 * 8 + cout), "byte")
    else:
        work = (2.0 * n * pix * cout * cin * ks * ks, "flop")
    with _Timed(cls, *work):
        check(lib().wcmc_conv2d_igemm_bf16x3(_ptr(xs), n, h, w, cin, _ptr(wp), _ptr(bias), *yv, _ptr(ysp), cout,
                                             ks, pad, ACT[act], LEAKY_SLOPE, _ptr(gate), ACT[gate_act], LEAKY_SLOPE,
                                             _ptr(part), _ptr(gate_mask), _ptr(mask), terms, _stream()), "conv2d_igemm_bf16x3")
    out = ysp if out_split else yf
    ret = (out,) + ((part,) if colsum else ()) + ((mask,) if mask_out else ())
    return ret if len(ret) > 1 else out


def conv2d_out_f16_raw(xs, dims, wp16, bias, cout, ks, pad):
    """The forward of an un-gated 5x5 output layer with one fp16 MFMA per product (wcmc_split_to_f16 + wcmc_conv2d_out_f16): xs the
    split input of dims (n, cin, h, w), wp16 packed with mode 4; returns conv(x, W) + bias as an fp32 NHWC view."""
    n, cin, h, w = dims
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    x16 = torch.empty(lib().wcmc_split_to_f16_elems(n, h, w, cin), device=xs.device, dtype=torch.int16)
    check(lib().wcmc_split_to_f16(_ptr(xs), n, h, w, cin, _ptr(x16), _stream()), "split_to_f16")
    y = nhwc_empty(n, cout, ho, wo, xs.device)
    with _Timed(_igemm_class(cin, cout, ks, (n, ho, wo), 1).replace("_x1", "_h1"), 2.0 * n * min(ho * wo, h * w) * cout * cin * ks * ks, "flop"):
        check(lib().wcmc_conv2d_out_f16(_ptr(x16), n, h, w, cin, _ptr(wp16), _ptr(bias), *_v(y), cout, ks, pad, _stream()), "conv2d_out_f16")
    return y


def conv1x1_pair_x_raw(xs, dims, wp1, b1, cout1, act1, wp2, b2, cout2, act2, gate_mask=None, gate_act="linear",
                       colsum=False, mask_out=True):
    """Two 1x1 layers in one launch (wcmc_conv1x1_pair_bf16x3): returns (split result of the first layer, its 1-bit
    mask or None, its column-sum partials or None, fp32 NHWC output of the second layer)."""
    n, cin, h, w = dims
    dev = xs.device
    ysp = _split_empty(n, cout1, h, w, dev)
    mask = torch.empty(n * h * w * ((cout1 + 7) // 8), device=dev, dtype=torch.uint8) if mask_out else None
    part = None
    if colsum:
        part = torch.empty(lib().wcmc_conv2d_igemm_colsum_elems(n, h, w, cout1), device=dev, dtype=torch.float32)
    y2 = nhwc_empty(n, cout2, h, w, dev)
    with _Timed("conv_pw", 4.0 * n * h * w * ((cin + 7) // 8 * 8 + cout1 + (cout2 + 3) // 4 * 4), "byte"):
        check(lib().wcmc_conv1x1_pair_bf16x3(_ptr(xs), n, h, w, cin, _ptr(wp1), _ptr(b1), cout1, ACT[act1], LEAKY_SLOPE,
                                             _ptr(ysp), _ptr(mask), _ptr(gate_mask), ACT[gate_act], LEAKY_SLOPE,
                                             _ptr(part), _ptr(wp2), _ptr(b2), cout2, ACT[act2], LEAKY_SLOPE,
                                             *_v(y2), _stream()), "conv1x1_pair_bf16x3")
    return ysp, mask, part, y2


def colsum_finish_raw(part, dims):
    n, c, h, w = dims
    db = torch.empty(c, device=part.device, dtype=torch.float32)
    check(lib().wcmc_colsum_finish(_ptr(part), n, h, w, c, _ptr(db), _stream()), "colsum_finish")
    return db


# ---- deferred slab reductions ----------------------------------------------------------------------------------------------
# A weight-gradient launch is a split-K GEMM into slabs plus the slabs' reduction (and the bias gradient's finish).  Nothing reads
# dw before the optimiser -- or, in a weight-normalised model, before its weight-norm backward -- so inside a
# ``deferred_wgrad_reduce()`` scope (the interface opens one around its backward passes) the reductions of the SMALL layers are
# collected per stream and run as ONE launch (``wcmc_conv2d_wgrad_reduce_multi``) when the scope ends or the weight-norm backward
# asks: a PathNet's fifteen U-Net reductions of 5-15 us each, which neither fill the chip nor amortise their launch boundaries.
# Layers whose slabs are large (KPCN's 5x5 layers: 60 MB) keep their reduction right behind the GEMM, while the slabs are still
# in the Infinity Cache.  Results are bit-identical either way.
DEFER_MAX_BYTES = 24 << 20
_DEFERRED = None            # None, or {stream id: (stream, [entries])} while a scope is open


class deferred_wgrad_reduce:
    def __enter__(self):
        global _DEFERRED
        self.outer = _DEFERRED
        if _DEFERRED is None:
            _DEFERRED = {}
        return self

    def __exit__(self, *exc):
        global _DEFERRED
        if self.outer is None:
            pending, _DEFERRED = _DEFERRED, None
            if exc[0] is None:
                for st, entries in pending.values():
                    with torch.cuda.stream(st):
                        _reduce_multi(entries)
        return False


def flush_wgrad_reduce():
    """Run the reductions collected so far on the CURRENT stream (their results are about to be read).  Entries are only ever
    queued under the stream their GEMM ran on and never under a weight-gradient side stream (conv2d_wgrad_x_raw reduces inline
    there), so the reader's stream is where they all are."""
    if _DEFERRED:
        st = torch.cuda.current_stream()
        hit = _DEFERRED.pop(st.cuda_stream, None)
        if hit is not None:
            _reduce_multi(hit[1])


def _on_side_stream():
    cur = torch.cuda.current_stream().cuda_stream
    return any(s.cuda_stream == cur for s in _SIDE_STREAMS.values())


def _reduce_multi(entries):
    for terms in sorted({e[-1] for e in entries}):
        group = [e for e in entries if e[-1] == terms]
        for i in range(0, len(group), 32):
            chunk = group[i:i + 32]
            m = len(chunk)
            ap, ai = ctypes.c_void_p * m, ctypes.c_int * m
            cols = list(zip(*chunk))            # ws, dw, db, cs, n, ho, wo, cout, cin, ks, terms
            ptrs = lambda ts: ap(*[(t if isinstance(t, int) else t.data_ptr()) if t is not None else 0 for t in ts])
            check(lib().wcmc_conv2d_wgrad_reduce_multi(m, ptrs(cols[0]), ptrs(cols[1]), ptrs(cols[2]), ptrs(cols[3]), ai(*cols[4]),
                                                       ai(*cols[5]), ai(*cols[6]), ai(*cols[7]), ai(*cols[8]), ai(*cols[9]), terms,
                                                       _stream()), "conv2d_wgrad_reduce_multi")


def conv2d_wgrad_x_raw(xs, xdims, dys, cout, ks, pad, weight_shape, want_bias=True, colsum_part=None, terms=None, sinks=(0, 0),
                       dw_flushed=False):
    """dw (and db) of one layer.  colsum_part: the per-tile column sums of dys that the launch producing dys left; the bias
    gradient is then finished by the slab-reduction launch itself (no column-sum pass, no finish launch).  sinks: data_ptr of the
    weight / bias PARAMETER (0: none) -- their gradients go straight into the optimiser's bucket where one is registered.
    dw_flushed: the weight is an output of ``_WeightNormMulti``, whose backward flushes this stream's deferred reductions before
    it reads dw (``_flushed_by_consumer``)."""
    n, cin, h, w = xdims
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    nbytes = lib().wcmc_conv2d_wgrad_bf16x3_workspace_bytes(n, ho, wo, cout, cin, ks)
    ws = torch.empty((nbytes + 3) // 4, device=xs.device, dtype=torch.float32)
    dw, dw_view = _sink_ex(sinks[0], weight_shape, xs.device)
    db, db_view = _sink_ex(sinks[1], (cout,), xs.device) if (want_bias or colsum_part is not None) else (None, True)
    args = (_ptr(xs), n, h, w, cin, _ptr(dys), cout, ks, pad, _ptr(dw), _ptr(db), _ptr(ws), ws.numel() * 4)
    cs = _ptr(colsum_part)
    terms = wgrad_terms() if terms is None else terms
    # A reduction may be deferred only where the memory it will write is certain to be the gradient's when it runs:
    # a bucket view (the optimiser's memory; AccumulateGrad adopts the tensor -- a parameter that already has a .grad, or needs
    # none, gets a fresh tensor from _sink_ex, which autograd adds into .grad or drops at once), or the weight gradient of an
    # effective weight of a weight-normalised layer (dw_flushed: consumed by the weight-norm node, which flushes first; the entry
    # then holds the tensor itself).  Any other weight -- a leaf that is no Parameter, a scaled, tied or otherwise computed
    # tensor -- is reduced inline: its consumer reads dw without flushing.  And never on a weight-gradient side
    # stream: the reader flushes ITS stream's entries.
    safe = (dw_view or dw_flushed) and db_view
    if (_PROFILER is None and _DEFERRED is not None and safe and nbytes <= DEFER_MAX_BYTES and (db is None or colsum_part is not None)
            and not _on_side_stream()):
        check(lib().wcmc_conv2d_wgrad_bf16x3(*args, 1, cs, terms, _stream()), "conv2d_wgrad_bf16x3")      # the GEMM now,
        st = torch.cuda.current_stream()                                                                 # the reduction later
        # (bucket views by ADDRESS: a reference held here would keep AccumulateGrad from adopting the tensor -- it would clone it, unreduced)
        _DEFERRED.setdefault(st.cuda_stream, (st, []))[1].append((ws, dw.data_ptr() if dw_view else dw, db.data_ptr() if db is not None else 0,
                                                                  colsum_part, n, ho, wo, cout, cin, ks, terms))
    elif _PROFILER is None:
        check(lib().wcmc_conv2d_wgrad_bf16x3(*args, 0, cs, terms, _stream()), "conv2d_wgrad_bf16x3")
    else:       # bracket the split-K GEMM launch alone; the slab reduce + bias gradient is its own class
        with _Timed(_wgrad_class(n, ho, cin, cout, ks), 2.0 * n * ho * wo * cout * cin * ks * ks, "flop"):
            check(lib().wcmc_conv2d_wgrad_bf16x3(*args, 1, cs, terms, _stream()), "conv2d_wgrad_bf16x3")
        with _Timed("conv_wgrad_finish", 0.0, "flop"):
            check(lib().wcmc_conv2d_wgrad_bf16x3(*args, 2, cs, terms, _stream()), "conv2d_wgrad_bf16x3")
    return dw, db


# The data gradient's activation gate comes from the 1-bit mask the forward launch left (1/16 of the bytes of re-reading the
# activation's hi plane; the predicate is the same, so results are bit-identical to gating on the activation).
#
# The bias gradient of a layer is the column sum of its dy.  The data-gradient GEMM that produces dy leaves per-tile column
# sums; the slab-reduction launch of the layer's weight gradient finishes them (wcmc_conv2d_wgrad_bf16x3, dy_colsum_partial)
# instead of a wcmc_colsum_finish launch per layer: ~55 launches less per step.


def _chainx_forward(ctx, xs0, dims0, spec, params, extra_saved=None):
    """Shared forward of the split-bf16 chains: xs0 is the chain input as a split tensor of dims0.  extra_saved: a
    callable y -> tensors saved behind the chain's own (a fused consumer of the chain's output)."""
    ks, pad, acts = spec[:3]
    # spec[3] (optional): the input channels [c0, c1) whose gradient the producer of x will read (``pbuffer_cat``: only the
    # P-buffer's mean carries gradient, 3 of KPCN's 39 input channels) -- the first layer's data gradient is then formed for
    # the 8-aligned range round them only
    ctx.dx_channels = spec[3] if len(spec) > 3 else None
    spec = tuple(spec[:3])
    nl = len(acts)
    n = dims0[0]
    dims = [dims0]
    xs = [xs0]
    masks = []
    y = None
    # the last two layers of a 1x1 chain in one launch where the library has a fused instance (PathNet.final:
    # 128 -> 128 -> 3): the hidden activation is written once and not re-read
    pair = (ks == 1 and pad == 0 and nl >= 2 and
            lib().wcmc_conv1x1_pair_supported(params[2 * nl - 4].shape[1], params[2 * nl - 4].shape[0],
                                              params[2 * nl - 2].shape[0]))
    ctx.terms = chain_terms(ks, dims0[1])          # the backward multiplies as the mode of ITS forward says
    oterms = _chain_out_terms(ks, acts[-1], params[2 * nl - 2].shape[1], params[2 * nl - 2].shape[0], pair)     # ("h": one fp16 MFMA)
    # (packing every chain of a sub-network AHEAD in one launch -- five U-Net chains, a KPCN branch before its PathNet runs -- was
    # built and measured in round 6: 10.93 -> 10.96 ms per step, same box, three alternations: the 16 pack launches of a step cost nothing)
    packs = _pack_chain_x([params[2 * l] for l in range(nl)], ks, oterms) if 2 * nl <= PACK_MAX_ENTRIES else None
    ctx.wp1 = [pk[1] for pk in packs] if packs is not None else None      # the data-gradient orientation, for the backward
    pack0 = (lambda l: packs[l][0]) if packs is not None else (lambda l: _pack_x(params[2 * l], _fwd_pack_mode(oterms) if l == nl - 1 else 0))
    for l in range(nl):
        wt, b = params[2 * l], params[2 * l + 1]
        cout = wt.shape[0]
        if wt.shape[1] != dims[l][1]:
            raise RuntimeError("conv chain layer %d: weight expects %d input channels, got a tensor with %d"
                               % (l, wt.shape[1], dims[l][1]))
        wp = pack0(l)
        hidden = l < nl - 1
        if pair and l == nl - 2:
            xs1, mask1, _, y = conv1x1_pair_x_raw(xs[l], dims[l], wp, b.detach(), cout, acts[l], pack0(l + 1),
                                                  params[2 * l + 3].detach(), params[2 * l + 2].shape[0], acts[l + 1])
            hh, ww = dims[l][2], dims[l][3]
            dims.append((n, cout, hh, ww))
            dims.append((n, params[2 * l + 2].shape[0], hh, ww))
            xs.append(xs1)
            masks.append(mask1)
            break
        if not hidden and oterms == "h":
            out = conv2d_out_f16_raw(xs[l], dims[l], wp, b.detach(), cout, ks, pad)
        else:
            out = conv2d_x_raw(xs[l], dims[l], wp, b.detach(), cout, ks, pad, acts[l], out_split=hidden, mask_out=hidden,
                               terms=3 if hidden else oterms)
        hh, ww = dims[l][2] + 2 * pad - ks + 1, dims[l][3] + 2 * pad - ks + 1
        dims.append((n, cout, hh, ww))
        if hidden:
            xs.append(out[0] if EMULATE_HIDDEN is None else EMULATE_HIDDEN(out[0], dims[-1], ks))
            masks.append(out[1])       # (hi > 0) bits of the hidden activation: the data gradient's ReLU gate
        else:
            y = out
    ctx.spec, ctx.dims = spec, dims
    ctx.bias_ptrs = [params[2 * l + 1].data_ptr() if isinstance(params[2 * l + 1], torch.nn.Parameter) else 0 for l in range(nl)]
    keep_y = [y] if acts[-1] != "linear" else []
    extra = tuple(extra_saved(y)) if extra_saved is not None else ()
    ctx.n_extra = len(extra)
    ctx.save_for_backward(*xs, *masks, *keep_y, *[params[2 * l] for l in range(nl)], *extra)
    if DEBUG_ACTS is not None:
        DEBUG_ACTS.extend(unsplit_debug(xs[l + 1], *dims[l + 1]) for l in range(nl - 1))
        if acts[-1] != "linear":
            DEBUG_ACTS.append(y)
    return y


def _chainx_backward(ctx, dy, need_dx, dys=None, part=None):
    """Shared backward: returns (dx as an fp32 NHWC view or None, [dw0, db0, dw1, db1, ...]).
    dys: the output gradient already as a split tensor (linear output layers only); part: its column-sum partials."""
    ks, pad, acts = ctx.spec
    dims = ctx.dims
    nl = len(acts)
    saved = ctx.saved_tensors
    xs = saved[:nl]
    masks = saved[nl:2 * nl - 1]
    off = 2 * nl - 1
    if dys is None:
        dy = _as_nhwc_nograd(dy)
        gated = acts[-1] != "linear"
        # split (output-activation backward folded in) + the last layer's bias-gradient partials in one pass over dy
        dys, part = split_dy_colsum_raw(dims[nl], dy=dy, post=saved[off] if gated else None, act=acts[-1])
        off += 1 if gated else 0
    else:
        assert acts[-1] == "linear"
    ws = saved[off:len(saved) - getattr(ctx, "n_extra", 0)]
    # part: per-tile column sums of dys when the launch that produced dys left them
    grads = [None] * (2 * nl)
    dx = None
    main = torch.cuda.current_stream()
    side = _side_stream(dys.device)
    keep = []
    wp1 = getattr(ctx, "wp1", None)
    wterms, dterms = ctx.terms
    bptrs = getattr(ctx, "bias_ptrs", None) or [0] * nl
    sink_of = lambda l: (ws[l].data_ptr() if isinstance(ws[l], torch.nn.Parameter) else 0, bptrs[l])
    flushed = [_flushed_by_consumer(w) for w in ws]
    pack1 = (lambda l: wp1[l]) if wp1 is not None else (lambda l: _pack_x(ws[l], _dgrad_mode(dterms)))
    for l in range(nl - 1, -1, -1):
        wt = ws[l]
        cout = wt.shape[0]
        if side is not None:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                dw, db = conv2d_wgrad_x_raw(xs[l], dims[l], dys, cout, ks, pad, wt.shape, want_bias=part is None,
                                            colsum_part=part, terms=wterms, sinks=sink_of(l), dw_flushed=flushed[l])
            dw.record_stream(main)
            db.record_stream(main)
            keep.append(dys)
            keep.append(part)
        else:
            dw, db = conv2d_wgrad_x_raw(xs[l], dims[l], dys, cout, ks, pad, wt.shape, want_bias=part is None,
                                        colsum_part=part, terms=wterms, sinks=sink_of(l), dw_flushed=flushed[l])
        grads[2 * l], grads[2 * l + 1] = dw, db
        if (l == 1 and need_dx and ks == 1 and pad == 0 and
                lib().wcmc_conv1x1_pair_supported(cout, wt.shape[1], ws[0].shape[1])):
            # the data gradients of layers 1 and 0 in one launch (PathNet.final: 3 -> 128 -> 128): the 128-channel
            # gradient of the hidden activation is written once (the weight gradient of layer 0 reads it) and feeds
            # the second GEMM from LDS
            dys, _, part, dx = conv1x1_pair_x_raw(dys, dims[2], pack1(1), None, wt.shape[1], "linear",
                                                  pack1(0), None, ws[0].shape[1], "linear",
                                                  gate_mask=masks[0], gate_act=acts[0], colsum=True, mask_out=False)
        elif l > 0:
            wpt = pack1(l)
            dys, part = conv2d_x_raw(dys, dims[l + 1], wpt, None, wt.shape[1], ks, ks - 1 - pad, "linear",
                                     out_split=True, gate_act=acts[l - 1], colsum=True, terms=dterms, gate_mask=masks[l - 1])
        elif need_dx and dx is None:
            sub = getattr(ctx, "dx_channels", None)
            if sub is not None and (sub[1] + 7) // 8 * 8 - sub[0] // 8 * 8 <= wt.shape[1] // 2:
                # the consumer reads channels [c0, c1) only: a GEMM over the 8-aligned rows round them (KPCN's first layer: 16 of
                # 48 padded rows, one cout tile instead of four); the rest of dx is zero, never read
                a0, a1 = sub[0] // 8 * 8, min((sub[1] + 7) // 8 * 8, wt.shape[1])
                nn_, _, hh_, ww_ = dims[0]
                dx = nhwc_empty(nn_, wt.shape[1], hh_, ww_, dys.device, zero=True)
                wsub = _pack_x(wt.detach()[:, a0:a1].contiguous(), _dgrad_mode(dterms))
                conv2d_x_raw(dys, dims[l + 1], wsub, None, a1 - a0, ks, ks - 1 - pad, "linear", out_split=False, terms=dterms,
                             out=dx[:, a0:a1])
            else:
                wpt = pack1(l)
                dx = conv2d_x_raw(dys, dims[l + 1], wpt, None, wt.shape[1], ks, ks - 1 - pad, "linear",
                                  out_split=False, terms=dterms)
    if side is not None:
        main.wait_stream(side)
    del keep
    return dx, grads


class _ConvChainX(torch.autograd.Function):
    """``_ConvChain`` on the split-bf16 GEMMs: intermediates live as split tensors (same bytes as
    fp32), only the chain's input and output are fp32 NHWC views."""

    @staticmethod
    def forward(ctx, x, spec, *params):
        _need_cuda(x, *params)
        return _chainx_forward(ctx, split_raw(x), tuple(x.shape), spec, params)

    @staticmethod
    def backward(ctx, dy):
        dx, grads = _chainx_backward(ctx, dy, ctx.needs_input_grad[0])
        return (dx, None, *grads)


def _split_shared(x):
    """split_raw, remembered ON the tensor object: the two PathNets embed the SAME converted ``paths`` tensor
    (interfaces.py:195-196; PathNet._paths_nhwc keeps that object in the batch dictionary for one step), so its
    168 MB split is made once per step.  Valid for the version and stream it was made on."""
    tag = (x._version, torch.cuda.current_stream().cuda_stream)
    cached = getattr(x, "_wcmc_split", None)
    if cached is not None and cached[0] == tag:
        return cached[1]
    if cached is not None and cached[0] == (x._version, None):      # presplit_shared: made before the streams forked
        cached[1].record_stream(torch.cuda.current_stream())
        return cached[1]
    xs = split_raw(x)
    if not x.requires_grad:
        x._wcmc_split = (tag, xs)
    return xs


class _ChainSppMeanX(torch.autograd.Function):
    """``y = chain(x); m = y.view(B,S,...).mean(1)`` (networks.py:33-36) as one node.  y feeds the concatenation
    and m the U-Net, so y's gradient is ``g_y + repeat_S(g_m) / S``: formed once, directly as the split dy of
    the chain's backward (``wcmc_add_broadcast_split``) instead of broadcast + add + split."""

    @staticmethod
    def forward(ctx, x, s, spec, *params):
        _need_cuda(x, *params)
        assert spec[2][-1] == "linear"
        y = _chainx_forward(ctx, _split_shared(x), tuple(x.shape), spec, params)
        bs, c, h, w = y.shape
        m = nhwc_empty(bs // s, c, h, w, y.device)
        check(lib().wcmc_spp_reduce(*_v(y), *_v(m), bs // s, s, h, w, c, 1.0 / s, _stream()), "spp_reduce")
        ctx.s = s
        return y, m

    @staticmethod
    def backward(ctx, gy, gm):
        s = ctx.s
        bs, c, h, w = ctx.dims[-1]
        gy = _as_nhwc_nograd(gy) if gy is not None else None
        gm = _as_nhwc_nograd(gm) if gm is not None else None
        dev = (gy if gy is not None else gm).device
        dys, part = split_dy_colsum_raw((bs, c, h, w), dy=gy, gm=gm, s=s, scale=1.0 / s)
        dx, grads = _chainx_backward(ctx, None, ctx.needs_input_grad[0], dys=dys, part=part)
        return (dx, None, None, *grads)


# PathNet.embedding as one launch per direction (csrc/pathnet_fused.hip): hidden activations stay on chip in the forward and
# are recomputed in the backward.  Default mode only (its backward arithmetic is built in); WCMC_FUSE_EMBED=0: A/B switch.
FUSE_EMBED = os.environ.get("WCMC_FUSE_EMBED", "1") != "0"


def _dense_pixel_stride(g):
    """Pixel stride (floats) of an NHWC view whose pixels form one dense run (rows and images back to back), else None."""
    n, c, h, w = g.shape
    sn, sc, sh, sw = g.stride()
    if sc == 1 and sw >= c and sw % 4 == 0 and sh == w * sw and (n == 1 or sn == h * sh) and g.data_ptr() % 16 == 0:
        return sw
    return None


class _EmbedSppMeanFusedX(torch.autograd.Function):
    """``y = chain3(x); m = y.view(B,S,...).mean(1)`` (networks.py:33-36) with the three 1x1 layers in ONE launch
    (``wcmc_embed3_fwd``) and a backward that recomputes the hidden activations (``wcmc_embed3_bwd``): nothing but x, y and
    the two gradients of y ever touches HBM."""

    @staticmethod
    def forward(ctx, x, s, *params):
        _need_cuda(x, *params)
        xs = _split_shared(x)
        n, cin, h, w = x.shape
        ws_ = [params[0], params[2], params[4]]
        packs = _pack_chain_x(ws_, 1)                        # [(forward, data-gradient orientation)] per layer
        y = torch.empty((n, h, w, 64), device=x.device, dtype=torch.float32).permute(0, 3, 1, 2)
        m = nhwc_empty(n // s, 64, h, w, y.device)
        wb = (_ptr(packs[0][0]), _ptr(params[1].detach()), _ptr(packs[1][0]), _ptr(params[3].detach()), _ptr(packs[2][0]),
              _ptr(params[5].detach()))
        if lib().wcmc_embed3_mean_supported(s, h * w):
            # the mean leaves with y (the kernel walks the S samples of a pixel tile and keeps their sum in registers)
            with _Timed("embed3_fwd", 4.0 * n * h * w * ((cin + 7) // 8 * 8 + 64 + 64 // s), "byte"):
                check(lib().wcmc_embed3_mean_fwd(_ptr(xs), n * h * w, cin, *wb, _ptr(y), _ptr(m), s, h * w, _stream()), "embed3_mean_fwd")
        else:
            with _Timed("embed3_fwd", 4.0 * n * h * w * ((cin + 7) // 8 * 8 + 64), "byte"):
                check(lib().wcmc_embed3_fwd(_ptr(xs), n * h * w, cin, *wb, _ptr(y), _stream()), "embed3_fwd")
            check(lib().wcmc_spp_reduce(*_v(y), *_v(m), n // s, s, h, w, 64, 1.0 / s, _stream()), "spp_reduce")
        ctx.s, ctx.dims = s, (n, cin, h, w)
        ctx.packs = packs
        ctx.save_for_backward(xs, *params)
        return y, m

    @staticmethod
    def backward(ctx, gy, gm):
        s = ctx.s
        n, cin, h, w = ctx.dims
        xs, w0, b0, w1, b1, w2, b2 = ctx.saved_tensors
        gy = _as_nhwc_nograd(gy) if gy is not None else None
        gm = _as_nhwc_nograd(gm) if gm is not None else None
        if gy is not None and _dense_pixel_stride(gy) is None:
            gy = to_nhwc_raw(gy)
        if gm is not None and _dense_pixel_stride(gm) is None:
            gm = to_nhwc_raw(gm)
        dev = xs.device
        sk = lambda t: _sink(t.data_ptr() if isinstance(t, torch.nn.Parameter) else 0, t.shape, dev)
        dw0, dw1, dw2, db0, db1, db2 = sk(w0), sk(w1), sk(w2), sk(b0), sk(b1), sk(b2)
        nb = lib().wcmc_embed3_bwd_workspace_bytes()
        ws = torch.empty(nb // 4, device=dev, dtype=torch.float32)
        packs = ctx.packs
        with _Timed("embed3_bwd", 4.0 * n * h * w * ((cin + 7) // 8 * 8 + 64 + (64 // s if gm is not None else 0)), "byte"):
            check(lib().wcmc_embed3_bwd(_ptr(xs), n * h * w, cin, _ptr(packs[0][0]), _ptr(b0), _ptr(packs[1][0]), _ptr(b1),
                                        _ptr(packs[1][1]), _ptr(packs[2][1]), _ptr(gy), _dense_pixel_stride(gy) if gy is not None else 0,
                                        _ptr(gm), _dense_pixel_stride(gm) if gm is not None else 0, s, h * w, 1.0 / s,
                                        _ptr(dw0), _ptr(db0), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(ws), nb, _stream()),
                  "embed3_bwd")
        return (None, None, dw0, db0, dw1, db1, dw2, db2)


class _FinalFusedX(torch.autograd.Function):
    """``chain2(cat([flat, repeat_S(prop)], 1))`` (networks.py:39-42) as one launch per direction (``wcmc_final2_*``): neither
    the 128-channel concatenation nor the hidden activation is written; the backward recomputes them."""

    @staticmethod
    def forward(ctx, flat, prop, s, *params):
        _need_cuda(flat, prop, *params)
        bs, c1, h, w = flat.shape
        b = prop.shape[0]
        outc = params[2].shape[0]
        packs = _pack_chain_x([params[0], params[2]], 1)
        osz = 4 if outc <= 4 else 8                           # pixel stride of the output: round_up(outc, 4)
        buf = torch.empty((bs, h, w, osz), device=flat.device, dtype=torch.float32)
        with _Timed("final2_fwd", 4.0 * bs * h * w * (64 + 64 // s + osz), "byte"):
            check(lib().wcmc_final2_fwd(_ptr(flat), _dense_pixel_stride(flat), _ptr(prop), _dense_pixel_stride(prop), b, s, h * w,
                                        _ptr(packs[0][0]), _ptr(params[1].detach()), _ptr(packs[1][0]), _ptr(params[3].detach()), outc,
                                        _ptr(buf), _stream()), "final2_fwd")
        ctx.geom, ctx.packs = (b, s, h, w, outc), packs
        ctx.save_for_backward(flat, prop, *params)
        return buf.permute(0, 3, 1, 2)[:, :outc]

    @staticmethod
    def backward(ctx, g):
        b, s, h, w, outc = ctx.geom
        flat, prop, w0, b0, w1, b1 = ctx.saved_tensors
        g = _as_nhwc_nograd(g)
        osz = 4 if outc <= 4 else 8
        if not (_dense_pixel_stride(g) == osz):
            g = to_nhwc_raw(g)
        dev = flat.device
        dy = torch.empty((b * s, h, w, 64), device=dev, dtype=torch.float32).permute(0, 3, 1, 2)
        dprop = nhwc_empty(b, 64, h, w, dev)
        sk = lambda t: _sink(t.data_ptr() if isinstance(t, torch.nn.Parameter) else 0, t.shape, dev)
        dw0, dw1, db0, db1 = sk(w0), sk(w1), sk(b0), sk(b1)
        nb = lib().wcmc_final2_bwd_workspace_bytes()
        ws = torch.empty(nb // 4, device=dev, dtype=torch.float32)
        packs = ctx.packs
        with _Timed("final2_bwd", 4.0 * b * s * h * w * (64 + 64 // s + osz + 64 + 64 // s), "byte"):
            check(lib().wcmc_final2_bwd(_ptr(flat), _dense_pixel_stride(flat), _ptr(prop), _dense_pixel_stride(prop), b, s, h * w,
                                        _ptr(packs[0][0]), _ptr(b0), _ptr(packs[1][0]), _ptr(b1), outc, _ptr(packs[0][1]), _ptr(packs[1][1]),
                                        _ptr(g), _ptr(dy), _ptr(dprop), _ptr(dw0), _ptr(db0), _ptr(dw1), _ptr(db1), _ptr(ws), nb,
                                        _stream()), "final2_bwd")
        return (dy if ctx.needs_input_grad[0] else None, dprop if ctx.needs_input_grad[1] else None, None, dw0, db0, dw1, db1)


# WCMC_FUSE_FINAL=0: A/B switch back to concatenation + fused layer pair (csrc/pathnet_fused.hip; default mode only)
FUSE_FINAL = os.environ.get("WCMC_FUSE_FINAL", "1") != "0"


class _CatBroadcastChainX(torch.autograd.Function):
    """``chain(cat([flat, repeat_S(prop)], 1))`` (networks.py:39-42) with the concatenation written once,
    directly as the chain's split input (``wcmc_cat_broadcast_split``); the backward splits the chain's
    input gradient into the per-sample half (a view) and the spp-summed half."""

    @staticmethod
    def forward(ctx, flat, prop, s, spec, *params):
        _need_cuda(flat, prop, *params)
        bs, c1, h, w = flat.shape
        b, c2 = prop.shape[0], prop.shape[1]
        assert bs == b * s and c1 % 8 == 0 and prop.shape[2:] == flat.shape[2:]
        xs0 = _split_empty(bs, c1 + c2, h, w, flat.device)
        check(lib().wcmc_cat_broadcast_split(*_v(flat), *_v(prop), _ptr(xs0), b, s, h, w, c1, c2, _stream()),
              "cat_broadcast_split")
        ctx.cat = (b, s, c1, c2)
        return _chainx_forward(ctx, xs0, (bs, c1 + c2, h, w), spec, params)

    @staticmethod
    def backward(ctx, dy):
        b, s, c1, c2 = ctx.cat
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dx, grads = _chainx_backward(ctx, dy, need)
        dflat = dprop = None
        if need:
            _, _, h, w = dx.shape
            dflat = dx[:, :c1]
            if s == 1:                               # plain concatenation: both halves are views
                dprop = dx[:, c1:]
            else:
                dprop = nhwc_empty(b, c2, h, w, dx.device)
                check(lib().wcmc_spp_reduce(*_v(dx[:, c1:]), *_v(dprop), b, s, h, w, c2, 1.0, _stream()), "spp_reduce")
        return (dflat, dprop, None, None, *grads)


class _CatUpsampleChainX(torch.autograd.Function):
    """``chain(cat([upsample2(deep), skip], 1))`` (a U-Net level's right chain) with the bilinear upsampling evaluated
    inside the concatenation kernel (``wcmc_cat_upsample_split``): the upsampled tensor is never written; the
    backward is the chain's, then ``upsample2``'s on the first channels of its input gradient."""

    @staticmethod
    def forward(ctx, deep, skip, spec, *params):
        _need_cuda(deep, skip, *params)
        n, c1, hd, wd = deep.shape
        c2, h, w = skip.shape[1:]
        assert skip.shape[0] == n and h == 2 * hd and w == 2 * wd and c1 % 8 == 0
        xs0 = _split_empty(n, c1 + c2, h, w, deep.device)
        check(lib().wcmc_cat_upsample_split(*_v(deep), *_v(skip), _ptr(xs0), n, h, w, c1, c2, _stream()), "cat_upsample_split")
        ctx.cat = (n, c1, c2, h, w)
        return _chainx_forward(ctx, xs0, (n, c1 + c2, h, w), spec, params)

    @staticmethod
    def backward(ctx, dy):
        n, c1, c2, h, w = ctx.cat
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dx, grads = _chainx_backward(ctx, dy, need)
        ddeep = dskip = None
        if need:
            g = dx[:, :c1]
            ddeep = nhwc_empty(n, c1, h // 2, w // 2, dx.device)
            check(lib().wcmc_upsample2_bwd(*_v(g), *_v(ddeep), n, h // 2, w // 2, c1, _stream()), "upsample2_bwd")
            dskip = dx[:, c1:]
        return (ddeep, dskip, None, *grads)


def cat_upsample_chain(deep, skip, ksize, pad, acts, params):
    """``conv_chain(cat([upsample2(deep), skip], 1), ...)``; one autograd node on the split-bf16 path."""
    if split_path() and deep.shape[1] % 8 == 0:
        return _CatUpsampleChainX.apply(as_nhwc(deep), as_nhwc(skip), (ksize, pad, tuple(acts)), *params)
    return cat_broadcast_chain(upsample2(deep), skip, 1, ksize, pad, acts, params)


def conv_chain(x, ksize, pad, acts, params):
    if not split_path():
        return _ConvChain.apply(as_nhwc(x), (ksize, pad, tuple(acts)), *params)
    hint = getattr(x, "_wcmc_grad_channels", None)          # left by pbuffer_cat on its output
    spec = (ksize, pad, tuple(acts)) + ((tuple(hint),) if hint is not None else ())
    return _ConvChainX.apply(as_nhwc(x), spec, *params)


_UNFUSED_NOTED = set()


def _note_unfused(what, why):
    """A fused PathNet chain exists for the reference's shapes (support/networks.py:18-24) in the reduced-backward modes; another
    shape or mode runs the same arithmetic layer by layer in HIP -- correct, slower -- and says so once."""
    if (what, why) not in _UNFUSED_NOTED:
        _UNFUSED_NOTED.add((what, why))
        import warnings
        warnings.warn("wcmc_amd: %s runs layer by layer (no fused kernel for %s)" % (what, why), RuntimeWarning, stacklevel=3)


def conv_chain_spp_mean(x, s, ksize, pad, acts, params):
    """``y = conv_chain(x, ...); return y, spp_mean(y, s)``; one autograd node on the split-bf16 path."""
    # (DEBUG_ACTS: the parity tests' hook wants the hidden activations, which the fused chain never materialises)
    if (FUSE_EMBED and DEBUG_ACTS is None and ksize == 1 and pad == 0 and len(acts) == 3 and
            tuple(acts) == ("relu", "relu", "linear") and not x.requires_grad and x.is_cuda):
        if not reduced_backward():
            _note_unfused("PathNet.embedding", "precision mode %s" % PRECISION)
        elif not lib().wcmc_embed3_supported(params[0].shape[1], params[0].shape[0], params[2].shape[0], params[4].shape[0]):
            _note_unfused("PathNet.embedding", "channels %d -> %d -> %d -> %d" % (params[0].shape[1], params[0].shape[0],
                                                                                 params[2].shape[0], params[4].shape[0]))
        elif getattr(x, "_wcmc_split", None) is not None or is_nhwc_view(x):
            return _EmbedSppMeanFusedX.apply(x, s, *params)
    if split_path() and acts[-1] == "linear":
        pre = getattr(x, "_wcmc_split", None)
        if pre is not None and pre[0] == (x._version, None) and not x.requires_grad:
            return _ChainSppMeanX.apply(x, s, (ksize, pad, tuple(acts)), *params)      # channel-first x, split attached
        return _ChainSppMeanX.apply(as_nhwc(x), s, (ksize, pad, tuple(acts)), *params)
    y = conv_chain(x, ksize, pad, acts, params)
    return y, spp_mean(y, s)


def cat_broadcast_chain(flat, prop, s, ksize, pad, acts, params):
    """``conv_chain(cat_broadcast(flat, prop, s), ...)``; fused into one autograd node on the split-bf16 path."""
    if (FUSE_FINAL and DEBUG_ACTS is None and ksize == 1 and pad == 0 and
            tuple(acts) == ("relu", "relu") and flat.is_cuda and prop.shape[0] * s == flat.shape[0]):
        if not reduced_backward():
            _note_unfused("PathNet.final", "precision mode %s" % PRECISION)
        elif not (lib().wcmc_final2_supported(flat.shape[1], prop.shape[1], params[0].shape[0], params[2].shape[0],
                                             flat.shape[2] * flat.shape[3]) and params[0].shape[1] == 128):
            _note_unfused("PathNet.final", "channels %d + %d -> %d -> %d at %d pixels per image" %
                          (flat.shape[1], prop.shape[1], params[0].shape[0], params[2].shape[0], flat.shape[2] * flat.shape[3]))
        else:
            fl, pr = as_nhwc(flat), as_nhwc(prop)
            if _dense_pixel_stride(fl) is not None and _dense_pixel_stride(pr) is not None:
                return _FinalFusedX.apply(fl, pr, s, *params)
    if split_path() and flat.shape[1] % 8 == 0:
        return _CatBroadcastChainX.apply(as_nhwc(flat), as_nhwc(prop), s, (ksize, pad, tuple(acts)), *params)
    return conv_chain(cat_broadcast(flat, prop, s), ksize, pad, acts, params)


# ------------------------------------------------------------------------ kernel apply
class _KernelApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, logits):
        _need_cuda(data, logits)
        n, k2, h, w = logits.shape
        k = int(round(k2 ** 0.5))
        c = data.shape[1]
        assert k * k == k2 and data.shape[0] == n and data.shape[2:] == logits.shape[2:]
        out = torch.empty((n, c, h, w), device=logits.device, dtype=torch.float32)
        lse = torch.empty(n * h * w, device=logits.device, dtype=torch.float32)
        # algorithmic bytes: logits + radiance in + result out (15.13 MB per 92x92 patch-branch)
        with _Timed("kernel_apply_fwd", 4.0 * n * h * w * (k2 + 2 * c), "byte"):
            check(lib().wcmc_kernel_apply_fwd(*_v(logits), _ptr(data), *data.stride(), _ptr(out), *out.stride(),
                                              _ptr(lse), n, c, h, w, k, _stream()), "kernel_apply_fwd")
        ctx.save_for_backward(data, logits, out, lse)
        ctx.k = k
        return out

    @staticmethod
    def backward(ctx, g):
        data, logits, out, lse = ctx.saved_tensors
        n, k2, h, w = logits.shape
        c = data.shape[1]
        dl = nhwc_empty(n, k2, h, w, logits.device)
        dd = torch.zeros((n, c, h, w), device=logits.device, dtype=torch.float32) \
            if ctx.needs_input_grad[0] else None
        # algorithmic bytes: logits in + d_logits out + radiance, result and its gradient in (30.06 MB / patch-branch)
        with _Timed("kernel_apply_bwd", 4.0 * n * h * w * (2 * k2 + 3 * c), "byte"):
            check(lib().wcmc_kernel_apply_bwd(*_v(logits), _ptr(data), *data.stride(), _ptr(out), *out.stride(),
                                              _ptr(g), *g.stride(), _ptr(lse), *_v(dl), _ptr(dd),
                                              n, c, h, w, ctx.k, _stream()), "kernel_apply_bwd")
        return dd, dl


def kernel_apply(data, logits):
    """softmax(k*k logits) applied as a zero-extended gather kernel over ``data``."""
    return _KernelApply.apply(data, as_nhwc(logits))


def chain_kernel_apply(x, data, ksize, pad, acts, params):
    """``kernel_apply(data, conv_chain(x, ...))`` with ``data`` already cropped to the chain's output size.  (Round 2 also had
    the two as ONE autograd node whose backward wrote d_logits straight into the chain's split gradient; it measured neutral
    -- 369-371 patches/s either way -- and was removed in round 3.)"""
    return kernel_apply(data, conv_chain(x, ksize, pad, acts, params))


class _Recombine(torch.autograd.Function):
    """radiance = albedo * r_diffuse + exp(r_specular) - 1 (albedo is data: no gradient)."""

    @staticmethod
    def forward(ctx, albedo, r_d, r_s):
        _need_cuda(albedo, r_d, r_s)
        n, c, h, w = r_d.shape
        out = torch.empty((n, c, h, w), device=r_d.device, dtype=torch.float32)
        check(lib().wcmc_recombine_fwd(_ptr(albedo), *albedo.stride(), _ptr(r_d), *r_d.stride(), _ptr(r_s),
                                       *r_s.stride(), _ptr(out), n, c, h, w, _stream()), "recombine_fwd")
        ctx.save_for_backward(albedo, r_s)
        return out

    @staticmethod
    def backward(ctx, g):
        albedo, r_s = ctx.saved_tensors
        n, c, h, w = r_s.shape
        g = g.contiguous()
        dd = torch.empty((n, c, h, w), device=g.device, dtype=torch.float32)
        ds = torch.empty((n, c, h, w), device=g.device, dtype=torch.float32)
        check(lib().wcmc_recombine_bwd(_ptr(g), _ptr(albedo), *albedo.stride(), _ptr(r_s), *r_s.stride(), _ptr(dd),
                                       _ptr(ds), n, c, h, w, _stream()), "recombine_bwd")
        return None, dd, ds


def recombine(albedo, r_diffuse, r_specular):
    return _Recombine.apply(albedo, r_diffuse, r_specular)


# ------------------------------------------------------------------------ image losses
def _image_loss_raw(x, ref, eps, want_l1, want_rel):
    _need_cuda(x, ref)
    assert x.shape == ref.shape and x.dim() == 4, (x.shape, ref.shape)
    n, c, h, w = x.shape
    ws = torch.empty(lib().wcmc_image_loss_workspace_bytes() // 4, device=x.device, dtype=torch.float32)
    l1 = torch.empty((), device=x.device, dtype=torch.float32) if want_l1 else None
    rel = torch.empty((), device=x.device, dtype=torch.float32) if want_rel else None
    check(lib().wcmc_image_loss_fwd(_ptr(x), *x.stride(), _ptr(ref), *ref.stride(), float(eps), _ptr(l1), _ptr(rel), _ptr(ws),
                                    ws.numel() * 4, n, c, h, w, _stream()), "image_loss_fwd")
    return l1, rel


class _L1Mean(torch.autograd.Function):
    """``torch.nn.L1Loss()(x, ref)`` (mean reduction; ref carries no gradient) as one pass + a one-block finish; the
    backward is one launch: ``g * sign(x - ref) / numel``."""

    @staticmethod
    def forward(ctx, x, ref):
        l1, _ = _image_loss_raw(x, ref, 0.0, True, False)
        ctx.save_for_backward(x, ref)
        return l1

    @staticmethod
    def backward(ctx, g):
        x, ref = ctx.saved_tensors
        n, c, h, w = x.shape
        dx = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
        g = g.contiguous()
        check(lib().wcmc_l1_mean_bwd(_ptr(x), *x.stride(), _ptr(ref), *ref.stride(), _ptr(g), _ptr(dx), n, c, h, w, _stream()),
              "l1_mean_bwd")
        return dx, None


def l1_mean(x, ref):
    """mean |x - ref| of two (N,C,H,W) tensors (any strides); differentiable in x."""
    return _L1Mean.apply(x, ref.detach())


def image_metrics(x, ref, eps=1e-2):
    """(L1 mean, RelativeMSE) of x against ref in one pass, no gradient (the logged ``l_total`` and ``rmse`` of a step,
    ``interfaces.py:240-249``)."""
    return _image_loss_raw(x.detach(), ref.detach(), eps, True, True)


def relative_mse(x, ref, eps=1e-2):
    """``support.losses.RelativeMSE`` without a gradient (validation, ``interfaces.py:296-300``)."""
    return _image_loss_raw(x.detach(), ref.detach(), eps, False, True)[1]


LOSS2_KINDS = {"smape": 0, "tonemapped_mse": 1, "tonemapped_relative_mse": 2}


class _ImageLoss2(torch.autograd.Function):
    """SMAPE / TonemappedMSE / TonemappedRelativeMSE (support/losses.py:267-320) of an (N,C,H,W) pair: one HIP pass + a one-block
    finish forward (``wcmc_image_loss2_fwd``), one pass backward (``wcmc_image_loss2_bwd``); ref carries no gradient."""

    @staticmethod
    def forward(ctx, x, ref, kind, eps):
        _need_cuda(x, ref)
        assert x.shape == ref.shape and x.dim() == 4, (x.shape, ref.shape)
        n, c, h, w = x.shape
        ws = torch.empty(lib().wcmc_image_loss_workspace_bytes() // 4, device=x.device, dtype=torch.float32)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        check(lib().wcmc_image_loss2_fwd(kind, _ptr(x), *x.stride(), _ptr(ref), *ref.stride(), float(eps), _ptr(loss), _ptr(ws),
                                         ws.numel() * 4, n, c, h, w, _stream()), "image_loss2_fwd")
        ctx.save_for_backward(x, ref)
        ctx.kind, ctx.eps = kind, float(eps)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, ref = ctx.saved_tensors
        n, c, h, w = x.shape
        dx = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
        g = g.contiguous()
        check(lib().wcmc_image_loss2_bwd(ctx.kind, _ptr(x), *x.stride(), _ptr(ref), *ref.stride(), ctx.eps, _ptr(g), _ptr(dx),
                                         n, c, h, w, _stream()), "image_loss2_bwd")
        return dx, None, None, None


def image_loss2(x, ref, kind, eps=1e-2):
    """kind: 'smape' | 'tonemapped_mse' | 'tonemapped_relative_mse'; differentiable in x."""
    return _ImageLoss2.apply(x, ref.detach(), LOSS2_KINDS[kind], eps)


def clip_grad_norm_(parameters, max_norm):
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (interfaces.py:454-458, 826-833) as three HIP launches per 96
    gradient tensors (``wcmc_grad_norm_clip``); returns the total norm before clipping as a 0-d device tensor."""
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros(())
    _need_cuda(*grads)
    grads = [g if g.is_contiguous() else None for g in grads]
    if any(g is None for g in grads):
        raise RuntimeError("clip_grad_norm_: gradients must be contiguous")
    if len(grads) > 96:
        # (more tensors than one table holds: norms of the groups first, then one common factor -- not needed by any model here)
        raise NotImplementedError("clip_grad_norm_: more than 96 gradient tensors")
    m = len(grads)
    numel = (ctypes.c_int64 * m)(*[g.numel() for g in grads])
    nbytes = lib().wcmc_grad_norm_clip_workspace_bytes(m, numel)
    ws = torch.empty((nbytes + 3) // 4, device=grads[0].device, dtype=torch.float32)
    out = torch.empty(2, device=grads[0].device, dtype=torch.float32)
    check(lib().wcmc_grad_norm_clip(m, (ctypes.c_void_p * m)(*[g.data_ptr() for g in grads]), numel, float(max_norm), _ptr(out),
                                    _ptr(ws), ws.numel() * 4, _stream()), "grad_norm_clip")
    return out[0]


# ------------------------------------------------------------------------ U-Net glue
class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, c, h, w = x.shape
        y = nhwc_empty(n, c, h // 2, w // 2, x.device)
        check(lib().wcmc_maxpool2_fwd(*_v(x), *_v(y), n, h, w, c, _stream()), "maxpool2_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        g = _as_nhwc_nograd(g)
        dx = nhwc_empty(n, c, h, w, x.device)
        check(lib().wcmc_maxpool2_bwd(*_v(x), *_v(g), *_v(dx), n, h, w, c, _stream()), "maxpool2_bwd")
        return dx


class _MaxPool2Skip(torch.autograd.Function):
    """``(x, maxpool2(x))`` as ONE node (a U-Net level: x feeds the skip connection, its pooled copy the level below): the two
    gradients of x arrive together and are summed inside the pooling backward's pass (``wcmc_maxpool2_bwd_add``) instead of by
    autograd's elementwise add -- one launch and one pass over the tensor less per level."""

    @staticmethod
    def forward(ctx, x):
        n, c, h, w = x.shape
        y = nhwc_empty(n, c, h // 2, w // 2, x.device)
        check(lib().wcmc_maxpool2_fwd(*_v(x), *_v(y), n, h, w, c, _stream()), "maxpool2_fwd")
        ctx.save_for_backward(x)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, g_skip, g_pool):
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        if g_pool is None:
            return g_skip
        g_pool = _as_nhwc_nograd(g_pool)
        dx = nhwc_empty(n, c, h, w, x.device)
        if g_skip is None:
            check(lib().wcmc_maxpool2_bwd(*_v(x), *_v(g_pool), *_v(dx), n, h, w, c, _stream()), "maxpool2_bwd")
        else:
            g_skip = _as_nhwc_nograd(g_skip)
            check(lib().wcmc_maxpool2_bwd_add(*_v(x), *_v(g_pool), *_v(g_skip), *_v(dx), n, h, w, c, _stream()), "maxpool2_bwd_add")
        return dx


def maxpool2_skip(x):
    """``(x, maxpool2(x))``: see ``_MaxPool2Skip``."""
    return _MaxPool2Skip.apply(as_nhwc(x))


class _Upsample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, c, h, w = x.shape
        y = nhwc_empty(n, c, 2 * h, 2 * w, x.device)
        check(lib().wcmc_upsample2_fwd(*_v(x), *_v(y), n, h, w, c, _stream()), "upsample2_fwd")
        return y

    @staticmethod
    def backward(ctx, g):
        n, c, h2, w2 = g.shape
        g = _as_nhwc_nograd(g)
        dx = nhwc_empty(n, c, h2 // 2, w2 // 2, g.device)
        check(lib().wcmc_upsample2_bwd(*_v(g), *_v(dx), n, h2 // 2, w2 // 2, c, _stream()), "upsample2_bwd")
        return dx


def maxpool2(x):
    return _MaxPool2.apply(as_nhwc(x))


def upsample2(x):
    return _Upsample2.apply(as_nhwc(x))


class _CatChannels(torch.autograd.Function):
    """cat([a, b], 1) into one NHWC buffer (channel counts multiples of 4); backward = two views."""

    @staticmethod
    def forward(ctx, a, b):
        n, ca, h, w = a.shape
        cb = b.shape[1]
        assert ca % 4 == 0, "concat offset must keep 16-byte alignment"
        out = nhwc_empty(n, ca + cb, h, w, a.device)
        out[:, :ca].copy_(a)      # strided device copies (plumbing, no arithmetic)
        out[:, ca:].copy_(b)
        ctx.ca = ca
        return out

    @staticmethod
    def backward(ctx, g):
        g = _as_nhwc_nograd(g)
        return g[:, :ctx.ca], g[:, ctx.ca:]


def cat_channels(a, b):
    return _CatChannels.apply(as_nhwc(a), as_nhwc(b))


# ------------------------------------------------------------------------ PathNet glue
class _SppMean(torch.autograd.Function):
    """(B*S,C,H,W) -> (B,C,H,W): mean over the S samples of a patch (networks.py:35-36)."""

    @staticmethod
    def forward(ctx, x, s):
        bs, c, h, w = x.shape
        b = bs // s
        y = nhwc_empty(b, c, h, w, x.device)
        check(lib().wcmc_spp_reduce(*_v(x), *_v(y), b, s, h, w, c, 1.0 / s, _stream()), "spp_reduce")
        ctx.s = s
        return y

    @staticmethod
    def backward(ctx, g):
        g = _as_nhwc_nograd(g)
        b, c, h, w = g.shape
        dx = nhwc_empty(b * ctx.s, c, h, w, g.device)
        check(lib().wcmc_spp_broadcast(*_v(g), *_v(dx), b, ctx.s, h, w, c, 1.0 / ctx.s, 0, _stream()),
              "spp_broadcast")
        return dx, None


def spp_mean(x, s):
    return _SppMean.apply(as_nhwc(x), s)


class _CatBroadcast(torch.autograd.Function):
    """cat([flat (B*S,C1), repeat_S(ctx (B,C2))], 1) without materialising the repeat twice
    (networks.py:39-40)."""

    @staticmethod
    def forward(ctx, flat, prop, s):
        bs, c1, h, w = flat.shape
        b, c2 = prop.shape[0], prop.shape[1]
        assert c1 % 4 == 0 and bs == b * s
        out = nhwc_empty(bs, c1 + c2, h, w, flat.device)
        out[:, :c1].copy_(flat)
        check(lib().wcmc_spp_broadcast(*_v(prop), *_v(out[:, c1:]), b, s, h, w, c2, 1.0, 0, _stream()),
              "spp_broadcast")
        ctx.dims = (b, s, c1, c2)
        return out

    @staticmethod
    def backward(ctx, g):
        b, s, c1, c2 = ctx.dims
        g = _as_nhwc_nograd(g)
        _, _, h, w = g.shape
        dprop = nhwc_empty(b, c2, h, w, g.device)
        check(lib().wcmc_spp_reduce(*_v(g[:, c1:]), *_v(dprop), b, s, h, w, c2, 1.0, _stream()), "spp_reduce")
        return g[:, :c1], dprop, None


def cat_broadcast(flat, prop, s):
    return _CatBroadcast.apply(as_nhwc(flat), as_nhwc(prop), s)


# ------------------------------------------------------------------------ interface glue
class _PBufferCat(torch.autograd.Function):
    """cat([base, P.mean(1), P.var(1).mean(1,keepdim).detach()/S], 1)  (interfaces.py:165-176)."""

    @staticmethod
    def forward(ctx, base, p):
        _need_cuda(base, p)
        b, s, cp, h, w = p.shape
        cb = base.shape[1]
        out = nhwc_empty(b, cb + cp + 1, h, w, p.device)
        check(lib().wcmc_pbuffer_cat_fwd(_ptr(base), *base.stride(), _ptr(p), *p.stride(), *_v(out),
                                         b, s, cb, cp, h, w, _stream()), "pbuffer_cat_fwd")
        ctx.dims = (b, s, cb, cp, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        b, s, cb, cp, h, w = ctx.dims
        g = _as_nhwc_nograd(g)
        dp = nhwc_empty(b * s, cp, h, w, g.device).unflatten(0, (b, s))
        check(lib().wcmc_pbuffer_cat_bwd(*_v(g), _ptr(dp), *dp.stride(), b, s, cb, cp, h, w, _stream()),
              "pbuffer_cat_bwd")
        return None, dp


def pbuffer_cat(base, p):
    out = _PBufferCat.apply(base, p)
    # the backward reads the gradient of channels [cb, cb + cp) only (the variance channel is detached, the base is data): a
    # conv chain that consumes `out` forms no more of its input gradient than that (conv_chain)
    out._wcmc_grad_channels = (base.shape[1], base.shape[1] + p.shape[2])
    return out


class _SampleCat(torch.autograd.Function):
    """cat([features, P, repeat_S(P.var(1).mean(1, keepdims).detach() / S)], 2) on (B,S,C,H,W) per-sample tensors
    (interfaces.py:394-403, 797-806)."""

    @staticmethod
    def forward(ctx, features, p):
        _need_cuda(features, p)
        b, s, c, h, w = features.shape
        cp = p.shape[2]
        assert p.shape[:2] == (b, s) and p.shape[3:] == (h, w)
        out = torch.empty((b, s, c + cp + 1, h, w), device=p.device, dtype=torch.float32)
        check(lib().wcmc_sample_cat_fwd(_ptr(features), *features.stride(), _ptr(p), *p.stride(), _ptr(out),
                                        b, s, c, cp, h, w, _stream()), "sample_cat_fwd")
        ctx.split = (c, cp)
        return out

    @staticmethod
    def backward(ctx, g):
        c, cp = ctx.split
        return g[:, :, :c], g[:, :, c:c + cp]


def sample_features_cat(features, p):
    return _SampleCat.apply(features, p)


class _FeatureMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, ref, idx_patch, idx_batch):
        _need_cuda(p, ref)
        b, s, c, h, w = p.shape
        nbytes = lib().wcmc_feature_mse_workspace_bytes(b, s, c, h, w)
        ws = torch.empty((nbytes + 3) // 4, device=p.device, dtype=torch.float32)
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        check(lib().wcmc_feature_mse_fwd(_ptr(p), *p.stride(), _ptr(ref), *ref.stride(),
                                         ctypes.c_void_p(idx_patch.data_ptr()),
                                         ctypes.c_void_p(idx_batch.data_ptr() if idx_batch is not None else 0),
                                         _ptr(loss), _ptr(ws), ws.numel() * 4, b, s, c, h, w, _stream()),
              "feature_mse_fwd")
        ctx.save_for_backward(p, idx_patch, ws)
        ctx.idx_batch = idx_batch
        return loss

    @staticmethod
    def backward(ctx, g):
        p, idx_patch, ws = ctx.saved_tensors
        idx_batch = ctx.idx_batch
        b, s, c, h, w = p.shape
        dp = torch.empty((b, s, c, h, w), device=p.device, dtype=torch.float32)
        g = g.contiguous()
        check(lib().wcmc_feature_mse_bwd(_ptr(p), *p.stride(), ctypes.c_void_p(idx_patch.data_ptr()),
                                         ctypes.c_void_p(idx_batch.data_ptr() if idx_batch is not None else 0),
                                         _ptr(g), _ptr(dp), _ptr(ws), ws.numel() * 4, b, s, c, h, w, _stream()),
              "feature_mse_bwd")
        return dp, None, None, None


class _GRS(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, ref, idx_patch, idx_batch, alpha):
        _need_cuda(p, ref)
        b, s, c, h, w = p.shape
        nbytes = lib().wcmc_feature_mse_workspace_bytes(b, s, c, h, w)
        ws = torch.empty((nbytes + 3) // 4, device=p.device, dtype=torch.float32)
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        check(lib().wcmc_grs_fwd(_ptr(p), *p.stride(), _ptr(ref), *ref.stride(),
                                 ctypes.c_void_p(idx_patch.data_ptr()), ctypes.c_void_p(idx_batch.data_ptr()),
                                 float(alpha), _ptr(loss), _ptr(ws), ws.numel() * 4, b, s, c, h, w, _stream()),
              "grs_fwd")
        ctx.save_for_backward(p, idx_patch, idx_batch, ws)
        return loss

    @staticmethod
    def backward(ctx, g):
        p, idx_patch, idx_batch, ws = ctx.saved_tensors
        b, s, c, h, w = p.shape
        dp = torch.empty((b, s, c, h, w), device=p.device, dtype=torch.float32)
        g = g.contiguous()
        check(lib().wcmc_grs_bwd(_ptr(p), *p.stride(), ctypes.c_void_p(idx_patch.data_ptr()),
                                 ctypes.c_void_p(idx_batch.data_ptr()), _ptr(g), _ptr(dp), _ptr(ws),
                                 ws.numel() * 4, b, s, c, h, w, _stream()), "grs_bwd")
        return dp, None, None, None, None


def grs_loss(p, ref, idx_patch, idx_batch, alpha=2.0):
    """GlobalRelativeSimilarityLoss on int64 DEVICE permutations."""
    return _GRS.apply(p, ref, idx_patch, idx_batch, alpha)


def feature_mse(p, ref, idx_patch, idx_batch):
    """idx_* are int64 DEVICE tensors (idx_batch may be None for non_local=False)."""
    return _FeatureMSE.apply(p, ref, idx_patch, idx_batch)


# ------------------------------------------------------------------------ optimiser
def clip_adam_(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, clip=1.0,
               grad_scale=1.0, guard=None):
    """In-place fused clip_grad_value_ + Adam over flat fp32 buffers (no-op when the device float
    ``guard`` is 0)."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq, guard)
    check(lib().wcmc_clip_adam(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                               clip, lr, beta1, beta2, eps, int(step), grad_scale, _ptr(guard), _stream()),
          "clip_adam")


def clip_adam_hyper(step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """The seven per-step floats of ``clip_adam_dev_`` (host arithmetic of ``wcmc_clip_adam``; no GPU call)."""
    out = (ctypes.c_float * 7)()
    lib().wcmc_clip_adam_hyper(float(lr), float(beta1), float(beta2), float(eps), int(step), out)
    return list(out)


def clip_adam_dev_(param, grad, exp_avg, exp_avg_sq, hyper, clip=1.0, grad_scale=1.0, guard=None):
    """``clip_adam_`` with its per-step scalars read from the device tensor ``hyper`` (7 floats, ``clip_adam_hyper``): the
    form a hipGraph can replay with other values every step."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq, hyper, guard)
    assert hyper.numel() >= 7 and hyper.is_contiguous()
    check(lib().wcmc_clip_adam_dev(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), clip,
                                   grad_scale, _ptr(hyper), _ptr(guard), _stream()), "clip_adam_dev")


def step_guard_(losses, ok, sums, flags):
    """``wcmc_step_guard``: flags[i] = isfinite(losses[i]), flags[n] = guard = all finite and ok; ok <- guard; sums[i] += losses[i]
    under the guard.  losses: 0-d fp32 device tensors; ok (1), sums (n), flags (n + 1): fp32 device tensors."""
    n = len(losses)
    _need_cuda(ok, sums, flags, *losses)
    assert sums.numel() == n and flags.numel() == n + 1 and sums.is_contiguous() and flags.is_contiguous()
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in losses])
    check(lib().wcmc_step_guard(arr, n, _ptr(ok), _ptr(sums), _ptr(flags), _stream()), "step_guard")


def step_guard_local_(losses, ok, flags, flag_slot):
    """``wcmc_step_guard_local`` (multi-rank tail, graph A): flags[i] = isfinite(losses[i]); flag_slot[0] = 1 - (all finite and ok)."""
    n = len(losses)
    _need_cuda(ok, flags, flag_slot, *losses)
    assert flags.numel() == n + 1 and flags.is_contiguous()
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in losses])
    check(lib().wcmc_step_guard_local(arr, n, _ptr(ok), _ptr(flags), _ptr(flag_slot), _stream()), "step_guard_local")


def step_guard_global_(losses, flag_slot, ok, sums, flags):
    """``wcmc_step_guard_global`` (multi-rank tail, graph B): guard = (flag_slot[0] == 0) -> flags[n], ok; sums[i] += losses[i] under it."""
    n = len(losses)
    _need_cuda(ok, sums, flags, flag_slot, *losses)
    assert sums.numel() == n and flags.numel() == n + 1
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in losses])
    check(lib().wcmc_step_guard_global(arr, n, _ptr(flag_slot), _ptr(ok), _ptr(sums), _ptr(flags), _stream()), "step_guard_global")


# ---------------------------------------------------------------------------------- data step
def _need_dense(t, ndim):
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != ndim or not t.is_contiguous():
        raise RuntimeError("wcmc_amd preprocessing takes contiguous fp32 CUDA tensors in the reference's numpy "
                           "layout (got %s %s %s); there is no CPU path" % (t.device, t.dtype, tuple(t.shape)))


def preprocess_llpm(sample, max_depth=5):
    """``DenoiseDataset._preprocess_llpm`` (datasets.py:302-361): raw (h,w,s,C) -> (h,w,s,37)."""
    _need_dense(sample, 4)
    h, w, s, c = sample.shape
    out = torch.empty((h, w, s, 7 + 5 * (max_depth + 1)), device=sample.device, dtype=torch.float32)
    check(lib().wcmc_preprocess_llpm(_ptr(sample), h * w * s, c, max_depth, _ptr(out), _stream()), "preprocess_llpm")
    return out


def preprocess_kpcn(sample, max_depth=5):
    """``DenoiseDataset._preprocess_kpcn`` (datasets.py:487-582): raw (h,w,s,C) -> (h,w,44)."""
    _need_dense(sample, 4)
    h, w, s, c = sample.shape
    out = torch.empty((h, w, 44), device=sample.device, dtype=torch.float32)
    nbytes = lib().wcmc_preprocess_kpcn_workspace_bytes(h, w)
    ws = torch.empty((nbytes + 3) // 4, device=sample.device, dtype=torch.float32)
    check(lib().wcmc_preprocess_kpcn(_ptr(sample), h, w, s, c, max_depth, _ptr(out), _ptr(ws), ws.numel() * 4, _stream()),
          "preprocess_kpcn")
    return out



def assemble_kpcn_patches(kpcn, llpm, gt, origins, patch):
    """The batch dictionary of the KPCN base model for windows of `patch` pixels at `origins` ((B, 2) int32 device
    tensor of (row, column)) of one image's preprocessed buffers (datasets.py:1026-1146 on the device)."""
    _need_cuda(kpcn, gt)
    if not origins.is_cuda:
        raise RuntimeError("assemble_kpcn_patches: origins must be a device tensor")
    h, w = kpcn.shape[:2]
    assert kpcn.shape == (h, w, 44) and gt.shape == (h, w, 9) and kpcn.is_contiguous() and gt.is_contiguous()
    assert origins.dtype == torch.int32 and origins.dim() == 2 and origins.shape[1] == 2 and origins.is_contiguous()
    b, s = origins.shape[0], 0
    if llpm is not None:
        assert llpm.shape[:2] == (h, w) and llpm.shape[3] == 37 and llpm.is_contiguous()
        s = llpm.shape[2]
    dev = kpcn.device
    cin = 35 if llpm is not None else 34
    shapes = {"kpcn_diffuse_in": (b, cin, patch, patch), "kpcn_specular_in": (b, cin, patch, patch),
              "kpcn_diffuse_buffer": (b, 3, patch, patch), "kpcn_specular_buffer": (b, 3, patch, patch),
              "kpcn_albedo": (b, 3, patch, patch), "target_diffuse": (b, 3, patch, patch),
              "target_specular": (b, 3, patch, patch), "target_total": (b, 3, patch, patch)}
    if llpm is not None:
        shapes["paths"] = (b, s, 36, patch, patch)
    # ONE allocation, the entries are views of it: a consumer on another stream keeps the batch alive with one
    # `record_stream` and frees one block (nine of each cost the training thread 0.25 ms per step: scripts/diag_loader_gap.py)
    sizes = {k: (math.prod(v) + 63) // 64 * 64 for k, v in shapes.items()}          # (every entry starts on a 256-byte boundary)
    flat = torch.empty(sum(sizes.values()), device=dev, dtype=torch.float32)
    out, off = {}, 0
    for k, shp in shapes.items():
        out[k] = flat[off:off + math.prod(shp)].view(shp)
        off += sizes[k]
    check(lib().wcmc_assemble_kpcn_patches(_ptr(kpcn), _ptr(llpm), _ptr(gt), ctypes.c_void_p(origins.data_ptr()), b, h, w,
                                           s, patch, _ptr(out["kpcn_diffuse_in"]), _ptr(out["kpcn_specular_in"]),
                                           _ptr(out["kpcn_diffuse_buffer"]), _ptr(out["kpcn_specular_buffer"]),
                                           _ptr(out["kpcn_albedo"]), _ptr(out.get("paths")), _ptr(out["target_diffuse"]),
                                           _ptr(out["target_specular"]), _ptr(out["target_total"]), _stream()),
          "assemble_kpcn_patches")
    return out


def gradients(buf):
    """``DenoiseDataset._gradients`` (datasets.py:286-300): (h,w,c) -> (h,w,2c)."""
    _need_dense(buf, 3)
    h, w, c = buf.shape
    out = torch.empty((h, w, 2 * c), device=buf.device, dtype=torch.float32)
    check(lib().wcmc_gradients(_ptr(buf), h, w, c, _ptr(out), _stream()), "gradients")
    return out


def reflect_index(i, n):
    """Source index of position ``i`` of a line of ``n`` entries under scipy's 'reflect' boundary (``wcmc_reflect_index``: the
    map the Gaussian passes of ``importance_map`` use; no GPU call)."""
    return int(lib().wcmc_reflect_index(int(i), int(n)))


def importance_map(img):
    """``gradient_importance_map`` (datasets.py:17-36): (H, W) or (H, W, 3) -> (H, W) in [0, 1]."""
    if img.dim() == 2:
        h, w, c = img.shape[0], img.shape[1], 1
    elif img.dim() == 3 and img.shape[2] in (1, 3):
        h, w, c = img.shape
    else:
        raise ValueError("importance_map: the image should be (H, W) or (H, W, 3), got %s" % (tuple(img.shape),))
    _need_dense(img, img.dim())
    out = torch.empty((h, w), device=img.device, dtype=torch.float32)
    nbytes = lib().wcmc_importance_map_workspace_bytes(h, w, c)
    ws = torch.empty((nbytes + 3) // 4, device=img.device, dtype=torch.float32)
    check(lib().wcmc_importance_map(_ptr(img), h, w, c, _ptr(out), _ptr(ws), ws.numel() * 4, _stream()), "importance_map")
    return out


def sampling_prob(raw, gt, patch_size=128, max_depth=5):
    """The patch-sampling map of ``_offline_preprocess`` (datasets.py:697-715): sanitised raw (H, W, S, 104) and gt (H, W, 9)
    -> (H - patch_size, W - patch_size), a distribution over patch origins."""
    _need_dense(raw, 4)
    _need_dense(gt, 3)
    h, w, s, c = raw.shape
    if tuple(gt.shape) != (h, w, 9):
        raise ValueError("sampling_prob: gt should be (%d, %d, 9), got %s" % (h, w, tuple(gt.shape)))
    if h <= patch_size or w <= patch_size:
        raise ValueError("sampling_prob: the image (%d x %d) must be larger than the patch (%d) in both dimensions"
                         % (h, w, patch_size))
    out = torch.empty((h - patch_size, w - patch_size), device=raw.device, dtype=torch.float32)
    nbytes = lib().wcmc_sampling_prob_workspace_bytes(h, w, patch_size)
    ws = torch.empty((nbytes + 7) // 8, device=raw.device, dtype=torch.float64)
    check(lib().wcmc_sampling_prob(_ptr(raw), _ptr(gt), h, w, s, c, max_depth, patch_size, _ptr(out), _ptr(ws), ws.numel() * 8,
                                   _stream()), "sampling_prob")
    return out


def sanitize_(x):
    """NaN / Inf / >= 1e38 -> 1e38 in place (datasets.py:623-624)."""
    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("sanitize_ takes a contiguous fp32 CUDA tensor (got %s %s); there is no CPU path" % (x.device, x.dtype))
    check(lib().wcmc_sanitize(_ptr(x), x.numel(), _stream()), "sanitize")
    return x


def random_permutation(n, device, out=None, seed=None):
    """A pseudo-random permutation of range(n) as an int64 device tensor, without the sort behind
    ``torch.randperm(n, device=...)`` (``wcmc_random_permutation``: keyed Feistel network).  The 62-bit key is drawn
    from torch's default CPU generator, so ``torch.manual_seed`` fixes the sequence of permutations."""
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=device)
    assert out.is_cuda and out.dtype == torch.int64 and out.numel() == n and out.is_contiguous()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    check(lib().wcmc_random_permutation(_ptr(out), n, int(seed), _stream()), "random_permutation")
    return out


def random_permutation_dev(out, state, slot):
    """``random_permutation`` keyed from the device tensor ``state`` = [seed, step counter] (int64) and ``slot``: the form a hipGraph
    can replay with another key every step (``wcmc_random_permutation_dev``)."""
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and state.is_cuda and state.dtype == torch.int64 and state.numel() >= 2
    check(lib().wcmc_random_permutation_dev(_ptr(out), out.numel(), _ptr(state), int(slot), _stream()), "random_permutation_dev")
    return out


def step_counter_advance(state):
    """state[1] += 1 on the device (``wcmc_step_counter_advance``)."""
    check(lib().wcmc_step_counter_advance(_ptr(state), _stream()), "step_counter_advance")


def permutation_key(seed, counter, slot):
    """Host mirror of the key ``random_permutation_dev`` forms (``wcmc_permutation_key``; no GPU call)."""
    return int(lib().wcmc_permutation_key(int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), int(slot)))


# ------------------------------------------------------------------------------------------------- full-frame evaluation
def image_eval(out, ipt, tgt, has_hit=None, eps=1e-4):
    """The 40 image metrics of one denoised frame (``wcmc_image_eval``; test_models.py:234-251, support/metrics.py): a (2, 4, 5)
    fp64 device tensor [comparison (out vs tgt, ipt vs tgt)][tone map (linear, _tonemap, tonemap, tonemap28)][metric (RelMSE,
    RelL1, DSSIM, L1, MSE)].  out / ipt / tgt: fp32 (H, W, 3) device tensors of any strides (a channel-first frame passes as
    ``frame.permute(1, 2, 0)`` without a copy); has_hit: the same form or None -- out is taken from ipt wherever it is 0."""
    _need_cuda(out, ipt, tgt, has_hit)
    h, w = out.shape[:2]
    for t in (out, ipt, tgt) + ((has_hit,) if has_hit is not None else ()):
        if t.dim() != 3 or tuple(t.shape) != (h, w, 3):
            raise ValueError("image_eval: images must be (H, W, 3) of one size (got %s and %s)"
                             % (tuple(out.shape), tuple(t.shape)))
    if h < 7 or w < 7:
        raise ValueError("image_eval: the image is %d x %d; SSIM's 7x7 window needs at least 7 x 7" % (h, w))
    dev = out.device
    res = torch.empty((2, 4, 5), device=dev, dtype=torch.float64)
    nbytes = lib().wcmc_image_eval_workspace_bytes(h, w)
    ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
    hh = has_hit if has_hit is not None else None
    hs = hh.stride() if hh is not None else (0, 0, 0)
    check(lib().wcmc_image_eval(_ptr(out), *out.stride(), _ptr(ipt), *ipt.stride(), _ptr(tgt), *tgt.stride(), _ptr(hh), *hs,
                                h, w, float(eps), _ptr(res), _ptr(ws), ws.numel() * 8, _stream()), "image_eval")
    return res


def check_tile_coords(coords, h, w, patch):
    """Host check of a (B, 6) tile table (i_start, j_start, i_end, j_end, i, j) before it goes to ``stitch_tiles``: every owned
    window lies inside the frame and inside its tile."""
    for i0, j0, i1, j1, i, j in coords:
        if not (0 <= i0 < i1 <= h and 0 <= j0 < j1 <= w and i <= i0 and j <= j0 and i1 <= i + patch and j1 <= j + patch):
            raise ValueError("stitch_tiles: tile %s does not fit a %d x %d frame of %d-pixel tiles"
                             % ((i0, j0, i1, j1, i, j), h, w, patch))


def stitch_tiles(out, p_buffers, coords, out_rad, out_path=None, patch=128):
    """Paste one batch of tiles into the full frame (``wcmc_stitch_tiles``; the slice loop of test_models.py:75-89).
    out: (B, 3, ho, wo) network output ('replicate'-padded back to ``patch`` on the fly when smaller); p_buffers: None, a
    (B, S, C, patch, patch) tensor or a dict of them; coords: device int32 (B, 6) table whose rows passed
    ``check_tile_coords``; out_rad (3, H, W) and out_path ((S, C, H, W), or a dict of them keyed like p_buffers) are written
    in place.  Bit-identical to the slice copies."""
    _need_cuda(out, out_rad)
    if not (coords.is_cuda and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 6
            and coords.is_contiguous()):
        raise RuntimeError("stitch_tiles: coords must be a contiguous device int32 (B, 6) tensor")
    b, c3, ho, wo = out.shape
    _, h, w = out_rad.shape
    assert c3 == 3 and coords.shape[0] == b and out_rad.shape[0] == 3 and out_rad.is_contiguous()
    pairs = []
    if p_buffers is not None:
        if isinstance(p_buffers, dict):
            pairs = [(p_buffers[k], out_path[k]) for k in p_buffers]
        else:
            pairs = [(p_buffers, out_path)]
    for pb, op in pairs:
        _need_cuda(pb, op)
        assert pb.dim() == 5 and pb.shape[0] == b and tuple(pb.shape[3:]) == (patch, patch) and pb.is_contiguous()
        assert tuple(op.shape) == (pb.shape[1], pb.shape[2], h, w) and op.is_contiguous()
    # two P-buffers of one shape per launch; anything else in further launches (the radiance is re-copied: same values)
    groups = [pairs[i:i + 2] for i in range(0, len(pairs), 2)] or [[]]
    if len(pairs) == 2 and pairs[0][0].shape != pairs[1][0].shape:
        groups = [[pairs[0]], [pairs[1]]]
    for g in groups:
        pa, oa = g[0] if len(g) > 0 else (None, None)
        pbb, ob = g[1] if len(g) > 1 else (None, None)
        s, c = (pa.shape[1], pa.shape[2]) if pa is not None else (0, 0)
        check(lib().wcmc_stitch_tiles(_ptr(out), *out.stride(), ho, wo, _ptr(pa), _ptr(pbb), s, c, patch,
                                      ctypes.c_void_p(coords.data_ptr()), b, h, w, _ptr(out_rad), _ptr(oa), _ptr(ob),
                                      _stream()), "stitch_tiles")
    return out_rad, out_path
