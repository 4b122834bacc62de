"""What every module of the package stands on: activation codes, the per-launch profiler hook and the profiler classes of the conv
launches, pointer / stream / stride helpers and the NHWC views."""
import ctypes

import torch

from .. import ops as _sw          # the package itself: switches and rebound state are read there, when a function runs
from .._lib import check, lib

ACT = {"linear": 0, "relu": 1, "leaky_relu": 2}
LEAKY_SLOPE = 0.01


# Optional per-launch timing (bench.py): HIP events recorded on the launch stream around an op.  The profiler object is the
# package's ``_PROFILER``: conv_split.py reads it too.
def set_profiler(prof):
    """prof: object with .add(name, work, unit, ev_start, ev_end) or None to disable."""
    _sw._PROFILER = prof


class _Timed:
    def __init__(self, name, work, unit):
        self.args = (name, work, unit)

    def __enter__(self):
        if _sw._PROFILER is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _sw._PROFILER is not None:
            self.e1.record()
            _sw._PROFILER.add(*self.args, self.e0, self.e1)
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
