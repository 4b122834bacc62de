"""What every module of the package stands on: activation codes, the per-launch profiler hook and the launch-plan queries that name
the conv launches' profiler classes, pointer / stream / stride helpers and the NHWC views."""
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


def conv_launch_plan(n, h, w, cin, cout, ks, pad, terms=3, out_split=True, ystrides=(0, 0, 0), gate=False, f16=False):
    """(profiler class, kernel instance as rocprofv3 prints it) of the launch ``wcmc_conv2d_igemm_bf16x3`` -- f16: ``wcmc_conv2d_out_f16`` --
    would run for these arguments: asked of the library's own launch plan (``wcmc_conv2d_launch_plan_bf16x3``), which touches no device.
    ystrides: (sn, sh, sw) of the fp32 output view when not out_split; gate: a gate TENSOR is given (a bit mask is not one)."""
    cls, ker = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    check(lib().wcmc_conv2d_launch_plan_bf16x3(n, h, w, cin, cout, ks, pad, terms, int(out_split), *ystrides, int(gate), int(f16),
                                               cls, ker, 128), "conv2d_launch_plan_bf16x3")
    return cls.value.decode(), ker.value.decode()


def wgrad_launch_plan(n, h, w, cin, cout, ks, pad, terms=3):
    """(profiler class, kernel instance) of the GEMM launch of ``wcmc_conv2d_wgrad_bf16x3``, as ``conv_launch_plan``."""
    cls, ker = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    check(lib().wcmc_conv2d_wgrad_launch_plan_bf16x3(n, h, w, cin, cout, ks, pad, terms, cls, ker, 128), "conv2d_wgrad_launch_plan_bf16x3")
    return cls.value.decode(), ker.value.decode()


def _timed_conv(dims, cout, ks, pad, terms, yf, gate, f16=False):
    """The profiler bracket of one GEMM launch, under the class the library's launch plan names for it (yf: the fp32 output view,
    None for a split output; gate: a gate tensor is given).  Without a profiler nothing is classified."""
    if _sw._PROFILER is None:
        return _Timed(None, 0.0, "flop")
    n, cin, h, w = dims
    pix = min((h + 2 * pad - ks + 1) * (w + 2 * pad - ks + 1), h * w)
    cls = conv_launch_plan(n, h, w, cin, cout, ks, pad, terms, yf is None, (0, 0, 0) if yf is None else _v(yf)[1:], gate, f16)[0]
    if cls == "conv_pw":    # algorithmic bytes: the split input and the split / fp32 output, 4 B per channel and pixel
        return _Timed(cls, 4.0 * n * pix * ((cin + 7) // 8 * 8 + cout), "byte")
    return _Timed(cls, 2.0 * n * pix * cout * cin * ks * ks, "flop")
