"""The exact-fp32 conv chain (csrc/conv.hip)."""
import torch

from .. import ops as _sw          # the package itself: switches and rebound state are read there, when a function runs
from .._lib import check, lib
from ._base import ACT, LEAKY_SLOPE, _Timed, _as_nhwc_nograd, _need_cuda, _ptr, _stream, _v, nhwc_empty
from .streams import _side_stream


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


def _layer_label(cin, cout, ks):
    """Profiler LABEL of a layer shape in the exact-fp32 mode.  The fp32 library has one GEMM kernel: these strings name no kernel,
    they sort the launches by the shapes the split-bf16 classes of the same names cover (1x1 PathNet pairs, the U-Net's 3x3
    layers of 64-channel slabs, KPCN's 5x5 layers with seven cout tiles per block), so that the two modes' tables read side by side."""
    kp, tiles = (cin + 7) // 8 * 8, (cout + 15) // 16
    if ks == 1 and (kp, cout) in ((64, 64), (40, 64), (128, 128), (8, 128)):
        return "conv_pw"
    if ks == 3 and kp >= 32 and tiles % 4 == 0 and kp % 64 == 0:
        return "conv_halo3"
    seven = min((7, 4, 2, 1), key=lambda t: (-(-tiles // t)) * (t + 2)) == 7
    return "conv_halo7" if ks == 5 and kp >= 32 and seven else "conv_igemm"


def conv2d_raw(x, wp, bias, cout, ks, pad, act, gate=None, gate_act="linear", out=None):
    """One implicit-GEMM launch: out = act(conv(x) + bias) [* act'(gate)]."""
    n, cin, h, w = x.shape
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    if out is None:
        out = nhwc_empty(n, cout, ho, wo, x.device)
    g = _v(gate) if gate is not None else (_ptr(None), 0, 0, 0)
    # algorithmic FLOPs: 2 * pixels * Cout * Cin * ks^2 of the (smaller) valid-conv side
    pix = min(ho * wo, h * w)
    with _Timed(_layer_label(cin, cout, ks), 2.0 * n * pix * cout * cin * ks * ks, "flop"):
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
        if _sw.DEBUG_ACTS is not None:
            _sw.DEBUG_ACTS.extend(t for t, a in zip(xs[1:], acts) if a != "linear")
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
