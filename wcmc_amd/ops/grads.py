"""Where weight gradients land: the optimiser's gradient sinks, weight normalisation (csrc/weight_norm.hip) and the deferred slab
reductions of the split-bf16 weight gradients."""
import ctypes
import weakref

import torch

from .. import ops as _sw          # the package itself: switches and rebound state are read there, when a function runs
from .._lib import check, lib
from ._base import _need_cuda, _stream
from .streams import _SIDE_STREAMS


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


# ---- deferred slab reductions ----------------------------------------------------------------------------------------------
# A weight-gradient launch is a split-K GEMM into slabs plus the slabs' reduction (and the bias gradient's finish).  Nothing reads
# dw before the optimiser -- or, in a weight-normalised model, before its weight-norm backward -- so inside a
# ``deferred_wgrad_reduce()`` scope (the interface opens one around its backward passes) the reductions of the SMALL layers are
# collected per stream and run as ONE launch (``wcmc_conv2d_wgrad_reduce_multi``) when the scope ends or the weight-norm backward
# asks: a PathNet's fifteen U-Net reductions of 5-15 us each, which neither fill the chip nor amortise their launch boundaries.
# Layers whose slabs are large (KPCN's 5x5 layers: 60 MB) keep their reduction right behind the GEMM, while the slabs are still
# in the Infinity Cache.  Results are bit-identical either way.  (``DEFER_MAX_BYTES`` and the open scope's entries, ``_DEFERRED``,
# live in the package: a test assigns the one and reads the other.)
class deferred_wgrad_reduce:
    def __enter__(self):
        self.outer = _sw._DEFERRED
        if _sw._DEFERRED is None:
            _sw._DEFERRED = {}
        return self

    def __exit__(self, *exc):
        if self.outer is None:
            pending, _sw._DEFERRED = _sw._DEFERRED, None
            if exc[0] is None:
                for st, entries in pending.values():
                    with torch.cuda.stream(st):
                        _reduce_multi(entries)
        return False


def flush_wgrad_reduce():
    """Run the reductions collected so far on the CURRENT stream (their results are about to be read).  Entries are only ever
    queued under the stream their GEMM ran on and never under a weight-gradient side stream (conv2d_wgrad_x_raw reduces inline
    there), so the reader's stream is where they all are."""
    if _sw._DEFERRED:
        st = torch.cuda.current_stream()
        hit = _sw._DEFERRED.pop(st.cuda_stream, None)
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
