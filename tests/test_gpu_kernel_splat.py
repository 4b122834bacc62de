"""Kernel splat on the MI355X (csrc/kernel_splat.hip through ops.kernel_splat / ops.logit_max and the two modules) against the
fp64 restatement tests/splat_ref.py.

Inputs are drawn as tests/test_gpu_ops.py draws them (data = gen + 0.5, logits = gen * 3, upstream gradients = gen), the metric
is that file's max-norm relative error and the bar its default, 2e-5 against fp64: an fp32 torch evaluation of the restatement
sits at <= 1.4e-6 on such inputs (sums, normalised output and both gradients), the kernel's sums are at most 441 fp32 adds deep.
The forward and the backward have a fixed summation order, so repeated runs are compared with ``torch.equal``; ``into`` adds the
new slabs onto the previous sums, which is another association than summing three separate results, so that comparison is held
to 2e-5, not to equality.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from splat_ref import splat_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 2e-5

# (N, C, h, w, k).  The kernel's tile is 16 x 8 source pixels (SP_TW x SP_TH): the last shape is two tiles and one pixel in each
# direction -- 3 x 3 ragged tiles, every destination summed from up to 3 x 3 slabs.
SHAPES = [(1, 3, 5, 7, 21), (2, 3, 23, 37, 21), (1, 1, 92, 92, 21), (2, 4, 33, 17, 21), (3, 2, 16, 16, 5), (1, 3, 9, 9, 3),
          (70, 3, 20, 12, 21), (1, 3, 17, 33, 21)]
MODES = ["softmax", "shift"]
WHICH = {"g_r": (True, False), "g_w": (False, True), "both": (True, True)}


def ops():
    from wcmc_amd import ops as _ops
    return _ops


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def assert_close(a, b, tol=TOL, what=""):
    assert tuple(a.shape) == tuple(b.shape), (what, a.shape, b.shape)
    e = rel_err(a, b)
    print("%s: rel err %.3e (bar %.1e)" % (what, e, tol))
    assert e <= tol, "%s: rel err %.3e > %.1e" % (what, e, tol)


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _inputs(shape):
    n, c, h, w, k = shape
    return (gen(n, c, h, w, seed=11) + 0.5, gen(n, k * k, h, w, seed=12, scale=3.0), gen(n, c, h, w, seed=13),
            gen(n, h, w, seed=14))


def _normalised(r, w):
    return r / (w.unsqueeze(1) + 1e-8)


@functools.lru_cache(maxsize=None)
def _reference(shape, mode):
    """fp64: sums, normalised output, and (d_logits, d_data) for g_r alone, g_w alone and both.  Computed once per case."""
    data, logits, g_r, g_w = _inputs(shape)
    d64, l64 = data.double().requires_grad_(), logits.double().requires_grad_()
    shift = logits.double().amax(dim=(1, 2, 3)) if mode == "shift" else None
    r, w = splat_ref(d64, l64, shift)
    grads = {}
    for which, (use_r, use_w) in WHICH.items():
        outs = ([r] if use_r else []) + ([w] if use_w else [])
        gs = ([g_r.double()] if use_r else []) + ([g_w.double()] if use_w else [])
        dl, dd = torch.autograd.grad(outs, [l64, d64], gs, retain_graph=True, allow_unused=True)
        grads[which] = (dl, dd if dd is not None else torch.zeros_like(d64))
    return r.detach(), w.detach(), _normalised(r, w).detach(), grads


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_splat_and_its_gradients_against_fp64(shape, mode):
    data, logits, g_r, g_w = _inputs(shape)
    r64, w64, out64, grads64 = _reference(shape, mode)
    dg, lg = data.to(DEV).requires_grad_(), logits.to(DEV).requires_grad_()
    shift = logits.amax(dim=(1, 2, 3)).to(DEV) if mode == "shift" else None
    r, w = ops().kernel_splat(dg, lg, shift=shift)
    assert_close(r, r64, what="sum_r")
    assert_close(w, w64, what="sum_w")
    assert_close(_normalised(r, w), out64, what="normalised")
    for which, (use_r, use_w) in WHICH.items():
        outs = ([r] if use_r else []) + ([w] if use_w else [])
        gs = ([g_r.to(DEV)] if use_r else []) + ([g_w.to(DEV)] if use_w else [])
        dl, dd = torch.autograd.grad(outs, [lg, dg], gs, retain_graph=True, allow_unused=True)
        assert_close(dl, grads64[which][0], what="d_logits (%s)" % which)
        assert_close(dd if dd is not None else torch.zeros_like(dg), grads64[which][1], what="d_data (%s)" % which)


# ------------------------------------------------------------------------------------------------------- known answers
KA = (1, 3, 26, 29)
SPIKE = (0 + 10) * 21 + (2 + 10)            # tap (dy, dx) = (0, +2)


def test_known_answer_box_filter():
    """Zero logits, zero shift: every weight is 1, the splat is the 21 x 21 box sum."""
    n, c, h, w = KA
    data = (gen(n, c, h, w, seed=21) + 0.5).to(DEV)
    r, sw = ops().kernel_splat(data, torch.zeros((n, 441, h, w), device=DEV), shift=torch.zeros(n, device=DEV))
    assert_close(r, 441 * F.avg_pool2d(F.pad(data.double(), (10,) * 4), 21, 1), tol=1e-5, what="box sum_r")
    assert_close(sw, 441 * F.avg_pool2d(F.pad(torch.ones((n, 1, h, w), dtype=torch.float64), (10,) * 4), 21, 1)[:, 0],
                 tol=1e-5, what="box sum_w")


@pytest.mark.parametrize("mode", MODES)
def test_known_answer_one_tap_pins_the_direction(mode):
    """One tap, (dy, dx) = (0, +2): the SOURCE q lands on q + (0, 2) -- the image moves two columns to the right, the mirror
    image of the gather's known answer."""
    n, c, h, w = KA
    data = (gen(n, c, h, w, seed=22) + 0.5).to(DEV)
    if mode == "shift":
        logits = torch.full((n, 441, h, w), -1e30, device=DEV)
        logits[:, SPIKE] = 0.0
        r, sw = ops().kernel_splat(data, logits, shift=torch.zeros(n, device=DEV))
    else:
        logits = torch.zeros((n, 441, h, w), device=DEV)
        logits[:, SPIKE] = 80.0
        r, sw = ops().kernel_splat(data, logits)
    want_r, want_w = torch.zeros_like(data), torch.zeros((n, h, w), device=DEV)
    want_r[..., :, 2:] = data[..., :, :-2]
    want_w[..., :, 2:] = 1.0
    assert_close(r, want_r, tol=1e-6, what="one tap sum_r")
    assert_close(sw, want_w, tol=1e-6, what="one tap sum_w")


# ------------------------------------------------------------------------------------- shift, accumulation, progressive form
MID = (2, 3, 23, 37, 21)


def test_normalised_output_does_not_depend_on_the_shift():
    data, logits, _, _ = _inputs(MID)
    data, logits = data.to(DEV), logits.to(DEV)
    m = logits.amax(dim=(1, 2, 3))
    a = _normalised(*ops().kernel_splat(data, logits, shift=m))
    b = _normalised(*ops().kernel_splat(data, logits, shift=m + 5))
    assert_close(b, a, what="shift + 5")


def _samples(shape, count=3):
    n, c, h, w, k = shape
    datas = [gen(n, c, h, w, seed=31 + s) + 0.5 for s in range(count)]
    logitss = [gen(n, k * k, h, w, seed=41 + s, scale=3.0) + (4.0 if s == 1 else 0.0) for s in range(count)]
    return datas, logitss


@pytest.mark.parametrize("mode", MODES)
def test_into_equals_the_sum_of_separate_calls(mode):
    datas, logitss = _samples(MID)
    shift = torch.stack([l.amax(dim=(1, 2, 3)) for l in logitss]).amax(dim=0).to(DEV) if mode == "shift" else None
    acc, parts = None, []
    for d, l in zip(datas, logitss):
        acc = ops().kernel_splat(d.to(DEV), l.to(DEV), shift=shift, into=acc)
        parts.append(ops().kernel_splat(d.to(DEV), l.to(DEV), shift=shift))
    assert_close(acc[0], sum(p[0].double() for p in parts), what="into sum_r")
    assert_close(acc[1], sum(p[1].double() for p in parts), what="into sum_w")


def test_progressive_kernel_apply_equals_one_evaluation_at_the_global_maximum():
    """Three samples, the second's logits raised by 4 so that the running maximum moves; forward and the gradients with respect
    to every sample's logits and data, against the restatement evaluated once with the global maximum as the shift."""
    from wcmc_amd import modules
    n, c, h, w, k = MID
    datas, logitss = _samples(MID)
    g = gen(n, c, h, w, seed=51)
    d64 = [d.double().requires_grad_() for d in datas]
    l64 = [l.double().requires_grad_() for l in logitss]
    gmax = torch.stack([l.double().amax(dim=(1, 2, 3)) for l in logitss]).amax(dim=0)
    r64 = w64 = 0
    for d, l in zip(d64, l64):
        r, sw = splat_ref(d, l, gmax)
        r64, w64 = r64 + r, w64 + sw
    out64 = _normalised(r64, w64)
    grads64 = torch.autograd.grad([out64], l64 + d64, [g.double()])

    pka = modules.ProgressiveKernelApply(splat=True)
    dg = [d.to(DEV).requires_grad_() for d in datas]
    lg = [l.to(DEV).requires_grad_() for l in logitss]
    sum_r = sum_w = max_w = None
    maxima = []
    for d, l in zip(dg, lg):
        sum_r, sum_w, max_w = pka(d, l, sum_r, sum_w, max_w)
        assert not max_w.requires_grad
        maxima.append(max_w.cpu())
    assert torch.equal(maxima[0], logitss[0].amax(dim=(1, 2, 3))) and bool((maxima[1] > maxima[0] + 3).all())   # it moved
    assert torch.equal(maxima[2], gmax.float())
    out = _normalised(sum_r, sum_w)
    assert_close(out, out64, what="progressive output")
    grads = torch.autograd.grad([out], lg + dg, [g.to(DEV)])
    for i, (a, b) in enumerate(zip(grads, grads64)):
        assert_close(a, b, what="progressive %s of sample %d" % ("d_logits" if i < 3 else "d_data", i % 3))


@pytest.mark.parametrize("mode", MODES)
def test_forward_and_backward_are_bitwise_reproducible(mode):
    data, logits, g_r, g_w = _inputs(MID)
    prev = (gen(2, 3, 23, 37, seed=61).to(DEV), gen(2, 23, 37, seed=62).to(DEV))
    shift = logits.amax(dim=(1, 2, 3)).to(DEV) if mode == "shift" else None
    runs = []
    for _ in range(2):
        dg, lg = data.to(DEV).requires_grad_(), logits.to(DEV).requires_grad_()
        r, w = ops().kernel_splat(dg, lg, shift=shift, into=prev)
        dl, dd = torch.autograd.grad([r, w], [lg, dg], [g_r.to(DEV), g_w.to(DEV)])
        runs.append((r.detach(), w.detach(), dl, dd))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("mode", MODES)
def test_layouts_give_the_same_result(mode):
    """logits as a plain NCHW tensor (converted by the op) and as an ``nhwc_empty`` view with its padded pixel stride; data as a
    contiguous tensor and as a cropped view of a larger tensor that is NaN outside; the softmax module crops by itself."""
    from wcmc_amd import modules
    n, c, h, w, k = MID
    data, logits, g_r, g_w = _inputs(MID)
    shift = logits.amax(dim=(1, 2, 3)).to(DEV) if mode == "shift" else None
    g_r, g_w = g_r.to(DEV), g_w.to(DEV)

    def run(d, l):
        r, sw = ops().kernel_splat(d, l, shift=shift)
        dl, dd = torch.autograd.grad([r, sw], [l, d], [g_r, g_w])
        return r.detach(), sw.detach(), dl, dd
    base = run(data.to(DEV).requires_grad_(), logits.to(DEV).requires_grad_())

    lv = ops().nhwc_empty(n, k * k, h, w, DEV)
    assert lv.stride(3) == 444 and ops().is_nhwc_view(lv)
    lv.copy_(logits)
    big = torch.full((n, c, h + 6, w + 8), float("nan"), device=DEV)
    big[:, :, 3:3 + h, 4:4 + w] = data
    dv = big[:, :, 3:3 + h, 4:4 + w].detach().requires_grad_()
    assert not dv.is_contiguous()
    for what, got in (("nhwc view", run(data.to(DEV).requires_grad_(), lv.requires_grad_())),
                      ("cropped data", run(dv, logits.to(DEV).requires_grad_()))):
        for name, a, b in zip(("sum_r", "sum_w", "d_logits", "d_data"), got, base):
            assert_close(a, b, tol=1e-7, what="%s: %s" % (what, name))
    if mode == "softmax":
        out = modules.KernelApply(softmax=True, splat=True)(big, logits.to(DEV))
        assert_close(out, _normalised(base[0], base[1]), tol=1e-7, what="KernelApply(splat=True) crops data like kernels")


# ---------------------------------------------------------------------------------------------------------------- logit_max
def test_logit_max_equals_amax_and_a_nan_shows():
    logits = gen(3, 441, 23, 37, seed=71, scale=3.0)
    assert torch.equal(ops().logit_max(logits.to(DEV)).cpu(), logits.amax(dim=(1, 2, 3)))
    lv = ops().nhwc_empty(3, 441, 23, 37, DEV)
    lv.copy_(logits)
    assert torch.equal(ops().logit_max(lv).cpu(), logits.amax(dim=(1, 2, 3)))
    # k = 5: 25 taps in a pixel stride of 28 -- what lies in the padding is not a logit
    small = gen(2, 25, 9, 11, seed=72, scale=3.0)
    buf = torch.full((2, 9, 11, 28), 1e9, device=DEV)
    sv = buf.permute(0, 3, 1, 2)[:, :25]
    sv.copy_(small)
    assert ops().is_nhwc_view(sv)
    assert torch.equal(ops().logit_max(sv).cpu(), small.amax(dim=(1, 2, 3)))
    poisoned = logits.clone()
    poisoned[1, 200, 11, 5] = float("nan")
    got, want = ops().logit_max(poisoned.to(DEV)).cpu(), poisoned.amax(dim=(1, 2, 3))
    assert bool(torch.isnan(got[1])) and bool(torch.isnan(want[1]))
    assert torch.equal(got[[0, 2]], want[[0, 2]])


# ------------------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_are_refused_with_a_message():
    o = ops()
    data = torch.zeros((1, 3, 8, 8), device=DEV)
    with pytest.raises(RuntimeError, match="odd"):
        o.kernel_splat(data, torch.zeros((1, 16, 8, 8), device=DEV))                    # even k
    with pytest.raises(RuntimeError, match="not a square"):
        o.kernel_splat(data, torch.zeros((1, 440, 8, 8), device=DEV))
    with pytest.raises(RuntimeError, match="C = 5"):
        o.kernel_splat(torch.zeros((1, 5, 8, 8), device=DEV), torch.zeros((1, 9, 8, 8), device=DEV))
    with pytest.raises(ValueError, match="differ"):
        o.kernel_splat(data, torch.zeros((1, 9, 8, 7), device=DEV))                     # mismatched shapes
    with pytest.raises(ValueError, match="differ"):
        o.kernel_splat(data, torch.zeros((2, 9, 8, 8), device=DEV))
    with pytest.raises(ValueError, match="shift"):
        o.kernel_splat(data, torch.zeros((1, 9, 8, 8), device=DEV), shift=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError, match="into"):
        o.kernel_splat(data, torch.zeros((1, 9, 8, 8), device=DEV), into=(torch.zeros((1, 3, 8, 8), device=DEV),
                                                                          torch.zeros((1, 1, 8, 8), device=DEV)))
    # the raw entry point: shift mode without a shift (tests/test_cpu_kernel_splat.py holds the rest of the ABI's refusals)
    import ctypes
    from wcmc_amd import _lib
    lg = o.nhwc_empty(1, 9, 8, 8, DEV, zero=True)
    out_r, out_w = torch.zeros((1, 3, 8, 8), device=DEV), torch.zeros((1, 8, 8), device=DEV)
    ws = torch.zeros(1 << 16, device=DEV)
    before = (out_r.clone(), out_w.clone())
    rc = _lib.lib().wcmc_kernel_splat_fwd(*o._v(lg), o._ptr(data), *data.stride(), o._ptr(out_r), o._ptr(out_w), ctypes.c_void_p(0),
                                          1, ctypes.c_void_p(0), 0, o._ptr(ws), ws.numel() * 4, 1, 3, 8, 8, 9, o._stream())
    assert rc == -1 and "shift" in _lib.lib().wcmc_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(out_r, before[0]) and torch.equal(out_w, before[1])              # nothing was launched
