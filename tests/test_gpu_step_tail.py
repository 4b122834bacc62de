"""The kernels at the tail of the step -- FeatureMSE / GRS, kernel apply, recombine -- against fp64 at step size.

Their gradients enter the step scaled by small loss weights and, in tests/test_gpu_bench_config.py, are seen only through a whole
network; here each op's forward and backward is compared directly, at the benchmark geometry (B=8, S=8, 92x92; 21x21 kernels)
and at the layouts the step passes (NHWC-backed P-buffers, cropped radiance, an upstream gradient that is not 1).

Every quantity is computed three times on the same inputs: the CPU oracle in float64 (the reference), the CPU oracle in float32
(the yardstick) and the product.  The bar is

    K_BAR x max(fp32 oracle's distance to fp64, FLOOR [, LSE_ULP x max |lse|])      capped at the project's 1e-3 contract

and never derives from the product's error.  Measured distances, per case: profiles/r08_step_tail_fp64.txt
(scripts/step_tail_fp64.py runs the functions of this file with the assertions off and prints every figure):

    kernel          largest product distance (fp32 oracle on it)                  largest product / max(fp32 oracle, floor, bound)
    FeatureMSE      1.8e-7 (1.5e-7)  dP, C = 8                                     0.09
    GRS             1.0e-5 (1.0e-5)  dP past the overflow edge; 1.2e-6 otherwise   1.00
    kernel apply    1.6e-5 (5.0e-7)  d_logits, logits +-500, bound 6.0e-5          0.60 (5x7 image, d_logits 1.2e-6)
    recombine       1.7e-7 (1.6e-7)  forward, 8x3x92x92                            0.69

FLOOR = 2e-6 (max-norm, relative to the tensor's max): the fp32 oracle's FeatureMSE dP at (8,8,3,92,92) is 1.5e-7 from fp64 and its
loss 7.5e-9 -- it accumulates in a different order than a kernel may, so a kernel is not held to the oracle's own luck: the
floor is two fp32 ulps of a quantity of the magnitude of GRS's exponents (|alpha d - lse| < 32: ulp 1.9e-6), the coarsest
rounding any of these kernels performs on well-scaled inputs.
FLOOR_RECOMBINE = 2.4e-7 (elementwise relative): two fp32 ulps -- expf's documented bound plus the rounding of one product.
LSE_ULP = 1.2e-7: kernel apply's backward rebuilds the weights as exp2(l log2e - lse log2e) from an fp32 LSE, one ulp of
|lse| log2e in the exponent = a relative weight error of 1.2e-7 |lse|; the fp32 oracle subtracts the max exactly and is no fair
yardstick for large logits, so the bound enters the bar by arithmetic (|lse| from the fp64 oracle, i.e. from the inputs).
"""
import ctypes
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import losses as ol            # noqa: E402
from oracle import modules as om           # noqa: E402
from test_gpu_ops import DEV, gen, ops     # noqa: E402

K_BAR = 8.0
FLOOR = 2e-6
FLOOR_RECOMBINE = 2.4e-7
LSE_ULP = 1.2e-7
CONTRACT = 1e-3

ASSERT = True           # scripts/step_tail_fp64.py turns the assertions off and reads RECORDS
RECORDS = []            # (kernel, case, quantity, product distance, fp32 oracle distance, bar)
ORACLE_SECONDS = [0.0]  # wall time of the fp64 + fp32 oracle runs of this file


class _oracle_clock:
    def __enter__(self):
        self.t0 = time.time()

    def __exit__(self, *exc):
        ORACLE_SECONDS[0] += time.time() - self.t0
        return False


def maxnorm(a, ref):
    """max |a - ref| / max |ref| in fp64."""
    a, b = a.detach().double().cpu(), ref.detach().double().cpu()
    assert tuple(a.shape) == tuple(b.shape), (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def elementwise(a, ref, scale):
    """max over the entries of |a - ref| / scale (scale > 0, fp64): no entry hides behind the tensor's largest."""
    a, b = a.detach().double().cpu(), ref.detach().double().cpu()
    assert tuple(a.shape) == tuple(b.shape), (a.shape, b.shape)
    return ((a - b).abs() / scale.double().clamp_min(1e-300)).max().item()


def hold(kernel, case, what, d_prod, d_f32, floor=FLOOR, extra=0.0):
    """Record and print the three-way figures, then hold the product to K_BAR x max(fp32 oracle, floor, extra) <= CONTRACT."""
    bar = min(CONTRACT, K_BAR * max(d_f32, floor, extra))
    RECORDS.append((kernel, case, what, d_prod, d_f32, bar))
    print("%-12s %-44s %-10s product %.3e  fp32 oracle %.3e  ratio %8.2f  bar %.3e"
          % (kernel, case, what, d_prod, d_f32, d_prod / max(d_f32, floor, extra), bar))
    if ASSERT:
        assert math.isfinite(d_prod) and d_prod <= bar, \
            "%s %s %s: product is %.3e from fp64 > bar %.3e (fp32 oracle %.3e)" % (kernel, case, what, d_prod, bar, d_f32)


def _scalar_dist(a, ref):
    a, b = float(a), float(ref)
    return abs(a - b) / max(abs(b), 1e-300)


# ============================================================================ FeatureMSE / GRS
FM_BIG = [(8, 8, 3, 92, 92),       # N = 541,696 rows: the forward's grid-stride loop runs three times
          (16, 8, 3, 92, 92)]      # N = 1,083,392 > 4096 x 256: the backward's loop runs a second time as well
FM_SMALL = [(2, 3, 1, 5, 7), (3, 2, 4, 9, 6), (1, 5, 5, 7, 11), (2, 3, 8, 6, 13)]       # ragged, C in {1, 4, 5, 8}; one with B = 1
FM_SHAPES = FM_BIG + FM_SMALL
GRS_ALPHAS = [0.5, 2.0]


def _perm_with_fixed_points(n, g):
    """A permutation of [0, n) that leaves about 40 % of the entries where they are."""
    idx = torch.arange(n)
    mov = torch.nonzero(torch.rand(n, generator=g) < 0.6).flatten()
    idx[mov] = mov[torch.randperm(mov.numel(), generator=g)]
    assert int((idx == torch.arange(n)).sum()) > 0 and torch.equal(idx.sort().values, torch.arange(n))
    return idx


def fm_inputs(shape, seed, pairing="random", ref_kind="positive", p_scale=1.0):
    b, s, c, h, w = shape
    p = (gen(b, s, c, h, w, seed=seed) + 0.5) * p_scale
    if ref_kind == "positive":
        ref = gen(b, 3, h, w, seed=seed + 1) + 1.0
    else:                                                   # negative components (the tone map clamps them) and exact zeros
        ref = gen(b, 3, h, w, seed=seed + 1, scale=2.0)
        ref.view(-1)[::5] = 0.0
        assert bool((ref < 0).any()) and bool((ref == 0).any()) and bool((ref > 0).any())
    g = torch.Generator().manual_seed(seed + 2)
    n, shw = b * s * h * w, s * h * w
    if pairing == "random":
        ip, ib = torch.randperm(shw, generator=g), torch.randperm(n, generator=g)
    elif pairing == "fixed":
        ip, ib = _perm_with_fixed_points(shw, g), _perm_with_fixed_points(n, g)
    else:
        ip, ib = torch.arange(shw), torch.arange(n)
    return p, ref, ip, ib


def fm_oracle(kind, p, ref, ip, ib, alpha, factor, dtype):
    """(loss, d(factor * loss)/dP) of the CPU oracle in `dtype`."""
    with _oracle_clock():
        pr = p.detach().clone().to(dtype).requires_grad_(True)      # (a clone: .to(float32) would hand back p itself)
        if kind == "fmse":
            loss = ol.feature_mse(pr, ref.to(dtype), ip, ib)
        else:
            loss = ol.global_relative_similarity(pr, ref.to(dtype), ip, ib, alpha)
        (factor * loss).backward()
        return loss.detach(), pr.grad


def fm_layouts(p, ref):
    """The same values as (name, P, ref) in the layouts the step passes: contiguous; the NHWC-backed `unflatten` view PathNet
    returns, with a cropped reference; a channel slice of a wider NHWC-backed P (disentanglement)."""
    o = ops()
    b, s, c, h, w = p.shape
    pd, rd = p.to(DEV), ref.to(DEV)
    yield "contiguous", pd, rd
    rwide = torch.full((b, 3, h + 3, w + 5), float("nan"), device=DEV)
    rwide[:, :, 1:1 + h, 2:2 + w] = rd
    pn = o.to_nhwc_raw(pd.view(b * s, c, h, w)).unflatten(0, (b, s))
    assert (c == 1 or pn.stride(2) == 1) and pn.stride(4) == (c + 3) // 4 * 4 and not pn.is_contiguous()      # pixel-major
    yield "nhwc", pn, rwide[:, :, 1:1 + h, 2:2 + w]
    wide = gen(b, s, c + 3, h, w, seed=977).to(DEV)
    wide[:, :, 2:2 + c] = pd
    wn = o.to_nhwc_raw(wide.view(b * s, c + 3, h, w)).unflatten(0, (b, s))
    yield "slice", wn[:, :, 2:2 + c], rd


def fm_product(kind, pdev, refdev, ip, ib, alpha, factor):
    o = ops()
    pl = pdev.detach().requires_grad_(True)
    ipd, ibd = ip.to(DEV), (ib.to(DEV) if ib is not None else None)
    loss = o.feature_mse(pl, refdev, ipd, ibd) if kind == "fmse" else o.grs_loss(pl, refdev, ipd, ibd, alpha)
    (loss if factor == 1.0 else factor * loss).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), pl.grad.cpu()


def fm_three_way(kind, case, p, ref, ip, ib, alpha=None, factor=1.0):
    """Product in every layout (all bit-identical) against the fp64 oracle, with the fp32 oracle as the yardstick."""
    kernel = "FeatureMSE" if kind == "fmse" else "GRS"
    l64, g64 = fm_oracle(kind, p, ref, ip, ib, alpha, factor, torch.float64)
    l32, g32 = fm_oracle(kind, p, ref, ip, ib, alpha, factor, torch.float32)
    first = None
    for name, pdev, rdev in fm_layouts(p, ref):
        loss, grad = fm_product(kind, pdev, rdev, ip, ib, alpha, factor)
        assert tuple(grad.shape) == tuple(p.shape)
        if first is None:
            first = (loss, grad)
        else:
            assert torch.equal(loss, first[0]), "%s %s: the loss of the %s layout differs from the contiguous one" % (kernel, case, name)
            assert torch.equal(grad, first[1]), "%s %s: dP of the %s layout differs from the contiguous one" % (kernel, case, name)
    loss, grad = first
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), "%s %s: not finite" % (kernel, case)
    hold(kernel, case, "loss", _scalar_dist(loss, l64), _scalar_dist(l32, l64))
    hold(kernel, case, "dP", maxnorm(grad, g64), maxnorm(g32, g64))
    return loss, grad


def _tag(shape):
    return "x".join(str(v) for v in shape)


def run_feature_mse(shape):
    t = _tag(shape)
    p, ref, ip, ib = fm_inputs(shape, seed=500)
    fm_three_way("fmse", t + " base", p, ref, ip, ib)
    fm_three_way("fmse", t + " upstream 0.1", p, ref, ip, ib, factor=0.1)
    fm_three_way("fmse", t + " non_local=False", p, ref, ip, None)
    fm_three_way("fmse", t + " non_local=False upstream 0.1", p, ref, ip, None, factor=0.1)
    p, ref, ip, ib = fm_inputs(shape, seed=510, pairing="fixed")
    fm_three_way("fmse", t + " fixed points", p, ref, ip, ib, factor=0.1)
    p, ref, ip, ib = fm_inputs(shape, seed=520, ref_kind="signed")
    fm_three_way("fmse", t + " signed reference", p, ref, ip, ib)
    # the identity pairing: every displacement is exactly zero, and so are the loss and dP, in every layout
    p, ref, ip, ib = fm_inputs(shape, seed=530, pairing="identity")
    for idb in (ib, None):
        for name, pdev, rdev in fm_layouts(p, ref):
            loss, grad = fm_product("fmse", pdev, rdev, ip, idb, None, 0.1)
            assert loss.item() == 0.0 and bool((grad == 0).all()), (t, name, "identity pairing", loss.item(), grad.abs().max().item())


def run_grs(shape, alpha):
    t = _tag(shape)
    p, ref, ip, ib = fm_inputs(shape, seed=540)
    fm_three_way("grs", t + " alpha %g" % alpha, p, ref, ip, ib, alpha=alpha)
    p, ref, ip, ib = fm_inputs(shape, seed=550, pairing="fixed", ref_kind="signed")
    fm_three_way("grs", t + " alpha %g fixed points, signed reference, upstream 0.1" % alpha, p, ref, ip, ib, alpha=alpha, factor=0.1)


def _max_abs_disp(p, ref, ip, ib):
    b, s, c, h, w = p.shape
    r = ol.tonemap_gamma(ref.double()).unsqueeze(1).expand(b, s, 3, h, w)
    pr, rr = ol._rows(p.double()), ol._rows(r)
    return max(ol.pair_displacement(pr, rr, ip).abs().max().item(),
               ol.pair_displacement(pr.reshape(-1, c), rr.reshape(-1, 3), ib).abs().max().item())


def run_grs_overflow(shape):
    """P scaled until alpha max|d| is past 88, where fp32 exp overflows: the kernel subtracts the largest exponent first."""
    alpha = 2.0
    p, ref, ip, ib = fm_inputs(shape, seed=560)
    scale = math.sqrt(130.0 / (alpha * _max_abs_disp(p, ref, ip, ib)))
    p, ref, ip, ib = fm_inputs(shape, seed=560, p_scale=scale)
    top = alpha * _max_abs_disp(p, ref, ip, ib)
    assert top > 88.0, top
    loss, grad = fm_three_way("grs", _tag(shape) + " alpha 2, alpha max|d| = %.0f" % top, p, ref, ip, ib, alpha=alpha)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0.0


@pytest.mark.parametrize("shape", FM_SHAPES, ids=_tag)
def test_feature_mse_loss_and_gradient_against_fp64(shape):
    run_feature_mse(shape)


@pytest.mark.parametrize("alpha", GRS_ALPHAS)
@pytest.mark.parametrize("shape", FM_SHAPES, ids=_tag)
def test_grs_loss_and_gradient_against_fp64(shape, alpha):
    run_grs(shape, alpha)


@pytest.mark.parametrize("shape", [FM_BIG[0], FM_SMALL[1], FM_SMALL[3]], ids=_tag)
def test_grs_past_the_fp32_exp_overflow_edge(shape):
    run_grs_overflow(shape)


def run_two_live_nodes(shape=FM_BIG[0]):
    """Two FeatureMSE nodes on different P-buffers (the diffuse and the specular one), then a GRS node, ONE backward of their
    weighted sum: each node's backward reads the workspace its own forward left (inverse pairings, displacements, lse), after
    the other forwards have run.  Each dP is, bit for bit, the dP of that node run alone, and matches fp64."""
    o = ops()
    b, s, c, h, w = shape
    nodes = []
    for i, (kind, weight) in enumerate((("fmse", 0.1), ("fmse", 0.25), ("grs", 0.05))):
        p, ref, ip, ib = fm_inputs(shape, seed=600 + 10 * i)
        nodes.append((kind, weight, p, ref, ip, ib))
    leaves, total = [], None
    for kind, weight, p, ref, ip, ib in nodes:
        pl = o.to_nhwc_raw(p.view(b * s, c, h, w).to(DEV)).unflatten(0, (b, s)).requires_grad_(True)
        ipd, ibd, rd = ip.to(DEV), ib.to(DEV), ref.to(DEV)
        loss = o.feature_mse(pl, rd, ipd, ibd) if kind == "fmse" else o.grs_loss(pl, rd, ipd, ibd, 2.0)
        leaves.append((pl, loss))
        total = weight * loss if total is None else total + weight * loss
    total.backward()
    torch.cuda.synchronize()
    for i, ((kind, weight, p, ref, ip, ib), (pl, loss)) in enumerate(zip(nodes, leaves)):
        case = "%s node %d of 3 (%s, weight %g)" % (_tag(shape), i, kind, weight)
        pn = o.to_nhwc_raw(p.view(b * s, c, h, w).to(DEV)).unflatten(0, (b, s))
        l_alone, g_alone = fm_product(kind, pn, ref.to(DEV), ip, ib, 2.0, weight)
        assert torch.equal(loss.detach().cpu(), l_alone), case + ": the loss differs from the node run alone"
        assert torch.equal(pl.grad.cpu(), g_alone), case + ": dP differs from the node run alone"
        kernel = "FeatureMSE" if kind == "fmse" else "GRS"
        l64, g64 = fm_oracle(kind, p, ref, ip, ib, 2.0, weight, torch.float64)
        l32, g32 = fm_oracle(kind, p, ref, ip, ib, 2.0, weight, torch.float32)
        hold(kernel, case, "loss", _scalar_dist(loss.item(), l64), _scalar_dist(l32, l64))
        hold(kernel, case, "dP", maxnorm(pl.grad, g64), maxnorm(g32, g64))


def test_two_feature_mse_nodes_and_a_grs_node_keep_their_own_workspaces():
    run_two_live_nodes()


def test_feature_mse_abi_refusals_launch_nothing():
    """C = 9, a workspace one byte short, grs_* without idx_batch and alpha <= 0 return an error; the loss, the workspace and dP
    keep their sentinels: nothing was launched."""
    from wcmc_amd._lib import lib
    o, L = ops(), lib()
    b, s, h, w = 2, 3, 5, 7
    ref = (gen(b, 3, h, w, seed=701) + 1).to(DEV)
    ip, ib = torch.randperm(s * h * w).to(DEV), torch.randperm(b * s * h * w).to(DEV)
    st = o._stream()

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None else 0)

    def attempt(c, short=0, use_ib=True, alpha=None, grs=False, bwd=True):
        # (bwd=False where only the forward refuses: the backward's contract is a workspace its forward has filled)
        p = (gen(b, s, c, h, w, seed=700) + 1).to(DEV)
        nbytes = L.wcmc_feature_mse_workspace_bytes(b, s, min(c, 8), h, w)
        assert nbytes > 0
        ws = torch.full(((nbytes + 3) // 4,), 7.0, device=DEV)
        loss = torch.full((), -3.0, device=DEV)
        dp = torch.full((b, s, c, h, w), 5.0, device=DEV)
        gs = torch.ones((), device=DEV)
        ibp = ptr(ib if use_ib else None)
        if grs:
            rc_f = L.wcmc_grs_fwd(ptr(p), *p.stride(), ptr(ref), *ref.stride(), ptr(ip), ibp, float(2.0 if alpha is None else alpha),
                                  ptr(loss), ptr(ws), nbytes - short, b, s, c, h, w, st)
            msg_f = L.wcmc_last_error().decode()
            rc_b = L.wcmc_grs_bwd(ptr(p), *p.stride(), ptr(ip), ibp, ptr(gs), ptr(dp), ptr(ws), nbytes - short, b, s, c, h, w,
                                  st) if bwd else None
        else:
            rc_f = L.wcmc_feature_mse_fwd(ptr(p), *p.stride(), ptr(ref), *ref.stride(), ptr(ip), ibp, ptr(loss), ptr(ws),
                                          nbytes - short, b, s, c, h, w, st)
            msg_f = L.wcmc_last_error().decode()
            rc_b = L.wcmc_feature_mse_bwd(ptr(p), *p.stride(), ptr(ip), ibp, ptr(gs), ptr(dp), ptr(ws), nbytes - short, b, s, c,
                                          h, w, st) if bwd else None
        msg_b = L.wcmc_last_error().decode()
        torch.cuda.synchronize()
        untouched = loss.item() == -3.0 and bool((ws == 7.0).all())
        return rc_f, rc_b, msg_f, msg_b, untouched, bool((dp == 5.0).all())

    # the arguments themselves are sound: the same call with nothing wrong succeeds and writes
    for grs in (False, True):
        rc_f, rc_b, _, _, untouched, dp_untouched = attempt(8, grs=grs)
        assert rc_f == 0 and rc_b == 0 and not untouched and not dp_untouched
    for grs in (False, True):
        rc_f, rc_b, mf, mb, untouched, dp_untouched = attempt(9, grs=grs)
        assert rc_f != 0 and rc_b != 0 and "C <= 8" in mf and "C <= 8" in mb and untouched and dp_untouched, ("C = 9", grs, mf, mb)
        rc_f, rc_b, mf, mb, untouched, dp_untouched = attempt(3, short=1, grs=grs)
        assert rc_f != 0 and rc_b != 0 and "workspace" in mf and "workspace" in mb and untouched and dp_untouched, ("workspace", grs, mf, mb)
    rc_f, rc_b, mf, mb, untouched, dp_untouched = attempt(3, use_ib=False, grs=True)
    assert rc_f != 0 and rc_b != 0 and "pairings" in mf and "pairings" in mb and untouched and dp_untouched, ("idx_batch", mf, mb)
    for alpha in (0.0, -2.0, float("nan")):
        rc_f, _, mf, _, untouched, _ = attempt(3, alpha=alpha, grs=True, bwd=False)
        assert rc_f != 0 and "alpha > 0" in mf and untouched, ("alpha", alpha, mf)
    # and through ops: an error, not a quiet result
    p9 = torch.zeros(b, s, 9, h, w, device=DEV)
    with pytest.raises(RuntimeError, match="C <= 8"):
        o.feature_mse(p9, ref, ip, ib)
    with pytest.raises(RuntimeError, match="alpha > 0"):
        o.grs_loss(p9[:, :, :3], ref, ip, ib, 0.0)


# ============================================================================ kernel apply
KA_N, KA_C, KA_HW, KA_K = 8, 3, 92, 21
KA_CASES = ["normal", "pm50", "pm500", "hdr", "special", "ragged 37x45", "tiny 5x7"]
KA_SPECIAL = {"equal": (0, 10, 11), "spike": (1, 40, 50)}      # (image, y, x) of the two special pixels of the "special" case


def ka_inputs(name):
    """(data, logits, upstream gradient) of one input family, fp32 on the CPU."""
    n, c, h, w = KA_N, KA_C, KA_HW, KA_HW
    if name == "ragged 37x45":
        n, h, w = 2, 37, 45
    elif name == "tiny 5x7":
        n, h, w = 1, 5, 7
    elif name == "special":
        n = 2
    k2 = KA_K * KA_K
    g = torch.Generator().manual_seed(800 + KA_CASES.index(name))
    data = torch.randn(n, c, h, w, generator=g) + 0.5                           # radiance N(0.5, 1)
    logits = torch.randn(n, k2, h, w, generator=g) * 3.0                        # N(0, 3^2): the family of tests/test_gpu_ops.py
    if name == "pm50":
        logits = gen(n, k2, h, w, seed=811, scale=50.0)                         # spiky kernels
    elif name == "pm500":
        logits = gen(n, k2, h, w, seed=812, scale=500.0)
    elif name == "hdr":                                                         # log-normal radiance and a few values near 1e4
        data = torch.exp(torch.randn(n, c, h, w, generator=g) * 1.5)
        at = torch.randint(0, data.numel(), (6,), generator=g)
        data.view(-1)[at] = torch.tensor([9.7e3, 1.0e4, 1.04e4, 1.1e4, 8.9e3, 1.2e4])
    elif name == "special":
        i, y, x = KA_SPECIAL["equal"]
        logits[i, :, y, x] = 1.7                                                # all taps equal: weights 1/441
        i, y, x = KA_SPECIAL["spike"]
        logits[i, 137, y, x] = logits[i, :, y, x].max() + 80.0                  # a single tap 80 above the rest
    up = gen(n, c, h, w, seed=820 + KA_CASES.index(name))
    return data, logits, up


_KA_KEPT = {}


def ka_oracle(name, data, logits, up):
    """fp64 and fp32 oracle, image by image (the unfolded radiance of one 92x92 image is 90 MB in fp64):
    {dtype: (out, d_logits, d_data)} and max |lse| over the pixels (from the fp64 logits)."""
    if name in _KA_KEPT:
        return _KA_KEPT[name]
    res = {}
    with _oracle_clock():
        for dtype in (torch.float64, torch.float32):
            outs, dls, dds = [], [], []
            for i in range(data.shape[0]):
                dr = data[i:i + 1].clone().to(dtype).requires_grad_(True)
                lr = logits[i:i + 1].clone().to(dtype).requires_grad_(True)
                out = om.kernel_apply(dr, lr)
                out.backward(up[i:i + 1].to(dtype))
                outs.append(out.detach()); dls.append(lr.grad); dds.append(dr.grad)
            res[dtype] = (torch.cat(outs), torch.cat(dls), torch.cat(dds))
        lse = torch.logsumexp(logits.double(), dim=1).abs().max().item()
    if name == "normal":                      # the mutation check reads it again
        _KA_KEPT[name] = (res, lse)
    return res, lse


def ka_product(route, data, logits, up):
    """route "strip": logits as an NHWC view, cropped (strided) radiance without a gradient -- what KPCN passes; the backward is the
    persistent strip kernel.  route "tile": gradient on the radiance as well -- the tile kernel.  (out, d_logits, d_data or None)"""
    o = ops()
    n, k2, h, w = logits.shape
    if route == "strip":
        wide = torch.full((n, data.shape[1], h + 6, w + 8), float("nan"), device=DEV)
        wide[:, :, 3:3 + h, 4:4 + w] = data.to(DEV)
        dd = wide[:, :, 3:3 + h, 4:4 + w]
        ld = o.nhwc_empty(n, k2, h, w, DEV)
        ld.copy_(logits.to(DEV))
        ld.requires_grad_(True)
        assert o.is_nhwc_view(ld) and not dd.is_contiguous()
        out = o._KernelApply.apply(dd, ld)
    else:
        dd, ld = data.to(DEV).requires_grad_(True), logits.to(DEV).requires_grad_(True)
        out = o.kernel_apply(dd, ld)
    out.backward(up.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), ld.grad.cpu(), (dd.grad.cpu() if route == "tile" else None)


def run_kernel_apply(name, routes=("strip", "tile")):
    data, logits, up = ka_inputs(name)
    res, lse = ka_oracle(name, data, logits, up)
    (o64, l64, d64), (o32, l32, d32) = res[torch.float64], res[torch.float32]
    lse_bound = LSE_ULP * lse                   # one ulp of |lse| log2e in the backward's exponent
    for route in routes:
        out, dl, dd = ka_product(route, data, logits, up)
        case = "%s %s (max |lse| %.0f)" % (name, route, lse)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all()), case + ": not finite"
        hold("kernel_apply", case, "out", maxnorm(out, o64), maxnorm(o32, o64))
        hold("kernel_apply", case, "d_logits", maxnorm(dl, l64), maxnorm(l32, l64), extra=lse_bound)
        if dd is not None:
            hold("kernel_apply", case, "d_data", maxnorm(dd, d64), maxnorm(d32, d64), extra=lse_bound)
        if name == "special":
            # the two special pixels on their own scale: the tensor's max must not hide them
            i, y, x = KA_SPECIAL["equal"]
            hold("kernel_apply", case + " equal-taps pixel", "out", maxnorm(out[i, :, y, x], o64[i, :, y, x]),
                 maxnorm(o32[i, :, y, x], o64[i, :, y, x]))
            hold("kernel_apply", case + " equal-taps pixel", "d_logits", maxnorm(dl[i, :, y, x], l64[i, :, y, x]),
                 maxnorm(l32[i, :, y, x], l64[i, :, y, x]))
            i, y, x = KA_SPECIAL["spike"]       # (its d_logits row is pure cancellation, ~0: held by the tensor's max above)
            hold("kernel_apply", case + " spike pixel", "out", maxnorm(out[i, :, y, x], o64[i, :, y, x]),
                 maxnorm(o32[i, :, y, x], o64[i, :, y, x]))


@pytest.mark.parametrize("name", KA_CASES)
def test_kernel_apply_both_routes_against_fp64(name):
    run_kernel_apply(name)


# ============================================================================ recombine
RC_SHAPES = [(8, 3, 92, 92), (1, 1, 5, 7), (3, 4, 33, 17)]
RC_LAYOUTS = ["contiguous", "cropped", "nhwc"]


def rc_inputs(shape, seed=900):
    n, c, h, w = shape
    albedo = (gen(n, c, h, w, seed=seed) + 1.0) * 0.5                 # [0, 1]
    albedo.view(-1)[::5] = 0.0                                        # exact zeros
    r_d = gen(n, c, h, w, seed=seed + 1, scale=3.0)
    r_s = gen(n, c, h, w, seed=seed + 2, scale=20.0)                  # exp() spans 2e-9 .. 4.9e8
    up = gen(n, c, h, w, seed=seed + 3)
    return albedo, r_d, r_s, up


def rc_oracle(albedo, r_d, r_s, up, dtype):
    with _oracle_clock():
        a, d, s = albedo.to(dtype), r_d.clone().to(dtype).requires_grad_(True), r_s.clone().to(dtype).requires_grad_(True)
        out = a * d + torch.exp(s) - 1
        out.backward(up.to(dtype))
        return out.detach(), d.grad, s.grad


def _cropped(t):
    n, c, h, w = t.shape
    wide = torch.full((n, c, h + 4, w + 6), float("nan"), device=DEV)
    wide[:, :, 2:2 + h, 3:3 + w] = t.to(DEV)
    v = wide[:, :, 2:2 + h, 3:3 + w]
    assert not v.is_contiguous()
    return v


def rc_product(layout, albedo, r_d, r_s, up):
    o = ops()
    if layout == "contiguous":
        a, d, s = albedo.to(DEV), r_d.to(DEV), r_s.to(DEV)
    elif layout == "cropped":                   # as KPCN.forward passes them
        a, d, s = _cropped(albedo), _cropped(r_d), _cropped(r_s)
    else:                                       # one NHWC-backed argument
        a, d, s = albedo.to(DEV), o.to_nhwc_raw(r_d.to(DEV)), _cropped(r_s)
        assert o.is_nhwc_view(d)
    d, s = d.detach().requires_grad_(True), s.detach().requires_grad_(True)
    out = o.recombine(a, d, s)
    out.backward(up.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), d.grad.cpu(), s.grad.cpu()


def run_recombine(shape, layouts=RC_LAYOUTS):
    albedo, r_d, r_s, up = rc_inputs(shape)
    o64, dd64, ds64 = rc_oracle(albedo, r_d, r_s, up, torch.float64)
    o32, dd32, ds32 = rc_oracle(albedo, r_d, r_s, up, torch.float32)
    # entry by entry: the forward on the scale of its terms (albedo r_d + exp(r_s) - 1 cancels), the gradients relative to
    # themselves (a zero albedo gives exactly zero)
    s_out = (albedo.double() * r_d.double()).abs() + torch.exp(r_s.double()) + 1.0
    for layout in layouts:
        case = "%s %s" % (_tag(shape), layout)
        out, dd, ds = rc_product(layout, albedo, r_d, r_s, up)
        assert bool((dd[albedo == 0] == 0).all()), case + ": d r_diffuse is not zero where the albedo is"
        hold("recombine", case, "out", elementwise(out, o64, s_out), elementwise(o32, o64, s_out), floor=FLOOR_RECOMBINE)
        hold("recombine", case, "d_diffuse", elementwise(dd, dd64, dd64.abs()), elementwise(dd32, dd64, dd64.abs()), floor=FLOOR_RECOMBINE)
        hold("recombine", case, "d_specular", elementwise(ds, ds64, ds64.abs()), elementwise(ds32, ds64, ds64.abs()), floor=FLOOR_RECOMBINE)


@pytest.mark.parametrize("shape", RC_SHAPES, ids=_tag)
def test_recombine_forward_and_gradients_against_fp64(shape):
    run_recombine(shape)


# ============================================================================ the bars have teeth
def _mutations():
    o = ops()
    return {
        "_FeatureMSE": (o._FeatureMSE, lambda: fm_three_way("fmse", "mutated", *fm_inputs(FM_BIG[0], seed=500), factor=0.1), "FeatureMSE mutated dP"),
        "_GRS": (o._GRS, lambda: fm_three_way("grs", "mutated", *fm_inputs(FM_BIG[0], seed=540), alpha=2.0), "GRS mutated dP"),
        "_KernelApply": (o._KernelApply, lambda: run_kernel_apply("normal", routes=("strip",)), "kernel_apply normal strip .* d_logits"),
        "_Recombine": (o._Recombine, lambda: run_recombine(RC_SHAPES[0], layouts=("cropped",)), "recombine .* d_diffuse"),
    }


@pytest.mark.parametrize("which", ["_FeatureMSE", "_GRS", "_KernelApply", "_Recombine"])
def test_a_one_percent_error_in_a_backward_fails_the_fp64_comparison(which, monkeypatch):
    """Precedent: tests/test_gpu_bench_config.py::test_the_gradient_bars_catch_a_one_percent_gradient_error.  The op's Python-level
    backward scales what it returns by 1.01; the benchmark-size comparison of this file must raise on that op's first gradient,
    and the hook must have run.  A bar that lets 1 % through is not a bar."""
    cls, run, first_failure = _mutations()[which]
    orig, calls = cls.backward, [0]

    def backward(ctx, *g):
        calls[0] += 1
        out = orig(ctx, *g)
        for t in (out if isinstance(out, tuple) else (out,)):
            if isinstance(t, torch.Tensor):
                t.mul_(1.01)
        return out

    n0 = len(RECORDS)
    monkeypatch.setattr(cls, "backward", staticmethod(backward))
    with pytest.raises(AssertionError, match=first_failure):
        run()
    monkeypatch.undo()
    del RECORDS[n0:]                      # figures of a mutated run are not measurements
    assert calls[0] > 0, "%s.backward never ran" % which
    run()                                 # the same comparison, unpatched, passes
