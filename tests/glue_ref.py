"""Plain-torch restatements of the glue kernels (csrc/elementwise.hip) and of the optimiser tail (csrc/optim.hip), with the
per-element error bound of every rounded operation: the yardstick of tests/test_gpu_glue.py and tests/test_gpu_optim_tail.py.
tests/test_cpu_glue_ref.py holds each reference to the torch functional it stands for, each bound to an fp32 emulation of the
kernel's own formula, and shows that a wrong variant of each op fails the comparison functions below.

Conventions
  * exact operations (selections, copies, one fp32 operation on fp32 operands) are restated in CPU fp32 and compared with
    ``assert_bit_equal``: ``torch.equal`` on the non-NaN entries, NaN positions equal;
  * rounded operations are restated in fp64 and come with a bound TENSOR  SAFETY * k * U * A(|operands|):  k = the number of
    rounded operations on the path to one output, U = 2^-24 (fp32 round to nearest), A = the same linear map on absolute
    values, SAFETY = 2 (a second rounding where an emulation has no fused multiply-add, and the second-order terms).  They
    are compared with ``assert_within``: |got - want| <= bound for EVERY element.
"""
import math

import torch

U = 2.0 ** -24
SAFETY = 2.0
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------- comparisons
def bit_equal(got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    if tuple(got.shape) != tuple(want.shape) or got.dtype != want.dtype:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(got[~gn], want[~wn]))


def assert_bit_equal(got, want, what=""):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "%s: NaN positions differ (%d got, %d wanted)" % (what, int(gn.sum()), int(wn.sum()))
    if not torch.equal(got[~gn], want[~wn]):
        bad = (got != want) & ~gn
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d entries differ, first at %s: got %r, want %r" % (what, int(bad.sum()), i, float(got[i]), float(want[i])))


def ratio(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0, x / 0 as inf): <= 1 passes."""
    got, want, bound = got.detach().double().cpu(), want.detach().double().cpu(), bound.detach().double().cpu()
    err = (got - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, INF), r)
    return float(r.max()) if r.numel() else 0.0


RATIOS = {}          # what -> largest ratio seen (tests print it; the summary quotes it)


def assert_within(got, want, bound, what=""):
    assert tuple(got.shape) == tuple(want.shape) == tuple(bound.shape), (what, got.shape, want.shape, bound.shape)
    r = ratio(got, want, bound)
    key = what.split(" ")[0]
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print("%s: max |err| / bound = %.3f" % (what, r))
    assert r <= 1.0, "%s: |err| / bound = %.3e > 1" % (what, r)


# ---------------------------------------------------------------------------------------------------- data makers
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def windows(x):
    """(N,C,H,W) -> (4,N,C,H/2,W/2): the 2x2 windows in ATen's scan order (0,0),(0,1),(1,0),(1,1)."""
    return torch.stack([x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]])


def unwindows(w):
    _, n, c, ho, wo = w.shape
    x = torch.empty(n, c, 2 * ho, 2 * wo, dtype=w.dtype)
    x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2] = w[0], w[1], w[2], w[3]
    return x


PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
POOL_KINDS = ("random", "relu", "ties", "zeros", "nan", "inf")


def pool_data(shape, kind, seed=0):
    """Max-pool inputs whose windows hold what uniform random floats never do.  Window i (flattened over n, c, y, x) gets pattern
    i mod (number of patterns), so that every pattern occurs whenever there are enough windows and the first ones always do."""
    x = rnd(*shape, seed=seed)
    w = windows(x).reshape(4, -1)
    nw = w.shape[1]
    idx = torch.arange(nw)
    if kind == "random":
        pass
    elif kind == "relu":                      # post-ReLU activations: all-zero windows, all-equal windows
        w = torch.relu(w)
        w[:, idx % 3 == 0] = 0.0
        w[:, idx % 3 == 1] = w[0, idx % 3 == 1]
    elif kind == "ties":                      # two equal maxima at each of the six position pairs
        for k, (a, b) in enumerate(PAIRS):
            sel = idx % 6 == k
            w[a, sel] = 2.0
            w[b, sel] = 2.0
    elif kind == "zeros":                     # +0.0 / -0.0 mixed: a 4-bit pattern of signs per window
        for j in range(4):
            w[j] = torch.where((idx >> j) % 2 == 1, torch.tensor(-0.0), torch.tensor(0.0))
    elif kind == "nan":                       # of every 11 windows: one NaN at each position (4), two NaNs at each pair (6), none (1)
        for j in range(4):
            w[j, idx % 11 == j] = NAN
        for k, (a, b) in enumerate(PAIRS):
            sel = idx % 11 == 4 + k
            w[a, sel] = NAN
            w[b, sel] = NAN
        if nw == 1:                           # (a single window: NaN at position 1, a larger finite value after it)
            w[:, 0] = torch.tensor([0.5, NAN, 0.75, 0.25])
    elif kind == "inf":
        w[0, idx % 5 == 0] = INF
        w[3, idx % 5 == 1] = INF
        w[:, idx % 5 == 2] = -INF
        w[1, idx % 5 == 3] = -INF
        w[2, idx % 5 == 4] = INF
        w[3, idx % 5 == 4] = INF
    else:
        raise ValueError(kind)
    return unwindows(w.reshape(4, shape[0], shape[1], shape[2] // 2, shape[3] // 2)).contiguous()


def nhwc_buffer(n, c, h, w, pad_fill, wide=None, device="cpu", valid=None):
    """An NHWC view (N,C,H,W) (channel stride 1) built by hand.  wide = (c0, ctot): the view is the channel slice [c0, c0 + c) of a
    buffer of ctot channels (both multiples of 4).  The pad lanes [c, round_up(c, 4)) and every other channel of the wide buffer
    hold ``pad_fill``; the valid lanes hold ``valid`` (a CPU (N,C,H,W) tensor) or stay at pad_fill.  Returns (view, whole buffer)."""
    c4 = (c + 3) // 4 * 4
    c0, ctot = wide if wide is not None else (0, c4)
    assert c0 % 4 == 0 and ctot % 4 == 0 and c0 + c4 <= ctot
    buf = torch.full((n, h, w, ctot), float(pad_fill), dtype=torch.float32)
    if valid is not None:
        buf[..., c0:c0 + c] = valid.permute(0, 2, 3, 1)
    buf = buf.to(device)
    return buf.permute(0, 3, 1, 2)[:, c0:c0 + c], buf


def outside(buf, c, wide=None):
    """(pad lanes, everything outside [c0, c0 + round_up(c,4))) of the whole buffer of ``nhwc_buffer``."""
    c4 = (c + 3) // 4 * 4
    c0 = wide[0] if wide is not None else 0
    b = buf.detach().cpu()
    return b[..., c0 + c:c0 + c4], torch.cat([b[..., :c0], b[..., c0 + c4:]], -1)


# ---------------------------------------------------------------------------------------------------- the cases of both test files
POOL_SHAPES = [(1, 1, 2, 2), (2, 3, 2, 6), (1, 5, 6, 2), (3, 7, 4, 10), (1, 64, 8, 8), (2, 20, 12, 16)]
UP_SHAPES = [(1, 1, 1, 1), (1, 3, 1, 5), (2, 5, 4, 1), (1, 4, 2, 2), (2, 7, 3, 5), (1, 64, 8, 8)]
CATB_SHAPES = [(1, 1, 4, 1, 1, 1), (2, 3, 8, 3, 3, 7), (1, 8, 64, 6, 4, 4), (2, 2, 4, 5, 1, 9)]          # (B, S, C1, C2, h, w)
SPP_SHAPES = [(1, 1, 4, 1, 1), (2, 3, 5, 3, 7), (1, 8, 64, 4, 4), (2, 2, 3, 1, 9)]                        # (B, S, C, h, w)
PB_W = [1, 63, 64, 65, 130]
PB_REST = [(s, h, cb, cp) for s in (2, 3, 8) for h in (1, 5) for cb in (1, 34) for cp in (1, 2, 3, 6)]


# ---------------------------------------------------------------------------------------------------- max-pool
def maxpool2_index(x, tie="first", nan="propagate"):
    """(max, index in window order) by ATen's rule: the running maximum is replaced by a larger value or by a NaN.  tie = "last"
    and nan = "drop" are the WRONG variants (>= instead of >; no NaN clause, what fmaxf does)."""
    w = windows(x)
    m, k = w[0].clone(), torch.zeros(w[0].shape, dtype=torch.int64)
    for j in range(1, 4):
        upd = (w[j] >= m) if tie == "last" else (w[j] > m)
        if nan == "propagate":
            upd = upd | torch.isnan(w[j])
        else:
            upd = upd | (torch.isnan(m) & ~torch.isnan(w[j]))        # fmaxf: the non-NaN operand wins
        m = torch.where(upd, w[j], m)
        k = torch.where(upd, torch.full_like(k, j), k)
    return m, k


def maxpool2_fwd(x, **kw):
    return maxpool2_index(x, **kw)[0]


def maxpool2_bwd(x, dy, add=None, **kw):
    """dx: dy goes to the selected position, zero elsewhere; + add (the skip connection's gradient) in ONE fp32 add."""
    _, k = maxpool2_index(x, **kw)
    g = torch.stack([torch.where(k == j, dy, torch.zeros_like(dy)) for j in range(4)])
    dx = unwindows(g)
    return dx if add is None else add + dx


# ---------------------------------------------------------------------------------------------------- bilinear x2
def up_matrix(L, clamp=True):
    """(2L, L) fp64: one axis of bilinear x2 with align_corners=False.  out[2i] = .25 in[i-1] + .75 in[i], out[2i+1] = .75 in[i] +
    .25 in[i+1], neighbour index clamped to the image (clamp=False, the WRONG variant, drops the tap instead)."""
    m = torch.zeros(2 * L, L, dtype=torch.float64)
    for f in range(2 * L):
        i = f // 2
        nb = i + 1 if f % 2 else i - 1
        m[f, i] += 0.75
        if clamp:
            nb = min(max(nb, 0), L - 1)
        if 0 <= nb < L:
            m[f, nb] += 0.25
    return m


UP_FWD_K, UP_BWD_K = 4, 16


def upsample2_fwd(x, clamp=True):
    """(fp64 result, bound).  The kernel forms  fl(.5625 v00) then three fused multiply-adds (.1875 v01, .1875 v10, .0625 v11): the
    weights are dyadic and exact, so FOUR rounded operations, each relative to a partial sum that |.|-sums bound:
    |err| <= 4 U A(|x|), A = the same interpolation of the absolute values."""
    my, mx = up_matrix(x.shape[2], clamp), up_matrix(x.shape[3], clamp)
    f = lambda t: torch.einsum("yi,ncij,xj->ncyx", my, t.double(), mx)       # noqa: E731
    return f(x), SAFETY * UP_FWD_K * U * f(x.abs())


def upsample2_bwd(dy, clamp=True):
    """(fp64 result, bound).  dx[i] gathers from <= 4 x 4 fine pixels (up_taps: <= 4 per axis), one fused multiply-add each with
    an exact dyadic weight product, starting from 0: at most SIXTEEN rounded operations: |err| <= 16 U A^T(|dy|)."""
    my, mx = up_matrix(dy.shape[2] // 2, clamp), up_matrix(dy.shape[3] // 2, clamp)
    f = lambda t: torch.einsum("yi,ncyx,xj->ncij", my, t.double(), mx)       # noqa: E731
    return f(dy), SAFETY * UP_BWD_K * U * f(dy.abs())


def upsample2_fwd_fp32(x):
    """fp32 emulation of upsample2_fwd_kernel: same taps, same order (two roundings per multiply-add instead of one)."""
    n, c, h, w = x.shape
    fy, fx = torch.arange(2 * h), torch.arange(2 * w)
    iy, ix = fy // 2, fx // 2
    ny = torch.where(fy % 2 == 1, (iy + 1).clamp(max=h - 1), (iy - 1).clamp(min=0))
    nx = torch.where(fx % 2 == 1, (ix + 1).clamp(max=w - 1), (ix - 1).clamp(min=0))
    g = lambda yy, xx: x[:, :, yy][:, :, :, xx]                              # noqa: E731
    r = 0.5625 * g(iy, ix)
    r = r + 0.1875 * g(iy, nx)
    r = r + 0.1875 * g(ny, ix)
    return r + 0.0625 * g(ny, nx)


def upsample2_bwd_fp32(dy):
    """fp32 emulation of upsample2_bwd_kernel: the taps of up_taps in its order, accumulated from 0."""
    n, c, h2, w2 = dy.shape
    h, w = h2 // 2, w2 // 2

    def taps(i, L):
        t = [(2 * i, 1.0 if i == 0 else 0.75), (2 * i + 1, 1.0 if i == L - 1 else 0.75)]
        if i > 0:
            t.append((2 * i - 1, 0.25))
        if i < L - 1:
            t.append((2 * i + 2, 0.25))
        return t
    dx = torch.zeros(n, c, h, w)
    for y in range(h):
        for x in range(w):
            acc = torch.zeros(n, c)
            for fy_, wy in taps(y, h):
                for fx_, wx in taps(x, w):
                    acc = acc + (wy * wx) * dy[:, :, fy_, fx_]
            dx[:, :, y, x] = acc
    return dx


# ---------------------------------------------------------------------------------------------------- spp mean / broadcast / cat
def spp_reduce(x, s, scale):
    """(B*S,C,H,W) -> (B,C,H,W): scale * sum over the S samples.  Kernel: S sequential adds from 0 (the first is exact) and one
    multiply: <= S rounded operations; the bar the issue sets is (S + 1) U sum|v| scale."""
    bs, c, h, w = x.shape
    v = x.double().view(bs // s, s, c, h, w)
    return v.sum(1) * scale, SAFETY * (s + 1) * U * v.abs().sum(1) * scale


def spp_reduce_fp32(x, s, scale):
    bs, c, h, w = x.shape
    v = x.view(bs // s, s, c, h, w)
    acc = torch.zeros(bs // s, c, h, w)
    for i in range(s):
        acc = acc + v[:, i]
    return torch.tensor(scale, dtype=torch.float32) * acc


def spp_broadcast(g, s, scale, into=None):
    """(B,C,H,W) -> (B*S,C,H,W): fl(scale * g) repeated over the samples -- ONE fp32 multiply by the fp32 scale (exact restatement in
    CPU fp32; torch's mean backward DIVIDES by S instead, equal for S a power of two and within one rounding otherwise); with
    ``into`` (accumulate = 1) one fp32 add on top."""
    v = (torch.tensor(scale, dtype=torch.float32) * g).repeat_interleave(s, 0)
    return v if into is None else v + into


def cat_channels(a, b):
    return torch.cat([a, b], 1)


def cat_broadcast(flat, prop, s):
    """networks.py:39-40: cat([flat, repeat_S(prop)], 1)."""
    return torch.cat([flat, prop.repeat_interleave(s, 0)], 1)


# ---------------------------------------------------------------------------------------------------- P-buffer cat
def pvar_and_bound(p):
    """fp64 p.var(1).mean(1, keepdim)/S of a (B,S,Cp,H,W) tensor and the bound of the kernels' TWO-PASS fp32 evaluation.

    Kernel, per channel:  s1 = x_0 + ... + x_{S-1} (S - 1 rounded adds),  mh = fl(s1 / S);  d_s = fl(x_s - mh);
    s2 = sum fl(d_s^2) (S - 1 rounded adds);  v_c = fl(s2 / (S - 1)).  Then varsum = sum_c v_c (<= Cp adds), / Cp, / S.
      * mh = mean + e with |e| <= em := S U sum|x_s| / S  (S - 1 adds and the division).
      * In exact arithmetic sum (x_s - mean - e)^2 = sum (x_s - mean)^2 + S e^2, because the deviations sum to zero: the error
        of the mean enters in SECOND order only.  That is what the two passes buy; a one-pass E[x^2] - mean^2 loses
        U mean^2 / sigma^2 relative instead.  shift_c := S em^2 / (S - 1).
      * d_s is one correctly rounded subtraction: relative error U OF d_s (not of x_s), so d_s^2 carries 2 U, its rounding U, the
        sequential sum <= (S - 1) U, the division U:  v_c is (S + 3) U relative to the shifted sum.
      * varsum: Cp adds from 0 and two divisions: (Cp + 2) U more.
    |err| <= (S + Cp + 5) U (want + shift) + shift,   shift = sum_c shift_c / (Cp S)  --  of relative size (S U |mean| / sigma)^2."""
    b, s, cp, h, w = p.shape
    x = p.double()
    want = x.var(1).mean(1, keepdim=True) / s
    em = s * U * x.abs().sum(1) / s
    shift = (s * em * em / (s - 1)).sum(1, keepdim=True) / (cp * s)
    return want, SAFETY * ((s + cp + 5) * U * (want + shift) + shift)


def pmean_and_bound(p):
    s = p.shape[1]
    x = p.double()
    return x.mean(1), SAFETY * (s + 1) * U * x.abs().sum(1) / s


def pbuffer_cat(base, p, biased=False):
    """interfaces.py:165-176: cat([base, P.mean(1), P.var(1).mean(1, keepdim)/S], 1) in fp64 with its bound (0 on the copied
    channels: they are exact).  biased=True is the WRONG variant (divides by S instead of S - 1)."""
    s = p.shape[1]
    mean, bm = pmean_and_bound(p)
    var, bv = pvar_and_bound(p)
    if biased:
        var = p.double().var(1, unbiased=False).mean(1, keepdim=True) / s
    want = torch.cat([base.double(), mean, var], 1)
    return want, torch.cat([torch.zeros_like(base, dtype=torch.float64), bm, bv], 1)


def pstats_fp32(p, one_pass=False):
    """fp32 emulation of the statistics of pbuffer_cat_fwd_kernel / sample_cat_kernel (one_pass=True: the formula they avoid)."""
    b, s, cp, h, w = p.shape
    s1 = torch.zeros(b, cp, h, w)
    for i in range(s):
        s1 = s1 + p[:, i]
    mean = s1 / float(s)
    s2 = torch.zeros(b, cp, h, w)
    if one_pass:
        for i in range(s):
            s2 = s2 + p[:, i] * p[:, i]
        s2 = s2 - float(s) * mean * mean
    else:
        for i in range(s):
            d = p[:, i] - mean
            s2 = s2 + d * d
    v = s2 / float(s - 1)
    acc = torch.zeros(b, h, w)
    for c in range(cp):
        acc = acc + v[:, c]
    return mean, (acc / float(cp) / float(s)).unsqueeze(1)


def pbuffer_cat_bwd(g, s, cb, cp):
    """d P: fl(g[:, cb:cb+cp] * fl(1/S)) for every sample -- one fp32 multiply, restated exactly in CPU fp32 (B,S,Cp,H,W)."""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(s), dtype=torch.float32)
    return (g[:, cb:cb + cp] * inv).unsqueeze(1).expand(-1, s, -1, -1, -1).contiguous()


def sample_cat(features, p):
    """interfaces.py:394-403: cat([features, P, repeat_S(P.var(1).mean(1, keepdims)/S)], 2) in fp64 with its bound."""
    s = p.shape[1]
    var, bv = pvar_and_bound(p)
    want = torch.cat([features.double(), p.double(), var.unsqueeze(1).expand(-1, s, -1, -1, -1)], 2)
    z = lambda t: torch.zeros_like(t, dtype=torch.float64)                  # noqa: E731
    return want, torch.cat([z(features), z(p), bv.unsqueeze(1).expand(-1, s, -1, -1, -1)], 2)


def pdata(b, s, cp, h, w, seed=0):
    """P-buffer samples with the two pixels rounding is judged at: pixel 0 of every row has |mean| = 100 sigma (a one-pass variance
    loses ~1e-3 there), the last pixel of every row is constant over the samples with a short mantissa (variance exactly 0)."""
    p = rnd(b, s, cp, h, w, seed=seed)
    p[..., 0] = 100.0 + p[..., 0]
    if w > 1:
        p[..., w - 1] = (torch.arange(cp, dtype=torch.float32).view(1, 1, cp, 1) + 1.0) / 64.0
    return p


# ---------------------------------------------------------------------------------------------------- clip + Adam
def f32(v):
    return float(torch.tensor(v, dtype=torch.float64).float())


def adam_scalars(step, lr, beta1, beta2, eps):
    """The seven host scalars of wcmc_clip_adam, each rounded to fp32 as the launch passes them."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return [f32(lr / bc1), f32(beta1), f32(beta2), f32(1.0 - beta1), f32(1.0 - beta2), f32(eps), f32(1.0 / math.sqrt(bc2))]


def clamp_grad(g, clip, nan="propagate"):
    """clip_grad_value_ = torch.clamp: NaN stays NaN, +-Inf becomes +-clip.  nan = "minmax" is the WRONG variant (fminf(fmaxf()))."""
    if nan == "minmax":
        return torch.where(torch.isnan(g), torch.full_like(g, -clip), g.clamp(-clip, clip))
    return g.clamp(-clip, clip)


class AdamRef:
    """fp64 Adam after clip_grad_value_ on the kernel's fp32 scalars, and the per-element bound of the fp32 kernel along the
    trajectory.  The kernel, per element and step (no contraction: the library is built with -ffp-contract=off):
        gc = clamp(fl(g * grad_scale))                         exact for the power-of-two scales tested
        m  = fl(fl(b1 m) + fl(omb1 gc))                        3 rounded operations
        v  = fl(fl(b2 v) + fl(fl(omb2 gc) gc))                 4
        p  = fl(p - fl(fl(ss m) / fl(fl(sqrt(v) ibc) + eps)))  the FIVE of the update (mul, sqrt, mul, add, div) and the subtraction
    The errors Em, Ev, Ep of the carried state obey (first order, SAFETY on every local rounding term)
        Em <- b1 Em + 3 U (b1 |m| + omb1 |gc|)
        Ev <- b2 Ev + 4 U (b2 v + omb2 gc^2)
        dD  = ibc min(sqrt(Ev), Ev / (2 sqrt(max(v - Ev, 0)))) + 3 U D          D = sqrt(v) ibc + eps >= eps
        du  = ss Em / Dlow + |u| dD / Dlow + 2 U |u|                            u = ss m / D, Dlow = max(D - dD, eps)
        Ep <- Ep + du + U |p|
    wrong = "no_bc2" is the WRONG variant without the bias correction of v."""

    def __init__(self, p, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip=1.0, wrong=None):
        self.p = p.double().clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.Ep, self.Em, self.Ev = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.h = (lr, beta1, beta2, eps)
        self.clip, self.wrong, self.t = clip, wrong, 0

    def step(self, g, grad_scale=1.0):
        """g: fp32 gradient as handed to the kernel.  Returns the clipped fp32 gradient the kernel leaves behind."""
        self.t += 1
        ss, b1, b2, omb1, omb2, eps, ibc = adam_scalars(self.t, *self.h)
        if self.wrong == "no_bc2":
            ibc = 1.0
        gc32 = clamp_grad(g * torch.tensor(grad_scale, dtype=torch.float32), self.clip, "minmax" if self.wrong == "minmax" else "propagate")
        gc = gc32.double()
        k = SAFETY * U
        self.Em = b1 * self.Em + 3 * k * (b1 * self.m.abs() + omb1 * gc.abs())
        self.Ev = b2 * self.Ev + 4 * k * (b2 * self.v + omb2 * gc * gc)
        self.m = b1 * self.m + omb1 * gc
        self.v = b2 * self.v + omb2 * gc * gc
        D = self.v.sqrt() * ibc + eps
        lo = (self.v - self.Ev).clamp_min(0).sqrt()
        dsq = torch.minimum(self.Ev.sqrt(), torch.where(lo > 0, self.Ev / (2 * lo), torch.full_like(lo, INF)))
        dD = ibc * dsq + 3 * k * D
        Dlow = (D - dD).clamp_min(eps)
        u = ss * self.m / D
        du = ss * self.Em / Dlow + u.abs() * dD / Dlow + 2 * k * u.abs()
        self.p = self.p - u
        self.Ep = self.Ep + du + k * self.p.abs()
        return gc32


def adam_fp32_step(p, g, m, v, t, h, clip=1.0, grad_scale=1.0):
    """fp32 emulation of clip_adam_kernel, in place, operation for operation."""
    ss, b1, b2, omb1, omb2, eps, ibc = [torch.tensor(x, dtype=torch.float32) for x in adam_scalars(t, *h)]
    gc = clamp_grad(g * torch.tensor(grad_scale, dtype=torch.float32), clip)
    g.copy_(gc)
    m.copy_(b1 * m + omb1 * gc)
    v.copy_(b2 * v + omb2 * gc * gc)
    p.sub_(ss * m / (v.sqrt() * ibc + eps))


def adam_grads(n, seed, clip=1.0, kind="edges"):
    """Gradients with the values the clamp and the update are judged at, cycled over the elements: +-clip exactly, +-Inf, beyond
    the clip, inside it, and zeros (kind "zeros": all zero -- with zero moments the update is exactly 0; kind "nan": a NaN at
    element 0 and at the last element)."""
    g = rnd(n, seed=seed, scale=3.0)
    if kind == "zeros":
        return torch.zeros(n)
    pat = torch.tensor([clip, -clip, INF, -INF, 0.0])
    i = torch.arange(n)
    sel = i % 7 < 5
    g[sel] = pat[(i % 7)[sel]]
    if kind == "nan":
        g[0] = NAN
        g[n - 1] = NAN
    return g


# ---------------------------------------------------------------------------------------------------- step guard
def guard_ref(losses, ok, sums, add_nan=False):
    """wcmc_step_guard on python floats: (flags[0..n], ok, sums).  sums[i] += loss_i in ONE fp32 add under the guard; add_nan=True
    is the WRONG variant that adds whatever the loss holds."""
    fin = [math.isfinite(v) for v in losses]
    guard = float(ok) if all(fin) else 0.0
    new = torch.tensor(sums, dtype=torch.float32).clone()
    if guard != 0.0 or add_nan:
        new = new + torch.tensor(losses, dtype=torch.float32)
    return [1.0 if f else 0.0 for f in fin] + [guard], guard, new


# ---------------------------------------------------------------------------------------------------- clip_grad_norm_
GN_CHUNK = 4096


def grad_norm(grads, max_norm):
    """(fp64 total norm, its relative bound, fp64 clamped coefficient).  Every block sums one 4096-element chunk: a lane squares and
    adds 16 values (1 + 15 rounded operations on the deepest path... 16 counted), the wave's xor tree 6, the 4 waves 3; the finish
    block adds ceil(blocks / 256) partials per lane, 6, 3: all terms are >= 0, so the sum of squares is
    (16 + 1 + 6 + 3 + ceil(blocks/256) + 6 + 3) U relative, the square root halves that and adds its own U."""
    blocks = sum(-(-g.numel() // GN_CHUNK) for g in grads)
    depth = 16 + 1 + 6 + 3 + -(-blocks // 256) + 6 + 3
    nrm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    return nrm, SAFETY * (depth / 2.0 + 1.0) * U, min(1.0, max_norm / (nrm + 1e-6))
