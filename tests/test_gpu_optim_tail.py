"""The launches the captured optimiser tail replays (csrc/optim.hip, the gradient-norm kernels of csrc/elementwise.hip and the keyed
permutation of csrc/feature_mse.hip), each called directly and held to tests/glue_ref.py: clip + Adam per element along an fp64
trajectory, the step guards over their whole truth table, clip_grad_norm_ at its chunk edges, the device-keyed permutation
against its host-keyed form."""
import ctypes
import math

import pytest
import torch

import glue_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -777.0


def ops():
    from wcmc_amd import ops as _ops
    return _ops


def L():
    from wcmc_amd._lib import lib
    return lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------- clip + Adam
BIG = 4 * 4096 * 256 + 1024 + 3          # the grid-stride loop of clip_adam_kernel runs a second time above 4 096 * 256 float4s; + tail
ADAM_N = [1, 2, 3, 4, 5, 7, 1023, 4097, BIG]
ADAM_HYPER = [dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8), dict(lr=3e-4, beta1=0.8, beta2=0.95, eps=1e-6)]


def adam_compare(state, ref, what):
    p, m, v = state
    for got, want, bound, name in ((p, ref.p, ref.Ep, "p"), (m, ref.m, ref.Em, "m"), (v, ref.v, ref.Ev, "v")):
        got = got.detach().cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), "%s %s: NaN positions differ" % (what, name)
        R.assert_within(got[~nan], want[~nan], bound[~nan], "clip_adam(%s) %s" % (name, what))


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("hyper", ADAM_HYPER, ids=["default", "other"])
@pytest.mark.parametrize("n", ADAM_N)
def test_clip_adam_per_element_along_an_fp64_trajectory(n, hyper, scale):
    """Five steps against fp64 Adam after clip_grad_value_ on the launch's seven fp32 scalars (glue_ref.AdamRef; the CPU test holds
    it to torch.optim.Adam).  Bound per element and per state tensor, carried along the trajectory, safety factor 2 on every local
    term:  m: 3 rounded operations, v: 4, the update: FIVE (mul, sqrt, mul, add, div) and the subtraction -- derivation in
    AdamRef's docstring.  The clipped gradient left in `grad` is bit-equal: +-clip stay, +-Inf become +-clip, NaN stays NaN and
    reaches p, m and v of its element only; zero gradients on zero moments move nothing."""
    o = ops()
    kinds = ("edges", "nan", "zeros") if n < BIG else ("nan",)
    for kind in kinds:
        p0 = R.rnd(n, seed=20)
        ref = R.AdamRef(p0, **hyper)
        p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        for t in range(1, 6):
            gcpu = R.adam_grads(n, seed=30 + t, kind=kind) / scale
            gc = ref.step(gcpu, scale)
            g = gcpu.to(DEV)
            o.clip_adam_(p, g, m, v, t, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], grad_scale=scale)
            R.assert_bit_equal(g, gc, "clipped gradient, step %d" % t)
        adam_compare((p, m, v), ref, "n=%d %s" % (n, kind))
        if kind == "nan":
            bad = torch.isnan(p).nonzero().flatten().tolist()
            assert bad == sorted({0, n - 1}), bad
        if kind == "zeros":
            assert torch.equal(p.cpu(), p0) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0


def _dev_state(n, seed=20):
    p0 = R.rnd(n, seed=seed)
    return [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]


@pytest.mark.parametrize("guard", [None, 0.0, 1.0])
@pytest.mark.parametrize("n", [1, 5, 4097])
def test_clip_adam_dev_with_clip_adam_hyper_is_bit_equal_to_clip_adam(n, guard):
    o = ops()
    hyper = ADAM_HYPER[1]
    a, b = _dev_state(n), _dev_state(n)
    gd = None if guard is None else torch.full((1,), guard, device=DEV)
    for step in (1, 2, 1000, 100000):
        gcpu = R.adam_grads(n, seed=50 + step % 7, kind="nan" if step == 1000 else "edges") * 2
        ga, gb = gcpu.to(DEV), gcpu.to(DEV)
        before = [t.clone() for t in a]
        o.clip_adam_(a[0], ga, a[1], a[2], step, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], grad_scale=0.5, guard=gd)
        h7 = o.clip_adam_hyper(step, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"])
        assert [R.f32(x) for x in h7] == h7 and all(abs(x - y) <= 2 * R.U * abs(y) for x, y in zip(h7, R.adam_scalars(step, *[hyper[k] for k in ("lr", "beta1", "beta2", "eps")])))
        o.clip_adam_dev_(b[0], gb, b[1], b[2], torch.tensor(h7, device=DEV), grad_scale=0.5, guard=gd)
        for x, y, name in zip(a + [ga], b + [gb], ("p", "m", "v", "grad")):
            R.assert_bit_equal(y, x, "clip_adam_dev_ %s at step %d" % (name, step))
        if guard == 0.0:                     # a zero guard: nothing moves, the gradient is not even clipped
            for x, y in zip(a + [ga], before + [gcpu]):
                R.assert_bit_equal(x, y, "zero guard")
        else:
            assert not torch.equal(a[0], before[0])


def test_captured_clip_adam_dev_replays_with_refreshed_hyper():
    """What the captured step relies on: ONE captured clip_adam_dev_ launch (a single linear branch), replayed three times with `hyper`
    refreshed in place before each replay, equals three eager clip_adam_ steps bit for bit."""
    o = ops()
    n, hyper = 4097, ADAM_HYPER[0]
    hv = [hyper[k] for k in ("lr", "beta1", "beta2", "eps")]
    grads = [R.adam_grads(n, seed=60 + t) for t in range(1, 5)]
    a = _dev_state(n)
    for t in range(1, 5):
        o.clip_adam_(a[0], grads[t - 1].to(DEV), a[1], a[2], t, *hv)
    b = _dev_state(n)
    g = grads[0].to(DEV)
    h7 = torch.tensor(o.clip_adam_hyper(1, *hv), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # (warm-up outside the capture: step 1)
        o.clip_adam_dev_(b[0], g, b[1], b[2], h7)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    g.copy_(grads[1].to(DEV))
    h7.copy_(torch.tensor(o.clip_adam_hyper(2, *hv), device=DEV))
    with torch.cuda.graph(graph):
        o.clip_adam_dev_(b[0], g, b[1], b[2], h7)
    for t in (2, 3, 4):
        g.copy_(grads[t - 1].to(DEV))
        h7.copy_(torch.tensor(o.clip_adam_hyper(t, *hv), device=DEV))
        graph.replay()
    torch.cuda.synchronize()
    for x, y, name in zip(a, b, ("p", "m", "v")):
        R.assert_bit_equal(y, x, "replayed " + name)


# ---------------------------------------------------------------------------------------------------- step guards
def _guard_case(n, bad, slot, ok):
    losses = [0.25 * (i + 1) for i in range(n)]
    if bad is not None:
        losses[slot] = bad
    return losses, [1.0 + i for i in range(n)], ok


def _guard_buffers(losses, sums, ok):
    n = len(losses)
    lt = [torch.tensor(v, device=DEV) for v in losses]
    return lt, torch.tensor([ok], device=DEV), torch.tensor(sums, device=DEV), torch.full((n + 1,), SENTINEL, device=DEV)


GUARD_CASES = [(bad, where, ok) for bad in (None, R.NAN, R.INF, -R.INF) for where in ("first", "last") for ok in (0.0, 1.0)]


@pytest.mark.parametrize("n", [1, 7, 16])
def test_step_guard_truth_table(n):
    """flags[0..n], ok and sums exactly, for every loss finite / NaN / +Inf / -Inf at the first and at the last slot and ok in {0, 1}:
    under a zero guard the sums are unchanged, a non-finite loss is never added; the local / global pair with the slot passed
    straight through reproduces step_guard_ bit for bit."""
    o = ops()
    for bad, where, ok in GUARD_CASES:
        losses, sums, ok = _guard_case(n, bad, 0 if where == "first" else n - 1, ok)
        flags_w, guard_w, sums_w = R.guard_ref(losses, ok, sums)
        lt, okt, st, ft = _guard_buffers(losses, sums, ok)
        o.step_guard_(lt, okt, st, ft)
        what = "n=%d bad=%r %s ok=%r" % (n, bad, where, ok)
        assert ft.tolist() == flags_w and okt.item() == guard_w, what
        R.assert_bit_equal(st, sums_w, "sums " + what)
        lt2, okt2, st2, ft2 = _guard_buffers(losses, sums, ok)
        slot = torch.full((1,), SENTINEL, device=DEV)
        o.step_guard_local_(lt2, okt2, ft2, slot)
        assert slot.item() == 1.0 - guard_w and okt2.item() == ok and ft2.tolist()[:n] == flags_w[:n] and ft2[n].item() == SENTINEL, what
        o.step_guard_global_(lt2, slot, okt2, st2, ft2)
        assert ft2.tolist() == flags_w and okt2.item() == guard_w, what
        R.assert_bit_equal(st2, sums_w, "sums (local + global) " + what)


@pytest.mark.parametrize("ranks_bad", [0, 1, 2])
def test_step_guard_global_reads_the_rank_sum(ranks_bad):
    o = ops()
    losses, sums, ok = _guard_case(7, None, 0, 1.0)
    lt, okt, st, ft = _guard_buffers(losses, sums, ok)
    o.step_guard_global_(lt, torch.tensor([float(ranks_bad)], device=DEV), okt, st, ft)
    guard = 1.0 if ranks_bad == 0 else 0.0
    assert ft[7].item() == guard and okt.item() == guard
    want = torch.tensor(sums) + torch.tensor(losses) if guard else torch.tensor(sums)
    R.assert_bit_equal(st, want, "sums")


def test_step_guard_stays_down_until_ok_is_reset():
    o = ops()
    n = 7
    losses, sums, _ = _guard_case(n, R.NAN, 3, 1.0)
    lt, okt, st, ft = _guard_buffers(losses, sums, 1.0)
    o.step_guard_(lt, okt, st, ft)
    assert okt.item() == 0.0
    good = [torch.tensor(0.5, device=DEV) for _ in range(n)]
    o.step_guard_(good, okt, st, ft)
    assert ft.tolist() == [1.0] * n + [0.0] and okt.item() == 0.0
    R.assert_bit_equal(st, torch.tensor(sums), "sums under a guard that stays down")
    okt.fill_(1.0)
    o.step_guard_(good, okt, st, ft)
    assert ft[n].item() == 1.0 and okt.item() == 1.0
    R.assert_bit_equal(st, torch.tensor(sums) + 0.5, "sums after the reset")


@pytest.mark.parametrize("n", [0, 17])
def test_step_guards_refuse_bad_counts_and_null_losses(n):
    h = L()
    m = max(n, 1)
    lt = [torch.tensor(1.0, device=DEV) for _ in range(m)]
    arr = (ctypes.c_void_p * m)(*[t.data_ptr() for t in lt])
    ok, slot = torch.full((1,), SENTINEL, device=DEV), torch.full((1,), SENTINEL, device=DEV)
    sums, flags = torch.full((m,), SENTINEL, device=DEV), torch.full((m + 1,), SENTINEL, device=DEV)
    assert h.wcmc_step_guard(arr, n, ptr(ok), ptr(sums), ptr(flags), stream()) != 0
    assert h.wcmc_step_guard_local(arr, n, ptr(ok), ptr(flags), ptr(slot), stream()) != 0
    assert h.wcmc_step_guard_global(arr, n, ptr(slot), ptr(ok), ptr(sums), ptr(flags), stream()) != 0
    null = (ctypes.c_void_p * 3)(lt[0].data_ptr(), None, lt[0].data_ptr())
    assert h.wcmc_step_guard(null, 3, ptr(ok), ptr(sums), ptr(flags), stream()) != 0
    assert h.wcmc_step_guard_local(null, 3, ptr(ok), ptr(flags), ptr(slot), stream()) != 0
    assert h.wcmc_step_guard_global(null, 3, ptr(slot), ptr(ok), ptr(sums), ptr(flags), stream()) != 0
    torch.cuda.synchronize()
    for t in (ok, slot, sums, flags):
        assert bool((t == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- clip_grad_norm_
def _norm_clip(grads, max_norm):
    """wcmc_grad_norm_clip through the C ABI, as ops.clip_grad_norm_ calls it: returns (norm, coefficient) as fp32 values."""
    h = L()
    m = len(grads)
    numel = (ctypes.c_int64 * m)(*[g.numel() for g in grads])
    nbytes = h.wcmc_grad_norm_clip_workspace_bytes(m, numel)
    ws = torch.empty((nbytes + 3) // 4, device=DEV)
    out = torch.empty(2, device=DEV)
    assert h.wcmc_grad_norm_clip(m, (ctypes.c_void_p * m)(*[g.data_ptr() for g in grads]), numel, float(max_norm), ptr(out), ptr(ws),
                                 ws.numel() * 4, stream()) == 0
    return out[0].item(), out[1].item()


def _check_norm_clip(gcpu, max_norm, what):
    """Total norm against fp64 inside the summation-depth bound (glue_ref.grad_norm: 16 per lane, the wave's tree, 4 waves, the finish
    block, the square root); the coefficient against fp64 on the kernel's own norm (add, divide: 2 rounded operations); the scaled
    gradients per element <= 2 * 2^-24 * |g coef| on the kernel's own coefficient (ONE multiply)."""
    grads = [g.to(DEV) for g in gcpu]
    nrm, coef = _norm_clip(grads, max_norm)
    want, rel, _ = R.grad_norm(gcpu, max_norm)
    r = abs(nrm - want) / (rel * want) if want > 0 else (0.0 if nrm == 0.0 else R.INF)
    R.RATIOS["grad_norm"] = max(R.RATIOS.get("grad_norm", 0.0), r)
    print("grad_norm %s: |err| / bound = %.3f" % (what, r))
    assert r <= 1.0, (what, nrm, want)
    c64 = max_norm / (nrm + R.f32(1e-6))
    if c64 >= 1.0 + 4 * R.U:
        assert coef == 1.0, (what, coef)
    elif c64 <= 1.0 - 4 * R.U:
        assert abs(coef - c64) <= R.SAFETY * 2 * R.U * c64, (what, coef, c64)
    else:
        assert abs(coef - min(c64, 1.0)) <= R.SAFETY * 2 * R.U, (what, coef, c64)
    for g, g0 in zip(grads, gcpu):
        if coef >= 1.0:
            R.assert_bit_equal(g, g0, "unclipped gradients " + what)
        else:
            w = g0.double() * coef
            R.assert_within(g, w, R.SAFETY * R.U * w.abs(), "grad_scale " + what)
    return nrm, coef


@pytest.mark.parametrize("max_norm", [0.5, 1e4])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 8192])
def test_clip_grad_norm_at_the_chunk_edges(n, max_norm):
    _check_norm_clip([R.rnd(n, seed=70, scale=2.0)], max_norm, "n=%d max_norm=%g" % (n, max_norm))


def test_clip_grad_norm_96_tensors_and_refuses_97():
    o = ops()
    sizes = [1 + (i * 977) % 9000 for i in range(96)]
    gcpu = [R.rnd(n, seed=100 + i) for i, n in enumerate(sizes)]
    _check_norm_clip(gcpu, 3.0, "96 tensors")
    ps = [torch.zeros(n, device=DEV, requires_grad=True) for n in sizes]
    for p, g in zip(ps, gcpu):
        p.grad = g.to(DEV)
    total = o.clip_grad_norm_(ps, 3.0)
    want, rel, coef = R.grad_norm(gcpu, 3.0)
    assert abs(total.item() - want) <= rel * want
    extra = torch.zeros(3, device=DEV, requires_grad=True)
    extra.grad = torch.ones(3, device=DEV)
    with pytest.raises(NotImplementedError):
        o.clip_grad_norm_(ps + [extra], 3.0)


def test_clip_grad_norm_edge_values():
    # all-zero gradients: norm 0, untouched
    nrm, coef = _check_norm_clip([torch.zeros(5000), torch.zeros(3)], 1.0, "zeros")
    assert nrm == 0.0 and coef == 1.0
    # the norm within one ulp on either side of max_norm, and of max_norm - 1e-6 (where the coefficient crosses 1)
    one = torch.tensor(1.0)
    for centre in (1.0, 1.0 - 1e-6):
        c = torch.tensor(centre, dtype=torch.float32)
        for v in (torch.nextafter(c, 0 * one), c, torch.nextafter(c, 2 * one)):
            _check_norm_clip([v.reshape(1).clone()], 1.0, "norm %r" % v.item())
    # a +Inf gradient: what torch does on the CPU (coefficient 0: NaN at the Inf, 0 elsewhere)
    g0 = R.rnd(5000, seed=71)
    g0[17] = R.INF
    pr = torch.zeros(5000, requires_grad=True)
    pr.grad = g0.clone()
    total = torch.nn.utils.clip_grad_norm_([pr], 1.0)
    g = g0.to(DEV)
    nrm, coef = _norm_clip([g], 1.0)
    assert math.isinf(nrm) and math.isinf(total.item()) and coef == 0.0
    R.assert_bit_equal(g, pr.grad, "gradients after an infinite norm")
    assert int(torch.isnan(g).sum()) == 1 and bool(torch.isnan(g[17]))


# ---------------------------------------------------------------------------------------------------- device-keyed permutation
@pytest.mark.parametrize("n", [1, 2, 5, 64, 1000])
def test_random_permutation_dev_and_step_counter_advance(n):
    """The contract of include/wcmc_hip.h: state = {seed, step counter}; random_permutation_dev(state, slot) ==
    random_permutation(key = permutation_key(seed, counter, slot)); step_counter_advance: counter += 1."""
    o = ops()
    seed, counter = 0x1234567 + n, 41
    state = torch.tensor([seed, counter], dtype=torch.int64, device=DEV)
    outs = []
    for slot in (0, 1, 7):
        a = o.random_permutation_dev(torch.empty(n, dtype=torch.int64, device=DEV), state, slot)
        assert torch.equal(torch.sort(a).values, torch.arange(n, device=DEV)), "not a bijection"
        assert torch.equal(o.random_permutation_dev(torch.empty(n, dtype=torch.int64, device=DEV), state, slot), a)
        assert torch.equal(o.random_permutation(n, DEV, seed=o.permutation_key(seed, counter, slot)), a)
        outs.append(a)
    o.step_counter_advance(state)
    assert state.tolist() == [seed, counter + 1]
    b = o.random_permutation_dev(torch.empty(n, dtype=torch.int64, device=DEV), state, 0)
    assert torch.equal(torch.sort(b).values, torch.arange(n, device=DEV))
    assert torch.equal(o.random_permutation(n, DEV, seed=o.permutation_key(seed, counter + 1, 0)), b)
    if n >= 64:
        assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2]) and not torch.equal(outs[1], outs[2])
        assert not torch.equal(outs[0], b)
    out = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    assert L().wcmc_random_permutation_dev(ptr(out), n, ptr(state), 8, stream()) != 0          # slots are 0..7
    assert bool((out == -1).all())
