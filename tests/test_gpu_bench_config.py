"""Parity of the configuration ``bench.py`` measures -- not a smaller or simpler relative of it.

``bench.build_interface`` + ``GraphedTrainStep`` with the library's default switches (split-bf16 GEMMs, forked
weight-gradient stream, forked specular stream, fused chain glue, fused 1x1 pairs, fused clip + Adam), BASELINE
configs[2] at its per-GPU shape (8 patches of 128x128, S=8), for two consecutive steps, against
``oracle.step.train_step`` on the same weights, inputs and FeatureMSE pairings (``rng='device'``, the bench's switch:
read back from the product; ``rng='cpu'``: the reference's ``torch.randperm`` stream, ``losses.py:35,50``).  What is compared, per step (``interfaces.py:122-251``):

  * every ``loss_dict`` scalar, 1e-3 relative (north star);
  * the denoised patches ``radiance / diffuse / specular`` (8,3,92,92), 1e-3 of the tensor's max (north star);
  * every parameter gradient with the flip-robust metric of ``conftest.assert_grad_close``: relative L2 and
    cosine, no fallback (the max-norm is printed for information only);
  * the parameter DELTAS of each Adam step against the oracle's (step 2 restarts the oracle from the product's
    weights, so that it compares two implementations of one step, not two networks a few sign ties apart).
"""
import copy
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from conftest import assert_grad_close, cosine, rel_l2      # noqa: E402
from oracle import step as ostep                             # noqa: E402
from oracle.models import KPCN as OKPCN                      # noqa: E402
from oracle.networks import PathNet as OPathNet              # noqa: E402

DEV = "cuda"
# Per-tensor gradient bars, no fallback, against an fp64 run of the CPU oracle (``oracle.step.train_step`` on ``.double()``
# models and batches: independent of every HIP kernel), on THREE draws (weights, biases, weight_g, batches and pairing keys all
# move with the seed).  The yardstick of a draw is the fp32 CPU ORACLE's own distance to fp64 (relative L2 per tensor): what fp32
# arithmetic costs on that draw, which no product kernel can move.  (Rounds 5-6 stated the bar as a ratio to the PRODUCT's own
# exact-fp32 run against the fp32 oracle: a defect in a kernel every mode shares -- kernel apply, the losses, weight-norm,
# recombine, pooling, clip + Adam -- raised its own yardstick and passed.  The report files still record that bar's decision.)
#     seed  mode        product vs fp64   fp32 oracle vs fp64   product vs fp32 oracle   (profiles/r07_grad_bar_fp64.txt: worst tensors)
#     0     bf16x321h   3.11e-3           2.1e-4                3.12e-3      worst / max(Y, 2e-4) = 14.7
#     1     bf16x321h   1.49e-3           2.5e-4                1.54e-3                             6.0
#     2     bf16x321h   3.12e-2           1.9e-3                3.12e-2                            16.1   (ill-conditioned: specular weight_g)
#     0     fp32        3.4e-4                                  3.0e-4       worst per-tensor ratio, floor 2e-4: 1.60
#     1     fp32        4.0e-4                                  3.9e-4                                               1.69
#     2     fp32        4.0e-3            9.3e-4                3.8e-3                                               5.31
# (B=1, tests/test_gpu_models.py::test_full_size_step_against_oracle: exact fp32 7.9e-4 from fp64, per-tensor ratio 2.3.)
# Exact fp32 MFMA (``--precision fp32``), per tensor: relative L2 to fp64 <= FP32_A x max(the fp32 oracle's for that tensor,
#   FP32_FLOOR); 1 - cos <= (that bar)^2 / 2.  FP32_A = 1.5 x the worst ratio (5.31, the ill-conditioned draw; 1.6-1.7 on the
#   others).  As good as an fp32 implementation, within a small factor.
# Default mode: relative L2 to fp64 <= min(GRAD_K x max(Y, GRAD_FLOOR), GRAD_CEIL), Y = the fp32 oracle's WORST tensor on the
#   draw; 1 - cos <= (that bar)^2 / 2 (the same distance for a small angle).  GRAD_K = 1.5 x the worst ratio (16.1); the floor
#   is the fp32 oracle's own smallest worst-tensor distance (2.1e-4), low enough that a 1 % scale error fails on a
#   well-conditioned draw (bar 6.2e-3 on seed 1).  GRAD_CEIL is held below the 3.8e-2 the rounds 5-6 bar granted on seed 2 and
#   sits 1.12 x above the measured 3.12e-2 there -- the margin that cap leaves.
# The outputs and loss scalars north_star names are held at 1e-3 against the fp32 oracle on every draw (measured 3.5e-4 / 2e-5).
FP32_A, FP32_FLOOR = 8.0, 2e-4
GRAD_K, GRAD_FLOOR, GRAD_CEIL = 25.0, 2e-4, 3.5e-2
OLD_K, OLD_FLOOR = 10.0, 5e-4                 # rounds 5-6: ratio to the product's own exact-fp32 run (recorded, not asserted)
GRAD_L2, GRAD_COS = 5e-3, 1.25e-5             # (absolute bar against the fp32 oracle on a well-conditioned draw: the C2 test below)
_RUNS = {}                                    # (mode, rng, weight_norm, seed) -> parity_report's result, unperturbed runs only
_ORACLE64 = {}                                # step 0 of the fp64 oracle per draw: it does not depend on the product
REPORT_DIR = os.environ.get("WCMC_TEST_REPORTS", os.path.join(ROOT, "test_reports"))     # (git-ignored)
FP64_SECONDS = [0.0, 0]                       # wall time spent in fp64 oracle steps by this process, and their number


def _run(mode, rng_mode, weight_norm, seed):
    """parity_report of the unperturbed step in precision `mode` (cached): (report, failures, gradients)."""
    from wcmc_amd import ops
    key = (mode, rng_mode, bool(weight_norm), int(seed))
    if key not in _RUNS:
        old = ops.PRECISION
        ops.set_precision(mode)
        try:
            _RUNS[key] = parity_report(rng_mode, weight_norm, seed=seed, pin_defaults=(mode == old))
        finally:
            ops.set_precision(old)
    return _RUNS[key]


def _fp32_yardstick(weight_norm, seed):
    """Worst per-tensor relative L2 of the exact-fp32 run against the fp32 oracle (the rounds 5-6 yardstick)."""
    return max(r[1] for r in _run("fp32", "device", weight_norm, seed)[0] if " grad " in r[0])


def _max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _grads(report):
    return [r for r in report if " grad " in r[0]]


def fp32_mode_fails(report):
    """The exact-fp32 bar: each tensor against fp64 within FP32_A x the fp32 oracle's own distance (or the floor)."""
    fails = []
    for name, _, _, _, e64, c64, y64, _ in _grads(report):
        bar = FP32_A * max(y64, FP32_FLOOR)
        if e64 > bar or c64 > 0.5 * bar * bar:
            fails.append("%s: vs fp64 rel L2 %.3e, 1-cos %.2e; bar %.3e = %.0f x max(fp32 oracle %.3e, %.0e)"
                         % (name, e64, c64, bar, FP32_A, y64, FP32_FLOOR))
    return fails


def default_bar(report):
    """(bar, Y): the default mode's relative-L2 bar against fp64 on this draw, and the fp32 oracle's worst tensor Y."""
    y = max(r[6] for r in _grads(report))
    return min(GRAD_K * max(y, GRAD_FLOOR), GRAD_CEIL), y


def default_mode_fails(report):
    bar, y = default_bar(report)
    return ["%s: vs fp64 rel L2 %.3e, 1-cos %.2e; bar %.3e (fp32 oracle's worst %.3e)" % (r[0], r[4], r[5], bar, y)
            for r in _grads(report) if r[4] > bar or r[5] > 0.5 * bar * bar]


def old_ratio_verdict(report, yard):
    """What the rounds 5-6 bar decided: rel L2 to the fp32 oracle <= OLD_K x max(yard, OLD_FLOOR), 1 - cos <= bar^2 / 2, where
    yard is the worst tensor of the PRODUCT's exact-fp32 run against the fp32 oracle on the same draw."""
    bar = OLD_K * max(yard, OLD_FLOOR)
    bad = [r[0] for r in _grads(report) if r[1] > bar or r[2] > 0.5 * bar * bar]
    return bar, bad


def write_report(fname, report, head):
    lines = ["# %s\n" % line for line in head]
    lines.append("# %-58s %-31s %-20s %s\n" % ("", "product vs fp64 (relL2, 1-cos)", "fp32 oracle vs fp64", "product vs fp32 oracle"))
    for r in sorted(report, key=lambda r: -(r[4] if len(r) > 4 else r[1])):
        if len(r) > 4:
            lines.append("%-60s %.3e  %.2e    %.3e  %.2e   %.3e  %.2e  max-norm %.2e\n" % (r[0], r[4], r[5], r[6], r[7], r[1], r[2], r[3]))
        else:
            lines.append("%-60s %.3e\n" % (r[0], r[1]))
    _write(fname, lines)


def _summary(report):
    g = _grads(report)
    w = max(g, key=lambda r: r[4])
    return ("worst tensor vs fp64 %.3e (%s); fp32 oracle's worst vs fp64 %.3e; worst vs the fp32 oracle %.3e"
            % (w[4], w[0], max(r[6] for r in g), max(r[1] for r in g)))


@pytest.mark.parametrize("rng_mode,weight_norm,seed", [("device", True, 0), ("device", True, 1), ("device", True, 2),
                                                       ("cpu", True, 1), ("device", False, 1)])
def test_benchmarked_configuration_two_steps_against_oracle(rng_mode, weight_norm, seed):
    """``weight_norm=True`` is the PathNet parametrisation ``bench.py`` runs (``config.pathnet_weight_norm``: upstream sbmc's
    ConvChain default, ``support/networks.py:18-24``), with ``weight_g`` moved off ``||weight_v||`` so that the normalisation
    acts; ``False`` the plain weights of rounds 1-4 (``bench.py --no-pathnet-weight-norm``, the line's ``other_parametrisation``
    leg).  Same bars for both.  ``rng_mode='device'`` is the switch ``bench.py`` runs with (``config.feature_mse_rng``): the pairings come from the
    keyed device bijection (``GraphedTrainStep._draw``), are read back from ``fm.static_perms`` after the replay and handed to
    the oracle; ``'cpu'`` is the reference's ``torch.randperm`` stream (``losses.py:35,50``), drawn identically on both sides."""
    from wcmc_amd import ops
    report, fails, _ = _run(ops.PRECISION, rng_mode, weight_norm, seed)
    bar, y = default_bar(report)
    yard = _fp32_yardstick(weight_norm, seed)
    old_bar, old_bad = old_ratio_verdict(report, yard)
    write_report("bench_config_parity_%s%s_seed%d.txt" % (rng_mode, "" if weight_norm else "_plain", seed), report, [
        "seed %d, default mode: %s" % (seed, _summary(report)),
        "bar against fp64: min(%g x max(%.3e, %g), %g) = %.3e" % (GRAD_K, y, GRAD_FLOOR, GRAD_CEIL, bar),
        "fp64 oracle so far in this process: %d steps, %.0f s" % (FP64_SECONDS[1], FP64_SECONDS[0]),
        "old ratio bar (rounds 5-6): %.3e against the fp32 oracle (product's exact-fp32 worst %.3e) -> %s"
        % (old_bar, yard, "PASS" if not old_bad else "FAIL %s" % old_bad[:3])])
    fails = fails + default_mode_fails(report)
    assert not fails, "\n".join(fails)


def _write(fname, lines):
    """A report file under REPORT_DIR (per-tensor rows, bars, and what the rounds 5-6 bar decided)."""
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, fname), "w") as f:
        f.write("".join(lines))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exact_fp32_mode_against_fp64_oracle(seed):
    """The product in exact fp32 MFMA arithmetic is as good as an fp32 implementation, tensor by tensor: its distance to the fp64
    oracle within FP32_A x the fp32 CPU oracle's (floor FP32_FLOOR).  The conv GEMMs are exact here, so this is the check that
    holds the kernels every precision mode shares (kernel apply, FeatureMSE, the image losses, weight-norm, recombine, the P-buffer
    cat, pooling and upsampling, clip and Adam): a 1 % scale error in any of their backwards fails it
    (test_the_gradient_bars_catch_a_one_percent_gradient_error)."""
    report, fails, _ = _run("fp32", "device", True, seed)
    f32 = fp32_mode_fails(report)
    write_report("bench_config_parity_fp32_seed%d.txt" % seed, report, [
        "seed %d, exact fp32 MFMA: %s" % (seed, _summary(report)),
        "bar per tensor: %g x max(fp32 oracle's distance to fp64, %g); %d tensors over it" % (FP32_A, FP32_FLOOR, len(f32))])
    fails = fails + f32
    assert not fails, "\n".join(fails)


def _scaled_backward(cls, counter):
    """cls.backward with every gradient it returns scaled by 1 + 1e-2, in place (a defect of 1 % in that op's backward)."""
    orig = cls.backward

    def backward(ctx, *g):
        counter[0] += 1
        out = orig(ctx, *g)
        for t in (out if isinstance(out, tuple) else (out,)):
            if isinstance(t, torch.Tensor):
                t.mul_(1.0 + 1e-2)
        return out
    return orig, staticmethod(backward)


def test_the_gradient_bars_catch_a_one_percent_gradient_error():
    """The bars have teeth: one op's Python-level backward scales its gradients by 1 + 1e-2 (patched before the step is
    captured, restored after), and the report must FAIL.  A shared op (kernel apply: every mode runs it) must fail the exact-fp32
    check; the rounds 5-6 ratio bar, whose yardstick ran through the same op, is recorded for the same defect.  An op of the
    split-bf16 path only (the KPCN / U-Net conv chains) must fail the default-mode check.  Every mutation must have run (the hook
    was called) and moved the gradients (against the unperturbed run of the same draw): none is vacuous."""
    from wcmc_amd import ops
    seed, mode = 1, ops.PRECISION
    lines = []

    def mutated(cls, m):
        counter = [0]
        orig, patched = _scaled_backward(cls, counter)
        old = ops.PRECISION
        ops.set_precision(m)
        cls.backward = patched
        try:
            rep = parity_report("device", True, seed=seed, pin_defaults=False)
        finally:
            cls.backward = orig
            ops.set_precision(old)
        assert counter[0] > 0, "%s.backward never ran in the benchmarked step (%s)" % (cls.__name__, m)
        moved = max(rel_l2(rep[2][k], g) for k, g in _run(m, "device", True, seed)[2].items())
        assert moved > 2e-3, "the %s mutation did not move the gradients (%s): %.3e" % (cls.__name__, m, moved)
        return rep, moved

    # a shared op, exact-fp32 mode: the exact-fp32 check fails
    rep32, m32 = mutated(ops._KernelApply, "fp32")
    f32 = fp32_mode_fails(rep32[0])
    lines.append("_KernelApply x 1.01, fp32: gradients moved %.3e from the unperturbed run; exact-fp32 check: %d tensors fail%s"
                 % (m32, len(f32), "" if not f32 else " (first: %s)" % f32[0]))
    # the same defect in the default mode, judged by the old ratio bar (its yardstick: the mutated exact-fp32 run) and the new one
    repd, md = mutated(ops._KernelApply, mode)
    yard = max(r[1] for r in _grads(rep32[0]))
    old_bar, old_bad = old_ratio_verdict(repd[0], yard)
    fd = default_mode_fails(repd[0])
    lines.append("_KernelApply x 1.01, %s: gradients moved %.3e; old ratio bar %.3e (mutated exact-fp32 yardstick %.3e) -> %s; "
                 "default-mode check against fp64: %d tensors fail" % (mode, md, old_bar, yard, "PASS" if not old_bad else "FAIL", len(fd)))
    # an op of the split-bf16 path only, default mode: the default-mode check fails
    reps, ms = mutated(ops._ConvChainX, mode)
    fs = default_mode_fails(reps[0])
    lines.append("_ConvChainX x 1.01, %s: gradients moved %.3e; default-mode check against fp64: %d tensors fail%s"
                 % (mode, ms, len(fs), "" if not fs else " (first: %s)" % fs[0]))
    _write("bench_config_mutations.txt", [line + "\n" for line in lines])
    assert f32, "a 1 % error in kernel apply's backward passes the exact-fp32 check"
    assert fd, "a 1 % error in kernel apply's backward passes the default-mode check"
    assert fs, "a 1 % error in the split-bf16 conv chains' backward passes the default-mode check"


def _double(batch):
    return {k: v.double() if v.is_floating_point() else v for k, v in batch.items()}


def parity_report(rng_mode, weight_norm, seed=0, pin_defaults=True, bars=None):
    """The comparison itself; returns (report rows, failures, gradients).  seed: shifts the weights' seed, the bias / weight_g draws,
    the batches and the pairing keys together (scripts/calibrate_grad_bar.py runs several to put the gradient bars on more than one
    draw).  Two oracles run beside the product on the same weights, batches and pairings: the fp32 CPU oracle (what the reference
    computes) and the same oracle in fp64 (the yardstick of both).  Gradient rows: (name, relative L2, 1 - cos, max-norm error of
    the product against the fp32 oracle, relative L2 and 1 - cos of the product against fp64, relative L2 and 1 - cos of the fp32
    oracle against fp64); the other rows: (name, error, None, None / delta error in lr).  failures: losses, outputs and Adam deltas
    against the fp32 oracle, and the per-tensor gradient bar against it when ``bars`` = (relative L2, 1 - cos) is given; the
    callers hold the gradients against fp64 (``fp32_mode_fails``, ``default_mode_fails``).  gradients: {(step, model, name): the
    product's post-clip gradient on the CPU}."""
    import bench
    from wcmc_amd import ops
    from wcmc_amd.graph import GraphedTrainStep
    from wcmc_amd.synthetic import make_batch
    assert not pin_defaults or (ops.PRECISION == os.environ.get("WCMC_PRECISION", ops.MODES[0]) and not ops.USE_SIDE_STREAM and ops.USE_BRANCH_STREAM and ops.FUSE_EMBED and ops.FUSE_FINAL), \
        "this test pins the DEFAULT switches (the ones bench.py runs with)"
    B, S, H = bench.B_PER_GPU, bench.SPP, bench.PATCH
    device = torch.device("cuda", 0)
    itf = bench.build_interface(device, None, rng=rng_mode, weight_norm=weight_norm, seed=seed)      # the bench's own constructor
    hmods = itf.models
    torch.manual_seed(0)
    omods = {"dncnn": OKPCN(39), "backbone_diffuse": OPathNet(36, weight_norm=weight_norm),
             "backbone_specular": OPathNet(36, weight_norm=weight_norm)}
    assert hmods["backbone_diffuse"].embedding.weight_norm == weight_norm and not hmods["dncnn"].diffuse.weight_norm
    # biases are zero at init (a degenerate case for bias-path bugs): give both sides the same random ones
    g = torch.Generator().manual_seed(77 + seed)
    for k, m in hmods.items():
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("bias"):
                    p.copy_((torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(device))
                if n.endswith("weight_g"):      # g = ||v|| at init (w = v): move it so that g * v / ||v|| is not the identity
                    p.mul_((torch.rand(p.shape, generator=g) * 0.6 + 0.7).to(device))
        omods[k].load_state_dict({n: v.detach().cpu().clone() for n, v in m.state_dict().items()})
    oopt = {"optim_" + k: torch.optim.Adam(m.parameters(), lr=1e-4) for k, m in omods.items()}
    # the fp64 oracle: same weights, its own Adam moments
    with torch.random.fork_rng(devices=[]):                               # (its initialisation draws leave the CPU stream alone)
        o64 = {"dncnn": OKPCN(39), "backbone_diffuse": OPathNet(36, weight_norm=weight_norm),
               "backbone_specular": OPathNet(36, weight_norm=weight_norm)}
    for k in o64:
        o64[k].load_state_dict(omods[k].state_dict())
        o64[k].double()
    oopt64 = {"optim_" + k: torch.optim.Adam(m.parameters(), lr=1e-4) for k, m in o64.items()}
    cfg = dict(use_llpm_buf=True, manif_learn=True, train_branches=True, disentanglement_option="m11r11", w_manif=0.1)
    batches = [make_batch(B, S, H, seed=40 + i + 10 * seed, device="cpu") for i in range(2)]
    dbatches = [{k: v.to(device) for k, v in b.items()} for b in batches]

    graphed = GraphedTrainStep(itf, dbatches[0])                          # capture (its warm-up draws pairings)
    p_start = {mn: {k: v.detach().cpu().clone() for k, v in m.named_parameters()} for mn, m in hmods.items()}
    for mn in omods:                                                      # warm-up runs no optimiser: still equal
        for k, q in omods[mn].named_parameters():
            assert torch.equal(p_start[mn][k], q.detach()), (mn, k)

    ho = H - 36
    torch.manual_seed(1234 + seed)
    perms = [[ostep.draw_perms(B, S, ho, ho), ostep.draw_perms(B, S, ho, ho)] for _ in range(2)]
    torch.manual_seed(1234 + seed)                                        # the graph draws the same stream, same order
    report, fails = [], []
    ograds = [{}, {}]
    hgrads = {}
    lr = 1e-4
    p_prev = {mn: dict(d) for mn, d in p_start.items()}
    fm = itf.loss_funcs["l_manif"]
    assert fm.rng == rng_mode
    for step in range(2):
        if rng_mode == "device":
            # the product draws; the oracle is handed what it drew (every permutation checked to be a bijection)
            graphed(dbatches[step])
            torch.cuda.synchronize()
            perms[step] = [(ip.cpu().clone(), ib.cpu().clone()) for ip, ib in fm.static_perms]
            for pair in perms[step]:
                for t in pair:
                    assert torch.equal(torch.sort(t).values, torch.arange(t.numel())), "device pairing is not a permutation"
            assert not torch.equal(perms[step][0][0], perms[step][1][0]) and not torch.equal(perms[step][0][1], perms[step][1][1])
            if step == 1:
                assert not torch.equal(perms[0][0][0], perms[1][0][0]), "the pairings must change from step to step"
            loss_o, out_o = ostep.train_step(omods, oopt, batches[step], cfg, perms[step])
        else:
            loss_o, out_o = ostep.train_step(omods, oopt, batches[step], cfg, perms[step])
            graphed(dbatches[step])
            torch.cuda.synchronize()
            assert torch.equal(fm.static_perms[1][0].cpu(), perms[step][1][0])
        # the fp64 oracle on the pairings just used; its first step depends on the draw alone (cached)
        key64 = (rng_mode, bool(weight_norm), int(seed))
        hit = _ORACLE64.get(key64) if step == 0 else None
        if hit is not None and all(torch.equal(a, b) for pa, pb in zip(hit[0], perms[0]) for a, b in zip(pa, pb)) and \
                all(torch.equal(hit[1][mn][k], v) for mn, d in p_start.items() for k, v in d.items()):
            g64 = hit[2]
            for k, o in oopt64.items():
                o.load_state_dict(copy.deepcopy(hit[3][k]))
        else:
            t0 = time.time()
            ostep.train_step(o64, oopt64, _double(batches[step]), cfg, perms[step])
            FP64_SECONDS[0] += time.time() - t0
            FP64_SECONDS[1] += 1
            g64 = {mn: [q.grad.detach().clone() for q in o64[mn].parameters()] for mn in o64}
            if step == 0:
                _ORACLE64[key64] = (perms[0], p_start, g64, {k: copy.deepcopy(o.state_dict()) for k, o in oopt64.items()})
        for k, v in loss_o.items():
            np.testing.assert_allclose(graphed.losses[k].item(), v.item(), rtol=1e-3, err_msg="step %d %s" % (step, k))
        for k in ("radiance", "diffuse", "specular"):
            e = _max_rel(itf.last_out[k], out_o[k])
            if e > 1e-3:
                fails.append("step %d denoised %s: %.3e" % (step, k, e))
            report.append(("step%d out %s" % (step, k), e, None, None))
        for mn in omods:
            for (k, p), (_, q), r in zip(hmods[mn].named_parameters(), omods[mn].named_parameters(), g64[mn]):
                got = p.grad.clamp(-1.0, 1.0).cpu()    # the oracle's .grad is post clip_grad_value_ (interfaces.py:260-261)
                ograds[step][(mn, k)] = q.grad.detach().clone()
                hgrads[(step, mn, k)] = got
                if bars is not None:
                    try:
                        assert_grad_close(got, q.grad, what="step %d grad %s %s" % (step, mn, k), l2=bars[0], cos=bars[1])
                    except AssertionError as err:
                        fails.append(str(err))
                report.append(("step%d grad %s %s" % (step, mn, k), rel_l2(got, q.grad), 1.0 - cosine(got, q.grad), _max_rel(got, q.grad),
                               rel_l2(got, r), 1.0 - cosine(got, r), rel_l2(q.grad, r), 1.0 - cosine(q.grad, r)))
        # The Adam step itself: parameter DELTAS of this step against the oracle's.  Adam's first step is
        # -lr * g / (|g| + eps) = -lr * sign(g): an entry whose gradient is smaller than the gradient error may go the other
        # way (2 * lr apart) in two correct implementations.  So (i) entries whose oracle gradient is well conditioned (>= half
        # the tensor's rms, in every step so far) must agree to 5 % of lr, and (ii) at most 1 % of a tensor's entries (two
        # entries for small tensors) may be such ties (more than lr / 2 apart), and in the first step every one of them must BE a
        # tie: an oracle gradient below 5 % of the tensor's rms.  "No update" or "wrong sign" fails both everywhere.
        # (Round 6: one entry -> two.  With a gradient error of ~2e-3 of the rms an entry lies within the error of zero with
        # probability ~0.16 %; over the ~130 tensors of about a hundred entries and two steps a tensor with two such entries is
        # an event of every few draws, and a change of summation order -- the exact tile heights of the KPCN launches -- met one.)
        for mn in omods:
            for (k, p), (_, q) in zip(hmods[mn].named_parameters(), omods[mn].named_parameters()):
                d_h = p.detach().cpu() - p_prev[mn][k]
                d_o = q.detach() - p_prev[mn][k]
                well = torch.ones_like(d_o, dtype=torch.bool)
                for st in range(step + 1):
                    g = ograds[st][(mn, k)]
                    well &= g.abs() >= 0.5 * g.pow(2).mean().sqrt()
                worst = float((d_h - d_o)[well].abs().max()) if bool(well.any()) else 0.0   # (a 3-entry bias may have none)
                ties = int(((d_h - d_o).abs() > 0.5 * lr).sum())
                report.append(("step%d delta %s %s" % (step, mn, k), rel_l2(d_h, d_o), None, worst / lr))
                if worst > 0.05 * lr:
                    fails.append("step %d parameter delta %s %s: %.3e lr apart on a well-conditioned entry" % (step, mn, k, worst / lr))
                if ties > max(2, d_h.numel() // 100):
                    fails.append("step %d parameter delta %s %s: %d of %d entries more than lr/2 apart" % (step, mn, k, ties, d_h.numel()))
                if step == 0 and ties:
                    g0 = ograds[0][(mn, k)]
                    big = float(g0[(d_h - d_o).abs() > 0.5 * lr].abs().max()) / max(float(g0.pow(2).mean().sqrt()), 1e-30)
                    if big > 0.05:
                        fails.append("step 0 parameter delta %s %s: an entry whose oracle gradient is %.3f of the tensor's rms went the other way" % (mn, k, big))
                if float(d_h.abs().max()) <= 0.5 * lr:
                    fails.append("step %d: parameters of %s %s did not move" % (step, mn, k))
        # Step 2 starts from the PRODUCT's weights on both sides: the ~0.1 % of entries that took the other side of a sign
        # tie above would otherwise make step 2 compare two slightly different networks (measured: up to 2.7e-3 in relative
        # L2 on the KPCN input layer) instead of two implementations of the same step.  Adam's moments stay the oracle's own.
        for mn in omods:
            with torch.no_grad():
                for (k, p), (_, q), q64 in zip(hmods[mn].named_parameters(), omods[mn].named_parameters(), o64[mn].parameters()):
                    q.copy_(p.detach().cpu())
                    q64.copy_(p.detach().cpu().double())
                    p_prev[mn][k] = p.detach().cpu().clone()
    graphed.close()
    return report, fails, hgrads


def test_c2_vanilla_full_size_graphed_step_against_oracle():
    """BASELINE configs[1]: KPCN-Vanilla (diffuse + specular, n_in = 34, no PathNet, no manifold loss), 128x128, batch 8 on one
    MI355X, default switches, one hipGraph replay: loss scalars and denoised patches at 1e-3, gradients by relative L2."""
    import types
    from wcmc_amd import KPCN, ops
    from wcmc_amd.graph import GraphedTrainStep
    from wcmc_amd.optim import FusedClipAdam
    from wcmc_amd.support.interfaces import KPCNInterface
    from wcmc_amd.support.losses import RelativeMSE
    from wcmc_amd.synthetic import make_batch
    assert ops.PRECISION == os.environ.get("WCMC_PRECISION", ops.MODES[0])      # (the default; WCMC_PRECISION probes another mode against the same bars)
    torch.manual_seed(11)
    omod = {"dncnn": OKPCN(34)}
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for n, p in omod["dncnn"].named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.2 - 0.1)
    hmod = {"dncnn": KPCN(34)}
    hmod["dncnn"].load_state_dict(omod["dncnn"].state_dict())
    hmod["dncnn"].to(DEV)
    oopt = {"optim_dncnn": torch.optim.Adam(omod["dncnn"].parameters(), lr=1e-4)}
    hopt = {"optim_dncnn": torch.optim.Adam(hmod["dncnn"].parameters(), lr=1e-4)}
    lf = {"l_diffuse": torch.nn.L1Loss(), "l_specular": torch.nn.L1Loss(), "l_recon": torch.nn.L1Loss(), "l_test": RelativeMSE()}
    itf = KPCNInterface(hmod, hopt, lf, types.SimpleNamespace(model_name="c2"), train_branches=True)
    itf.fused_optim = FusedClipAdam(hmod, hopt)
    itf.iters = 1
    itf.to_train_mode()
    batch = make_batch(8, 8, 128, seed=60, device="cpu", use_llpm=False)
    dbatch = {k: v.to(DEV) for k, v in batch.items()}
    step = GraphedTrainStep(itf, dbatch)
    loss_o, out_o = ostep.train_step(omod, oopt, batch, dict(use_llpm_buf=False, manif_learn=False, train_branches=True), None)
    step(dbatch)
    torch.cuda.synchronize()
    for k, v in loss_o.items():
        np.testing.assert_allclose(step.losses[k].item(), v.item(), rtol=1e-3, err_msg=k)
    for k in ("radiance", "diffuse", "specular"):
        assert _max_rel(itf.last_out[k], out_o[k]) <= 1e-3, k
    worst = max(((rel_l2(p.grad.clamp(-1.0, 1.0), q.grad), 1.0 - cosine(p.grad.clamp(-1.0, 1.0), q.grad), k)
                 for (k, p), (_, q) in zip(hmod["dncnn"].named_parameters(), omod["dncnn"].named_parameters())))
    print("C2 grad worst tensor: rel L2 %.3e 1-cos %.3e %s; outputs %s" %
          (worst + (" ".join("%.2e" % _max_rel(itf.last_out[k], out_o[k]) for k in ("radiance", "diffuse", "specular")),)))
    for (k, p), (_, q) in zip(hmod["dncnn"].named_parameters(), omod["dncnn"].named_parameters()):
        assert_grad_close(p.grad.clamp(-1.0, 1.0), q.grad, what="C2 grad " + k, l2=GRAD_L2, cos=GRAD_COS)
