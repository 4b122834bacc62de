"""The structural-similarity training loss on the GPU (csrc/dssim_loss.hip, ops.dssim_loss, support.losses.DSSIM / WithDSSIM,
``--dssim_weight``) against its fp64 restatement (tests/ssim_loss_ref.py).

Value: |loss - fp64| <= 2e-6, the bar of the project's SSIM kernel (section 10, tests/test_gpu_image_eval.py).
Gradient: e = max|dx - dx64| / max|dx64| <= max(4 * e_yardstick, 1e-6), where the yardstick is the fp32 torch-op evaluation of the
restatement on the same inputs and device, run here (not the code under test); 4 allows for another order in the 49-term sums and
the three box sums.  Both figures per case are written to ``test_reports/dssim_loss_error.txt`` (profiles/dssim_loss_error.txt is a
copy of one run)."""
import functools
import os

import pytest
import torch

import ssim_loss_ref as slr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("WCMC_TEST_REPORTS", os.path.join(ROOT, "test_reports"))     # (git-ignored)
DEV = "cuda:0"
VALUE_BAR, GRAD_FACTOR, GRAD_FLOOR = 2e-6, 4.0, 1e-6
RECORDS = {}

# one window | one window row / column | ragged tiles on both axes | the step's shape
SHAPES = [(1, 1, 7, 7), (1, 1, 7, 8), (3, 1, 40, 8), (2, 3, 7, 40), (1, 3, 9, 33), (1, 2, 23, 71), (8, 3, 92, 92)]
# input kinds: log-normal radiance with negative entries | the same scaled by 1e3 (tonemap none: the variance cancellation bites) |
# a crop_like view of a larger tensor | a channel-last permuted view
CASES = [(s, t, r, "radiance") for s in SHAPES for t in ("none", "reinhard") for r in (2.0, 1.0)]
CASES += [(s, "none", 2.0, "bright") for s in ((1, 1, 7, 7), (1, 3, 9, 33), (1, 2, 23, 71), (8, 3, 92, 92))]
CASES += [(s, t, 2.0, k) for s in ((2, 3, 7, 40), (1, 2, 23, 71), (8, 3, 92, 92)) for t in ("none", "reinhard") for k in ("crop", "nhwc")]


def _id(case):
    return "%s-%s-R%g-%s" % ("x".join(map(str, case[0])), case[1], case[2], case[3])


@functools.lru_cache(maxsize=None)
def _host(shape, kind):
    """(x, ref) on the host, fp32, no exact zero."""
    scale = 1e3 if kind == "bright" else 1.0
    x, r = slr.radiance(shape, 11, scale), slr.radiance(shape, 12, scale)
    x = 0.5 * (x + r) + 0.5 * (x - r) * 0.6                      # correlated with the reference, like a denoised image
    assert bool((x != 0).all()) and bool((r != 0).all()) and bool((x < 0).any())
    return x, r


@functools.lru_cache(maxsize=None)
def _reference(shape, tonemap, data_range, kind):
    """fp64 loss and gradient (CPU), computed once per case and left unchanged."""
    x, r = _host(shape, kind)
    return slr.dssim64(x, r, tonemap, data_range)


def _device_inputs(shape, kind):
    from wcmc_amd.support.utils import crop_like
    x, r = _host(shape, kind)
    if kind == "crop":                                           # the centre of a tensor 12 pixels larger, read in place
        n, c, h, w = shape
        big = [torch.full((n, c, h + 12, w + 12), float("nan")) for _ in range(2)]
        for b, t in zip(big, (x, r)):
            b[:, :, 6:6 + h, 6:6 + w] = t
        xd, rd = (crop_like(b.to(DEV), t) for b, t in zip(big, (x, r)))
        assert not xd.is_contiguous() and xd.shape == x.shape
        return xd, rd
    if kind == "nhwc":
        xd, rd = (t.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2) for t in (x, r))
        assert xd.shape == x.shape and (xd.stride(1) == 1)
        return xd, rd
    return x.to(DEV), r.to(DEV)


def _write_report():
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "dssim_loss_error.txt"), "w") as f:
        f.write("ops.dssim_loss against tests/ssim_loss_ref.py in fp64.  value: |loss - fp64| (bar %g).  grad: max|dx - dx64| / max|dx64|; "
                "'torch32': the fp32 torch-op evaluation of the restatement on the same device; bar: max(%g * torch32, %g)\n"
                % (VALUE_BAR, GRAD_FACTOR, GRAD_FLOOR))
        f.write("%-40s %11s %11s %11s %11s\n" % ("case", "value", "torch32", "grad", "torch32"))
        for name, rec in RECORDS.items():
            f.write("%-40s %11.3e %11.3e %11.3e %11.3e\n" % ((name,) + rec))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_value_and_gradient_against_fp64(case):
    from wcmc_amd import ops
    shape, tonemap, data_range, kind = case
    l64, d64 = _reference(*case)
    x, r = _device_inputs(shape, kind)
    # the yardstick: the restatement in fp32 torch ops, same inputs, same device
    xy = x.detach().clone().requires_grad_(True)
    ly = slr.dssim(xy, r, tonemap, data_range)
    ly.backward()
    scale = d64.abs().max().item()
    assert scale > 0
    ev_y, eg_y = abs(ly.item() - l64.item()), (xy.grad.double().cpu() - d64).abs().max().item() / scale
    # the kernel
    xk = x.detach().requires_grad_(True)
    lk = ops.dssim_loss(xk, r, tonemap, data_range)
    assert lk.shape == () and lk.dtype == torch.float32
    lk.backward()
    assert xk.grad.shape == x.shape
    ev, eg = abs(lk.item() - l64.item()), (xk.grad.double().cpu() - d64).abs().max().item() / scale
    RECORDS[_id(case)] = (ev, ev_y, eg, eg_y)
    _write_report()
    print("%s: value %.3e (torch32 %.3e), grad %.3e (torch32 %.3e)" % (_id(case), ev, ev_y, eg, eg_y))
    assert ev <= VALUE_BAR
    assert eg <= max(GRAD_FACTOR * eg_y, GRAD_FLOOR)


def test_known_answers():
    from wcmc_amd import ops
    # identical images: S = 1 in every window
    x = slr.radiance((2, 3, 23, 40), 3).to(DEV).requires_grad_(True)
    loss = ops.dssim_loss(x, x.detach().clone())
    loss.backward()
    assert abs(loss.item()) <= 1e-6 and x.grad.abs().max().item() <= 1e-6
    # constant planes: the variances vanish, S = (2pq + C1) / (p^2 + q^2 + C1)
    for p, q, tonemap, data_range in ((0.25, 0.75, "none", 2.0), (0.25, 0.75, "none", 1.0), (3.0, 0.5, "reinhard", 2.0)):
        a, b = torch.full((1, 2, 17, 35), p, device=DEV), torch.full((1, 2, 17, 35), q, device=DEV)
        tp, tq = (p, q) if tonemap == "none" else (p / (1 + p), q / (1 + q))
        c1 = (0.01 * data_range) ** 2
        want = 1 - (2 * tp * tq + c1) / (tp * tp + tq * tq + c1)
        assert abs(ops.dssim_loss(a, b, tonemap, data_range).item() - want) <= 2e-6
    # a plane that is negative everywhere is clamped by the tone map: no gradient reaches it
    x = slr.radiance((1, 2, 12, 40), 4).abs()
    x[:, 1] *= -1
    x = x.to(DEV).requires_grad_(True)
    ops.dssim_loss(x, slr.radiance((1, 2, 12, 40), 5).to(DEV), "reinhard").backward()
    assert bool((x.grad[:, 1] == 0).all()) and x.grad[:, 0].abs().max().item() > 0


def test_agrees_with_the_evaluation_metric():
    """One (1, 3, 40, 56) frame, Reinhard, data range 2: the ``_tonemap`` DSSIM of ``ops.image_eval`` within the two bars added."""
    from wcmc_amd import ops
    x, r = (t.to(DEV) for t in _host((1, 3, 40, 56), "radiance"))
    ev = ops.image_eval(x[0].permute(1, 2, 0), r[0].permute(1, 2, 0), r[0].permute(1, 2, 0))
    assert abs(ops.dssim_loss(x, r, "reinhard", 2.0).item() - ev[0, 1, 2].item()) <= 4e-6
    assert ev[0, 1, 2].item() > 1e-2                             # the frames differ: the comparison says something


def test_nan_pixel_gives_nan_loss():
    from wcmc_amd import ops
    x, r = (t.to(DEV) for t in _host((1, 2, 23, 71), "radiance"))
    x = x.clone()
    x[0, 1, 20, 70] = float("nan")                               # read by the last window of the last tile alone
    for tonemap in ("none", "reinhard"):
        assert torch.isnan(ops.dssim_loss(x, r, tonemap)).item()


@pytest.mark.parametrize("shape", [(8, 3, 92, 92), (1, 2, 23, 71)])
def test_two_runs_are_bitwise_equal_and_the_incoming_gradient_scales(shape):
    from wcmc_amd import ops
    x, r = (t.to(DEV) for t in _host(shape, "radiance"))
    runs = []
    for weight in (1.0, 1.0, 3.0):
        xk = x.detach().clone().requires_grad_(True)
        loss = ops.dssim_loss(xk, r)
        (weight * loss).backward()
        runs.append((loss.detach(), xk.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][1].abs().max().item() > 0
    # (3 * loss).backward(): three times dx, to the rounding of one fp32 product
    assert (runs[2][1] - 3.0 * runs[0][1]).abs().max().item() <= 3e-7 * 3.0 * runs[0][1].abs().max().item()


def test_loss_modules_run_the_kernels_and_refuse_aloud():
    from wcmc_amd import ops
    from wcmc_amd.support import losses
    x, r = (t.to(DEV) for t in _host((2, 3, 7, 40), "radiance"))
    assert torch.equal(losses.DSSIM()(x, r), ops.dssim_loss(x, r))
    assert torch.equal(losses.DSSIM("none", 1.0)(x, r), ops.dssim_loss(x, r, "none", 1.0))
    mixed = losses.WithDSSIM(torch.nn.L1Loss(), 0.25)(x, r)
    assert torch.equal(mixed, 0.75 * ops.l1_mean(x, r) + 0.25 * ops.dssim_loss(x, r))
    # a CUDA image the kernel refuses (fp64) takes the torch expression and says so once
    with pytest.warns(RuntimeWarning, match="DSSIM: dtype"):
        got = losses.DSSIM()(x.double(), r.double())
    assert abs(got.item() - slr.dssim64(x, r)[0].item()) <= 1e-12


# ------------------------------------------------------------------------------------------------- the step
ARGV = ["--desc", "d", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--train_branches", "--single_gpu", "--not_save"]
SIZES = {"dncnn_in_size": 34 + 5, "pnet_in_size": 36, "pnet_out_size": 3}


def _interface(tmp_path, name, weight):
    from wcmc_amd import train_kpcn as tk
    args = tk.check_args(tk.parse_args(ARGV + ["--save", str(tmp_path), "--model_name", name, "--dssim_weight", str(weight)]))
    torch.manual_seed(41)                                        # the same weights for every interface of this module
    itf = tk.init_model(SIZES, args, torch.device(DEV))[0][0]
    itf.iters = 1
    itf.to_train_mode()
    return itf


def _mixed64(itf, batch, br, weight):
    from wcmc_amd.support.utils import crop_like
    out = itf.last_out[br].double().cpu()
    tgt = crop_like(batch["target_" + br], itf.last_out[br]).double().cpu()
    return (1 - weight) * (out - tgt).abs().mean().item() + weight * slr.dssim(out, tgt, "reinhard", 2.0).item()


def test_one_eager_step_with_the_flag(tmp_path):
    """64 x 64 patches, batch 2, diffuse + specular: the logged branch losses are 0.5 * L1 + 0.5 * DSSIM (+ the weighted manifold
    term) of the step's own outputs, and every KPCN parameter's gradient is finite and differs from the flag-off step's."""
    from wcmc_amd.support.losses import WithDSSIM
    from wcmc_amd.synthetic import make_batch
    batch = make_batch(2, 4, 64, seed=51, device=DEV)
    grads = {}
    for weight in (0.0, 0.5):
        itf = _interface(tmp_path, "eager%g" % weight, weight)
        assert (type(itf.loss_funcs["l_diffuse"]) is WithDSSIM) == (weight > 0)
        torch.manual_seed(52)
        itf.preprocess(batch)
        itf.train_batch(batch)
        torch.cuda.synchronize()
        ld = {k: v.item() for k, v in itf.last_loss_dict.items()}
        assert itf.last_out["diffuse"].shape[2] >= 7
        for br in ("diffuse", "specular"):
            want = _mixed64(itf, batch, br, weight) + itf.w_manif * ld["l_manif_" + br]
            assert abs(ld["l_" + br] - want) <= 1e-5 * abs(want), (weight, br, ld["l_" + br], want)
        grads[weight] = {k: p.grad.detach().clone() for k, p in itf.models["dncnn"].named_parameters()}
    assert grads[0.5] and grads[0.0].keys() == grads[0.5].keys()
    for k, g in grads[0.5].items():
        assert bool(torch.isfinite(g).all()), k
        assert not torch.equal(g, grads[0.0][k]), k


def test_graphed_step_with_the_flag_equals_the_eager_step(tmp_path):
    """``--graph`` with the flag on, in the form ``halves_supported()`` selects: two replayed steps, finite losses equal to the eager
    run's.  The step is closed before the test ends (one live captured step per process: DESIGN.md section 8 item 8)."""
    from wcmc_amd.graph import GraphedTrainStep
    from wcmc_amd.synthetic import make_batch
    batches = [make_batch(2, 4, 64, seed=61 + i, device=DEV) for i in range(2)]
    logged = {}
    for graphed in (False, True):
        itf = _interface(tmp_path, "graph%d" % graphed, 0.5)
        step = None
        if graphed:
            assert itf.halves_supported()
            step = GraphedTrainStep(itf, batches[0], two_stream=itf.halves_supported())
        try:
            torch.manual_seed(62)
            rows = []
            for b in batches:
                if graphed:
                    step(b)
                else:
                    itf.preprocess(b)
                    itf.train_batch(b)
                torch.cuda.synchronize()
                rows.append({k: v.item() for k, v in itf.last_loss_dict.items()})
            if graphed:
                step.flush()
        finally:
            if step is not None:
                step.close()
        logged[graphed] = rows
    for a, b in zip(logged[False], logged[True]):
        assert a.keys() == b.keys() and {"l_diffuse", "l_specular", "l_total"} <= a.keys()
        for k in a:
            assert b[k] == b[k] and abs(b[k]) != float("inf"), k
            assert abs(a[k] - b[k]) <= 1e-5 * abs(a[k]), (k, a[k], b[k])
