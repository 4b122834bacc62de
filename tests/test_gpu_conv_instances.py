"""Every kernel instance the split-bf16 convolution dispatch can launch, against an fp64 convolution: the rows of
tests/conv_instances.py: CASES (two or more per instance; tests/test_cpu_conv_instances.py proves, without a GPU, that each row runs
the instance it names, and this file asks the plan again with the strides it launches with).

Reference: fp64 ``F.conv2d`` (``torch.nn.grad.conv2d_weight`` for the weight gradients) on the operands the INSTANCE multiplies,
read from its name (conv_instances.planes): fp32 operands for a three-term instance, x rounded to bf16 for a two-term one, x and W
rounded for a one-term one, both rounded to fp16 for the fp16 launch -- as test_two_term_..., test_one_term_... and test_fp16_... of
tests/test_gpu_ops.py do; where the plan falls back to a more exact instance the reference follows it.  Bias, activation and gate
are applied in fp64.  The bar is the 2e-5 (max-norm relative error, test_gpu_ops.assert_close) those tests hold the same kernel
families to, for the outputs and for the column sums.

No row differentiates through an activation, so no upstream value has to be kept off a kink; the one place where a rounding may
legitimately decide a sign is the output bit mask, which is held to the reference only where |pre-activation| > 1e-4 (and to the
kernel's own hi plane everywhere).

Every row appends its errors to RECORDS; the last test prints the table and writes it to the report directory
(profiles/conv_instances_error.txt is one such run)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import conv_instances as CI                                            # noqa: E402
from oracle import modules as om                                       # noqa: E402
from test_gpu_ops import DEV, _bf16_round, assert_close, gen, ops, rel_err      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("WCMC_TEST_REPORTS", os.path.join(ROOT, "test_reports"))     # (git-ignored)
BAR = 2e-5
# Rows whose bar is derived instead (4 x the error of an fp64 emulation of the instance's split-bf16 product on the row's inputs
# against the full fp64 reference; never from the kernel's output): row -> (bar, emulation error).  None today.
DERIVED_BARS = {}
RECORDS = []            # (instance, case id, what, rel err, bar)
SENTINEL = -12345.678   # fills the wider buffer of an out=fp32-in-wider-buffer row


def _id(row):
    return "-".join(str(a) for a in row[1:10]) + "-" + row[10].replace(" ", ",")


def _seed(row):
    return 7000 + 10 * CI.CASES.index(row)


def _last_slab(cin):
    """First channel of the last 8-channel unit: the finest grain at which any instance cuts its channels into slabs."""
    return (cin - 1) // 8 * 8


# ---------------------------------------------------------------------------------------------------- forward rows
@functools.lru_cache(maxsize=None)
def _forward_inputs(row):
    _, kind, n, cin, h, w, cout, ks, pad, _, _ = row
    opt, s = CI.options(row), _seed(row)
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    x = gen(n, cin, h, w, seed=s)
    wt = gen(cout, cin, ks, ks, seed=s + 1, scale=(2.0 / (cin * ks * ks)) ** 0.5 * 1.7)
    b = gen(cout, seed=s + 2, scale=0.2) if opt["bias"] else None
    g = gen(n, cout, ho, wo, seed=s + 3) if opt["gate"] != "none" else None
    return x, wt, b, g


def _reference(row, x_ref, keep, mutate=False):
    """fp64 conv + bias + activation + gate on the operands the instance multiplies; x_ref: the x operand, already rounded as the
    instance does.  mutate: one tap of the last channel slab of the weights zeroed -- how these kernels go wrong.
    Returns (pre-activation, result)."""
    instance, _, _, cin, _, _, _, ks, pad, _, _ = row
    opt = CI.options(row)
    _, wt, b, _ = _forward_inputs(row)
    _, wp, f16 = CI.planes(instance)
    wr = (wt.half() if f16 else _bf16_round(wt) if wp == 1 else wt).double()
    if mutate:
        wr = wr.clone()
        wr[:, _last_slab(cin):, ks // 2, ks - 1] = 0.0
    pre = F.conv2d(x_ref, wr, b.double() if b is not None else None, padding=pad)
    y = om._activation(pre, opt["act"])
    if keep is None:
        return pre, y
    off = om.LEAKY_SLOPE if opt["gate_act"] == "leaky_relu" else 0.0      # what a closed gate multiplies by (include/wcmc_hip.h)
    return pre, y * torch.where(keep, torch.ones((), dtype=torch.float64), torch.full((), off, dtype=torch.float64))


def _launch_forward(row):
    """One launch of the row through ops.conv2d_x_raw / conv2d_out_f16_raw.  Returns a dictionary: y (fp32 result on the device, as
    (N, Cout, Ho, Wo)), x_ref, keep, and what the options ask for (ysplit, part, mask, wide)."""
    instance, kind, n, cin, h, w, cout, ks, pad, terms, _ = row
    o, opt = ops(), CI.options(row)
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    x, wt, b, g = _forward_inputs(row)
    ap, wp, f16 = CI.planes(instance)
    xs = o.split_raw(o.to_nhwc_raw(x.to(DEV)))
    bd = b.to(DEV) if b is not None else None
    res = {"keep": None}
    if kind == "h":
        assert f16 and o.conv_launch_plan(n, h, w, cin, cout, ks, pad, 1, False, CI.dense_strides(cout, ho, wo), f16=True)[1] == instance
        res["y"] = o.conv2d_out_f16_raw(xs, (n, cin, h, w), o._pack_x(wt.to(DEV), 4), bd, cout, ks, pad)
        res["x_ref"] = o.unsplit_debug(xs, n, cin, h, w).half().double().cpu()      # the kernel's operand: fp16 of the split value
        return res
    assert not f16
    res["x_ref"] = (x if ap == 2 else _bf16_round(x)).double()
    wpk = o._pack_x(wt.to(DEV), 0 if terms == 3 else 3)           # forward orientation; the K order follows the plan (x_plan_k)
    split = opt["out"] == "split"
    kw = {}
    if opt["gate"] == "tensor":
        gs = o.split_raw(o.to_nhwc_raw(g.to(DEV)))
        kw.update(gate=gs, gate_act=opt["gate_act"])
        res["keep"] = (o.unsplit_debug(gs, n, cout, ho, wo) > 0).cpu()
    elif opt["gate"] == "mask":
        res["keep"] = g > -0.3                                    # ~65 % of the outputs pass
        cp = (cout + 7) // 8 * 8
        bits = torch.zeros(n, ho, wo, cp, dtype=torch.bool)
        bits[..., :cout] = res["keep"].permute(0, 2, 3, 1)
        kw.update(gate_mask=torch.from_numpy(np.packbits(bits.numpy().reshape(-1, cp), axis=1, bitorder="little").reshape(-1)).to(DEV),
                  gate_act=opt["gate_act"])
    if opt["out"] == "fp32-in-wider-buffer":
        cw = (cout + 3) // 4 * 4 + CI.WIDE_EXTRA
        res["wide"] = torch.full((n, ho, wo, cw), SENTINEL, device=DEV, dtype=torch.float32)
        kw["out"] = res["wide"].permute(0, 3, 1, 2)[:, CI.WIDE_OFFSET:CI.WIDE_OFFSET + cout]
        ys = (kw["out"].stride(0), kw["out"].stride(2), kw["out"].stride(3))
        assert ys == CI.wide_strides(cout, ho, wo)
    else:
        ys = (0, 0, 0) if split else CI.dense_strides(cout, ho, wo)
    # the launch below runs the instance the row names: the plan, asked with the launch's own arguments
    assert o.conv_launch_plan(n, h, w, cin, cout, ks, pad, terms, split, ys, gate=opt["gate"] == "tensor")[1] == instance
    out = o.conv2d_x_raw(xs, (n, cin, h, w), wpk, bd, cout, ks, pad, opt["act"], out_split=split, colsum=opt["colsum"],
                         mask_out=opt["mask_out"], terms=terms, **kw)
    out = list(out) if isinstance(out, tuple) else [out]
    first = out.pop(0)
    if split:
        res["ysplit"], res["y"] = first, o.unsplit_debug(first, n, cout, ho, wo)
    else:
        res["y"] = first
    if opt["colsum"]:
        res["part"] = out.pop(0)
    if opt["mask_out"]:
        res["mask"] = out.pop(0)
    res.update(xs=xs, wpk=wpk, bd=bd)
    return res


def _bar(row):
    return DERIVED_BARS[row][0] if row in DERIVED_BARS else BAR


def _check_forward(row, record=True):
    instance, kind, n, cin, h, w, cout, ks, pad, terms, _ = row
    o, opt = ops(), CI.options(row)
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    res = _launch_forward(row)
    pre, ref = _reference(row, res["x_ref"], res["keep"])
    errs = [("y", rel_err(res["y"], ref))]
    if opt["colsum"]:
        db = o.colsum_finish_raw(res["part"], (n, cout, ho, wo))
        errs.append(("column sums", rel_err(db, ref.sum(dim=(0, 2, 3)))))
    if record:
        for what, e in errs:
            print("%s %s: %s rel err %.3e (bar %.1e)" % (instance, _id(row), what, e, _bar(row)))
            RECORDS.append((instance, _id(row), what, e, _bar(row)))
    assert tuple(res["y"].shape) == (n, cout, ho, wo) and bool(torch.isfinite(res["y"]).all())
    for what, e in errs:
        assert e <= _bar(row), "%s %s: %s rel err %.3e > %.1e" % (instance, _id(row), what, e, _bar(row))
    if opt["out"] == "split":
        # pad channels [Cout, round_up(Cout, 8)) of both planes are zeros: the consumers' loaders have no channel masks (conv_bf16x3.hip)
        cp = (cout + 7) // 8 * 8
        planes = res["ysplit"].view(torch.bfloat16).view(n, ho, wo, 2, cp)
        assert res["ysplit"].numel() == n * ho * wo * 2 * cp and bool((planes[..., cout:].float() == 0).all()), "pad channels of the split output"
    if opt["out"] == "fp32-in-wider-buffer":
        # the view contract lets a launch write [0, round_up(Cout, 4)) of a pixel of its view (include/wcmc_hip.h); every other byte keeps the sentinel
        wide = res["wide"].cpu()
        c4 = (cout + 3) // 4 * 4
        outside = torch.cat([wide[..., :CI.WIDE_OFFSET], wide[..., CI.WIDE_OFFSET + c4:]], dim=-1)
        assert outside.shape[-1] == CI.WIDE_EXTRA
        assert bool((outside.contiguous().view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32)).all()), "bytes outside the slice were written"
    if opt["mask_out"]:
        # the bit mask against the hi plane of the output (test_gate_from_bit_mask_...) and, away from the kink, against the reference
        cp = (cout + 7) // 8 * 8
        bits = torch.from_numpy(np.unpackbits(res["mask"].cpu().numpy().reshape(n * ho * wo, -1), axis=1, bitorder="little")).bool()
        hi = res["ysplit"].view(torch.bfloat16).view(n * ho * wo, 2, cp)[:, 0].float().cpu()
        assert torch.equal(bits[:, :cp], hi > 0)
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(n * ho * wo, cout)
        sure = flat(pre.abs() > 1e-4)
        assert torch.equal(bits[:, :cout][sure], flat(ref > 0)[sure]) and 0.1 < float(bits[:, :cout].float().mean()) < 0.9
        # a second launch gated by that mask == the one gated by the tensor itself, bit for bit (same instance: a gate TENSOR keeps
        # a launch off conv_pw, so the pointwise rows stop at the mask)
        if o.conv_launch_plan(n, h, w, cin, cout, ks, pad, terms, True, gate=True)[1] == instance:
            run = lambda **g: o.conv2d_x_raw(res["xs"], (n, cin, h, w), res["wpk"], res["bd"], cout, ks, pad, opt["act"], out_split=True,
                                             terms=terms, gate_act="relu", **g)
            by_tensor, by_mask = run(gate=res["ysplit"]), run(gate_mask=res["mask"])
            assert torch.equal(by_tensor, by_mask)
            want = om._activation(pre, opt["act"]) * (hi[:, :cout] > 0).reshape(n, ho, wo, cout).permute(0, 3, 1, 2).double()
            assert_close(o.unsplit_debug(by_mask, n, cout, ho, wo), want, tol=_bar(row), what="gated by its own mask")
    return res, ref


# ---------------------------------------------------------------------------------------------------- weight-gradient rows
@functools.lru_cache(maxsize=None)
def _wgrad_reference(row):
    instance, _, n, cin, h, w, cout, ks, pad, terms, _ = row
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    s = _seed(row)
    x, dy = gen(n, cin, h, w, seed=s), gen(n, cout, ho, wo, seed=s + 1)
    rounded = CI.planes(instance)[0] == 1                # a one-term instance multiplies the hi planes: the gradient of the rounded operands
    xr, dyr = (_bf16_round(x), _bf16_round(dy)) if rounded else (x, dy)
    dw = torch.nn.grad.conv2d_weight(xr.double(), (cout, cin, ks, ks), dyr.double(), padding=pad)
    return x, dy, dw, dy.double().sum(dim=(0, 2, 3))     # (the bias gradient sums hi + lo of dy whatever the terms)


def _check_wgrad(row, record=True, mutate=False):
    instance, _, n, cin, h, w, cout, ks, pad, terms, _ = row
    o, opt = ops(), CI.options(row)
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    x, dy, dw_ref, db_ref = _wgrad_reference(row)
    if mutate:
        dw_ref = dw_ref.clone()
        dw_ref[:, _last_slab(cin):, ks // 2, ks - 1] = 0.0
    assert o.wgrad_launch_plan(n, h, w, cin, cout, ks, pad, terms)[1] == instance
    xs = o.split_raw(o.to_nhwc_raw(x.to(DEV)))
    if opt["colsum"]:      # the split dy and its column sums in one pass, as a chain's backward enters; the reduction launch finishes db
        dys, part = o.split_dy_colsum_raw((n, cout, ho, wo), dy=o.to_nhwc_raw(dy.to(DEV)))
        dw, db = o.conv2d_wgrad_x_raw(xs, (n, cin, h, w), dys, cout, ks, pad, (cout, cin, ks, ks), want_bias=False, colsum_part=part, terms=terms)
    else:
        dys = o.split_raw(o.to_nhwc_raw(dy.to(DEV)))
        dw, db = o.conv2d_wgrad_x_raw(xs, (n, cin, h, w), dys, cout, ks, pad, (cout, cin, ks, ks), want_bias=opt["bias"], terms=terms)
    assert (db is None) == opt["nobias"]
    errs = [("dw", rel_err(dw, dw_ref))] + ([("db", rel_err(db, db_ref))] if db is not None else [])
    if record:
        for what, e in errs:
            print("%s %s: %s rel err %.3e (bar %.1e)" % (instance, _id(row), what, e, _bar(row)))
            RECORDS.append((instance, _id(row), what, e, _bar(row)))
    assert tuple(dw.shape) == (cout, cin, ks, ks) and bool(torch.isfinite(dw).all())
    for what, e in errs:
        assert e <= _bar(row), "%s %s: %s rel err %.3e > %.1e" % (instance, _id(row), what, e, _bar(row))


@pytest.mark.parametrize("row", CI.CASES, ids=_id)
def test_instance_against_fp64(row):
    try:
        if row[1] == "w":
            _check_wgrad(row)
        else:
            _check_forward(row)
    except RuntimeError as e:      # a device fault ends the session: nothing more is launched on a card that has faulted
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("device fault in %s %s: %s" % (row[0], _id(row), e), returncode=3)
        raise


# ---------------------------------------------------------------------------------------------------- the bar has teeth
def _ragged_row(instance):
    return next(r for r in CI.CASES if r[0] == instance and r[2] >= 2)


# one ragged row per family (and of each weight-gradient kernel)
TEETH = ("conv_pw_bf16x3_kernel<4, 10, true, 0>", "conv_halo3_bf16x3_kernel<1, 4, 2, 0>", "conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 2>",
         "conv_halo64_bf16x3_kernel<4, 3, 3, 0, 0, 2, 2, 0>", "conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 0>",
         "conv_igemm_bf16x3_kernel<7, true, true, 0>", "conv_wgrad_bf16x3_kernel<7, 2>", "conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 1>",
         "conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>")


@pytest.mark.parametrize("instance", TEETH)
def test_one_zeroed_tap_of_the_last_channel_slab_fails_the_comparison(instance):
    """The comparison of a ragged row against a reference that is wrong the way these kernels go wrong -- one tap of the last
    channel slab missing -- raises; against the true reference it passes (precedent:
    test_a_one_percent_error_in_a_backward_fails_the_fp64_comparison)."""
    row = _ragged_row(instance)
    if row[1] == "w":
        with pytest.raises(AssertionError, match="dw rel err"):
            _check_wgrad(row, record=False, mutate=True)
        _check_wgrad(row, record=False)
        return
    res = _launch_forward(row)
    _, wrong = _reference(row, res["x_ref"], res["keep"], mutate=True)
    _, true = _reference(row, res["x_ref"], res["keep"])
    with pytest.raises(AssertionError, match="rel err"):
        assert_close(res["y"], wrong, tol=_bar(row), what="zeroed tap")
    assert_close(res["y"], true, tol=_bar(row), what="true reference")


# ---------------------------------------------------------------------------------------------------- the table
def format_records():
    lines = ["# instance | case (kind-N-Cin-H-W-Cout-ks-pad-terms-options) | what | max-norm rel err against fp64 | bar"]
    for instance, case, what, e, bar in RECORDS:
        lines.append("%-52s %-90s %-11s %.3e  %.1e%s" % (instance, case, what, e, bar, "" if bar == BAR else "  (derived bar)"))
    lines.append("")
    lines.append("# largest error per instance (%d instances, %d rows)" % (len({r[0] for r in RECORDS}), len({r[1] for r in RECORDS})))
    for instance in sorted({r[0] for r in RECORDS}):
        lines.append("%-52s %.3e" % (instance, max(r[3] for r in RECORDS if r[0] == instance)))
    for row, (bar, emu) in DERIVED_BARS.items():
        lines.append("# derived bar: %s %s: fp64 emulation of the split-bf16 product %.3e against the full fp64 reference, bar 4 x = %.3e" % (row[0], _id(row), emu, bar))
    return "\n".join(lines) + "\n"


def test_error_table_of_this_run(request):
    """Printed, and written to the report directory, for whatever part of this file has run before; after the whole file every listed
    instance has been held to fp64 by every one of its rows."""
    text = format_records()
    print(text)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "conv_instances_error.txt"), "w") as f:
        f.write(text)
    assert all(e <= bar for _, _, _, e, bar in RECORDS)
    mine = [i for i in request.session.items if i.module is request.module]
    if len(mine) == len(CI.CASES) + len(TEETH) + 1:
        assert {r[0] for r in RECORDS} == set(CI.INSTANCES) and {r[1] for r in RECORDS} == {_id(r) for r in CI.CASES}
