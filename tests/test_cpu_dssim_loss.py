"""The structural-similarity training loss without a GPU: the fp64 restatement against the SSIM yardstick of
the evaluation, the closed-form gradient against autograd, the new entry points in the header, the binding and the built library,
their argument checks (which precede any HIP call), the torch route of the loss modules and the launchers' flag."""
import ctypes
import os
import re

import pytest
import torch

import image_eval_ref as ier
import ssim_loss_ref as slr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wcmc_dssim_loss_workspace_bytes", "wcmc_dssim_loss_fwd", "wcmc_dssim_loss_bwd")
SHAPES = [(1, 1, 7, 7), (1, 1, 7, 8), (3, 1, 40, 8), (1, 3, 9, 33), (2, 2, 23, 31)]


def test_restatement_equals_the_evaluation_yardstick():
    """One 3-channel frame, Reinhard, data range 2: the loss is 1 - image_eval_ref.ssim of the tm_reinhard images."""
    for seed, (h, w) in enumerate([(40, 56), (7, 7), (9, 11)]):
        x, r = slr.radiance((1, 3, h, w), seed), slr.radiance((1, 3, h, w), 100 + seed)
        a, b = (ier.tm_reinhard(t[0].permute(1, 2, 0).numpy()) for t in (x, r))
        got = slr.dssim(x.double(), r.double(), "reinhard", 2.0).item()
        assert abs(got - (1.0 - ier.ssim(a, b))) <= 1e-12, (h, w)
    assert abs(got - (1.0 - ier.ssim_direct(a, b))) <= 1e-12            # the explicit 7x7 loop, at 9 x 11
    # without a tone map the restatement is the SSIM of the raw images
    raw = slr.dssim(x.double(), r.double(), "none", 2.0).item()
    assert abs(raw - (1.0 - ier.ssim_direct(x[0].permute(1, 2, 0).numpy(), r[0].permute(1, 2, 0).numpy()))) <= 1e-12


@pytest.mark.parametrize("tonemap", ["none", "reinhard"])
@pytest.mark.parametrize("shape", SHAPES)
def test_three_box_sums_equal_autograd(shape, tonemap):
    x, r = slr.radiance(shape, 1), slr.radiance(shape, 2)
    for data_range, g in ((2.0, 1.0), (1.0, 3.0)):
        _, want = slr.dssim64(x, r, tonemap, data_range)
        got = slr.box_gradient(x, r, tonemap, data_range, g)
        assert (got - g * want).abs().max().item() <= 1e-12 * max(1.0, g * want.abs().max().item())
        assert want.abs().max().item() > 0
    if tonemap == "reinhard":
        assert (got[x < 0] == 0).all() and bool((x < 0).any())          # a clamped pixel receives no gradient


def test_new_symbols_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from wcmc_amd._lib import SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "wcmc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(wcmc_[a-z0-9_]+)\s*\(", header))
    h = lib()
    for name in NEW:
        assert name in declared and name in SIGNATURES, name
        assert getattr(h, name) is not None
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert len(m.group(1).split(",")) == len(SIGNATURES[name][1]), name
    assert h.wcmc_abi_version() == 4
    # one fp64 partial sum per 32 x 8 tile of windows and plane
    assert h.wcmc_dssim_loss_workspace_bytes(8, 3, 92, 92) == 24 * 3 * 11 * 8
    assert h.wcmc_dssim_loss_workspace_bytes(1, 1, 7, 7) == 8
    assert h.wcmc_dssim_loss_workspace_bytes(8, 3, 6, 92) == 0
    assert h.wcmc_dssim_loss_workspace_bytes(8, 3, 92, 6) == 0
    assert h.wcmc_dssim_loss_workspace_bytes(0, 3, 92, 92) == 0
    assert h.wcmc_dssim_loss_workspace_bytes(65536, 1, 92, 92) == 0
    from wcmc_amd import ops
    assert ops.dssim_loss is ops.image.dssim_loss and ops.DSSIM_TONEMAPS == {"none": 0, "reinhard": 1}
    assert ops.dssim_loss_supported(8, 3, 92, 92) and not ops.dssim_loss_supported(8, 3, 6, 92)


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Every refusal of the C ABI: the library's error code, a message that names the entry point, nothing launched (the checks
    precede every HIP call, so this runs without a GPU)."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)     # `one`: non-null, never dereferenced by the checks
    good = dict(x=one, ref=one, tonemap=1, data_range=2.0, loss=one, ws=one, ws_bytes=1 << 20, grad=one, dx=one, N=2, C=3, H=9, W=11)

    def fwd(**kw):
        a = dict(good, **kw)
        return L.wcmc_dssim_loss_fwd(a["x"], 297, 99, 11, 1, a["ref"], 297, 99, 11, 1, a["tonemap"], a["data_range"], a["loss"],
                                     a["ws"], a["ws_bytes"], a["N"], a["C"], a["H"], a["W"], null)

    def bwd(**kw):
        a = dict(good, **kw)
        return L.wcmc_dssim_loss_bwd(a["x"], 297, 99, 11, 1, a["ref"], 297, 99, 11, 1, a["tonemap"], a["data_range"], a["grad"],
                                     a["dx"], a["N"], a["C"], a["H"], a["W"], null)
    common = {"H < 7": dict(H=6), "W < 7": dict(W=6), "unknown tone map": dict(tonemap=2), "negative tone map": dict(tonemap=-1),
              "data_range 0": dict(data_range=0.0), "data_range < 0": dict(data_range=-1.0), "data_range nan": dict(data_range=float("nan")),
              "null x": dict(x=null), "null ref": dict(ref=null), "N = 0": dict(N=0), "too many planes": dict(N=65536, C=1)}
    for call, who, own in ((fwd, "dssim_loss_fwd", {"null loss": dict(loss=null), "null workspace": dict(ws=null)}),
                           (bwd, "dssim_loss_bwd", {"null grad_loss": dict(grad=null), "null dx": dict(dx=null)})):
        for what, kw in dict(common, **own).items():
            assert call(**kw) == -1, (who, what)                                 # WCMC_ERR_BAD_ARG
            assert who in L.wcmc_last_error().decode(), (who, what)
    assert "7 x 7" in (fwd(H=6), L.wcmc_last_error().decode())[1]
    need = L.wcmc_dssim_loss_workspace_bytes(2, 3, 9, 11)
    assert need == 6 * 8
    assert fwd(ws_bytes=need - 1) == -3                                          # WCMC_ERR_WORKSPACE
    msg = L.wcmc_last_error().decode()
    assert "dssim_loss_fwd" in msg and "workspace" in msg and str(need) in msg


def test_python_side_refusals():
    from wcmc_amd import ops
    x = torch.zeros(1, 3, 9, 9)
    with pytest.raises(ValueError, match="tonemap 'gamma'"):
        ops.dssim_loss(x, x, tonemap="gamma")
    with pytest.raises(Exception):                                               # no CPU path in the ops package
        ops.dssim_loss(x, x)


@pytest.mark.parametrize("tonemap", ["none", "reinhard"])
def test_loss_modules_take_the_torch_expression_on_cpu_tensors(tonemap):
    from wcmc_amd.support import losses
    assert "DSSIM" in losses.__all__ and "WithDSSIM" in losses.__all__
    x, r = slr.radiance((2, 3, 23, 31), 5), slr.radiance((2, 3, 23, 31), 6)
    for data_range in (2.0, 1.0):
        want, dwant = slr.dssim64(x, r, tonemap, data_range)
        xd = x.double().requires_grad_(True)
        got = losses.DSSIM(tonemap, data_range)(xd, r.double())
        assert abs(got.item() - want.item()) <= 1e-14
        got.backward()
        assert (xd.grad - dwant).abs().max().item() <= 1e-14
        mixed = losses.WithDSSIM(torch.nn.L1Loss(), 0.25, tonemap, data_range)(x.double(), r.double())
        l1 = (x.double() - r.double()).abs().mean()
        assert abs(mixed.item() - (0.75 * l1 + 0.25 * want).item()) <= 1e-14
    # any module is a base; the weights' ends
    base = losses.TonemappedRelativeMSE()
    assert torch.equal(losses.WithDSSIM(base, 0.0)(x, r), base(x, r) + 0.0 * losses.DSSIM()(x, r))
    assert abs(losses.WithDSSIM(base, 1.0)(x.double(), r.double()).item() - slr.dssim64(x, r)[0].item()) <= 1e-14
    with pytest.raises(ValueError, match="weight should be in"):
        losses.WithDSSIM(base, 1.5)
    with pytest.raises(ValueError, match="tonemap"):
        losses.DSSIM("gamma")
    with pytest.raises(ValueError, match="data_range"):
        losses.DSSIM(data_range=0.0)


KPCN_ARGV = ["--desc", "d", "--use_llpm_buf", "--manif_learn", "--manif_loss", "FMSE", "--train_branches", "--single_gpu"]
SIZES = {"dncnn_in_size": 34 + 5, "pnet_in_size": 36, "pnet_out_size": 3}


def test_flag_off_leaves_the_loss_objects_as_they_were(tmp_path):
    from wcmc_amd import train_kpcn as tk
    from wcmc_amd.support import interfaces
    for extra in ([], ["--dssim_weight", "0"], ["--dssim_weight", "0.0"]):
        args = tk.check_args(tk.parse_args(KPCN_ARGV + ["--save", str(tmp_path), "--model_name", "off%d" % len(extra)] + extra))
        assert args.dssim_weight == 0.0
        lf = tk.init_model(SIZES, args, torch.device("cpu"))[0][0].loss_funcs
        for k in ("l_diffuse", "l_specular", "l_recon"):
            assert type(lf[k]) is torch.nn.L1Loss and interfaces._is_plain_l1(lf[k]), k
    # arguments that never met the flag (evaluate / denoise parse with build_parser alone) behave as flag off
    args = tk.check_args(tk.build_parser().parse_args(KPCN_ARGV + ["--save", str(tmp_path), "--model_name", "bare"]))
    assert not hasattr(args, "dssim_weight")
    assert type(tk.init_model(SIZES, args, torch.device("cpu"))[0][0].loss_funcs["l_recon"]) is torch.nn.L1Loss


def test_flag_on_wraps_the_trained_image_losses_and_no_other(tmp_path):
    from wcmc_amd import train_kpcn as tk
    from wcmc_amd.support.losses import DSSIM, FeatureMSE, RelativeMSE, WithDSSIM
    for n, mode in enumerate(([], ["--kpcn_pre"])):
        args = tk.check_args(tk.parse_args(KPCN_ARGV + mode + ["--save", str(tmp_path), "--model_name", "on%d" % n, "--dssim_weight", "0.3"]))
        lf = tk.init_model(SIZES, args, torch.device("cpu"))[0][0].loss_funcs
        for k in ("l_diffuse", "l_specular", "l_recon"):
            assert type(lf[k]) is WithDSSIM and type(lf[k].base) is torch.nn.L1Loss and lf[k].weight == 0.3, k
            assert type(lf[k].dssim) is DSSIM and (lf[k].dssim.tonemap, lf[k].dssim.data_range) == ("reinhard", 2.0)
        assert type(lf["l_test"]) is RelativeMSE and type(lf["l_manif"]) is FeatureMSE
    # --kpcn_ref shares the dictionary
    args = tk.check_args(tk.parse_args(["--desc", "d", "--kpcn_ref", "--train_branches", "--single_gpu", "--save", str(tmp_path),
                                        "--model_name", "ref", "--dssim_weight", "1"]))
    lf = tk.init_model({"dncnn_in_size": 34, "pnet_in_size": 36, "pnet_out_size": 3}, args, torch.device("cpu"))[0][0].loss_funcs
    assert type(lf["l_recon"]) is WithDSSIM and lf["l_recon"].weight == 1.0 and type(lf["l_test"]) is RelativeMSE


def test_sample_based_launchers_wrap_l_recon_alone():
    import types
    from wcmc_amd import train_kpcn as tk
    from wcmc_amd import train_lbmc as tl
    from wcmc_amd.support.losses import RelativeMSE, TonemappedRelativeMSE, WithDSSIM
    on, off = types.SimpleNamespace(dssim_weight=0.4), types.SimpleNamespace(dssim_weight=0.0)
    recon, test = TonemappedRelativeMSE(), RelativeMSE()
    lf = tk.with_dssim(off, {"l_recon": recon, "l_test": test}, ("l_recon",))
    assert lf["l_recon"] is recon and lf["l_test"] is test
    lf = tk.with_dssim(on, {"l_recon": recon, "l_test": test, "l_manif": None}, ("l_recon",))
    assert type(lf["l_recon"]) is WithDSSIM and lf["l_recon"].base is recon and lf["l_test"] is test and lf["l_manif"] is None
    # the launchers call it with l_recon alone
    import inspect
    from wcmc_amd import train_sbmc as ts
    for mod in (ts, tl):
        assert re.search(r"with_dssim\(args, .*\('l_recon',\)\)", inspect.getsource(mod.init_model)), mod.__name__


@pytest.mark.parametrize("launcher", ["train_kpcn", "train_sbmc", "train_lbmc"])
def test_flag_range_is_an_argument_error_that_names_the_flag(launcher):
    import importlib
    from wcmc_amd import train_kpcn as tk
    mod = importlib.import_module("wcmc_amd." + launcher)
    parse = lambda *a: tk.parse_args(["--desc", "x", *a], mod.build_parser())      # noqa: E731  (what each main() calls)
    assert parse().dssim_weight == 0.0 and parse("--dssim_weight", "0.25").dssim_weight == 0.25
    for bad in ("1.5", "-0.1", "nan"):
        with pytest.raises(RuntimeError, match="`--dssim_weight` should be in \\[0, 1\\]"):
            tk.check_args(parse("--dssim_weight", bad))
    tk.check_args(parse("--dssim_weight", "1"))
    with pytest.raises(SystemExit):
        parse("--dssim_weight", "much")
    text = " ".join(mod.build_parser().format_help().split())
    assert "--dssim_weight" in text
    helps = " ".join(tk.multi_spp_parser().format_help().split())
    assert "MIXED" in helps and "no value is recommended" in helps
    # the launcher's own parser keeps the flag surface earlier tests pin: the flag is read ahead of it
    assert "dssim_weight" not in {a.dest for a in mod.build_parser()._actions}
