"""Kernel splat without a GPU: the fp64 restatement against the direct loop of the specification, the new entry points in the
header, the binding and the built library, their argument checks (which precede any HIP call), and the two modules."""
import ctypes
import os
import re

import pytest
import torch

from splat_ref import splat_loop, splat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wcmc_kernel_splat_fwd", "wcmc_kernel_splat_bwd", "wcmc_logit_max")


def _gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale)


@pytest.mark.parametrize("shape,k", [((2, 3, 4, 6), 5), ((1, 2, 3, 3), 7)])
@pytest.mark.parametrize("mode", ["softmax", "shift"])
def test_restatement_equals_the_direct_loop(shape, k, mode):
    n, c, h, w = shape
    data, logits = _gen(n, c, h, w, seed=1) + 0.5, _gen(n, k * k, h, w, seed=2, scale=3.0)
    shift = logits.amax(dim=(1, 2, 3)) if mode == "shift" else None
    (r0, w0), (r1, w1) = splat_ref(data, logits, shift), splat_loop(data, logits, shift)
    assert (r0 - r1).abs().max().item() <= 1e-15 * max(1.0, r1.abs().max().item())
    assert (w0 - w1).abs().max().item() <= 1e-15 * max(1.0, w1.abs().max().item())
    if mode == "softmax":                   # every source pixel hands out a total weight of 1, less what leaves the image
        assert w0.sum().item() <= n * h * w + 1e-9 and w0.min().item() > 0


def test_new_symbols_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from wcmc_amd._lib import SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "wcmc_hip.h")).read()
    declared = set(re.findall(r"\b(wcmc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    h = lib()
    for name in NEW + ("wcmc_kernel_splat_fwd_workspace_bytes", "wcmc_logit_max_workspace_bytes"):
        assert name in declared and name in SIGNATURES, name
        assert getattr(h, name) is not None
    # [N][tiles][C + 1][8 + k - 1][16 + k - 1] floats: the workload's shape, and nothing for an unsupported one
    assert h.wcmc_kernel_splat_fwd_workspace_bytes(8, 3, 128, 128, 441) == 8 * 128 * 4 * 28 * 36 * 4
    assert h.wcmc_kernel_splat_fwd_workspace_bytes(8, 3, 128, 128, 440) == 0
    assert h.wcmc_logit_max_workspace_bytes(8) > 0


def test_new_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Even k, a k2 that is no square, C > 4, k > 21 and a null shift in shift mode: WCMC_ERR_BAD_ARG and a message that names
    the entry point; nothing is launched (the checks precede every HIP call, so this runs without a GPU)."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)     # `one`: non-null and 16-byte aligned, never dereferenced by the checks

    def fwd(c, k2, mode, shift):
        return L.wcmc_kernel_splat_fwd(one, 448, 448, 448, one, 1, 1, 1, 1, one, one, null, mode, shift, 0, one, 1 << 30,
                                       1, c, 4, 4, k2, null)

    def bwd(c, k2, mode, shift):
        return L.wcmc_kernel_splat_bwd(one, 448, 448, 448, one, 1, 1, 1, 1, one, 1, 1, 1, 1, null, 0, 0, 0, one, mode, shift,
                                       one, 448, 448, 448, null, 1, c, 4, 4, k2, null)
    cases = {"even k": (3, 16, 1, one, "odd"), "k2 not a square": (3, 440, 1, one, "not a square"),
             "C > 4": (5, 441, 1, one, "C = 5"), "k > 21": (3, 529, 1, one, "at most 21"),
             "null shift": (3, 441, 1, null, "shift"), "unknown mode": (3, 441, 7, one, "mode")}
    for what, (c, k2, mode, shift, word) in cases.items():
        for name, fn in (("kernel_splat_fwd", fwd), ("kernel_splat_bwd", bwd)):
            assert fn(c, k2, mode, shift) == -1, (what, name)                    # WCMC_ERR_BAD_ARG
            msg = L.wcmc_last_error().decode()
            assert name in msg and word in msg, (what, name, msg)
    # both gradients absent; a logits view that breaks the NHWC contract; a workspace that is too small
    assert L.wcmc_kernel_splat_bwd(one, 448, 448, 448, one, 1, 1, 1, 1, null, 0, 0, 0, 0, null, 0, 0, 0, one, 0, null, one, 448,
                                   448, 448, null, 1, 3, 4, 4, 441, null) == -1
    assert "gradients" in L.wcmc_last_error().decode()
    assert L.wcmc_kernel_splat_fwd(one, 441, 441, 441, one, 1, 1, 1, 1, one, one, null, 0, null, 0, one, 1 << 30, 1, 3, 4, 4, 441,
                                   null) == -2
    assert L.wcmc_kernel_splat_fwd(one, 448, 448, 448, one, 1, 1, 1, 1, one, one, null, 0, null, 0, one, 16, 1, 3, 4, 4, 441,
                                   null) == -3
    assert "workspace" in L.wcmc_last_error().decode()
    assert L.wcmc_logit_max(one, 448, 448, 448, null, one, 1 << 20, 1, 4, 4, 441, null) == -1
    assert "logit_max" in L.wcmc_last_error().decode()
    assert L.wcmc_logit_max(one, 448, 448, 448, one, one, 0, 1, 4, 4, 441, null) == -3


def test_modules_construct_and_the_unbuilt_forms_stay_refused():
    from wcmc_amd import modules
    assert modules.KernelApply(softmax=True, splat=True).splat is True
    assert modules.KernelApply(softmax=True, splat=False).splat is False
    modules.ProgressiveKernelApply(splat=True)
    modules.ProgressiveKernelApply()
    with pytest.raises(AssertionError, match="softmax"):
        modules.KernelApply(softmax=False)
    with pytest.raises(AssertionError, match="softmax"):
        modules.KernelApply(softmax=False, splat=True)
    with pytest.raises(AssertionError, match="splat"):
        modules.ProgressiveKernelApply(splat=False)


def test_splat_ops_have_no_cpu_path():
    from wcmc_amd import modules, ops
    data, logits = torch.zeros(1, 3, 4, 4), torch.zeros(1, 9, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.kernel_splat(data, logits)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.logit_max(logits)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.KernelApply(splat=True)(data, logits)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.ProgressiveKernelApply()(data, logits, None, None, None)
