"""The P-buffer filter without a GPU: the fp64 restatement against the direct loop of the specification, the new entry points in the
header, the binding and the built library, their argument checks (which precede any HIP call), the Python-side refusals and the
command lines' argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from rhf_ref import rhf_loop, rhf_ref, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wcmc_pbuffer_filter_workspace_bytes", "wcmc_pbuffer_filter")


@pytest.mark.parametrize("masked", [False, True])
def test_restatement_equals_the_direct_loop(masked):
    h, w, s, c, r, f = 6, 7, 3, 2, 2, 1
    img, p = scene(h, w, s, c, seed=3)
    mask = None
    if masked:
        mask = torch.ones((h, w), dtype=torch.uint8)
        mask[0, 0] = mask[2, 3] = mask[5, 6] = mask[3, 0] = 0
    (o0, w0), (o1, w1) = rhf_ref(img, p, r, f, 1.0, 1e-3, mask), rhf_loop(img, p, r, f, 1.0, 1e-3, mask)
    assert (o0 - o1).abs().max().item() <= 1e-12 * o1.abs().max().item()
    assert (w0 - w1).abs().max().item() <= 1e-12 * w1.abs().max().item()
    assert w1.max().item() > 1.5                      # the weights are not all 0 or 1: the case tests the distance
    if masked:
        assert w0[0, 0] == 0 and w0[2, 3] == 0 and torch.equal(o0[2, 3], img[2, 3].double())
        assert ((w0 >= 1) | (mask == 0)).all()
    else:
        assert (w0 >= 1).all()


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
    # {mu, v} per channel and pixel, and nothing for an unsupported shape
    assert h.wcmc_pbuffer_filter_workspace_bytes(8, 3, 720, 1280) == 3 * 720 * 1280 * 8
    assert h.wcmc_pbuffer_filter_workspace_bytes(8, 33, 720, 1280) == 0
    assert h.wcmc_pbuffer_filter_workspace_bytes(0, 3, 720, 1280) == 0
    assert h.wcmc_pbuffer_filter_workspace_bytes(8, 3, 0, 1280) == 0


def test_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    """Every refusal of the C ABI: the library's error code, a message that names the op, nothing launched (the checks precede
    every HIP call, so this runs without a GPU)."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)     # `one`: non-null, never dereferenced by the checks
    good = dict(image=one, p_buffer=one, mask=null, mask_bytes=0, out=one, wsum=one, ws=one, ws_bytes=1 << 30, H=8, W=8, S=2, C=3,
                Cr=3, R=10, f=1, b=1.0, eps=1e-3, passes=3)

    def call(**kw):
        a = dict(good, **kw)
        return L.wcmc_pbuffer_filter(a["image"], 24, 3, 1, a["p_buffer"], 192, 64, 8, 1, a["mask"], a["mask_bytes"], a["out"],
                                     a["wsum"], a["ws"], a["ws_bytes"], a["H"], a["W"], a["S"], a["C"], a["Cr"], a["R"], a["f"],
                                     a["b"], a["eps"], a["passes"], null)
    bad_arg = {"R > 10": dict(R=11), "R < 0": dict(R=-1), "f > 3": dict(f=4), "C > 32": dict(C=33), "C < 1": dict(C=0),
               "Cr > 4": dict(Cr=5), "S < 1": dict(S=0), "b <= 0": dict(b=0.0), "b < 0": dict(b=-1.0), "eps <= 0": dict(eps=0.0),
               "b nan": dict(b=float("nan")), "null image": dict(image=null), "null p_buffer": dict(p_buffer=null),
               "null out": dict(out=null), "null wsum": dict(wsum=null), "null workspace": dict(ws=null),
               "mask element size": dict(mask=one, mask_bytes=2), "passes": dict(passes=0)}
    for what, kw in bad_arg.items():
        assert call(**kw) == -1, what                                            # WCMC_ERR_BAD_ARG
        assert "pbuffer_filter" in L.wcmc_last_error().decode(), what
    assert call(ws_bytes=8 * 8 * 3 * 8 - 1) == -3                                # WCMC_ERR_WORKSPACE
    msg = L.wcmc_last_error().decode()
    assert "pbuffer_filter" in msg and "workspace" in msg and str(8 * 8 * 3 * 8) in msg


def test_python_side_refusals():
    from wcmc_amd import ops
    assert ops.pbuffer_filter is ops.filter.pbuffer_filter
    img, p = torch.zeros(4, 5, 3), torch.zeros(2, 3, 4, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pbuffer_filter(img, p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pbuffer_filter(img, p, mask=torch.ones(4, 5, dtype=torch.uint8))
    cases = [
        (dict(image=torch.zeros(3, 4, 5)), ValueError, "differ in frame size"),
        (dict(image=torch.zeros(4, 5)), ValueError, r"\(H, W, Cr\)"),
        (dict(p_buffer=torch.zeros(3, 4, 5)), ValueError, r"\(S, C, H, W\)"),
        (dict(image=torch.zeros(4, 5, 5)), ValueError, "5 channels"),
        (dict(p_buffer=torch.zeros(2, 33, 4, 5)), ValueError, "33 channels"),
        (dict(p_buffer=torch.zeros(0, 3, 4, 5)), ValueError, "no samples"),
        (dict(image=img.double()), TypeError, "image must be float32"),
        (dict(p_buffer=p.half()), TypeError, "p_buffer must be float32"),
        (dict(image=img.clone().requires_grad_()), RuntimeError, "image requires grad"),
        (dict(p_buffer=p.clone().requires_grad_()), RuntimeError, "p_buffer requires grad"),
        (dict(radius=11), ValueError, "radius 11"), (dict(radius=-1), ValueError, "radius -1"),
        (dict(radius=2.5), ValueError, "radius 2.5"), (dict(patch_radius=4), ValueError, "patch_radius 4"),
        (dict(bandwidth=0.0), ValueError, "must be positive"), (dict(eps=-1.0), ValueError, "must be positive"),
        (dict(mask=torch.ones(5, 4, dtype=torch.uint8)), ValueError, "mask must be an"),
        (dict(mask=torch.ones(4, 5, dtype=torch.int64)), TypeError, "mask must be uint8, bool or float32"),
    ]
    for kw, exc, word in cases:
        with pytest.raises(exc, match=word):
            ops.pbuffer_filter(**dict(dict(image=img, p_buffer=p), **kw))


def test_rhf_filter_refuses_mismatched_branches_and_has_no_cpu_path():
    from wcmc_amd import rhf
    img = torch.zeros(4, 5, 3)
    with pytest.raises(ValueError, match="one S, H and W"):
        rhf.rhf_filter(img, {"diffuse": torch.zeros(2, 3, 4, 5), "specular": torch.zeros(3, 3, 4, 5)})
    with pytest.raises(ValueError, match="empty dict"):
        rhf.rhf_filter(img, {})
    with pytest.raises(RuntimeError, match="no CPU path"):
        rhf.rhf_filter(img, {"diffuse": torch.zeros(2, 3, 4, 5), "specular": torch.zeros(2, 3, 4, 5)}, torch.ones(4, 5))


def test_command_line_argument_errors(tmp_path):
    from wcmc_amd import rhf
    np.save(tmp_path / "img.npy", np.zeros((4, 5, 3), np.float32))
    np.save(tmp_path / "p.npy", np.zeros((4, 5, 2, 3), np.float32))
    np.save(tmp_path / "p_small.npy", np.zeros((4, 4, 2, 3), np.float32))
    np.save(tmp_path / "p_wide.npy", np.zeros((4, 5, 1, 33), np.float32))
    np.save(tmp_path / "grey.npy", np.zeros((4, 5), np.float32))
    np.save(tmp_path / "mask_bad.npy", np.zeros((5, 4), np.uint8))
    base = lambda **kw: sum((["--" + k, str(v)] for k, v in dict(dict(image=tmp_path / "img.npy", pbuffer=tmp_path / "p.npy",   # noqa: E731
                                                                      output_dir=tmp_path / "out"), **kw).items()), [])
    with pytest.raises(SystemExit):
        rhf.main(["--image", "x.npy"])                                   # --pbuffer and --output_dir are required
    for kw, exc, word in [(dict(radius=11), ValueError, "--radius should be in 0..10"),
                          (dict(patch_radius=4), ValueError, "--patch_radius should be in 0..3"),
                          (dict(bandwidth=0), ValueError, "--bandwidth should be positive"),
                          (dict(eps=-1), ValueError, "--eps should be positive"),
                          (dict(image=tmp_path / "none.npy"), FileNotFoundError, "none.npy"),
                          (dict(image=tmp_path / "grey.npy"), ValueError, r"not an \(H, W, 3\) frame"),
                          (dict(pbuffer=tmp_path / "p_small.npy"), ValueError, r"not \(H, W, S, C\) with the 4 x 5"),
                          (dict(pbuffer=tmp_path / "p_wide.npy"), ValueError, "33 channels"),
                          (dict(mask=tmp_path / "mask_bad.npy"), ValueError, r"--mask .* is not the \(H, W\)")]:
        with pytest.raises(exc, match=word):
            rhf.main(base(**kw))
    assert not (tmp_path / "out").exists()                               # nothing was written on the way to an error
    assert " ".join(rhf.build_parser().format_help().split()).count("nobody has tuned it") == 4


def test_denoise_rhf_flag_needs_the_pbuffer_and_checks_its_parameters(tmp_path):
    from wcmc_amd import denoise
    np.save(tmp_path / "scene.npy", np.zeros((64, 64, 2, 104), np.float32))
    argv = ["--save", "w", "--model_name", "KPCN_x", "--input", str(tmp_path / "scene.npy"), "--output_dir", "o"]
    parse = lambda extra: denoise.build_parser().parse_args(argv + extra)      # noqa: E731
    args = parse([])
    assert args.rhf is False and (args.rhf_radius, args.rhf_patch_radius, args.rhf_bandwidth, args.rhf_eps) == (10, 1, 1.0, 1e-3)
    denoise.check_inputs(args)                                           # without the flag: as before
    with pytest.raises(ValueError, match=r"--rhf: the model computes no P-buffer \(it needs --use_llpm_buf\)"):
        denoise.check_inputs(parse(["--rhf"]))
    with pytest.raises(ValueError, match="--rhf_radius should be in 0..10"):
        denoise.check_inputs(parse(["--rhf", "--use_llpm_buf", "--rhf_radius", "12"]))
    with pytest.raises(ValueError, match="--rhf_bandwidth should be positive"):
        denoise.check_inputs(parse(["--rhf", "--use_llpm_buf", "--rhf_bandwidth", "0"]))
    denoise.check_inputs(parse(["--rhf", "--use_llpm_buf", "--rhf_patch_radius", "3"]))
    assert " ".join(denoise.build_parser().format_help().split()).count("nobody has tuned it") == 4
