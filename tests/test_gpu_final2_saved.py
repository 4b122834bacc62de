"""PathNet.final's backward on the forward's saved tensors (``wcmc_final2_fwd`` with ``h_hi``, ``wcmc_final2_bwd`` with ``out`` and
``h_hi``; ``ops.SAVE_FINAL_HIDDEN``) against the backward that recomputes them (the same entries with null pointers there).

The saved route changes no arithmetic: every MFMA that remains runs on the same operands in the same order on the same grid, so
every comparison here is ``torch.equal`` -- there is no tolerance to choose.
"""
import ctypes
import os
import re

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dflat", "dprop", "dw0", "db0", "dw1", "db1")


def ops():
    from wcmc_amd import ops as _ops
    return _ops


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def inputs(case):
    b, s, h, w, outc = case
    params = [gen(128, 128, 1, 1, seed=502, scale=(2.0 / 128) ** 0.5 * 1.7), gen(128, seed=503, scale=0.2),
              gen(outc, 128, 1, 1, seed=504, scale=(2.0 / 128) ** 0.5 * 1.7), gen(outc, seed=505, scale=0.2)]
    return gen(b * s, 64, h, w, seed=500), gen(b, 64, h, w, seed=501), params, gen(b * s, outc, h, w, seed=506)


class _Spy:
    """The library, with the names and the arguments of the entries called through it."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)

        return recorded


def run_routes(case, flat, prop, params, g, monkeypatch):
    """{save: (out, [d_flat, d_prop, dW0, db0, dW1, db1])} of ``cat_broadcast_chain`` with SAVE_FINAL_HIDDEN on and off; asserts
    that each route ran its own pair of entries."""
    o = ops()
    assert o.reduced_backward() and o.FUSE_FINAL
    s = case[1]
    res = {}
    for save in (True, False):
        monkeypatch.setattr(o, "SAVE_FINAL_HIDDEN", save)
        spy = _Spy(o.pathnet_fused.lib())
        monkeypatch.setattr(o.pathnet_fused, "lib", lambda spy=spy: spy)
        fd = o.to_nhwc_raw(flat.to(DEV)).requires_grad_(True)
        pd = o.to_nhwc_raw(prop.to(DEV)).requires_grad_(True)
        ps = [t.to(DEV).requires_grad_(True) for t in params]
        out = o.cat_broadcast_chain(fd, pd, s, 1, 0, ["relu", "relu"], ps)
        out.backward(g.to(DEV))
        res[save] = (out.detach().clone(), [fd.grad.clone(), pd.grad.clone()] + [t.grad.clone() for t in ps])
        called = [c for c in spy.calls if c[0].startswith("wcmc_final2_fwd") or (c[0].startswith("wcmc_final2_bwd") and "workspace" not in c[0])]
        assert [c[0] for c in called] == ["wcmc_final2_fwd", "wcmc_final2_bwd"], called
        # the form each launch took: (h_hi) of the forward, (out, h_hi) of the backward -- filled on the saved route, null on the other
        given = [bool(a.value) for a in (called[0][1][13], called[1][1][15], called[1][1][16])]
        assert given == [save] * 3, (save, given)
        if save:            # ... and the backward was handed the forward's own output and plane
            assert called[1][1][15].value == called[0][1][12].value and called[1][1][16].value == called[0][1][13].value
    return res


def assert_routes_equal(res):
    assert torch.equal(res[True][0], res[False][0]), "out"
    for got, want, name in zip(res[True][1], res[False][1], NAMES):
        assert got.shape == want.shape and torch.equal(got, want), "%s: %d entries differ, max |diff| %.3e" % (
            name, int((got != want).sum()), float((got - want).abs().max()))


# (5, 2, 64, 64, 3): 320 super-tiles on 256 workgroups -- some walk two: register accumulation across tiles, LDS reuse across the
# super-tile boundary; (1, 2, 8, 24, 8), (2, 3, 8, 8, 5): eight-float output pixels, outc not a multiple of 4
@gpu
@pytest.mark.parametrize("case", [(1, 1, 8, 8, 3), (2, 3, 8, 8, 3), (1, 2, 8, 24, 8), (2, 3, 8, 8, 5), (3, 2, 8, 24, 1), (5, 2, 64, 64, 3)])
def test_saved_route_is_bitwise_the_recompute_route(case, monkeypatch):
    flat, prop, params, g = inputs(case)
    res = run_routes(case, flat, prop, params, g, monkeypatch)
    assert_routes_equal(res)
    assert all(float(t.abs().max()) > 0 for t in res[True][1])          # (nothing compared equal because it was never written)


@gpu
@pytest.mark.parametrize("dead", ["some", "all"])
def test_saved_route_gates_dead_units_like_the_recompute_route(dead, monkeypatch):
    """Gates that are closed: half of the hidden channels and one output channel (b0 / b1 strongly negative), then every unit --
    both routes bitwise equal, and with every unit dead every gradient exactly zero."""
    case = (2, 3, 8, 8, 3)
    flat, prop, params, g = inputs(case)
    if dead == "some":
        params[1][::2] = -100.0
        params[3][1] = -100.0
    else:
        params[1][:] = -100.0
        params[3][:] = -100.0
    res = run_routes(case, flat, prop, params, g, monkeypatch)
    assert_routes_equal(res)
    if dead == "some":
        assert float(res[True][0][:, 1].abs().max()) == 0.0 and float(res[True][0].abs().max()) > 0.0
        db0 = res[True][1][3]
        assert float(db0[::2].abs().max()) == 0.0 and float(db0[1::2].abs().max()) > 0.0
    else:
        assert float(res[True][0].abs().max()) == 0.0
        for t, name in zip(res[True][1], NAMES):
            assert float(t.abs().max()) == 0.0, name


def _fwd_pair(o, case, flat, prop, params):
    """(out of wcmc_final2_fwd without h_hi, out and plane of it with h_hi), called through the C ABI on the same inputs."""
    from wcmc_amd._lib import check, lib
    b, s, h, w, outc = case
    fd, pd = o.to_nhwc_raw(flat.to(DEV)), o.to_nhwc_raw(prop.to(DEV))
    ps = [t.to(DEV) for t in params]
    packs = o._pack_chain_x([ps[0], ps[2]], 1)
    osz = 4 if outc <= 4 else 8
    m = b * s * h * w
    args = lambda out: (fd.data_ptr(), fd.stride(3), pd.data_ptr(), pd.stride(3), b, s, h * w, packs[0][0].data_ptr(), ps[1].data_ptr(),
                        packs[1][0].data_ptr(), ps[3].data_ptr(), outc, out.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    out0 = torch.full((m, osz), 7.0, device=DEV)
    out1 = torch.full((m, osz), 9.0, device=DEV)
    plane = torch.full((m, 128), 3.0, device=DEV, dtype=torch.bfloat16)
    check(lib().wcmc_final2_fwd(*args(out0), None, stream), "final2_fwd")
    check(lib().wcmc_final2_fwd(*args(out1), plane.data_ptr(), stream), "final2_fwd with h_hi")
    torch.cuda.synchronize()
    return out0, out1, plane


@gpu
@pytest.mark.parametrize("case", [(2, 3, 8, 8, 3), (1, 2, 8, 24, 8), (5, 2, 64, 64, 3)])
def test_saved_plane_is_the_hi_plane_of_the_hidden_activation(case, monkeypatch):
    """The plane ``wcmc_final2_fwd`` writes into ``h_hi`` = the hi plane of the layer-by-layer path's hidden activation, bit for bit, taken
    two ways: from the split tensor that path wrote (``wcmc_conv1x1_pair_bf16x3``'s first result), and from its ``DEBUG_ACTS``
    value (hi + lo, exact in fp32) run through the library's own split (``wcmc_split_bf16``).  The second way cannot tell the hi
    plane where hi + lo lies exactly half way between two bf16 values (lo was itself rounded, to half an ulp of hi: the re-split
    then rounds to even, which need not be hi): there the plane must be one of those two neighbours, everywhere else the re-split's
    hi, and the first way pins every entry.  ``out`` with ``h_hi`` = ``out`` without it, bit for bit."""
    o = ops()
    b, s, h, w, outc = case
    m = b * s * h * w
    flat, prop, params, _ = inputs(case)
    out0, out1, plane = _fwd_pair(o, case, flat, prop, params)
    assert torch.equal(out0, out1)
    acts, written = [], []
    pair = o.conv_split.conv1x1_pair_x_raw

    def pair_keeping_its_split(*a, **k):
        r = pair(*a, **k)
        written.append(r[0])
        return r

    # (the hidden activation leaves the fused layer pair where the library has that instance, outc <= 4, and the first layer's own
    # launch otherwise, where the identity below sees it)
    monkeypatch.setattr(o.conv_split, "conv1x1_pair_x_raw", pair_keeping_its_split)
    monkeypatch.setattr(o, "EMULATE_HIDDEN", lambda split, dims, ks: (written.append(split), split)[1])
    monkeypatch.setattr(o, "FUSE_FINAL", False)
    monkeypatch.setattr(o, "DEBUG_ACTS", acts)
    with torch.no_grad():
        ref = o.cat_broadcast_chain(o.to_nhwc_raw(flat.to(DEV)), o.to_nhwc_raw(prop.to(DEV)), s, 1, 0, ["relu", "relu"],
                                    [t.to(DEV) for t in params])
    monkeypatch.setattr(o, "DEBUG_ACTS", None)
    monkeypatch.setattr(o, "EMULATE_HIDDEN", None)
    assert len(acts) == 2 and tuple(acts[0].shape) == (b * s, 128, h, w) and len(written) == 1
    assert torch.equal(out1.view(b * s, h, w, -1)[..., :outc].permute(0, 3, 1, 2), ref)
    hi_of = lambda split: split.view(m, 2, 128)[:, 0].contiguous()          # [N][H][W][2][128] bf16 in int16 storage
    got = plane.view(torch.int16)
    assert torch.equal(got, hi_of(written[0])), "%d entries differ from the split the layer-by-layer path wrote" % int((got != hi_of(written[0])).sum())
    v = o.to_nhwc_raw(acts[0].contiguous())
    resplit = hi_of(o.split_raw(v))
    bits = v.permute(0, 2, 3, 1).reshape(m, 128).contiguous().view(torch.int32)
    tie = (bits & 0xffff) == 0x8000
    print("re-split: %d of %d entries are ties, %d of them re-split to the other neighbour" % (int(tie.sum()), tie.numel(), int((got != resplit).sum())))
    assert torch.equal(got[~tie], resplit[~tie])
    assert bool(((got.int() == (bits >> 16)) | (got.int() == (bits >> 16) + 1))[tie].all()) and float(tie.float().mean()) < 0.01
    assert float(plane.float().max()) > 0.0 and float(plane.float().min()) == 0.0


# ---------------------------------------------------------------------------------------------- host side: no GPU needed
def test_new_entries_refuse_bad_arguments_before_any_launch():
    """Misaligned ``h_hi`` and ``out``, one of the pair without the other in the backward, and a short workspace: the error codes
    include/wcmc_hip.h documents, from checks that precede every HIP call (so this runs without a device; a launch would not return
    one of these codes).  (A null ``h_hi`` in the forward, and a null pair in the backward, are the plain forms: no refusals.)"""
    from wcmc_amd._lib import lib
    L = lib()
    BAD_ARG, ALIGNMENT, WORKSPACE = -1, -2, -3
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(24)      # never dereferenced by the checks
    nb = L.wcmc_final2_bwd_workspace_bytes()
    common = (one, 64, one, 64, 1, 1, 64, one, one, one, one, 3)
    fwd = lambda out, h: L.wcmc_final2_fwd(*common, out, h, null)
    bwd = lambda out, h, n=nb: L.wcmc_final2_bwd(*common, one, one, one, out, h, one, one, one, one, one, one, one, n, null)
    for call, want, what in ((lambda: fwd(one, odd), ALIGNMENT, "fwd: misaligned h_hi"),
                             (lambda: fwd(null, one), BAD_ARG, "fwd: null out"), (lambda: fwd(odd, one), BAD_ARG, "fwd: misaligned out"),
                             (lambda: fwd(null, null), BAD_ARG, "fwd, plain form: null out"),
                             (lambda: bwd(one, null), BAD_ARG, "bwd: out without h_hi"), (lambda: bwd(null, one), BAD_ARG, "bwd: h_hi without out"),
                             (lambda: bwd(odd, one), ALIGNMENT, "bwd: misaligned out"), (lambda: bwd(one, odd), ALIGNMENT, "bwd: misaligned h_hi"),
                             (lambda: bwd(one, one, nb - 1), WORKSPACE, "bwd: short workspace"),
                             (lambda: bwd(one, one, 0), WORKSPACE, "bwd: no workspace bytes"),
                             (lambda: bwd(null, null, nb - 1), WORKSPACE, "bwd, recomputing form: short workspace")):
        rc = call()
        msg = L.wcmc_last_error().decode()
        assert rc == want and "final2" in msg, (what, rc, msg)
        if "without" in what:           # the message says which of the pair is missing
            assert what.split(": ")[1] in msg, (what, msg)
    # a plane of 2 GiB or more does not fit the 32-bit buffer range: refused like dy
    assert L.wcmc_final2_fwd(one, 64, one, 64, 1, 1, 1 << 23, one, one, one, one, 3, one, one, null) == BAD_ARG


def test_header_binding_and_libraries_agree_on_the_new_entries():
    """Type by type: the prototypes of the two entries in include/wcmc_hip.h against ``_lib.SIGNATURES``; both libraries export them."""
    from wcmc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wcmc_hip.h")).read(), flags=re.S)

    def code(param):
        t = param.strip().rsplit(None, 1)[0] if "*" not in param else "ptr"
        return {"ptr": _lib.P, "int": _lib.I, "int64_t": _lib.L, "size_t": _lib.Z}[t]

    libs = [ctypes.CDLL(path) for path in (_lib.LIB_PATH, os.path.join(os.path.dirname(_lib.LIB_PATH), "libwcmc_hip_debug.so"))]
    # (the pointers of the saved form: h_hi behind out in the forward; out, h_hi behind gout in the backward)
    for name, at, names in (("wcmc_final2_fwd", 12, ["out", "h_hi", "stream"]), ("wcmc_final2_bwd", 14, ["gout", "out", "h_hi", "dy"])):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = m.group(1).split(",")
        assert res is _lib.I and [code(a) for a in params] == args, name
        assert [p.strip().rsplit(None, 1)[-1].lstrip("*") for p in params[at:at + len(names)]] == names, name
        for h in libs:
            assert getattr(h, name) is not None, name
    for gone in ("wcmc_final2_fwd_save", "wcmc_final2_bwd_saved"):
        assert gone not in _lib.SIGNATURES and not re.search(r"\b%s\b" % gone, header) and not any(hasattr(h, gone) for h in libs), gone
    from wcmc_amd import ops
    assert ops.SAVE_FINAL_HIDDEN in (True, False) and not hasattr(ops.pathnet_fused, "SAVE_FINAL_HIDDEN")
