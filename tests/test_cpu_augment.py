"""Dihedral patch augmentation without a GPU: the two patch entry points, which take the code table, in the
header, the binding and the built library; their argument checks (which precede any HIP call); the host check of a code table; the eight codes against the
reference's flip-then-rotate draws; the loader's private draw; the launchers' argument errors."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wcmc_assemble_kpcn_patches": 21, "wcmc_assemble_sample_patches": 19}
# ABI 3 folded the variants of the four batch assemblers into the base names: these six are gone
GONE = tuple(base + suffix for base, suffixes in (("wcmc_assemble_kpcn_patches", ("_prefix", "_aug")),
                                                  ("wcmc_assemble_sample_patches", ("_prefix", "_aug")),
                                                  ("wcmc_assemble_kpcn_tiles", ("_aug",)), ("wcmc_assemble_sample_tiles", ("_aug",)))
             for suffix in suffixes)


def T(a, t):
    """The transform of code t."""
    return np.rot90(np.fliplr(a) if t & 4 else a, k=t & 3)


def test_new_symbols_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from wcmc_amd._lib import SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "wcmc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(wcmc_[a-z0-9_]+)\s*\(", header))
    h = lib()
    for name, nargs in NEW.items():
        assert name in declared and name in SIGNATURES, name
        assert getattr(h, name) is not None
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        # the buffers, the origins and the table, B H W S_total s P, the flags of the sample form, the outputs, the stream
        assert len(m.group(1).split(",")) == len(SIGNATURES[name][1]) == nargs, name
    assert len(GONE) == 6
    for name in GONE:
        assert name not in declared and name not in SIGNATURES, name
        with pytest.raises(AttributeError):
            getattr(h, name)


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Every refusal of the C ABI: the library's error code and a message of its own that names the op; nothing is launched (the checks
    precede every HIP call, so this runs without a GPU)."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)     # `one`: non-null, never dereferenced by the checks
    good = dict(a=one, llpm=one, gt=one, origins=one, tr=one, B=2, H=24, W=40, S=3, s=2, P=8, out=one, paths=one, sbmc_p=one, use_p=1)

    def kpcn(**kw):
        a = dict(good, **kw)
        return L.wcmc_assemble_kpcn_patches(a["a"], a["llpm"], a["gt"], a["origins"], a["tr"], a["B"], a["H"], a["W"], a["S"], a["s"],
                                            a["P"], a["out"], one, one, one, one, a["paths"], one, one, one, null)

    def sample(**kw):
        a = dict(good, **kw)
        return L.wcmc_assemble_sample_patches(a["a"], a["sbmc_p"], a["llpm"], a["gt"], a["origins"], a["tr"], a["B"], a["H"], a["W"],
                                              a["S"], a["s"], a["P"], 1, a["use_p"], a["out"], one, a["paths"], one, null)
    # (a null table is the plain batch, not an error: with it a bad argument is still refused, by the same check and with the sizes
    # it was given -- the KPCN form has five kinds of refusal since the null table stopped being one, this entry holds the numbers)
    shared = {"null transforms, P > H": (dict(tr=null, P=25), "a 25-pixel patch does not fit the 24 x 40 frame"),
              "s = 0": (dict(s=0), "1 <= s <= S_total"),
              "s > S_total": (dict(s=4), "1 <= s <= S_total"), "S_total = 0": (dict(S=0, s=0), "1 <= s <= S_total"),
              "P > H": (dict(P=25), "does not fit"), "P > W": (dict(H=64, P=41), "does not fit"), "P = 0": (dict(P=0), "must be positive"),
              "B = 0": (dict(B=0), "must be positive"), "null buffer": (dict(a=null), "null pointer"),
              "null gt": (dict(gt=null), "null pointer"), "null origins": (dict(origins=null), "null pointer"),
              "null output": (dict(out=null), "null pointer"), "llpm without paths": (dict(paths=null), "without a paths output")}
    for fn, op, extra in ((kpcn, "assemble_kpcn_patches", {}),
                          (sample, "assemble_sample_patches", {"use_sbmc_buf without sbmc_p": (dict(sbmc_p=null), "needs sbmc_p")})):
        seen = set()
        for what, (kw, word) in dict(shared, **extra).items():
            assert fn(**kw) == -1, (op, what)                                    # WCMC_ERR_BAD_ARG
            msg = L.wcmc_last_error().decode()
            assert msg.startswith(op + ":") and word in msg, (op, what, msg)
            seen.add(word)
        assert len(seen) >= 6                                                    # each kind of refusal has its own message
    # ... also without llpm, where the KPCN form reads neither sample count (S_total = s = 0 is what ops passes then)
    assert kpcn(tr=null, llpm=null, paths=null, S=0, s=0, P=25) == -1
    msg = L.wcmc_last_error().decode()
    assert msg.startswith("assemble_kpcn_patches:") and "does not fit" in msg, msg


def test_check_patch_transforms_refuses_length_dtype_and_range():
    from wcmc_amd import ops
    assert ops.check_patch_transforms is ops.data.check_patch_transforms
    ok = np.arange(8, dtype=np.int32)
    ops.check_patch_transforms(ok, 8)
    ops.check_patch_transforms(torch.from_numpy(ok), 8)
    ops.check_patch_transforms(np.zeros(0, np.int32), 0)
    cases = [(ok, 7, "one code per patch"), (ok[:3], 8, "one code per patch"), (ok.reshape(2, 4), 8, "one code per patch"),
             (ok.astype(np.int64), 8, "int32"), (ok.astype(np.float32), 8, "int32"), (torch.arange(8), 8, "int32"),
             (list(range(8)), 8, "int32"), (np.array([0, 8], np.int32), 2, "outside 0..7"), (np.array([-1, 3], np.int32), 2, "outside 0..7"),
             (torch.tensor([7, 9], dtype=torch.int32), 2, "outside 0..7")]
    for t, b, word in cases:
        for who in ("assemble_kpcn_patches", "assemble_sample_patches"):
            with pytest.raises(ValueError, match=word) as e:
                ops.check_patch_transforms(t, b, who=who)
            assert str(e.value).startswith(who + ":")


def test_the_eight_codes_are_the_sixteen_draws_of_the_reference_two_each():
    """`_random_rot(_random_flip(.))` (datasets.py:718-758): flipud or not, fliplr or not, then rot90 by k -- sixteen equally likely
    draws.  On an index array without symmetry they give eight distinct arrays, each twice, and those are T_0..T_7."""
    a = np.arange(25).reshape(5, 5)
    codes = [T(a, t) for t in range(8)]
    assert np.array_equal(codes[0], a)
    assert len({c.tobytes() for c in codes}) == 8
    hits = [0] * 8
    for ud, lr, k in itertools.product((0, 1), (0, 1), range(4)):
        x = np.flipud(a) if ud else a
        x = np.fliplr(x) if lr else x
        x = np.rot90(x, k)
        match = [t for t in range(8) if np.array_equal(codes[t], x)]
        assert len(match) == 1, (ud, lr, k)
        hits[match[0]] += 1
    assert hits == [2] * 8
    # the table of the specification, derived here from the index array: output (y, x) <- window (sy, sx)
    P = 5
    for t in range(8):
        for y, x in itertools.product(range(P), range(P)):
            sy, sx = [(y, x), (x, P - 1 - y), (P - 1 - y, P - 1 - x), (P - 1 - x, y)][t & 3]
            if t & 4:
                sx = P - 1 - sx
            assert codes[t][y, x] == a[sy, sx], (t, y, x)


def _bare_loader(seed, ppi=16):
    """A PatchLoader with only what the draw reads (its constructor opens device streams)."""
    from wcmc_amd.support.datasets import PatchBatcher
    from wcmc_amd.support.loader import PatchLoader
    ld = PatchLoader.__new__(PatchLoader)
    ld.augment, ld.augment_seed, ld.epoch = True, seed, -1
    ld.batcher = PatchBatcher(8, 4)
    ld.batcher.patches_per_image = ppi
    return ld


def test_the_loaders_draw_is_reproducible_private_and_keyed():
    a, b, c = _bare_loader(3), _bare_loader(3), _bare_loader(4)
    state = np.random.get_state()
    draws = {(img, ep, spp): a.patch_transforms(img, epoch=ep, spp=spp) for img in (0, 1, 5) for ep in (0, 1) for spp in (None, 2, 3)}
    now = np.random.get_state()
    assert state[0] == now[0] and np.array_equal(state[1], now[1]) and state[2:] == now[2:]       # the process-wide stream is untouched
    for key, d in draws.items():
        assert d.dtype == np.int32 and d.shape == (16,) and d.min() >= 0 and d.max() <= 7
        assert np.array_equal(d, b.patch_transforms(key[0], epoch=key[1], spp=key[2])), key         # same seed, same codes
    assert any(not np.array_equal(d, c.patch_transforms(k[0], epoch=k[1], spp=k[2])) for k, d in draws.items())  # another seed
    # image, pass and sample count each key the draw
    assert len({d.tobytes() for d in draws.values()}) == len(draws)
    # the default pass is the current one; the first pass is 0
    assert np.array_equal(a.patch_transforms(1), draws[(1, 0, None)])
    a.epoch = 1
    assert np.array_equal(a.patch_transforms(1), draws[(1, 1, None)])
    # a prefix of a longer draw is not promised, but the length is honoured and all eight codes turn up
    many = a.patch_transforms(0, n=4096, epoch=0)
    assert many.shape == (4096,) and set(many.tolist()) == set(range(8))
    counts = np.bincount(many, minlength=8)
    assert counts.min() > 512 - 5 * 22 and counts.max() < 512 + 5 * 22        # uniform: 512 +- 5 sigma (sigma = sqrt(4096 * 7 / 64) = 21.2)


@pytest.mark.parametrize("launcher", ["train_kpcn", "train_sbmc", "train_lbmc"])
def test_launchers_take_the_flags_only_with_a_data_dir(launcher):
    import importlib
    from wcmc_amd import train_kpcn as tk
    mod = importlib.import_module("wcmc_amd." + launcher)
    extra = [] if launcher == "train_kpcn" else ["--denoiser", "json:dumps"]
    check = tk.check_args if launcher == "train_kpcn" else mod.ts.check_args if launcher == "train_lbmc" else mod.check_args
    parse = lambda *a: tk.parse_args(["--desc", "x", *extra, *a], mod.build_parser())      # noqa: E731
    args = parse()
    check(args)
    assert args.augment is False and args.augment_seed == 0 and tk.augment_loader_args(args) == {}
    args = parse("--from_data_dir", "--augment")
    check(args)
    assert tk.augment_loader_args(args) == {"augment": True, "augment_seed": 0}
    args = parse("--from_data_dir", "--augment", "--augment_seed", "11")
    check(args)
    assert tk.augment_loader_args(args) == {"augment": True, "augment_seed": 11}
    with pytest.raises(RuntimeError, match="`--augment` .* needs `--from_data_dir`"):
        check(parse("--augment"))
    with pytest.raises(RuntimeError, match="`--augment_seed` .* needs `--from_data_dir`"):
        check(parse("--augment_seed", "3"))
    with pytest.raises(RuntimeError, match="`--augment_seed` needs `--augment`"):
        check(parse("--from_data_dir", "--augment_seed", "3"))
    with pytest.raises(RuntimeError, match="`--augment_seed` should be non-negative"):
        check(parse("--from_data_dir", "--augment", "--augment_seed", "-1"))
    with pytest.raises(SystemExit):
        parse("--augment_seed", "three")
    text = mod.build_parser().format_help()
    assert "--augment" in text and "--augment_seed" in text
    # the launcher's own parser keeps the flag surface earlier tests pin: the two flags are read ahead of it
    assert not {"augment", "augment_seed"} & {a.dest for a in mod.build_parser()._actions}
