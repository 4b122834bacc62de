#!/usr/bin/env python3
"""Generate ``tests/golden/sbmc_data.npz`` by running the REAL reference (``support/datasets.py``, the launchers' parsers).

Run on the development machine only (the reference tree is not on the GPU machine), as ``make_golden_dataset.py``:

    python tests/golden/make_golden_sbmc.py

pre/<case>/...     ``DenoiseDataset._preprocess_sbmc`` (:363-485) on three raws of ``make_golden.raw_samples`` with the SBMC channels
                   overridden (``sbmc_raw``): probabilities 24:48 signed, light directions 48:60 beyond +-1, bounce types 60:66
                   integers 0..31 -- every clamp and every tag bit.  The overrides are multiples of 1/8 (they compress).  The
                   test regenerates the inputs from the recorded seed; a crc of them is recorded.
                   ``pre/int16_overflow``: what ``astype(np.int16)`` made of a bounce code of 1e38 on the machine that wrote the
                   golden (1 = all five tags 0, as the kernel defines it).  The value is NOT part of the three cases.
item/<combo>/<window>/<key>
                   ``DenoiseDataset.__getitem__`` (:1026-1146) with ``sampling='grid'`` over one (40, 48, 4) scene, PATCH_SIZE
                   lowered to 16 on the instance, for use_g_buf x use_sbmc_buf x use_llpm_buf and for base_model='lbmc' (llpm on and
                   off); ``_sbmc_s`` / ``_sbmc_p`` / ``_llpm`` / ``_prob_imp`` written by the real ``_offline_preprocess`` (:584-715) in a
                   temporary directory (placeholders named ``_llpm_<k>.npy`` keep its continuation loop, :632-641, from opening
                   continuation files that do not exist).  Windows 0, 1 and 5 of the grid: origins (0, 0), (0, 16) and (16, 32), the
                   last whole one.  The scene is ``scene_raw``: eleven records of ``sbmc_raw`` laid out as record[(y + 3x + 5s) % 11],
                   so that every plane of an item is periodic (the file stays small) while every step along y, x, s or c, and every
                   window shift, changes the values.
item8/...          the same for a (19, 21, 3) scene with PATCH_SIZE 8, all buffers on: windows 0 and 4 (origins (0, 0), (8, 8)).
sizes/<combo>      (dncnn_in_size, pnet_in_size) of every combination at pnet_out_size 3 and 0; names/<combo>: the files written.
full/...           one tile of ``FullImageDataset('sbmc')`` (:1174-1425) over a (128, 128, 2) scene, with its ``has_hit``.
parser/<launcher>  names, defaults and actions of ``train_sbmc.py`` / ``train_lbmc.py``'s argument parsers: the ``add_argument`` calls
                   of their ``__main__`` blocks evaluated on the reference's own ``BasicArgumentParser`` (json).

Only data is written.
"""
import ast
import io
import json
import os
import sys
import tempfile
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_dataset as mgd  # noqa: E402

# name: (h, w, s, seed)
PRE = {"a": (12, 10, 4, 911), "b": (9, 17, 8, 912), "c": (6, 5, 2, 913)}
SCENE = (40, 48, 4, 921, 931)                       # h, w, s, raw seed, gt seed
SCENE_PATCH, SCENE_WINDOWS = 16, {0: (0, 0), 1: (0, 16), 5: (16, 32)}
SCENE8 = (19, 21, 3, 922, 932)
SCENE8_PATCH, SCENE8_WINDOWS = 8, {0: (0, 0), 4: (8, 8)}
FULL = (128, 128, 2, 923, 933)
# combo: (base_model, use_g_buf, use_sbmc_buf, use_llpm_buf)
COMBOS = {"g%d_p%d_l%d" % (g, p, l): ("sbmc", bool(g), bool(p), bool(l)) for g in (1, 0) for p in (1, 0) for l in (1, 0)}
COMBOS.update({"lbmc_l1": ("lbmc", False, True, True), "lbmc_l0": ("lbmc", False, True, False)})   # (lbmc overrides both flags)


def sbmc_raw(h, w, s, seed):
    """``make_golden.raw_samples`` with the channels only ``_preprocess_sbmc`` reads overridden (multiples of 1/8)."""
    x = mg.raw_samples(h, w, s, seed)
    rng = np.random.RandomState(seed + 5000)
    x[..., 24:48] = rng.randint(-16, 48, size=(h, w, s, 24)).astype(np.float32) / 8.0          # signed: max(prob, 0)
    x[..., 48:60] = rng.randint(-20, 21, size=(h, w, s, 12)).astype(np.float32) / 8.0          # beyond +-1: the clip
    x[..., 60:66] = rng.randint(0, 32, size=(h, w, s, 6)).astype(np.float32)                   # every tag bit
    return x


def scene_raw(h, w, s, seed):
    """(h, w, s, 104): record[(y + 3x + 5s) % 11] of eleven ``sbmc_raw`` records."""
    table = sbmc_raw(11, 1, 1, seed)[:, 0, 0, :]
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(s), indexing="ij")
    return np.ascontiguousarray(table[(y + 3 * x + 5 * k) % 11])


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.float32).tobytes())


def write_scene(rd, root, name, raw, gt, patch, spp):
    """The scene's files under root/train, preprocessed by the real ``_offline_preprocess``; returns the names written."""
    for d in ("gt", "input"):
        os.makedirs(os.path.join(root, "train", d), exist_ok=True)
    inp = os.path.join(root, "train", "input")
    np.save(os.path.join(root, "train", "gt", name + ".npy"), gt)
    np.save(os.path.join(inp, name + ".npy"), raw)
    placeholders = [os.path.join(inp, "%s_llpm_%d.npy" % (name, k)) for k in range(1, 8)]
    for f in placeholders:
        open(f, "wb").close()
    ds = rd.DenoiseDataset(root, spp, base_model="sbmc", mode="train", use_llpm_buf=True)
    ds.PATCH_SIZE = patch
    ds._offline_preprocess(llpm=True, sbmc=True, kpcn=False, overwrite=False)
    for f in placeholders:
        os.remove(f)
    return sorted(os.listdir(inp))


def gen_preprocess(rd, out):
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "train", "gt"))
        ds = rd.DenoiseDataset(tmp, 4, base_model="sbmc", mode="train")
        for name, (h, w, s, seed) in PRE.items():
            x = sbmc_raw(h, w, s, seed)
            ss, pp = ds._preprocess_sbmc(x.copy())
            assert ss.shape == (h, w, s, 27) and pp.shape == (h, w, s, 66) and ss.dtype == pp.dtype == np.float32
            out["pre/%s/params" % name] = np.array([h, w, s, seed], dtype=np.int64)
            out["pre/%s/raw_crc" % name] = np.int64(crc(x))
            out["pre/%s/sbmc_s" % name], out["pre/%s/sbmc_p" % name] = ss, pp
        x = sbmc_raw(2, 2, 2, 914)
        x[..., 60:66] = np.float32(1.0e+38)
        with np.errstate(all="ignore"):
            _, pp = ds._preprocess_sbmc(x)
        out["pre/int16_overflow"] = np.int64(int(not pp[..., 36:].any()))
        print("bounce code 1e38 -> all tags zero on this machine:", bool(out["pre/int16_overflow"]))


def gen_items(rd, out, tag, scene, patch, windows, combos):
    h, w, s, seed, gseed = scene
    raw, gt = scene_raw(h, w, s, seed), mgd.test_gt(h, w, gseed)
    out["%s/params" % tag] = np.array([h, w, s, seed, gseed, patch], dtype=np.int64)
    out["%s/raw_crc" % tag] = np.int64(crc(raw))
    with tempfile.TemporaryDirectory() as tmp:
        names = write_scene(rd, tmp, "scene", raw, gt, patch, s)
        out["%s/files" % tag] = np.array(names)
        for combo in combos:
            bm, g, p, l = COMBOS[combo]
            ds = rd.DenoiseDataset(tmp, s, base_model=bm, mode="train", batch_size=8, sampling="grid", use_g_buf=g, use_sbmc_buf=p,
                                   use_llpm_buf=l, pnet_out_size=3)
            ds0 = rd.DenoiseDataset(tmp, s, base_model=bm, mode="train", use_g_buf=g, use_sbmc_buf=p, use_llpm_buf=l, pnet_out_size=0)
            out["sizes/%s" % combo] = np.array([ds.dncnn_in_size, ds.pnet_in_size, ds0.dncnn_in_size, ds0.pnet_in_size], dtype=np.int64)
            out["flags/%s" % combo] = np.array([ds.base_model == "sbmc", ds.use_g_buf, ds.use_sbmc_buf, ds.use_llpm_buf], dtype=np.int64)
            ds.PATCH_SIZE = patch
            ds[0]                                                    # item 0 cuts the grid
            for i, origin in windows.items():
                it = ds[i]
                assert it["target_image"].shape == (3, patch, patch), (combo, i, it["target_image"].shape)
                assert np.array_equal(it["target_image"], gt[origin[0]:origin[0] + patch, origin[1]:origin[1] + patch, :3].transpose(2, 0, 1))
                for k, v in it.items():
                    out["%s/%s/%d/%s" % (tag, combo, i, k)] = np.ascontiguousarray(v)
            print(tag, combo, {k: v.shape for k, v in it.items()}, "dncnn_in_size", ds.dncnn_in_size)


def gen_full(rd, out):
    """One FullImageDataset('sbmc') tile; the class needs no mount paths when every file is where it first looks."""
    h, w, s, seed, gseed = FULL
    raw, gt = scene_raw(h, w, s, seed), mgd.test_gt(h, w, gseed)
    raw[:7, :, :, 60] = 0.0                                          # rows without a hit (has_hit reads the first bounce type)
    out["full/params"] = np.array([h, w, s, seed, gseed], dtype=np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        write_scene(rd, tmp, "scene", raw, gt, 16, s)
        ds = rd.FullImageDataset(os.path.join(tmp, "train", "input", "scene.npy"), s, "sbmc", True, True, True, 3)
        assert len(ds) == 1
        item, i0, j0, i1, j1, i, j = ds[0]
        out["full/coords"] = np.array([i0, j0, i1, j1, i, j], dtype=np.int64)
        out["full/has_hit"] = np.ascontiguousarray(ds.has_hit)
        out["full/sizes"] = np.array([ds.dncnn_in_size, ds.pnet_in_size], dtype=np.int64)
        for k, v in item.items():
            out["full/item/%s" % k] = np.ascontiguousarray(v)
        print("full", {k: v.shape for k, v in item.items()}, "has_hit", ds.has_hit.shape, float(ds.has_hit.mean()))


def parser_table(ru, launcher):
    """The add_argument calls of the launcher's ``__main__`` block on the reference's BasicArgumentParser: {dest: [default, action]}."""
    tree = ast.parse(open(os.path.join(mg.REF, launcher)).read())
    parser = ru.BasicArgumentParser()
    for node in ast.walk(tree):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument"
                and isinstance(node.func.value, ast.Name) and node.func.value.id == "parser"):
            eval(compile(ast.Expression(node), launcher, "eval"), {"parser": parser})
    return {a.dest: [a.default, type(a).__name__, list(a.option_strings), bool(a.required)]
            for a in parser._actions if a.dest != "help"}


def main():
    mg.import_reference()
    np.bool = bool                                     # the reference predates numpy 1.24 (datasets.py:430-438)
    import support.datasets as rd
    import support.utils as ru
    out = {}
    gen_preprocess(rd, out)
    gen_items(rd, out, "item", SCENE, SCENE_PATCH, SCENE_WINDOWS, list(COMBOS))
    gen_items(rd, out, "item8", SCENE8, SCENE8_PATCH, SCENE8_WINDOWS, ["g1_p1_l1"])
    gen_full(rd, out)
    for launcher in ("train_sbmc.py", "train_lbmc.py"):
        out["parser/" + launcher[:-3]] = np.array(json.dumps(parser_table(ru, launcher), sort_keys=True))
    fn = os.path.join(HERE, "sbmc_data.npz")
    # an .npz whose members are LZMA-compressed (numpy.load reads them through zipfile as it reads deflated ones): the periodic
    # planes repeat at distances beyond deflate's 32 KB window -- 470 KB instead of 910 KB
    with zipfile.ZipFile(fn, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in out.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(k + ".npy", b.getvalue())
    print("sbmc_data.npz: %d entries, %d bytes" % (len(out), os.path.getsize(fn)))


if __name__ == "__main__":
    main()
