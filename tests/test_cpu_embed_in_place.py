"""The in-place form of the fused PathNet.embedding (the ``x_nchw`` source of ``wcmc_embed3_mean_fwd`` / ``wcmc_embed3_bwd``): what
can be checked without a GPU."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wcmc_embed3_nchw_supported", "wcmc_embed3_mean_fwd", "wcmc_embed3_bwd")
# ABI 4 folded the in-place spellings (and the final chain's _save / _saved ones) into the base names: these four are gone
GONE = ("wcmc_embed3_mean_fwd_nchw", "wcmc_embed3_bwd_nchw", "wcmc_final2_fwd_save", "wcmc_final2_bwd_saved")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from wcmc_amd._lib import lib
    return lib()


def test_supported_query_answers_without_a_device():
    h = _lib()
    q = h.wcmc_embed3_nchw_supported
    dense = lambda c, n, hh, ww: (c, n, hh, ww, c * hh * ww, hh * ww, ww, 1)
    assert q(*dense(36, 64, 128, 128)) == 1                   # the benchmark's `paths`
    assert q(*dense(36, 2, 8, 8)) == 1 and q(*dense(1, 1, 8, 8)) == 1 and q(*dense(64, 4, 8, 8)) == 1
    assert q(*dense(65, 4, 8, 8)) == 0 and q(*dense(0, 4, 8, 8)) == 0           # Cin in 1..64
    assert q(*dense(36, 6, 20, 23)) == 0 and q(*dense(36, 2, 4, 8)) == 0        # H * W % 64: a tile lies in one sample
    assert q(36, 4, 8, 8, 36 * 128, 128, 16, 2) == 0                            # W stride 2
    assert q(36, 4, 8, 8, 36 * 128, 128, 16, 1) == 0                            # rows apart: the plane is not one run
    assert q(36, 4, 8, 8, 45 * 64 + 7, 64, 8, 1) == 1 and q(36, 4, 8, 8, 45 * 100, 100, 8, 1) == 1      # a slice in N and C
    assert q(36, 4, 8, 8, 36 * 64, 63, 8, 1) == 0                               # channel planes overlap
    assert q(36, 4, 8, 8, -36 * 64, 64, 8, 1) == 0 and q(36, 1, 8, 8, 0, 64, 8, 1) == 1
    assert q(36, 1 << 20, 8, 8, 36 * 64, 64, 8, 1) == 0                         # y would pass 2 GiB
    assert q(36, 2, 8, 8, 1 << 40, 1 << 30, 8, 1) == 0                          # 64 channel rows do not fit 31 bits of offset


def test_python_predicate_follows_the_switches(monkeypatch):
    _lib()
    from wcmc_amd import ops
    x = torch.zeros(4, 36, 8, 16)
    if ops.reduced_backward():
        assert ops.embed_in_place_supported(x) and ops.embed_in_place_supported(x[1:3, 2:30])
    assert not ops.embed_in_place_supported(x, (16, 16, 16))                    # no fused chain for these widths
    assert not ops.embed_in_place_supported(x[..., ::2]) and not ops.embed_in_place_supported(x[:, :, :5])
    assert not ops.embed_in_place_supported(x.double()) and not ops.embed_in_place_supported(x.clone().requires_grad_(True))
    for name in ("EMBED_IN_PLACE", "FUSE_EMBED"):
        monkeypatch.setattr(ops, name, False)
        assert not ops.embed_in_place_supported(x)
        monkeypatch.setattr(ops, name, True)
    monkeypatch.setattr(ops, "PRECISION", "bf16x3")
    assert not ops.embed_in_place_supported(x)


def test_entries_reject_bad_arguments_before_any_launch():
    import ctypes
    h = _lib()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    P = ctypes.c_void_p
    w = [P(a)] * 8
    BAD_ARG, ALIGNMENT = -1, -2
    err = lambda: h.wcmc_last_error().decode()
    # H * W = 60: not readable in place; neither source; both sources; misaligned x_nchw
    assert h.wcmc_embed3_mean_fwd(None, P(a), 36 * 60, 60, 120, 36, *w, 1, 60, None) == BAD_ARG
    assert "wcmc_embed3_nchw_supported" in err()
    assert h.wcmc_embed3_mean_fwd(None, None, 36 * 64, 64, 128, 36, *w, 1, 64, None) == BAD_ARG and "neither" in err()
    assert h.wcmc_embed3_mean_fwd(P(a), P(a), 36 * 64, 64, 128, 36, *w, 1, 64, None) == BAD_ARG and "both" in err()
    assert h.wcmc_embed3_mean_fwd(None, P(a + 2), 36 * 64, 64, 128, 36, *w, 1, 64, None) == ALIGNMENT
    g = [P(a)] * 7
    tail = (64, P(a), 64, 1, 64, 1.0, *([P(a)] * 6), P(a), 1 << 30, None)
    assert h.wcmc_embed3_bwd(None, None, 36 * 64, 64, 128, 36, *g, *tail) == BAD_ARG and "neither" in err()
    assert h.wcmc_embed3_bwd(P(a), P(a), 36 * 64, 64, 128, 36, *g, *tail) == BAD_ARG and "both" in err()
    assert h.wcmc_embed3_bwd(None, P(a), 36 * 64, 63, 128, 36, *g, *tail) == BAD_ARG                   # channel planes overlap
    assert "wcmc_embed3_nchw_supported" in err()


def test_header_binding_and_integration_notes_list_the_entries():
    from wcmc_amd._lib import SIGNATURES, I, L, P
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wcmc_hip.h")).read(), flags=re.S)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m and name in SIGNATURES and name in notes, name
        assert len(m.group(1).split(",")) == len(SIGNATURES[name][1]), name
        if name != NEW[0]:      # both sources lead: (x_split, x_nchw, sample stride, channel stride, M, Cin, ...)
            lead = [p.strip() for p in m.group(1).split(",")[:6]]
            assert [p.rsplit(None, 1)[-1].lstrip("*") for p in lead] == ["x_split", "x_nchw", "x_sample_stride", "x_channel_stride", "M", "Cin"]
            assert SIGNATURES[name][1][:6] == [P, P, L, L, L, I], name
    # the plain forward keeps the split source alone: the merged entries take three arguments more in its place
    assert len(SIGNATURES["wcmc_embed3_mean_fwd"][1]) == len(SIGNATURES["wcmc_embed3_fwd"][1]) + 3 + 3
    for name in GONE:
        assert name not in SIGNATURES and not re.search(r"\b%s\b" % name, header), name
    assert "EMBED_IN_PLACE" in notes
