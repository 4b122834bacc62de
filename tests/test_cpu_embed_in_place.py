"""The in-place entries of the fused PathNet.embedding (``wcmc_embed3_*_nchw``): what can be checked without a GPU."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wcmc_embed3_nchw_supported", "wcmc_embed3_mean_fwd_nchw", "wcmc_embed3_bwd_nchw")


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
    # H * W = 60: not readable in place; null x; misaligned x
    assert h.wcmc_embed3_mean_fwd_nchw(P(a), 36 * 60, 60, 120, 36, *w, 1, 60, None) < 0
    assert b"wcmc_embed3_nchw_supported" in h.wcmc_last_error()
    assert h.wcmc_embed3_mean_fwd_nchw(None, 36 * 64, 64, 128, 36, *w, 1, 64, None) < 0
    assert h.wcmc_embed3_mean_fwd_nchw(P(a + 2), 36 * 64, 64, 128, 36, *w, 1, 64, None) < 0
    g = [P(a)] * 7
    assert h.wcmc_embed3_bwd_nchw(None, 36 * 64, 64, 128, 36, *g, 64, P(a), 64, 1, 64, 1.0, *([P(a)] * 6), P(a), 1 << 30, None) < 0
    assert h.wcmc_embed3_bwd_nchw(P(a), 36 * 64, 63, 128, 36, *g, 64, P(a), 64, 1, 64, 1.0, *([P(a)] * 6), P(a), 1 << 30, None) < 0


def test_header_binding_and_integration_notes_list_the_entries():
    from wcmc_amd._lib import SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wcmc_hip.h")).read(), flags=re.S)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m and name in SIGNATURES and name in notes, name
        assert len(m.group(1).split(",")) == len(SIGNATURES[name][1]), name
    # the in-place entries take (x, sample stride, channel stride) where the split entries take x_split
    for new, old in (("wcmc_embed3_mean_fwd_nchw", "wcmc_embed3_mean_fwd"), ("wcmc_embed3_bwd_nchw", "wcmc_embed3_bwd")):
        assert len(SIGNATURES[new][1]) == len(SIGNATURES[old][1]) + 2 and SIGNATURES[new][1][3:] == SIGNATURES[old][1][1:]
    assert "EMBED_IN_PLACE" in notes
