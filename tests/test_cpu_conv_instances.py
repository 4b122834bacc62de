"""The table of tests/conv_instances.py against the release library's own launch plan (wcmc_conv2d_launch_plan_bf16x3,
wcmc_conv2d_wgrad_launch_plan_bf16x3), without a GPU: the sweep names exactly the listed kernel instances, every instance has its
rows, and every row runs the instance it claims -- so tests/test_gpu_conv_instances.py, which launches the rows, cannot claim a
kernel it does not run, and an instance added to the dispatch fails here until it has rows."""
import collections
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import conv_instances as CI      # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from wcmc_amd import _lib
    assert _lib.LIB_PATH.endswith("libwcmc_hip.so") or os.environ.get("WCMC_DEBUG_LIB") == "1"
    return _lib.lib()


def _asker(L, length=128):
    """query -> kernel instance, or None where the plan refuses the arguments."""
    cls, ker = ctypes.create_string_buffer(length), ctypes.create_string_buffer(length)

    def ask(q):
        if q[0] == "w":
            rc = L.wcmc_conv2d_wgrad_launch_plan_bf16x3(*q[1:], cls, ker, length)
        else:
            n, h, w, cin, cout, ks, pad, terms, split, gate, f16 = q[1:12]
            ys = (0, 0, 0) if split else q[12] if len(q) > 12 else CI.dense_strides(cout, h + 2 * pad - ks + 1, w + 2 * pad - ks + 1)
            rc = L.wcmc_conv2d_launch_plan_bf16x3(n, h, w, cin, cout, ks, pad, terms, split, *ys, gate, f16, cls, ker, length)
        return ker.value.decode() if rc == 0 else None
    return ask


def test_the_sweep_yields_exactly_the_listed_instances(L):
    ask = _asker(L)
    found = {ask(q) for q in CI.sweep_queries()} - {None}
    assert CI.INSTANCES == sorted(CI.INSTANCES) and len(set(CI.INSTANCES)) == len(CI.INSTANCES)
    assert sorted(found) == CI.INSTANCES, {"not listed": sorted(found - set(CI.INSTANCES)), "no longer planned": sorted(set(CI.INSTANCES) - found)}


# what every family must see at least once (a gate tensor keeps a launch off conv_pw: x_plan_pw)
SEEN_BY_EVERY_FAMILY = ("gate=tensor", "gate=mask", "colsum", "mask_out", "out=split", "out=fp32", "out=fp32-in-wider-buffer")


def test_every_instance_has_a_smallest_and_a_ragged_row():
    rows = collections.defaultdict(list)
    for row in CI.CASES:
        assert len(row) == 11 and row[1] in ("f", "h", "w"), row
        CI.options(row)                                   # (every token is a known one)
        rows[row[0]].append(row)
    assert set(rows) == set(CI.INSTANCES), {"rows of an unlisted instance": sorted(set(rows) - set(CI.INSTANCES)),
                                            "without rows": sorted(set(CI.INSTANCES) - set(rows))}
    for instance in CI.INSTANCES:
        assert len(rows[instance]) >= 2, instance
        assert len(set(rows[instance])) == len(rows[instance]), instance
        assert any(r[2] >= 2 for r in rows[instance]), (instance, "no row with N >= 2")
    assert len(set(CI.CASES)) == len(CI.CASES)
    seen = collections.defaultdict(set)
    for row in CI.CASES:
        seen[CI.family(row[0])].update(row[10].split())
    for fam in ("pw", "halo3", "halo", "halo64", "igemm"):
        missing = [t for t in SEEN_BY_EVERY_FAMILY if t not in seen[fam] and not (fam == "pw" and t == "gate=tensor")]
        assert not missing, (fam, missing)
    assert {"bias", "colsum", "nobias"} <= seen["wgrad"]
    # the kernel sizes no other test launches: ks = 4 on the halo kernels, 2 and 7 on the streaming GEMM, 7 on the one-tap weight gradient
    ks_of = collections.defaultdict(set)
    for row in CI.CASES:
        ks_of[row[0].split("_bf16x3")[0]].add(row[7])
    assert 4 in ks_of["conv_halo"] and {2, 7} <= ks_of["conv_igemm"] and 7 in ks_of["conv_wgrad"]


@pytest.mark.parametrize("row", CI.CASES, ids=lambda r: "-".join(str(a) for a in r[1:10]) + "-" + r[10].replace(" ", ","))
def test_a_row_runs_the_instance_it_names(L, row):
    o = CI.options(row)
    if row[1] == "w":
        assert o["bias"] + o["colsum"] + o["nobias"] == 1, row
    else:
        assert o["out"] in ("split", "fp32", "fp32-in-wider-buffer") and o["gate"] in ("none", "tensor", "mask"), row
        # what the entry refuses: a gate, a mask or column sums with an fp32 output; anything but a dense un-gated fp32 view from the fp16 launch
        assert o["out"] == "split" or (o["gate"] == "none" and not o["colsum"] and not o["mask_out"]), row
        assert row[1] == "f" or (o["out"] == "fp32" and o["act"] == "linear"), row
    assert _asker(L)(CI.plan_query(row)) == row[0]
