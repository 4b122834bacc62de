"""Which kernel a split-bf16 conv launch runs, asked of the library's own launch plan (wcmc_conv2d_launch_plan_bf16x3,
wcmc_conv2d_wgrad_launch_plan_bf16x3) against a frozen table.  CPU tests on the release library: that they pass on a machine
without a GPU is the proof that the query touches no device.

The classes of the table were produced at the commit before the query existed, by the Python mirror of the dispatch it replaced
(ops/_base.py: _igemm_class, _wgrad_class), the kernel names by reading the dispatch; where the mirror was wrong the row says so."""
import ctypes
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from wcmc_amd import _lib
    assert _lib.LIB_PATH.endswith("libwcmc_hip.so") or os.environ.get("WCMC_DEBUG_LIB") == "1"
    return _lib.lib()


# Row: (arguments, profiler class, kernel instance as rocprofv3 prints it without "wcmc::").
#   ("f", N, H, W, Cin, Cout, ks, pad, terms, split output, gate tensor, fp16 launch): wcmc_conv2d_igemm_bf16x3 / wcmc_conv2d_out_f16
#   (an fp32 output is the dense NHWC view ops.nhwc_empty makes, or has the strides (sn, sh, sw) appended to the row); ("w", N, H, W, Cin, Cout, ks, pad, terms): wcmc_conv2d_wgrad_bf16x3.
# (a) every distinct conv launch of one step of the benchmark in its default mode (B = 8, spp = 8, 128 x 128 patches; both PathNets,
# weight-normalised, feeding KPCN through pbuffer_cat; forward and backward with a profiler set), in launch order: the queries logged
# during one profiled step on the MI355X, and the same list derived without a GPU by running the models with every library launch
# stubbed out.  The PathNets' 1x1 chains run the fused kernels of pathnet_fused.hip there and launch no GEMM of these entry points.
# The classes are those of the Python mirror this table replaced, which agreed on every row.
BENCH_ROWS = [
    (('f', 8, 128, 128, 64, 64, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 128, 128, 64, 64, 3, 1, 3, 0, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 64, 64, 64, 128, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 64, 64, 128, 128, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 64, 64, 128, 128, 3, 1, 3, 0, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 32, 32, 128, 256, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 32, 32, 256, 256, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 32, 32, 256, 256, 3, 1, 3, 0, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 64, 64, 384, 128, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 128, 128, 192, 64, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 128, 128, 39, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 124, 124, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 120, 120, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 116, 116, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 112, 112, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 108, 108, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 104, 104, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 100, 100, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt3', 'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 2, 2, 0>'),
    (('f', 8, 96, 96, 100, 441, 5, 0, 1, 0, 0, 1), 'conv_halo64_pt4_h1', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 1>'),
    (('w', 8, 96, 96, 100, 441, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('f', 8, 92, 92, 441, 100, 5, 4, 2, 1, 0, 0), 'conv_halo64_pt3_x2', 'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 2, 0>'),
    (('w', 8, 100, 100, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('f', 8, 96, 96, 100, 100, 5, 4, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('w', 8, 104, 104, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('f', 8, 100, 100, 100, 100, 5, 4, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('w', 8, 108, 108, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('f', 8, 104, 104, 100, 100, 5, 4, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('w', 8, 112, 112, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('f', 8, 108, 108, 100, 100, 5, 4, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('w', 8, 116, 116, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('f', 8, 112, 112, 100, 100, 5, 4, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('w', 8, 120, 120, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('f', 8, 116, 116, 100, 100, 5, 4, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('w', 8, 124, 124, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('f', 8, 120, 120, 100, 100, 5, 4, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('w', 8, 128, 128, 39, 100, 5, 0, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 1>'),
    (('f', 8, 124, 124, 100, 7, 5, 4, 2, 0, 0, 0, (655360, 5120, 40)), 'conv_igemm', 'conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 1, 2, 0>'),
    (('w', 8, 128, 128, 64, 64, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 1>'),
    (('f', 8, 128, 128, 64, 64, 3, 1, 2, 1, 0, 0), 'conv_halo3_x2', 'conv_halo3_bf16x3_kernel<1, 2, 2, 0>'),
    (('w', 8, 128, 128, 192, 64, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 1>'),
    (('f', 8, 128, 128, 64, 192, 3, 1, 2, 0, 0, 0), 'conv_halo3_x2', 'conv_halo3_bf16x3_kernel<1, 2, 2, 0>'),
    (('w', 8, 64, 64, 128, 128, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 1>'),
    (('f', 8, 64, 64, 128, 128, 3, 1, 2, 1, 0, 0), 'conv_halo3_x2', 'conv_halo3_bf16x3_kernel<1, 4, 2, 0>'),
    (('w', 8, 64, 64, 384, 128, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 1>'),
    (('f', 8, 64, 64, 128, 384, 3, 1, 2, 0, 0, 0), 'conv_halo3_x2', 'conv_halo3_bf16x3_kernel<1, 4, 2, 0>'),
    (('w', 8, 32, 32, 256, 256, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 1>'),
    (('f', 8, 32, 32, 256, 256, 3, 1, 2, 1, 0, 0), 'conv_halo3_x2', 'conv_halo3_bf16x3_kernel<1, 4, 2, 0>'),
    (('w', 8, 32, 32, 128, 256, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 1>'),
    (('f', 8, 32, 32, 256, 128, 3, 1, 2, 0, 0, 0), 'conv_halo3_x2', 'conv_halo3_bf16x3_kernel<1, 4, 2, 0>'),
    (('w', 8, 64, 64, 64, 128, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 1>'),
    (('f', 8, 64, 64, 128, 64, 3, 1, 2, 0, 0, 0), 'conv_halo3_x2', 'conv_halo3_bf16x3_kernel<1, 4, 2, 0>'),
    (('f', 8, 128, 128, 64, 64, 3, 1, 2, 0, 0, 0), 'conv_halo3_x2', 'conv_halo3_bf16x3_kernel<1, 2, 2, 0>'),
]
# (b) the edges of the plans: 5x5 100 -> 100 at the output heights where the 12- and the 16-row tilings trade places and mix (N = 1, 8);
# the two- / one-term grants and their refusals; the 3x3 slab rules; the pointwise pairs and what keeps a 1x1 launch off them; every
# row of tests/test_gpu_ops.py: WGRAD_TERM_CASES; the 64-row threshold of the filter-row weight gradient; 14 cin tiles
EDGE_ROWS = [
    (('f', 1, 96, 96, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 1, 100, 100, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt3', 'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 2, 2, 0>'),
    (('f', 1, 104, 104, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 1, 108, 108, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 1, 112, 112, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 1, 120, 120, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 1, 124, 124, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 1, 128, 128, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 1, 132, 132, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt3', 'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 2, 2, 0>'),
    (('f', 8, 96, 96, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 100, 100, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt3', 'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 2, 2, 0>'),
    (('f', 8, 104, 104, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 108, 108, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 112, 112, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 120, 120, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 124, 124, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 128, 128, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 132, 132, 100, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 132, 132, 100, 100, 5, 0, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('f', 8, 132, 132, 120, 100, 5, 0, 2, 1, 0, 0), 'conv_halo64_pt4', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 132, 132, 441, 100, 5, 0, 3, 1, 0, 0), 'conv_halo64_cs32', 'conv_halo64_bf16x3_kernel<7, 2, 3, 0, 160, 2, 2, 0>'),
    (('f', 8, 132, 132, 441, 100, 5, 0, 2, 1, 0, 0), 'conv_halo64_pt4_x2', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>'),
    (('f', 8, 132, 132, 100, 100, 5, 0, 1, 0, 0, 0), 'conv_halo64_pt4_x1', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 0>'),
    (('f', 8, 132, 132, 100, 100, 5, 0, 1, 0, 0, 1), 'conv_halo64_pt4_h1', 'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 1>'),
    # (96 output rows: the 12-row tiling of the two-term, one-term and fp16 instances)
    (('f', 8, 100, 100, 100, 100, 5, 0, 2, 1, 0, 0), 'conv_halo64_pt3_x2', 'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 2, 0>'),
    (('f', 8, 100, 100, 100, 100, 5, 0, 1, 0, 0, 0), 'conv_halo64_pt3_x1', 'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 1, 0>'),
    (('f', 8, 100, 100, 100, 100, 5, 0, 1, 0, 0, 1), 'conv_halo64_pt3_h1', 'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 1, 1>'),
    (('f', 8, 132, 132, 100, 39, 5, 0, 3, 1, 0, 0), 'conv_igemm', 'conv_halo64_bf16x3_kernel<4, 3, 4, 0, 80, 2, 2, 0>'),
    (('f', 8, 132, 132, 100, 16, 5, 0, 2, 1, 0, 0), 'conv_igemm', 'conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 1, 2, 0>'),
    (('f', 8, 64, 64, 64, 64, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 64, 64, 128, 128, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 64, 64, 192, 64, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 64, 64, 192, 64, 3, 1, 2, 1, 0, 0), 'conv_igemm', 'conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 1>'),
    (('f', 8, 64, 64, 40, 64, 3, 1, 3, 1, 0, 0), 'conv_igemm', 'conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 2>'),
    (('f', 8, 64, 64, 64, 32, 3, 1, 3, 1, 0, 0), 'conv_igemm', 'conv_halo_bf16x3_kernel<2, 8, 16, 0, 2, 2>'),
    (('f', 8, 64, 64, 24, 64, 3, 1, 3, 1, 0, 0), 'conv_igemm', 'conv_igemm_bf16x3_kernel<4, true, true, 0>'),
    # (512 -> 512 has cins and couts in whole 64s: conv_halo3 at any size; the 8x16 tiling of small grids is the 40 -> 64 and 64 -> 32 rows' kernel)
    (('f', 8, 8, 8, 512, 512, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 16, 16, 512, 512, 3, 1, 3, 1, 0, 0), 'conv_halo3', 'conv_halo3_bf16x3_kernel<2, 2, 2, 0>'),
    (('f', 8, 128, 128, 64, 64, 1, 0, 3, 1, 0, 0), 'conv_pw', 'conv_pw_bf16x3_kernel<4, 16, true, 0>'),
    (('f', 8, 128, 128, 36, 64, 1, 0, 3, 1, 0, 0), 'conv_pw', 'conv_pw_bf16x3_kernel<4, 10, true, 0>'),
    (('f', 8, 128, 128, 128, 128, 1, 0, 3, 1, 0, 0), 'conv_pw', 'conv_pw_bf16x3_kernel<8, 32, true, 0>'),
    (('f', 8, 128, 128, 3, 128, 1, 0, 3, 1, 0, 0), 'conv_pw', 'conv_pw_bf16x3_kernel<8, 2, true, 0>'),
    (('f', 8, 128, 128, 128, 3, 1, 0, 3, 1, 0, 0), 'conv_igemm', 'conv_igemm_bf16x3_kernel<1, false, true, 0>'),
    (('f', 8, 128, 128, 64, 64, 1, 1, 3, 1, 0, 0), 'conv_igemm', 'conv_igemm_bf16x3_kernel<4, true, true, 0>'),
    (('f', 8, 128, 128, 64, 64, 1, 0, 3, 1, 1, 0), 'conv_igemm', 'conv_igemm_bf16x3_kernel<4, false, true, 0>'),      # (the Python mirror this table replaced said conv_pw)
    (('w', 8, 44, 44, 100, 100, 5, 0, 3), 'conv_wgrad_rows', 'conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>'),
    (('w', 8, 44, 44, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('w', 2, 30, 101, 100, 100, 5, 2, 3), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<7, 2>'),
    (('w', 2, 30, 101, 100, 100, 5, 2, 1), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<7, 1>'),
    (('w', 3, 30, 101, 100, 100, 5, 2, 3), 'conv_wgrad_rows', 'conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>'),
    (('w', 3, 30, 101, 100, 100, 5, 2, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('w', 2, 40, 40, 100, 441, 5, 0, 3), 'conv_wgrad_rows', 'conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>'),
    (('w', 2, 40, 40, 100, 441, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('w', 2, 40, 37, 39, 100, 5, 0, 3), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 2>'),
    (('w', 2, 40, 37, 39, 100, 5, 0, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 1>'),
    (('w', 1, 70, 35, 256, 128, 3, 1, 3), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 2>'),
    (('w', 1, 70, 35, 256, 128, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 1>'),
    (('w', 2, 40, 37, 64, 64, 3, 1, 3), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 2>'),
    (('w', 2, 40, 37, 64, 64, 3, 1, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 1>'),
    (('w', 12, 48, 40, 128, 128, 1, 0, 3), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<1, 8, 8, 0, 2>'),
    (('w', 12, 48, 40, 128, 128, 1, 0, 1), 'conv_wgrad', 'conv_wgrad_rows_bf16x3_kernel<1, 8, 8, 0, 1>'),
    (('w', 16, 64, 64, 36, 64, 1, 0, 3), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<4, 2>'),
    (('w', 16, 64, 64, 36, 64, 1, 0, 1), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<4, 1>'),
    (('w', 2, 11, 13, 34, 100, 5, 0, 3), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<7, 2>'),
    (('w', 2, 11, 13, 34, 100, 5, 0, 1), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<7, 1>'),
    (('w', 3, 9, 10, 128, 3, 1, 0, 3), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<4, 2>'),
    (('w', 3, 9, 10, 128, 3, 1, 0, 1), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<4, 1>'),
    (('w', 1, 67, 68, 100, 100, 5, 0, 3), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<7, 2>'),
    (('w', 1, 68, 68, 100, 100, 5, 0, 3), 'conv_wgrad_rows', 'conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>'),
    (('w', 8, 36, 36, 224, 100, 5, 0, 3), 'conv_wgrad_rows', 'conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>'),      # (the Python mirror this table replaced said conv_wgrad)
    (('w', 1, 67, 68, 100, 100, 5, 0, 1), 'conv_wgrad', 'conv_wgrad_bf16x3_kernel<7, 1>'),
    (('w', 1, 68, 68, 100, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),
    (('w', 8, 36, 36, 224, 100, 5, 0, 1), 'conv_wgrad_rows', 'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>'),      # (the Python mirror this table replaced said conv_wgrad)
]


def _strides(cout, ho, wo):
    cp = (cout + 3) // 4 * 4
    return (ho * wo * cp, wo * cp, cp)


def _ask(L, args, length=128):
    """(status, class, kernel) of one row's arguments."""
    cls, ker = ctypes.create_string_buffer(length), ctypes.create_string_buffer(length)
    if args[0] == "w":
        rc = L.wcmc_conv2d_wgrad_launch_plan_bf16x3(*args[1:], cls, ker, length)
    else:
        n, h, w, cin, cout, ks, pad, terms, split, gate, f16 = args[1:12]
        ys = (0, 0, 0) if split else args[12] if len(args) > 12 else _strides(cout, h + 2 * pad - ks + 1, w + 2 * pad - ks + 1)
        rc = L.wcmc_conv2d_launch_plan_bf16x3(n, h, w, cin, cout, ks, pad, terms, split, *ys, gate, f16, cls, ker, length)
    return rc, cls.value.decode(), ker.value.decode()


@pytest.mark.parametrize("row", BENCH_ROWS + EDGE_ROWS, ids=lambda r: "-".join(str(a) for a in r[0]))
def test_launch_plan_matches_the_frozen_table(L, row):
    args, cls, kernel = row
    assert _ask(L, args) == (0, cls, kernel)


def test_single_kernel_classes_name_the_kernel_the_benchmark_prints(L):
    """A class that bench.rocprof_names maps to ONE kernel instance is given to that instance only: bench's string contains the
    library's kernel name (conv_pw and conv_halo3_x2 stand for several instances there and are not held to it)."""
    import bench
    checked = set()
    for args, cls, kernel in BENCH_ROWS + EDGE_ROWS:
        terms = args[-1] if args[0] == "w" else 3
        printed = bench.rocprof_names(terms if terms in (1, 3) else 3).get(cls)
        if printed is None or cls in ("conv_pw", "conv_halo3_x2"):
            assert cls in ("conv_igemm", "conv_wgrad", "conv_pw", "conv_halo3_x2"), cls
            continue
        assert "wcmc::" + kernel in printed, (args, cls, kernel, printed)
        checked.add(cls)
    # every single-instance class of bench.rocprof_names but conv_halo7, which the release library never runs (the debug-library test below)
    assert {"conv_halo64_pt3", "conv_halo64_pt4", "conv_halo64_pt3_x2", "conv_halo64_pt4_x2", "conv_halo64_pt3_x1", "conv_halo64_pt4_x1",
            "conv_halo64_pt3_h1", "conv_halo64_pt4_h1", "conv_halo64_cs32", "conv_halo3", "conv_wgrad_rows"} == checked


def test_debug_library_query_follows_its_switches(L, monkeypatch):
    """The A/B switches are read inside the plan functions: libwcmc_hip_debug.so answers for the kernel the switch selects, the release
    library reads no environment variable."""
    import bench
    from wcmc_amd import _lib
    D = ctypes.CDLL(os.path.join(ROOT, "wcmc_amd", "libwcmc_hip_debug.so"))
    for name in ("wcmc_conv2d_launch_plan_bf16x3", "wcmc_conv2d_wgrad_launch_plan_bf16x3"):
        getattr(D, name).restype, getattr(D, name).argtypes = _lib.SIGNATURES[name]
    cases = (   # switch, a row of the table above, (class, kernel) under the switch
        ("WCMC_HALO64", ("f", 8, 132, 132, 100, 100, 5, 0, 3, 1, 0, 0), ("conv_halo7", "conv_halo_bf16x3_kernel<7, 8, 16, 0, 2, 2>")),
        ("WCMC_HALO3", ("f", 8, 64, 64, 64, 64, 3, 1, 3, 1, 0, 0), ("conv_igemm", "conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 2>")),
        ("WCMC_IGEMM_PW", ("f", 8, 128, 128, 64, 64, 1, 0, 3, 1, 0, 0), ("conv_igemm", "conv_igemm_bf16x3_kernel<4, false, true, 0>")),
        ("WCMC_WGRAD_ROWS", ("w", 8, 44, 44, 100, 100, 5, 0, 1), ("conv_wgrad", "conv_wgrad_bf16x3_kernel<7, 1>")),
        ("WCMC_WGRAD_ROWS8", ("w", 8, 44, 44, 100, 100, 5, 0, 3), ("conv_wgrad_rows", "conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 2>")))
    table = {r[0]: r[1:] for r in BENCH_ROWS + EDGE_ROWS}
    for switch, args, switched in cases:
        monkeypatch.delenv(switch, raising=False)
        assert _ask(D, args)[1:] == table[args], switch                  # the defaults are the release library's plan
        monkeypatch.setenv(switch, "0")
        assert _ask(D, args)[1:] == switched and _ask(L, args)[1:] == table[args], switch
        monkeypatch.delenv(switch)
    assert "wcmc::conv_halo_bf16x3_kernel<7, 8, 16, 0, 2, 2>" == bench.rocprof_names(3)["conv_halo7"]


def test_benchmarked_launches_run_kernels_of_the_committed_profile(L):
    """Every kernel the plan names for a launch of the benchmarked step occurs in the rocprofv3 kernel statistics of that step."""
    import csv
    import bench
    with open(os.path.join(ROOT, "profiles", bench.PROFILE_ROUND + "_bench_kernel_stats.csv")) as f:
        names = [r["Name"] for r in csv.DictReader(f)]
    for args, _, kernel in BENCH_ROWS:
        assert any("wcmc::" + kernel + "(" in n for n in names), (args, kernel)


def test_refused_arguments_return_the_launch_error(L):
    ok = ("f", 8, 132, 132, 100, 100, 5, 0, 3, 1, 0, 0)
    assert _ask(L, ok)[0] == 0
    bad = {"terms = 0": ok[:8] + (0,) + ok[9:], "ks = 0": ok[:6] + (0,) + ok[7:], "empty output": ("f", 8, 4, 4, 100, 100, 5, 0, 3, 1, 0, 0),
           "N = 0": ("f", 0) + ok[2:], "a gate tensor with the fp32 output": ("f", 8, 132, 132, 100, 100, 5, 0, 3, 0, 1, 0),
           "fp16 launch without an instance": ("f", 8, 132, 132, 100, 39, 5, 0, 1, 0, 0, 1),
           "an operand of 2 GiB": ("f", 64, 132, 132, 512, 512, 5, 0, 3, 1, 0, 0),
           "wgrad: terms = 2": ("w", 8, 44, 44, 100, 100, 5, 0, 2), "wgrad: terms = 0": ("w", 8, 44, 44, 100, 100, 5, 0, 0),
           "wgrad: ks = 0": ("w", 8, 44, 44, 100, 100, 0, 0, 3), "wgrad: empty output": ("w", 8, 4, 4, 100, 100, 5, 0, 3)}
    for what, args in bad.items():
        rc = _ask(L, args)[0]
        msg = L.wcmc_last_error().decode()
        assert rc < 0 and "launch_plan" in msg, (what, rc, msg)
    for args in (ok, ("w", 8, 44, 44, 100, 100, 5, 0, 3)):          # a buffer too short for the kernel's name; none at all
        assert _ask(L, args, length=16)[0] < 0 and "too short" in L.wcmc_last_error().decode()
    assert L.wcmc_conv2d_launch_plan_bf16x3(8, 132, 132, 100, 100, 5, 0, 3, 1, 0, 0, 0, 0, 0, None, None, 0) < 0
    assert L.wcmc_conv2d_wgrad_launch_plan_bf16x3(8, 44, 44, 100, 100, 5, 0, 3, None, None, 0) < 0


# the exact-fp32 mode's layer labels (ops/conv_fp32.py): what the mirror returned for (cin, cout, ks) alone; every other shape of the grid is "conv_igemm"
FP32_LABELS = {
    "conv_pw": [(3, 128, 1), (36, 64, 1), (39, 64, 1), (64, 64, 1), (128, 128, 1)],
    "conv_halo3": [(64, 64, 3), (64, 128, 3), (64, 441, 3), (128, 64, 3), (128, 128, 3), (128, 441, 3), (441, 64, 3), (441, 128, 3), (441, 441, 3)],
    "conv_halo7": [(36, 100, 5), (36, 441, 5), (39, 100, 5), (39, 441, 5), (64, 100, 5), (64, 441, 5), (100, 100, 5), (100, 441, 5), (128, 100, 5),
                   (128, 441, 5), (441, 100, 5), (441, 441, 5)]}


def test_fp32_layer_labels_are_what_they_were():
    from wcmc_amd.ops.conv_fp32 import _layer_label
    want = {shape: label for label, shapes in FP32_LABELS.items() for shape in shapes}
    for shape in itertools.product((3, 36, 39, 64, 100, 128, 441), (3, 64, 100, 128, 441), (1, 3, 5)):
        assert _layer_label(*shape) == want.get(shape, "conv_igemm"), shape
