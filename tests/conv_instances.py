"""Every kernel instance the split-bf16 convolution dispatch of the release library can launch, and the shapes that hold each of
them to an fp64 convolution.  A plain module (no test functions), shared by tests/test_cpu_conv_instances.py -- which asks the
library's launch plan, without a GPU, that SWEEP yields exactly INSTANCES and that every row of CASES runs the instance it names --
and tests/test_gpu_conv_instances.py, which launches every row.

A row of CASES is (instance, kind, N, Cin, H, W, Cout, ks, pad, terms, options):
  kind     "f": ops.conv2d_x_raw, "h": ops.conv2d_out_f16_raw (the fp16 launch), "w": ops.conv2d_wgrad_x_raw
  terms    bf16 MFMAs per product the launch ASKS for; the instance's name says what it multiplies (planes())
  options  "f" / "h" rows: out=split | fp32 | fp32-in-wider-buffer, gate=none | tensor | mask, gate_act=relu (default) | leaky_relu,
           colsum, mask_out, bias, act=linear (default) | relu | leaky_relu
           "w" rows: bias (the launch sums dy itself) | colsum (the bias gradient is finished from the column sums the producer of
           dy left) | nobias
Each instance has a smallest row (N = 1 where the plan allows, less than one tile) and a ragged one (N >= 2; output height and
width no tile divides; a cout that is no multiple of 16 and at least two channel slabs with a short last one, where the instance
takes such shapes; pad > 0 where it takes a pad; 16- and 12-row tiles in one launch for the 16-row instances of conv_halo64).
What the plans refuse stays out: a gate tensor needs the split output and keeps a launch off conv_pw, conv_pw and conv_halo3
take whole blocks of channels only, the fp16 launch exists for seven-tile cout blocks and writes a dense fp32 view, un-gated."""
import itertools

# The grid asked of the plan: every combination below, through wcmc_conv2d_launch_plan_bf16x3 (FORWARD: terms, split output, gate
# tensor, fp16 launch) and wcmc_conv2d_wgrad_launch_plan_bf16x3 (terms 3 and 1); pad in {0, ks / 2, ks - 1}.  (1, 70, 75) has
# N * Ho >= 64 and Wo > 64 for the filter-row weight gradients; 448 channels take the 32-channel-slab plans.
SWEEP = {
    "sizes": ((1, 8, 8), (2, 16, 16), (2, 40, 37), (8, 44, 44), (1, 70, 75)),
    "channels": (3, 24, 34, 64, 100, 128, 256, 448),
    "ks": (1, 2, 3, 4, 5, 7),
    "forward": ((3, 1, 0, 0), (3, 0, 0, 0), (3, 1, 1, 0), (2, 1, 0, 0), (2, 0, 0, 0), (2, 1, 1, 0), (1, 1, 0, 0), (1, 0, 0, 0), (1, 1, 1, 0),
                (1, 0, 0, 1)),
    "wgrad_terms": (3, 1),
}

WIDE_OFFSET, WIDE_EXTRA = 4, 12      # out=fp32-in-wider-buffer: the slice starts at channel 4 of a buffer 12 channels wider than round_up(Cout, 4)


def dense_strides(cout, ho, wo):
    """(sn, sh, sw) of the fp32 NHWC view ops.nhwc_empty makes."""
    cp = (cout + 3) // 4 * 4
    return (ho * wo * cp, wo * cp, cp)


def wide_strides(cout, ho, wo):
    """(sn, sh, sw) of a Cout-channel slice of the wider buffer of an out=fp32-in-wider-buffer row."""
    cw = (cout + 3) // 4 * 4 + WIDE_EXTRA
    return (ho * wo * cw, wo * cw, cw)


def sweep_queries():
    """The arguments of every query of SWEEP, as rows of tests/test_cpu_launch_plan.py: ("f", N, H, W, Cin, Cout, ks, pad, terms,
    split, gate, f16) and ("w", N, H, W, Cin, Cout, ks, pad, terms)."""
    for (n, h, w), cin, cout, ks in itertools.product(SWEEP["sizes"], SWEEP["channels"], SWEEP["channels"], SWEEP["ks"]):
        for pad in sorted({0, ks // 2, ks - 1}):
            if h + 2 * pad - ks + 1 <= 0 or w + 2 * pad - ks + 1 <= 0:
                continue
            for v in SWEEP["forward"]:
                yield ("f", n, h, w, cin, cout, ks, pad) + v
            for terms in SWEEP["wgrad_terms"]:
                yield ("w", n, h, w, cin, cout, ks, pad, terms)


def options(row):
    """The options of a row as a dictionary: out, gate, gate_act, act (strings) and colsum, mask_out, bias, nobias (booleans)."""
    o = {"out": None, "gate": "none", "gate_act": "relu", "act": "linear", "colsum": False, "mask_out": False, "bias": False, "nobias": False}
    for t in row[10].split():
        if "=" in t:
            k, v = t.split("=")
            assert k in ("out", "gate", "gate_act", "act"), t
            o[k] = v
        else:
            assert t in ("colsum", "mask_out", "bias", "nobias"), t
            o[t] = True
    return o


def plan_query(row):
    """The launch-plan query of a row, in the argument order of tests/test_cpu_launch_plan.py: _ask (the output strides appended for
    an fp32 output: those the GPU test launches with)."""
    instance, kind, n, cin, h, w, cout, ks, pad, terms, _ = row
    if kind == "w":
        return ("w", n, h, w, cin, cout, ks, pad, terms)
    o = options(row)
    ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    split = o["out"] == "split"
    ys = (0, 0, 0) if split else wide_strides(cout, ho, wo) if o["out"] == "fp32-in-wider-buffer" else dense_strides(cout, ho, wo)
    return ("f", n, h, w, cin, cout, ks, pad, terms, int(split), int(o["gate"] == "tensor"), int(kind == "h"), ys)


def family(instance):
    """pw, halo3, halo64, halo, igemm or wgrad."""
    for f in ("conv_pw", "conv_halo3", "conv_halo64", "conv_halo", "conv_igemm", "conv_wgrad"):
        if instance.startswith(f + "_"):
            return f[5:]
    raise ValueError(instance)


def planes(instance):
    """(planes of x, planes of W, fp16) the named instance multiplies, read from its template arguments as tests/test_gpu_ops.py:
    _x_planes does: (2, 2, 0) three terms, (1, 2, 0) two (x rounded to bf16), (1, 1, 0) one (x and W rounded), (1, 1, 1) both fp16."""
    a = [s.strip() for s in instance[instance.index("<") + 1:-1].split(",")]
    if instance.startswith("conv_halo64_"):
        return int(a[5]), int(a[6]), int(a[7])
    if instance.startswith("conv_halo_"):
        return int(a[5]), 2, 0
    if instance.startswith("conv_halo3_"):
        return int(a[0]), 2, 0
    if instance.startswith("conv_wgrad_"):
        return int(a[-1]), int(a[-1]), 0
    return 2, 2, 0


# What SWEEP yields on the release library, sorted.  A new instance in the dispatch fails tests/test_cpu_conv_instances.py until it is
# listed here and given rows below.
INSTANCES = [
    'conv_halo3_bf16x3_kernel<1, 2, 2, 0>',
    'conv_halo3_bf16x3_kernel<1, 4, 2, 0>',
    'conv_halo3_bf16x3_kernel<2, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<1, 3, 3, 0, 0, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<1, 3, 3, 0, 80, 1, 2, 0>',
    'conv_halo64_bf16x3_kernel<1, 3, 3, 0, 80, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 1, 2, 0>',
    'conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<2, 3, 3, 0, 0, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<2, 3, 3, 0, 80, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<2, 3, 4, 0, 80, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<4, 3, 3, 0, 0, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<4, 3, 3, 0, 80, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<4, 3, 4, 0, 80, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<7, 2, 3, 0, 160, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 1, 0>',
    'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 1, 1>',
    'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 2, 0>',
    'conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 2, 2, 0>',
    'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 0>',
    'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 1>',
    'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>',
    'conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>',
    'conv_halo_bf16x3_kernel<1, 16, 16, 0, 3, 2>',
    'conv_halo_bf16x3_kernel<1, 8, 16, 0, 2, 2>',
    'conv_halo_bf16x3_kernel<2, 16, 16, 0, 3, 2>',
    'conv_halo_bf16x3_kernel<2, 8, 16, 0, 2, 2>',
    'conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 1>',
    'conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 2>',
    'conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 1>',
    'conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 2>',
    'conv_halo_bf16x3_kernel<7, 16, 16, 0, 3, 1>',
    'conv_halo_bf16x3_kernel<7, 16, 16, 0, 3, 2>',
    'conv_igemm_bf16x3_kernel<1, false, true, 0>',
    'conv_igemm_bf16x3_kernel<1, true, true, 0>',
    'conv_igemm_bf16x3_kernel<2, false, true, 0>',
    'conv_igemm_bf16x3_kernel<2, true, true, 0>',
    'conv_igemm_bf16x3_kernel<4, false, true, 0>',
    'conv_igemm_bf16x3_kernel<4, true, true, 0>',
    'conv_igemm_bf16x3_kernel<7, false, true, 0>',
    'conv_igemm_bf16x3_kernel<7, true, true, 0>',
    'conv_pw_bf16x3_kernel<4, 10, false, 0>',
    'conv_pw_bf16x3_kernel<4, 10, true, 0>',
    'conv_pw_bf16x3_kernel<4, 16, false, 0>',
    'conv_pw_bf16x3_kernel<4, 16, true, 0>',
    'conv_pw_bf16x3_kernel<8, 2, false, 0>',
    'conv_pw_bf16x3_kernel<8, 2, true, 0>',
    'conv_pw_bf16x3_kernel<8, 32, false, 0>',
    'conv_pw_bf16x3_kernel<8, 32, true, 0>',
    'conv_wgrad_bf16x3_kernel<4, 1>',
    'conv_wgrad_bf16x3_kernel<4, 2>',
    'conv_wgrad_bf16x3_kernel<7, 1>',
    'conv_wgrad_bf16x3_kernel<7, 2>',
    'conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>',
    'conv_wgrad_rows_bf16x3_kernel<1, 8, 8, 0, 1>',
    'conv_wgrad_rows_bf16x3_kernel<1, 8, 8, 0, 2>',
    'conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 1>',
    'conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 2>',
    'conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 1>',
    'conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 2>',
    'conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 1>',
    'conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 2>',
    'conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>',
]

# Two rows or more per instance: the smallest, then a ragged one (the module docstring).
CASES = [
    ('conv_halo3_bf16x3_kernel<1, 2, 2, 0>', 'f', 1, 64, 8, 8, 64, 3, 0, 2, 'out=split gate=mask colsum bias act=relu'),
    ('conv_halo3_bf16x3_kernel<1, 2, 2, 0>', 'f', 2, 64, 21, 26, 120, 3, 1, 2, 'out=fp32 gate=none bias act=linear'),
    ('conv_halo3_bf16x3_kernel<1, 4, 2, 0>', 'f', 1, 128, 8, 8, 64, 3, 0, 2, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_halo3_bf16x3_kernel<1, 4, 2, 0>', 'f', 2, 256, 21, 26, 120, 3, 1, 2, 'out=split gate=tensor colsum act=relu'),
    ('conv_halo3_bf16x3_kernel<2, 2, 2, 0>', 'f', 1, 64, 8, 8, 64, 3, 0, 3, 'out=split gate=none mask_out bias act=relu'),
    ('conv_halo3_bf16x3_kernel<2, 2, 2, 0>', 'f', 2, 128, 21, 26, 120, 3, 1, 3, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 3, 0, 0, 2, 2, 0>', 'f', 1, 256, 8, 8, 3, 5, 0, 3, 'out=split gate=mask colsum bias act=relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 3, 0, 0, 2, 2, 0>', 'f', 2, 288, 21, 26, 3, 5, 2, 3, 'out=fp32 gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<1, 3, 3, 0, 80, 1, 2, 0>', 'f', 1, 34, 8, 8, 3, 5, 0, 2, 'out=split gate=none mask_out bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 3, 0, 80, 1, 2, 0>', 'f', 2, 72, 21, 26, 3, 5, 2, 2, 'out=fp32 gate=none act=relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 3, 0, 80, 2, 2, 0>', 'f', 1, 34, 8, 8, 3, 5, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<1, 3, 3, 0, 80, 2, 2, 0>', 'f', 2, 104, 21, 26, 3, 5, 2, 3, 'out=split gate=tensor colsum bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 1, 2, 0>', 'f', 1, 34, 40, 37, 3, 5, 2, 2, 'out=fp32-in-wider-buffer gate=none bias act=relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 1, 2, 0>', 'f', 2, 72, 40, 37, 3, 5, 4, 2, 'out=split gate=tensor mask_out act=relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 2, 2, 0>', 'f', 1, 34, 40, 37, 3, 5, 2, 3, 'out=split gate=none colsum mask_out bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 2, 2, 0>', 'f', 2, 104, 40, 37, 3, 5, 4, 3, 'out=fp32 gate=none bias act=relu'),
    ('conv_halo64_bf16x3_kernel<2, 3, 3, 0, 0, 2, 2, 0>', 'f', 1, 256, 8, 8, 24, 5, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<2, 3, 3, 0, 0, 2, 2, 0>', 'f', 2, 288, 21, 26, 24, 5, 2, 3, 'out=split gate=tensor colsum mask_out act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<2, 3, 3, 0, 80, 2, 2, 0>', 'f', 1, 34, 8, 8, 24, 5, 0, 3, 'out=split gate=mask bias act=relu'),
    ('conv_halo64_bf16x3_kernel<2, 3, 3, 0, 80, 2, 2, 0>', 'f', 2, 104, 21, 26, 24, 5, 2, 3, 'out=fp32 gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<2, 3, 4, 0, 80, 2, 2, 0>', 'f', 1, 34, 40, 37, 24, 5, 2, 3, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<2, 3, 4, 0, 80, 2, 2, 0>', 'f', 2, 104, 40, 37, 24, 5, 4, 3, 'out=split gate=tensor act=relu'),
    ('conv_halo64_bf16x3_kernel<4, 3, 3, 0, 0, 2, 2, 0>', 'f', 1, 256, 8, 8, 34, 5, 0, 3, 'out=split gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<4, 3, 3, 0, 0, 2, 2, 0>', 'f', 2, 288, 21, 26, 120, 5, 2, 3, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<4, 3, 3, 0, 80, 2, 2, 0>', 'f', 1, 34, 8, 8, 34, 5, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=relu'),
    ('conv_halo64_bf16x3_kernel<4, 3, 3, 0, 80, 2, 2, 0>', 'f', 2, 104, 21, 26, 120, 5, 2, 3, 'out=split gate=tensor act=linear'),
    ('conv_halo64_bf16x3_kernel<4, 3, 4, 0, 80, 2, 2, 0>', 'f', 1, 34, 40, 37, 34, 5, 2, 3, 'out=split gate=mask colsum mask_out bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<4, 3, 4, 0, 80, 2, 2, 0>', 'f', 2, 104, 40, 37, 120, 5, 4, 3, 'out=fp32 gate=none bias act=relu'),
    ('conv_halo64_bf16x3_kernel<7, 2, 3, 0, 160, 2, 2, 0>', 'f', 1, 256, 8, 8, 100, 5, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 2, 3, 0, 160, 2, 2, 0>', 'f', 2, 288, 21, 26, 200, 5, 2, 3, 'out=split gate=tensor colsum mask_out act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 1, 0>', 'f', 1, 34, 8, 8, 100, 5, 0, 1, 'out=split gate=mask colsum bias act=relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 1, 0>', 'f', 2, 72, 21, 26, 200, 5, 2, 1, 'out=fp32 gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 1, 1>', 'h', 1, 34, 8, 8, 100, 5, 0, 1, 'out=fp32 gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 1, 1>', 'h', 2, 72, 21, 26, 200, 5, 2, 1, 'out=fp32 gate=none act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 2, 0>', 'f', 1, 34, 8, 8, 100, 5, 0, 2, 'out=split gate=none mask_out bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 1, 2, 0>', 'f', 2, 72, 21, 26, 200, 5, 2, 2, 'out=fp32 gate=none act=relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 2, 2, 0>', 'f', 1, 34, 8, 8, 100, 5, 0, 3, 'out=split gate=none colsum mask_out bias act=relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 3, 0, 80, 2, 2, 0>', 'f', 2, 104, 21, 26, 200, 5, 2, 3, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 0>', 'f', 1, 34, 40, 37, 100, 5, 2, 1, 'out=fp32-in-wider-buffer gate=none bias act=relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 0>', 'f', 2, 72, 40, 37, 200, 5, 4, 1, 'out=split gate=tensor colsum act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 1>', 'h', 1, 34, 40, 37, 100, 5, 2, 1, 'out=fp32 gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 1>', 'h', 2, 72, 40, 37, 200, 5, 4, 1, 'out=fp32 gate=none act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>', 'f', 1, 34, 40, 37, 100, 5, 2, 2, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>', 'f', 2, 72, 40, 37, 200, 5, 4, 2, 'out=split gate=tensor mask_out bias act=relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>', 'f', 1, 34, 40, 37, 100, 5, 2, 3, 'out=fp32-in-wider-buffer gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>', 'f', 2, 104, 40, 37, 200, 5, 4, 3, 'out=split gate=tensor colsum mask_out act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<1, 16, 16, 0, 3, 2>', 'f', 1, 34, 8, 8, 3, 3, 0, 3, 'out=split gate=mask colsum bias act=relu'),
    ('conv_halo_bf16x3_kernel<1, 16, 16, 0, 3, 2>', 'f', 2, 100, 15, 37, 3, 3, 1, 3, 'out=fp32 gate=none bias act=linear'),
    ('conv_halo_bf16x3_kernel<1, 8, 16, 0, 2, 2>', 'f', 1, 34, 16, 16, 3, 3, 1, 3, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<1, 8, 16, 0, 2, 2>', 'f', 2, 100, 21, 26, 3, 3, 1, 3, 'out=split gate=tensor colsum act=relu'),
    ('conv_halo_bf16x3_kernel<2, 16, 16, 0, 3, 2>', 'f', 1, 34, 8, 8, 24, 3, 0, 3, 'out=split gate=none mask_out bias act=relu'),
    ('conv_halo_bf16x3_kernel<2, 16, 16, 0, 3, 2>', 'f', 2, 100, 15, 37, 24, 3, 1, 3, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<2, 8, 16, 0, 2, 2>', 'f', 1, 34, 16, 16, 24, 3, 1, 3, 'out=fp32-in-wider-buffer gate=none bias act=relu'),
    ('conv_halo_bf16x3_kernel<2, 8, 16, 0, 2, 2>', 'f', 2, 100, 21, 26, 24, 3, 1, 3, 'out=split gate=tensor mask_out act=relu'),
    ('conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 1>', 'f', 1, 34, 8, 8, 34, 3, 0, 2, 'out=split gate=none colsum mask_out bias act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 1>', 'f', 2, 200, 15, 37, 120, 3, 1, 2, 'out=fp32 gate=none bias act=relu'),
    ('conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 2>', 'f', 1, 34, 8, 8, 34, 3, 0, 3, 'out=split gate=mask bias act=linear'),
    ('conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 2>', 'f', 2, 100, 15, 37, 120, 3, 1, 3, 'out=fp32 gate=none act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 1>', 'f', 1, 34, 16, 16, 34, 3, 1, 2, 'out=fp32-in-wider-buffer gate=none bias act=relu'),
    ('conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 1>', 'f', 2, 200, 21, 26, 120, 3, 1, 2, 'out=split gate=tensor colsum mask_out bias act=relu'),
    ('conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 2>', 'f', 1, 34, 16, 16, 34, 3, 1, 3, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 2>', 'f', 2, 100, 21, 26, 120, 3, 1, 3, 'out=split gate=tensor act=relu'),
    ('conv_halo_bf16x3_kernel<7, 16, 16, 0, 3, 1>', 'f', 1, 34, 8, 8, 100, 3, 0, 2, 'out=split gate=none bias act=linear'),
    ('conv_halo_bf16x3_kernel<7, 16, 16, 0, 3, 1>', 'f', 2, 200, 21, 26, 200, 3, 1, 2, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<7, 16, 16, 0, 3, 2>', 'f', 1, 34, 8, 8, 100, 3, 0, 3, 'out=split gate=mask colsum mask_out bias act=relu'),
    ('conv_halo_bf16x3_kernel<7, 16, 16, 0, 3, 2>', 'f', 2, 100, 21, 26, 200, 3, 1, 3, 'out=fp32 gate=none act=linear'),
    ('conv_igemm_bf16x3_kernel<1, false, true, 0>', 'f', 1, 3, 8, 8, 3, 1, 0, 3, 'out=split gate=mask colsum bias act=relu'),
    ('conv_igemm_bf16x3_kernel<1, false, true, 0>', 'f', 2, 34, 21, 26, 3, 1, 0, 3, 'out=fp32 gate=none bias act=linear'),
    ('conv_igemm_bf16x3_kernel<1, true, true, 0>', 'f', 1, 3, 8, 8, 3, 3, 1, 3, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_igemm_bf16x3_kernel<1, true, true, 0>', 'f', 2, 34, 21, 26, 3, 7, 3, 3, 'out=split gate=tensor colsum act=relu'),
    ('conv_igemm_bf16x3_kernel<2, false, true, 0>', 'f', 1, 3, 8, 8, 24, 1, 0, 3, 'out=split gate=none mask_out bias act=relu'),
    ('conv_igemm_bf16x3_kernel<2, false, true, 0>', 'f', 2, 34, 21, 26, 24, 1, 0, 3, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_igemm_bf16x3_kernel<2, true, true, 0>', 'f', 1, 3, 8, 8, 24, 3, 1, 3, 'out=fp32-in-wider-buffer gate=none bias act=relu'),
    ('conv_igemm_bf16x3_kernel<2, true, true, 0>', 'f', 2, 34, 21, 26, 24, 7, 3, 3, 'out=split gate=tensor mask_out act=relu'),
    ('conv_igemm_bf16x3_kernel<4, false, true, 0>', 'f', 1, 3, 8, 8, 34, 1, 0, 3, 'out=split gate=none colsum mask_out bias act=leaky_relu'),
    ('conv_igemm_bf16x3_kernel<4, false, true, 0>', 'f', 2, 34, 21, 26, 120, 1, 0, 3, 'out=fp32 gate=none bias act=relu'),
    ('conv_igemm_bf16x3_kernel<4, true, true, 0>', 'f', 1, 3, 8, 8, 34, 3, 1, 3, 'out=fp32-in-wider-buffer gate=none bias act=linear'),
    ('conv_igemm_bf16x3_kernel<4, true, true, 0>', 'f', 2, 34, 21, 26, 120, 7, 3, 3, 'out=split gate=tensor colsum mask_out act=leaky_relu'),
    ('conv_igemm_bf16x3_kernel<7, false, true, 0>', 'f', 1, 3, 8, 8, 100, 1, 0, 3, 'out=split gate=mask bias act=relu'),
    ('conv_igemm_bf16x3_kernel<7, false, true, 0>', 'f', 2, 34, 21, 26, 200, 1, 0, 3, 'out=fp32 gate=none bias act=linear'),
    ('conv_igemm_bf16x3_kernel<7, true, true, 0>', 'f', 1, 3, 8, 8, 100, 3, 1, 3, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_igemm_bf16x3_kernel<7, true, true, 0>', 'f', 2, 34, 21, 26, 200, 7, 3, 3, 'out=split gate=tensor act=relu'),
    ('conv_pw_bf16x3_kernel<4, 10, false, 0>', 'f', 1, 34, 8, 8, 64, 1, 0, 3, 'out=fp32 gate=none bias act=relu'),
    ('conv_pw_bf16x3_kernel<4, 10, false, 0>', 'f', 2, 34, 21, 26, 64, 1, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=linear'),
    ('conv_pw_bf16x3_kernel<4, 10, true, 0>', 'f', 1, 34, 8, 8, 64, 1, 0, 3, 'out=split gate=mask colsum bias act=leaky_relu'),
    ('conv_pw_bf16x3_kernel<4, 10, true, 0>', 'f', 2, 34, 21, 26, 64, 1, 0, 3, 'out=split gate=none mask_out act=relu'),
    ('conv_pw_bf16x3_kernel<4, 16, false, 0>', 'f', 1, 64, 8, 8, 64, 1, 0, 3, 'out=fp32 gate=none bias act=linear'),
    ('conv_pw_bf16x3_kernel<4, 16, false, 0>', 'f', 2, 64, 21, 26, 64, 1, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_pw_bf16x3_kernel<4, 16, true, 0>', 'f', 1, 64, 8, 8, 64, 1, 0, 3, 'out=split gate=none colsum mask_out bias act=relu'),
    ('conv_pw_bf16x3_kernel<4, 16, true, 0>', 'f', 2, 64, 21, 26, 64, 1, 0, 3, 'out=split gate=mask act=linear'),
    ('conv_pw_bf16x3_kernel<8, 2, false, 0>', 'f', 1, 3, 8, 8, 128, 1, 0, 3, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_pw_bf16x3_kernel<8, 2, false, 0>', 'f', 2, 3, 21, 26, 128, 1, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=relu'),
    ('conv_pw_bf16x3_kernel<8, 2, true, 0>', 'f', 1, 3, 8, 8, 128, 1, 0, 3, 'out=split gate=none bias act=linear'),
    ('conv_pw_bf16x3_kernel<8, 2, true, 0>', 'f', 2, 3, 21, 26, 128, 1, 0, 3, 'out=split gate=mask colsum mask_out act=leaky_relu'),
    ('conv_pw_bf16x3_kernel<8, 32, false, 0>', 'f', 1, 128, 8, 8, 128, 1, 0, 3, 'out=fp32 gate=none bias act=relu'),
    ('conv_pw_bf16x3_kernel<8, 32, false, 0>', 'f', 2, 128, 21, 26, 128, 1, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=linear'),
    ('conv_pw_bf16x3_kernel<8, 32, true, 0>', 'f', 1, 128, 8, 8, 128, 1, 0, 3, 'out=split gate=mask colsum bias act=leaky_relu'),
    ('conv_pw_bf16x3_kernel<8, 32, true, 0>', 'f', 2, 128, 21, 26, 128, 1, 0, 3, 'out=split gate=none mask_out act=relu'),
    ('conv_wgrad_bf16x3_kernel<4, 1>', 'w', 1, 3, 8, 8, 3, 1, 0, 1, 'bias'),
    ('conv_wgrad_bf16x3_kernel<4, 1>', 'w', 2, 34, 21, 26, 120, 3, 1, 1, 'colsum'),
    ('conv_wgrad_bf16x3_kernel<4, 2>', 'w', 1, 3, 8, 8, 3, 1, 0, 3, 'nobias'),
    ('conv_wgrad_bf16x3_kernel<4, 2>', 'w', 2, 34, 21, 26, 120, 3, 1, 3, 'bias'),
    ('conv_wgrad_bf16x3_kernel<7, 1>', 'w', 1, 3, 8, 8, 100, 1, 0, 1, 'colsum'),
    ('conv_wgrad_bf16x3_kernel<7, 1>', 'w', 2, 34, 21, 26, 100, 3, 1, 1, 'nobias'),
    ('conv_wgrad_bf16x3_kernel<7, 2>', 'w', 1, 3, 8, 8, 100, 1, 0, 3, 'bias'),
    ('conv_wgrad_bf16x3_kernel<7, 2>', 'w', 2, 34, 21, 26, 100, 3, 1, 3, 'colsum'),
    ('conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>', 'w', 2, 100, 40, 37, 100, 5, 0, 3, 'nobias'),
    ('conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>', 'w', 3, 100, 25, 30, 100, 5, 2, 3, 'bias'),
    ('conv_wgrad_rows_bf16x3_kernel<1, 8, 8, 0, 1>', 'w', 2, 128, 40, 37, 120, 1, 0, 1, 'colsum'),
    ('conv_wgrad_rows_bf16x3_kernel<1, 8, 8, 0, 1>', 'w', 3, 128, 25, 30, 120, 1, 0, 1, 'nobias'),
    ('conv_wgrad_rows_bf16x3_kernel<1, 8, 8, 0, 2>', 'w', 2, 128, 40, 37, 120, 1, 0, 3, 'bias'),
    ('conv_wgrad_rows_bf16x3_kernel<1, 8, 8, 0, 2>', 'w', 3, 128, 25, 30, 120, 1, 0, 3, 'colsum'),
    ('conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 1>', 'w', 2, 64, 40, 37, 64, 3, 0, 1, 'nobias'),
    ('conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 1>', 'w', 3, 64, 25, 30, 120, 3, 1, 1, 'bias'),
    ('conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 2>', 'w', 2, 64, 40, 37, 64, 3, 0, 3, 'colsum'),
    ('conv_wgrad_rows_bf16x3_kernel<3, 4, 4, 0, 2>', 'w', 3, 64, 25, 30, 120, 3, 1, 3, 'nobias'),
    ('conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 1>', 'w', 2, 128, 40, 37, 120, 3, 0, 1, 'bias'),
    ('conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 1>', 'w', 3, 128, 25, 30, 120, 3, 1, 1, 'colsum'),
    ('conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 2>', 'w', 2, 128, 40, 37, 120, 3, 0, 3, 'nobias'),
    ('conv_wgrad_rows_bf16x3_kernel<3, 8, 8, 0, 2>', 'w', 3, 128, 25, 30, 120, 3, 1, 3, 'bias'),
    ('conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 1>', 'w', 2, 34, 40, 37, 100, 5, 0, 1, 'colsum'),
    ('conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 1>', 'w', 3, 34, 25, 30, 100, 5, 2, 1, 'nobias'),
    ('conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 2>', 'w', 2, 34, 40, 37, 100, 5, 0, 3, 'bias'),
    ('conv_wgrad_rows_bf16x3_kernel<5, 7, 3, 0, 2>', 'w', 3, 34, 25, 30, 100, 5, 2, 3, 'colsum'),
    ('conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>', 'w', 2, 100, 40, 37, 100, 5, 0, 1, 'nobias'),
    ('conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>', 'w', 3, 100, 25, 30, 100, 5, 2, 1, 'bias'),
    # kernel sizes outside {1, 3, 5}: ks = 4 runs the halo kernels, ks = 2, 6 and 7 the streaming GEMM and the one-tap weight gradient
    ('conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 2>', 'f', 2, 100, 22, 27, 34, 4, 1, 3, 'out=split gate=mask colsum mask_out bias act=relu'),
    ('conv_halo_bf16x3_kernel<7, 16, 16, 0, 3, 2>', 'f', 1, 34, 9, 9, 100, 4, 0, 3, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<4, 8, 16, 0, 2, 2>', 'f', 2, 200, 22, 27, 120, 4, 2, 2, 'out=split gate=tensor bias act=linear'),
    ('conv_igemm_bf16x3_kernel<4, true, true, 0>', 'f', 2, 34, 21, 26, 39, 2, 1, 3, 'out=split gate=mask colsum bias act=relu'),
    ('conv_igemm_bf16x3_kernel<1, false, true, 0>', 'f', 1, 34, 8, 8, 7, 2, 0, 3, 'out=fp32 gate=none bias act=linear'),
    ('conv_igemm_bf16x3_kernel<2, false, true, 0>', 'f', 1, 24, 16, 16, 24, 7, 0, 3, 'out=split gate=none mask_out bias act=relu'),
    ('conv_igemm_bf16x3_kernel<7, true, true, 0>', 'f', 2, 34, 22, 27, 100, 6, 3, 3, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_wgrad_bf16x3_kernel<4, 2>', 'w', 2, 34, 21, 26, 39, 7, 3, 3, 'bias'),
    ('conv_wgrad_bf16x3_kernel<4, 1>', 'w', 2, 34, 21, 26, 39, 7, 3, 1, 'colsum'),
    ('conv_wgrad_bf16x3_kernel<7, 2>', 'w', 2, 34, 21, 26, 100, 4, 2, 3, 'colsum'),
    ('conv_wgrad_bf16x3_kernel<7, 1>', 'w', 2, 34, 21, 26, 100, 2, 0, 1, 'bias'),
    # output rows wider than one 64-pixel chunk (Wo = 66) for the 5x5 filter-row weight gradients; N * Ho = 64 is their threshold
    ('conv_wgrad_rows8_bf16x3_kernel<0, 1, 2>', 'w', 2, 100, 36, 70, 100, 5, 0, 3, 'colsum'),
    ('conv_wgrad_rows_bf16x3_kernel<5, 7, 7, 0, 1>', 'w', 2, 100, 36, 70, 100, 5, 0, 1, 'colsum'),
    # 28 x 28 outputs = (16 + 12)^2 through every 16-row instance of conv_halo64: tile rows of 16 then 12 AND, right of the tile columns
    # of 16, the strip of transposed 12-wide workgroups (launch_xhalo64: rows16, stripX), in one launch
    ('conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 2, 2, 0>', 'f', 2, 104, 32, 32, 3, 5, 0, 3, 'out=split gate=mask gate_act=leaky_relu colsum mask_out bias act=relu'),
    ('conv_halo64_bf16x3_kernel<1, 3, 4, 0, 80, 1, 2, 0>', 'f', 2, 72, 32, 32, 3, 5, 0, 2, 'out=fp32 gate=none bias act=leaky_relu'),
    ('conv_halo64_bf16x3_kernel<2, 3, 4, 0, 80, 2, 2, 0>', 'f', 2, 104, 32, 32, 24, 5, 0, 3, 'out=split gate=tensor gate_act=leaky_relu colsum bias act=linear'),
    ('conv_halo64_bf16x3_kernel<4, 3, 4, 0, 80, 2, 2, 0>', 'f', 2, 104, 32, 32, 39, 5, 0, 3, 'out=fp32-in-wider-buffer gate=none bias act=relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 2, 2, 0>', 'f', 2, 104, 32, 32, 100, 5, 0, 3, 'out=split gate=none colsum mask_out act=relu'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 2, 0>', 'f', 2, 72, 32, 32, 100, 5, 0, 2, 'out=split gate=mask colsum bias act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 0>', 'f', 2, 72, 32, 32, 100, 5, 0, 1, 'out=fp32-in-wider-buffer gate=none bias act=linear'),
    ('conv_halo64_bf16x3_kernel<7, 3, 4, 0, 80, 1, 1, 1>', 'h', 2, 72, 32, 32, 100, 5, 0, 1, 'out=fp32 gate=none bias act=linear'),
    # the 16x16 tiling of conv_halo with FOUR cout tiles or fewer and more than one tile row: x_plan_halo gives it to launches of 256 to
    # 511 workgroups only (fewer, or more, run 8x16 tiles), so these rows need 29 / 15 images of 3 x 3 ragged tiles
    ('conv_halo_bf16x3_kernel<1, 16, 16, 0, 3, 2>', 'f', 29, 100, 37, 33, 3, 3, 1, 3, 'out=split gate=tensor gate_act=leaky_relu mask_out bias act=relu'),
    ('conv_halo_bf16x3_kernel<2, 16, 16, 0, 3, 2>', 'f', 29, 100, 37, 33, 24, 3, 1, 3, 'out=fp32-in-wider-buffer gate=none bias act=leaky_relu'),
    ('conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 2>', 'f', 29, 100, 37, 33, 34, 3, 1, 3, 'out=split gate=mask colsum bias act=relu'),
    ('conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 1>', 'f', 15, 200, 37, 33, 120, 3, 1, 2, 'out=split gate=mask gate_act=leaky_relu colsum mask_out act=linear'),
    ('conv_halo_bf16x3_kernel<4, 16, 16, 0, 3, 2>', 'f', 15, 100, 37, 33, 120, 3, 1, 3, 'out=fp32 gate=none bias act=relu'),
]
