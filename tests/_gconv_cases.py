"""The general-conv routes (csrc/gconv.hip: gconv_plan, gwgrad_route, gwm_route) that the bench workloads launch, and one float64 parity case per route.

PRODUCTION is every gconv_kernel / gconv3_kernel / gwgrad* instance that one eager training step of GALD (6 x 720 x 1280) and one of PraNet
(16 x 352 x 352) launch, built as bench.py's aux_workload builds them (instance names as a profiler prints them): recorded with gk.ROUTES when this
table was written, and the same 59 names as the gconv* / gwgrad* kernels of the round-5 profiles (profiles/r05_gald_kernel_stats.csv,
profiles/r05_pranet_kernel_stats.csv): 37 gconv_kernel, 6 gconv3_kernel and 16 weight-gradient instances, no difference to explain.
tests/test_gpu_gconv_routes.py repeats the recording and requires what it records to stay inside this set.  The one-conv gwgrad / gwgrad3 instances are the large weight
gradients the tape runs directly on its side stream beside the data-gradient chain (host/pranet.py: q.direct); the rest go through the batched flush.

CASES: one conv per row, run on channel-slice views (x: (ld, offset) in a tensor of ld channels; y: the conv output / its gradient), at default
switches.  The four names are the routes its forward (fp32 out where `f32`), data gradient, one-conv weight gradient and batched weight gradient
take; tests/test_host_gconv_routes.py checks them through the route query without a GPU, tests/test_gpu_gconv_routes.py runs them against float64.
A tensor's base address is aligned as torch allocates (>= 256 bytes), so a view's alignment class follows from (ld, offset, channels) alone.
"""
from collections import namedtuple

# (kh, kw), (sh, sw), (ph, pw), (dh, dw)
G_1X1 = ((1, 1), (1, 1), (0, 0), (1, 1))
G_3X3 = ((3, 3), (1, 1), (1, 1), (1, 1))
G_3X3S2 = ((3, 3), (2, 2), (1, 1), (1, 1))
G_3X3D3 = ((3, 3), (1, 1), (3, 3), (3, 3))
G_1X7 = ((1, 7), (1, 1), (0, 3), (1, 1))
G_7X1 = ((7, 1), (1, 1), (3, 0), (1, 1))
G_5X5 = ((5, 5), (1, 1), (2, 2), (1, 1))

PRODUCTION = frozenset([
    'gconv3_kernel<32, 4, 4>',
    'gconv3_kernel<32, 8, 4>',
    'gconv3_kernel<64, 4, 4>',
    'gconv3_kernel<64, 4, 8>',
    'gconv3_kernel<64, 8, 4>',
    'gconv3_kernel<80, 4, 4>',
    'gconv_kernel<112, 32, 4, 4, false, false, 1>',
    'gconv_kernel<112, 32, 4, 8, false, false, 1>',
    'gconv_kernel<112, 32, 8, 4, false, false, 1>',
    'gconv_kernel<112, 32, 8, 8, false, false, 1>',
    'gconv_kernel<16, 32, 4, 8, false, false, 1>',
    'gconv_kernel<16, 32, 8, 4, false, false, 1>',
    'gconv_kernel<16, 64, 4, 8, false, false, 1>',
    'gconv_kernel<16, 64, 8, 1, false, false, 1>',
    'gconv_kernel<16, 64, 8, 8, false, false, 1>',
    'gconv_kernel<32, 32, 1, 8, false, false, 1>',
    'gconv_kernel<32, 32, 4, 4, false, false, 1>',
    'gconv_kernel<32, 32, 4, 8, false, false, 1>',
    'gconv_kernel<32, 32, 8, 1, true, false, 1>',
    'gconv_kernel<32, 32, 8, 4, false, false, 1>',
    'gconv_kernel<32, 32, 8, 8, false, false, 1>',
    'gconv_kernel<32, 64, 4, 4, false, false, 1>',
    'gconv_kernel<32, 64, 4, 8, false, false, 1>',
    'gconv_kernel<32, 64, 8, 1, true, false, 1>',
    'gconv_kernel<32, 64, 8, 8, false, false, 1>',
    'gconv_kernel<32, 64, 8, 8, false, false, 2>',
    'gconv_kernel<32, 64, 8, 8, false, true, 1>',
    'gconv_kernel<64, 32, 1, 8, false, false, 1>',
    'gconv_kernel<64, 32, 4, 4, false, false, 1>',
    'gconv_kernel<64, 32, 4, 8, false, false, 1>',
    'gconv_kernel<64, 32, 8, 4, false, false, 1>',
    'gconv_kernel<64, 32, 8, 8, false, false, 1>',
    'gconv_kernel<64, 64, 4, 4, false, false, 1>',
    'gconv_kernel<64, 64, 4, 4, false, true, 1>',
    'gconv_kernel<64, 64, 8, 4, false, false, 1>',
    'gconv_kernel<64, 64, 8, 8, false, false, 1>',
    'gconv_kernel<64, 64, 8, 8, false, false, 2>',
    'gconv_kernel<64, 64, 8, 8, false, true, 1>',
    'gconv_kernel<80, 32, 4, 4, false, false, 1>',
    'gconv_kernel<80, 32, 4, 8, false, false, 1>',
    'gconv_kernel<80, 32, 8, 4, false, false, 1>',
    'gconv_kernel<80, 64, 4, 4, false, false, 1>',
    'gconv_kernel<80, 64, 4, 8, false, false, 1>',
    'gwgrad3_kernel<1, 8>',
    'gwgrad3_kernel<4, 4>',
    'gwgrad3_kernel<4, 8>',
    'gwgrad3_kernel<8, 4>',
    'gwgrad3_kernel<8, 8>',
    'gwgrad3_multi_kernel<1, 8>',
    'gwgrad3_multi_kernel<4, 4>',
    'gwgrad3_multi_kernel<4, 8>',
    'gwgrad3_multi_kernel<8, 4>',
    'gwgrad3_multi_kernel<8, 8>',
    'gwgrad_kernel<4, 8>',
    'gwgrad_kernel<8, 4>',
    'gwgrad_kernel<8, 8>',
    'gwgrad_multi_kernel<1, 8>',
    'gwgrad_multi_kernel<4, 4>',
    'gwgrad_multi_kernel<8, 8>',
])

Case = namedtuple("Case", "name Cin Cout geom B H W x_view y_view f32 fwd dgrad wgrad wgrad_multi")

# Edges the table holds on purpose (tests/test_host_gconv_routes.py checks the route of every row):
#  - a partial last row tile: every M = B * Ho * Wo here is not a multiple of 128;
#  - a ragged last column tile: N = 68 on 80-wide tiles, 334 on 112, 14 on 16, 40 / 96 on 64 (a tail of 40 / 32);
#  - Ca = 14 / 20 / 40 / 68 (not a multiple of 32) and 96 (a multiple of 32, not of 64: half of the last 64-channel chunk is padding);
#  - every AVEC / OVEC class of PRODUCTION, through (ld, offset) views in sentinel-filled tensors;
#  - padding, dilation 3, 1x7 / 7x1 / 5x5 kernels, stride-2 data gradients (GEN) at widths 32 and 64;
#  - both sides of each launch-size threshold (the "...:" rows; wgs = row tiles x column tiles): MI_GCONV_BN32_WGS 256, the demotion of 80 / 112-wide
#    tiles below 384 workgroups, MI_GCONV_KC32_WGS 1536 and MI_GCONV_KS2_WGS 320;
#  - K splits S = 1 (the small maps) and S > 1 with a ragged last split, for the one-conv and the batched weight gradients.
CASES = [
    Case('small 1x1 96 out', 32, 96, G_1X1, 2, 12, 14, (32, 0), (96, 0), False,
         'gconv_kernel<32, 32, 8, 8, false, false, 1>', 'gconv_kernel<32, 64, 8, 8, false, false, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('small 3x3 14 in', 14, 32, G_3X3, 2, 12, 14, (18, 2), (32, 0), False,
         'gconv_kernel<32, 32, 4, 8, false, false, 1>', 'gconv_kernel<16, 32, 8, 4, false, false, 1>',
         'gwgrad_kernel<8, 4>', 'gwgrad3_multi_kernel<8, 4>'),
    Case('small 1x1 14 out odd view', 96, 14, G_1X1, 2, 12, 14, (96, 0), (15, 1), False,
         'gconv_kernel<16, 64, 8, 1, false, false, 1>', 'gconv_kernel<32, 32, 1, 8, false, false, 1>',
         'gwgrad_kernel<1, 8>', 'gwgrad_multi_kernel<1, 8>'),
    Case('small 1x1 4-byte views', 20, 68, G_1X1, 2, 12, 14, (22, 2), (70, 2), False,
         'gconv_kernel<32, 32, 4, 4, false, false, 1>', 'gconv_kernel<32, 64, 4, 4, false, false, 1>',
         'gwgrad_kernel<4, 4>', 'gwgrad_multi_kernel<4, 4>'),
    Case('small 1x1 68 out', 32, 68, G_1X1, 2, 12, 14, (32, 0), (70, 2), False,
         'gconv_kernel<32, 32, 8, 4, false, false, 1>', 'gconv_kernel<32, 64, 4, 8, false, false, 1>',
         'gwgrad_kernel<4, 8>', 'gwgrad_multi_kernel<4, 8>'),
    Case('small 3x3 stride 2', 32, 40, G_3X3S2, 2, 12, 14, (32, 0), (40, 0), False,
         'gconv_kernel<32, 32, 8, 8, false, false, 1>', 'gconv_kernel<32, 64, 8, 8, false, true, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('side map fp32 1x1', 64, 1, G_1X1, 2, 36, 45, (64, 0), (1, 0), True,
         'gconv_kernel<32, 32, 8, 1, true, false, 1>', 'gconv_kernel<32, 32, 1, 8, false, false, 1>',
         'gwgrad_kernel<1, 8>', 'gwgrad_multi_kernel<1, 8>'),
    Case('side map fp32 3x3', 64, 1, G_3X3, 2, 36, 45, (64, 0), (1, 0), True,
         'gconv_kernel<32, 64, 8, 1, true, false, 1>', 'gconv_kernel<32, 32, 1, 8, false, false, 1>',
         'gwgrad_kernel<1, 8>', 'gwgrad3_multi_kernel<1, 8>'),
    Case('3x3 14 in on 16-wide', 40, 16, G_3X3, 2, 181, 190, (40, 0), (16, 0), False,
         'gconv_kernel<16, 64, 8, 8, false, false, 1>', 'gconv_kernel<64, 32, 8, 8, false, false, 1>',
         'gwgrad3_kernel<8, 8>', 'gwgrad3_multi_kernel<8, 8>'),
    Case('3x3 40 -> 16 4-byte in', 40, 16, G_3X3, 2, 181, 190, (42, 2), (16, 0), False,
         'gconv_kernel<16, 64, 4, 8, false, false, 1>', 'gconv_kernel<64, 32, 8, 4, false, false, 1>',
         'gwgrad3_kernel<8, 4>', 'gwgrad3_multi_kernel<8, 4>'),
    Case('1x1 16 out 4-byte in', 20, 16, G_1X1, 2, 181, 190, (22, 2), (16, 0), False,
         'gconv_kernel<16, 32, 4, 8, false, false, 1>', 'gconv_kernel<32, 32, 8, 4, false, false, 1>',
         'gwgrad_kernel<8, 4>', 'gwgrad_multi_kernel<8, 4>'),
    Case('3x3 14 <-> 40', 14, 40, G_3X3, 2, 181, 190, (18, 2), (42, 2), False,
         'gconv_kernel<64, 32, 4, 4, false, false, 1>', 'gconv_kernel<16, 64, 4, 4, false, false, 1>',
         'gwgrad3_kernel<4, 4>', 'gwgrad3_multi_kernel<4, 4>'),
    Case('3x3 40 -> 14 4-byte', 40, 14, G_3X3, 2, 181, 190, (40, 0), (18, 2), False,
         'gconv_kernel<16, 64, 8, 4, false, false, 1>', 'gconv_kernel<64, 32, 4, 8, false, false, 1>',
         'gwgrad3_kernel<4, 8>', 'gwgrad3_multi_kernel<4, 8>'),
    Case('3x3 40 -> 14 odd view', 40, 14, G_3X3, 2, 181, 190, (40, 0), (15, 1), False,
         'gconv_kernel<16, 64, 8, 1, false, false, 1>', 'gconv_kernel<64, 32, 1, 8, false, false, 1>',
         'gwgrad3_kernel<1, 8>', 'gwgrad3_multi_kernel<1, 8>'),
    Case('3x3 32 -> 40', 32, 40, G_3X3, 2, 120, 140, (32, 0), (40, 0), False,
         'gconv_kernel<64, 32, 8, 8, false, false, 1>', 'gconv_kernel<32, 64, 8, 8, false, false, 2>',
         'gwgrad_kernel<8, 8>', 'gwgrad3_multi_kernel<8, 8>'),
    Case('1x1 40 -> 68 on 80-wide', 40, 68, G_1X1, 4, 121, 135, (42, 2), (70, 2), False,
         'gconv_kernel<80, 32, 4, 4, false, false, 1>', 'gconv_kernel<64, 64, 4, 4, false, false, 1>',
         'gwgrad_kernel<4, 4>', 'gwgrad_multi_kernel<4, 4>'),
    Case('1x1 40 -> 136', 40, 136, G_1X1, 2, 120, 140, (42, 2), (136, 0), False,
         'gconv_kernel<80, 32, 4, 8, false, false, 1>', 'gconv_kernel<64, 64, 8, 4, false, false, 1>',
         'gwgrad_kernel<8, 4>', 'gwgrad_multi_kernel<8, 4>'),
    Case('1x1 40 -> 96 112-wide', 40, 96, G_1X1, 4, 121, 135, (40, 0), (96, 0), False,
         'gconv_kernel<112, 32, 8, 8, false, false, 1>', 'gconv_kernel<64, 64, 8, 8, false, false, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('1x1 68 -> 96 4-byte', 68, 96, G_1X1, 4, 121, 135, (70, 2), (98, 2), False,
         'gconv_kernel<112, 32, 4, 4, false, false, 1>', 'gconv_kernel<80, 64, 4, 4, false, false, 1>',
         'gwgrad_kernel<4, 4>', 'gwgrad_multi_kernel<4, 4>'),
    Case('3x3 20 -> 104 window 32', 20, 104, G_3X3, 2, 181, 190, (22, 2), (104, 0), False,
         'gconv_kernel<112, 32, 4, 8, false, false, 1>', 'gconv3_kernel<32, 8, 4>',
         'gwgrad3_kernel<8, 4>', 'gwgrad3_multi_kernel<8, 4>'),
    Case('3x3 20 -> 104 4-byte', 20, 104, G_3X3, 2, 181, 190, (22, 2), (106, 2), False,
         'gconv_kernel<112, 32, 4, 4, false, false, 1>', 'gconv3_kernel<32, 4, 4>',
         'gwgrad3_kernel<4, 4>', 'gwgrad3_multi_kernel<4, 4>'),
    Case('1x1 96 -> 136', 96, 136, G_1X1, 4, 121, 135, (98, 2), (136, 0), False,
         'gconv_kernel<80, 64, 4, 8, false, false, 1>', 'gconv_kernel<112, 32, 8, 4, false, false, 1>',
         'gwgrad_kernel<8, 4>', 'gwgrad_multi_kernel<8, 4>'),
    Case('1x1 32 -> 68 80-wide', 32, 68, G_1X1, 4, 121, 135, (32, 0), (70, 2), False,
         'gconv_kernel<80, 32, 8, 4, false, false, 1>', 'gconv_kernel<32, 64, 4, 8, false, false, 1>',
         'gwgrad_kernel<4, 8>', 'gwgrad_multi_kernel<4, 8>'),
    Case('3x3 stride 2 68 -> 40', 68, 40, G_3X3S2, 4, 60, 70, (70, 2), (42, 2), False,
         'gconv_kernel<32, 64, 4, 4, false, false, 2>', 'gconv_kernel<64, 64, 4, 4, false, true, 1>',
         'gwgrad_kernel<4, 4>', 'gwgrad_multi_kernel<4, 4>'),
    Case('3x3 stride 2 40 -> 40', 40, 40, G_3X3S2, 2, 120, 140, (40, 0), (40, 0), False,
         'gconv_kernel<32, 64, 8, 8, false, false, 2>', 'gconv_kernel<64, 64, 8, 8, false, true, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('3x3 40 -> 40', 40, 40, G_3X3, 2, 120, 140, (40, 0), (40, 0), False,
         'gconv_kernel<64, 64, 8, 8, false, false, 2>', 'gconv_kernel<64, 64, 8, 8, false, false, 2>',
         'gwgrad_kernel<8, 8>', 'gwgrad3_multi_kernel<8, 8>'),
    Case('3x3 32 -> 32', 32, 32, G_3X3, 2, 181, 190, (32, 0), (32, 0), False,
         'gconv_kernel<32, 32, 8, 8, false, false, 1>', 'gconv_kernel<32, 32, 8, 8, false, false, 1>',
         'gwgrad3_kernel<8, 8>', 'gwgrad3_multi_kernel<8, 8>'),
    Case('3x3 128 -> 128 window 64', 128, 128, G_3X3, 2, 120, 140, (128, 0), (130, 2), False,
         'gconv3_kernel<64, 8, 4>', 'gconv3_kernel<64, 4, 8>',
         'gwgrad_kernel<4, 8>', 'gwgrad3_multi_kernel<4, 8>'),
    Case('3x3 128 -> 136 window 80', 128, 136, G_3X3, 2, 120, 140, (130, 2), (138, 2), False,
         'gconv3_kernel<80, 4, 4>', 'gconv3_kernel<64, 4, 4>',
         'gwgrad_kernel<4, 4>', 'gwgrad3_multi_kernel<4, 4>'),
    Case('3x3 dil 3 window', 104, 68, G_3X3D3, 2, 120, 140, (106, 2), (70, 2), False,
         'gconv3_kernel<80, 4, 4>', 'gconv_kernel<64, 64, 4, 4, false, false, 1>',
         'gwgrad_kernel<4, 4>', 'gwgrad3_multi_kernel<4, 4>'),
    Case('1x7 40 -> 334 on 112-wide', 40, 334, G_1X7, 2, 120, 140, (40, 0), (334, 0), False,
         'gconv_kernel<112, 32, 8, 4, false, false, 1>', 'gconv_kernel<64, 64, 4, 8, false, false, 2>',
         'gwgrad_kernel<4, 8>', 'gwgrad_multi_kernel<4, 8>'),
    Case('7x1 68 -> 68', 68, 68, G_7X1, 2, 120, 140, (70, 2), (68, 0), False,
         'gconv_kernel<64, 64, 4, 4, false, false, 1>', 'gconv_kernel<64, 64, 4, 4, false, false, 1>',
         'gwgrad_kernel<4, 4>', 'gwgrad_multi_kernel<4, 4>'),
    Case('5x5 pad 2', 32, 48, G_5X5, 2, 60, 70, (32, 0), (48, 0), False,
         'gconv_kernel<32, 32, 8, 8, false, false, 1>', 'gconv_kernel<32, 64, 8, 8, false, false, 2>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('BN32_WGS: 127 x 2 < 256', 64, 96, G_1X1, 2, 85, 95, (64, 0), (96, 0), False,
         'gconv_kernel<32, 32, 8, 8, false, false, 1>', 'gconv_kernel<32, 64, 8, 8, false, false, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('BN32_WGS: 128 x 2 = 256', 64, 96, G_1X1, 2, 84, 97, (64, 0), (96, 0), False,
         'gconv_kernel<64, 32, 8, 8, false, false, 1>', 'gconv_kernel<32, 64, 8, 8, false, false, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('demotion: 383 80-wide < 384', 32, 68, G_1X1, 2, 145, 169, (32, 0), (68, 0), False,
         'gconv_kernel<64, 32, 8, 4, false, false, 1>', 'gconv_kernel<32, 64, 4, 8, false, false, 1>',
         'gwgrad_kernel<4, 8>', 'gwgrad_multi_kernel<4, 8>'),
    Case('demotion: 384 80-wide', 32, 68, G_1X1, 2, 146, 168, (32, 0), (68, 0), False,
         'gconv_kernel<80, 32, 8, 4, false, false, 1>', 'gconv_kernel<32, 64, 4, 8, false, false, 1>',
         'gwgrad_kernel<4, 8>', 'gwgrad_multi_kernel<4, 8>'),
    Case('KC32_WGS: 383 x 4 < 1536', 128, 256, G_1X1, 2, 145, 169, (128, 0), (256, 0), False,
         'gconv_kernel<64, 64, 8, 8, false, false, 1>', 'gconv_kernel<64, 64, 8, 8, false, false, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('KC32_WGS: 384 x 4 = 1536', 128, 256, G_1X1, 2, 146, 168, (128, 0), (256, 0), False,
         'gconv_kernel<64, 32, 8, 8, false, false, 1>', 'gconv_kernel<64, 64, 8, 8, false, false, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad_multi_kernel<8, 8>'),
    Case('KS2_WGS: 160 x 2 = 320', 64, 128, G_3X3, 2, 93, 110, (64, 0), (128, 0), False,
         'gconv_kernel<64, 64, 8, 8, false, false, 2>', 'gconv_kernel<32, 64, 8, 8, false, false, 2>',
         'gwgrad_kernel<8, 8>', 'gwgrad3_multi_kernel<8, 8>'),
    Case('KS2_WGS: 161 x 2 > 320', 64, 128, G_3X3, 2, 94, 109, (64, 0), (128, 0), False,
         'gconv_kernel<64, 64, 8, 8, false, false, 1>', 'gconv_kernel<32, 64, 8, 8, false, false, 1>',
         'gwgrad_kernel<8, 8>', 'gwgrad3_multi_kernel<8, 8>'),
]


def geom8(case):
    """(kh, kw, sh, sw, ph, pw, dh, dw) as gk takes it"""
    k, s, p, d = case.geom
    return k + s + p + d


def out_hw(case):
    kh, kw, sh, sw, ph, pw, dh, dw = geom8(case)
    return (case.H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (case.W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def query_routes(gk, case, base=1 << 30):
    """The four routes of a case through the host query, for views into tensors whose storage starts at `base` (a torch-like, 256-byte aligned address)."""
    geom = geom8(case)
    Ho, Wo = out_hw(case)
    (ldi, offi), (ldo, offo) = case.x_view, case.y_view
    xa, ya = base + 2 * offi, base + 2 * offo
    dy_shape, x_shape = (case.B, Ho, Wo, case.Cout), (case.B, case.H, case.W, case.Cin)
    return {
        "fwd": gk.gconv_route(xa, ldi, base + (4 if case.f32 else 2) * offo, ldo, x_shape, case.Cout, geom, out_f32=case.f32),
        "dgrad": gk.gconv_route(ya, ldo, xa, ldi, dy_shape, case.Cin, geom, gk.GATHER_DGRAD, (case.H, case.W)),
        "wgrad": gk.gconv_wgrad_route(ya, ldo, xa, ldi, dy_shape, x_shape, geom),
        "wgrad_multi": gk.gconv_wgrad_route(ya, ldo, xa, ldi, dy_shape, x_shape, geom, multi=True),
    }
