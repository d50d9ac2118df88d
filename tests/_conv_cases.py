"""The implicit-GEMM conv routes (csrc/igemm_nt.hip: mi_conv_plan; csrc/igemm_tn.hip: wgrad_plan) that the DeepLab bench workloads launch, and one float64
parity case per route.

PRODUCTION is every plan name (kernels.ConvPlan.name / WgradPlan.name: one per instantiation the product library can launch, a generic epilogue named by the
flags it reads) that one eager training step launches in each of bench.py's workloads on this family, built as bench.py builds them at B = 8, 769 x 769:
the default (frozen BatchNorm), deeplab_bn (trainable BatchNorm: the `stats` epilogues) and fada (4 source + 4 target crops: the discriminator's LeakyReLU
epilogues g325 / g384, its fp32 head g17, the one-call q3 / tn.m1 weight gradients).  Recorded on an MI355X with kernels.ROUTES through
tests/_conv_record.py when this table was written: 29 names in the default step, 6 more in deeplab_bn, 6 more in fada.  tests/test_gpu_conv_routes.py repeats the
recording and requires what it records to stay inside this set.

CASES: one conv per row at default switches, at the smallest shape that reaches the route (tests/test_host_conv_routes.py checks every row through the plan
queries without a GPU; tests/test_gpu_conv_routes.py runs them against float64).  No row is spare: each is the only case of a PRODUCTION name or of an edge
that the host test asserts, so deleting one fails there.
"""
from collections import namedtuple

PRODUCTION = frozenset([
    'nt.mt4.gen.g0',
    'nt.mt4.gen.g1',
    'nt.mt4.gen.g128',
    'nt.mt4.gen.g69',
    'nt.mt4.gen.stats',
    'nt.mt4.unit.e69',
    'nt.mt4.unit.g384',
    'nt.mt5.unit.e128',
    'nt.mt5.unit.e130.stg',
    'nt.mt5.unit.e69',
    'nt.mt5.unit.e71.stg',
    'nt.mt5.unit.g0',
    'nt.mt5.unit.g1',
    'nt.mt5.unit.g17',
    'nt.mt5.unit.g325',
    'nt.mt5.unit.g384',
    'nt.mt5.unit.pref.g2',
    'nt.mt5.unit.stats',
    'nt.mt6.unit.e130.stg',
    'nt.mt6.unit.e71.stg',
    'nt.mt6.unit.g0',
    'nt.mt6.unit.stats',
    'pp.mtg10.e0.k0',
    'pp.mtg10.e0.k1',
    'pp.mtg10.e1.k0',
    'pp.mtg10.e128.k0',
    'pp.mtg10.e128.k1',
    'pp.mtg10.e48.k0',
    'pp.mtg10.e69.k0',
    'pp.mtg10.e69.k1',
    'pp.mtg10.stats.k0',
    'pp.mtg10.stats.k1',
    'q3',
    'q3.deferred',
    's4',
    's4.deferred',
    'tn.m0.deferred',
    'tn.m1',
    'tn.m1.deferred',
    'tn256.m2.aspp',
    'tn256.m2.deferred',
])

# epilogue flags (include/mi355seg.h MI_EPI_*)
SCALE_BIAS, RESIDUAL, RELU, MASK, OUT_F32, ZSPLIT, WRITE_MASK, BITMASK, LEAKY, STATS = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
ZGW = 20            # columns per fp32 tap plane of the ZSPLIT store (kernels.ASPP_ZGW)

# A forward ("fwd": a = x [B,H,W,Cin], N = Cout) or data-gradient ("dgrad": a = dy [B,Ho,Wo,Cout], N = Cin) launch of the conv Cin -> Cout, k x k, stride,
# dilation (pad = dilation for 3x3, 0 for 1x1) on a B x H x W input, with the epilogue `flags`; `plan` is the route it must take.
ConvCase = namedtuple("ConvCase", "plan mode B H W Cin Cout ksize stride dil flags")
# The weight gradient of the same kind of conv (out_map 1: the ASPP scatter, Cout = 704 im2col columns of which 36 * ncls are live), one-call and deferred.
WgradCase = namedtuple("WgradCase", "plan plan_deferred B H W Cin Cout ksize stride dil out_map")

# Shapes (B = 2 throughout, so that 3x3 windows of a later tile cross an image boundary):
#   13 x 15           M = 390: one round of MT 4, four row tiles, the last one partial
#   33 x 35 stride 2  M = 612 (forward) / 2310 (data gradient): the general gather, 128-row tiles only
#   61 x 60, 65 x 65  M = 7320 / 8450: MT 5 at N = 1040 (one round) / 1024 (one round), 2048 (two rounds: 53 x 16 tiles on 512 slots)
#   69 x 67, 73 x 71  M = 9246 / 10366: MT 6 at N = 1040 / 1024 (one round), 2048 (two rounds)
#   99 x 105          M = 20790 >= 20480: the ping-pong loop by rule, MTG 10 (65 tiles, a 310-row last tile); 101 x 102, M = 20604: MTG 8
# N = 144 / 1040 / 264 / 272 / 280: a ragged last column tile (128-wide for nt, 256-wide for pp).  The staged epilogue (.stg) moves the sign bits through LDS
# when N % 128 == 0 (what the network launches) and bytewise otherwise: one case of each per flag set.
CONV_CASES = [
    ConvCase('nt.mt4.unit.e69', "fwd", 2, 13, 15, 64, 144, 3, 1, 2, 69),
    ConvCase('nt.mt4.unit.g384', "dgrad", 2, 13, 15, 144, 64, 3, 1, 1, BITMASK | LEAKY),
    ConvCase('nt.mt4.gen.g1', "fwd", 2, 33, 35, 64, 136, 1, 2, 1, SCALE_BIAS),
    ConvCase('nt.mt4.gen.g69', "fwd", 2, 33, 35, 64, 144, 3, 2, 1, 69),
    ConvCase('nt.mt4.gen.stats', "fwd", 2, 33, 35, 64, 136, 1, 2, 1, STATS),
    ConvCase('nt.mt4.gen.g0', "dgrad", 2, 33, 35, 136, 64, 3, 2, 1, 0),
    ConvCase('nt.mt4.gen.g128', "dgrad", 2, 33, 35, 144, 64, 1, 2, 1, BITMASK),
    ConvCase('nt.mt5.unit.e128', "dgrad", 2, 61, 60, 1040, 64, 1, 1, 1, 128),
    ConvCase('nt.mt5.unit.e130.stg', "dgrad", 2, 61, 60, 1040, 64, 1, 1, 1, 130),
    ConvCase('nt.mt5.unit.e69', "fwd", 2, 65, 65, 64, 2048, 1, 1, 1, 69),
    ConvCase('nt.mt5.unit.e71.stg', "fwd", 2, 65, 65, 64, 1024, 1, 1, 1, 71),
    ConvCase('nt.mt5.unit.g0', "dgrad", 2, 65, 65, 1024, 64, 3, 1, 4, 0),
    ConvCase('nt.mt5.unit.g1', "fwd", 2, 61, 60, 64, 1040, 1, 1, 1, SCALE_BIAS),
    ConvCase('nt.mt5.unit.g17', "fwd", 2, 65, 65, 64, 1024, 1, 1, 1, SCALE_BIAS | OUT_F32),
    ConvCase('nt.mt5.unit.g325', "fwd", 2, 61, 60, 64, 1040, 3, 1, 1, SCALE_BIAS | RELU | WRITE_MASK | LEAKY),
    ConvCase('nt.mt5.unit.g384', "dgrad", 2, 65, 65, 1024, 64, 1, 1, 1, BITMASK | LEAKY),
    ConvCase('nt.mt5.unit.pref.g2', "dgrad", 2, 65, 65, 1024, 64, 1, 1, 1, RESIDUAL),
    ConvCase('nt.mt5.unit.stats', "fwd", 2, 61, 60, 64, 1040, 1, 1, 1, STATS),
    ConvCase('nt.mt6.unit.e130.stg', "dgrad", 2, 73, 71, 1024, 64, 1, 1, 1, 130),
    ConvCase('nt.mt6.unit.e71.stg', "fwd", 2, 69, 67, 64, 1040, 1, 1, 1, 71),
    ConvCase('nt.mt6.unit.g0', "dgrad", 2, 73, 71, 2048, 64, 1, 1, 1, 0),
    ConvCase('nt.mt6.unit.stats', "fwd", 2, 73, 71, 64, 1024, 3, 1, 2, STATS),
    ConvCase('pp.mtg10.e0.k0', "dgrad", 2, 99, 105, 264, 512, 1, 1, 1, 0),
    ConvCase('pp.mtg10.e0.k1', "dgrad", 2, 99, 105, 264, 64, 3, 1, 2, 0),
    ConvCase('pp.mtg10.e1.k0', "fwd", 2, 99, 105, 512, 264, 1, 1, 1, SCALE_BIAS),
    ConvCase('pp.mtg10.e128.k0', "dgrad", 2, 99, 105, 272, 512, 1, 1, 1, 128),
    ConvCase('pp.mtg10.e128.k1', "dgrad", 2, 99, 105, 272, 64, 3, 1, 4, 128),
    ConvCase('pp.mtg10.e48.k0', "fwd", 2, 99, 105, 512, 280, 1, 1, 1, OUT_F32 | ZSPLIT),
    ConvCase('pp.mtg10.e69.k0', "fwd", 2, 99, 105, 512, 272, 1, 1, 1, 69),
    ConvCase('pp.mtg10.e69.k1', "fwd", 2, 99, 105, 64, 272, 3, 1, 1, 69),
    ConvCase('pp.mtg10.stats.k0', "fwd", 2, 99, 105, 512, 264, 1, 1, 1, STATS),
    ConvCase('pp.mtg10.stats.k1', "fwd", 2, 99, 105, 64, 264, 3, 1, 2, STATS),
    ConvCase('pp.mtg8.e69.k1', "fwd", 2, 101, 102, 64, 272, 3, 1, 1, 69),            # not launched by the step: the other tile height of the rule
    ConvCase('nt.mt4.unit.g8', "dgrad", 2, 13, 15, 144, 64, 3, 1, 1, MASK),           # not launched by the step: the bf16 ReLU-mask operand of the C-ABI
]

# q3 by rule: 3x3 stride 1 with O * I >= 256 * 256 and at least 8 slabs of 64 padded pixels per split; one-call plans the split for 512 workgroup slots, deferred
# for 448, so S differs.  d in {1, 2, 4}; 320 -> 256: a ragged i tile (128-wide); 256 -> 264: a ragged o tile (64-wide); 270 x 18, d = 1: WP = W + 2 d = 20,
# the narrowest map the kernel takes - 270 x 17 (WP = 19) falls to tn.m1, with S = 14 and a ragged last split.
# s4 / tn256 / tn: S = 1 on the 9 x 11 / 13 x 15 maps, S > 1 with a last split shorter than the others on the larger ones.
# 72 -> 136 on 2 x 33 x 35 (tn.m1 and s4, the kernels that share the fragment block and, with every other one, the workgroup decode and the slab store of
# csrc/wgrad_common.h): two o tiles of which the second holds 8 channels, a 72-channel i tile, S > 1 with a short last split whose last K step has 6 pixels.
WGRAD_CASES = [
    WgradCase('q3', 'q3.deferred', 2, 67, 70, 256, 256, 3, 1, 1, 0),
    WgradCase('q3', 'q3.deferred', 2, 66, 69, 256, 256, 3, 1, 2, 0),
    WgradCase('q3', 'q3.deferred', 2, 64, 67, 256, 256, 3, 1, 4, 0),
    WgradCase('q3', 'q3.deferred', 2, 32, 35, 512, 512, 3, 1, 1, 0),
    WgradCase('q3', 'q3.deferred', 2, 54, 57, 320, 256, 3, 1, 2, 0),
    WgradCase('q3', 'q3.deferred', 2, 60, 63, 256, 264, 3, 1, 1, 0),
    WgradCase('q3', 'q3.deferred', 2, 270, 18, 256, 256, 3, 1, 1, 0),
    WgradCase('tn.m1', 'tn.m1.deferred', 2, 270, 17, 256, 256, 3, 1, 1, 0),
    WgradCase('tn.m1', 'tn.m1.deferred', 2, 13, 15, 64, 64, 3, 1, 1, 0),
    WgradCase('tn.m1', 'tn.m1.deferred', 2, 45, 47, 64, 72, 3, 1, 1, 0),
    WgradCase('tn.m1', 'tn.m1.deferred', 2, 33, 35, 72, 136, 3, 1, 1, 0),
    WgradCase('tn.m0', 'tn.m0.deferred', 2, 33, 35, 64, 128, 3, 2, 1, 0),
    WgradCase('tn.m0', 'tn.m0.deferred', 2, 65, 67, 64, 136, 1, 2, 1, 0),
    WgradCase('s4', 's4.deferred', 2, 9, 11, 64, 256, 1, 1, 1, 0),
    WgradCase('s4', 's4.deferred', 2, 45, 47, 64, 256, 1, 1, 1, 0),
    WgradCase('s4', 's4.deferred', 2, 33, 35, 72, 136, 1, 1, 1, 0),
    WgradCase('tn256.m2', 'tn256.m2.deferred', 2, 9, 11, 512, 1024, 1, 1, 1, 0),
    WgradCase('tn256.m2', 'tn256.m2.deferred', 2, 45, 47, 512, 1024, 1, 1, 1, 0),
    WgradCase('tn256.m2.aspp', 'tn256.m2.aspp.deferred', 2, 33, 35, 768, 704, 1, 1, 1, 1),
]
ASPP_NCLS = 19      # classes of the out_map 1 case: 36 * 19 = 684 live columns of the 704

CASES = CONV_CASES + WGRAD_CASES


def case_id(c):
    if isinstance(c, ConvCase):
        return "%s %s %dx%dx%d %d->%d k%d s%d d%d" % (c.plan, c.mode, c.B, c.H, c.W, c.Cin, c.Cout, c.ksize, c.stride, c.dil)
    return "wgrad %s %dx%dx%d %d->%d k%d s%d d%d" % (c.plan, c.B, c.H, c.W, c.Cin, c.Cout, c.ksize, c.stride, c.dil)


def pad_of(c):
    return c.dil if c.ksize == 3 else 0


def out_hw(c):
    p = pad_of(c)
    return (c.H + 2 * p - c.dil * (c.ksize - 1) - 1) // c.stride + 1, (c.W + 2 * p - c.dil * (c.ksize - 1) - 1) // c.stride + 1


def launch_geometry(c):
    """(a_shape, N, out_hw) of a ConvCase's launch as kernels.conv_gemm takes them"""
    Ho, Wo = out_hw(c)
    if c.mode == "fwd":
        return (c.B, c.H, c.W, c.Cin), c.Cout, (Ho, Wo)
    return (c.B, Ho, Wo, c.Cout), c.Cin, (c.H, c.W)


def query_plan(K, c):
    """The plan of a ConvCase, or the (one-call, deferred) plans of a WgradCase, through the host queries"""
    if isinstance(c, ConvCase):
        a_shape, N, ohw = launch_geometry(c)
        return K.conv_gemm_plan(a_shape, N, ohw, c.ksize, c.stride, pad_of(c), c.dil, c.flags)
    Ho, Wo = out_hw(c)
    dy, x = (c.B, Ho, Wo, c.Cout), (c.B, c.H, c.W, c.Cin)
    return tuple(K.conv_wgrad_plan(dy, x, c.ksize, c.stride, pad_of(c), c.dil, c.out_map, deferred) for deferred in (False, True))
