"""The bilinear-resize parity cases (csrc/gnet.hip: mi_gresize), one row per case: shape, dtype, convention, scale factor or size, the (ld, offset)
of every view, and the forward / backward kernel instance the row claims.  tests/test_host_gelem_routes.py checks the claims through the route query
(gk.gresize_route -> mi_gresize_route, which calls the planning function the launch calls) without a GPU; tests/test_gpu_gelem.py runs every row that
is not route-only against F.interpolate in float64.

The dispatch (gresize_plan): vec8 = bf16, C % 8 == 0, every ld % 8 == 0, 16-byte aligned views.  Forward: vec8 -> fwd8, otherwise fwd<T>.  Backward,
with mag = (1 / scale_h) * (1 / scale_w) (a scale of 0 counts as the output extent): vec8 and mag <= 256 -> bwd8; C >= 8 and mag >= 4 -> pix<T>;
mag >= 16 and at most 2^22 source elements -> wave<T>; otherwise the gather kernel bwd<T>.

bar: "fixed" - every source coordinate is exact in fp32 (power-of-two scale factors, identity, a scale of 0), or the row is one of the nine cases of
tests/test_gpu_gops.py::test_bilinear_resize_both_conventions, which keep that test's bars (1e-5 fp32, _close_bf16 bf16); "measured" - the source
coordinate carries fp32 rounding, the bar is twice the deviation of torch's own fp32 CPU evaluation from float64 on the same operands."""
import collections

import numpy as np

FWD, FWD8 = "gresize_fwd_kernel<%s>", "gresize_fwd8_kernel"
GATHER, WAVE, PIX, BWD8 = "gresize_bwd_kernel<%s>", "gresize_bwd_wave_kernel<%s>", "gresize_bwd_pix_kernel<%s>", "gresize_bwd8_kernel"
F, H = "float", "__bf16"

# x / out: the forward's views; dout / dx: the backward's; each (ld, channel offset) inside a wider sentinel-filled tensor (ld == C, offset 0: contiguous)
ResizeCase = collections.namedtuple("ResizeCase", "name B H W C f32 align sf size x out dout dx fwd bwd bar gpu zeros")


def _c(name, B, H, W, C, f32, align, sf, size, fwd, bwd, bar, x=None, out=None, dout=None, dx=None, gpu=True, zeros=False):
    same = (C, 0)
    x = x or same
    out = out or same
    return ResizeCase(name, B, H, W, C, f32, align, sf, size, x, out, dout or out, dx or x, fwd, bwd, bar, gpu, zeros)


def out_hw(c):
    """F.interpolate's output size: floor(in * scale_factor), or the size given."""
    if c.size is not None:
        return c.size
    return int(np.floor(c.H * c.sf)), int(np.floor(c.W * c.sf))


RESIZE_CASES = [
    # ---- the nine scale-factor cases of test_bilinear_resize_both_conventions, as they are (B = 2; fp32 C = 1, bf16 C = 32 contiguous)
    _c("x32_f32", 2, 11, 11, 1, True, False, 32, None, FWD % F, WAVE % F, "fixed"),                 # 69 candidate rows: the wave's lane loop runs twice
    _c("down4_f32", 2, 44, 44, 1, True, False, 0.25, None, FWD % F, GATHER % F, "fixed", zeros=True),   # three of four source elements get no contribution
    _c("x2_f32", 2, 11, 11, 1, True, False, 2, None, FWD % F, GATHER % F, "fixed"),
    _c("x8_f32", 2, 12, 9, 1, True, False, 8, None, FWD % F, WAVE % F, "fixed"),
    _c("x2_align_6x5", 2, 6, 5, 32, False, True, 2, None, FWD8, BWD8, "fixed"),
    _c("x2_align_3x3", 2, 3, 3, 32, False, True, 2, None, FWD8, BWD8, "fixed"),
    _c("x2_9x7", 2, 9, 7, 32, False, False, 2, None, FWD8, BWD8, "fixed"),
    _c("down2_bf16", 2, 16, 12, 32, False, False, 0.5, None, FWD8, BWD8, "fixed"),
    _c("x4_5x6", 2, 5, 6, 32, False, False, 4, None, FWD8, BWD8, "fixed"),                           # mag 16: 8 / 6 candidate columns (two full 4-wide trips / one and a half)
    # ---- size-given, non-dyadic ratios, both conventions: GALD's 23x40 <-> 45x80 <-> 90x160 chain scaled down, PraNet's tester resize
    _c("fit_12x20_23x40_align", 2, 12, 20, 16, False, True, None, (23, 40), FWD8, BWD8, "measured", x=(32, 8), out=(24, 8)),
    _c("fit_12x20_23x40", 2, 12, 20, 16, False, False, None, (23, 40), FWD8, BWD8, "measured", x=(32, 16), out=(16, 0)),
    _c("fit_23x40_45x77", 1, 23, 40, 8, False, False, None, (45, 77), FWD8, BWD8, "measured", x=(16, 8), out=(8, 0)),
    _c("fit_23x40_45x77_align", 1, 23, 40, 8, False, True, None, (45, 77), FWD8, BWD8, "measured"),
    _c("local_10x19_45x80_align", 2, 10, 19, 12, False, True, None, (45, 80), FWD % H, PIX % H, "measured", x=(20, 4), out=(12, 0), dout=(14, 2), dx=(12, 0)),
    _c("local_10x19_45x80", 2, 10, 19, 12, False, False, None, (45, 80), FWD % H, PIX % H, "measured"),
    _c("fit_12x20_23x40_f32", 2, 12, 20, 1, True, False, None, (23, 40), FWD % F, GATHER % F, "measured"),
    _c("fit_12x20_23x40_f32_align", 2, 12, 20, 3, True, True, None, (23, 40), FWD % F, GATHER % F, "measured", x=(5, 1), out=(4, 1)),
    _c("tester_88_300x211", 1, 88, 88, 1, True, False, None, (300, 211), FWD % F, GATHER % F, "measured"),
    # ---- downscales: the source elements between the taps receive nothing; their gradient is exactly 0
    _c("down4_bf16_gather", 2, 16, 12, 3, False, False, 0.25, None, FWD % H, GATHER % H, "fixed", x=(8, 5), out=(4, 1), zeros=True),
    _c("down4_bf16_vec8", 2, 16, 12, 8, False, False, 0.25, None, FWD8, BWD8, "fixed", x=(16, 8), out=(8, 0), zeros=True),
    # ---- degenerate sizes
    _c("one_to_5x7", 2, 1, 1, 1, True, False, None, (5, 7), FWD % F, WAVE % F, "measured"),
    _c("one_to_5x7_align", 2, 1, 1, 1, True, True, None, (5, 7), FWD % F, WAVE % F, "fixed"),       # align: scale 0, the `scale <= 0` full-range branch
    _c("one_to_5x7_align_vec8", 2, 1, 1, 8, False, True, None, (5, 7), FWD8, BWD8, "fixed"),        # ... in bwd8: all 5 x 7 destinations are candidates
    _c("one_to_5x7_align_pix", 2, 1, 1, 9, False, True, None, (5, 7), FWD % H, PIX % H, "fixed", x=(12, 1), out=(10, 1)),
    _c("one_to_3x3_align_gather", 2, 1, 1, 2, True, True, None, (3, 3), FWD % F, GATHER % F, "fixed"),
    _c("5x7_to_one_align", 2, 5, 7, 3, True, True, None, (1, 1), FWD % F, GATHER % F, "fixed", zeros=True),
    _c("identity_7x6", 2, 7, 6, 4, False, False, None, (7, 6), FWD % H, GATHER % H, "fixed", x=(6, 1), out=(4, 0)),
    _c("identity_7x6_align_f32", 1, 7, 6, 2, True, True, None, (7, 6), FWD % F, GATHER % F, "fixed"),
    _c("row_1x9_1x20", 2, 1, 9, 1, True, False, None, (1, 20), FWD % F, GATHER % F, "measured"),
    _c("column_9x1_20x1_align", 2, 9, 1, 2, False, True, None, (20, 1), FWD % H, GATHER % H, "measured", x=(4, 2), out=(2, 0)),
    # ---- fp32 class logits (GALD's unfused forward(): C = 19), mag just below and at 4 with C >= 8
    _c("logits19_7x10_28x37", 2, 7, 10, 19, True, False, None, (28, 37), FWD % F, PIX % F, "measured", dx=(21, 1)),
    _c("logits19_x2", 1, 6, 5, 19, True, False, 2, None, FWD % F, PIX % F, "fixed"),                # mag = 4
    _c("logits19_8x8_16x15", 1, 8, 8, 19, True, False, None, (16, 15), FWD % F, GATHER % F, "measured"),      # mag = 3.75
    _c("c9_x2", 1, 6, 5, 9, False, False, 2, None, FWD % H, PIX % H, "fixed"),                      # mag = 4
    _c("c9_8x8_16x15", 1, 8, 8, 9, False, False, None, (16, 15), FWD % H, GATHER % H, "measured"),  # mag = 3.75
    # ---- pix on misaligned bf16 views; more than 64 channels (the lane loop runs twice, the second trip partial)
    _c("pix_c16_odd_offset", 2, 5, 6, 16, False, False, 4, None, FWD % H, PIX % H, "fixed", x=(40, 3), out=(24, 5)),     # 8 / 6 candidate columns
    _c("fwd_c8_2byte_offset", 2, 5, 6, 8, False, True, None, (11, 13), FWD % H, PIX % H, "measured", x=(16, 1), out=(16, 7)),
    _c("pix_c72", 1, 3, 4, 72, False, False, None, (7, 9), FWD % H, PIX % H, "measured", x=(80, 1), out=(73, 1)),
    _c("pix_c72_f32", 1, 3, 4, 72, True, True, None, (13, 17), FWD % F, PIX % F, "measured"),
    # ---- mag <= 256 and > 256 on an eight-wide view: the second falls through to pix (17 / 25-34 candidate columns: partial 8-wide trips)
    _c("vec8_x16", 1, 2, 3, 8, False, False, 16, None, FWD8, BWD8, "fixed"),                         # mag = 256
    _c("vec8_x17", 1, 2, 3, 8, False, False, 17, None, FWD8, PIX % H, "measured"),                   # mag = 289
    # ---- bf16 with C < 8: mag just below and at 16; the x32 magnification in bf16
    _c("c3_x4_wave", 2, 4, 4, 3, False, False, 4, None, FWD % H, WAVE % H, "fixed", x=(4, 1), out=(6, 2)),               # mag = 16
    _c("c2_x4_wave_f32", 2, 4, 5, 2, True, False, 4, None, FWD % F, WAVE % F, "fixed", dout=(3, 1)),                   # mag = 16
    _c("c3_16x16_64x63", 1, 16, 16, 3, False, False, None, (64, 63), FWD % H, GATHER % H, "measured", x=(4, 1), out=(3, 0)),   # mag = 15.75
    _c("c1_16x16_64x63_f32", 1, 16, 16, 1, True, False, None, (64, 63), FWD % F, GATHER % F, "measured"),
    _c("c4_x32_wave", 1, 3, 2, 4, False, False, 32, None, FWD % H, WAVE % H, "fixed"),
    # ---- 2^22 and 2^22 + 1 source elements at mag >= 16: route only
    _c("nsrc_2p22", 1, 2048, 2048, 1, True, False, 4, None, FWD % F, WAVE % F, "fixed", gpu=False),
    _c("nsrc_2p22_plus_1", 1, 5, 838861, 1, True, False, 4, None, FWD % F, GATHER % F, "fixed", gpu=False),
]

INSTANCES = {FWD % F, FWD % H, FWD8, GATHER % F, GATHER % H, WAVE % F, WAVE % H, PIX % F, PIX % H, BWD8}


def scales(gk, c):
    return gk.resize_scales((c.H, c.W), out_hw(c), c.align, c.sf)


def mag(gk, c):
    """The backward's magnification, in fp32 as gresize_plan computes it."""
    sh, sw = scales(gk, c)
    Ho, Wo = out_hw(c)
    f = np.float32
    return float((f(1) / f(sh) if sh > 0 else f(Ho)) * (f(1) / f(sw) if sw > 0 else f(Wo)))


def query_routes(gk, c, base):
    """(forward, backward) GResizeRoute of a case whose four tensors all start at the aligned address `base`."""
    es = 4 if c.f32 else 2
    shape = (c.B, c.H, c.W, c.C)
    fwd = gk.gresize_route(base + es * c.x[1], c.x[0], base + es * c.out[1], c.out[0], c.f32, shape, out_hw(c), c.align, c.sf)
    bwd = gk.gresize_route(base + es * c.dx[1], c.dx[0], base + es * c.dout[1], c.dout[0], c.f32, shape, out_hw(c), c.align, c.sf, backward=True)
    return fwd, bwd


def touch_counts(n_in, n_out, scale, align):
    """For every source index, how many destination indices have a tap on it - the candidate count left after the trim of bwd8 / pix; the source map of
    csrc/gnet.hip: rs_src in fp32."""
    f = np.float32
    d = np.arange(n_out, dtype=np.float32)
    s = f(scale) * d if align else np.maximum(f(scale) * (d + f(0.5)) - f(0.5), f(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return [int(((i0 == i) | (i1 == i)).sum()) for i in range(n_in)]
