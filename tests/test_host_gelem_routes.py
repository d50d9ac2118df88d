"""The resize parity cases reach the kernel instances they claim - checked on the host through mi_gresize_route, which calls the planning function the
launch calls (csrc/gnet.hip: gresize_plan).  No GPU: a retuned threshold or a removed case fails here and names the instance or threshold side that lost
its float64 case (tests/test_gpu_gelem.py)."""
import re

import pytest

import __graft_entry__ as entry
from _gelem_cases import BWD8, FWD8, INSTANCES, RESIZE_CASES, mag, out_hw, query_routes, scales, touch_counts

BASE = 1 << 30          # a fake tensor address, aligned as torch allocations are


@pytest.fixture(scope="module")
def gk():
    entry.build()
    from rnd_semantic_segmentation_amd import gk as g
    return g


@pytest.fixture(scope="module")
def routes(gk):
    return [query_routes(gk, c, BASE) for c in RESIZE_CASES]


def test_every_case_lands_on_the_instance_it_names(gk, routes):
    wrong = ["%s %s: %s, not %s" % (c.name, k, r.name, want) for c, rs in zip(RESIZE_CASES, routes) for k, r, want in (("fwd", rs[0], c.fwd), ("bwd", rs[1], c.bwd))
             if r.name != want]
    assert not wrong, "\n".join(wrong)
    assert len({c.name for c in RESIZE_CASES}) == len(RESIZE_CASES)
    # any 256-byte aligned base gives the same routes: the alignment classes come from (ld, offset, channels) alone
    assert [query_routes(gk, c, BASE + 256 * 3) for c in RESIZE_CASES] == routes


def test_the_gpu_cases_cover_all_ten_instances(routes):
    covered = {r.name for c, rs in zip(RESIZE_CASES, routes) if c.gpu for r in rs}
    assert len(INSTANCES) == 10
    assert covered == INSTANCES, "resize instances without a float64 parity case: %s" % sorted(INSTANCES - covered)


def test_both_sides_of_every_threshold_are_held(gk, routes):
    rows = [(c, rs[1], mag(gk, c)) for c, rs in zip(RESIZE_CASES, routes)]
    K = type(routes[0][1])
    vec8 = lambda c: not c.f32 and c.C % 8 == 0 and all(v[0] % 8 == 0 and v[1] % 8 == 0 for v in (c.dx, c.dout))
    # mag 4 with C >= 8 (no eight-wide view): pix from 4 up, the gather kernel just below
    for f32 in (True, False):
        assert any(c.gpu and c.f32 == f32 and c.C >= 8 and not vec8(c) and m == 4.0 and r.kernel == K.BWD_PIX for c, r, m in rows), f32
        assert any(c.gpu and c.f32 == f32 and c.C >= 8 and not vec8(c) and 3.5 <= m < 4.0 and r.kernel == K.BWD_GATHER for c, r, m in rows), f32
    # mag 16 with C < 8: wave from 16 up, the gather kernel just below
    for f32 in (True, False):
        assert any(c.gpu and c.f32 == f32 and c.C < 8 and m == 16.0 and r.kernel == K.BWD_WAVE for c, r, m in rows), f32
        assert any(c.gpu and c.f32 == f32 and c.C < 8 and 15.5 <= m < 16.0 and r.kernel == K.BWD_GATHER for c, r, m in rows), f32
    # mag 256 on an eight-wide view: bwd8 up to 256, above it the fall-through to pix
    assert any(c.gpu and vec8(c) and m == 256.0 and r.kernel == K.BWD8 for c, r, m in rows)
    assert any(c.gpu and vec8(c) and 256.0 < m < 300.0 and r.kernel == K.BWD_PIX for c, r, m in rows)
    # 2^22 source elements at mag >= 16 (route only)
    n = lambda c: c.B * c.H * c.W * c.C
    assert any(n(c) == 1 << 22 and m >= 16.0 and r.kernel == K.BWD_WAVE for c, r, m in rows)
    assert any(n(c) == (1 << 22) + 1 and m >= 16.0 and r.kernel == K.BWD_GATHER for c, r, m in rows)
    # a scale of 0 (align_corners from or to one pixel) in every backward kernel
    zero = {r.kernel for c, r, m in rows if c.gpu and 0.0 in scales(gk, c)}
    assert zero == {K.BWD_GATHER, K.BWD_WAVE, K.BWD_PIX, K.BWD8}, zero


def test_the_cases_hold_the_edges_they_claim(gk, routes):
    K = type(routes[0][1])
    gpu = [(c, rs) for c, rs in zip(RESIZE_CASES, routes) if c.gpu]
    # candidate columns after the trim: bwd8 walks them four, pix eight at a time - full trips, partial trips, and more than one trip
    def counts(kernel):
        out = set()
        for c, rs in gpu:
            if rs[1].kernel == kernel and 0.0 not in scales(gk, c):
                out |= set(touch_counts(c.W, out_hw(c)[1], scales(gk, c)[1], c.align))
        return out
    for kernel, trip in ((K.BWD8, 4), (K.BWD_PIX, 8)):
        cs = counts(kernel)
        assert any(n % trip == 0 and n > 0 for n in cs) and any(n % trip and n < trip for n in cs) and any(n % trip and n > trip for n in cs), (kernel, sorted(cs))
    # the wave kernel's lane loop: more than 64 candidate rows (x32), in both dtypes
    for f32 in (True, False):
        assert any(rs[1].kernel == K.BWD_WAVE and c.f32 == f32 and c.sf == 32 and c.H >= 3 for c, rs in gpu), f32
    # pix with more than 64 channels, not a multiple of 64
    assert any(rs[1].kernel == K.BWD_PIX and c.C > 64 and c.C % 64 for c, rs in gpu)
    # scalar bf16 forward on a C % 8 == 0 view that is only 2-byte aligned; pix on an odd channel offset
    assert any(rs[0].name == "gresize_fwd_kernel<__bf16>" and c.C % 8 == 0 and c.x[1] % 2 for c, rs in gpu)
    assert any(rs[1].kernel == K.BWD_PIX and not c.f32 and c.C >= 8 and c.dx[1] % 2 for c, rs in gpu)
    # size-given non-dyadic ratios under both conventions, backward included; downscales; degenerate extents
    assert {c.align for c, _ in gpu if c.size is not None and c.bar == "measured" and c.H > 1 and c.W > 1} == {True, False}
    assert any(c.zeros and c.sf == 0.25 and rs[1].kernel == k for k in (K.BWD_GATHER, K.BWD8) for c, rs in gpu)
    assert any((c.H, c.W) == (1, 1) and not c.align for c, _ in gpu) and any(out_hw(c) == (1, 1) and c.align for c, _ in gpu)
    assert any(out_hw(c) == (c.H, c.W) for c, _ in gpu) and any(c.H == 1 and c.W > 1 for c, _ in gpu) and any(c.W == 1 and c.H > 1 for c, _ in gpu)
    # views: some case writes each of out / dx into a channel slice of a wider tensor, and reads x / dout from one
    for v in ("x", "out", "dout", "dx"):
        assert any(getattr(c, v)[0] > c.C for c, _ in gpu), v
    # grids: the forward and the gather kernel are capped at 16 384 workgroups, the others launch one item per thread / wave
    assert all(rs[0].grid <= 16384 and rs[0].grid >= 1 for _, rs in zip(RESIZE_CASES, routes))
    big = dict((c.name, rs) for c, rs in zip(RESIZE_CASES, routes))["nsrc_2p22_plus_1"]
    assert big[1].grid == 16384 and big[0].grid == 16384


def test_the_existing_scale_factor_cases_are_kept():
    from test_gpu_gops import test_bilinear_resize_both_conventions as t
    old = next(m for m in t.pytestmark if m.name == "parametrize").args[1]
    mine = {(c.H, c.W, c.sf, c.align, c.f32) for c in RESIZE_CASES if c.sf is not None and c.B == 2 and c.C in (1, 32) and c.x == (c.C, 0)}
    assert set(old) <= mine, set(old) - mine


def test_descriptor_length_and_kernel_codes_match_the_header(gk):
    from rnd_semantic_segmentation_amd import _lib
    hdr = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define MI_GRESIZE_ROUTE_LEN (\d+)", hdr).group(1)) == gk.GRESIZE_ROUTE_LEN
    R = gk.GResizeRoute
    for name, code in (("FWD", R.FWD), ("FWD8", R.FWD8), ("BWD_GATHER", R.BWD_GATHER), ("BWD_WAVE", R.BWD_WAVE), ("BWD_PIX", R.BWD_PIX), ("BWD8", R.BWD8)):
        assert int(re.search(r"#define MI_GRESIZE_%s (\d+)" % name, hdr).group(1)) == code, name
    assert R(R.BWD_PIX, 1, 7).name == "gresize_bwd_pix_kernel<float>" and R(R.BWD8, 0, 7).name == BWD8 and R(R.FWD8, 0, 1).name == FWD8


def test_the_query_validates_like_the_launch(gk):
    from rnd_semantic_segmentation_amd._lib import MiError
    with pytest.raises(MiError, match="bad shape"):
        gk.gresize_route(BASE, 4, BASE, 8, False, (1, 2, 2, 8), (4, 4), False)          # ldx < C
