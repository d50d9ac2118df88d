"""The general-conv parity cases reach the routes they claim - checked on the host through mi_gconv_route / mi_gconv_wgrad_route, which call the
planning functions the launches call (csrc/gconv.hip: gconv_plan, gwgrad_route, gwm_route).  No GPU: a retuned threshold or a removed case fails here
and names the routes that lost their float64 case (tests/test_gpu_gconv_routes.py)."""
import re

import pytest

import __graft_entry__ as entry
from _gconv_cases import CASES, PRODUCTION, out_hw, query_routes
from test_gpu_gops import CONV_CASE_ROUTES, CONV_CASES

KINDS = ("fwd", "dgrad", "wgrad", "wgrad_multi")
BASE = 1 << 30          # a fake tensor address, aligned as torch allocations are


@pytest.fixture(scope="module")
def gk():
    entry.build()
    from rnd_semantic_segmentation_amd import gk as g
    return g


@pytest.fixture(scope="module")
def routes(gk):
    return [query_routes(gk, c, BASE) for c in CASES]


def test_every_case_lands_on_the_route_it_names(gk, routes):
    wrong = ["%s %s: %s, not %s" % (c.name, k, r[k].name, getattr(c, k)) for c, r in zip(CASES, routes) for k in KINDS if r[k].name != getattr(c, k)]
    assert not wrong, "\n".join(wrong)
    # any 256-byte aligned base gives the same routes: the alignment classes come from (ld, offset, channels) alone
    assert [query_routes(gk, c, BASE + 256 * 3) for c in CASES] == routes


def test_the_cases_cover_every_production_route(routes):
    covered = {r.name for rs in routes for r in rs.values()}
    missing = sorted(PRODUCTION - covered)
    assert not missing, "production routes without a float64 parity case: %s" % missing
    assert len([n for n in PRODUCTION if n.startswith("gconv_kernel")]) == 37 and len([n for n in PRODUCTION if n.startswith("gconv3")]) == 6
    assert len([n for n in PRODUCTION if n.startswith("gwgrad")]) == 16


def test_the_cases_hold_the_edges_they_claim(routes):
    fwd = [(c, r["fwd"]) for c, r in zip(CASES, routes)]
    assert all((c.B * out_hw(c)[0] * out_hw(c)[1]) % 128 for c in CASES), "every case has a partial last row tile"
    # ragged last column tiles: (N, BN) pairs of the forward or the data gradient
    pairs = {(c.Cout, r["fwd"].bn) for c, r in zip(CASES, routes)} | {(c.Cin, r["dgrad"].bn) for c, r in zip(CASES, routes)}
    for n, bn in ((68, 80), (334, 112), (14, 16)):
        assert (n, bn) in pairs, (n, bn)
    assert any(bn == 64 and n % 64 for n, bn in pairs), "a tail at width 64"
    # K padding: Ca not a multiple of 32, and a multiple of 32 but not of 64
    assert any(c.Cin % 32 for c in CASES) and any(c.Cin % 64 == 32 for c in CASES)
    # stride-2 data gradients on the general source map at widths 32 and 64
    assert {r["dgrad"].bn for r in (rs for rs in routes) if r["dgrad"].gen} >= {32, 64}
    # launch-size thresholds, both sides (MI_GCONV_BN32_WGS 256, demotion below 384, MI_GCONV_KC32_WGS 1536, MI_GCONV_KS2_WGS 320)
    def wgs64(c, r):
        return r.grid_x * -(-c.Cout // 64)
    assert any(r.bn == 32 and c.Cout > 32 and 250 <= wgs64(c, r) < 256 for c, r in fwd)
    assert any(r.bn == 64 and wgs64(c, r) == 256 for c, r in fwd)
    assert any(r.bn == 64 and c.Cout == 68 and r.grid_x == 383 for c, r in fwd) and any(r.bn == 80 and r.grid_x * r.grid_y == 384 for c, r in fwd)
    assert any(r.kc == 64 and r.grid_x * r.grid_y == 1532 for c, r in fwd) and any(r.kc == 32 and r.grid_x * r.grid_y == 1536 for c, r in fwd)
    assert any(r.ks == 2 and r.grid_x * r.grid_y == 320 for c, r in fwd) and any(r.ks == 1 and r.bn == 64 and r.kc == 64 and r.grid_x * r.grid_y == 322 for c, r in fwd)
    # K splits: S = 1 and S > 1 with a ragged last split, one-conv and batched
    for kind in ("wgrad", "wgrad_multi"):
        ss = [(r[kind].S, (c.B * out_hw(c)[0] * out_hw(c)[1]) % r[kind].rows) for c, r in zip(CASES, routes)]
        assert any(s == 1 for s, _ in ss) and any(s > 1 and tail for s, tail in ss), kind


def test_descriptor_lengths_match_the_header(gk):
    from rnd_semantic_segmentation_amd import _lib
    hdr = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define MI_GROUTE_LEN (\d+)", hdr).group(1)) == gk.GROUTE_LEN
    assert int(re.search(r"#define MI_GWROUTE_LEN (\d+)", hdr).group(1)) == gk.GWROUTE_LEN


def test_conv_cases_take_the_routes_their_comments_name(gk):
    """tests/test_gpu_gops.py: CONV_CASE_ROUTES (the rows whose comments name a tile) through the route query."""
    for i, (fwd, dgrad) in CONV_CASE_ROUTES.items():
        Cin, Cout, k, s, p, d, B, H, W, (ldi, offi), (ldo, offo) = CONV_CASES[i]
        geom = k + s + p + d
        Ho, Wo = gk.conv_out_hw(H, W, *geom)
        assert gk.gconv_route(BASE + 2 * offi, ldi, BASE + 2 * offo, ldo, (B, H, W, Cin), Cout, geom).name == fwd, CONV_CASES[i]
        assert gk.gconv_route(BASE + 2 * offo, ldo, BASE + 2 * offi, ldi, (B, Ho, Wo, Cout), Cin, geom, gk.GATHER_DGRAD, (H, W)).name == dgrad, CONV_CASES[i]
