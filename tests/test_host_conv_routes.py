"""The implicit-GEMM conv parity cases reach the routes they claim - checked on the host through mi_conv_gemm_plan / mi_conv_wgrad_plan, which call the planning
functions the launches call (csrc/igemm_nt.hip: mi_conv_plan; csrc/igemm_tn.hip: wgrad_plan).  No GPU: a retuned threshold or a removed case fails here and names
the routes that lost their float64 case (tests/test_gpu_conv_routes.py)."""
import re

import pytest

import __graft_entry__ as entry
from _conv_cases import CASES, CONV_CASES, PRODUCTION, WGRAD_CASES, ConvCase, case_id, launch_geometry, out_hw, pad_of, query_plan


@pytest.fixture(scope="module")
def K():
    entry.build()
    from rnd_semantic_segmentation_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def conv_plans(K):
    return [query_plan(K, c) for c in CONV_CASES]


@pytest.fixture(scope="module")
def wgrad_plans(K):
    return [query_plan(K, c) for c in WGRAD_CASES]


def test_every_case_lands_on_the_plan_it_names(conv_plans, wgrad_plans):
    wrong = ["%s: %s" % (case_id(c), p.name) for c, p in zip(CONV_CASES, conv_plans) if p.name != c.plan]
    wrong += ["%s: %s / %s, not %s / %s" % (case_id(c), one.name, de.name, c.plan, c.plan_deferred)
              for c, (one, de) in zip(WGRAD_CASES, wgrad_plans) if (one.name, de.name) != (c.plan, c.plan_deferred)]
    assert not wrong, "cases that no longer reach the plan they name:\n" + "\n".join(wrong)


def test_the_cases_cover_every_production_route(conv_plans, wgrad_plans):
    covered = {p.name for p in conv_plans} | {p.name for pair in wgrad_plans for p in pair}
    missing = sorted(PRODUCTION - covered)
    assert not missing, "production routes without a float64 parity case: %s" % missing


def test_the_cases_hold_the_edges_they_claim(conv_plans, wgrad_plans):
    conv = list(zip(CONV_CASES, conv_plans))
    M = {c: launch_geometry(c)[2][0] * launch_geometry(c)[2][1] * c.B for c in CONV_CASES}
    N = {c: launch_geometry(c)[1] for c in CONV_CASES}
    for c, p in conv:
        rows = 32 * p.mt
        assert p.m_tiles == -(-M[c] // rows) and p.m_tiles > 1 and M[c] % rows, "a partial last row tile, after full ones: %s" % case_id(c)
        assert p.n_tiles == -(-N[c] // (256 if p.kernel else 128)), case_id(c)
    # ragged last column tiles, nt at every tile height and pp
    for mt in (4, 5, 6):
        assert any(p.kernel == 0 and p.mt == mt and N[c] % 128 for c, p in conv), "nt MT %d with N %% 128 != 0" % mt
    assert any(p.kernel == 1 and N[c] % 256 for c, p in conv), "pp with N % 256 != 0"
    # the staged epilogue with the sign bits through LDS (N % 128 == 0) and bytewise
    for epi in (71, 130):
        assert {N[c] % 128 == 0 for c, p in conv if p.staged and p.epi == epi} == {True, False}, "nt.*.e%d.stg needs a case with N %% 128 == 0 and one without" % epi
    # two rounds for an MT 5 and an MT 6 case (fewer rounds is why the model picks the taller tile), and the one-round forms
    for mt in (5, 6):
        assert {min(p.rounds, 2) for c, p in conv if p.kernel == 0 and p.mt == mt} == {1, 2}, "nt.mt%d needs a one-round and a two-round case" % mt
    # pp by rule: both tile heights, 3x3 with B >= 2 (windows cross an image boundary inside a tile), both K orders
    for mtg in (8, 10):
        assert any(p.kernel == 1 and p.mt == mtg for c, p in conv), "no case reaches pp.mtg%d by rule" % mtg
    for korder in (0, 1):
        assert any(p.kernel == 1 and p.korder == korder and (c.ksize == 3 and c.B >= 2 or not korder) for c, p in conv), "no pp case with K order %d (.k%d)" % (korder, korder)
    # the general gather at stride 2: 1x1 and 3x3, forward and data gradient
    assert all(c.stride == 2 and p.mt == 4 for c, p in conv if not p.unit), "nt.*.gen cases are the stride-2 launches, on 128-row tiles"
    for ksize, mode in ((1, "fwd"), (3, "fwd"), (1, "dgrad"), (3, "dgrad")):
        assert any(not p.unit and (c.ksize, c.mode) == (ksize, mode) for c, p in conv), "no nt.mt4.gen case with a %dx%d %s" % (ksize, ksize, mode)
    # the prefetched-residual form and every compile-time epilogue of the product build
    assert any(p.pref for c, p in conv), "no nt.*.pref case"
    for epi in (69, 71, 128, 130, 512, -1):
        assert any(p.kernel == 0 and p.epi == epi for c, p in conv), "no nt case with the compile-time epilogue %d" % epi
    for epi in (0, 1, 48, 69, 128, 512):
        assert any(p.kernel == 1 and p.epi == epi for c, p in conv), "no pp case with the compile-time epilogue %d" % epi
    assert any(c.flags & 8 for c, p in conv), "no case with the bf16 ReLU-mask operand (MI_EPI_MASK)"
    # weight gradients
    wg = list(zip(WGRAD_CASES, wgrad_plans))
    q3 = [(c, one, de) for c, (one, de) in wg if one.kernel == 3]
    assert all(de.kernel == 3 and de.deferred and not one.deferred for c, one, de in q3), "a q3 case whose deferred form leaves q3"
    assert {c.dil for c, one, de in q3 if one.S != de.S} >= {1, 2, 4}, "q3 at d in {1, 2, 4} where the one-call and deferred splits differ"
    assert all(one.steps >= 8 and de.steps >= 8 for c, one, de in q3), "q3 by rule, not forced"
    for dil in (1, 2, 4):
        assert any(c.dil == dil and c.Cin == c.Cout == 256 and one.steps == 8 for c, one, de in q3), \
            "q3 256 -> 256 (layer1 / layer2 / layer3: d = 1 / 2 / 4) at d = %d on the rule's threshold (8 slabs per split: the smallest map)" % dil
    assert any(c.Cout % 64 for c, one, de in q3) and any(c.Cin % 128 for c, one, de in q3), "q3 with a ragged o tile and a ragged i tile"
    assert any(c.W + 2 * c.dil == 20 for c, one, de in q3), "q3 at WP = 20"
    assert any(c.W + 2 * c.dil == 19 and c.Cin * c.Cout >= 256 * 256 and one.kernel == 0 for c, (one, de) in wg), "WP = 19 stays on the per-tap kernel"
    assert any(c.Cin == c.Cout == 512 for c, one, de in q3), "q3 on the 512 -> 512 convs of layer4 (eight o tiles x four i tiles: the fewest splits)"
    for kern, name in ((0, "tn"), (1, "tn256"), (4, "s4")):
        for form in (0, 1):
            ss = [(pl[form].S, (c.B * out_hw(c)[0] * out_hw(c)[1]) % (pl[form].steps * pl[form].step_rows)) for c, pl in wg if pl[form].kernel == kern and not c.out_map]
            assert any(s == 1 for s, _ in ss) and any(s > 1 and tail for s, tail in ss), "%s: S = 1, and S > 1 with a ragged last split" % name
    # tn: the unit-stride form (tn.m1) and the general gather (tn.m0, stride 2) for 1x1 and 3x3; S = 1 and S > 1 for each form
    for mode, ksizes in ((1, (3,)), (0, (1, 3))):
        for ksize in ksizes:
            assert any(one.kernel == 0 and one.mode == mode and c.ksize == ksize for c, (one, de) in wg), "no tn.m%d case with a %dx%d conv" % (mode, ksize, ksize)
        ss = {min(one.S, 2) for c, (one, de) in wg if one.kernel == 0 and one.mode == mode}
        assert ss == {1, 2}, "tn.m%d: S = 1 and S > 1" % mode
    assert any(one.kernel == 0 and one.mode == 1 and one.S > 1 and c.Cout % 128 for c, (one, de) in wg), "no tn.m1 case with several splits and a ragged o tile"
    # the shared decode / slab store (csrc/wgrad_common.h) on the 128 x 128 tile: a partial LAST o tile behind a full one and a partial i tile in one launch,
    # with several splits, a short last split and a partial last K step - for the per-tap kernel and for the deep stream
    for kern, mode, name in ((0, 1, "tn.m1"), (4, 0, "s4")):
        assert any(one.kernel == kern and one.mode == mode and one.o_tiles > 1 and c.Cout % 128 and c.Cin % 128 and one.S > 1
                   and M % (one.steps * one.step_rows) and M % one.step_rows
                   for c, (one, de) in wg for M in [c.B * out_hw(c)[0] * out_hw(c)[1]]), "no %s case with a ragged last o tile, a ragged i tile and a ragged last split" % name
    assert any(c.out_map == 1 for c in WGRAD_CASES), "no out_map 1 (.aspp) case"


def test_descriptor_lengths_match_the_header(K):
    from rnd_semantic_segmentation_amd import _lib
    hdr = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define MI_CPLAN_LEN (\d+)", hdr).group(1)) == K.CPLAN_LEN
    assert int(re.search(r"#define MI_WPLAN_LEN (\d+)", hdr).group(1)) == K.WPLAN_LEN


def test_old_route_queries_agree_with_the_plans(K, conv_plans, wgrad_plans):
    from rnd_semantic_segmentation_amd import _lib
    L = _lib.lib()
    for c, p in zip(CONV_CASES, conv_plans):
        (B, Ha, Wa, Ca), N, (Ho, Wo) = launch_geometry(c)
        assert L.mi_conv_gemm_route(B, Ha, Wa, Ca, Ho, Wo, N, c.ksize, c.stride, c.flags) == p.kernel, case_id(c)
    for c, (one, de) in zip(WGRAD_CASES, wgrad_plans):
        Ho, Wo = out_hw(c)
        assert L.mi_conv_wgrad_route(c.B, c.H, c.W, c.Cin, Ho, Wo, c.Cout, c.ksize, c.stride, pad_of(c), c.dil, c.out_map) == one.kernel == de.kernel, case_id(c)


def test_plan_names_are_one_per_instantiation(K):
    """A name is a function of the fields that select a template instantiation (and, for the generic epilogue, the flags it reads)."""
    assert all(isinstance(c, ConvCase) or c.plan_deferred.endswith(".deferred") for c in CASES)
    p = K.conv_gemm_plan((2, 65, 65, 64), 1024, (65, 65), 1, 1, 0, 1, 71)
    assert (p.name, p.mt, p.unit, p.pref, p.staged, p.epi) == ("nt.mt5.unit.e71.stg", 5, 1, 0, 1, 71)
    p = K.conv_gemm_plan((2, 99, 105, 64), 256, (99, 105), 3, 1, 1, 1, 69, wide=8)       # mi_conv_gemm_pp with an explicit tile height
    assert (p.name, p.kernel, p.mt) == ("pp.mtg8.e69.k1", 1, 8)
