"""mi_surface_score (csrc/surface_score.hip) on the GPU against the brute-force numpy reference of tests/_surface_ref.py: every integer with ==,
the two sums of sqrt(d2) within (n + 2) * 2^-52 relative of math.fsum over float64 square roots (one rounding per square root and per add: derived,
not measured); the torch-op composition literal_surface_stats as a second derivation; PranetTester with TEST.SURFACE_METRICS on a stub net."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import _polyp_ref as polyp_ref
import _surface_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.cases()
TOLS = (0.0, 2.0, 3.5)
PERCENTILES = (95, 100, 50)
STUB_SEED = 3
LITERAL_BAR = 1.6e-7                         # 4 x 4.11e-8, the measured maximum (test_agrees_with_the_literal_torch_composition)
K = None
M = None


@pytest.fixture(scope="module", autouse=True)
def _kern():
    global K, M
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rnd_semantic_segmentation_amd import kernels
    from rnd_semantic_segmentation_amd.host import metrics
    K, M = kernels, metrics
    yield


def _run(pred, lab, cls=1, q=95, tol=TOLS):
    r = K.surface_score(torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(lab)).cuda(), cls, q, tol)
    assert r.ints.shape == (pred.shape[0], 27) and r.ints.dtype == torch.int64 and r.sums.shape == (pred.shape[0], 2) and r.sums.dtype == torch.float64
    return r.ints.cpu().numpy(), r.sums.cpu().numpy()


_REF = {}


def _reference(key, pred, lab, cls, q, tol):
    """The reference of one image, computed once and left unchanged."""
    if key not in _REF:
        _REF[key] = ref.reference(pred, lab, cls, q, tol)
    return _REF[key]


def _assert_image(tag, ints, sums, want_ints, d2):
    assert np.array_equal(ints, want_ints), (tag, ints.tolist(), want_ints.tolist())
    n = int(want_ints[2] + want_ints[3])
    for k, w in enumerate(ref.sums(d2)):
        assert abs(sums[k] - w) <= (n + 2) * 2.0 ** -52 * w, (tag, k, sums[k], w)


@pytest.mark.parametrize("q", PERCENTILES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_single_images_equal_the_reference(name, q):
    """far_blobs_200x517: the histogram splits d2 at bit 12 (8192 high cells of 4096 values); the two order statistics of q = 95, 147425 and
    147514, fall into the neighbouring high cells 35 and 36, the maxima into cells 32 and 36."""
    p, g = CASES[name]
    assert (p == 1).any() and (g == 1).any()
    want_ints, d2, _ = _reference((name, q), p, g, 1, q, TOLS)
    ints, sums = _run(p[None], g[None], 1, q, TOLS)
    _assert_image((name, q), ints[0], sums[0], want_ints, d2)
    assert ints[0, 10] == 1 and ints[0, 17:].sum() == 0                # cells of tolerances beyond T stay 0


@pytest.mark.parametrize("tol", [(), (2.0,), (0.0, 2.0, 3.5), (0.0, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 100.0)])
def test_tolerance_counts(tol):
    p, g = CASES["speckle_33x64"]
    want_ints, d2, _ = ref.reference(p, g, 1, 95, tol)
    ints, sums = _run(p[None], g[None], 1, 95, tol)
    _assert_image(tol, ints[0], sums[0], want_ints, d2)
    if tol:
        assert ints[0, 11] + ints[0, 12] > 0                           # the masks share surface pixels: the counts at tau = 0 or 2 are not empty
    if len(tol) == 8:
        assert ints[0, 25] + ints[0, 26] == ints[0, 2] + ints[0, 3]    # tau = 100 holds every surface pixel of a 33 x 64 image


def test_batch_of_two_different_images():
    (p0, g0), (p1, g1) = CASES["speckle_37x45"], CASES["corners_37x45"]
    pred, lab = np.stack([p0, p1]), np.stack([g0, g1])
    ints, sums = _run(pred, lab)
    for b, name in enumerate(("speckle_37x45", "corners_37x45")):
        want_ints, d2, _ = _reference((name, 95), pred[b], lab[b], 1, 95, TOLS)
        _assert_image(("B2", b), ints[b], sums[b], want_ints, d2)
    assert not np.array_equal(ints[0], ints[1])


def test_batch_with_an_empty_prediction_and_a_both_empty_image():
    p0, g0 = CASES["speckle_37x45"]
    z = np.zeros_like(p0)
    pred, lab = np.stack([p0, z, z]), np.stack([g0, g0, z.astype(np.int64)])
    ints, sums = _run(pred, lab)
    for b in range(3):
        want_ints, d2, _ = ref.reference(pred[b], lab[b], 1, 95, TOLS)
        _assert_image(("B3", b), ints[b], sums[b], want_ints, d2)
    assert ints[:, 10].tolist() == [1, 0, 1]
    assert ints[1, 3] > 0 and ints[1, 4:10].sum() == 0 and ints[1, 11:].sum() == 0 and (sums[1:] == 0).all()
    assert ints[2, :10].sum() == 0
    stats = [M.surface_image_stats(ints[b], sums[b], TOLS) for b in range(3)]
    assert stats[1]["defined"] is False and stats[1]["HD"] is None and stats[1]["NSD@2"] == 0.0
    assert stats[2] == {"HD": 0.0, "HD95": 0.0, "ASSD": 0.0, "NSD@0": 1.0, "NSD@2": 1.0, "NSD@3.5": 1.0, "defined": True}


def test_class_3_of_a_map_with_several_values():
    pred, lab = ref.multi_class_map(37, 45, 6).astype(np.uint8), ref.multi_class_map(37, 45, 5)
    assert len(np.unique(lab)) == 5 and (pred == 3).any() and (lab == 3).any()
    want_ints, d2, _ = ref.reference(pred, lab, 3, 95, TOLS)
    ints, sums = _run(pred[None], lab[None], 3)
    _assert_image("cls3", ints[0], sums[0], want_ints, d2)
    other = _run(pred[None], lab[None], 1)[0]
    assert not np.array_equal(other[0], ints[0])


def test_labels_other_than_the_class_are_background():
    p, g = CASES["speckle_37x45"]
    noisy = g.copy()
    noisy[g == 0] = np.where(np.random.RandomState(9).rand(int((g == 0).sum())) < 0.3, 255, 2)
    a, b = _run(p[None], g[None]), _run(p[None], noisy[None])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


def test_two_calls_give_equal_bits():
    (p0, g0), (p1, g1) = CASES["speckle_37x45"], CASES["corners_37x45"]
    pred, lab = torch.from_numpy(np.stack([p0, p1])).cuda(), torch.from_numpy(np.stack([g0, g1])).cuda()
    a = K.surface_score(pred, lab, 1, 95, TOLS)
    p, g = CASES["far_blobs_200x517"]
    K.surface_score(torch.from_numpy(p[None]).cuda(), torch.from_numpy(g[None]).cuda())      # another size through the cached workspace in between
    b = K.surface_score(pred, lab, 1, 95, TOLS)
    assert torch.equal(a.ints, b.ints) and torch.equal(a.sums.view(torch.int64), b.sums.view(torch.int64))


def test_capped_grid_takes_a_second_trip():
    """The row launches hold at most 2^14 workgroups, one row each: 81 images of 205 x 5 are 16 605 rows, so 221 workgroups walk a second row."""
    g = np.random.RandomState(7)
    pred, lab = (g.rand(81, 205, 5) < 0.4).astype(np.uint8), (g.rand(81, 205, 5) < 0.4).astype(np.int64)
    assert 81 * 205 > 1 << 14
    ints, sums = _run(pred, lab, 1, 95, (1.0,))
    for b in range(81):
        assert (pred[b] == 1).any() and (lab[b] == 1).any()
        want_ints, d2, _ = ref.reference(pred[b], lab[b], 1, 95, (1.0,))
        _assert_image(("cap", b), ints[b], sums[b], want_ints, d2)


def test_agrees_with_the_literal_torch_composition():
    """The second derivation: literal_surface_stats (shifted comparisons, fp32 cdist, min, sort) on the GPU.  Its distances are fp32 square roots
    of exact integers, so they - not the integers - carry a tolerance: the gap |kernel - literal| / max(value, 1) of HD, HD95 and ASSD was asked
    to stay within 1e-9 and measured larger, as fp32 must: largest 4.11e-8 (HD95 of full_vs_rect_33x64; HD of far_blobs_200x517 3.43e-8, ASSD
    at most 5.4e-9), against fp32's half ulp of 6e-8.  The bar is four times the measured maximum.  NSD, an integer ratio on both sides, is
    compared exactly."""
    worst = 0.0
    for name in sorted(CASES):
        p, g = CASES[name]
        ints, sums = _run(p[None], g[None])
        got = M.surface_image_stats(ints[0], sums[0], TOLS)
        lit = M.literal_surface_stats(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), 1, 95, TOLS)
        assert list(got) == list(lit)
        for k in ("HD", "HD95", "ASSD"):
            gap = abs(got[k] - lit[k]) / max(got[k], 1.0)
            worst = max(worst, gap)
            print("literal gap %-20s %-5s %.3e" % (name, k, gap))
            assert gap <= LITERAL_BAR, (name, k, got[k], lit[k])
        for k in ("NSD@0", "NSD@2", "NSD@3.5"):
            assert got[k] == lit[k], (name, k)
    print("literal gap, largest: %.3e" % worst)


def test_wrapper_refusals():
    from rnd_semantic_segmentation_amd import _lib
    p, g = CASES["speckle_37x45"]
    pred, lab = torch.from_numpy(p[None]).cuda(), torch.from_numpy(g[None]).cuda()
    with pytest.raises(_lib.MiError, match="int64"):
        K.surface_score(pred, lab.int())
    with pytest.raises(_lib.MiError, match="uint8"):
        K.surface_score(pred.long(), lab)
    with pytest.raises(_lib.MiError, match="one device"):
        K.surface_score(pred[0], lab[0])
    with pytest.raises(_lib.MiError, match="one device"):
        K.surface_score(pred, lab[:, :20])
    with pytest.raises(_lib.MiError, match="contiguous"):
        K.surface_score(pred.transpose(1, 2), lab.transpose(1, 2))
    with pytest.raises(_lib.MiError, match="tolerances"):
        K.surface_score(pred, lab, tolerances=(1.0,) * 9)
    with pytest.raises(_lib.MiError, match="tolerances"):
        K.surface_score(pred, lab, tolerances=(-1.0,))
    with pytest.raises(_lib.MiError, match="percentile"):
        K.surface_score(pred, lab, percentile=0)
    with pytest.raises(_lib.MiError, match="percentile"):
        K.surface_score(pred, lab, percentile=95.5)
    with pytest.raises(_lib.MiError, match="cls"):
        K.surface_score(pred, lab, cls=256)


# ------------------------------------------------------------------------------------------------ the tester
class _Log(logging.Logger):
    def __init__(self):
        super().__init__("surface")
        self.lines = []

    def info(self, msg, *a, **k):
        self.lines.append(str(msg))


class _Stub(torch.nn.Module):
    """In place of the net: four fixed synthetic maps for a batch of 2 (PranetTester reads the last, res2)."""

    def __init__(self, maps):
        super().__init__()
        self.maps = maps

    def forward(self, x):
        return (self.maps * 0.5, self.maps * 0.25, self.maps * 2, self.maps)


def _cfg(tmp_path, *opts):
    from rnd_semantic_segmentation_amd.host import config as hc
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_list(["MODEL.NUM_CLASSES", 2, "OUTPUT_DIR", str(tmp_path)] + list(opts))
    cfg.freeze()
    return cfg


def _stub_inputs():
    """Two smooth maps (an ellipse of logit +4 in -4, a little noise) at 32 x 32 and speckled elliptic labels at 37 x 45."""
    g = np.random.RandomState(STUB_SEED)
    maps = np.stack([8.0 * ref.ellipse(32, 32, 15, 14, 9, 11) - 4.0, 8.0 * ref.ellipse(32, 32, 18, 20, 7, 6) - 4.0])[:, None]
    maps = (maps + 0.3 * g.randn(2, 1, 32, 32)).astype(np.float32)
    lab = np.stack([ref.speckle(ref.ellipse(37, 45, 17, 21, 11, 15), 0.02, 11), ref.speckle(ref.ellipse(37, 45, 22, 26, 8, 9), 0.02, 12)]).astype(np.int64)
    return maps, lab


def _stub_run(tmp_path, lab, maps, *opts):
    from rnd_semantic_segmentation_amd.host import pranet
    log = _Log()
    x = torch.zeros(2, 3, 32, 32)
    tester = pranet.PranetTester(_cfg(tmp_path, *opts), torch.device("cuda"), [(x, torch.from_numpy(lab), ["first", "second"])], log)
    tester.model = _Stub(torch.from_numpy(maps).cuda())
    tester.test()
    return log.lines, tester


SURF = ("TEST.SURFACE_METRICS", True, "TEST.SURFACE_PERCENTILE", 90, "TEST.SURFACE_TOLERANCES", (1.0, 3.0))
POLYP = ("TEST.POLYP_METRICS", True)


def test_tester_with_a_stub_net(tmp_path):
    maps, lab = _stub_inputs()
    pref = polyp_ref.reference_map(maps[:, 0], lab.shape[1:])
    assert float(np.abs(2 * pref - 1).min()) > 1e-4                                           # no pixel near the threshold: the mask is the reference's
    mask = (pref > 1 - pref).astype(np.uint8)
    assert all((mask[b] == 1).any() and (lab[b] == 1).any() for b in range(2))
    wants = [ref.reference(mask[b], lab[b], 1, 90, (1.0, 3.0))[2] for b in range(2)]
    want = {"HD": np.mean([w["HD"] for w in wants]), "HD90": np.mean([w["HDq"] for w in wants]), "ASSD": np.mean([w["ASSD"] for w in wants]),
            "NSD@1": np.mean([w["NSD"][0] for w in wants]), "NSD@3": np.mean([w["NSD"][1] for w in wants])}
    runs = {}
    for key, opts in (("off", ()), ("surf", SURF), ("polyp", POLYP), ("both", POLYP + SURF)):
        runs[key] = _stub_run(tmp_path / key, lab, maps, *opts)
    off, surf, polyp, both = (runs[k][0] for k in ("off", "surf", "polyp", "both"))
    assert len(off) > 2 and surf[:len(off)] == off and both[:len(polyp)] == polyp and polyp[:len(off)] == off      # earlier lines unchanged
    assert len(surf) == len(off) + 2 and len(both) == len(polyp) + 2 and surf[len(off):] == both[len(polyp):]
    assert surf[len(off)].startswith("Surface metric, val result over 2 images (0 undefined): HD/HD90 ")
    for key in ("off", "surf", "polyp", "both"):
        m, m0 = runs[key][1].meter, runs["off"][1].meter                                     # the intersection / union meters, bit for bit
        for attr in ("intersection_sum", "union_sum", "target_sum", "res_sum", "iou_sum", "f1_sum"):
            assert np.array_equal(np.asarray(getattr(m, attr)), np.asarray(getattr(m0, attr))), (key, attr)
        assert m.count == m0.count == 1
        assert os.path.exists(tmp_path / key / "pranet_surface_metrics.json") == (key in ("surf", "both"))
        assert os.path.exists(tmp_path / key / "pranet_polyp_metrics.json") == (key in ("polyp", "both"))
    assert open(tmp_path / "polyp" / "pranet_polyp_metrics.json", "rb").read() == open(tmp_path / "both" / "pranet_polyp_metrics.json", "rb").read()
    for key in ("surf", "both"):
        data = json.load(open(tmp_path / key / "pranet_surface_metrics.json"))
        assert set(data) == set(want) | {"images", "undefined", "percentile", "tolerances"}
        assert (data["images"], data["undefined"], data["percentile"], data["tolerances"]) == (2, 0, 90, [1.0, 3.0])
        for k, w in want.items():
            assert abs(data[k] - w) <= 1e-12 * max(w, 1.0), (key, k, data[k], w)
    noisy = lab.copy()
    noisy[1, 0, 0] = 255                                                                      # a label outside {0, 1} is background here ...
    lines, _ = _stub_run(tmp_path / "noisy", noisy, maps, *SURF)
    assert lines[len(off):] == surf[len(off):]
    with pytest.raises(ValueError, match="second"):                                           # ... and POLYP_METRICS refuses it as before
        _stub_run(tmp_path / "noisy_both", noisy, maps, *(POLYP + SURF))


def test_tester_counts_an_undefined_image(tmp_path):
    maps, lab = _stub_inputs()
    lab[1] = 0                                                                                # the second image has no ground truth: undefined
    lines, tester = _stub_run(tmp_path, lab, maps, *SURF)
    data = json.load(open(tmp_path / "pranet_surface_metrics.json"))
    assert (data["images"], data["undefined"]) == (2, 1) and tester.surface_meter.undefined == 1
    pref = polyp_ref.reference_map(maps[:, 0], lab.shape[1:])
    w = ref.reference((pref[0] > 1 - pref[0]).astype(np.uint8), lab[0], 1, 90, (1.0, 3.0))[2]
    assert abs(data["HD"] - w["HD"]) <= 1e-12 * w["HD"] and abs(data["NSD@1"] - w["NSD"][0] / 2) <= 1e-12
