"""GPU side of the polyp metrics: mi_polyp_score (csrc/polyp_score.hip) and PranetTester under TEST.POLYP_METRICS.  Staged as test_gpu_classwise.py:
the kernel's map against a float64 restatement (tests/_polyp_ref.py), then every statistic against numpy on the kernel's own map (integers exact),
then the whole chain - kernel outputs through host/metrics.py polyp_image_stats - against the literal float64 evaluation of the float64 map, which
shares nothing with the kernel.  Shapes are the smallest that reach each path: an odd size with a partial last workgroup row, an even width, both
axes shrinking, identity in y with growth in x; one and two images, the two with different ranges so that a per-image min-max would fail.

Measured on an MI355X at these shapes (the tolerances below are about 4 x the maxima, boxes and fp32 exponentials differ in the last bits):
  map        max |prob - reference_map| over the eight cases                     2.5e-06  (per case 6.2e-07 .. 2.5e-06)   -> MAP_TOL 1e-5
  sums       max relative error of the quadrant sums against float64 numpy       4.3e-16  (1.4e-16 .. 4.3e-16)            -> SUMS_TOL 2e-15
  metrics    max |S, MAE - literal float64 evaluation of the float64 map|        4.2e-08  (9.5e-09 .. 4.2e-08)            -> METRIC_TOL 2e-7
The curves (Dice, IoU, F, E per threshold) are functions of integers once q agrees, which the chosen seeds guarantee: they are held to 1e-12."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import _polyp_ref as ref

pytestmark = pytest.mark.gpu

MAP_TOL = 1e-5
SUMS_TOL = 2e-15
METRIC_TOL = 2e-7

SHAPES = {"odd": ((11, 13), (37, 45)), "even": ((9, 12), (33, 64)), "shrink": ((24, 24), (17, 19)), "ident_y": ((16, 16), (16, 40))}
# seeds for which the float64 map has no pixel with 255 p within 1e-3 of an integer (the batch's minimum and maximum aside) and none with
# |2 p - 1| < 1e-4: found by search on the CPU, asserted in _case
SEEDS = {("odd", 1): 11, ("odd", 2): 1348, ("even", 1): 276, ("even", 2): 2208, ("shrink", 1): 1, ("shrink", 2): 7, ("ident_y", 1): 1, ("ident_y", 2): 23}
STUB_SEED = 8464                             # the same property for the tester's stub maps (32 x 32 -> 37 x 45, two images)
CASES = [(s, B) for s in SHAPES for B in (1, 2)]

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


def make_inputs(shape, B, seed):
    """(low fp32 [B,h,w], labels int64 [B,H,W]): image 0 spans logits of about +/-9, image 1 (B == 2) a narrow range around 1 - only the batch-wide
    min-max maps both into [0, 1] as the tester does.  The ground truth is a rectangle plus speckle."""
    (h, w), (H, W) = SHAPES[shape]
    g = np.random.RandomState(seed)
    low = (g.randn(B, h, w) * 3).astype(np.float32)
    if B == 2:
        low[1] = low[1] / 6 + 1
    lab = np.zeros((B, H, W), np.int64)
    for b in range(B):
        lab[b, H // 4 + b:H // 4 + b + H // 2, W // 3:W // 3 + W // 2 + b] = 1
    flip = g.rand(B, H, W) < 0.03
    lab[flip] = 1 - lab[flip]
    return low, lab


def margins(p):
    """(distance of 255 p from the nearest integer, minimum over the pixels that are not the batch's extremes; minimum of |2 p - 1|)."""
    inner = p[(p > 0) & (p < 1 - 1e-6)] * 255
    return float(np.abs(inner - np.rint(inner)).min()), float(np.abs(2 * p - 1).min())


_CASE = {}


def _case(shape, B):
    """Inputs, the float64 reference map and its per-image metrics, and the kernel's outputs with every side output; computed once, left unchanged."""
    key = (shape, B)
    if key not in _CASE:
        low, lab = make_inputs(shape, B, SEEDS[key])
        pref = ref.reference_map(low, lab.shape[1:])
        near_int, near_half = margins(pref)
        assert near_int > 1e-3 and near_half > 1e-4, (key, near_int, near_half)
        sig = 1 / (1 + np.exp(-ref.reference_logits(low, lab.shape[1:])))
        assert sig.max() - sig.min() > 0.5                     # the maximum normalises to float32 1.0 on both sides: q = 255
        want = [ref.reference_metrics(pref[b], lab[b]) for b in range(B)]
        r = K.polyp_score(torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda(), want_prob=True, want_pred=True)
        got = {k: getattr(r, k).cpu().numpy() for k in r._fields}
        for a in [low, lab, pref, sig] + list(got.values()):
            a.setflags(write=False)
        _CASE[key] = dict(low=low, lab=lab, pref=pref, sig=sig, want=want, got=got)
    return _CASE[key]


# ------------------------------------------------------------------------------------------------ the map
@pytest.mark.parametrize("shape,B", CASES)
def test_map_parity_with_the_float64_restatement(shape, B):
    c = _case(shape, B)
    prob = c["got"]["prob"]
    err = float(np.abs(prob.astype(np.float64) - c["pref"]).max())
    print("\n[polyp map] %s B=%d: max |prob - float64 reference| %.3e" % (shape, B, err))
    assert err < MAP_TOL
    assert prob.dtype == np.float32 and prob.min() == 0.0 and prob.max() <= 1.0
    sums = c["got"]["sums"]
    assert (sums[:, 22] == sums[0, 22]).all() and (sums[:, 23] == sums[0, 23]).all()          # one min / max for the batch
    assert abs(sums[0, 22] - c["sig"].min()) < MAP_TOL and abs(sums[0, 23] - c["sig"].max()) < MAP_TOL


# ------------------------------------------------------------------------------------------------ the statistics of the kernel's own map
@pytest.mark.parametrize("shape,B", CASES)
def test_statistics_equal_numpy_on_the_kernels_own_map(shape, B):
    c = _case(shape, B)
    got = c["got"]
    worst = 0.0
    for b in range(B):
        hist, sums, counts, pred = ref.counted(got["prob"][b], c["lab"][b])
        assert np.array_equal(got["hist"][b], hist)
        assert np.array_equal(got["counts"][b], counts) and counts[3] == 0
        assert np.array_equal(got["pred"][b], pred)
        assert got["sums"][b, 20] == sums[20] and got["sums"][b, 21] == sums[21]
        assert M.polyp_centre(*got["counts"][b, :3]) == (int(sums[20]), int(sums[21]))
        zero = sums[:20] == 0
        assert (got["sums"][b, :20][zero] == 0).all()
        rel = np.abs(got["sums"][b, :20][~zero] - sums[:20][~zero]) / np.abs(sums[:20][~zero])
        worst = max(worst, float(rel.max()))
        assert np.array_equal(got["sums"][b, 4:20:5], sums[4:20:5])                            # the per-quadrant foreground counts are integers
    print("\n[polyp sums] %s B=%d: max relative error of the quadrant sums %.3e" % (shape, B, worst))
    assert worst < SUMS_TOL


# ------------------------------------------------------------------------------------------------ end to end
def _assert_metrics(got, want, tag, exact_curves=True):
    worst = 0.0
    for k in ("dice", "iou", "f", "e"):
        err = float(np.abs(got[k] - want[k]).max())
        worst = max(worst, err)
        # the curves are functions of integers (TP_t, FP_t, G, N): with the same q on both sides only float64 rounding separates them
        assert err < (1e-12 if exact_curves else METRIC_TOL), (tag, k, err)
    for k in ("S", "MAE"):
        worst = max(worst, abs(got[k] - want[k]))
        assert abs(got[k] - want[k]) < METRIC_TOL, (tag, k, got[k], want[k])
    return worst


@pytest.mark.parametrize("shape,B", CASES)
def test_end_to_end_against_the_literal_float64_evaluation(shape, B):
    c = _case(shape, B)
    H, W = c["lab"].shape[1:]
    worst = 0.0
    for b in range(B):
        q_ref = ref.quantise(c["pref"][b])
        g = c["lab"][b] == 1
        assert np.array_equal(c["got"]["hist"][b], np.stack([np.bincount(q_ref[~g], minlength=256), np.bincount(q_ref[g], minlength=256)]))
        got = M.polyp_image_stats(c["got"]["hist"][b], c["got"]["sums"][b], H, W)
        worst = max(worst, _assert_metrics(got, c["want"][b], (shape, B, b)))
    print("\n[polyp metrics] %s B=%d: max |metric - literal float64| %.3e" % (shape, B, worst))


@pytest.mark.parametrize("shape,B", CASES)
def test_mask_equals_the_literal_testers(shape, B):
    """pred against the mask of PranetTester.predict's own torch composition (gresize, sigmoid, batch min-max, p > 1 - p) on the same map; the
    inputs have no pixel with |2 p - 1| < 1e-4 in the float64 reference (_case asserts it), so the comparison is equality."""
    from rnd_semantic_segmentation_amd import gk
    c = _case(shape, B)
    low = torch.from_numpy(c["low"].copy()).cuda()
    out = gk.gresize(low.unsqueeze(3).contiguous(), c["lab"].shape[1:], False).permute(0, 3, 1, 2)
    p = out.sigmoid().squeeze(1)
    p = (p - p.min()) / (p.max() - p.min() + 1e-8)
    literal = (p > 1 - p).to(torch.uint8).cpu().numpy()
    assert np.array_equal(c["got"]["pred"], literal)
    assert np.array_equal(c["got"]["pred"], (c["pref"] > 0.5).astype(np.uint8))
    assert 0 < literal.mean() < 1


# ------------------------------------------------------------------------------------------------ contention and degenerate inputs
def _degenerate(name):
    """One image at the odd shape, on the random map of the end-to-end case (so its q is the reference's, _case asserts the margins) unless named."""
    (h, w), (H, W) = SHAPES["odd"]
    low, lab = make_inputs("odd", 1, SEEDS[("odd", 1)])
    if name == "saturated":                     # logits of +/-40 at the label size (identity resize): every pixel in bin 0 or bin 255, whole waves in one cell
        low = np.where(np.arange(W)[None, None, :] < W // 2, -40.0, 40.0).astype(np.float32) * np.ones((1, H, 1), np.float32)
        low[0, ::5, ::7] *= -1
    elif name == "constant":                    # max == min: every p is 0
        low = np.full((1, h, w), 0.75, np.float32)
    elif name == "G_is_0":
        lab = np.zeros_like(lab)
    elif name == "G_is_N":
        lab = np.ones_like(lab)
    elif name == "last_column":
        lab = np.zeros_like(lab)
        lab[0, 5:30, W - 1] = 1
    return low, lab


@pytest.mark.parametrize("name", ["saturated", "constant", "G_is_0", "G_is_N", "last_column"])
def test_contention_and_degenerate_inputs(name):
    low, lab = _degenerate(name)
    H, W = lab.shape[1:]
    r = K.polyp_score(torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda(), want_prob=True, want_pred=True)
    prob, hist, sums, counts = r.prob.cpu().numpy()[0], r.hist.cpu().numpy()[0], r.sums.cpu().numpy()[0], r.counts.cpu().numpy()[0]
    h_np, s_np, c_np, pred_np = ref.counted(prob, lab[0])
    assert np.array_equal(hist, h_np) and np.array_equal(counts, c_np) and np.array_equal(r.pred.cpu().numpy()[0], pred_np)
    assert sums[20] == s_np[20] and sums[21] == s_np[21] and int(hist.sum()) == H * W
    if name == "saturated":
        assert hist[:, 1:255].sum() == 0 and hist[:, 0].sum() > 0 and hist[:, 255].sum() > 0
        assert set(np.unique(prob)) == {0.0, 1.0}
    if name == "constant":
        assert (prob == 0).all() and hist[:, 1:].sum() == 0 and (sums[[0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18]] == 0).all()
    if name == "G_is_0":
        assert counts[0] == 0 and hist[1].sum() == 0 and (sums[20], sums[21]) == (0, 0)
    if name == "G_is_N":
        assert counts[0] == H * W and hist[0].sum() == 0
    if name == "last_column":
        assert sums[20] == W and sums[5 + 4] == 0 and sums[15 + 4] == 0
    pref = ref.reference_map(low, (H, W))[0]
    assert np.array_equal(ref.quantise(prob), ref.quantise(pref))          # bins 0 / 255 by construction, or the margins of the end-to-end map
    _assert_metrics(M.polyp_image_stats(hist, sums, H, W), ref.reference_metrics(pref, lab[0]), name)


# ------------------------------------------------------------------------------------------------ determinism and side outputs
def test_reproducible_and_independent_of_the_side_outputs():
    low, lab = make_inputs("odd", 2, 5)
    low, lab = torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda()
    a = K.polyp_score(low, lab, want_prob=True, want_pred=True)
    b = K.polyp_score(low, lab, want_prob=True, want_pred=True)
    c = K.polyp_score(low, lab, want_prob=False, want_pred=False)
    d = K.polyp_score(low, lab, want_prob=False, want_pred=True)
    assert c.prob is None and c.pred is None and d.prob is None
    for other in (b, c, d):
        assert torch.equal(a.sums.view(torch.int64), other.sums.view(torch.int64))            # bit-equal doubles
        assert torch.equal(a.hist, other.hist) and torch.equal(a.counts, other.counts)
    assert torch.equal(a.prob, b.prob) and torch.equal(a.pred, b.pred) and torch.equal(a.pred, d.pred)
    assert int(a.counts[:, 3].sum()) == 0


def test_labels_outside_0_1_are_reported():
    low, lab = make_inputs("even", 2, 6)
    clean = K.polyp_score(torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda())
    lab = lab.copy()
    lab[1, 3, 4:9] = 255
    lab[1, 20, 63] = 2
    was_fg = int((make_inputs("even", 2, 6)[1][1][lab[1] > 1] == 1).sum())
    r = K.polyp_score(torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda())
    assert r.counts[:, 3].tolist() == [0, 6]
    assert int(r.counts[1, 0]) == int(clean.counts[1, 0]) - was_fg                            # counted as background
    assert torch.equal(r.hist[0], clean.hist[0]) and int(r.hist[1].sum()) == 33 * 64


def test_wrapper_refusals():
    from rnd_semantic_segmentation_amd import _lib
    low, lab = make_inputs("odd", 2, 5)
    low, lab = torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda()
    with pytest.raises(_lib.MiError, match="int64"):
        K.polyp_score(low, lab.int())
    with pytest.raises(_lib.MiError, match="float32"):
        K.polyp_score(low.double(), lab)
    with pytest.raises(_lib.MiError, match="one device"):
        K.polyp_score(low[:1], lab)
    with pytest.raises(_lib.MiError, match="contiguous"):
        K.polyp_score(low.transpose(1, 2), lab)


# ------------------------------------------------------------------------------------------------ the tester
class _Log(logging.Logger):
    def __init__(self):
        super().__init__("polyp")
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


def _stub_run(tmp_path, lab, maps, *opts):
    from rnd_semantic_segmentation_amd.host import pranet
    log = _Log()
    x = torch.zeros(2, 3, 32, 32)
    tester = pranet.PranetTester(_cfg(tmp_path, *opts), torch.device("cuda"), [(x, torch.from_numpy(lab), ["first", "second"])], log)
    tester.model = _Stub(torch.from_numpy(maps).cuda())
    tester.test()
    return log.lines


def _stub_inputs(seed=None):
    g = np.random.RandomState(STUB_SEED if seed is None else seed)
    maps = (g.randn(2, 1, 32, 32) * 3).astype(np.float32)
    maps[1] = maps[1] / 4 - 1
    lab = make_inputs("odd", 2, 21)[1]
    return maps, lab


def test_tester_with_a_stub_net(tmp_path):
    maps, lab = _stub_inputs()
    on = _stub_run(tmp_path / "on", lab, maps, "TEST.POLYP_METRICS", True)
    off = _stub_run(tmp_path / "off", lab, maps)
    assert not os.path.exists(tmp_path / "off" / "pranet_polyp_metrics.json") and not any("Polyp" in s for s in off)
    assert on[:len(off)] == off and len(off) > 2                                              # the intersection / union lines, unchanged
    pref = ref.reference_map(maps[:, 0], lab.shape[1:])
    assert margins(pref)[0] > 1e-3 and margins(pref)[1] > 1e-4
    want, curves = ref.aggregate([ref.reference_metrics(pref[b], lab[b]) for b in range(2)])
    rlog = _Log()
    rlog.info("Polyp metric, val result over 2 images: mDice/mIoU {:.4f}/{:.4f}.".format(want["mDice"], want["mIoU"]))
    rlog.info("Polyp metric, val result: meanF/maxF {:.4f}/{:.4f}, S-measure {:.4f}.".format(want["meanF"], want["maxF"], want["S"]))
    rlog.info("Polyp metric, val result: meanE/maxE {:.4f}/{:.4f}, MAE {:.4f}.".format(want["meanE"], want["maxE"], want["MAE"]))
    assert on[len(off):] == rlog.lines, (on[len(off):], rlog.lines)
    data = json.load(open(tmp_path / "on" / "pranet_polyp_metrics.json"))
    assert set(data) == set(M.POLYP_KEYS) | {"images", "dice_curve", "iou_curve"} and data["images"] == 2
    for k in M.POLYP_KEYS:
        assert abs(data[k] - want[k]) < METRIC_TOL, (k, data[k], want[k])
    assert np.abs(np.array(data["dice_curve"]) - curves["dice"]).max() < METRIC_TOL
    assert np.abs(np.array(data["iou_curve"]) - curves["iou"]).max() < METRIC_TOL
    bad = lab.copy()
    bad[1, 0, 0] = 255
    with pytest.raises(ValueError, match="second"):
        _stub_run(tmp_path / "bad", bad, maps, "TEST.POLYP_METRICS", True)
    assert len(_stub_run(tmp_path / "bad_off", bad, maps)) == len(off)                        # the default path ignores 255 as ever


def test_tester_with_a_real_net(tmp_path):
    from rnd_semantic_segmentation_amd.host import pranet, synth
    img, mask = synth.synth_polyp(2, 64, 64, seed=8)
    lines = {}
    for key, opts in (("off", ()), ("on", ("TEST.POLYP_METRICS", True))):
        log = _Log()
        torch.manual_seed(13)
        tester = pranet.PranetTester(_cfg(tmp_path / key, *opts), torch.device("cuda"), [(torch.from_numpy(img), torch.from_numpy(mask), ["a", "b"])], log)
        assert tester.model.precision == "fp32"
        tester.test()
        lines[key] = log.lines
    assert lines["on"][:len(lines["off"])] == lines["off"] and len(lines["on"]) == len(lines["off"]) + 3
    data = json.load(open(tmp_path / "on" / "pranet_polyp_metrics.json"))
    assert data["images"] == 2 and all(np.isfinite(v).all() for v in (np.asarray(v, dtype=np.float64) for v in data.values()))
    assert not os.path.exists(tmp_path / "off" / "pranet_polyp_metrics.json")
