"""Host side of the precision-recall curves and the calibration numbers (TEST.CURVES), no GPU: literal_curves of host/metrics.py against the
numpy restatement of tests/_curves_ref.py on maps with values on bin edges, tied maxima and out-of-range labels; the histograms' sum identities;
curves_summary against sklearn's average precision, a direct float64 ECE, a brute-force threshold scan and the masks literal_pseudo writes; the
TEST.CURVES* and TEST.PSEUDO_CLASS_THRESHOLDS keys with every refusal; the shipped configuration; the C-ABI entries mi_upsample_curves /
mi_upsample_curves_slide: declared, exported, in the ctypes table, refusing before any launch."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import _curves_ref as ref
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    entry.build()
    return _lib.lib()


def _cfg(tmp_path, *opts):
    from core.configs import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["MODEL.NUM_CLASSES", 19, "OUTPUT_DIR", str(tmp_path)] + list(opts))
    return cfg


def _map(K, hw, seed, sharp=4.0, half_tie=True):
    """A [K,H,W] fp32 probability map (softmax of noise) with planted values: exactly 0 and 1, bin edges j/256 and m/15, tied maxima; and labels
    with -1, K, 254, 255 and 300 among them.  half_tie False leaves out the one pixel where two classes hold exactly 0.5 each."""
    g = np.random.RandomState(seed)
    z = g.randn(K, *hw) * sharp
    p = np.exp(z - z.max(0))
    p = (p / p.sum(0)).astype(np.float32)
    H, W = hw
    flat = p.reshape(K, -1)
    n = flat.shape[1]
    cols = g.permutation(n)
    c = 0
    for j in (0, 1, 37, 128, 255, 256) if half_tie else (0, 1, 37, 255, 256):      # class 0 exactly on a curve-bin edge (0 and 1 among them)
        flat[:, cols[c]] = 0.0
        flat[0, cols[c]] = np.float32(j / 256.0)
        if K > 1:
            flat[1, cols[c]] = np.float32(1.0 - j / 256.0)
        c += 1
    for m in range(16):                                      # the maximum exactly on a calibration-bin edge m/15 (fp32-rounded)
        flat[:, cols[c]] = 0.0
        flat[min(K - 1, 2), cols[c]] = np.float32(m) / np.float32(15)
        c += 1
    for a, b in ((0, K - 1), (1, 0), (K - 1, K // 2)) if K > 1 else ():      # ties for the maximum: the lowest index wins
        flat[:, cols[c]] = np.float32(0.125)
        flat[a, cols[c]] = flat[b, cols[c]] = np.float32(0.4375)
        c += 1
    lab = g.randint(0, K, size=hw).astype(np.int64)
    odd = np.array([-1, K, 254, 255, 300], dtype=np.int64)
    where = g.rand(*hw) < 0.3
    lab[where] = odd[g.randint(0, odd.size, size=int(where.sum()))]
    return p, lab


CASES = [(19, (23, 31), 1), (5, (16, 20), 2), (2, (17, 9), 3), (32, (12, 14), 4), (1, (6, 7), 5)]


@pytest.mark.parametrize("K,hw,seed", CASES)
@pytest.mark.parametrize("M", [1, 15, 64])
def test_literal_equals_the_numpy_restatement(K, hw, seed, M):
    p, lab = _map(K, hw, seed)
    pr, cal = metrics.literal_curves(torch.from_numpy(p)[None], torch.from_numpy(lab)[None], K, M)
    want_pr, want_cal = ref.curves_ref(p, lab, K, M)
    assert pr.dtype == torch.int64 and tuple(pr.shape) == (K, 256, 2) and tuple(cal.shape) == (M, 3)
    assert np.array_equal(pr.numpy(), want_pr) and np.array_equal(cal.numpy(), want_cal)
    counted = int(((lab >= 0) & (lab < K)).sum())
    assert 0 < counted < lab.size                                            # the out-of-range labels are there and count nowhere
    for k in range(K):
        assert int(pr[k].sum()) == counted and int(pr[k, :, 1].sum()) == int((lab == k).sum())
    assert int(cal[:, 0].sum()) == counted and int(cal[:, 1].sum()) <= counted
    if K > 1:
        assert int(pr[0, 0].sum()) > 0 and int(pr[0, 255].sum()) > 0             # exact 0 and exact 1 were counted in the end bins


def test_ties_edges_and_labels_by_hand():
    p = np.zeros((3, 1, 6), np.float32)
    p[:, 0, 0] = (0.5, 0.5, 0.0)           # a tie: pred 0
    p[:, 0, 1] = (0.25, 0.25, 0.5)
    p[:, 0, 2] = (1.0, 0.0, 0.0)
    p[:, 0, 3] = (0.0, 1.0, 0.0)           # label 255: counts nowhere
    p[:, 0, 4] = (0.0, 0.0, 1.0)           # label 3 == K: counts nowhere
    p[:, 0, 5] = (0.2, 0.2, 0.6)           # label -1
    lab = np.array([[1, 2, 0, 255, 3, -1]])
    pr, cal = metrics.literal_curves(torch.from_numpy(p)[None], torch.from_numpy(lab)[None], 3, 4)
    assert int(pr.sum()) == 9
    assert pr[0, 128].tolist() == [1, 0] and pr[1, 128].tolist() == [0, 1] and pr[2, 0].tolist() == [2, 0]
    assert pr[0, 64].tolist() == [1, 0] and pr[2, 128].tolist() == [0, 1] and pr[0, 255].tolist() == [0, 1]
    # conf 0.5 -> bin 2 of 4 (twice: a miss - the tie goes to class 0, the label is 1 - and a hit), conf 1.0 -> clamped into bin 3
    assert cal.tolist() == [[0, 0, 0], [0, 0, 0], [2, 1, 2 << 23], [1, 1, 1 << 24]]


def test_literal_refuses_bad_arguments():
    p = torch.full((1, 3, 4, 4), 1 / 3)
    lab = torch.zeros(1, 4, 4, dtype=torch.int64)
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="ece_bins"):
            metrics.literal_curves(p, lab, 3, bad)
    with pytest.raises(ValueError, match="map must be"):
        metrics.literal_curves(p, lab, 4, 15)


# ------------------------------------------------------------------------------------------------ the summary
def _scores(p, lab, K):
    counted = (lab >= 0) & (lab < K)
    b = np.minimum(255, np.trunc(p[:, counted] * np.float32(256)).astype(np.int64))
    return b, lab[counted], p[:, counted]


@pytest.mark.parametrize("K,hw,seed,sharp", [(19, (40, 50), 11, 4.0), (5, (30, 30), 12, 1.0), (19, (40, 50), 13, 12.0)])
def test_average_precision_equals_sklearn(K, hw, seed, sharp):
    sk = pytest.importorskip("sklearn.metrics", reason="sklearn is the reference of the average precision")
    p, lab = _map(K, hw, seed, sharp)
    pr, cal = ref.curves_ref(p, lab, K, 15)
    table = metrics.curves_summary(pr, cal, None, 0.9)
    b, lc, _ = _scores(p, lab, K)
    worst, aps = 0.0, []
    for k in range(K):
        if not (lc == k).any():
            assert table["ap"][k] is None
            continue
        want = sk.average_precision_score(lc == k, b[k] / 256.0)
        worst = max(worst, abs(want - table["ap"][k]))
        aps.append(table["ap"][k])
    print("AP against sklearn, K=%d sharp %.0f: largest difference %.2e" % (K, sharp, worst))
    assert worst <= 1e-12 and aps          # two float64 sums of at most 256 terms not above 1
    assert table["map"] == sum(aps) / len(aps)


def test_a_class_without_positives_is_left_out():
    pr = np.zeros((3, 256, 2), np.int64)
    pr[0, 200, 1] = 5
    pr[0, 10, 0] = 5
    pr[1, 0, 0] = 10                        # never the label
    pr[2, 100, 1] = 2
    pr[2, 150, 0] = 8
    cal = np.zeros((2, 3), np.int64)
    t = metrics.curves_summary(pr, cal, ["a", "b", "c"], 0.5)
    assert t["classes"] == ["a", "b", "c"] and t["positives"] == [5, 0, 2]
    assert t["ap"][1] is None and t["best_f1"][1] is None and t["pseudo_class_thresholds"][1] == 1.0
    assert t["ap"][0] == 1.0 and t["best_f1"][0] == 1.0 and t["best_f1_threshold"][0] == 11 / 256
    assert t["ap"][2] == 0.2 and t["map"] == 0.6
    # class 2: at t >= 0.5 the 8 negatives in bin 150 are all that is left (precision 0) until nothing is left (precision 1 by definition)
    assert t["threshold_at_precision"][2] == 151 / 256 and t["recall_at_precision"][2] == 0.0
    assert t["threshold_at_precision"][0] == 0.5 and t["recall_at_precision"][0] == 1.0
    c = t["calibration"]
    assert c["ece"] is None and c["count"] == [0, 0] and c["accuracy"] == [None, None]
    json.dumps(t)                           # no NaN, nothing numpy


@pytest.mark.parametrize("target", [0.5, 0.9, 1.0])
def test_threshold_at_precision_equals_a_brute_force_scan(target):
    K = 7
    p, lab = _map(K, (40, 40), 21, 2.0)
    pr, cal = ref.curves_ref(p, lab, K, 15)
    table = metrics.curves_summary(pr, cal, None, target)
    b, lc, _ = _scores(p, lab, K)
    for k in range(K):
        found = None
        for j in range(128, 256):
            kept = b[k] >= j
            tp, n = int((kept & (lc == k)).sum()), int(kept.sum())
            if (tp / n if n else 1.0) >= target:
                found = (j / 256, tp / int((lc == k).sum()))
                break
        if found is None:
            assert table["threshold_at_precision"][k] is None and table["pseudo_class_thresholds"][k] == 1.0
        else:
            assert (table["threshold_at_precision"][k], table["recall_at_precision"][k]) == found
            assert table["pseudo_class_thresholds"][k] == found[0]
        f1 = []
        for j in range(256):
            kept = b[k] >= j
            tp, n, pos = int((kept & (lc == k)).sum()), int(kept.sum()), int((lc == k).sum())
            P, R = (tp / n if n else 1.0), tp / pos
            f1.append(2 * P * R / (P + R) if P + R else 0.0)
        assert abs(table["best_f1"][k] - max(f1)) < 1e-15 and table["best_f1_threshold"][k] == int(np.argmax(f1)) / 256


def test_ece_equals_a_direct_evaluation():
    K, M = 19, 15
    p, lab = _map(K, (40, 50), 31, 3.0)
    pr, cal = ref.curves_ref(p, lab, K, M)
    c = metrics.curves_summary(pr, cal)["calibration"]
    _, lc, pc = _scores(p, lab, K)
    conf = pc.max(0)
    hit = (pc.argmax(0) == lc).astype(np.float64)
    m = np.minimum(M - 1, np.trunc(conf * np.float32(M)).astype(np.int64))
    conf64 = np.trunc(conf.astype(np.float64) * 2 ** 24) / 2 ** 24              # the histogram keeps 24 fractional bits
    ece, mce = 0.0, 0.0
    for j in range(M):
        sel = m == j
        if sel.any():
            gap = abs(hit[sel].mean() - conf64[sel].mean())
            ece += sel.sum() / conf.size * gap
            mce = max(mce, gap)
            assert abs(c["accuracy"][j] - hit[sel].mean()) < 1e-12 and abs(c["confidence"][j] - conf64[sel].mean()) < 1e-12
        else:
            assert c["accuracy"][j] is None and c["count"][j] == 0
    assert abs(c["ece"] - ece) < 1e-12 and abs(c["mce"] - mce) < 1e-12
    assert abs(c["overall_accuracy"] - hit.mean()) < 1e-12 and abs(c["mean_confidence"] - conf64.mean()) < 1e-12
    assert abs(conf64.mean() - conf.astype(np.float64).mean()) < 2.0 ** -24      # the truncation loses less than one unit per pixel


def test_precision_above_one_half_is_the_pseudo_labels_precision():
    """For t_j >= 0.5, p_c >= t_j implies that c is the prediction: the masks literal_pseudo writes with the scalar threshold t_j keep for class c
    exactly the pixels the curve counts at j.  The one exception, at t = 0.5 itself: two classes that hold exactly 0.5 each - both count at
    j = 128, only the lower index is the prediction (the last lines)."""
    K = 5
    p, lab = _map(K, (30, 40), 41, 2.0, half_tie=False)
    pr, cal = ref.curves_ref(p, lab, K, 15)
    counted = (lab >= 0) & (lab < K)
    out = torch.from_numpy(p)[None]
    for j in (128, 160, 200, 255):
        mask = metrics.literal_pseudo(out, [j / 256] * K).numpy()
        for k in range(K):
            kept = (mask == k) & counted
            tp, n = int((kept & (lab == k)).sum()), int(kept.sum())
            assert tp == int(pr[k, j:, 1].sum()) and n == int(pr[k, j:].sum())
    tie = torch.tensor([0.5, 0.5, 0.0]).reshape(1, 3, 1, 1)
    pr, _ = metrics.literal_curves(tie, torch.ones(1, 1, 1, dtype=torch.int64), 3, 15)
    assert int(pr[0, 128:].sum()) == 1 and int(pr[1, 128:].sum()) == 1 and metrics.literal_pseudo(tie, [0.5] * 3).tolist() == [[0]]


def test_summary_refuses_bad_arguments():
    pr, cal = np.zeros((3, 256, 2), np.int64), np.zeros((15, 3), np.int64)
    for bad in (0.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="target precision"):
            metrics.curves_summary(pr, cal, None, bad)
    with pytest.raises(ValueError, match="pr must be"):
        metrics.curves_summary(pr[:, :128], cal)


# ------------------------------------------------------------------------------------------------ configuration
def test_config_keys_defaults_and_settings(tmp_path):
    from core.configs import cfg as global_cfg
    t = global_cfg.TEST
    assert t.CURVES is False and t.CURVES_ECE_BINS == 15 and t.CURVES_PRECISION == 0.9 and tuple(t.PSEUDO_CLASS_THRESHOLDS) == ()
    assert metrics.curves_settings(global_cfg) is None and metrics.class_threshold_settings(global_cfg) is None
    assert metrics.curves_settings(_cfg(tmp_path, "TEST.CURVES", "True")) == (15, 0.9)
    assert metrics.curves_settings(_cfg(tmp_path, "TEST.CURVES", True, "TEST.CURVES_ECE_BINS", 64, "TEST.CURVES_PRECISION", 1.0)) == (64, 1.0)
    bare = type("C", (), {"TEST": {}, "MODEL": type("M", (), {"NUM_CLASSES": 19})()})()      # an older tree: the defaults
    assert metrics.curves_settings(bare) is None and metrics.class_threshold_settings(bare) is None
    metrics.require_no_curves(bare, "AnyTester")
    metrics.require_no_curves(_cfg(tmp_path), "AnyTester")


@pytest.mark.parametrize("key,bad", [("CURVES_ECE_BINS", 0), ("CURVES_ECE_BINS", 65), ("CURVES_ECE_BINS", -3), ("CURVES_PRECISION", 0.0),
                                     ("CURVES_PRECISION", 1.5), ("CURVES_PRECISION", -0.5), ("CURVES_PRECISION", float("nan"))])
def test_settings_refuse_bad_values(tmp_path, key, bad):
    with pytest.raises(ValueError, match=key):
        metrics.curves_settings(_cfg(tmp_path, "TEST.CURVES", True, "TEST." + key, bad))
    plain = type("C", (), {"TEST": {"CURVES": True, key: bad}})()
    with pytest.raises(ValueError, match=key):
        metrics.curves_settings(plain)


def test_settings_refuse_other_types():
    for test in ({"CURVES": 1}, {"CURVES": True, "CURVES_ECE_BINS": 15.0}, {"CURVES": True, "CURVES_ECE_BINS": True},
                 {"CURVES": True, "CURVES_PRECISION": "0.9"}, {"CURVES": True, "CURVES_PRECISION": True}):
        with pytest.raises(ValueError, match="CURVES"):
            metrics.curves_settings(type("C", (), {"TEST": test})())


@pytest.mark.parametrize("key,value", [("CURVES_ECE_BINS", 10), ("CURVES_PRECISION", 0.8)])
def test_a_stray_key_is_refused(tmp_path, key, value):
    from core.testers.aspp_tester import ASPPTester
    from core.testers.gald_tester import GALDTester
    from core.testers.pranet_tester import PranetTester
    logger = type("L", (), {"info": lambda self, s: None})()
    stray = _cfg(tmp_path, "TEST." + key, value)
    with pytest.raises(NotImplementedError, match=key):
        metrics.curves_settings(stray)
    with pytest.raises(NotImplementedError, match=key):
        metrics.require_no_curves(stray, "AnyTester")
    with pytest.raises(NotImplementedError, match=key):
        ASPPTester(stray, torch.device("cpu"), [], logger, [0] * 57, {}, saveres=False)
    with pytest.raises(NotImplementedError, match=key):
        PranetTester(stray, torch.device("cpu"), [], logger)
    with pytest.raises(NotImplementedError, match=key):
        GALDTester(stray, torch.device("cpu"), [], logger, [0] * 57)


def test_other_testers_refuse_the_keys(tmp_path):
    from core.testers.gald_tester import GALDTester
    from core.testers.pranet_tester import PranetTester
    logger = type("L", (), {"info": lambda self, s: None})()
    for on, needle in ((_cfg(tmp_path, "TEST.CURVES", True), "TEST.CURVES"),
                       (_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", [0.5] * 19), "TEST.PSEUDO_CLASS_THRESHOLDS")):
        with pytest.raises(NotImplementedError, match=needle):
            metrics.require_no_curves(on, "AnyTester")
        with pytest.raises(NotImplementedError, match="PranetTester: " + needle):
            PranetTester(on, torch.device("cpu"), [], logger)
        with pytest.raises(NotImplementedError, match="GALDTester: " + needle):
            GALDTester(on, torch.device("cpu"), [], logger, [0] * 57)


def test_class_threshold_rules(tmp_path):
    from core.testers.aspp_tester import ASPPTester
    logger = type("L", (), {"info": lambda self, s: None})()
    good = [0.5 + 0.02 * i for i in range(19)]
    assert metrics.class_threshold_settings(_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", good)) == tuple(good)
    assert metrics.class_threshold_settings(_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", [0.0] * 18 + [1.0])) == (0.0,) * 18 + (1.0,)
    with pytest.raises(ValueError, match="18 values for 19 classes"):
        metrics.class_threshold_settings(_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", good[:18]))
    with pytest.raises(ValueError, match="20 values for 19 classes"):
        metrics.class_threshold_settings(_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", good + [0.5]))
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            metrics.class_threshold_settings(_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", good[:18] + [bad]))
    with pytest.raises(NotImplementedError, match="PSEUDO_CLASSWISE"):
        metrics.class_threshold_settings(_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", good, "TEST.PSEUDO_CLASSWISE", True))
    with pytest.raises(NotImplementedError, match="PSEUDO_THRESHOLD"):
        metrics.class_threshold_settings(_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", good, "TEST.PSEUDO_THRESHOLD", 0.9))
    with pytest.raises(NotImplementedError, match="PSEUDO_CLASSWISE"):
        ASPPTester(_cfg(tmp_path, "TEST.PSEUDO_CLASS_THRESHOLDS", good, "TEST.PSEUDO_CLASSWISE", True), torch.device("cpu"), [], logger, [0] * 57,
                   {}, saveres=False)
    with pytest.raises(ValueError, match="must be a list"):
        metrics.class_threshold_settings(type("C", (), {"TEST": {"PSEUDO_CLASS_THRESHOLDS": 0.5}})())


def test_shipped_configuration_loads():
    from core.configs import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_test_curves.yaml"))
    assert metrics.curves_settings(cfg) == (15, 0.9) and metrics.class_threshold_settings(cfg) is None
    assert metrics.boundary_settings(cfg) is None and metrics.crf_settings(cfg) is None and metrics.slide_settings(cfg) is None
    assert cfg.MODEL.NUM_CLASSES == 19 and cfg.DATASETS.TEST == "cityscapes_val" and tuple(cfg.INPUT.INPUT_SIZE_TEST) == (2048, 1024)
    assert "deeplabv2_r101_test_curves.yaml" in open(os.path.join(ROOT, "README.md")).read()


# ------------------------------------------------------------------------------------------------ the tester on CPU tensors (the literal path)
def test_predict_and_score_counts_curves_on_cpu_tensors():
    K = 4
    p, lab = _map(K, (12, 15), 51)
    out = torch.from_numpy(p)[None]

    class Net(torch.nn.Module):
        def forward(self, x, size=None):
            return x

    fe, cl = Net(), type("Cl", (torch.nn.Module,), {"forward": lambda self, f, size=None: torch.log(out.clamp_min(1e-30))})()
    pr = torch.zeros(K, 256, 2, dtype=torch.int64)
    cal = torch.zeros(15, 3, dtype=torch.int64)
    y = torch.from_numpy(lab)[None]
    before = metrics.predict_and_score(fe, cl, torch.zeros(1, 3, 12, 15), y, num_classes=K)
    for _ in range(2):
        r = metrics.predict_and_score(fe, cl, torch.zeros(1, 3, 12, 15), y, num_classes=K, curves=(pr, cal))
    assert torch.equal(r.cmt, before.cmt) and torch.equal(r.pred, before.pred)
    # softmax(log p) is p up to rounding: the reference is literal_curves on the map inference() returns
    want = metrics.literal_curves(metrics.inference(fe, cl, torch.zeros(1, 3, 12, 15), y, flip=False), y, K, 15)
    assert torch.equal(pr, 2 * want[0]) and torch.equal(cal, 2 * want[1]) and int(pr.sum()) > 0


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entries_are_exported_declared_and_in_the_table(built):
    header = open(_lib.HEADER_PATH).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("mi_upsample_curves", 12), ("mi_upsample_curves_slide", 14)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(h, name)
        assert "int %s(" % name in header
    assert "upsample_curves.hip" in entry.SOURCES


def test_entries_refuse_before_any_launch(built):
    one = ctypes.c_void_p(16)                     # non-null, 16-byte aligned dummy: validation fails before it is dereferenced
    src = (_lib.MiProbSource * 17)()
    for s in src:
        s.low, s.h, s.w, s.mirror = 16, 5, 7, 0
    sp = ctypes.cast(src, ctypes.c_void_p)

    def multi(n=1, K=19, H=33, W=33, labels=one, bins=15, pr=one, cal=one, src=sp, div_a=1.0, div_b=1.0):
        return built.mi_upsample_curves(src, n, K, H, W, div_a, div_b, labels, bins, pr, cal, None)

    def windows(specs):
        win = (_lib.MiSlideWindow * max(1, len(specs)))()
        for w, (low, mirror, y0, x0) in zip(win, specs):
            w.low, w.low_mirror, w.y0, w.x0 = low, mirror, y0, x0
        return ctypes.cast(win, ctypes.c_void_p)

    full = [(16, None, 0, 0), (16, None, 0, 10), (16, None, 10, 0), (16, None, 10, 10)]

    def slide(specs=full, n=None, K=19, wh=20, ww=20, H=30, W=30, labels=one, bins=15, pr=one, cal=one, win=True):
        return built.mi_upsample_curves_slide(windows(specs) if win else None, len(specs) if n is None else n, 5, 5, wh, ww, K, H, W, labels, bins,
                                              pr, cal, None)

    def refused(call, needle, **kw):
        assert call(**kw) == -22
        assert needle in built.mi_last_error(), built.mi_last_error()

    # what mi_upsample_predict_score refuses about its sources
    refused(multi, b"1 <= n <= 16", n=0)
    refused(multi, b"1 <= n <= 16", n=17)
    refused(multi, b"K <= 32", K=0)
    refused(multi, b"K <= 32", K=33)
    refused(multi, b"bad dimension", H=0)
    refused(multi, b"null operand", src=None)
    refused(multi, b"zero divisor", div_a=0.0)
    refused(multi, b"zero divisor", div_b=0.0)
    bad = (_lib.MiProbSource * 1)()
    bad[0].low, bad[0].h, bad[0].w = 16, 0, 7
    refused(multi, b"bad source", src=ctypes.cast(bad, ctypes.c_void_p))
    # what mi_upsample_predict_score_slide refuses about its windows, the cover check included
    refused(slide, b"null operand", win=False)
    refused(slide, b"1 <= n <= 64", specs=[], n=0)
    refused(slide, b"1 <= n <= 64", specs=full * 17, n=65)
    refused(slide, b"K <= 32", K=33)
    refused(slide, b"only upsampling", wh=4)
    refused(slide, b"leaves the 30 x 30", specs=full[:3] + [(16, None, 11, 10)])
    refused(slide, b"leaves the 30 x 30", wh=31)
    refused(slide, b"mirror maps on some windows only", specs=full[:3] + [(16, 16, 10, 10)])
    refused(slide, b"no window covers", specs=full[:3])
    # the entries' own
    for call in (multi, slide):
        refused(call, b"null labels", labels=None)
        refused(call, b"neither pr nor cal", pr=None, cal=None)
        refused(call, b"ece_bins", bins=0)
        refused(call, b"ece_bins", bins=65)
        refused(call, b"ece_bins", bins=-1, pr=None)
    refused(multi, b"reaches 2^31", H=46341, W=46341)
    refused(slide, b"reaches 2^31", specs=full[:1], wh=46341, ww=46341, H=46341, W=46341)
