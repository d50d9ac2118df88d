"""Host side of the polyp metrics (TEST.POLYP_METRICS), no GPU: host/metrics.py polyp_image_stats - which sees only a 2 x 256 histogram and the
per-quadrant moment sums - against the literal float64 evaluation of tests/_polyp_ref.py on the arrays themselves (two different derivations: this
is the test that protects the formulas), PolypMeter's aggregation and lines, the config key and the testers' refusals, and the C-ABI entry
mi_polyp_score with its refusals before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import _polyp_ref as ref
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


@pytest.fixture(scope="module")
def built():
    entry.build()
    return _lib.lib()


def _blob(H, W, seed):
    """An elliptic ground truth somewhere inside the image."""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = g.uniform(0.3, 0.7) * H, g.uniform(0.3, 0.7) * W
    return ((((yy - cy) / (0.3 * H)) ** 2 + ((xx - cx) / (0.25 * W)) ** 2) < 1).astype(np.int64)


def _random_map(H, W, seed):
    return np.random.RandomState(seed).rand(H, W).astype(np.float32).astype(np.float64)      # fp32 values, as the kernel's map holds


def _near_binary(gt, seed):
    """What a trained net produces: sigmoid of +/-(8 + noise), the sign following the ground truth except in a band of errors."""
    g = np.random.RandomState(seed)
    z = (8.0 + g.randn(*gt.shape)) * np.where(gt == 1, 1.0, -1.0)
    z[:, : gt.shape[1] // 5] *= -1
    p = 1 / (1 + np.exp(-z))
    p = (p - p.min()) / (p.max() - p.min() + 1e-8)
    return p.astype(np.float32).astype(np.float64)


def _cases():
    out = {}
    for (H, W), seed in (((37, 45), 1), ((33, 64), 2)):
        out["random_%dx%d" % (H, W)] = (_random_map(H, W, seed), _blob(H, W, seed))
    H, W = 37, 45
    p = _random_map(H, W, 3)
    out["G_is_0"] = (p, np.zeros((H, W), np.int64))
    out["G_is_N"] = (p, np.ones((H, W), np.int64))
    out["constant_map"] = (np.zeros((H, W)), _blob(H, W, 4))
    last = np.zeros((H, W), np.int64)
    last[5:30, W - 1] = 1
    out["last_column"] = (p, last)                                    # cx == W: both right quadrants are empty
    one = np.zeros((H, W), np.int64)
    one[0, 0] = 1
    out["single_pixel"] = (p, one)                                    # cx == cy == 1: the LT quadrant is one pixel, G == 1
    out["near_binary"] = (_near_binary(_blob(H, W, 5), 5), _blob(H, W, 5))
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_from_counts_equals_the_literal_evaluation(name):
    p, g = CASES[name]
    hist, sums, counts, _ = ref.counted(p, g)
    got = metrics.polyp_image_stats(hist, sums, *g.shape)
    want = ref.reference_metrics(p, g)
    for k in ("dice", "iou", "f", "e"):
        assert got[k].shape == (256,) and np.isfinite(got[k]).all()
        err = np.abs(got[k] - want[k]).max()
        assert err <= RTOL * max(np.abs(want[k]).max(), 1e-300), (name, k, err)
    for k in ("S", "MAE"):
        assert np.isfinite(got[k]) and abs(got[k] - want[k]) <= RTOL * max(abs(want[k]), 1e-300) + (1e-15 if want[k] == 0 else 0), (name, k, got[k], want[k])
    assert metrics.polyp_centre(*counts[:3]) == (int(sums[20]), int(sums[21]))


def test_edge_cases_take_the_branches_they_are_built_for():
    p, g = CASES["last_column"]
    _, sums, _, _ = ref.counted(p, g)
    assert int(sums[20]) == g.shape[1] and sums[5 + 4] == 0 and sums[15 + 4] == 0       # cx == W, nothing right of it
    _, sums, _, _ = ref.counted(*CASES["single_pixel"])
    assert (int(sums[20]), int(sums[21])) == (1, 1) and sums[4] == 1
    hist, _, _, _ = ref.counted(*CASES["near_binary"])
    assert hist[:, [0, 254, 255]].sum() > 0.8 * hist.sum()                              # the mass sits in the end bins (truncation: 254 below the maximum)
    hist, sums, _, _ = ref.counted(*CASES["constant_map"])
    assert hist[:, 1:].sum() == 0
    r = metrics.polyp_image_stats(hist, sums, 37, 45)
    assert r["dice"][1:].max() == 0 and r["dice"][0] > 0                                # an empty prediction above threshold 0
    r0 = metrics.polyp_image_stats(*ref.counted(*CASES["G_is_0"])[:2], 37, 45)
    assert r0["dice"][0] == 0 and r0["S"] == pytest.approx(1 - CASES["G_is_0"][0].mean(), rel=1e-12)
    empty = np.zeros((37, 45))
    r1 = metrics.polyp_image_stats(*ref.counted(empty, np.zeros((37, 45), np.int64))[:2], 37, 45)
    assert r1["dice"][1] == 1 and r1["iou"][1] == 1 and r1["f"][1] == 1                 # prediction and ground truth both empty


def test_image_stats_refuses_inconsistent_input():
    hist, sums, _, _ = ref.counted(*CASES["random_37x45"])
    with pytest.raises(ValueError, match="histogram holds"):
        metrics.polyp_image_stats(hist, sums, 37, 46)
    with pytest.raises(ValueError, match=r"\[2, 256\]"):
        metrics.polyp_image_stats(hist[:, :128], sums, 37, 45)
    with pytest.raises(ValueError, match=r"\[2, 256\]"):
        metrics.polyp_image_stats(hist, sums[:20], 37, 45)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg, *a, **k):
        self.lines.append(str(msg))


def test_polyp_meter_aggregates_three_images():
    names = ["random_37x45", "near_binary", "last_column"]
    meter = metrics.PolypMeter()
    for n in names:
        p, g = CASES[n]
        hist, sums, _, _ = ref.counted(p, g)
        meter.update(metrics.polyp_image_stats(hist, sums, *g.shape))
    want, curves = ref.aggregate([ref.reference_metrics(*CASES[n]) for n in names])
    got = meter.as_dict()
    assert list(got) == list(metrics.POLYP_KEYS) + ["images"] and got["images"] == 3
    for k in metrics.POLYP_KEYS:
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    for k in curves:
        assert np.abs(meter.mean_curves()[k] - curves[k]).max() <= 1e-12
    assert got["maxF"] >= got["meanF"] and got["maxE"] >= got["meanE"]
    log = _Log()
    meter.summary(log)
    assert log.lines == [
        "Polyp metric, val result over 3 images: mDice/mIoU {:.4f}/{:.4f}.".format(want["mDice"], want["mIoU"]),
        "Polyp metric, val result: meanF/maxF {:.4f}/{:.4f}, S-measure {:.4f}.".format(want["meanF"], want["maxF"], want["S"]),
        "Polyp metric, val result: meanE/maxE {:.4f}/{:.4f}, MAE {:.4f}.".format(want["meanE"], want["maxE"], want["MAE"]),
    ]
    meter.reset()
    assert meter.count == 0 and meter.as_dict()["images"] == 0


# ------------------------------------------------------------------------------------------------ configuration and testers
def _cfg(tmp_path, *opts):
    from core.configs import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path)] + list(opts))
    return cfg


def test_config_key_default_merge_and_type_check(tmp_path):
    from core.configs import cfg as global_cfg
    assert global_cfg.TEST.POLYP_METRICS is False and metrics.polyp_settings(global_cfg) is False
    assert metrics.polyp_settings(_cfg(tmp_path, "TEST.POLYP_METRICS", "True")) is True          # test.py's trailing KEY VAL list
    assert metrics.polyp_settings(_cfg(tmp_path, "TEST.POLYP_METRICS", True)) is True
    for bad in ("1", 1, "yes", 0.5):
        with pytest.raises(ValueError, match="Type mismatch"):
            _cfg(tmp_path, "TEST.POLYP_METRICS", bad)
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "pranet_test_kvasir_polyp.yaml"))
    assert cfg.TEST.POLYP_METRICS is True and cfg.DATASETS.TEST == "polyp_val" and cfg.MODEL.NUM_CLASSES == 2 and cfg.AUG.NAME == "pra"
    base = global_cfg.clone()
    base.defrost()
    base.merge_from_file(os.path.join(ROOT, "configs", "pranet_src_kvasir.yaml"))
    cfg.TEST.POLYP_METRICS = False
    assert cfg == base                                                # the Kvasir configuration with the key on, nothing else
    bare = type("C", (), {"TEST": {}})()                              # a cfg without the key (an older tree): off
    assert metrics.polyp_settings(bare) is False


def test_testers_refuse_or_accept_the_key(tmp_path):
    from core.testers.aspp_tester import ASPPTester
    from core.testers.gald_tester import GALDTester
    from core.testers.pranet_tester import PranetTester
    logger = _Log()
    on = _cfg(tmp_path, "TEST.POLYP_METRICS", True)
    with pytest.raises(NotImplementedError, match="POLYP_METRICS"):
        ASPPTester(on, torch.device("cpu"), [], logger, [0] * 57, {})
    with pytest.raises(NotImplementedError, match="POLYP_METRICS"):
        GALDTester(on, torch.device("cpu"), [], logger, [0] * 57)
    t = PranetTester(on, torch.device("cpu"), [], logger)
    assert t.model is not None and t.polyp_metrics is True
    t = PranetTester(_cfg(tmp_path), torch.device("cpu"), [], logger)
    assert t.model is not None and t.polyp_metrics is False
    # the keys PranetTester refuses stay refused with the key on
    for opts, needle in ((("TEST.SCALES", "(0.7, 1.0)"), "SCALES"), (("TEST.FLIP", True), "FLIP"), (("TEST.PSEUDO_THRESHOLD", 0.5), "PSEUDO_THRESHOLD"),
                         (("TEST.PSEUDO_CLASSWISE", True), "PSEUDO_CLASSWISE")):
        with pytest.raises(NotImplementedError, match=needle):
            PranetTester(_cfg(tmp_path, "TEST.POLYP_METRICS", True, *opts), torch.device("cpu"), [], logger)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entries_are_declared_exported_and_built(built):
    header = open(_lib.HEADER_PATH).read()
    for name, nargs in (("mi_polyp_score", 15), ("mi_polyp_score_workspace", 5)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert name + "(" in header
    assert _lib.SIGNATURES["mi_polyp_score_workspace"][0] is ctypes.c_size_t and _lib.SIGNATURES["mi_polyp_score"][0] is ctypes.c_int
    assert "polyp_score.hip" in entry.SOURCES
    assert "#define MI_POLYP_SUMS 24" in header and "#define MI_POLYP_COUNTS 4" in header
    from rnd_semantic_segmentation_amd import kernels
    assert (kernels.POLYP_SUMS, kernels.POLYP_COUNTS) == (24, 4)


def test_entry_refuses_bad_arguments_before_any_launch(built):
    one = ctypes.c_void_p(16)                     # non-null, aligned dummy: validation fails before it is dereferenced
    big = 1 << 40

    def call(low=one, labels=one, B=2, h=11, w=13, H=37, W=45, hist=one, sums=one, counts=one, prob=None, pred=None, ws=one, ws_bytes=big):
        return built.mi_polyp_score(low, labels, B, h, w, H, W, hist, sums, counts, prob, pred, ws, ws_bytes, None)

    def refused(needle, **kw):
        assert call(**kw) == -22
        err = built.mi_last_error()
        assert needle in err and b"mi_polyp_score" in err, err

    for k in ("low", "labels", "hist", "sums", "counts", "ws"):
        refused(b"null operand", **{k: None})
    for k in ("B", "h", "w", "H", "W"):
        refused(b"bad dimension", **{k: 0})
        refused(b"bad dimension", **{k: -3})
    need = built.mi_polyp_score_workspace(2, 11, 13, 37, 45)
    assert need > 0 and built.mi_polyp_score_workspace(0, 11, 13, 37, 45) == 0
    refused(b"workspace too small", ws_bytes=need - 1)
    refused(b"workspace too small", ws_bytes=0)
    refused(b"index arithmetic", B=70000)
    refused(b"index arithmetic", H=(1 << 20) + 1)
    refused(b"index arithmetic", B=4096, H=1 << 20, W=1 << 20)
    # the workspace grows with the label size and the batch, not with the map
    assert built.mi_polyp_score_workspace(16, 352, 352, 1072, 1920) > built.mi_polyp_score_workspace(1, 352, 352, 352, 352)
    assert built.mi_polyp_score_workspace(2, 11, 13, 37, 45) == built.mi_polyp_score_workspace(2, 24, 24, 37, 45)


def test_wrapper_has_no_cpu_path():
    from rnd_semantic_segmentation_amd import kernels
    with pytest.raises(_lib.MiError, match="GPU"):
        kernels.polyp_score(torch.zeros(1, 4, 4), torch.zeros(1, 8, 8, dtype=torch.int64))
