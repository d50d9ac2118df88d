"""Host side of the lesion-wise metrics and the mask clean-up (TEST.LESION_METRICS, TEST.MASK_MIN_AREA, TEST.MASK_KEEP_LARGEST), no GPU: the
raster flood fill of tests/_components_ref.py against scipy.ndimage.label (an outside implementation) on the GPU test's cases at both
connectivities, host/metrics.py lesion_image_stats and LesionMeter on hand-computed integers, the config keys, the YAML file and the testers'
refusals, the torch-op composition literal_lesion_stats against the flood fill on the CPU, and the C-ABI entries mi_label_components and
mi_lesion_score with their refusals before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import _components_ref as ref
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL_CASES = ref.label_cases()
LESION_CASES = ref.lesion_cases()


@pytest.fixture(scope="module")
def built():
    entry.build()
    return _lib.lib()


class _Log(object):
    def __init__(self):
        self.lines = []

    def info(self, msg, *a, **k):
        self.lines.append(str(msg))


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("name", sorted(LABEL_CASES))
def test_flood_fill_against_scipy(name, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    m = LABEL_CASES[name] == 1
    want, n = ndi.label(m, structure=ndi.generate_binary_structure(2, 1 if connectivity == 4 else 2))
    labels, roots, count = ref.label(m, connectivity)
    assert count == n and np.array_equal(labels, want)
    assert ((roots == -1) == ~m).all()
    for k in range(1, n + 1):                                          # the root is the component's first pixel in raster order
        assert (roots[labels == k] == np.flatnonzero(labels.ravel() == k)[0]).all()
    firsts = [np.flatnonzero(labels.ravel() == k)[0] for k in range(1, n + 1)]
    assert firsts == sorted(firsts)


def test_the_cases_are_what_their_names_say():
    assert ref.spiral(33, 64)[1] >= 8 and ref.label(LABEL_CASES["spiral_33x64"] == 1, 4)[2] == 1
    assert ref.label(LABEL_CASES["u_shape_6x9"] == 1, 8)[2] == 3 and ref.label(LABEL_CASES["u_shape_6x9"] == 1, 4)[2] == 4
    assert ref.label(LABEL_CASES["checker_37x45"] == 1, 4)[2] == 833 and ref.label(LABEL_CASES["checker_37x45"] == 1, 8)[2] == 1
    assert ref.label(LABEL_CASES["comb_40x130"] == 1, 4)[2] == 1
    assert ref.label(LABEL_CASES["frame_in_frame_37x45"] == 1, 4)[2] == 4 == ref.label(LABEL_CASES["frame_in_frame_37x45"] == 1, 8)[2]
    assert ref.label(LABEL_CASES["speckle_37x45"] == 1, 4)[2] > 30
    labels, _, n = ref.label(LABEL_CASES["blobs_200x517"] == 1, 8)
    assert n > 100 and np.bincount(labels.ravel())[1:].max() > 5000
    for name, (p, g) in LESION_CASES.items():
        assert p.dtype == np.uint8 and g.dtype == np.int64 and p.shape == g.shape == (37, 80) and (p == 1).any() and (g == 1).any(), name


def test_reference_integers_by_hand():
    """The `tie` case: components of 24, 24 and 10 pixels; the label is the prediction moved two pixels to the right."""
    p, g = LESION_CASES["tie"]
    ints, f = ref.reference(p, g, 1, 8, 0, False, 0)
    assert ints.tolist() == [58, 58, 58, 3, 3, 3, 3, 3, 24, 24, 4 * 4 + 6 * 2 + 8, 0] and np.array_equal(f, p)
    ints, f = ref.reference(p, g, 1, 8, 11, False, 0)
    assert ints.tolist() == [58, 48, 58, 3, 2, 3, 2, 2, 24, 24, 28, 1]
    ints, f = ref.reference(p, g, 1, 8, 0, True, 0)
    assert ints.tolist() == [58, 24, 58, 3, 1, 3, 1, 1, 24, 24, 16, 2] and f[4:8, 60:66].all() and f.sum() == 24
    assert ref.reference(p, g, 1, 8, 0, False, 667)[0][6:8].tolist() == [1, 1]      # 16/24 and 12/24 miss two thirds, 8/10 passes
    assert ref.reference(p, g, 1, 8, 0, False, 666)[0][6:8].tolist() == [2, 2]
    assert ref.reference(p, g, 0, 8, 0, False, 0)[1].max() == 1                      # cls 0: the other value is 1


# ------------------------------------------------------------------------------------------------ statistics and the meter
def test_lesion_image_stats_and_refusals():
    s = metrics.lesion_image_stats([353, 305, 680, 5, 1, 2, 1, 1, 305, 387, 293, 4])
    assert s == {"pred_pixels": 353, "kept_pixels": 305, "lesion_pixels": 680, "pred_components": 5, "kept_components": 1, "lesions": 2,
                 "true_positives": 1, "detected": 1, "largest_pred": 305, "largest_lesion": 387, "overlap_pixels": 293, "removed_components": 4,
                 "false_positives": 0, "missed": 1}
    assert metrics.lesion_image_stats(torch.tensor([0] * 12))["missed"] == 0
    assert len(metrics.LESION_FIELDS) == metrics.LESION_INTS == ref.INTS == 12
    with pytest.raises(ValueError, match=r"\[12\]"):
        metrics.lesion_image_stats([0] * 11)
    for bad in ([3, 3, 3, 2, 1, 1, 1, 1, 2, 3, 1, 0],                  # removed != components - kept
                [3, 3, 3, 2, 2, 1, 3, 1, 2, 3, 1, 0],                  # more true positives than components
                [3, 3, 3, 2, 2, 1, 1, 2, 2, 3, 1, 0],                  # more detected than lesions
                [3, 4, 3, 2, 2, 1, 1, 1, 2, 3, 1, 0],                  # kept pixels above the prediction's
                [3, 3, 3, 2, 2, 1, 1, 1, 2, 3, -1, 0]):
        with pytest.raises(ValueError, match="contradict"):
            metrics.lesion_image_stats(bad)


def test_lesion_meter_sums_ratios_and_nones():
    meter = metrics.LesionMeter()
    empty = meter.as_dict()
    assert empty["images"] == 0 and empty["lesion_recall"] is None and empty["component_precision"] is None and empty["lesion_f1"] is None
    assert empty["false_positives_per_image"] is None
    rows = ([100, 90, 80, 4, 3, 2, 2, 1, 50, 60, 40, 1],               # 3 kept: 2 true, 1 false; 2 lesions, 1 detected; 10 pixels removed
            [30, 30, 0, 2, 2, 0, 0, 0, 20, 0, 0, 0],                   # no lesion, two predictions: a false alarm image
            [0, 0, 50, 0, 0, 1, 0, 0, 0, 50, 0, 0],                    # a lesion, no prediction: a missed image
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    for r in rows:
        meter.update(metrics.lesion_image_stats(r))
    d = meter.as_dict()
    assert (d["images"], d["lesions"], d["detected"], d["kept_components"], d["true_positives"], d["false_positives"]) == (4, 3, 1, 5, 2, 3)
    assert d["lesion_recall"] == 1 / 3 and d["component_precision"] == 2 / 5 and d["false_positives_per_image"] == 3 / 4
    assert abs(d["lesion_f1"] - 2 * (1 / 3) * (2 / 5) / (1 / 3 + 2 / 5)) < 1e-15
    assert (d["images_missed"], d["images_false_alarm"], d["removed_components"], d["removed_pixels"]) == (1, 1, 1, 10)
    log = _Log()
    meter.summary(log)
    assert len(log.lines) == 2 and log.lines[0].startswith("Lesion metric, val result over 4 images: recall 0.3333 (1/3 lesions), precision 0.4000 (2/5")
    assert "false positives per image 0.7500, images missed 1, false alarms 1, removed components 1" in log.lines[1]
    only_missed = metrics.LesionMeter()                                # recall 0, no component at all: precision and F1 have no value
    only_missed.update(metrics.lesion_image_stats(rows[2]))
    d = only_missed.as_dict()
    assert d["lesion_recall"] == 0.0 and d["component_precision"] is None and d["lesion_f1"] is None and d["false_positives_per_image"] == 0.0
    zero = metrics.LesionMeter()                                       # recall 0 and precision 0: F1 has no value either
    zero.update(metrics.lesion_image_stats([5, 5, 5, 1, 1, 1, 0, 0, 5, 5, 0, 0]))
    assert zero.as_dict()["lesion_f1"] is None and zero.as_dict()["component_precision"] == 0.0
    only_missed.summary(log)
    assert "precision n/a" in log.lines[2] and "F1 n/a" in log.lines[2]
    meter.reset()
    assert meter.as_dict() == empty


# ------------------------------------------------------------------------------------------------ configuration and testers
def _cfg(tmp_path, *opts):
    from core.configs import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path)] + list(opts))
    return cfg


def test_config_keys_defaults_activation_and_validation(tmp_path):
    from core.configs import cfg as global_cfg
    t = global_cfg.TEST
    assert (t.LESION_METRICS, t.LESION_CONNECTIVITY, t.LESION_OVERLAP, t.MASK_MIN_AREA, t.MASK_KEEP_LARGEST) == (False, 8, 0.0, 0, False)
    assert metrics.lesion_settings(global_cfg) is None
    assert metrics.lesion_settings(_cfg(tmp_path, "TEST.LESION_CONNECTIVITY", 4, "TEST.LESION_OVERLAP", 0.5)) is None      # nothing switched on
    assert metrics.lesion_settings(_cfg(tmp_path, "TEST.LESION_METRICS", "True")) == (True, 8, 0.0, 0, False)
    assert metrics.lesion_settings(_cfg(tmp_path, "TEST.MASK_MIN_AREA", 64)) == (False, 8, 0.0, 64, False)
    assert metrics.lesion_settings(_cfg(tmp_path, "TEST.MASK_KEEP_LARGEST", True)) == (False, 8, 0.0, 0, True)
    assert metrics.lesion_settings(_cfg(tmp_path, "TEST.LESION_METRICS", True, "TEST.LESION_CONNECTIVITY", 4, "TEST.LESION_OVERLAP", 0.25,
                                        "TEST.MASK_MIN_AREA", 9, "TEST.MASK_KEEP_LARGEST", True)) == (True, 4, 0.25, 9, True)
    for key, bad in (("LESION_METRICS", 1), ("MASK_KEEP_LARGEST", "yes"), ("LESION_CONNECTIVITY", 8.0), ("MASK_MIN_AREA", 2.5)):
        with pytest.raises(ValueError, match="Type mismatch"):
            _cfg(tmp_path, "TEST." + key, bad)
    for key, bad in (("LESION_CONNECTIVITY", 6), ("LESION_CONNECTIVITY", 0), ("LESION_OVERLAP", 1.5), ("LESION_OVERLAP", -0.1), ("MASK_MIN_AREA", -1)):
        with pytest.raises(ValueError, match="TEST." + key):
            metrics.lesion_settings(_cfg(tmp_path, "TEST." + key, bad))
    bare = type("C", (), {"TEST": {}})()                              # a cfg without the keys (an older tree): off
    assert metrics.lesion_settings(bare) is None
    half = type("C", (), {"TEST": {"MASK_MIN_AREA": 5}})()
    assert metrics.lesion_settings(half) == (False, 8, 0.0, 5, False)
    for key, bad in (("LESION_METRICS", 1), ("LESION_CONNECTIVITY", True), ("LESION_OVERLAP", "0.5"), ("MASK_MIN_AREA", 2.0), ("MASK_KEEP_LARGEST", 1)):
        with pytest.raises(ValueError, match="TEST." + key):
            metrics.lesion_settings(type("C", (), {"TEST": {key: bad}})())


def test_yaml_file(tmp_path):
    from core.configs import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "pranet_test_kvasir_lesion.yaml"))
    assert metrics.lesion_settings(cfg) == (True, 8, 0.0, 64, False)
    assert metrics.surface_settings(cfg) == (95, (2.0,)) and cfg.TEST.POLYP_METRICS is True
    base = global_cfg.clone()
    base.defrost()
    base.merge_from_file(os.path.join(ROOT, "configs", "pranet_test_kvasir_surface.yaml"))
    cfg.TEST.LESION_METRICS, cfg.TEST.MASK_MIN_AREA = False, 0
    assert cfg == base                                                # the surface test configuration with the two keys, nothing else


def test_testers_refuse_or_accept_the_keys(tmp_path):
    from core.testers.aspp_tester import ASPPTester
    from core.testers.gald_tester import GALDTester
    from core.testers.pranet_tester import PranetTester
    logger = _Log()
    for opts in (("TEST.LESION_METRICS", True), ("TEST.MASK_MIN_AREA", 3), ("TEST.MASK_KEEP_LARGEST", True)):
        on = _cfg(tmp_path, *opts)
        with pytest.raises(NotImplementedError, match="LESION_METRICS"):
            ASPPTester(on, torch.device("cpu"), [], logger, [0] * 57, {})
        with pytest.raises(NotImplementedError, match="LESION_METRICS"):
            GALDTester(on, torch.device("cpu"), [], logger, [0] * 57)
        with pytest.raises(NotImplementedError, match="someone"):
            metrics.require_no_lesion(on, "someone")
    metrics.require_no_lesion(_cfg(tmp_path), "anyone")
    t = PranetTester(_cfg(tmp_path, "TEST.LESION_METRICS", True, "TEST.MASK_MIN_AREA", 64), torch.device("cpu"), [], logger)
    assert t.lesion == (True, 8, 0.0, 64, False) and t.surface is None
    assert PranetTester(_cfg(tmp_path), torch.device("cpu"), [], logger).lesion is None
    with pytest.raises(ValueError, match="LESION_CONNECTIVITY"):
        PranetTester(_cfg(tmp_path, "TEST.LESION_CONNECTIVITY", 5), torch.device("cpu"), [], logger)


# ------------------------------------------------------------------------------------------------ the literal composition
@pytest.mark.parametrize("name", sorted(LESION_CASES))
def test_literal_composition_against_the_flood_fill(name):
    p, g = LESION_CASES[name]
    for connectivity, min_area, keep_largest, overlap in ((8, 0, False, 0.0), (4, 0, False, 0.5), (8, 12, False, 0.001), (4, 2, True, 1.0),
                                                          (8, 10 ** 6, True, 0.0)):
        want_ints, want_f = ref.reference(p, g, 1, connectivity, min_area, keep_largest, int(round(1000 * overlap)))
        ints, f = metrics.literal_lesion_stats(torch.from_numpy(p), torch.from_numpy(g), 1, connectivity, min_area, keep_largest, overlap)
        assert ints == want_ints.tolist(), (name, connectivity, min_area, keep_largest, overlap)
        assert f.dtype == torch.uint8 and np.array_equal(f.numpy(), want_f)


def test_literal_composition_on_the_label_cases():
    """Roots through the composition: the spiral needs as many rounds as it has pixels, the comb joins at the bottom."""
    for name in ("spiral_33x64", "comb_40x130", "u_shape_6x9", "checker_37x45", "empty_9x70"):
        m = LABEL_CASES[name]
        for connectivity in (4, 8):
            want_ints, want_f = ref.reference(m, m.astype(np.int64), 1, connectivity, 2, False, 1000)
            ints, f = metrics.literal_lesion_stats(torch.from_numpy(m), torch.from_numpy(m.astype(np.int64)), 1, connectivity, 2, False, 1.0)
            assert ints == want_ints.tolist() and np.array_equal(f.numpy(), want_f), (name, connectivity)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.literal_lesion_stats(torch.zeros(2, 2, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int64), connectivity=6)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entries_are_declared_exported_and_built(built):
    header = open(_lib.HEADER_PATH).read()
    for name, nargs in (("mi_label_components", 12), ("mi_label_components_workspace", 3), ("mi_lesion_score", 15), ("mi_lesion_score_workspace", 3)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert name + "(" in header
        assert _lib.SIGNATURES[name][0] is (ctypes.c_size_t if name.endswith("_workspace") else ctypes.c_int)
    assert "components.hip" in entry.SOURCES and "#define MI_LESION_INTS 12" in header
    from rnd_semantic_segmentation_amd import kernels
    assert kernels.LESION_INTS == 12
    assert [kernels.lesion_permille(v) for v in (0.0, 0.001, 0.0004, 0.5, 0.9996, 1.0)] == [0, 1, 0, 500, 1000, 1000]


def test_label_entry_refuses_bad_arguments_before_any_launch(built):
    one = ctypes.c_void_p(16)                     # non-null, aligned dummy: validation fails before it is dereferenced
    big = 1 << 40

    def call(mask=one, B=2, H=37, W=45, cls=1, connectivity=8, labels=one, roots=one, counts=one, ws=one, ws_bytes=big):
        return built.mi_label_components(mask, B, H, W, cls, connectivity, labels, roots, counts, ws, ws_bytes, None)

    def refused(needle, code=-22, **kw):
        assert call(**kw) == code
        err = built.mi_last_error()
        assert needle in err and b"mi_label_components" in err, err

    for k in ("mask", "counts", "ws"):
        refused(b"null operand", **{k: None})
    refused(b"both NULL", labels=None, roots=None)
    for k in ("B", "H", "W"):
        refused(b"bad dimension", **{k: 0})
        refused(b"bad dimension", **{k: -3})
    refused(b"beyond the limits", B=65536)
    refused(b"beyond the limits", H=4097)
    refused(b"beyond the limits", W=4097)
    for cls in (-1, 256):
        refused(b"cls", cls=cls)
    for c in (0, 6, -8, 16):
        refused(b"connectivity", connectivity=c)
    refused(b"8-byte aligned", ws=ctypes.c_void_p(20))
    need = built.mi_label_components_workspace(2, 37, 45)
    assert need >= 2 * 37 * 45 * 8
    for size in ((0, 37, 45), (2, 0, 45), (2, 37, -1), (65536, 37, 45), (2, 4097, 45), (2, 37, 4097)):
        assert built.mi_label_components_workspace(*size) == 0
    assert built.mi_label_components_workspace(65535, 1, 1) > 0 and built.mi_label_components_workspace(1, 4096, 4096) >= 8 * 4096 * 4096
    refused(b"workspace too small", code=-12, ws_bytes=need - 1)
    refused(b"workspace too small", code=-12, ws_bytes=0)


def test_lesion_entry_refuses_bad_arguments_before_any_launch(built):
    one = ctypes.c_void_p(16)
    big = 1 << 40

    def call(pred=one, labels=one, B=2, H=37, W=45, cls=1, connectivity=8, min_area=0, keep_largest=0, permille=0, filtered=one, ints=one, ws=one,
             ws_bytes=big):
        return built.mi_lesion_score(pred, labels, B, H, W, cls, connectivity, min_area, keep_largest, permille, filtered, ints, ws, ws_bytes, None)

    def refused(needle, code=-22, **kw):
        assert call(**kw) == code
        err = built.mi_last_error()
        assert needle in err and b"mi_lesion_score" in err, err

    for k in ("pred", "labels", "ints", "ws"):
        refused(b"null operand", **{k: None})
    for k in ("B", "H", "W"):
        refused(b"bad dimension", **{k: 0})
        refused(b"bad dimension", **{k: -3})
    refused(b"beyond the limits", B=65536)
    refused(b"beyond the limits", H=4097)
    refused(b"beyond the limits", W=4097)
    for cls in (-1, 256):
        refused(b"cls", cls=cls)
    for c in (0, 6, -4):
        refused(b"connectivity", connectivity=c)
    refused(b"min_area", min_area=-1)
    for k in (-1, 2):
        refused(b"keep_largest", keep_largest=k)
    for t in (-1, 1001):
        refused(b"overlap_permille", permille=t)
    refused(b"8-byte aligned", ws=ctypes.c_void_p(20))
    need = built.mi_lesion_score_workspace(2, 37, 45)
    assert need >= 2 * 37 * 45 * 24
    for size in ((0, 37, 45), (2, 0, 45), (2, 37, -1), (65536, 37, 45), (2, 4097, 45), (2, 37, 4097)):
        assert built.mi_lesion_score_workspace(*size) == 0
    assert built.mi_lesion_score_workspace(65535, 1, 1) > 0 and built.mi_lesion_score_workspace(1, 4096, 4096) >= 24 * 4096 * 4096
    refused(b"workspace too small", code=-12, ws_bytes=need - 1)
    refused(b"workspace too small", code=-12, ws_bytes=0)
    assert built.mi_lesion_score_workspace(16, 1072, 1920) > built.mi_lesion_score_workspace(1, 352, 352)


def test_wrappers_have_no_cpu_path():
    from rnd_semantic_segmentation_amd import kernels
    with pytest.raises(_lib.MiError, match="GPU"):
        kernels.lesion_score(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(_lib.MiError, match="GPU"):
        kernels.label_components(torch.zeros(1, 4, 4, dtype=torch.uint8))
