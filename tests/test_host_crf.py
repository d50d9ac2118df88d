"""Host side of the CRF refinement (TEST.CRF), no GPU: the torch restatement of tests/_crf_ref.py against the definition written as a per-pixel
double loop, the TEST.CRF* keys with every refusal and the stray-key rule, the other testers' refusal, the channel scale, the shipped
configuration, and the C-ABI entries mi_crf_workspace / mi_crf_refine: declared, exported, in the ctypes table, refusing before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import _crf_ref as ref
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = (58.395, 57.12, 57.375)


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


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("window,dilation,iters", [(3, 1, 2), (5, 2, 3), (7, 4, 1), (3, 6, 2)])
def test_restatement_equals_the_per_pixel_definition(window, dilation, iters):
    probs, image = ref.crf_inputs(3, 1, 6, 7, seed=window * 10 + dilation)
    par = dict(ref.DEFAULTS, window=window, dilation=dilation, iters=iters)
    got = ref.crf_ref(probs, image, CS, dtype=torch.float64, **par)[0].numpy()
    want = ref.crf_brute(probs[0].numpy(), image[0].numpy(), CS, **par)
    assert got.shape == want.shape == (3, 6, 7)
    assert np.abs(got - want).max() < 1e-13, np.abs(got - want).max()
    assert np.abs(got.sum(0) - 1).max() < 1e-13
    moved = (got.argmax(0) != probs[0].numpy().argmax(0)).mean()
    print("6 x 7, window %d dilation %d: the CRF moves %.0f %% of the pixels" % (window, dilation, 100 * moved))


def test_restatement_edge_cases():
    probs, image = ref.crf_inputs(5, 1, 1, 1, seed=3)
    U = torch.log(torch.clamp(probs.double(), min=ref.EPS))
    assert torch.equal(ref.crf_ref(probs, image, CS, dtype=torch.float64, **dict(ref.DEFAULTS, window=3, dilation=1, iters=2)), torch.softmax(U, 1))
    probs, image = ref.crf_inputs(4, 2, 9, 11, seed=4)
    assert torch.equal(ref.crf_ref(probs, image, CS, dtype=torch.float64, **dict(ref.DEFAULTS, iters=0)),
                       torch.softmax(torch.log(torch.clamp(probs.double(), min=ref.EPS)), 1))
    hard = torch.zeros(1, 3, 4, 5)
    hard[:, 1] = 1.0                                                 # exact zeros and ones: the eps clamp keeps everything finite
    out = ref.crf_ref(hard, torch.zeros(1, 3, 4, 5), CS, dtype=torch.float32, **ref.DEFAULTS)
    assert bool(torch.isfinite(out).all()) and bool((out.argmax(1) == 1).all())
    f32 = ref.crf_ref(probs, image, CS, dtype=torch.float32, **ref.DEFAULTS)
    f64 = ref.crf_ref(probs, image, CS, dtype=torch.float64, **ref.DEFAULTS)
    assert f32.dtype == torch.float32 and 0 < float((f32.double() - f64).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ configuration
def test_config_keys_defaults_and_settings(tmp_path):
    from core.configs import cfg as global_cfg
    t = global_cfg.TEST
    assert t.CRF is False and (t.CRF_ITER, t.CRF_WINDOW, t.CRF_DILATION) == (5, 7, 4)
    assert (t.CRF_POS_W, t.CRF_POS_XY, t.CRF_BI_W, t.CRF_BI_XY, t.CRF_BI_RGB) == (3.0, 3.0, 10.0, 80.0, 13.0)
    assert metrics.crf_settings(global_cfg) is None
    assert metrics.crf_settings(_cfg(tmp_path, "TEST.CRF", "True")) == ref.DEFAULTS          # test.py's trailing KEY VAL list
    got = metrics.crf_settings(_cfg(tmp_path, "TEST.CRF", True, "TEST.CRF_ITER", 0, "TEST.CRF_WINDOW", 11, "TEST.CRF_DILATION", 16, "TEST.CRF_POS_W", 0,
                                    "TEST.CRF_BI_RGB", "5"))
    assert got == dict(ref.DEFAULTS, iters=0, window=11, dilation=16, pos_w=0.0, bi_rgb=5.0) and isinstance(got["bi_rgb"], float)
    bare = type("C", (), {"TEST": {}})()                                                     # an older tree: the defaults
    assert metrics.crf_settings(bare) is None
    with pytest.raises(ValueError):
        _cfg(tmp_path, "TEST.CRF", "1")
    with pytest.raises(ValueError):
        _cfg(tmp_path, "TEST.CRF_ITER", 2.5)


@pytest.mark.parametrize("key,bad", [
    ("CRF_ITER", -1), ("CRF_ITER", 33), ("CRF_WINDOW", 4), ("CRF_WINDOW", 1), ("CRF_WINDOW", 13), ("CRF_DILATION", 0), ("CRF_DILATION", 17),
    ("CRF_POS_XY", 0.0), ("CRF_BI_XY", -1.0), ("CRF_BI_RGB", 0.0), ("CRF_BI_RGB", float("nan")), ("CRF_POS_XY", float("inf")),
    ("CRF_POS_W", -0.5), ("CRF_BI_W", float("inf")), ("CRF_BI_W", float("nan")),
])
def test_settings_refuse_what_the_entry_refuses(tmp_path, key, bad):
    with pytest.raises(ValueError, match=key):
        metrics.crf_settings(_cfg(tmp_path, "TEST.CRF", True, "TEST." + key, bad))


def test_too_many_classes_are_refused(tmp_path):
    with pytest.raises(ValueError, match="NUM_CLASSES"):
        metrics.crf_settings(_cfg(tmp_path, "TEST.CRF", True, "MODEL.NUM_CLASSES", 33))


@pytest.mark.parametrize("key,value", [("CRF_ITER", 3), ("CRF_WINDOW", 5), ("CRF_DILATION", 2), ("CRF_POS_W", 1.0), ("CRF_POS_XY", 2.0),
                                       ("CRF_BI_W", 4.0), ("CRF_BI_XY", 60.0), ("CRF_BI_RGB", 5.0)])
def test_a_stray_key_is_refused(tmp_path, key, value):
    from core.testers.aspp_tester import ASPPTester
    from core.testers.gald_tester import GALDTester
    from core.testers.pranet_tester import PranetTester
    logger = type("L", (), {"info": lambda self, s: None})()
    stray = _cfg(tmp_path, "TEST." + key, value)
    with pytest.raises(NotImplementedError, match=key):
        metrics.crf_settings(stray)
    with pytest.raises(NotImplementedError, match=key):
        metrics.require_no_crf(stray, "AnyTester")
    with pytest.raises(NotImplementedError, match=key):
        ASPPTester(stray, torch.device("cpu"), [], logger, [0] * 57, {}, saveres=False)
    with pytest.raises(NotImplementedError, match=key):
        PranetTester(stray, torch.device("cpu"), [], logger)
    with pytest.raises(NotImplementedError, match=key):
        GALDTester(stray, torch.device("cpu"), [], logger, [0] * 57)


def test_other_testers_refuse_the_key(tmp_path):
    from core.testers.gald_tester import GALDTester
    from core.testers.pranet_tester import PranetTester
    logger = type("L", (), {"info": lambda self, s: None})()
    on = _cfg(tmp_path, "TEST.CRF", True)
    metrics.require_no_crf(_cfg(tmp_path), "AnyTester")
    with pytest.raises(NotImplementedError, match="TEST.CRF"):
        metrics.require_no_crf(on, "AnyTester")
    with pytest.raises(NotImplementedError, match="PranetTester: TEST.CRF"):
        PranetTester(on, torch.device("cpu"), [], logger)
    with pytest.raises(NotImplementedError, match="GALDTester: TEST.CRF"):
        GALDTester(on, torch.device("cpu"), [], logger, [0] * 57)


def test_channel_scale(tmp_path):
    assert metrics.crf_channel_scale(_cfg(tmp_path)) == pytest.approx((0.229 * 255, 0.224 * 255, 0.225 * 255), rel=1e-15)
    bgr = _cfg(tmp_path, "INPUT.TO_BGR255", True, "INPUT.PIXEL_STD", [1.0, 1.0, 1.0], "INPUT.PIXEL_MEAN", [104.0, 116.7, 122.7])
    assert metrics.crf_channel_scale(bgr) == (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="PIXEL_STD"):
        metrics.crf_channel_scale(_cfg(tmp_path, "INPUT.PIXEL_STD", [1.0]))


def test_refinement_has_no_cpu_path(tmp_path):
    with pytest.raises(NotImplementedError, match="GPU"):
        metrics.crf_refine_output(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), (4, 4), CS, dict(ref.DEFAULTS))


def test_shipped_configuration_loads():
    from core.configs import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_pseudo_crf.yaml"))
    assert metrics.crf_settings(cfg) == ref.DEFAULTS and metrics.classwise_settings(cfg) == (True, 0.5, 0.9)
    assert cfg.MODEL.NUM_CLASSES == 19 and cfg.DATASETS.TEST == "cityscapes_train"
    assert "deeplabv2_r101_pseudo_crf.yaml" in open(os.path.join(ROOT, "README.md")).read()


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entries_are_exported_declared_and_in_the_table(built):
    header = open(_lib.HEADER_PATH).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs, ret in (("mi_crf_workspace", 4, "size_t "), ("mi_crf_refine", 23, "int ")):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(h, name)
        assert (ret + name + "(") in header
    assert "crf.hip" in entry.SOURCES
    assert built.mi_crf_workspace(1, 19, 1024, 2048) == 2 * 1024 * 2048 * 20 * 4          # two pixel-major Q buffers, classes padded to 4
    assert built.mi_crf_workspace(2, 3, 5, 7) >= 2 * 2 * 5 * 7 * 4 * 4
    assert built.mi_crf_workspace(1, 33, 8, 8) == 0 and built.mi_crf_workspace(0, 3, 8, 8) == 0


def _refine(lib, **kw):
    one = ctypes.c_void_p(16)                     # non-null, 16-byte aligned dummy: validation fails before it is dereferenced
    a = dict(probs=one, image=one, out=one, pred=None, conf=None, B=1, K=19, H=8, W=8, iters=5, window=7, dilation=4, pos_w=3.0, pos_xy=3.0,
             bi_w=10.0, bi_xy=80.0, bi_rgb=13.0, ws=one, ws_bytes=1 << 40)
    a.update(kw)
    return lib.mi_crf_refine(a["probs"], a["image"], 58.0, 57.0, 57.0, a["out"], a["pred"], a["conf"], a["B"], a["K"], a["H"], a["W"], a["iters"],
                             a["window"], a["dilation"], a["pos_w"], a["pos_xy"], a["bi_w"], a["bi_xy"], a["bi_rgb"], a["ws"], a["ws_bytes"], None)


REFUSALS = [
    (dict(K=0), -22, b"K 0"), (dict(K=33), -22, b"K 33"),
    (dict(window=6), -22, b"window 6"), (dict(window=1), -22, b"window 1"), (dict(window=13), -22, b"window 13"),
    (dict(dilation=0), -22, b"dilation 0"), (dict(dilation=17), -22, b"dilation 17"),
    (dict(iters=-1), -22, b"iters -1"), (dict(iters=33), -22, b"iters 33"),
    (dict(pos_xy=0.0), -22, b"sigma"), (dict(bi_xy=-2.0), -22, b"sigma"), (dict(bi_rgb=float("nan")), -22, b"sigma"),
    (dict(bi_rgb=float("inf")), -22, b"sigma"),
    (dict(pos_w=-1.0), -22, b"weight"), (dict(bi_w=float("inf")), -22, b"weight"), (dict(bi_w=float("nan")), -22, b"weight"),
    (dict(B=2, H=32768, W=32768), -22, b"2^31"), (dict(B=1, H=46341, W=46341), -22, b"2^31"),
    (dict(ws_bytes=2 * 8 * 8 * 20 * 4 - 1), -12, b"workspace too small"),
    (dict(out=None), -22, b"no output"),
    (dict(probs=None), -22, b"null"), (dict(image=None), -22, b"null"), (dict(ws=None), -22, b"null workspace"),
]


@pytest.mark.parametrize("kw,code,text", REFUSALS, ids=[",".join("%s=%s" % kv for kv in r[0].items()) for r in REFUSALS])
def test_entry_refuses_before_any_launch(built, kw, code, text):
    assert _refine(built, **kw) == code and text in built.mi_last_error(), built.mi_last_error()
