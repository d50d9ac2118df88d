"""Host side of sliding-window evaluation (TEST.SLIDE), no GPU: slide_plan against a brute-force enumeration, slide_inference (the literal
composition the kernels are held to) against inference() and a hand-written per-pixel average with a foreign classifier, the label-factor rule,
the TEST.SLIDE* keys and their refusals, and the C-ABI entries' refusals before any launch."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import metrics as M


# ------------------------------------------------------------------------------------------------ slide_plan
def _brute_axis(L, c, s):
    """The issue's rule, written as a walk instead of a closed form: keep stepping by s until a window reaches the end."""
    out, a = [], 0
    while True:
        b = min(a + c, L)
        out.append(max(b - c, 0))
        if b >= L:
            return out
        a += s


SWEEP = [(L, c, s) for L in (1, 2, 5, 7, 12, 13, 31) for c in (1, 2, 3, 5, 8, 13, 40) for s in (1, 2, 3, 5, 8, 13, 40) if s <= c]


def test_plan_equals_a_brute_force_walk_on_a_sweep():
    for (H, ch, sh), (W, cw, sw) in itertools.product(SWEEP[::7], SWEEP[::5]):
        rows, cols = _brute_axis(H, ch, sh), _brute_axis(W, cw, sw)
        if len(rows) * len(cols) > M.SLIDE_MAX_WINDOWS:
            with pytest.raises(ValueError, match="cap of 64"):
                M.slide_plan((H, W), (ch, cw), (sh, sw))
            continue
        got = M.slide_plan((H, W), (ch, cw), (sh, sw))
        assert got == (rows, cols, (min(ch, H), min(cw, W))), ((H, W), (ch, cw), (sh, sw), got)


@pytest.mark.parametrize("L,c,s", SWEEP)
def test_plan_axis_properties(L, c, s):
    n = max(L - c + s - 1, 0) // s + 1
    if n > M.SLIDE_MAX_WINDOWS:
        with pytest.raises(ValueError, match="cap of 64"):
            M.slide_plan((L, 1), (c, 1), (s, 1))
        return
    rows, cols, (wh, ww) = M.slide_plan((L, 1), (c, 1), (s, 1))
    assert cols == [0] and ww == 1 and len(rows) == n and rows == _brute_axis(L, c, s)
    assert wh == min(c, L)                                     # one size for every window
    assert rows[0] == 0 and rows[-1] + wh == L                 # the first starts at 0, the last ends at L
    assert all(0 <= a and a + wh <= L for a in rows)
    cover = np.zeros(L, np.int64)
    for a in rows:
        cover[a:a + wh] += 1                                   # pasting ones
    assert cover.min() >= 1                                    # every pixel covered
    want = np.array([sum(1 for a in rows if a <= p < a + wh) for p in range(L)])
    assert np.array_equal(cover, want)
    if c >= L:
        assert rows == [0]                                     # crop >= size: one window, the whole image


def test_plan_worked_example_and_order():
    rows, cols, window = M.slide_plan((1024, 2048), (769, 769), (513, 513))
    assert rows == [0, 255] and cols == [0, 513, 1026, 1279] and window == (769, 769)
    origins, window, r = M.slide_windows((1024, 2048), (2048, 4096), (769, 769), (513, 513))
    assert r == 2 and window == (769, 769)
    assert origins == [(0, 0), (0, 513), (0, 1026), (0, 1279), (255, 0), (255, 513), (255, 1026), (255, 1279)]      # row-major
    assert M.slide_plan((512, 1024), (769, 2000), (513, 1)) == ([0], [0], (512, 1024))


@pytest.mark.parametrize("crop,stride", [((0, 5), (1, 1)), ((5, -1), (1, 1)), ((5, 5), (0, 1)), ((5, 5), (1, 6)), ((5, 5), (6, 5)), ((5, 5), (1, -2))])
def test_plan_refuses_bad_crop_and_stride(crop, stride):
    with pytest.raises(ValueError):
        M.slide_plan((20, 20), crop, stride)


def test_plan_refuses_more_windows_than_the_cap_and_names_it():
    assert M.SLIDE_MAX_WINDOWS == 64 == _lib.SLIDE_MAX_WINDOWS
    rows, cols, _ = M.slide_plan((8 * 4 + 1, 8 * 4 + 1), (5, 5), (4, 4))
    assert len(rows) == 8 and len(cols) == 8                   # an 8 x 8 grid is allowed
    with pytest.raises(ValueError, match="64"):
        M.slide_plan((8 * 4 + 2, 8 * 4 + 1), (5, 5), (4, 4))   # 9 x 8


@pytest.mark.parametrize("label", [(20, 31), (21, 30), (20, 60), (40, 30), (10, 15), (30, 60)])
def test_label_must_be_a_whole_multiple_of_the_image(label):
    with pytest.raises(ValueError) as e:
        M.slide_label_factor((20, 30), label)
    assert "20 x 30" in str(e.value) and "%d x %d" % label in str(e.value)          # both sizes are printed
    assert M.slide_label_factor((20, 30), (20, 30)) == 1 and M.slide_label_factor((20, 30), (60, 90)) == 3


# ------------------------------------------------------------------------------------------------ slide_inference, foreign classifier on CPU
class _Backbone(torch.nn.Module):
    """A stride-2 feature extractor whose output depends on position inside the window (padding), as a real backbone's does."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv2d(3, 6, 3, stride=2, padding=1)

    def forward(self, x):
        return torch.relu(self.conv(x))


class _Head(torch.nn.Module):
    def __init__(self, K=5):
        super().__init__()
        torch.manual_seed(4)
        self.conv = torch.nn.Conv2d(6, K, 1)

    def forward(self, f):
        return self.conv(f) * 3


@pytest.fixture(scope="module")
def net():
    return _Backbone().eval(), _Head().eval()


def _image(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, H, W, generator=g)                # image 1 is there to be ignored, as inference() ignores it


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("r", [1, 2])
def test_crop_at_least_the_image_is_inference_itself(net, flip, r):
    fe, cls = net
    x = _image(18, 26)
    label = torch.zeros(2, 18 * r, 26 * r, dtype=torch.int64)
    want = M.inference(fe, cls, x[:1], label, flip=flip)
    for crop in ((18, 26), (19, 40)):
        got = M.slide_inference(fe, cls, x, label, crop, (7, 9), flip=flip)
        assert got.shape == (1, 5, 18 * r, 26 * r) and torch.equal(got, want)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("r", [1, 2])
def test_two_by_three_grid_equals_a_hand_written_per_pixel_average(net, flip, r):
    fe, cls = net
    H, W, crop, stride = 18, 26, (12, 12), (9, 7)
    x = _image(H, W, seed=1)
    label = torch.zeros(1, H * r, W * r, dtype=torch.int64)
    rows, cols, (wh, ww) = M.slide_plan((H, W), crop, stride)
    assert (rows, cols) == ([0, 6], [0, 7, 14])                # 2 x 3, clamped last row, an odd column origin
    got = M.slide_inference(fe, cls, x, label, crop, stride, flip=flip)
    # every window's map, by the reference's own inference() on the crop
    maps = {}
    for y0 in rows:
        for x0 in cols:
            maps[(y0, x0)] = M.inference(fe, cls, x[:1, :, y0:y0 + wh, x0:x0 + ww], torch.zeros(1, wh * r, ww * r), flip=flip)[0].numpy()
    want = np.zeros((5, H * r, W * r), np.float32)
    covers = set()
    for y in range(H * r):
        for xx in range(W * r):
            acc, cover = np.zeros(5, np.float32), 0
            for y0 in rows:                                    # row-major window order
                for x0 in cols:
                    if r * y0 <= y < r * (y0 + wh) and r * x0 <= xx < r * (x0 + ww):
                        acc = acc + maps[(y0, x0)][:, y - r * y0, xx - r * x0]
                        cover += 1
            want[:, y, xx] = acc / np.float32(cover)
            covers.add(cover)
    assert covers == {1, 2, 4}
    assert np.array_equal(got[0].numpy(), want)
    s = got.sum(1)
    assert float((s - 1).abs().max()) < 1e-5                   # still a distribution


def test_slide_inference_refuses_a_label_that_is_no_whole_multiple(net):
    fe, cls = net
    with pytest.raises(ValueError, match="18 x 26"):
        M.slide_inference(fe, cls, _image(18, 26), torch.zeros(1, 27, 39, dtype=torch.int64), (12, 12), (9, 7))
    with pytest.raises(ValueError, match="36 x 26"):
        M.slide_inference(fe, cls, _image(18, 26), torch.zeros(1, 36, 26, dtype=torch.int64), (12, 12), (9, 7))


def test_predict_and_score_slide_on_the_literal_path(net):
    fe, cls = net
    x = _image(18, 26, seed=2)
    g = torch.Generator().manual_seed(5)
    label = torch.randint(0, 5, (2, 18, 26), generator=g)
    label[0, :3] = 255
    out = M.slide_inference(fe, cls, x, label, (12, 12), (9, 7), flip=True)
    r = M.predict_and_score(fe, cls, x, label, flip=True, num_classes=5, threshold=0.5, slide=((12, 12), (9, 7)))
    assert torch.equal(r.pred, out.max(1)[1][0].to(torch.uint8))
    top = out.max(1)
    assert torch.equal(r.pseudo, torch.where(top[0] >= 0.5, top[1], torch.full_like(top[1], 255))[0].to(torch.uint8))
    plain = M.predict_and_score(fe, cls, x, label, flip=True, num_classes=5, threshold=0.5)
    assert not torch.equal(plain.pred, r.pred) or not torch.equal(plain.cmt, r.cmt)          # sliding is not a no-op on this net
    assert int(r.cmt.sum()) == 15 * 26
    table = [0.3, 0.4, 0.5, 0.6, 0.7]
    assert torch.equal(M.classwise_pseudo_labels(fe, cls, x, label, flip=True, num_classes=5, class_threshold=table, slide=((12, 12), (9, 7))),
                       M.literal_pseudo(out, table))
    with pytest.raises(NotImplementedError, match="single-scale"):
        M.predict_and_score(fe, cls, x, label, scales=(0.5, 1.0), num_classes=5, slide=((12, 12), (9, 7)))


# ------------------------------------------------------------------------------------------------ configuration
def _cfg(*opts):
    cfg = hc.cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(list(opts))
    return cfg


def test_slide_settings_defaults_and_order():
    cfg = _cfg()
    assert cfg.TEST.SLIDE is False and tuple(cfg.TEST.SLIDE_CROP) == (769, 769) and tuple(cfg.TEST.SLIDE_STRIDE) == (513, 513)
    assert M.slide_settings(cfg) is None
    assert M.slide_settings(_cfg("TEST.SLIDE", True)) == ((769, 769), (513, 513))
    # the keys are (width, height), the settings (h, w)
    assert M.slide_settings(_cfg("TEST.SLIDE", True, "TEST.SLIDE_CROP", (1025, 513), "TEST.SLIDE_STRIDE", (683, 342))) == ((513, 1025), (342, 683))
    assert M.slide_settings(_cfg("TEST.SLIDE", True, "TEST.FLIP", True)) is not None          # FLIP is supported


def test_slide_settings_refusals():
    for key, value in (("TEST.SLIDE_CROP", (513, 513)), ("TEST.SLIDE_STRIDE", (256, 256))):
        with pytest.raises(NotImplementedError, match=key.split(".")[1]):
            M.slide_settings(_cfg(key, value))                 # a stray key while SLIDE is False
    with pytest.raises(NotImplementedError, match="SCALES"):
        M.slide_settings(_cfg("TEST.SLIDE", True, "TEST.SCALES", (0.7, 1.0, 1.3)))
    with pytest.raises(ValueError):
        M.slide_settings(_cfg("TEST.SLIDE", True, "TEST.SLIDE_STRIDE", (770, 513)))            # stride > crop
    with pytest.raises(ValueError):
        M.slide_settings(_cfg("TEST.SLIDE", True, "TEST.SLIDE_CROP", (0, 769)))
    with pytest.raises(ValueError):
        M.slide_settings(_cfg("TEST.SLIDE", True, "TEST.SLIDE_CROP", (769, 769, 3)))


def test_other_testers_refuse_the_key_by_name():
    M.require_no_slide(_cfg(), "AnyTester")
    with pytest.raises(NotImplementedError, match="AnyTester: TEST.SLIDE"):
        M.require_no_slide(_cfg("TEST.SLIDE", True), "AnyTester")
    import inspect
    from rnd_semantic_segmentation_amd.host import gald, pranet
    assert 'require_no_slide(cfg, "GALDTester")' in inspect.getsource(gald.GALDTester.__init__)
    assert 'require_no_slide(cfg, "PranetTester")' in inspect.getsource(pranet.PranetTester.__init__)


def test_shipped_config_parses():
    import os
    cfg = hc.cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "deeplabv2_r101_test_slide.yaml"))
    assert M.slide_settings(cfg) == ((769, 769), (513, 513)) and tuple(cfg.INPUT.INPUT_SIZE_TEST) == (2048, 1024)
    rows, cols, _ = M.slide_plan((1024, 2048), *M.slide_settings(cfg))
    assert len(rows) * len(cols) == 8


# ------------------------------------------------------------------------------------------------ the C-ABI entries refuse before any launch
@pytest.fixture(scope="module")
def built():
    entry.build()
    return _lib.lib()


def _windows(specs):
    win = (_lib.MiSlideWindow * max(len(specs), 1))()
    for i, (low, mirror, y0, x0) in enumerate(specs):
        win[i].low, win[i].low_mirror, win[i].y0, win[i].x0 = low, mirror, y0, x0
    return win


def test_entries_exist_with_the_issues_signatures(built):
    assert len(_lib.SIGNATURES["mi_upsample_softmax_slide"][1]) == 11
    assert len(_lib.SIGNATURES["mi_upsample_predict_score_slide"][1]) == 19
    assert ctypes.sizeof(_lib.MiSlideWindow) == 24
    assert "MI_SLIDE_MAX_WINDOWS 64" in open(_lib.HEADER_PATH).read()


def test_launcher_refusals_need_no_gpu(built):
    """Every refusal returns -22 before a launch (no GPU exists here: a launch would fail differently)."""
    one, two = 16, 32                                          # non-null dummies: validation fails before they are dereferenced
    pred = ctypes.c_void_p(64)
    probs = ctypes.c_void_p(128)

    def softmax(specs, n=None, wh=20, ww=20, H=30, W=30, h=5, w=5, K=19):
        return built.mi_upsample_softmax_slide(_windows(specs), len(specs) if n is None else n, h, w, wh, ww, probs, K, H, W, None)

    def score(specs, n=None, wh=20, ww=20, H=30, W=30, K=19, labels=None, ignore=255, threshold=0.0, table=None, pseudo=None, counts=None, bins=0,
              hist=None):
        return built.mi_upsample_predict_score_slide(_windows(specs), len(specs) if n is None else n, 5, 5, wh, ww, K, H, W, labels, ignore, threshold,
                                                     table, pred, pseudo, counts, bins, hist, None)

    full = [(one, None, 0, 0), (one, None, 0, 10), (one, None, 10, 0), (one, None, 10, 10)]
    for call, who in ((softmax, b"mi_upsample_softmax_slide"), (score, b"mi_upsample_predict_score_slide")):
        for kw, needle in ((dict(specs=[], n=0), b"1 <= n <= 64"),
                           (dict(specs=full * 17, n=65), b"1 <= n <= 64"),
                           (dict(specs=full[:3] + [(one, None, 11, 10)]), b"leaves the 30 x 30"),
                           (dict(specs=full[:3] + [(one, None, 10, -1)]), b"leaves the 30 x 30"),
                           (dict(specs=full, wh=31, H=30), b"leaves the 30 x 30"),
                           (dict(specs=full[:3] + [(one, two, 10, 10)]), b"mirror maps on some windows only"),
                           (dict(specs=[(one, two, 0, 0)] + full[1:]), b"mirror maps on some windows only"),
                           (dict(specs=full[:3]), b"no window covers"),
                           (dict(specs=[full[0], full[3]]), b"no window covers"),
                           (dict(specs=full[:3] + [(None, None, 10, 10)]), b"without a low map"),
                           (dict(specs=full, K=33), b"K <= 32"),
                           (dict(specs=full, wh=4), b"only upsampling")):
            specs = kw.pop("specs")
            assert call(specs, **kw) == -22, (who, needle)
            err = built.mi_last_error()
            assert needle in err and who in err, err
    # what the scoring entries have always refused
    lab, cnt, tab, hist = ctypes.c_void_p(256), ctypes.c_void_p(512), (ctypes.c_float * 19)(*([0.5] * 19)), ctypes.c_void_p(1024)
    for kw, needle in ((dict(labels=lab), b"labels and counts go together"),
                       (dict(counts=cnt), b"labels and counts go together"),
                       (dict(labels=lab, counts=cnt, ignore=3), b"ignore_index inside"),
                       (dict(threshold=1.5), b"threshold outside [0, 1]"),
                       (dict(threshold=float("nan")), b"threshold outside [0, 1]"),
                       (dict(hist=hist, bins=0), b"hist without bins"),
                       (dict(hist=hist, bins=512), b"bins must be 1024"),
                       (dict(pseudo=pred, bins=1024), b"pseudo without class_threshold"),
                       (dict(table=(ctypes.c_float * 19)(*([0.5] * 18 + [1.5]))), b"threshold outside [0, 1]")):
        assert score(full, **kw) == -22, needle
        assert needle in built.mi_last_error(), built.mi_last_error()
    assert built.mi_upsample_predict_score_slide(_windows(full), 4, 5, 5, 20, 20, 19, 30, 30, None, 255, 0.0, None, None, None, None, 0, None, None) == -22
    assert b"null operand" in built.mi_last_error()
    assert built.mi_upsample_softmax_slide(None, 4, 5, 5, 20, 20, probs, 19, 30, 30, None) == -22 and b"null operand" in built.mi_last_error()
