"""mi_label_components and mi_lesion_score (csrc/components.hip) on the GPU against the raster flood fill of tests/_components_ref.py: every
comparison is == on integers, no tolerances and no excluded cases; the torch-op composition literal_lesion_stats as a second derivation;
PranetTester with TEST.LESION_METRICS / TEST.MASK_MIN_AREA on a stub net.  The cases are the smallest shapes at which the kernels can go wrong;
each asserts the property that makes it a case."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import _components_ref as ref
import _polyp_ref as polyp_ref
import _surface_ref as surface_ref

pytestmark = pytest.mark.gpu

LABEL_CASES = ref.label_cases()
LESION_CASES = ref.lesion_cases()
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


_REF = {}


def _label_ref(name, mask, connectivity, cls=1):
    """The flood fill of one image, computed once and left unchanged."""
    key = (name, connectivity, cls)
    if key not in _REF:
        _REF[key] = ref.label(np.asarray(mask) == cls, connectivity)
    return _REF[key]


def _lesion_ref(name, p, g, cls, connectivity, min_area, keep_largest, permille):
    key = (name, cls, connectivity, min_area, keep_largest, permille)
    if key not in _REF:
        _REF[key] = ref.reference(p, g, cls, connectivity, min_area, keep_largest, permille)
    return _REF[key]


def _label(mask, cls=1, connectivity=8, want_labels=True, want_roots=True):
    r = K.label_components(torch.from_numpy(np.ascontiguousarray(mask)).cuda(), cls, connectivity, want_labels, want_roots)
    assert r.counts.dtype == torch.int32 and r.counts.shape == (mask.shape[0],)
    for t in (r.labels, r.roots):
        assert t is None or (t.dtype == torch.int32 and tuple(t.shape) == mask.shape)
    return (None if r.labels is None else r.labels.cpu().numpy(), None if r.roots is None else r.roots.cpu().numpy(), r.counts.cpu().numpy())


def _assert_labels(tag, got, want):
    labels, roots, counts = got
    wl, wr, wn = want
    assert counts == wn, (tag, counts, wn)
    assert np.array_equal(labels, wl), (tag, "labels")
    assert np.array_equal(roots, wr), (tag, "roots")


def _score(pred, lab, **kw):
    r = K.lesion_score(torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(lab)).cuda(), **kw)
    assert r.ints.dtype == torch.int64 and tuple(r.ints.shape) == (pred.shape[0], 12)
    assert r.filtered.dtype == torch.uint8 and tuple(r.filtered.shape) == pred.shape
    return r.ints.cpu().numpy(), r.filtered.cpu().numpy()


# ------------------------------------------------------------------------------------------------ labelling
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("name", sorted(LABEL_CASES))
def test_single_images_equal_the_flood_fill(name, connectivity):
    m = LABEL_CASES[name]
    want = _label_ref(name, m, connectivity)
    labels, roots, counts = _label(m[None], 1, connectivity)
    _assert_labels((name, connectivity), (labels[0], roots[0], counts[0]), want)


@pytest.mark.parametrize("W", (1, 63, 64, 65, 130))
def test_words_1xW_have_runs_at_across_and_after_a_ballot_word(W):
    m = LABEL_CASES["words_1x%d" % W]
    assert m.shape == (1, W) and m.sum() == W - (1 if W > 64 else 0) and (W <= 64 or m[0, 64] == 0)
    labels, roots, counts = _label(m[None], 1, 4)
    assert counts[0] == (2 if W > 65 else 1)
    assert labels[0, 0, 0] == 1 and roots[0, 0, min(W, 64) - 1] == 0
    if W > 65:
        assert labels[0, 0, W - 1] == 2 and roots[0, 0, W - 1] == 65


def test_u_shape_arms_join_on_the_last_row():
    m = LABEL_CASES["u_shape_6x9"]
    assert m.shape == (6, 9) and m[0, 0] and m[0, 4] and not m[:5, 1:4].all(axis=1).any() and m[5, 0:5].all()
    for connectivity, n in ((8, 3), (4, 4)):
        labels, roots, counts = _label(m[None], 1, connectivity)
        assert counts[0] == n
        assert labels[0, 0, 0] == labels[0, 0, 4] == 1 and roots[0, 0, 4] == 0          # the arms are ONE component, number 1
        assert labels[0, 2, 2] not in (0, 1)                                           # the pixel between them is its own
        assert (labels[0, 1, 6] == labels[0, 2, 7]) == (connectivity == 8)             # the diagonal pair


def test_spiral_is_one_component_rooted_at_pixel_0():
    m, turns = ref.spiral(33, 64)
    assert np.array_equal(m, LABEL_CASES["spiral_33x64"]) and turns >= 8
    assert ((m[:-1] & m[1:]).sum() + (m[:, :-1] & m[:, 1:]).sum()) == m.sum() - 1       # a path: one pixel wide, no branch, no loop
    for connectivity in (4, 8):
        labels, roots, counts = _label(m[None], 1, connectivity)
        assert counts[0] == 1 and (roots[0][m == 1] == 0).all() and (labels[0] == m).all()


def test_checker_comb_and_frames():
    m = LABEL_CASES["checker_37x45"]
    assert _label(m[None], 1, 4)[2][0] == (37 * 45 + 1) // 2 == m.sum() and _label(m[None], 1, 8)[2][0] == 1
    m = LABEL_CASES["comb_40x130"]
    assert m.shape == (40, 130) and m[0].sum() == 65 and m[38].sum() == 65 and m[39].all()      # 65 teeth joined by the LAST row only
    assert _label(m[None], 1, 4)[2][0] == 1 and _label(m[None], 1, 8)[2][0] == 1
    m = LABEL_CASES["frame_in_frame_37x45"]
    assert _label(m[None], 1, 4)[2][0] == 4 and _label(m[None], 1, 8)[2][0] == 4


def test_speckle_and_blobs_have_many_and_large_components():
    m = LABEL_CASES["speckle_37x45"]
    labels, _, counts = _label(m[None], 1, 4)
    assert counts[0] > 30
    spans = [np.ptp(np.nonzero((labels[0] == k).any(axis=1))[0]) + 1 for k in range(1, counts[0] + 1)]
    assert max(spans) >= 5
    m = LABEL_CASES["blobs_200x517"]
    for connectivity in (4, 8):
        labels, _, counts = _label(m[None], 1, connectivity)
        assert counts[0] > 100 and np.bincount(labels[0].ravel())[1:].max() > 5000


def test_full_empty_and_single_pixel_images():
    labels, roots, counts = _label(LABEL_CASES["full_9x70"][None])
    assert counts[0] == 1 and (labels == 1).all() and (roots == 0).all()
    labels, roots, counts = _label(LABEL_CASES["empty_9x70"][None])
    assert counts[0] == 0 and (labels == 0).all() and (roots == -1).all()
    labels, roots, counts = _label(LABEL_CASES["single_9x70"][None])
    assert counts[0] == 1 and labels.sum() == 1 and labels[0, 4, 66] == 1 and roots[0, 4, 66] == 4 * 70 + 66 and (roots == -1).sum() == 9 * 70 - 1


@pytest.mark.parametrize("connectivity", (4, 8))
def test_batch_of_three_different_images_one_empty(connectivity):
    names = ("speckle_37x45", "empty_37x45", "frame_in_frame_37x45")
    batch = np.stack([LABEL_CASES[names[0]], np.zeros((37, 45), np.uint8), LABEL_CASES[names[2]]])
    labels, roots, counts = _label(batch, 1, connectivity)
    for b, name in enumerate(names):
        _assert_labels((name, b), (labels[b], roots[b], counts[b]), _label_ref(name, batch[b], connectivity))
    assert counts[1] == 0 and counts[0] != counts[2]


def test_class_3_of_a_map_with_several_values():
    m = surface_ref.multi_class_map(37, 45, 6).astype(np.uint8)
    assert len(np.unique(m)) == 5 and (m == 3).any()
    for connectivity in (4, 8):
        labels, roots, counts = _label(m[None], 3, connectivity)
        _assert_labels(("cls3", connectivity), (labels[0], roots[0], counts[0]), _label_ref("cls3", m, connectivity, 3))
        assert not np.array_equal(_label(m[None], 1, connectivity)[0], labels)


def test_labels_only_roots_only_and_both():
    m = LABEL_CASES["speckle_37x45"]
    want = _label_ref("speckle_37x45", m, 8)
    both = _label(m[None])
    only_l, only_r = _label(m[None], want_roots=False), _label(m[None], want_labels=False)
    assert only_l[1] is None and only_r[0] is None
    assert np.array_equal(only_l[0], both[0]) and np.array_equal(only_r[1], both[1]) and only_l[2] == only_r[2] == both[2]
    _assert_labels("both", (both[0][0], both[1][0], both[2][0]), want)


def test_two_calls_give_equal_bits():
    batch = torch.from_numpy(np.stack([LABEL_CASES["speckle_37x45"], LABEL_CASES["checker_37x45"]])).cuda()
    lab = torch.from_numpy(np.stack([LABEL_CASES["frame_in_frame_37x45"], LABEL_CASES["speckle_37x45"]]).astype(np.int64)).cuda()
    a, s = K.label_components(batch, want_roots=True), K.lesion_score(batch, lab, min_area=3)
    big = torch.from_numpy(LABEL_CASES["blobs_200x517"][None]).cuda()                   # another size through the cached workspaces in between
    K.label_components(big)
    K.lesion_score(big, big.long())
    b, t = K.label_components(batch, want_roots=True), K.lesion_score(batch, lab, min_area=3)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.roots, b.roots) and torch.equal(a.counts, b.counts)
    assert torch.equal(s.ints, t.ints) and torch.equal(s.filtered, t.filtered)


def test_capped_grid_takes_a_second_trip():
    """The row launches hold at most 2^14 workgroups, one row each: 81 images of 205 x 5 are 16 605 rows, so 221 workgroups walk a second row
    (in mi_lesion_score, with its 2 B planes, every workgroup does)."""
    g = np.random.RandomState(7)
    pred, lab = (g.rand(81, 205, 5) < 0.5).astype(np.uint8), (g.rand(81, 205, 5) < 0.5).astype(np.int64)
    assert 81 * 205 > 1 << 14
    labels, roots, counts = _label(pred, 1, 4)
    ints, filtered = _score(pred, lab, connectivity=4, min_area=4)
    for b in range(81):
        _assert_labels(("cap", b), (labels[b], roots[b], counts[b]), ref.label(pred[b] == 1, 4))
        want_ints, want_f = ref.reference(pred[b], lab[b], 1, 4, 4, False, 0)
        assert np.array_equal(ints[b], want_ints) and np.array_equal(filtered[b], want_f), ("cap", b)
    assert ints[:, 11].sum() > 81


# ------------------------------------------------------------------------------------------------ lesion scores
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("name", sorted(LESION_CASES))
def test_lesion_score_equals_the_reference(name, connectivity):
    """All twelve integers and the filtered mask, over min_area x keep_largest x overlap."""
    p, g = LESION_CASES[name]
    assert (p == 1).any() and (g == 1).any()
    everything = int(p.sum()) + 1
    removed = set()
    for min_area in (0, 1, 12, everything):
        for keep_largest in (False, True):
            for overlap in (0.0, 0.001, 0.5, 1.0):
                permille = int(round(1000 * overlap))
                want_ints, want_f = _lesion_ref(name, p, g, 1, connectivity, min_area, keep_largest, permille)
                ints, filtered = _score(p[None], g[None], connectivity=connectivity, min_area=min_area, keep_largest=keep_largest, overlap=overlap)
                tag = (name, connectivity, min_area, keep_largest, overlap)
                assert np.array_equal(ints[0], want_ints), (tag, ints[0].tolist(), want_ints.tolist())
                assert np.array_equal(filtered[0], want_f), tag
                assert ints[0, 11] == ints[0, 3] - ints[0, 4], tag
                assert not (filtered[0] & ~p).any(), tag                               # a subset of P
                if min_area <= 1 and not keep_largest:
                    assert np.array_equal(filtered[0], p), tag                         # no filter: P itself
                removed.add(int(ints[0, 11]))
    assert 0 in removed and len(removed) > 1 and max(removed) == _lesion_ref(name, p, g, 1, connectivity, 0, False, 0)[0][3]


def test_lesion_cases_show_what_they_are_named_for():
    s = {name: _score(p[None], g[None])[0][0] for name, (p, g) in LESION_CASES.items()}
    assert s["split"][3] == 2 and s["split"][5] == 1 and s["split"][6] == 2 and s["split"][7] == 1          # two true positives, one lesion
    assert s["bridge"][3] == 1 and s["bridge"][5] == 2 and s["bridge"][6] == 1 and s["bridge"][7] == 2      # one prediction detects two lesions
    assert s["specks"][3] == 5 and s["specks"][6] == 2 and s["specks"][7] == 2                              # three specks are false alarms
    p, g = LESION_CASES["specks"]
    assert _score(p[None], g[None], connectivity=4)[0][0][3] == 6                                           # the diagonal pair falls apart
    half = _score(p[None], g[None], overlap=0.5)[0][0]
    assert half[6] == 2 and half[7] == 1                       # the speck with exactly half its area on the lesion still counts; the lesion under it does not
    assert _score(p[None], g[None], overlap=0.501)[0][0][6] == 1
    p, g = LESION_CASES["tie"]
    ints, filtered = _score(p[None], g[None], keep_largest=True)
    assert ints[0, 8] == 24 and ints[0, 4] == 1 and ints[0, 1] == 24 and filtered[0, 4:8, 60:66].all() and not filtered[0, 20:26].any()      # the tie: first in raster order
    p, g = LESION_CASES["shifted"]
    assert _score(p[None], g[None], overlap=0.5)[0][0][6] == 2 and _score(p[None], g[None], overlap=1.0)[0][0][6] == 0


def test_lesion_batch_with_empty_masks_and_other_label_values():
    p, g = LESION_CASES["specks"]
    z = np.zeros_like(p)
    pred, lab = np.stack([p, z, p, z]), np.stack([g, g, z.astype(np.int64), z.astype(np.int64)])
    ints, filtered = _score(pred, lab, min_area=12)
    for b in range(4):
        want_ints, want_f = ref.reference(pred[b], lab[b], 1, 8, 12, False, 0)
        assert np.array_equal(ints[b], want_ints) and np.array_equal(filtered[b], want_f), b
    assert ints[1, :2].sum() == 0 and ints[1, 5] == 2 and ints[2, 5:8].sum() == 0 and ints[2, 4] > 0 and ints[3].sum() == 0
    noisy = lab.copy()
    noisy[lab == 0] = np.where(np.random.RandomState(9).rand(int((lab == 0).sum())) < 0.3, 255, 2)      # 255 and 2 are background
    again = _score(pred, noisy, min_area=12)
    assert np.array_equal(again[0], ints) and np.array_equal(again[1], filtered)


def test_lesion_class_3_and_class_0():
    pred, lab = surface_ref.multi_class_map(37, 45, 6).astype(np.uint8), surface_ref.multi_class_map(37, 45, 5)
    for cls in (3, 0):
        want_ints, want_f = ref.reference(pred, lab, cls, 8, 5, False, 100)
        ints, filtered = _score(pred[None], lab[None], cls=cls, min_area=5, overlap=0.1)
        assert np.array_equal(ints[0], want_ints) and np.array_equal(filtered[0], want_f), cls
        assert ints[0, 11] > 0 and set(np.unique(filtered)) == {cls, 1 if cls == 0 else 0}
    r = K.lesion_score(torch.from_numpy(pred[None]).cuda(), torch.from_numpy(lab[None]).cuda(), cls=3, min_area=5, overlap=0.1, want_filtered=False)
    assert r.filtered is None and np.array_equal(r.ints.cpu().numpy()[0], ref.reference(pred, lab, 3, 8, 5, False, 100)[0])


def test_agrees_with_the_literal_torch_composition():
    for name in sorted(LESION_CASES):
        p, g = LESION_CASES[name]
        for connectivity, min_area, keep_largest, overlap in ((8, 0, False, 0.0), (4, 12, False, 0.5), (8, 2, True, 0.001)):
            ints, filtered = _score(p[None], g[None], connectivity=connectivity, min_area=min_area, keep_largest=keep_largest, overlap=overlap)
            lit_ints, lit_f = M.literal_lesion_stats(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), 1, connectivity, min_area, keep_largest, overlap)
            assert ints[0].tolist() == [int(v) for v in lit_ints], (name, connectivity, min_area)
            assert np.array_equal(filtered[0], lit_f.cpu().numpy()), (name, connectivity, min_area)


def test_wrapper_refusals():
    from rnd_semantic_segmentation_amd import _lib
    p, g = LESION_CASES["specks"]
    pred, lab = torch.from_numpy(p[None]).cuda(), torch.from_numpy(g[None]).cuda()
    with pytest.raises(_lib.MiError, match="int64"):
        K.lesion_score(pred, lab.int())
    with pytest.raises(_lib.MiError, match="uint8"):
        K.lesion_score(pred.long(), lab)
    with pytest.raises(_lib.MiError, match="uint8"):
        K.label_components(pred.long())
    with pytest.raises(_lib.MiError, match="one device"):
        K.lesion_score(pred[0], lab[0])
    with pytest.raises(_lib.MiError, match="one device"):
        K.lesion_score(pred, lab[:, :20])
    with pytest.raises(_lib.MiError, match=r"\[B,H,W\]"):
        K.label_components(pred[0])
    with pytest.raises(_lib.MiError, match="contiguous"):
        K.lesion_score(pred.transpose(1, 2), lab.transpose(1, 2))
    with pytest.raises(_lib.MiError, match="contiguous"):
        K.label_components(pred.transpose(1, 2))
    for bad in (6, 0, "8"):
        with pytest.raises(_lib.MiError, match="connectivity"):
            K.lesion_score(pred, lab, connectivity=bad)
        with pytest.raises(_lib.MiError, match="connectivity"):
            K.label_components(pred, connectivity=bad)
    for bad in (-0.1, 1.001, "0.5"):
        with pytest.raises(_lib.MiError, match="overlap"):
            K.lesion_score(pred, lab, overlap=bad)
    for bad in (-1, 2.5, True):
        with pytest.raises(_lib.MiError, match="min_area"):
            K.lesion_score(pred, lab, min_area=bad)
    for bad in (256, -1, 1.5):
        with pytest.raises(_lib.MiError, match="cls"):
            K.lesion_score(pred, lab, cls=bad)
        with pytest.raises(_lib.MiError, match="cls"):
            K.label_components(pred, cls=bad)
    with pytest.raises(_lib.MiError, match="at least one"):
        K.label_components(pred, want_labels=False, want_roots=False)
    with pytest.raises(_lib.MiError, match="GPU"):
        K.label_components(pred.cpu())


# ------------------------------------------------------------------------------------------------ the tester
class _Log(logging.Logger):
    def __init__(self):
        super().__init__("lesion")
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


STUB_SEED = 3
MIN_AREA = 20


def _stub_inputs():
    """Two smooth maps (an ellipse of logit +4 in -4, a little noise) at 32 x 32, each with an added speck of 2 x 2 far from the ellipse, and
    speckled elliptic labels at 37 x 45."""
    g = np.random.RandomState(STUB_SEED)
    maps = np.stack([8.0 * surface_ref.ellipse(32, 32, 15, 14, 9, 11) - 4.0, 8.0 * surface_ref.ellipse(32, 32, 18, 20, 7, 6) - 4.0])[:, None]
    maps[0, 0, 28:30, 27:29] = 4.0
    maps[1, 0, 2:4, 3:5] = 4.0
    maps = (maps + 0.3 * g.randn(2, 1, 32, 32)).astype(np.float32)
    lab = np.stack([surface_ref.speckle(surface_ref.ellipse(37, 45, 17, 21, 11, 15), 0.02, 11),
                    surface_ref.speckle(surface_ref.ellipse(37, 45, 22, 26, 8, 9), 0.02, 12)]).astype(np.int64)
    return maps, lab


def _stub_run(tmp_path, lab, maps, *opts):
    from rnd_semantic_segmentation_amd.host import pranet
    log = _Log()
    x = torch.zeros(2, 3, 32, 32)
    tester = pranet.PranetTester(_cfg(tmp_path, *opts), torch.device("cuda"), [(x, torch.from_numpy(lab), ["first", "second"])], log)
    tester.model = _Stub(torch.from_numpy(maps).cuda())
    tester.test()
    return log.lines, tester


SURF = ("TEST.SURFACE_METRICS", True)
POLYP = ("TEST.POLYP_METRICS", True)
LESION = ("TEST.LESION_METRICS", True)
FILTER = ("TEST.MASK_MIN_AREA", MIN_AREA)
METER_ATTRS = ("intersection_sum", "union_sum", "target_sum", "res_sum", "iou_sum", "f1_sum")


def _reference_mask(maps, lab):
    pref = polyp_ref.reference_map(maps[:, 0], lab.shape[1:])
    assert float(np.abs(2 * pref - 1).min()) > 1e-4                                           # no pixel near the threshold: the mask is the reference's
    return (pref > 1 - pref).astype(np.uint8)


def _files(path):
    """The files of an output directory; the tester creates it only when it writes one."""
    return sorted(os.listdir(path)) if os.path.exists(path) else []


def _same_meter(a, b):
    return a.count == b.count and all(np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))) for k in METER_ATTRS)


def test_tester_with_the_keys_off_runs_nothing_new(tmp_path, monkeypatch):
    maps, lab = _stub_inputs()

    def never(*a, **k):
        raise AssertionError("lesion_score launched with the keys off")

    monkeypatch.setattr(K, "lesion_score", never)
    monkeypatch.setattr(K, "label_components", never)
    for opts in ((), SURF, POLYP + SURF):
        plain = _stub_run(tmp_path / "plain", lab, maps, *opts)
        named = _stub_run(tmp_path / "named", lab, maps, *(opts + ("TEST.LESION_METRICS", False, "TEST.MASK_MIN_AREA", 0, "TEST.MASK_KEEP_LARGEST", False,
                                                                  "TEST.LESION_CONNECTIVITY", 4, "TEST.LESION_OVERLAP", 0.5)))
        assert plain[0] == named[0] and len(plain[0]) >= 6 and not any("esion" in line or "filter" in line for line in plain[0])
        assert _same_meter(plain[1].meter, named[1].meter) and plain[1].lesion is None and plain[1].lesion_meter is None
        assert _files(tmp_path / "plain") == _files(tmp_path / "named") \
            == sorted(["pranet_surface_metrics.json"] * (SURF[0] in opts) + ["pranet_polyp_metrics.json"] * (POLYP[0] in opts))
        for name in _files(tmp_path / "plain"):
            assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "named" / name, "rb").read()


def test_tester_with_lesion_metrics_only(tmp_path):
    maps, lab = _stub_inputs()
    mask = _reference_mask(maps, lab)
    want = M.LesionMeter()
    for b in range(2):
        want.update(M.lesion_image_stats(ref.reference(mask[b], lab[b], 1, 4, 0, False, 500)[0]))
    assert want.sums["kept_components"] > want.sums["true_positives"] > 0 and want.sums["removed_components"] == 0      # the specks are false positives
    opts = LESION + ("TEST.LESION_CONNECTIVITY", 4, "TEST.LESION_OVERLAP", 0.5)
    runs = {key: _stub_run(tmp_path / key, lab, maps, *o) for key, o in (("off", ()), ("lesion", opts), ("all", POLYP + SURF), ("all_lesion", POLYP + SURF + opts))}
    for base, key in (("off", "lesion"), ("all", "all_lesion")):
        before, after = runs[base][0], runs[key][0]
        assert after[:len(before)] == before and len(after) == len(before) + 2                # earlier lines unchanged, the summary added
        assert after[len(before)].startswith("Lesion metric, val result over 2 images: recall ") and not any("Mask filter" in line for line in after)
        assert _same_meter(runs[base][1].meter, runs[key][1].meter)
        assert not os.path.exists(tmp_path / base / "pranet_lesion_metrics.json")
        data = json.load(open(tmp_path / key / "pranet_lesion_metrics.json"))
        assert data == dict(want.as_dict(), connectivity=4, overlap=0.5, min_area=0, keep_largest=False)
    for name in ("pranet_polyp_metrics.json", "pranet_surface_metrics.json"):
        assert open(tmp_path / "all" / name, "rb").read() == open(tmp_path / "all_lesion" / name, "rb").read()
    assert runs["lesion"][0][-2:] == runs["all_lesion"][0][-2:]


def test_tester_with_a_mask_filter(tmp_path):
    maps, lab = _stub_inputs()
    mask = _reference_mask(maps, lab)
    refs = [ref.reference(mask[b], lab[b], 1, 8, MIN_AREA, False, 0) for b in range(2)]
    filtered = np.stack([r[1] for r in refs])
    assert all(r[0][11] >= 1 and r[0][4] >= 1 for r in refs) and (filtered != mask).any()       # the filter removes the speck and keeps the polyp
    want_meter = M.AverageMeter()
    want_meter.update(*[np.asarray(v, dtype=np.float32) for v in M.intersectionAndUnion(filtered, lab, 2, 255)])
    plain_meter = M.AverageMeter()
    plain_meter.update(*[np.asarray(v, dtype=np.float32) for v in M.intersectionAndUnion(mask, lab, 2, 255)])
    assert not _same_meter(want_meter, plain_meter)
    want_surface = M.SurfaceMeter(95, (2.0,))
    for b in range(2):
        ints, d2, _ = surface_ref.reference(filtered[b], lab[b], 1, 95, (2.0,))
        want_surface.update(M.surface_image_stats(ints, np.array(surface_ref.sums(d2)), (2.0,), 95))
    runs = {key: _stub_run(tmp_path / key, lab, maps, *o) for key, o in (("plain", POLYP + SURF), ("filter", POLYP + SURF + FILTER), ("bare", FILTER),
                                                                        ("both", POLYP + SURF + FILTER + LESION))}
    assert _same_meter(runs["plain"][1].meter, plain_meter)
    for key in ("filter", "bare", "both"):
        assert _same_meter(runs[key][1].meter, want_meter), key
    for key in ("filter", "both"):
        data = json.load(open(tmp_path / key / "pranet_surface_metrics.json"))
        want = dict(want_surface.as_dict(), percentile=95, tolerances=[2.0])
        assert set(data) == set(want)
        for k, w in want.items():
            assert abs(data[k] - w) <= 1e-12 * max(w, 1.0) if isinstance(w, float) else data[k] == w, (key, k, data[k], w)
        assert open(tmp_path / key / "pranet_polyp_metrics.json", "rb").read() == open(tmp_path / "plain" / "pranet_polyp_metrics.json", "rb").read()
    # the speck moved the surface distances (with a speckled label either way: its stray pixels near the speck lose their nearest neighbour)
    assert json.load(open(tmp_path / "plain" / "pranet_surface_metrics.json"))["HD"] != json.load(open(tmp_path / "filter" / "pranet_surface_metrics.json"))["HD"]
    # only filter keys: no file, one more line - the one that states the filter
    assert not os.path.exists(tmp_path / "filter" / "pranet_lesion_metrics.json") and not os.path.exists(tmp_path / "bare")
    assert len(runs["filter"][0]) == len(runs["plain"][0]) + 1 and runs["filter"][0][-1].startswith("Mask filter: components below %d pixels removed" % MIN_AREA)
    assert len(runs["both"][0]) == len(runs["filter"][0]) + 2 and runs["both"][0][-3] == runs["filter"][0][-1]
    data = json.load(open(tmp_path / "both" / "pranet_lesion_metrics.json"))
    want = M.LesionMeter()
    for r in refs:
        want.update(M.lesion_image_stats(r[0]))
    assert data == dict(want.as_dict(), connectivity=8, overlap=0.0, min_area=MIN_AREA, keep_largest=False) and data["removed_components"] >= 2
    # keep_largest alone is a filter too
    lines, tester = _stub_run(tmp_path / "largest", lab, maps, "TEST.MASK_KEEP_LARGEST", True)
    largest = np.stack([ref.reference(mask[b], lab[b], 1, 8, 0, True, 0)[1] for b in range(2)])
    want_largest = M.AverageMeter()
    want_largest.update(*[np.asarray(v, dtype=np.float32) for v in M.intersectionAndUnion(largest, lab, 2, 255)])
    assert _same_meter(tester.meter, want_largest) and "only the largest kept" in lines[-1]
