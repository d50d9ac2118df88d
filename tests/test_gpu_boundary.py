"""GPU side of the boundary metrics (TEST.BOUNDARY): mi_boundary_score (csrc/boundary_score.hip) against the literal composition of
host/metrics.py (iterated max_pool2d erosion per class) - exact integer equality of all five histograms on every case.  Then accumulation,
bit-reproducibility, the wrapper's refusals, one graph capture, and ASPPTester on a small backbone with the key on, fused and literal."""
import io
import json
import os

import numpy as np
import pytest
import torch

import _boundary_ref as ref
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

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


def _blocks(H, W, Kc, seed, block, shift=(2, 3), noise=0.02, **kw):
    labels = ref.block_labels(H, W, Kc, seed, block=block, **kw)
    return ref.shifted_prediction(labels, Kc, seed + 1000, shift=shift, noise=noise), labels


def _uniform(H, W, Kc, value):
    return np.full((H, W), value, dtype=np.uint8), np.full((H, W), value, dtype=np.int64)


def _checkerboard(n):
    yy, xx = np.mgrid[:n, :n]
    board = (yy + xx) % 2
    return board.astype(np.uint8), board.astype(np.int64)


# name -> (inputs, K, ignore_index, D)
CASES = {
    "1x1": (lambda: _blocks(1, 1, 3, 1, (1, 1), holes=0.0), 3, 255, 5),
    "1x70": (lambda: _blocks(1, 70, 3, 2, (1, 20), shift=(0, 3)), 3, 255, 9),
    "70x1": (lambda: _blocks(70, 1, 3, 3, (20, 1), shift=(3, 0)), 3, 255, 9),
    "5x7-every-walk-ends-at-the-edge": (lambda: _uniform(5, 7, 2, 1), 2, 255, 64),
    "13x21-K19-D4": (lambda: _blocks(13, 21, 19, 4, (4, 5), shift=(1, 1)), 19, 255, 4),
    "checkerboard-40": (lambda: _checkerboard(40), 2, 255, 7),
    "uniform-150x300-cap-and-ramp": (lambda: _uniform(150, 300, 19, 11), 19, 255, 64),
    "blocks-70x150-D9": (lambda: _blocks(70, 150, 19, 5, (14, 40), noise=0.001, holes=0.0), 19, 255, 9),
    "blocks-150x300-D64": (lambda: _blocks(150, 300, 19, 6, (75, 150), shift=(5, 9), noise=0.0002, holes=0.0), 19, 255, 64),
    "K32": (lambda: _blocks(45, 83, 32, 7, (8, 12)), 32, 255, 12),
    "ignore-and-out-of-range-labels": (lambda: _blocks(52, 77, 7, 8, (9, 14), holes=0.08, stray=0.05), 7, 255, 10),
    "negative-ignore-index": (lambda: _blocks(31, 66, 5, 9, (7, 15), holes=0.05, ignore_index=-1, stray=0.03), 5, -1, 6),
    "pred-beyond-K": (lambda: (lambda lab: (ref.shifted_prediction(lab, 6, 77, beyond=0.1), lab))(ref.block_labels(47, 90, 6, 10, block=(10, 18))),
                      6, 255, 8),
    "D1": (lambda: _blocks(33, 130, 19, 11, (6, 25)), 19, 255, 1),
    # the row pass beyond one wave segment of 512 pixels, and widths that are multiples of 64 (the run-ending edge at column W then lies in a
    # chunk of its own): runs that straddle x = 512 and x = 1024, what every 1024- or 2048-wide label meets
    "6x64": (lambda: _blocks(6, 64, 3, 12, (3, 40), shift=(1, 2), noise=0.0, holes=0.0), 3, 255, 64),
    "20x128-D64": (lambda: _blocks(20, 128, 4, 13, (12, 70), shift=(1, 3), noise=0.002), 4, 255, 64),
    "5x576-second-segment-ends-at-W": (lambda: _blocks(5, 576, 3, 14, (4, 150), shift=(1, 7), noise=0.0, holes=0.0), 3, 255, 64),
    "9x1100-wide-blocks-D64": (lambda: _blocks(9, 1100, 5, 15, (6, 400), shift=(1, 11), noise=0.0005, holes=0.0), 5, 255, 64),
    "12x1024-wide-blocks-D64": (lambda: _blocks(12, 1024, 5, 16, (30, 400), shift=(2, 9), noise=0.0005, holes=0.0), 5, 255, 64),
    "140x1100-deep-blocks-D64": (lambda: _blocks(140, 1100, 5, 18, (140, 400), shift=(3, 11), noise=0.00002, holes=0.0), 5, 255, 64),
    # more row segments and more tiles than either launch's grid holds: workgroups stride
    "4300000x1-capped-grids": (lambda: _blocks(4300000, 1, 2, 17, (5000, 1), shift=(700, 0), noise=0.0001, holes=0.0001), 2, 255, 2),
}
_CACHE = {}


def _case(name):
    """(pred, labels on the GPU, K, ignore_index, D, the literal histograms): computed once per case and left unchanged."""
    if name not in _CACHE:
        make, Kc, ignore, D = CASES[name]
        pred, labels = make()
        pred, labels = torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda()
        _CACHE[name] = (pred, labels, Kc, ignore, D, M.literal_boundary_histograms(pred, labels, Kc, ignore, D))
    return _CACHE[name]


def _fused(pred, labels, Kc, ignore, D, into=None):
    hist = torch.zeros(5, Kc, D + 1, dtype=torch.int64, device="cuda") if into is None else into
    out = K.boundary_score(pred, labels, Kc, ignore, D, hist)
    assert out is hist
    return hist


@pytest.mark.parametrize("name", list(CASES))
def test_histograms_equal_the_literal_composition(name):
    pred, labels, Kc, ignore, D, want = _case(name)
    got = _fused(pred, labels, Kc, ignore, D)
    H, W = labels.shape
    wrong = int((got != want).sum())
    print("%s: %d x %d, K %d, D %d: %d labelled pixels, %d in cell 0, %d at the cap, %d hits; %d of %d cells differ"
          % (name, H, W, Kc, D, int(want[0].sum()), int(want[0, :, 0].sum()), int(want[0, :, D].sum()), int(want[3].sum()), wrong, want.numel()))
    assert torch.equal(got, want)
    assert int(want[0].sum()) == int(((labels >= 0) & (labels < Kc)).sum())


def test_the_cases_reach_what_they_are_for():
    """Each case exercises its path: the cap, the ramp, cell 0 only, max(eG, eP) differing from both, dropped pixels."""
    assert int(_case("checkerboard-40")[5][:, :, 1:].sum()) == 0 and int(_case("checkerboard-40")[5][0].sum()) == 1600
    uni = _case("uniform-150x300-cap-and-ramp")[5]
    assert int(uni[0, 11, 64]) == (150 - 128) * (300 - 128) and all(int(uni[0, 11, e]) == 2 * (150 + 300 - 4 * e) - 4 for e in range(64))
    edge = _case("5x7-every-walk-ends-at-the-edge")[5]
    assert edge[0, 1].tolist()[:4] == [20, 12, 3, 0] and int(edge[0, 1, 3:].sum()) == 0
    for name in ("blocks-70x150-D9", "blocks-150x300-D64"):
        h = _case(name)[5]
        assert not torch.equal(h[2], h[3]) and int(h[0, :, 9:].sum()) > 0 and int(h[1, :, 9:].sum()) > 0 and int(h[0, :, 1:9].sum()) > 0
    pred, labels, Kc, ignore, D, h = _case("ignore-and-out-of-range-labels")
    assert int((labels == 255).sum()) > 0 and int(((labels != 255) & ((labels < 0) | (labels >= Kc))).sum()) > 0
    assert int(h[0].sum()) < int(h[1].sum()) < labels.numel()               # stray labels count for P, ignored ones for neither
    pred, labels, Kc, ignore, D, h = _case("pred-beyond-K")
    assert int((pred >= Kc).sum()) > 0 and int(h[1].sum()) < int((labels != 255).sum())
    assert _case("D1")[5].shape[2] == 2
    for name, seams in (("5x576-second-segment-ends-at-W", (512,)), ("9x1100-wide-blocks-D64", (512, 1024)), ("12x1024-wide-blocks-D64", (512,)),
                        ("140x1100-deep-blocks-D64", (512, 1024))):
        labels = _case(name)[1]
        for x in seams:                                                      # a run of at least 20 pixels on either side of the segment seam
            assert bool((labels[:, x - 20:x + 20] == labels[:, x:x + 1]).all(1).any()), (name, x)
    assert all(_case(n)[1].shape[1] % 64 == 0 for n in ("6x64", "20x128-D64", "5x576-second-segment-ends-at-W", "12x1024-wide-blocks-D64"))
    assert int(_case("12x1024-wide-blocks-D64")[5][0, :, 2:].sum()) > 0
    deep = _case("140x1100-deep-blocks-D64")
    assert int(deep[5][0, :, 64].sum()) > 0 and int(deep[5][1, :, 64].sum()) > 0                 # walks to the cap
    assert int(M.boundary_survival(deep[1], 5, 64)[:, 512].max()) == 64                          # ... also on the segment seam


def test_two_launches_into_one_buffer_add_up():
    a, b = _case("blocks-70x150-D9"), _case("uniform-150x300-cap-and-ramp")
    D = 9
    hist = torch.zeros(5, 19, D + 1, dtype=torch.int64, device="cuda")
    _fused(a[0], a[1], 19, 255, D, into=hist)
    _fused(a[0], a[1], 19, 255, D, into=hist)
    assert torch.equal(hist, 2 * a[5])
    other = M.literal_boundary_histograms(b[0], b[1], 19, 255, D)           # a second picture of another size into the same buffer
    _fused(b[0], b[1], 19, 255, D, into=hist)
    assert torch.equal(hist, 2 * a[5] + other)
    big = torch.full((5, 19, D + 1), 1 << 40, dtype=torch.int64, device="cuda")       # 64-bit cells: nothing wraps at 2^32
    _fused(a[0], a[1], 19, 255, D, into=big)
    assert torch.equal(big, a[5] + (1 << 40))


def test_two_runs_give_identical_bits():
    pred, labels, Kc, ignore, D, want = _case("blocks-150x300-D64")
    first = _fused(pred, labels, Kc, ignore, D)
    K._workspace(K._lib.lib().mi_boundary_score_workspace(150, 300), pred.device, "boundary").fill_(0xA5)      # the workspace needs no initialisation
    second = _fused(pred, labels, Kc, ignore, D)
    assert torch.equal(first, second) and torch.equal(first, want)


def test_wrapper_refusals():
    from rnd_semantic_segmentation_amd._lib import MiError
    pred, labels, Kc, ignore, D, _ = _case("13x21-K19-D4")
    hist = torch.zeros(5, Kc, D + 1, dtype=torch.int64, device="cuda")
    for kw, word in ((dict(num_classes=33, hist=torch.zeros(5, 33, D + 1, dtype=torch.int64, device="cuda")), "K 33"),
                     (dict(max_width=65, hist=torch.zeros(5, Kc, 66, dtype=torch.int64, device="cuda")), "D 65"),
                     (dict(ignore_index=3), "ignore_index 3"),
                     (dict(hist=hist[:, :, :D].contiguous()), "hist must be"),
                     (dict(hist=hist.int()), "hist must be"),
                     (dict(pred=pred.long()), "pred must be"),
                     (dict(labels=labels.int()), "labels must be"),
                     (dict(labels=labels[:, :20].contiguous()), "one device"),
                     (dict(pred=pred.cpu()), "GPU")):
        a = dict(pred=pred, labels=labels, num_classes=Kc, ignore_index=ignore, max_width=D, hist=hist)
        a.update(kw)
        with pytest.raises(MiError, match=word):
            K.boundary_score(**a)
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0                                              # nothing was launched


def test_graph_capture_and_replay_with_changed_inputs():
    first, second = _case("blocks-70x150-D9"), _blocks(70, 150, 19, 55, (10, 30))
    second = (torch.from_numpy(second[0]).cuda(), torch.from_numpy(second[1]).cuda())
    pred, labels = first[0].clone(), first[1].clone()
    hist = torch.zeros(5, 19, 10, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up off the capture
        K.boundary_score(pred, labels, 19, 255, 9, hist)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(hist, first[5])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.boundary_score(pred, labels, 19, 255, 9, hist)
    hist.zero_()
    pred.copy_(second[0])
    labels.copy_(second[1])
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    got = hist.clone()
    del graph
    want = M.literal_boundary_histograms(second[0], second[1], 19, 255, 9)
    assert torch.equal(got, 2 * want) and not torch.equal(want, first[5])


# ------------------------------------------------------------------------------------------------ tester end to end
class _Lines:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)

    warning = info


def _run_tester(out, *opts):
    """ASPPTester on a [1, 1, 2, 2] bottleneck backbone + ASPP with formula weights over two synthetic 161 x 97 images, with --saveres (the set-up
    of tests/test_gpu_crf.py).  Returns the confusion matrix, its JSON, the log, the saved masks, the tester and the batches."""
    from PIL import Image
    from core.configs import cfg as global_cfg
    from core.datasets.build import build_dataset
    from core.testers.aspp_tester import ASPPTester
    from rnd_semantic_segmentation_amd.host import modules

    class Small(ASPPTester):
        build_feature_extractor = staticmethod(lambda cfg: modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False,
                                                                                             layers=(1, 1, 2, 2)))

    out.mkdir()
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["MODEL.FREEZE_BN", True, "MODEL.NUM_CLASSES", 19, "OUTPUT_DIR", str(out), "INPUT.INPUT_SIZE_TEST", (161, 97),
                         "PSEUDO_DIR", str(out / "pseudo"), "DATASETS.TEST", "cityscapes_val"] + list(opts))
    os.environ["MI_SYNTH_LEN"] = "2"
    try:
        data = build_dataset(cfg, mode="test", is_source=False)
        batches = list(torch.utils.data.DataLoader(data, batch_size=1, shuffle=False))
        log = _Lines()
        palette = [(5 * i) % 256 for i in range(768)]
        tester = Small(cfg, torch.device("cuda"), batches, log, palette, {i: "c%d" % i for i in range(19)}, saveres=True)
    finally:
        os.environ.pop("MI_SYNTH_LEN", None)
    synth.load_formula_weights(tester.feature_extractor)
    synth.load_formula_weights(tester.classifier)
    cmt = tester.test()
    folder = out / "pseudo" / "inference" / "cityscapes_val"
    masks = [np.array(Image.open(io.BytesIO((folder / f).read_bytes()))) for f in sorted(os.listdir(folder)) if f.endswith(".png")]
    return cmt, (out / "aspp_confusion_matrix.json").read_bytes(), log.lines, masks, tester, batches


_OFF = {}


def _key_off(tmp_path, fused):
    if fused not in _OFF:
        r = _run_tester(tmp_path / ("off-%s" % fused), "TEST.FUSED_SCORE", fused)
        assert not (tmp_path / ("off-%s" % fused) / "aspp_boundary_metrics.json").exists() and not any("oundary" in s for s in r[2])
        _OFF[fused] = r[:4]
    return _OFF[fused]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "literal"])
@pytest.mark.parametrize("widths", [(), (1, 3, 9)], ids=["two-percent", "three-widths"])
def test_aspp_tester_with_the_key_on(tmp_path, fused, widths):
    cmt, cmt_json, lines, masks, tester, batches = _run_tester(tmp_path / "on", "TEST.BOUNDARY", True, "TEST.BOUNDARY_WIDTHS", widths,
                                                               "TEST.FUSED_SCORE", fused)
    off = _key_off(tmp_path, fused)
    assert torch.equal(cmt, off[0]) and int(cmt.sum()) > 0 and cmt_json == off[1]            # the region metrics do not notice the key
    assert len(masks) == 2 and all(np.array_equal(a, b) for a, b in zip(masks, off[3]))
    assert [s for s in lines if "oundary" not in s] == off[2]
    want_widths = list(widths) if widths else [4]                                            # 2 % of hypot(97, 161) = 3.76
    D = want_widths[-1]
    want = torch.zeros(5, 19, D + 1, dtype=torch.int64)
    for mask, (x, y, _) in zip(masks, batches):
        assert tuple(y.shape[-2:]) == (97, 161) == mask.shape
        want += M.literal_boundary_histograms(torch.from_numpy(mask), y[0].long(), 19, 255, D)
    assert torch.equal(tester.boundary_hist, want) and not tester.boundary_hist.is_cuda
    table = json.loads((tmp_path / "on" / "aspp_boundary_metrics.json").read_text())
    summary = M.boundary_summary(want, want_widths, ["c%d" % i for i in range(19)])
    assert {k: table[k] for k in summary} == summary
    assert table["widths"] == want_widths and table["max_width"] == D and table["hist"] == want.tolist()
    assert table["classes"][3] == "c3" and len(table["boundary_iou"]) == len(want_widths) and len(table["boundary_iou"][0]) == 19
    present = [v for v in table["trimap_iou"][-1] if v is not None]
    assert present and table["mean_trimap_iou"][-1] == sum(present) / len(present)
    assert sum("Boundary metric" in s for s in lines) == len(want_widths) * 20 and sum("TEST.BOUNDARY" in s for s in lines) == 1
    print("tester %s widths %s: mean Boundary IoU %s, mean trimap IoU %s, %d of 19 classes present"
          % ("fused" if fused else "literal", want_widths, table["mean_boundary_iou"], table["mean_trimap_iou"], len(present)))


def test_mixed_label_sizes_need_explicit_widths():
    from rnd_semantic_segmentation_amd.host.tester import ASPPTester
    t = ASPPTester.__new__(ASPPTester)
    t.cfg = type("C", (), {"MODEL": type("M", (), {"NUM_CLASSES": 3})(), "INPUT": type("I", (), {"IGNORE_LABEL": 255})()})()
    t.logger, t.boundary, t.boundary_hist, t.boundary_size = _Lines(), (), None, None
    pred = torch.zeros(20, 30, dtype=torch.uint8, device="cuda")
    t._boundary_count(pred, pred.long())
    t._boundary_count(pred, pred.long())
    assert int(t.boundary_hist[0].sum()) == 1200 and t.boundary_widths == (1,)
    with pytest.raises(ValueError, match="TEST.BOUNDARY_WIDTHS"):
        t._boundary_count(pred[:10].contiguous(), pred[:10].long().contiguous())
    t.boundary, t.boundary_hist = (2, 5), None                                                # explicit widths: any size
    t._boundary_count(pred, pred.long())
    t._boundary_count(pred[:10].contiguous(), pred[:10].long().contiguous())
    assert int(t.boundary_hist[0].sum()) == 900 and tuple(t.boundary_hist.shape) == (5, 3, 6)


def test_other_testers_refuse_the_key_on_the_gpu(tmp_path):
    from core.configs import cfg as global_cfg
    from core.testers.gald_tester import GALDTester
    from core.testers.pranet_tester import PranetTester
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["MODEL.NUM_CLASSES", 19, "OUTPUT_DIR", str(tmp_path), "TEST.BOUNDARY", True])
    with pytest.raises(NotImplementedError, match="TEST.BOUNDARY"):
        PranetTester(cfg, torch.device("cuda"), [], _Lines())
    with pytest.raises(NotImplementedError, match="TEST.BOUNDARY"):
        GALDTester(cfg, torch.device("cuda"), [], _Lines(), [0] * 57)
