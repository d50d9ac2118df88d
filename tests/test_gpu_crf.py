"""GPU side of the CRF refinement (TEST.CRF): mi_crf_refine (csrc/crf.hip) against the float64 restatement of tests/_crf_ref.py.  The bound of every
case is CRF_FACTOR (16) times what the same restatement, run in float32 on the CPU, deviates from float64 on that case - computed here, not
hard-coded.  pred / conf are checked wherever the oracle's top-two margin exceeds that bound (at most 1 % of the pixels may fall under it).
Then bit-reproducibility, independence of the outputs, the refusals, one graph capture, and ASPPTester on a small backbone with the key on.
Every test prints the figures it asserts on."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import _crf_ref as ref
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

K = None
M = None
CS = (58.395, 57.12, 57.375)
# (K, B, H, W, window, dilation, iters)
CASES = [
    (19, 1, 13, 21, 5, 2, 3),        # halo larger than a third of the image
    (19, 2, 37, 53, 7, 4, 5),        # the defaults, odd sizes, the batch stride
    (3, 1, 9, 70, 7, 1, 5),          # wide and thin
    (2, 1, 40, 40, 3, 6, 10),        # dilation beyond the window
    (32, 1, 17, 19, 11, 1, 2),       # most classes, 120 neighbours
    (19, 1, 70, 150, 7, 4, 2),       # several tiles both ways
    (4, 1, 5, 40, 7, 4, 2),          # most vertical neighbours outside
    (5, 1, 1, 1, 3, 1, 2),           # no neighbour at all: both normalisers 0, the result is softmax(U)
    (19, 2, 37, 53, 7, 4, 0),        # iters = 0: the early return
]


@pytest.fixture(scope="module", autouse=True)
def _kern():
    global K, M
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rnd_semantic_segmentation_amd import kernels
    from rnd_semantic_segmentation_amd.host import metrics
    K, M = kernels, metrics
    yield


def _params(window, dilation, iters):
    return dict(ref.DEFAULTS, window=window, dilation=dilation, iters=iters)


_REFERENCE = {}


def _reference(key, probs, image, par):
    """(oracle float64, bound) of one case, computed once and left unchanged: bound = CRF_FACTOR * max |float32 restatement - float64|."""
    if key not in _REFERENCE:
        f64 = ref.crf_ref(probs, image, CS, dtype=torch.float64, **par)
        f32 = ref.crf_ref(probs, image, CS, dtype=torch.float32, **par)
        dev = float((f32.double() - f64).abs().max())
        _REFERENCE[key] = (f64, dev, ref.CRF_FACTOR * dev)
    return _REFERENCE[key]


def _check(tag, probs, image, par):
    """Runs the kernel with all three outputs and checks them against the oracle; returns the CrfResult."""
    f64, dev, bound = _reference(tag, probs, image, par)
    assert dev > 0, "the float32 restatement reproduces float64 exactly: no yardstick"
    r = K.crf_refine(probs.cuda(), image.cuda(), CS, want_probs=True, want_pred=True, want_conf=True, **par)
    got = r.probs.cpu().double()
    assert bool(torch.isfinite(got).all())
    err = float((got - f64).abs().max())
    top = f64.topk(min(2, f64.shape[1]), dim=1)
    margin = top.values[:, 0] - top.values[:, 1] if f64.shape[1] > 1 else torch.ones_like(top.values[:, 0])
    ok = margin > bound
    excluded = int((~ok).sum())
    moved = float((f64.argmax(1) != probs.argmax(1)).float().mean())
    conf_err = float((r.conf.cpu().double() - top.values[:, 0]).abs().max())
    print("crf %s: |kernel - f64| %.3g, float32 restatement %.3g, ratio %.2f (bound %.0f); conf %.3g; %d of %d pixels under the margin; the CRF moves "
          "%.1f %% of the pixels" % (tag, err, dev, err / dev, ref.CRF_FACTOR, conf_err, excluded, ok.numel(), 100 * moved))
    assert err <= bound, (err, bound)
    assert excluded <= 0.01 * ok.numel(), (excluded, ok.numel())
    assert torch.equal(r.pred.cpu().long()[ok], top.indices[:, 0][ok])
    assert conf_err <= bound, (conf_err, bound)
    assert r.pred.dtype == torch.uint8 and r.conf.dtype == torch.float32 and r.probs.shape == probs.shape
    return r


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_refine_matches_the_float64_oracle(case):
    Kc, B, H, W, window, dilation, iters = case
    probs, image = ref.crf_inputs(Kc, B, H, W, seed=sum(case))
    r = _check(case, probs, image, _params(window, dilation, iters))
    # pred / conf are the argmax / max of the very probabilities the call returns: lowest index among the maxima
    p = r.probs.cpu()
    assert torch.equal(r.pred.cpu().long(), p.argmax(1)) or torch.equal(p.gather(1, r.pred.cpu().long().unsqueeze(1))[:, 0], p.max(1).values)
    assert torch.equal(r.conf.cpu(), p.max(1).values)
    if (H, W) == (1, 1) or iters == 0:
        assert float((p.double() - torch.softmax(torch.log(torch.clamp(probs.double(), min=ref.EPS)), 1)).abs().max()) < 1e-6


def test_uniform_image_and_hard_probabilities_stay_finite():
    """Exact zeros and ones in the input: the eps clamp; a uniform image: gc = 1 everywhere."""
    Kc, H, W = 4, 23, 45
    region = (torch.arange(W).reshape(1, W) // 12 + torch.arange(H).reshape(H, 1) // 9) % Kc
    probs = torch.nn.functional.one_hot(region, Kc).permute(2, 0, 1).unsqueeze(0).float().contiguous()
    noise = torch.rand((1, Kc, H, W), generator=torch.Generator().manual_seed(7))
    probs = torch.where(noise[:, :1] > 0.85, torch.softmax(4 * noise, 1), probs).contiguous()      # some soft pixels among the hard ones
    assert int((probs == 0).sum()) > 0 and int((probs == 1).sum()) > 0
    image = torch.full((1, 3, H, W), 0.25)
    r = _check("uniform", probs, image, _params(7, 4, 5))
    assert bool(torch.isfinite(r.probs).all()) and bool(torch.isfinite(r.conf).all())


def test_two_calls_give_equal_bits_and_outputs_do_not_depend_on_each_other():
    probs, image = ref.crf_inputs(19, 2, 37, 53, seed=99)
    probs, image = probs.cuda(), image.cuda()
    par = _params(7, 4, 5)
    a = K.crf_refine(probs, image, CS, want_probs=True, want_pred=True, want_conf=True, **par)
    b = K.crf_refine(probs, image, CS, want_probs=True, want_pred=True, want_conf=True, **par)
    assert torch.equal(a.probs, b.probs) and torch.equal(a.pred, b.pred) and torch.equal(a.conf, b.conf)
    for wp, wd, wc in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        r = K.crf_refine(probs, image, CS, want_probs=wp, want_pred=wd, want_conf=wc, **par)
        assert (r.probs is None) == (not wp) and (r.pred is None) == (not wd) and (r.conf is None) == (not wc)
        assert (not wp or torch.equal(r.probs, a.probs)) and (not wd or torch.equal(r.pred, a.pred)) and (not wc or torch.equal(r.conf, a.conf))
    z = K.crf_refine(probs, image, CS, want_probs=False, want_pred=True, **_params(7, 4, 0))           # iters 0 with a side output only
    assert torch.equal(z.pred, K.crf_refine(probs, image, CS, want_pred=True, **_params(7, 4, 0)).pred)


def test_refusals_leave_the_outputs_untouched():
    from rnd_semantic_segmentation_amd import _lib
    from rnd_semantic_segmentation_amd._lib import MiError
    lib = _lib.lib()
    Kc, H, W = 19, 12, 20
    probs, image = [t.cuda() for t in ref.crf_inputs(Kc, 1, H, W, seed=5)]
    out = torch.full((1, Kc, H, W), -7.0, device="cuda")
    pred = torch.full((1, H, W), 77, dtype=torch.uint8, device="cuda")
    conf = torch.full((1, H, W), -7.0, device="cuda")
    ws = torch.empty(lib.mi_crf_workspace(1, Kc, H, W), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731

    def call(**kw):
        a = dict(out=out, pred=pred, conf=conf, K=Kc, H=H, W=W, B=1, iters=5, window=7, dilation=4, pos_w=3.0, pos_xy=3.0, bi_w=10.0, bi_xy=80.0,
                 bi_rgb=13.0, ws_bytes=ws.numel())
        a.update(kw)
        return lib.mi_crf_refine(p(probs), p(image), *CS, p(a["out"]), p(a["pred"]), p(a["conf"]), a["B"], a["K"], a["H"], a["W"], a["iters"], a["window"],
                                 a["dilation"], a["pos_w"], a["pos_xy"], a["bi_w"], a["bi_xy"], a["bi_rgb"], p(ws), a["ws_bytes"], None)

    nan, inf = float("nan"), float("inf")
    refusals = [(dict(K=0), -22), (dict(K=33), -22), (dict(window=6), -22), (dict(window=1), -22), (dict(window=13), -22), (dict(dilation=0), -22),
                (dict(dilation=17), -22), (dict(iters=-1), -22), (dict(iters=33), -22), (dict(pos_xy=0.0), -22), (dict(bi_xy=-1.0), -22),
                (dict(bi_rgb=nan), -22), (dict(pos_w=-1.0), -22), (dict(bi_w=inf), -22), (dict(pos_w=nan), -22),
                (dict(B=2, H=32768, W=32768), -22), (dict(ws_bytes=ws.numel() - 1), -12), (dict(out=None, pred=None, conf=None), -22)]
    for kw, code in refusals:
        assert call(**kw) == code and lib.mi_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((pred == 77).all()) and bool((conf == -7.0).all())
    assert call() == 0                                                       # the same arguments, nothing refused
    torch.cuda.synchronize()
    assert bool((out >= 0).all()) and bool((pred < Kc).all()) and bool((conf > 0).all())
    with pytest.raises(MiError, match="window"):
        K.crf_refine(probs, image, CS, **_params(4, 1, 1))
    with pytest.raises(MiError, match="image"):
        K.crf_refine(probs, image[:, :2].contiguous(), CS, **_params(3, 1, 1))
    with pytest.raises(MiError, match="GPU"):
        K.crf_refine(probs.cpu(), image.cpu(), CS, **_params(3, 1, 1))


def test_graph_capture_and_replay_with_changed_inputs():
    par = _params(7, 4, 5)
    first = [t.cuda() for t in ref.crf_inputs(19, 1, 37, 53, seed=1)]
    second = [t.cuda() for t in ref.crf_inputs(19, 1, 37, 53, seed=2)]
    probs, image = first[0].clone(), first[1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up off the capture
        K.crf_refine(probs, image, CS, want_pred=True, want_conf=True, **par)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = K.crf_refine(probs, image, CS, want_pred=True, want_conf=True, **par)
    probs.copy_(second[0])
    image.copy_(second[1])
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in held]
    del graph
    eager = K.crf_refine(second[0], second[1], CS, want_pred=True, want_conf=True, **par)
    assert all(torch.equal(g, e) for g, e in zip(got, eager))
    assert not torch.equal(eager.probs, K.crf_refine(first[0], first[1], CS, **par).probs)


def test_refine_output_resizes_the_image_to_the_label():
    probs, _ = ref.crf_inputs(19, 1, 37, 53, seed=11)
    _, small = ref.crf_inputs(19, 2, 19, 27, seed=12)
    probs, small = probs.cuda(), small.cuda()
    par = _params(7, 4, 2)
    got = M.crf_refine_output(probs, small, (37, 53), CS, par)
    want = K.crf_refine(probs, K.image_resize_ac(small[:1].contiguous(), (37, 53)), CS, **par).probs
    assert torch.equal(got, want) and got.shape == (1, 19, 37, 53)


# ------------------------------------------------------------------------------------------------ tester end to end
class _Lines:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)

    warning = info


def _run_tester(out, monkeypatch, *opts):
    """ASPPTester on a [1, 1, 2, 2] bottleneck backbone + ASPP with formula weights over two synthetic 161 x 97 images, with --saveres (the set-up of
    tests/test_gpu_classwise.py on a smaller net).  Returns the confusion matrix, its JSON, the log, the saved files, the tester, the batches and
    what went into / came out of every refinement."""
    from core.configs import cfg as global_cfg
    from core.datasets.build import build_dataset
    from core.testers.aspp_tester import ASPPTester
    from rnd_semantic_segmentation_amd.host import modules
    from rnd_semantic_segmentation_amd.host import tester as te

    class Small(ASPPTester):
        build_feature_extractor = staticmethod(lambda cfg: modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False,
                                                                                             layers=(1, 1, 2, 2)))

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
        tester = Small(cfg, torch.device("cuda"), batches, log, palette, {i: str(i) for i in range(19)}, saveres=True)
    finally:
        os.environ.pop("MI_SYNTH_LEN", None)
    synth.load_formula_weights(tester.feature_extractor)
    synth.load_formula_weights(tester.classifier)
    calls = []
    real = te.crf_refine_output

    def spy(output, image, size, cs, settings):
        refined = real(output, image, size, cs, settings)
        calls.append((output.detach().cpu().clone(), image.detach().cpu().clone(), tuple(size), tuple(cs), dict(settings), refined.detach().cpu().clone()))
        return refined

    monkeypatch.setattr(te, "crf_refine_output", spy)
    cmt = tester.test()
    monkeypatch.setattr(te, "crf_refine_output", real)
    folder = out / "pseudo" / "inference" / "cityscapes_val"
    files = {f: (folder / f).read_bytes() for f in sorted(os.listdir(folder))} if folder.exists() else {}
    return cmt, (out / "aspp_confusion_matrix.json").read_bytes(), log.lines, files, tester, batches, calls


_TESTER_REFERENCE = {}


def _tester_reference(calls, batches):
    """Per image of pass 1: (float32 restatement of the refinement of the literal path's output, the mask of the pixels the margin rule keeps, the
    bound).  The literal output is the same for every configuration of the key: computed once."""
    if "ref" not in _TESTER_REFERENCE:
        refs = []
        for (output, image, size, cs, settings, _), (x, y, _) in zip(calls, batches):
            assert tuple(output.shape[-2:]) == size == tuple(y.shape[-2:]) and settings == ref.DEFAULTS
            assert cs == pytest.approx((0.229 * 255, 0.224 * 255, 0.225 * 255))
            x0 = x[:1].float()
            if tuple(x0.shape[-2:]) != size:
                x0 = torch.nn.functional.interpolate(x0, size=size, mode="bilinear", align_corners=True)
            f64 = ref.crf_ref(output, x0, cs, dtype=torch.float64, **settings)
            f32 = ref.crf_ref(output, x0, cs, dtype=torch.float32, **settings)
            bound = ref.CRF_FACTOR * float((f32.double() - f64).abs().max())
            top = f64.topk(2, dim=1).values
            refs.append((f32, (top[:, 0] - top[:, 1] > bound)[0], bound))
        _TESTER_REFERENCE["ref"] = refs
    return _TESTER_REFERENCE["ref"]


def _masks(files):
    from PIL import Image
    return [np.array(Image.open(io.BytesIO(b))) for name, b in sorted(files.items()) if name.endswith(".png")]


@pytest.mark.parametrize("tag,opts", [("argmax", ()), ("threshold", ("TEST.PSEUDO_THRESHOLD", 0.9)), ("classwise", ("TEST.PSEUDO_CLASSWISE", True))])
def test_aspp_tester_with_the_key_on(tmp_path, monkeypatch, tag, opts):
    cmt, _, lines, files, tester, batches, calls = _run_tester(tmp_path, monkeypatch, "TEST.CRF", True, "TEST.FUSED_SCORE", True, *opts)
    assert len(calls) == (4 if tag == "classwise" else 2)                     # every literal output went through the refinement; both passes
    assert sum("TEST.CRF" in s and "literal path" in s for s in lines) == 1
    refs = _tester_reference(calls[:2], batches)
    masks = _masks(files)
    assert len(masks) == 2
    want_cmt = torch.zeros(19, 19, dtype=torch.int64)
    loose = 0
    hist = torch.zeros(19, M.PSEUDO_BINS, dtype=torch.int64)
    near_edge = 0
    for i, ((f32, keep, bound), (x, y, _)) in enumerate(zip(refs, batches)):
        refined = calls[i][5]                                                 # kernel and yardstick both lie within `bound` of the oracle: 2 * bound apart at most
        assert float((refined.double() - f32.double()).abs().max()) <= 2 * bound      # kernel and yardstick each within the bound of the oracle
        top = f32.max(1)
        pred, best = top[1][0], top[0][0]
        excluded = int((~keep).sum())
        assert excluded <= 0.01 * keep.numel(), (excluded, keep.numel())
        loose += excluded
        want_cmt += M.confusion_matrix(tester.cfg, pred.flatten(), y[0].long().flatten())
        if tag == "argmax":
            want = pred
            sure = keep
        elif tag == "threshold":
            want = torch.where(best >= 0.9, pred, torch.full_like(pred, 255))
            sure = keep & ((best - 0.9).abs() > 2 * bound)
        else:
            t = torch.from_numpy(tester.class_thresholds)[pred]
            want = torch.where(best >= t, pred, torch.full_like(pred, 255))
            sure = keep & ((best - t).abs() > 2 * bound)
            hist += M.literal_histogram(f32, 19)
            scaled = best.double() * M.PSEUDO_BINS
            near_edge += int((~keep | ((scaled - scaled.round()).abs() <= 2 * bound * M.PSEUDO_BINS)).sum())
        got = torch.from_numpy(masks[i].astype(np.int64))
        print("crf tester %s image %d: %d pixels under the margin, %d more near a threshold, %d of %d saved pixels are 255, mask differs in %d"
              % (tag, i, excluded, int((keep & ~sure).sum()), int((got == 255).sum()), got.numel(), int((got != want).sum())))
        assert torch.equal(got[sure], want[sure])
        assert int((~sure).sum()) <= 0.02 * sure.numel()
        if tag == "classwise":                                                # the median rule splits every class; 0.9 is above this small net's confidences
            assert 0 < int((got == 255).sum()) < got.numel()
    assert int(cmt.sum()) == int(want_cmt.sum()) > 0
    assert int((cmt - want_cmt).abs().sum()) <= 2 * loose, (int((cmt - want_cmt).abs().sum()), loose)
    if tag == "classwise":
        assert "class_thresholds.json" in files and int(tester.class_hist.sum()) == int(hist.sum())
        assert int((tester.class_hist - hist).abs().sum()) <= 2 * near_edge, (int((tester.class_hist - hist).abs().sum()), near_edge)
        cap = 1.0
        assert np.array_equal(tester.class_thresholds, M.class_thresholds(tester.class_hist, 0.5, cap))


def test_aspp_tester_with_the_key_off_is_todays_flow(tmp_path, monkeypatch):
    (tmp_path / "fused").mkdir()
    (tmp_path / "literal").mkdir()
    f = _run_tester(tmp_path / "fused", monkeypatch, "TEST.CRF", False, "TEST.FUSED_SCORE", True)
    lit = _run_tester(tmp_path / "literal", monkeypatch, "TEST.FUSED_SCORE", False)
    assert len(f[6]) == 0 and len(lit[6]) == 0                                # no refinement anywhere
    assert torch.equal(f[0], lit[0]) and int(f[0].sum()) > 0 and f[1] == lit[1] and f[2] == lit[2] and f[3] == lit[3] and len(f[3]) == 2
    assert not any("CRF" in s for s in f[2])


def test_other_testers_refuse_the_key_on_the_gpu(tmp_path):
    from core.configs import cfg as global_cfg
    from core.testers.gald_tester import GALDTester
    from core.testers.pranet_tester import PranetTester
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["MODEL.NUM_CLASSES", 19, "OUTPUT_DIR", str(tmp_path), "TEST.CRF", True])
    with pytest.raises(NotImplementedError, match="TEST.CRF"):
        PranetTester(cfg, torch.device("cuda"), [], _Lines())
    with pytest.raises(NotImplementedError, match="TEST.CRF"):
        GALDTester(cfg, torch.device("cuda"), [], _Lines(), [0] * 57)
