"""Host-side utilities the DeepLab path uses from the reference's core/utils/utility.py and
core/utils/adapt_lr.py, re-stated (same names, argument meaning and outputs).

Differences that are deliberate and documented:
 * intersectionAndUnionGPU / confusion_matrix use integer bincount on the tensor's own device (the
   reference runs float histc on CPU and a per-pixel Python loop, utility.py:157-159, :347-359);
   the integers produced are identical (tests/test_host_logic.py pins them to the reference's outputs).
 * setup_logger creates OUTPUT_DIR (the reference crashes if it is missing, utility.py:243).
 * strip_prefix_if_present works when the prefix is present (the reference forgets to import
   OrderedDict, utility.py:167).
 * inference() runs the upsample + softmax tail in one HIP kernel (mi_upsample_softmax).
 * multi_scale_inference() on the engine runs one resize (+ mirror) launch and one backbone + head pass per scale, then ONE kernel
   (mi_upsample_softmax_multi) that interpolates every low-resolution logit map, takes the softmax, sums in the reference's order and
   divides: the result is written once instead of being accumulated through full-size tensors.
 * predict_and_score() on the engine never builds the probability map: mi_upsample_predict_score takes the argmax of the same per-pixel values in
   registers, applies the pseudo-label threshold and counts the confusion matrix and the areas against the label in the same launch.
 * class-wise pseudo-label thresholds (PSEUDO_BINS, confidence_bin, class_thresholds, classwise_settings; TEST.PSEUDO_CLASSWISE) are not in the
   reference: the class-balanced rule of CBST / BDL / FADA self-distillation, stated in exact integers on a confidence histogram which the same
   kernel accumulates (mi_upsample_predict_score_cw).
 * the polyp metrics (polyp_image_stats, PolypMeter, polyp_settings; TEST.POLYP_METRICS) are not in the reference either: mean Dice / IoU,
   F-beta, E-measure, S-measure and MAE as PraNet and its successors report them on Kvasir, derived in float64 from the per-image histogram
   and moment sums of mi_polyp_score - the host never sees the probability map.
 * the CRF refinement (crf_settings, crf_channel_scale, crf_refine_output; TEST.CRF) is not in the reference either: the locally connected
   form of DeepLabV2's CRF stage, one HIP kernel family (mi_crf_refine) on the literal path's probability map.
 * sliding-window evaluation (slide_plan, slide_windows, slide_inference, slide_settings; TEST.SLIDE) is not in the reference either: the
   protocol DeepLab and PSPNet report Cityscapes under - crop-sized windows slid over the full-resolution picture, each evaluated as
   inference() evaluates a picture, averaged where they overlap.  slide_inference is the literal composition; predict_and_score(slide=...)
   on the engine runs the windows' backbone passes and then ONE kernel (mi_upsample_predict_score_slide).
 * the boundary metrics (boundary_survival, literal_boundary_histograms, boundary_summary, boundary_settings; TEST.BOUNDARY) are not in the
   reference either: Boundary IoU (Cheng et al., CVPR 2021) and DeepLab's trimap IoU at every band width up to 64 from five integer
   histograms of erosion counts, which mi_boundary_score adds up on the device in two launches per picture.
 * the surface-distance metrics (surface_image_stats, SurfaceMeter, literal_surface_stats, surface_settings; TEST.SURFACE_METRICS) are not in
   the reference either: Hausdorff distance, its percentile, average symmetric surface distance and surface Dice in medpy's conventions,
   from 27 integers and two sums per image which mi_surface_score computes exactly on the device - the host never sees a distance map.
"""
import json
import logging
import math
import os
import types
from collections import OrderedDict, defaultdict, deque

import numpy as np
import torch


# ----------------------------------------------------------------------------- learning rate (adapt_lr.py:12-17)
def adjust_learning_rate(method, base_lr, iters, max_iter, power):
    if method == "poly":
        return base_lr * ((1 - float(iters) / max_iter) ** power)
    raise NotImplementedError(method)


# ----------------------------------------------------------------------------- meters (utility.py:24-131)
class AverageMeter(object):
    """Per-class intersection / union / target / output accumulators; macro = mean over images of per-image
    ratios, micro = ratio of sums (utility.py:24-72)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.intersection_sum = 0
        self.union_sum = 0
        self.target_sum = 0
        self.res_sum = 0
        self.count = 0
        self.iou_sum = 0
        self.f1_sum = 0

    def update(self, intersection, union, target, res):
        self.iou_sum = self.iou_sum + intersection / (union + 1e-10)
        self.f1_sum = self.f1_sum + 2 * intersection / (target + res + 1e-10)
        self.intersection_sum = self.intersection_sum + intersection
        self.union_sum = self.union_sum + union
        self.target_sum = self.target_sum + target
        self.res_sum = self.res_sum + res
        self.count += 1

    def results(self):
        n = float(self.count)
        macro_f1, macro_iou = self.f1_sum / n, self.iou_sum / n
        micro_f1 = 2 * self.intersection_sum / (self.target_sum + self.res_sum + 1e-10)
        micro_iou = self.intersection_sum / (self.union_sum + 1e-10)
        return dict(macro_iou=macro_iou, macro_f1=macro_f1, micro_iou=micro_iou, micro_f1=micro_f1)

    def summary(self, logger, num_classes=2):
        r = self.results()
        logger.info("Macro metric, val result: mIoU/mF1 {:.4f}/{:.4f}.".format(np.mean(r["macro_iou"]), np.mean(r["macro_f1"])))
        logger.info("Micro metric, val result: mIoU/mF1 {:.4f}/{:.4f}.".format(np.mean(r["micro_iou"]), np.mean(r["micro_f1"])))
        for i in range(num_classes):
            logger.info("Macro metric, class {} iou/f1 score: {:.4f}/{:.4f}.".format(i, r["macro_iou"][i], r["macro_f1"][i]))
            logger.info("Micro metric, class {} iou/f1 score: {:.4f}/{:.4f}.".format(i, r["micro_iou"][i], r["micro_f1"][i]))


class SmoothedValue(object):
    def __init__(self, window_size=20):
        self.deque = deque(maxlen=window_size)
        self.series = []
        self.total = 0.0
        self.count = 0

    def update(self, value):
        self.deque.append(value)
        self.series.append(value)
        self.count += 1
        self.total += value

    @property
    def median(self):
        return torch.tensor(list(self.deque)).median().item()

    @property
    def avg(self):
        return torch.tensor(list(self.deque)).mean().item()

    @property
    def global_avg(self):
        return self.total / self.count


class MetricLogger(object):
    def __init__(self, delimiter="\t"):
        self.meters = defaultdict(SmoothedValue)
        self.delimiter = delimiter

    def update(self, **kwargs):
        for k, v in kwargs.items():
            if isinstance(v, torch.Tensor):
                v = v.item()
            assert isinstance(v, (float, int))
            self.meters[k].update(v)

    def __getattr__(self, attr):
        if attr in self.__dict__.get("meters", {}):
            return self.meters[attr]
        raise AttributeError("'{}' object has no attribute '{}'".format(type(self).__name__, attr))

    def __str__(self):
        return self.delimiter.join("{}: {:.4f} ({:.4f})".format(n, m.median, m.global_avg) for n, m in self.meters.items())


# ----------------------------------------------------------------------------- segmentation metrics
def _hist(values, K):
    values = values[(values >= 0) & (values < K)]
    return torch.bincount(values, minlength=K)[:K]


def intersectionAndUnionGPU(output, target, K, ignore_index=255):
    """utility.py:148-161.  Returns float32 tensors (area_intersection, area_union, area_target, area_output)
    on the inputs' device; like the reference it overwrites `output` where target is ignored."""
    assert output.dim() in [1, 2, 3]
    assert output.shape == target.shape
    output = output.reshape(-1)
    target = target.reshape(-1)
    output[target == ignore_index] = ignore_index
    inter = output[output == target]
    ai = _hist(inter.long(), K).float()
    ao = _hist(output.long(), K).float()
    at = _hist(target.long(), K).float()
    return ai, ao + at - ai, at, ao


def intersectionAndUnion(output, target, K, ignore_index=255):
    """numpy twin, utility.py:133-145."""
    output = np.asarray(output).reshape(-1).copy()
    target = np.asarray(target).reshape(-1)
    output[target == ignore_index] = 255
    inter = output[output == target]
    ai, _ = np.histogram(inter, bins=np.arange(K + 1))
    ao, _ = np.histogram(output, bins=np.arange(K + 1))
    at, _ = np.histogram(target, bins=np.arange(K + 1))
    return ai, ao + at - ai, at, ao


def confusion_matrix(cfg, pd, gt):
    """utility.py:347-359: cmt[gt, pd] += 1 where gt != 255, int64 [K,K] on CPU."""
    K = cfg.MODEL.NUM_CLASSES
    pd = pd.reshape(-1).long()
    gt = gt.reshape(-1).long()
    keep = (gt != 255) & (gt >= 0) & (gt < K) & (pd >= 0) & (pd < K)
    return torch.bincount(gt[keep] * K + pd[keep], minlength=K * K).reshape(K, K).cpu()


def strip_prefix_if_present(state_dict, prefix):
    keys = sorted(state_dict.keys())
    if not all(key.startswith(prefix) for key in keys):
        return state_dict
    return OrderedDict((key.replace(prefix, ""), value) for key, value in state_dict.items())


def inference(feature_extractor, classifier, image, label, flip=True):
    """utility.py:179-191: 1/8-resolution logits -> bilinear(align_corners) to the LABEL size -> softmax,
    image 0 only ([1,K,H,W]); flip averages the horizontally mirrored pass."""
    size = tuple(label.shape[-2:])
    if flip:
        image = torch.cat([image, torch.flip(image, [3])], 0)
    with torch.no_grad():
        feat = feature_extractor(image)
        if hasattr(classifier, "predict_probs"):            # fused upsample + softmax kernel
            probs = classifier.predict_probs(feat, size)
        else:                                               # a substituted / foreign classifier: the reference's literal tail
            probs = torch.nn.functional.softmax(
                torch.nn.functional.interpolate(classifier(feat), size=size, mode="bilinear", align_corners=True), dim=1)
    if flip:
        out = (probs[0] + probs[1].flip(2)) / 2
    else:
        out = probs[0]
    return out.unsqueeze(dim=0)


def multi_scale_plan(size, flip=True, scales=(0.7, 1.0, 1.3)):
    """What multi_scale_inference (utility.py:193-209) computes for an input of `size` (H, W), as data:
    (sizes, sources, divisors).  sizes[i] = (int(H * s_i), int(W * s_i)) with Python floats (:197); sources = [(i, mirrored)] in
    the order the reference adds them (s0, s0 mirrored, s1, ...); divisors = (len(scales), 2 if flip else 1) applied in that order
    (`output / len(scales) / 2`, :207-209)."""
    scales = list(scales)
    if not scales:
        raise ValueError("multi_scale_inference needs at least one scale")
    H, W = int(size[0]), int(size[1])
    sizes = [(int(H * s), int(W * s)) for s in scales]
    if any(h < 1 or w < 1 for h, w in sizes):
        raise ValueError("scales %r leave no pixels of a %dx%d input" % (scales, H, W))
    sources = [(i, m) for i in range(len(scales)) for m in ((False, True) if flip else (False,))]
    return sizes, sources, (len(scales), 2 if flip else 1)


def multi_scale_inference(feature_extractor, classifier, image, label, flip=True, scales=[0.7, 1.0, 1.3]):
    """utility.py:193-209: inference(flip=False) of the image resized (bilinear, align_corners) to every scale and, with flip, of its
    horizontal mirror (prediction mirrored back), averaged; [1,K,H,W] fp32 for image 0 at the LABEL's size."""
    sizes, sources, (div_a, div_b) = multi_scale_plan(image.shape[-2:], flip, scales)
    if hasattr(classifier, "predict_probs_multi") and image.is_cuda:
        from .. import kernels
        x0 = image[:1].float().contiguous()                 # inference() keeps image 0 only (utility.py:190)
        with torch.no_grad():
            feats = [feature_extractor(kernels.image_resize_ac(x0, hw, with_mirror=flip)) for hw in sizes]     # batch 1 or 2 per scale
            mirrors = [(False, True) if flip else (False,)] * len(sizes)
            return classifier.predict_probs_multi(feats, mirrors, tuple(label.shape[-2:]), (div_a, div_b))
    # a substituted / foreign classifier or CPU tensors: the reference's literal composition
    interpolate = torch.nn.functional.interpolate
    resized, output = {}, None
    for i, mirrored in sources:
        if i not in resized:
            resized[i] = interpolate(image, size=sizes[i], mode="bilinear", align_corners=True)
        pred = inference(feature_extractor, classifier, torch.flip(resized[i], [3]) if mirrored else resized[i], label, flip=False)
        if mirrored:
            pred = pred.flip(3)
        output = pred if output is None else output + pred
    output = output / div_a
    return output / div_b if flip else output


# ----------------------------------------------------------------------------- sliding-window evaluation (TEST.SLIDE)
SLIDE_MAX_WINDOWS = 64                  # MI_SLIDE_MAX_WINDOWS of include/mi355seg.h: the descriptors travel in the kernel arguments
SLIDE_CHUNK = 4                         # images per backbone batch of the engine's sliding-window paths
SLIDE_DEFAULTS = OrderedDict((("SLIDE_CROP", (769, 769)), ("SLIDE_STRIDE", (513, 513))))      # TEST.SLIDE_* of host/config.py, (width, height)


def slide_plan(size, crop, stride):
    """The window grid of sliding-window evaluation for an image of size (H, W); crop and stride are (h, w) here.  Returns (rows, cols,
    (wh, ww)): the row origins, the column origins and the one size every window has, (min(ch, H), min(cw, W)).  Per axis of length L:
    n = max(L - c + s - 1, 0) // s + 1 windows; window i starts at i * s, ends at min(i * s + c, L) and its start is then pulled back to
    max(end - c, 0): the first starts at 0, the last ends at L.  Windows are numbered row-major (row origin outer, column origin inner).
    Refused: a non-positive crop, a stride outside 1 .. crop, more than SLIDE_MAX_WINDOWS windows."""
    (H, W), (ch, cw), (sh, sw) = [tuple(int(v) for v in t) for t in (size, crop, stride)]
    if H < 1 or W < 1:
        raise ValueError("slide_plan: empty image %d x %d" % (H, W))
    if ch < 1 or cw < 1:
        raise ValueError("slide_plan: crop %r must be positive" % ((ch, cw),))
    if not (1 <= sh <= ch and 1 <= sw <= cw):
        raise ValueError("slide_plan: stride %r lies outside 1 .. crop %r" % ((sh, sw), (ch, cw)))

    def axis(L, c, s):
        out = []
        for i in range(max(L - c + s - 1, 0) // s + 1):
            b = min(i * s + c, L)
            out.append(max(b - c, 0))
        return out

    rows, cols = axis(H, ch, sh), axis(W, cw, sw)
    if len(rows) * len(cols) > SLIDE_MAX_WINDOWS:
        raise ValueError("slide_plan: %d x %d windows of %r with stride %r over %d x %d exceed the cap of %d windows"
                         % (len(rows), len(cols), (ch, cw), (sh, sw), H, W, SLIDE_MAX_WINDOWS))
    return rows, cols, (min(ch, H), min(cw, W))


def slide_label_factor(image_size, label_size):
    """The whole factor r by which the label is larger than the image, the same on both axes (1024 x 512 input, 2048 x 1024 label: 2)."""
    (H, W), (Hl, Wl) = [tuple(int(v) for v in t) for t in (image_size, label_size)]
    r = Hl // H if H > 0 else 0
    if r < 1 or Hl != r * H or Wl != r * W:
        raise ValueError("sliding-window evaluation needs a label that is a whole multiple of the image, the same on both axes: image %d x %d, "
                         "label %d x %d" % (H, W, Hl, Wl))
    return r


def slide_windows(image_size, label_size, crop, stride):
    """(origins, (wh, ww), r): the image-coordinate origins (y0, x0) of slide_plan's windows in row-major order, their size and the label
    factor.  Window (y0, x0) owns the label rectangle [r*y0, r*(y0+wh)) x [r*x0, r*(x0+ww))."""
    r = slide_label_factor(image_size, label_size)
    rows, cols, window = slide_plan(image_size, crop, stride)
    return [(y0, x0) for y0 in rows for x0 in cols], window, r


def _slide_feats(feature_extractor, image, origins, window, flip):
    """The backbone passes both engine paths of sliding-window evaluation share, so that they feed it identical batches: the crops of image 0
    in window order - with flip every crop followed by its horizontal mirror - in chunks of SLIDE_CHUNK images.  Returns the feature maps."""
    wh, ww = window
    x0 = image[:1]
    crops = []
    for y0, xo in origins:
        c = x0[:, :, y0:y0 + wh, xo:xo + ww]
        crops.append(c)
        if flip:
            crops.append(torch.flip(c, [3]))
    return [feature_extractor(torch.cat(crops[i:i + SLIDE_CHUNK], 0).contiguous()) for i in range(0, len(crops), SLIDE_CHUNK)]


def slide_inference(feature_extractor, classifier, image, label, crop, stride, flip=False):
    """Sliding-window evaluation as DeepLab and PSPNet report Cityscapes: windows of `crop` slid over image 0 with `stride` (both (h, w);
    slide_plan), each evaluated as inference() evaluates a picture - against its rectangle of the label, with (p + p_mirrored.flip) / 2 under
    flip - and the windows' probabilities averaged where they overlap: summed in window order, then one true division by the integer cover
    count.  [1,K,Hl,Wl] fp32 at the LABEL's size, which may be a whole multiple r of the image's.  This literal composition is the
    definition mi_upsample_softmax_slide is held to.  On the engine (a classifier with slide_lows, CUDA tensors) the windows' 1/8-resolution
    logits come from the batches the fused path uses (_slide_feats) and kernels.upsample_softmax turns each into probabilities; a substituted
    / foreign classifier or CPU tensors call inference() per window."""
    size = tuple(label.shape[-2:])
    origins, (wh, ww), r = slide_windows(image.shape[-2:], size, crop, stride)
    canvas = count = None
    engine = hasattr(classifier, "slide_lows") and image.is_cuda
    if engine:
        from .. import kernels
        with torch.no_grad():
            lows, mirror_lows = classifier.slide_lows(_slide_feats(feature_extractor, image, origins, (wh, ww), flip), flip)
    for i, (y0, x0) in enumerate(origins):
        ys, xs = slice(r * y0, r * (y0 + wh)), slice(r * x0, r * (x0 + ww))
        if engine:
            q = kernels.upsample_softmax(lows[i].unsqueeze(0), (r * wh, r * ww), want_pred=False)[0]
            if flip:
                pm = kernels.upsample_softmax(mirror_lows[i].unsqueeze(0), (r * wh, r * ww), want_pred=False)[0]
                q = (q[0] + pm[0].flip(2)) / 2
                q = q.unsqueeze(0)
        else:
            q = inference(feature_extractor, classifier, image[:1, :, y0:y0 + wh, x0:x0 + ww], label[..., ys, xs], flip=flip)
        if canvas is None:
            canvas = torch.zeros((1, q.shape[1]) + size, dtype=q.dtype, device=q.device)
            count = torch.zeros((1, 1) + size, dtype=q.dtype, device=q.device)
        canvas[:, :, ys, xs] += q
        count[:, :, ys, xs] += 1
    return canvas / count


def slide_settings(cfg):
    """None while TEST.SLIDE is False (absent = False), else (crop, stride), each (h, w): TEST.SLIDE_CROP / TEST.SLIDE_STRIDE are written
    (width, height) like the INPUT.*_SIZE_* keys.  A SLIDE_* key that differs from its default while SLIDE is False is refused instead of
    ignored; so is TEST.SCALES other than (1.0,) with SLIDE (multi-scale sliding would need a resize of probability maps the reference does
    not define).  TEST.FLIP is supported."""
    test = cfg.TEST
    on = test["SLIDE"] if "SLIDE" in test else False
    if not isinstance(on, bool):
        raise ValueError("TEST.SLIDE %r must be True or False" % (on,))
    v = OrderedDict((k, tuple(test[k]) if k in test else d) for k, d in SLIDE_DEFAULTS.items())
    if not on:
        stray = [k for k, d in SLIDE_DEFAULTS.items() if v[k] != d]
        if stray:
            raise NotImplementedError("TEST.%s %r belongs to TEST.SLIDE True" % (stray[0], v[stray[0]]))
        return None
    for k, t in v.items():
        if len(t) != 2 or any(isinstance(a, bool) or not isinstance(a, int) for a in t):
            raise ValueError("TEST.%s %r must be two integers (width, height)" % (k, t))
    scales, _ = tta_settings(cfg)
    if scales != (1.0,):
        raise NotImplementedError("TEST.SLIDE with TEST.SCALES %r: sliding-window evaluation is single-scale (TEST.FLIP is supported); leave "
                                  "SCALES at (1.0,)" % (scales,))
    crop, stride = (v["SLIDE_CROP"][1], v["SLIDE_CROP"][0]), (v["SLIDE_STRIDE"][1], v["SLIDE_STRIDE"][0])
    slide_plan(crop, crop, stride)                          # the crop and stride rules, before anything is built
    return crop, stride


def require_no_slide(cfg, who):
    """Sliding-window evaluation is built on the DeepLab evaluation tail: the other testers refuse the key rather than ignore it (a stray
    SLIDE_* key is refused by slide_settings itself)."""
    if slide_settings(cfg) is not None:
        raise NotImplementedError("%s: TEST.SLIDE - sliding-window evaluation exists for the DeepLab (feature extractor, classifier) pair only "
                                  "(ASPPTester); leave it False" % (who,))


# ----------------------------------------------------------------------------- boundary metrics (TEST.BOUNDARY)
BOUNDARY_MAX_WIDTH = 64                 # D of mi_boundary_score (include/mi355seg.h, where the definition stands)
BOUNDARY_MAX_CLASSES = 32
BOUNDARY_MAPS = 5                       # ground-truth bands, prediction bands, Boundary-IoU intersection, trimap intersection, trimap output area


def boundary_width(size):
    """The band width Boundary IoU is published with: 2 % of the picture's diagonal, at least 1 (23 for 512 x 1024, 46 for 1024 x 2048)."""
    return max(1, int(round(0.02 * math.hypot(int(size[0]), int(size[1])))))


def _boundary_check(K, ignore_index, D):
    if not 1 <= K <= BOUNDARY_MAX_CLASSES:
        raise ValueError("boundary metrics: %d classes lie outside 1..%d" % (K, BOUNDARY_MAX_CLASSES))
    if not 1 <= D <= BOUNDARY_MAX_WIDTH:
        raise ValueError("boundary metrics: width %d lies outside 1..%d" % (D, BOUNDARY_MAX_WIDTH))
    if ignore_index is not None and 0 <= ignore_index < K:
        raise ValueError("boundary metrics: ignore_index %d names a class (%d classes)" % (ignore_index, K))


def boundary_survival(L, K, D):
    """e_L of include/mi355seg.h in torch ops: for a class map L [H,W] (values outside [0, K) = no class) the number of 3 x 3 erosions, with
    everything outside the picture background, each pixel survives in the binary mask of its own class, capped at D; int64 [H,W], 0 where L
    has no class.  Literally: the masks of all classes side by side as channels, eroded D times by max_pool2d of the negated, zero-padded mask."""
    K, D = int(K), int(D)
    _boundary_check(K, None, D)
    L = L.reshape(L.shape[-2:]).long()
    m = torch.stack([L == k for k in range(K)]).unsqueeze(0).float()                 # [1,K,H,W]
    e = torch.zeros_like(m)
    for _ in range(D):
        m = -torch.nn.functional.max_pool2d(torch.nn.functional.pad(-m, (1, 1, 1, 1), value=0.0), 3, 1)
        e += m
    return e.sum(1)[0].long()


def literal_boundary_histograms(pred, labels, K, ignore_index, D):
    """What mi_boundary_score adds to hist for one picture, composed from torch ops on the inputs' device: int64 [5, K, D + 1].  The definition
    the kernel is tested against, and the path of CPU tensors."""
    K, D, ignore_index = int(K), int(D), int(ignore_index)
    _boundary_check(K, ignore_index, D)
    labels = labels.reshape(labels.shape[-2:]).long()
    pred = pred.reshape(pred.shape[-2:]).long()
    if pred.shape != labels.shape:
        raise ValueError("boundary metrics: pred %s and labels %s differ in size" % (tuple(pred.shape), tuple(labels.shape)))
    none = torch.full_like(labels, 255)
    G = torch.where((labels >= 0) & (labels < K), labels, none)
    P = torch.where((labels != ignore_index) & (pred >= 0) & (pred < K), pred, none)
    eG, eP = boundary_survival(G, K, D), boundary_survival(P, K, D)
    g, p = G < K, P < K
    hit = g & (G == P)

    def cells(sel, k, e):
        return torch.bincount(k[sel] * (D + 1) + e[sel], minlength=K * (D + 1)).reshape(K, D + 1)

    return torch.stack([cells(g, G, eG), cells(p, P, eP), cells(hit, G, torch.maximum(eG, eP)), cells(hit, G, eG), cells(p & g, P, eG)])


def boundary_accumulate(pred, label, K, ignore_index, D, hist):
    """One picture into the data set's hist (int64 [5, K, D + 1] on the picture's device): mi_boundary_score on the GPU, the literal composition
    for CPU tensors - the same integers."""
    if pred.is_cuda:
        from .. import kernels
        return kernels.boundary_score(pred.to(torch.uint8).contiguous(), label.long().contiguous(), K, ignore_index, D, hist)
    hist += literal_boundary_histograms(pred, label, K, ignore_index, D)
    return hist


def boundary_summary(hist, widths, names=None):
    """Boundary IoU and trimap IoU from hist (int64 [5, K, D + 1]) at every width d of `widths` (1 <= d <= D): with S_i[k] the sum of
    hist[i][k][:d], S2 / (S0 + S1 - S2) and S3 / (S0 + S4 - S3) per class.  A class whose union is 0 is None and left out of the mean (None
    when no class is left).  Returns widths, classes, boundary_iou / trimap_iou [width][class], mean_boundary_iou / mean_trimap_iou [width]."""
    hist = torch.as_tensor(hist).cpu().long()
    if hist.dim() != 3 or hist.shape[0] != BOUNDARY_MAPS:
        raise ValueError("boundary_summary: hist must be [%d, K, D + 1], got %s" % (BOUNDARY_MAPS, tuple(hist.shape)))
    K, D = hist.shape[1], hist.shape[2] - 1
    widths = [int(d) for d in widths]
    if any(not 1 <= d <= D for d in widths):
        raise ValueError("boundary_summary: widths %r lie outside 1..%d" % (widths, D))
    names = [str(n) for n in names] if names is not None and len(names) == K else [str(k) for k in range(K)]
    out = {"widths": widths, "classes": names, "boundary_iou": [], "trimap_iou": [], "mean_boundary_iou": [], "mean_trimap_iou": []}
    for d in widths:
        S = hist[:, :, :d].sum(2).tolist()
        for key, inter, other in (("boundary_iou", S[2], S[1]), ("trimap_iou", S[3], S[4])):
            union = [S[0][k] + other[k] - inter[k] for k in range(K)]
            row = [inter[k] / union[k] if union[k] > 0 else None for k in range(K)]
            kept = [v for v in row if v is not None]
            out[key].append(row)
            out["mean_" + key].append(sum(kept) / len(kept) if kept else None)
    return out


def boundary_settings(cfg):
    """None while TEST.BOUNDARY is False (absent = False), else the tuple of band widths: empty = the 2 % width of the first label's size
    (boundary_width), otherwise strictly increasing integers in 1..64.  TEST.BOUNDARY_WIDTHS changed while BOUNDARY is False is refused
    instead of ignored."""
    test = cfg.TEST
    on = test["BOUNDARY"] if "BOUNDARY" in test else False
    if not isinstance(on, bool):
        raise ValueError("TEST.BOUNDARY %r must be True or False" % (on,))
    widths = test["BOUNDARY_WIDTHS"] if "BOUNDARY_WIDTHS" in test else ()
    if not isinstance(widths, (tuple, list)):
        raise ValueError("TEST.BOUNDARY_WIDTHS %r must be a list of integers" % (widths,))
    widths = tuple(widths)
    if not on:
        if widths != ():
            raise NotImplementedError("TEST.BOUNDARY_WIDTHS %r belongs to TEST.BOUNDARY True" % (widths,))
        return None
    if any(isinstance(d, bool) or not isinstance(d, int) for d in widths):
        raise ValueError("TEST.BOUNDARY_WIDTHS %r must be integers" % (widths,))
    if any(not 1 <= d <= BOUNDARY_MAX_WIDTH for d in widths):
        raise ValueError("TEST.BOUNDARY_WIDTHS %r lie outside 1..%d" % (widths, BOUNDARY_MAX_WIDTH))
    if any(b <= a for a, b in zip(widths, widths[1:])):
        raise ValueError("TEST.BOUNDARY_WIDTHS %r must be strictly increasing" % (widths,))
    K = int(cfg.MODEL.NUM_CLASSES) if "MODEL" in cfg and "NUM_CLASSES" in cfg.MODEL else 1
    if not 1 <= K <= BOUNDARY_MAX_CLASSES:
        raise ValueError("TEST.BOUNDARY: MODEL.NUM_CLASSES %d lies outside 1..%d" % (K, BOUNDARY_MAX_CLASSES))
    ignore = int(cfg.INPUT.IGNORE_LABEL) if "INPUT" in cfg and "IGNORE_LABEL" in cfg.INPUT else 255
    if 0 <= ignore < K:
        raise ValueError("TEST.BOUNDARY: INPUT.IGNORE_LABEL %d names one of the %d classes" % (ignore, K))
    return widths


def require_no_boundary(cfg, who):
    """The boundary metrics are counted on ASPPTester's masks: the other testers refuse the key rather than ignore it (a stray BOUNDARY_WIDTHS
    is refused by boundary_settings itself)."""
    if boundary_settings(cfg) is not None:
        raise NotImplementedError("%s: TEST.BOUNDARY - Boundary IoU and trimap IoU exist for the DeepLab (feature extractor, classifier) pair "
                                  "only (ASPPTester); leave it False" % (who,))


# ----------------------------------------------------------------------------- precision-recall curves and calibration (TEST.CURVES)
CURVE_BINS = 256                        # probability bins per class (CV_BINS of csrc/upsample_curves.h)
CURVE_MAX_ECE_BINS = 64
CURVE_FIXED = 1 << 24                   # the fixed-point scale of the summed confidences
CURVE_DEFAULTS = OrderedDict((("CURVES_ECE_BINS", 15), ("CURVES_PRECISION", 0.9)))      # TEST.CURVES_* of host/config.py


def _curves_check(K, ece_bins):
    if not 1 <= K:
        raise ValueError("curves: %d classes" % (K,))
    if isinstance(ece_bins, bool) or not isinstance(ece_bins, int) or not 1 <= ece_bins <= CURVE_MAX_ECE_BINS:
        raise ValueError("curves: ece_bins %r lies outside 1..%d" % (ece_bins, CURVE_MAX_ECE_BINS))


def literal_curves(output, label, K, ece_bins):
    """What mi_upsample_curves adds to (pr, cal) for one picture, composed from torch ops on the map's device: the definition the kernel is
    tested against, and the path of CPU tensors, of TEST.FUSED_SCORE False and of TEST.CRF.  output [1,K,H,W] fp32 probabilities, label[0]
    the labels.  Only pixels whose label lies in [0, K) count (the confusion matrix's rule: 255, the ignore value and every other value
    outside count nowhere).  Returns two int64 tensors:
      pr  [K, 256, 2]   for every counted pixel and class k: pr[k, b, label == k] += 1, b = min(255, max(0, int(p_k * 256))) - a power-of-two
                        scale and a truncation, exact in fp32, like confidence_bin;
      cal [M, 3]        M = ece_bins; conf = the maximum of the K values, pred = the lowest index among the maxima,
                        m = min(M - 1, max(0, int(conf * float32(M)))) (an fp32 product, truncated):
                        cal[m] += (1, pred == label, int(conf * 2**24)) - the last a fixed-point sum: the scale is exact and the integer sum
                        does not depend on the order."""
    K, M = int(K), ece_bins
    _curves_check(K, M)
    p = output[0].float()
    if p.dim() != 3 or p.shape[0] != K:
        raise ValueError("curves: the map must be [1, %d, H, W], got %s" % (K, tuple(output.shape)))
    lab = label[0] if label.dim() == 3 else label
    lab = lab.reshape(p.shape[-2:]).long().to(p.device)
    counted = (lab >= 0) & (lab < K)
    lc = lab[counted]
    pc = p[:, counted]                                                   # [K, n]
    pr = torch.empty(K, CURVE_BINS, 2, dtype=torch.int64, device=p.device)
    for k in range(K):
        b = (pc[k] * float(CURVE_BINS)).long().clamp_(0, CURVE_BINS - 1)
        pr[k] = torch.bincount(b * 2 + (lc == k).long(), minlength=CURVE_BINS * 2).reshape(CURVE_BINS, 2)
    cal = torch.zeros(M, 3, dtype=torch.int64, device=p.device)
    if lc.numel():
        conf, pred = pc.max(0)                                           # the lowest index among equal maxima
        m = (conf * float(M)).long().clamp_(0, M - 1)
        cal[:, 0] = torch.bincount(m, minlength=M)
        cal[:, 1] = torch.bincount(m[pred == lc], minlength=M)
        cal[:, 2].index_add_(0, m, (conf * float(CURVE_FIXED)).long())
    return pr, cal


def _none_if_nan(v):
    v = float(v)
    return None if v != v else v


def curves_summary(pr, cal, names=None, target_precision=0.9):
    """Curves and calibration numbers, in float64, from pr int64 [K, 256, 2] and cal int64 [M, 3] (literal_curves / mi_upsample_curves).
    Per class k, at the thresholds t_j = j / 256, j = 0..255: TP_j = sum of pr[k, b, 1] over b >= j, FP_j the same of pr[k, b, 0];
    precision P_j = TP_j / (TP_j + FP_j), or 1 where nothing is left; recall R_j = TP_j / TP_0.
      ap            sum_j (R_j - R_{j+1}) P_j with R_256 = 0: sklearn's average_precision_score on the scores b / 256; a class without a
                    positive pixel (TP_0 == 0) has none (None) and is left out of mAP;
      best_f1 / best_f1_threshold      the largest 2 P R / (P + R) and the lowest t_j that reaches it;
      threshold_at_precision / recall_at_precision      the lowest t_j >= 0.5 with P_j >= target_precision and the recall kept there, None if none.
    Above one half "p_c >= t" implies "c is the prediction" (two values above one half cannot sum to one; at t = 0.5 itself the one exception is
    a pixel where two classes hold exactly 0.5 each), so for t >= 0.5 P_j and R_j are the precision and the coverage of the pseudo-labels
    TEST.PSEUDO_THRESHOLD = t would write for class c;
    pseudo_class_thresholds is the list TEST.PSEUDO_CLASS_THRESHOLDS takes: threshold_at_precision, and 1.0 where there is none.
    Calibration: per bin m its count n_m, accuracy and mean confidence (None when empty); ece = sum_m n_m / N |acc_m - conf_m|, mce the largest
    gap of a non-empty bin, accuracy and confidence over all counted pixels.  The bins are [m / M, (m + 1) / M) by truncation; Guo et al. (2017)
    use (m / M, (m + 1) / M]: the two differ only for a confidence exactly on a bin edge."""
    pr = np.asarray(torch.as_tensor(pr).cpu().numpy(), dtype=np.int64)
    cal = np.asarray(torch.as_tensor(cal).cpu().numpy(), dtype=np.int64)
    if pr.ndim != 3 or pr.shape[1:] != (CURVE_BINS, 2) or cal.ndim != 2 or cal.shape[1] != 3:
        raise ValueError("curves_summary: pr must be [K, %d, 2] and cal [M, 3], got %s and %s" % (CURVE_BINS, pr.shape, cal.shape))
    target = float(target_precision)
    if not 0.0 < target <= 1.0:
        raise ValueError("curves_summary: target precision %r lies outside (0, 1]" % (target_precision,))
    K, M = pr.shape[0], cal.shape[0]
    names = [str(n) for n in names] if names is not None and len(names) == K else [str(k) for k in range(K)]
    out = {"bins": CURVE_BINS, "classes": names, "target_precision": target, "positives": [], "ap": [], "best_f1": [], "best_f1_threshold": [],
           "threshold_at_precision": [], "recall_at_precision": [], "pseudo_class_thresholds": []}
    half = CURVE_BINS // 2
    for k in range(K):
        tp = np.cumsum(pr[k, ::-1, 1])[::-1].astype(np.float64)
        fp = np.cumsum(pr[k, ::-1, 0])[::-1].astype(np.float64)
        kept = tp + fp
        prec = np.where(kept > 0, tp / np.where(kept > 0, kept, 1.0), 1.0)
        out["positives"].append(int(tp[0]))
        if tp[0] == 0:
            for key in ("ap", "best_f1", "best_f1_threshold", "threshold_at_precision", "recall_at_precision"):
                out[key].append(None)
            out["pseudo_class_thresholds"].append(1.0)
            continue
        rec = tp / tp[0]
        out["ap"].append(float(np.sum((rec - np.append(rec[1:], 0.0)) * prec)))
        den = prec + rec
        f1 = np.where(den > 0, 2.0 * prec * rec / np.where(den > 0, den, 1.0), 0.0)
        j = int(np.argmax(f1))
        out["best_f1"].append(float(f1[j]))
        out["best_f1_threshold"].append(j / CURVE_BINS)
        ok = np.nonzero(prec[half:] >= target)[0]
        if ok.size:
            j = half + int(ok[0])
            out["threshold_at_precision"].append(j / CURVE_BINS)
            out["recall_at_precision"].append(float(rec[j]))
            out["pseudo_class_thresholds"].append(j / CURVE_BINS)
        else:
            out["threshold_at_precision"].append(None)
            out["recall_at_precision"].append(None)
            out["pseudo_class_thresholds"].append(1.0)
    aps = [v for v in out["ap"] if v is not None]
    out["map"] = sum(aps) / len(aps) if aps else None
    n = cal[:, 0].astype(np.float64)
    N = float(n.sum())
    acc = np.where(n > 0, cal[:, 1] / np.where(n > 0, n, 1.0), np.nan)
    conf = np.where(n > 0, cal[:, 2] / (np.where(n > 0, n, 1.0) * CURVE_FIXED), np.nan)
    gap = np.abs(acc - conf)
    out["calibration"] = {"bins": M, "count": [int(v) for v in cal[:, 0]], "accuracy": [_none_if_nan(v) for v in acc],
                          "confidence": [_none_if_nan(v) for v in conf],
                          "ece": float(np.sum(np.where(n > 0, n * gap, 0.0)) / N) if N else None,
                          "mce": float(np.nanmax(gap)) if N else None,
                          "overall_accuracy": float(cal[:, 1].sum() / N) if N else None,
                          "mean_confidence": float(cal[:, 2].sum() / (N * CURVE_FIXED)) if N else None}
    return out


def curves_accumulate(output, label, K, curves):
    """literal_curves of one [1,K,H,W] map into the data set's (pr, cal)."""
    pr, cal = literal_curves(output, label, K, int(curves[1].shape[0]))
    curves[0].add_(pr.to(curves[0].device))
    curves[1].add_(cal.to(curves[1].device))


def curves_settings(cfg):
    """None while TEST.CURVES is False (absent = False), else (ece_bins, target_precision): CURVES_ECE_BINS an integer in 1..64, CURVES_PRECISION
    in (0, 1].  A CURVES_* key changed while CURVES is False is refused instead of ignored."""
    test = cfg.TEST
    on = test["CURVES"] if "CURVES" in test else False
    if not isinstance(on, bool):
        raise ValueError("TEST.CURVES %r must be True or False" % (on,))
    bins = test["CURVES_ECE_BINS"] if "CURVES_ECE_BINS" in test else CURVE_DEFAULTS["CURVES_ECE_BINS"]
    target = test["CURVES_PRECISION"] if "CURVES_PRECISION" in test else CURVE_DEFAULTS["CURVES_PRECISION"]
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= CURVE_MAX_ECE_BINS:
        raise ValueError("TEST.CURVES_ECE_BINS %r must be an integer in 1..%d" % (bins, CURVE_MAX_ECE_BINS))
    if isinstance(target, bool) or not isinstance(target, (int, float)) or not 0.0 < target <= 1.0:      # (false for a NaN)
        raise ValueError("TEST.CURVES_PRECISION %r lies outside (0, 1]" % (target,))
    if not on:
        for key, v in (("CURVES_ECE_BINS", bins), ("CURVES_PRECISION", target)):
            if v != CURVE_DEFAULTS[key]:
                raise NotImplementedError("TEST.%s %r belongs to TEST.CURVES True" % (key, v))
        return None
    return int(bins), float(target)


def require_no_curves(cfg, who):
    """The curves are counted in ASPPTester's evaluation tail: the other testers refuse the key rather than ignore it (a stray CURVES_* key is
    refused by curves_settings itself), and TEST.PSEUDO_CLASS_THRESHOLDS with it."""
    if curves_settings(cfg) is not None:
        raise NotImplementedError("%s: TEST.CURVES - precision-recall curves and calibration exist for the DeepLab (feature extractor, classifier) "
                                  "pair only (ASPPTester); leave it False" % (who,))
    if "PSEUDO_CLASS_THRESHOLDS" in cfg.TEST and tuple(cfg.TEST["PSEUDO_CLASS_THRESHOLDS"]) != ():
        raise NotImplementedError("%s: TEST.PSEUDO_CLASS_THRESHOLDS - per-class pseudo-label thresholds exist for the DeepLab (feature extractor, "
                                  "classifier) pair only (ASPPTester); leave it ()" % (who,))


def class_threshold_settings(cfg):
    """None while TEST.PSEUDO_CLASS_THRESHOLDS is () (absent = ()), else the tuple of MODEL.NUM_CLASSES thresholds in [0, 1] the pseudo-label
    masks are written with in a single pass (pred where the winning probability >= its class's threshold, else 255) - for instance
    "pseudo_class_thresholds" of an aspp_curves.json counted on a labelled split.  Refused: together with PSEUDO_CLASSWISE (which takes its own
    thresholds from the set) or a non-zero PSEUDO_THRESHOLD, a wrong length, a value outside [0, 1]."""
    test = cfg.TEST
    values = test["PSEUDO_CLASS_THRESHOLDS"] if "PSEUDO_CLASS_THRESHOLDS" in test else ()
    if not isinstance(values, (tuple, list)):
        raise ValueError("TEST.PSEUDO_CLASS_THRESHOLDS %r must be a list of numbers" % (values,))
    values = tuple(values)
    if values == ():
        return None
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0 for v in values):
        raise ValueError("TEST.PSEUDO_CLASS_THRESHOLDS %r must be numbers in [0, 1]" % (values,))
    K = int(cfg.MODEL.NUM_CLASSES)
    if len(values) != K:
        raise ValueError("TEST.PSEUDO_CLASS_THRESHOLDS holds %d values for %d classes" % (len(values), K))
    classwise, _, _ = classwise_settings(cfg)
    if classwise:
        raise NotImplementedError("TEST.PSEUDO_CLASS_THRESHOLDS and TEST.PSEUDO_CLASSWISE True: the thresholds are given or taken from the set, not both")
    _, threshold = score_settings(cfg)
    if threshold != 0.0:
        raise NotImplementedError("TEST.PSEUDO_CLASS_THRESHOLDS and TEST.PSEUDO_THRESHOLD %r: one threshold or one per class, not both" % (threshold,))
    return tuple(float(v) for v in values)


def tta_settings(cfg):
    """(scales, flip) of cfg.TEST (SCALES / FLIP are not reference keys; absent = the defaults (1.0,) / False = plain inference())."""
    scales = tuple(cfg.TEST.SCALES) if "SCALES" in cfg.TEST else (1.0,)
    flip = bool(cfg.TEST.FLIP) if "FLIP" in cfg.TEST else False
    return scales, flip


def require_single_scale(cfg, who):
    """The reference defines multi-scale evaluation for a (feature extractor, classifier) pair only: other testers refuse the keys
    rather than ignore them."""
    scales, flip = tta_settings(cfg)
    if scales != (1.0,) or flip:
        raise NotImplementedError("%s: TEST.SCALES %r / TEST.FLIP %r - multi-scale, flip-averaged evaluation exists for the DeepLab "
                                  "(feature extractor, classifier) pair only (ASPPTester); leave both at their defaults" % (who, scales, flip))


def score_settings(cfg):
    """(fused, threshold) of cfg.TEST (FUSED_SCORE / PSEUDO_THRESHOLD are not reference keys; absent = True / 0.0 = the reference's plain
    argmax masks)."""
    fused = bool(cfg.TEST.FUSED_SCORE) if "FUSED_SCORE" in cfg.TEST else True
    threshold = float(cfg.TEST.PSEUDO_THRESHOLD) if "PSEUDO_THRESHOLD" in cfg.TEST else 0.0
    if not 0.0 <= threshold <= 1.0:
        raise ValueError("TEST.PSEUDO_THRESHOLD %r lies outside [0, 1]" % (threshold,))
    return fused, threshold


def require_plain_argmax(cfg, who):
    """Pseudo-label thresholding is built into the DeepLab evaluation tail only: other testers refuse the key rather than ignore it."""
    _, threshold = score_settings(cfg)
    if classwise_settings(cfg)[0]:
        raise NotImplementedError("%s: TEST.PSEUDO_CLASSWISE - class-wise pseudo-label thresholds exist for the DeepLab (feature extractor, "
                                  "classifier) pair only (ASPPTester); leave it False" % (who,))
    if threshold != 0.0:
        raise NotImplementedError("%s: TEST.PSEUDO_THRESHOLD %r - thresholded pseudo-labels exist for the DeepLab (feature extractor, "
                                  "classifier) pair only (ASPPTester); leave it at 0" % (who, threshold))


# ----------------------------------------------------------------------------- class-wise pseudo-label thresholds
PSEUDO_BINS = 1024                      # confidence bins per class; the kernel's histogram has this width and no other
PSEUDO_PORTION_DEFAULT = 0.5            # TEST.PSEUDO_PORTION of host/config.py: the median rule


def confidence_bin(best):
    """min(PSEUDO_BINS - 1, int(best * 1024)) on the fp32 value(s) `best` (a number, an array or a tensor; same container back, int64).
    Both steps are exact - a power-of-two scale and a truncation - so whoever sees the same fp32 winning probability gets the same bin: the
    kernel and this line cannot round differently."""
    if isinstance(best, torch.Tensor):
        return (best.float() * float(PSEUDO_BINS)).long().clamp_(max=PSEUDO_BINS - 1)
    out = np.minimum(PSEUDO_BINS - 1, (np.asarray(best, dtype=np.float32) * np.float32(PSEUDO_BINS)).astype(np.int64))
    return int(out) if out.ndim == 0 else out


def class_thresholds(hist, portion, cap):
    """One pseudo-label threshold per class from hist int64 [K, PSEUDO_BINS], hist[c, j] = the number of pixels predicted as c whose winning
    probability falls in bin j (confidence_bin).  float32 [K] (numpy).  Per class, in integers until the last line:
        n = hist[c].sum();  n == 0: t = cap
        r = min(n - 1, floor(portion * n))      the rank, ascending from 0, of the confidence at the `portion` quantile; `portion * n` is the
                                                Python product float * int (one rounding to a double), math.floor of it an int
        j = the smallest bin with cumsum(hist[c])[j] > r: the bin of the rank-r confidence
        t = min(j / 1024, cap) as float32       j / 1024 is exact
    A pixel keeps its label iff best >= t[pred]; t is a bin edge unless the cap bites, so that is bin >= j.  At least the share 1 - portion of
    every class survives while the cap does not bite: rare, hard classes keep their most confident half instead of nothing."""
    if isinstance(hist, torch.Tensor):
        hist = hist.cpu().numpy()
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[1] != PSEUDO_BINS or hist.dtype.kind not in "iu":
        raise ValueError("class_thresholds: hist must be an integer [K, %d] array, got %s %s" % (PSEUDO_BINS, hist.dtype, hist.shape))
    portion, cap = float(portion), float(cap)
    if not 0.0 <= portion <= 1.0 or not 0.0 <= cap <= 1.0:          # (false for a NaN)
        raise ValueError("class_thresholds: portion %r and cap %r must lie in [0, 1]" % (portion, cap))
    hist = hist.astype(np.int64)
    if (hist < 0).any():
        raise ValueError("class_thresholds: negative count")
    out = np.empty(hist.shape[0], dtype=np.float32)
    for c in range(hist.shape[0]):
        n = int(hist[c].sum())
        if n == 0:
            out[c] = np.float32(cap)
            continue
        r = min(n - 1, int(math.floor(portion * n)))
        j = int(np.searchsorted(np.cumsum(hist[c]), r, side="right"))          # the first j with cumsum[j] > r
        out[c] = min(np.float32(j / PSEUDO_BINS), np.float32(cap))
    return out


def threshold_table(hist, thresholds, names=None):
    """What ASPPTester logs and writes as class_thresholds.json: per class its name, the pixels predicted as it, its threshold and the share of
    those pixels in the bins at or above the threshold.  The share is the kept share exactly when the threshold is a bin edge (always, unless
    a cap that is no multiple of 1/1024 bites: then the cap's own bin is left out and the share is a lower bound)."""
    if isinstance(hist, torch.Tensor):
        hist = hist.cpu().numpy()
    hist = np.asarray(hist, dtype=np.int64)
    K = hist.shape[0]
    names = [str(c) for c in range(K)] if names is None else [str(v) for v in names]
    pixels = [int(v) for v in hist.sum(1)]
    first = [int(math.ceil(float(t) * PSEUDO_BINS)) for t in thresholds]          # float32 -> double and * 1024 are exact
    kept = [int(hist[c, first[c]:].sum()) / pixels[c] if pixels[c] else 0.0 for c in range(K)]
    return {"bins": PSEUDO_BINS, "classes": names, "pixels": pixels, "thresholds": [float(t) for t in thresholds], "kept": kept}


def classwise_settings(cfg):
    """(classwise, portion, cap) of cfg.TEST (PSEUDO_CLASSWISE / PSEUDO_PORTION are not reference keys; absent = False / 0.5).  The cap is
    TEST.PSEUDO_THRESHOLD, where 0 means no cap (1.0) under PSEUDO_CLASSWISE.  PSEUDO_PORTION changed while PSEUDO_CLASSWISE is False is
    refused instead of ignored."""
    classwise = bool(cfg.TEST.PSEUDO_CLASSWISE) if "PSEUDO_CLASSWISE" in cfg.TEST else False
    portion = cfg.TEST.PSEUDO_PORTION if "PSEUDO_PORTION" in cfg.TEST else PSEUDO_PORTION_DEFAULT
    if isinstance(portion, bool) or not isinstance(portion, (int, float)) or not 0.0 <= portion <= 1.0:      # (a merged value was checked there)
        raise ValueError("TEST.PSEUDO_PORTION %r lies outside [0, 1]" % (portion,))
    _, threshold = score_settings(cfg)
    if not classwise:
        if float(portion) != PSEUDO_PORTION_DEFAULT:
            raise NotImplementedError("TEST.PSEUDO_PORTION %r belongs to TEST.PSEUDO_CLASSWISE True" % (portion,))
        return False, float(portion), threshold
    return True, float(portion), threshold if threshold != 0.0 else 1.0


class ScoreResult(object):
    """What predict_and_score returns for one image: pred / pseudo uint8 [H,W] on the inputs' device (pseudo None for threshold 0), cmt int64
    [K,K] on the CPU as confusion_matrix returns it, intersection / union / target / output float32 [K] on the CPU holding the integers
    intersectionAndUnionGPU returns."""
    __slots__ = ("pred", "pseudo", "cmt", "intersection", "union", "target", "output")

    def __init__(self, pred, pseudo, cmt, intersection, union, target, output):
        self.pred, self.pseudo, self.cmt = pred, pseudo, cmt
        self.intersection, self.union, self.target, self.output = intersection, union, target, output


def scores_from_counts(counts, K, pred, pseudo):
    """ScoreResult from the [K*K + 3K] int64 counts (cmt, intersection, output, target: the layout of mi_upsample_predict_score)."""
    counts = counts.cpu()                                   # the one device-to-host copy
    cmt = counts[:K * K].reshape(K, K).clone()
    ai, ao, at = [counts[K * K + i * K:K * K + (i + 1) * K].float() for i in range(3)]
    return ScoreResult(pred, pseudo, cmt, ai, ao + at - ai, at, ao)


def _engine_masks(feature_extractor, classifier, image, size, flip, scales, **kw):
    """(pred, pseudo, counts) of the engine's evaluation tail: the backbone passes of inference / multi_scale_inference, then ONE kernel."""
    with torch.no_grad():
        if tuple(scales) == (1.0,) and not flip:
            return classifier.predict_mask(feature_extractor(image), size, **kw)
        from .. import kernels
        sizes, _, divisors = multi_scale_plan(image.shape[-2:], flip, scales)
        x0 = image[:1].float().contiguous()
        feats = [feature_extractor(kernels.image_resize_ac(x0, hw, with_mirror=flip)) for hw in sizes]
        mirrors = [(False, True) if flip else (False,)] * len(sizes)
        return classifier.predict_mask_multi(feats, mirrors, size, divisors, **kw)


def _engine_masks_slide(feature_extractor, classifier, image, size, flip, slide, **kw):
    """(pred, pseudo, counts) of the engine's sliding-window tail: the backbone passes of slide_inference (_slide_feats), then ONE kernel."""
    origins, (wh, ww), r = slide_windows(image.shape[-2:], size, *slide)
    with torch.no_grad():
        feats = _slide_feats(feature_extractor, image, origins, (wh, ww), flip)
        return classifier.predict_mask_slide(feats, flip, [(r * y0, r * x0) for y0, x0 in origins], (r * wh, r * ww), size, **kw)


def _require_single_scale_slide(scales):
    if tuple(scales) != (1.0,):
        raise NotImplementedError("sliding-window evaluation is single-scale: scales %r" % (tuple(scales),))


def _literal_output(feature_extractor, classifier, image, label, flip, scales, slide=None):
    if slide is not None:
        _require_single_scale_slide(scales)
        return slide_inference(feature_extractor, classifier, image, label, slide[0], slide[1], flip=flip)
    if tuple(scales) == (1.0,) and not flip:
        return inference(feature_extractor, classifier, image, label, flip=False)
    return multi_scale_inference(feature_extractor, classifier, image, label, flip=flip, scales=list(scales))


def _class_table(class_threshold, K, device):
    t = torch.as_tensor(np.asarray(class_threshold, dtype=np.float32) if not isinstance(class_threshold, torch.Tensor) else class_threshold,
                        dtype=torch.float32)
    if t.shape != (K,) or not bool(((t >= 0) & (t <= 1)).all()):
        raise ValueError("class_threshold must be %d values in [0, 1], got %r" % (K, t.tolist()))
    return t.to(device)


def literal_histogram(output, K):
    """The confidence histogram of one [1,K,H,W] probability map with torch ops (int64 [K, PSEUDO_BINS] on its device): what the kernel adds
    to `hist` for the same image."""
    top = output[:1].max(1)
    return torch.bincount((top[1] * PSEUDO_BINS + confidence_bin(top[0])).flatten(), minlength=K * PSEUDO_BINS).reshape(K, PSEUDO_BINS)


def literal_pseudo(output, class_threshold):
    """The class-wise pseudo-label mask of one [1,K,H,W] probability map with torch ops: uint8 [H,W], pred where max >= class_threshold[pred]."""
    top = output[:1].max(1)
    pred = top[1]
    t = _class_table(class_threshold, output.shape[1], output.device)
    return torch.where(top[0] >= t[pred], pred, torch.full_like(pred, 255))[0].to(torch.uint8)


def predict_and_score(feature_extractor, classifier, image, label, flip=False, scales=(1.0,), *, num_classes, ignore_index=255, threshold=0.0,
                      class_threshold=None, hist=None, slide=None, curves=None):
    """One image of ASPPTester.test(): inference(flip=False) (scales == (1.0,), no flip) or multi_scale_inference, then the argmax mask, the
    pseudo-label mask (argmax where the winning probability >= threshold, else 255; None for threshold 0), confusion_matrix and
    intersectionAndUnionGPU against label[:1].  On the engine (a classifier with predict_mask_multi, CUDA tensors) the backbone passes are
    those of inference / multi_scale_inference and everything after the logits is ONE kernel, which never writes the probability map; the
    integers are the same.  A substituted / foreign classifier or CPU tensors run the literal composition.
    Class-wise pseudo-labels: hist (the caller's int64 [K, PSEUDO_BINS] tensor, kept across images) receives this image's confidence histogram;
    class_threshold (K values in [0, 1]) replaces threshold in the pseudo-label mask: argmax where the winning probability >= its class's.
    slide = (crop, stride), each (h, w) (slide_settings): sliding-window evaluation - slide_inference instead of inference, on the engine
    ONE mi_upsample_predict_score_slide after the windows' backbone passes; scales must be (1.0,).  None: no sliding.
    curves = (pr, cal) (TEST.CURVES): the caller's int64 [K, 256, 2] and [ece_bins, 3] tensors, kept across images, receive this image's
    precision-recall and calibration histograms: on the engine one more launch on the same logits (mi_upsample_curves / _slide; the backbone passes
    and source lists are not recomputed), else literal_curves on the map."""
    K = int(num_classes)
    if not 0.0 <= float(threshold) <= 1.0:
        raise ValueError("threshold %r lies outside [0, 1]" % (threshold,))
    if hist is not None and (hist.dtype != torch.int64 or tuple(hist.shape) != (K, PSEUDO_BINS)):
        raise ValueError("hist must be int64 [%d, %d], got %s %s" % (K, PSEUDO_BINS, hist.dtype, tuple(hist.shape)))
    scales = tuple(scales)
    size = tuple(label.shape[-2:])
    y0 = label[:1]                                          # inference() keeps image 0 only (utility.py:190)
    if hasattr(classifier, "predict_mask_multi") and image.is_cuda:
        kw = dict(labels=y0[0].long().contiguous(), ignore_index=int(ignore_index), threshold=float(threshold), want_pseudo=threshold != 0)
        if class_threshold is not None:
            kw.update(class_threshold=_class_table(class_threshold, K, "cpu"), want_pseudo=True)
        if hist is not None:
            kw.update(hist=hist, want_pseudo=class_threshold is not None)
        if curves is not None:
            kw.update(curves=curves)
        if slide is not None:
            _require_single_scale_slide(scales)
            pred, pseudo, counts = _engine_masks_slide(feature_extractor, classifier, image, size, flip, slide, **kw)
        else:
            pred, pseudo, counts = _engine_masks(feature_extractor, classifier, image, size, flip, scales, **kw)
        return scores_from_counts(counts, K, pred, pseudo)
    output = _literal_output(feature_extractor, classifier, image, label, flip, scales, slide)
    top = output.max(1)
    pred = top[1]
    pseudo = None
    if class_threshold is not None:
        pseudo = literal_pseudo(output, class_threshold)
    elif threshold != 0 and hist is None:
        pseudo = torch.where(top[0] >= threshold, pred, torch.full_like(pred, 255))[0].to(torch.uint8)
    if hist is not None:
        hist.add_(literal_histogram(output, K).to(hist.device))
    if curves is not None:
        curves_accumulate(output, y0, K, curves)
    cmt = confusion_matrix(types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=K)), torch.flatten(pred), torch.flatten(y0))
    ai, union, at, ao = [t.cpu() for t in intersectionAndUnionGPU(pred.clone(), y0.long(), K, ignore_index)]
    return ScoreResult(pred[0].to(torch.uint8), pseudo, cmt, ai, union, at, ao)


def classwise_pseudo_labels(feature_extractor, classifier, image, label, flip=False, scales=(1.0,), *, num_classes, class_threshold, slide=None):
    """The second pass of class-wise pseudo-labelling for one image: the uint8 [H,W] mask, argmax where the winning probability >= its class's
    threshold, else 255.  No metric counting, no histogram.  Engine and literal composition, and `slide`, as in predict_and_score."""
    K = int(num_classes)
    size = tuple(label.shape[-2:])
    if hasattr(classifier, "predict_mask_multi") and image.is_cuda:
        if slide is not None:
            _require_single_scale_slide(scales)
            return _engine_masks_slide(feature_extractor, classifier, image, size, flip, slide,
                                       class_threshold=_class_table(class_threshold, K, "cpu"), want_pseudo=True)[1]
        return _engine_masks(feature_extractor, classifier, image, size, flip, tuple(scales), class_threshold=_class_table(class_threshold, K, "cpu"),
                             want_pseudo=True)[1]
    return literal_pseudo(_literal_output(feature_extractor, classifier, image, label, flip, tuple(scales), slide), class_threshold)


# ----------------------------------------------------------------------------- CRF refinement (TEST.CRF)
CRF_DEFAULTS = OrderedDict((("CRF_ITER", 5), ("CRF_WINDOW", 7), ("CRF_DILATION", 4), ("CRF_POS_W", 3.0), ("CRF_POS_XY", 3.0),
                                        ("CRF_BI_W", 10.0), ("CRF_BI_XY", 80.0), ("CRF_BI_RGB", 13.0)))      # TEST.CRF_* of host/config.py
CRF_MAX_CLASSES = 32


def crf_settings(cfg):
    """None while TEST.CRF is False (absent = False), else the keyword arguments of kernels.crf_refine: iters, window, dilation, pos_w, pos_xy,
    bi_w, bi_xy, bi_rgb.  Validates on the host what mi_crf_refine validates (include/mi355seg.h).  A CRF_* key that differs from its default
    while CRF is False is refused instead of ignored."""
    test = cfg.TEST
    on = test["CRF"] if "CRF" in test else False
    if not isinstance(on, bool):
        raise ValueError("TEST.CRF %r must be True or False" % (on,))
    v = OrderedDict((k, test[k] if k in test else d) for k, d in CRF_DEFAULTS.items())
    if not on:
        stray = [k for k, d in CRF_DEFAULTS.items() if isinstance(v[k], bool) or v[k] != d]
        if stray:
            raise NotImplementedError("TEST.%s %r belongs to TEST.CRF True" % (stray[0], v[stray[0]]))
        return None
    for k in ("CRF_ITER", "CRF_WINDOW", "CRF_DILATION"):
        if isinstance(v[k], bool) or not isinstance(v[k], int):
            raise ValueError("TEST.%s %r must be an integer" % (k, v[k]))
    for k in ("CRF_POS_W", "CRF_POS_XY", "CRF_BI_W", "CRF_BI_XY", "CRF_BI_RGB"):
        if isinstance(v[k], bool) or not isinstance(v[k], (int, float)) or not math.isfinite(v[k]):
            raise ValueError("TEST.%s %r must be a finite number" % (k, v[k]))
    if not 0 <= v["CRF_ITER"] <= 32:
        raise ValueError("TEST.CRF_ITER %r lies outside 0..32" % (v["CRF_ITER"],))
    if not 3 <= v["CRF_WINDOW"] <= 11 or v["CRF_WINDOW"] % 2 == 0:
        raise ValueError("TEST.CRF_WINDOW %r must be odd and in 3..11" % (v["CRF_WINDOW"],))
    if not 1 <= v["CRF_DILATION"] <= 16:
        raise ValueError("TEST.CRF_DILATION %r lies outside 1..16" % (v["CRF_DILATION"],))
    for k in ("CRF_POS_XY", "CRF_BI_XY", "CRF_BI_RGB"):
        if not v[k] > 0:
            raise ValueError("TEST.%s %r must be positive" % (k, v[k]))
    for k in ("CRF_POS_W", "CRF_BI_W"):
        if v[k] < 0:
            raise ValueError("TEST.%s %r must not be negative" % (k, v[k]))
    K = int(cfg.MODEL.NUM_CLASSES) if "MODEL" in cfg and "NUM_CLASSES" in cfg.MODEL else 1
    if not 1 <= K <= CRF_MAX_CLASSES:
        raise ValueError("TEST.CRF: MODEL.NUM_CLASSES %d lies outside 1..%d" % (K, CRF_MAX_CLASSES))
    return dict(iters=v["CRF_ITER"], window=v["CRF_WINDOW"], dilation=v["CRF_DILATION"], pos_w=float(v["CRF_POS_W"]), pos_xy=float(v["CRF_POS_XY"]),
                bi_w=float(v["CRF_BI_W"]), bi_xy=float(v["CRF_BI_XY"]), bi_rgb=float(v["CRF_BI_RGB"]))


def require_no_crf(cfg, who):
    """The CRF refinement sits between ASPPTester's evaluation tail and its argmax: the other testers refuse the key rather than ignore it
    (a stray CRF_* key is refused by crf_settings itself)."""
    if crf_settings(cfg) is not None:
        raise NotImplementedError("%s: TEST.CRF - the CRF refinement exists for the DeepLab (feature extractor, classifier) pair only "
                                  "(ASPPTester); leave it False" % (who,))


def crf_channel_scale(cfg):
    """The three factors that turn a difference of the normalised input tensor into a difference in 0..255 colour units: the transform divides
    by INPUT.PIXEL_STD after scaling the image to 0..255 (TO_BGR255) or to 0..1 (otherwise)."""
    std = [float(s) for s in cfg.INPUT.PIXEL_STD]
    if len(std) != 3:
        raise ValueError("TEST.CRF needs three INPUT.PIXEL_STD values, got %r" % (std,))
    return tuple(s * (1.0 if cfg.INPUT.TO_BGR255 else 255.0) for s in std)


def crf_refine_output(output, image, size, cs, settings):
    """The refined [1,K,H,W] map of one literal-path output: image 0 brought to the label's size (bilinear, align_corners, as the evaluation
    itself resizes), then kernels.crf_refine.  The engine only: there is no torch-op CRF to fall back to."""
    from .. import kernels
    if not output.is_cuda:
        raise NotImplementedError("TEST.CRF runs on the GPU only (mi_crf_refine); got a %s tensor" % (output.device,))
    x0 = image[:1].float().contiguous()
    if tuple(x0.shape[-2:]) != tuple(size):
        x0 = kernels.image_resize_ac(x0, tuple(size))
    return kernels.crf_refine(output[:1].float().contiguous(), x0, cs, **settings).probs


# ----------------------------------------------------------------------------- polyp metrics (TEST.POLYP_METRICS)
POLYP_EPS = 2.220446049250313e-16       # numpy's float64 eps, the constant of the published evaluation code
POLYP_BINS = 256                        # thresholds 0..255 on q = int(float32(p) * 255)
POLYP_KEYS = ("mDice", "mIoU", "meanF", "maxF", "S", "meanE", "maxE", "MAE")
POLYP_QUADRANT_SUMS = 20                # sums[:20] = [LT, RT, LB, RB][sum p, sum p^2, sum p g, sum p^2 g, sum g]; sums[20:22] = cx, cy


def polyp_settings(cfg):
    """TEST.POLYP_METRICS of cfg.TEST (not a reference key; absent = False): PranetTester also reports the polyp-segmentation metrics."""
    return bool(cfg.TEST.POLYP_METRICS) if "POLYP_METRICS" in cfg.TEST else False


def require_no_polyp_metrics(cfg, who):
    """The polyp metrics score PraNet's sigmoid map: testers of softmax models refuse the key rather than ignore it."""
    if polyp_settings(cfg):
        raise NotImplementedError("%s: TEST.POLYP_METRICS - the polyp metrics (Dice, IoU, F, S, E, MAE) exist for PranetTester only; leave it False"
                                  % (who,))


def _polyp_ratio(num, den, both_empty):
    """num / den per threshold; where den == 0: 1 if prediction and ground truth are both empty, else 0."""
    out = np.where(both_empty, 1.0, 0.0)
    nz = den != 0
    out[nz] = num[nz] / den[nz]
    return out


def _polyp_moments(n, s1, s2):
    """(mean, variance with divisor n - 1, clamped at 0) of n values from their sum and sum of squares; fewer than 2 values: variance 0."""
    mean = s1 / n
    var = max(0.0, (s2 - n * mean * mean) / (n - 1)) if n > 1 else 0.0
    return mean, var


def _polyp_object(n, s1, s2):
    """O(x) = 2 mean / (mean^2 + 1 + std(ddof=1) + eps) of n values from their sums; the std of fewer than 2 values is 0 (numpy: NaN)."""
    if n == 0:
        return 0.0
    mean, var = _polyp_moments(n, s1, s2)
    return 2.0 * mean / (mean * mean + 1.0 + math.sqrt(var) + POLYP_EPS)


def _polyp_ssim(n, sp, sp2, spg, gq):
    """The S-measure's region similarity of a quadrant of n pixels from sum p, sum p^2, sum p g, sum g (g^2 == g); fewer than 2 pixels: 0."""
    if n < 2:
        return 0.0
    x, var_p = _polyp_moments(n, sp, sp2)
    y, var_g = _polyp_moments(n, gq, gq)
    cov = (spg - n * x * y) / (n - 1)
    a = 4.0 * x * y * cov
    b = (x * x + y * y) * (var_p + var_g)
    if a != 0:
        return a / (b + POLYP_EPS)
    return 1.0 if b == 0 else 0.0


def polyp_image_stats(hist, sums, H, W):
    """One image's polyp metrics from what mi_polyp_score returns for it (or the same numbers computed elsewhere): hist int [2,256] (background,
    foreground) of q = int(float32(p) * 255), sums float64 [>= 22] (POLYP_QUADRANT_SUMS quadrant sums, cx, cy).  float64 throughout.
    Returns {"dice", "iou", "f", "e": float64 [256] curves over the thresholds q >= t, "S", "MAE": floats}.
    Definitions: Dice 2TP/(TP+FP+G), IoU TP/(FP+G), F-beta with beta^2 = 0.3, the E-measure in the closed form of Fan et al. (IJCAI 2018) over
    the four parts TP / FP / FN / TN, the S-measure of Fan et al. (ICCV 2017) with alpha = 0.5, MAE on the unquantised p.  Two deliberate
    departures from the published code, which yields NaN there: a quadrant of fewer than 2 pixels contributes 0, and the std of fewer than 2
    values is 0."""
    hist = np.asarray(hist.cpu() if isinstance(hist, torch.Tensor) else hist).astype(np.int64)
    sums = np.asarray(sums.cpu() if isinstance(sums, torch.Tensor) else sums, dtype=np.float64)
    H, W = int(H), int(W)
    N = H * W
    if hist.shape != (2, POLYP_BINS) or sums.ndim != 1 or sums.shape[0] < POLYP_QUADRANT_SUMS + 2:
        raise ValueError("polyp_image_stats: hist must be [2, %d] and sums hold at least %d values, got %s and %s"
                         % (POLYP_BINS, POLYP_QUADRANT_SUMS + 2, hist.shape, sums.shape))
    if int(hist.sum()) != N or (hist < 0).any():
        raise ValueError("polyp_image_stats: the histogram holds %d pixels, the image %d" % (int(hist.sum()), N))
    eps = POLYP_EPS
    G = int(hist[1].sum())
    tp = np.cumsum(hist[1][::-1])[::-1].astype(np.float64)          # TP_t = foreground pixels with q >= t
    fp = np.cumsum(hist[0][::-1])[::-1].astype(np.float64)
    empty = (tp + fp == 0) & (G == 0)
    dice = _polyp_ratio(2.0 * tp, tp + fp + G, empty)
    iou = _polyp_ratio(tp, fp + G, empty)
    prec = _polyp_ratio(tp, tp + fp, empty)
    rec = _polyp_ratio(tp, np.full(POLYP_BINS, float(G)), empty)
    f = _polyp_ratio(1.3 * prec * rec, 0.3 * prec + rec, empty)
    if G == 0:
        e = (N - tp - fp) / (N - 1 + eps)
    elif G == N:
        e = (tp + fp) / (N - 1 + eps)
    else:
        mu_b, mu_g = (tp + fp) / N, G / N
        e = np.zeros(POLYP_BINS)
        for a, b, part in ((1 - mu_b, 1 - mu_g, tp), (1 - mu_b, -mu_g, fp), (-mu_b, 1 - mu_g, G - tp), (-mu_b, -mu_g, N - G - fp)):
            align = 2.0 * a * b / (a * a + b * b + eps)
            e = e + (align + 1.0) ** 2 / 4.0 * part
        e = e / (N - 1 + eps)
    quad = sums[:POLYP_QUADRANT_SUMS].reshape(4, 5)
    sp, sp2, spg, sp2g = [float(v) for v in quad.sum(0)[:4]]
    mae = ((G - spg) + (sp - spg)) / N                              # sum over foreground of (1 - p) + sum over background of p
    yfrac = G / N
    if G == 0:
        s = 1.0 - sp / N
    elif G == N:
        s = sp / N
    else:
        # foreground: p over g == 1; background: 1 - p over g == 0, whose sums are n - sum p and n - 2 sum p + sum p^2
        nb, spb, sp2b = N - G, sp - spg, sp2 - sp2g
        s_obj = yfrac * _polyp_object(G, spg, sp2g) + (1.0 - yfrac) * _polyp_object(nb, nb - spb, nb - 2.0 * spb + sp2b)
        cx, cy = int(sums[POLYP_QUADRANT_SUMS]), int(sums[POLYP_QUADRANT_SUMS + 1])
        if not (0 <= cx <= W and 0 <= cy <= H):
            raise ValueError("polyp_image_stats: split point (%d, %d) outside the %d x %d image" % (cx, cy, H, W))
        sizes = (cx * cy, cy * (W - cx), (H - cy) * cx, (H - cy) * (W - cx))
        w1, w2, w3 = cx * cy / N, cy * (W - cx) / N, (H - cy) * cx / N
        weights = (w1, w2, w3, 1.0 - w1 - w2 - w3)
        s_reg = 0.0
        for n, wt, (qp, qp2, qpg, _, qg) in zip(sizes, weights, quad):
            s_reg += wt * _polyp_ssim(n, float(qp), float(qp2), float(qpg), float(qg))
        s = max(0.0, 0.5 * s_obj + 0.5 * s_reg)
    return {"dice": dice, "iou": iou, "f": f, "e": e, "S": float(s), "MAE": float(mae)}


def polyp_centre(G, col_sum, row_sum):
    """(cx, cy) of the S-measure's split from the integers G = sum g, sum(col g), sum(row g): int(round_half_even(sum / G)) + 1 in float64
    (Python's round is half-even), as mi_polyp_score computes it; (0, 0) when G == 0."""
    G = int(G)
    if G == 0:
        return 0, 0
    return int(round(int(col_sum) / G)) + 1, int(round(int(row_sum) / G)) + 1


class PolypMeter(object):
    """Dataset aggregation of polyp_image_stats: every curve is averaged over images, mean* is the mean of that curve over the 256 thresholds and
    max* its maximum; S and MAE are means over images."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.curves = {k: np.zeros(POLYP_BINS) for k in ("dice", "iou", "f", "e")}
        self.s_sum = 0.0
        self.mae_sum = 0.0
        self.count = 0

    def update(self, stats):
        for k in self.curves:
            self.curves[k] = self.curves[k] + np.asarray(stats[k], dtype=np.float64)
        self.s_sum += float(stats["S"])
        self.mae_sum += float(stats["MAE"])
        self.count += 1

    def mean_curves(self):
        n = float(max(self.count, 1))
        return {k: v / n for k, v in self.curves.items()}

    def as_dict(self):
        c = self.mean_curves()
        n = float(max(self.count, 1))
        return {"mDice": float(c["dice"].mean()), "mIoU": float(c["iou"].mean()), "meanF": float(c["f"].mean()), "maxF": float(c["f"].max()),
                "S": self.s_sum / n, "meanE": float(c["e"].mean()), "maxE": float(c["e"].max()), "MAE": self.mae_sum / n, "images": self.count}

    def summary(self, logger):
        r = self.as_dict()
        logger.info("Polyp metric, val result over {} images: mDice/mIoU {:.4f}/{:.4f}.".format(r["images"], r["mDice"], r["mIoU"]))
        logger.info("Polyp metric, val result: meanF/maxF {:.4f}/{:.4f}, S-measure {:.4f}.".format(r["meanF"], r["maxF"], r["S"]))
        logger.info("Polyp metric, val result: meanE/maxE {:.4f}/{:.4f}, MAE {:.4f}.".format(r["meanE"], r["maxE"], r["MAE"]))


# ----------------------------------------------------------------------------- surface-distance metrics (TEST.SURFACE_METRICS)
SURFACE_MAX_TOLERANCES = 8              # MI_SURFACE_MAX_TOL of include/mi355seg.h, where the definition stands
SURFACE_INTS = 27                       # |P|, |G|, |S(P)|, |S(G)|, 2 maxima of d2, 2 order statistics, floor r, remainder, defined, 2 x 8 tolerance counts


def _surface_check(percentile, tolerances, what):
    if isinstance(percentile, bool) or not isinstance(percentile, (int, np.integer)) or not 1 <= int(percentile) <= 100:
        raise ValueError("%s: the percentile %r must be an integer in 1..100" % (what, percentile))
    if not isinstance(tolerances, (tuple, list)):
        raise ValueError("%s: the tolerances %r must be a list of numbers" % (what, tolerances))
    if len(tolerances) > SURFACE_MAX_TOLERANCES:
        raise ValueError("%s: %d tolerances, at most %d" % (what, len(tolerances), SURFACE_MAX_TOLERANCES))
    for t in tolerances:
        if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not (t >= 0 and math.isfinite(t)):
            raise ValueError("%s: the tolerances %r must be finite numbers >= 0" % (what, tuple(tolerances)))
    return int(percentile), tuple(float(t) for t in tolerances)


def surface_settings(cfg):
    """None while TEST.SURFACE_METRICS is False (not a reference key; absent = False), else (percentile, tolerances) from
    TEST.SURFACE_PERCENTILE (an integer in 1..100, default 95) and TEST.SURFACE_TOLERANCES (at most 8 pixel distances >= 0, default (2.0,))."""
    test = cfg.TEST
    on = test["SURFACE_METRICS"] if "SURFACE_METRICS" in test else False
    if not isinstance(on, bool):
        raise ValueError("TEST.SURFACE_METRICS %r must be True or False" % (on,))
    if not on:
        return None
    return _surface_check(test["SURFACE_PERCENTILE"] if "SURFACE_PERCENTILE" in test else 95,
                          test["SURFACE_TOLERANCES"] if "SURFACE_TOLERANCES" in test else (2.0,), "TEST.SURFACE_PERCENTILE / TEST.SURFACE_TOLERANCES")


def require_no_surface(cfg, who):
    """The surface distances are measured on PranetTester's binary masks: testers of multi-class models refuse the key rather than ignore it."""
    if surface_settings(cfg) is not None:
        raise NotImplementedError("%s: TEST.SURFACE_METRICS - the surface-distance metrics (HD, HD95, ASSD, NSD) exist for PranetTester only; "
                                  "leave it False" % (who,))


def surface_keys(percentile, tolerances):
    """The metric names of one setting: HD, HD<percentile>, ASSD, then NSD@<tau> per tolerance."""
    return ["HD", "HD%d" % percentile, "ASSD"] + ["NSD@%g" % t for t in tolerances]


def surface_image_stats(ints, sums, tolerances=(2.0,), percentile=95):
    """One image's surface metrics from its row of mi_surface_score's ints [27] and sums [2] (or the same numbers computed elsewhere), float64
    throughout: {"HD", "HD<percentile>", "ASSD", "NSD@<tau>" per tolerance, "defined"}.  The definitions: include/mi355seg.h.  The percentile is
    numpy's linear interpolation between the two order statistics, with frac(r) = remainder / 100 from the kernel's integers.  Both masks empty:
    distances 0, NSD 1.  Exactly one empty: defined False, the distances None, NSD 0."""
    ints = np.asarray(ints.cpu() if isinstance(ints, torch.Tensor) else ints).astype(np.int64)
    sums = np.asarray(sums.cpu() if isinstance(sums, torch.Tensor) else sums, dtype=np.float64)
    percentile, tolerances = _surface_check(percentile, tuple(tolerances), "surface_image_stats")
    if ints.shape != (SURFACE_INTS,) or sums.shape != (2,):
        raise ValueError("surface_image_stats: ints must be [%d] and sums [2], got %s and %s" % (SURFACE_INTS, ints.shape, sums.shape))
    keys = surface_keys(percentile, tolerances)
    n_p, n_g = int(ints[2]), int(ints[3])
    n = n_p + n_g
    if bool(ints[10]) != ((n_p == 0) == (n_g == 0)) or (ints < 0).any():
        raise ValueError("surface_image_stats: surface counts %d / %d contradict the defined flag %d" % (n_p, n_g, int(ints[10])))
    if n == 0:
        return dict([(k, 1.0 if k.startswith("NSD@") else 0.0) for k in keys], defined=True)
    if n_p == 0 or n_g == 0:
        return dict([(k, 0.0 if k.startswith("NSD@") else None) for k in keys], defined=False)
    lo, hi = math.sqrt(float(ints[6])), math.sqrt(float(ints[7]))
    out = {"HD": math.sqrt(float(max(ints[4], ints[5]))), keys[1]: lo + (float(ints[9]) / 100.0) * (hi - lo),
           "ASSD": 0.5 * (float(sums[0]) / n_p + float(sums[1]) / n_g)}
    for t, k in enumerate(keys[3:]):
        out[k] = float(int(ints[11 + 2 * t]) + int(ints[12 + 2 * t])) / n
    out["defined"] = True
    return out


SURFACE_CDIST_PAIRS = 1 << 22           # pairs per torch.cdist call of literal_surface_stats


def literal_surface_stats(pred, label, cls=1, percentile=95, tolerances=(2.0,), pairs=SURFACE_CDIST_PAIRS):
    """What a user would write without mi_surface_score, from torch ops on the inputs' device (pred, label [H,W]): surfaces from shifted
    comparisons, their coordinates, chunked torch.cdist (fp32, exact differences rather than the matrix-product form), min, sort, and the
    percentile by hand.  The same dict as surface_image_stats; its distances carry fp32 rounding, and NSD compares the fp32 distance with tau.
    A cdist call sees at most `pairs` pairs: on the GPU, torch's exact-difference mode returned wrong distances for 4096 x 5330 points (2.2e7
    pairs; 1024 x 5330 were right, as was the CPU - DESIGN.md 4.4j), so the chunk shrinks with the other list's length."""
    percentile, tolerances = _surface_check(percentile, tuple(tolerances), "literal_surface_stats")
    keys = surface_keys(percentile, tolerances)

    def surface(m):
        p = torch.nn.functional.pad(m, (1, 1, 1, 1))
        return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])

    a = surface(pred == cls).nonzero().float()
    b = surface(label == cls).nonzero().float()
    n_p, n_g = a.shape[0], b.shape[0]
    if n_p + n_g == 0:
        return dict([(k, 1.0 if k.startswith("NSD@") else 0.0) for k in keys], defined=True)
    if n_p == 0 or n_g == 0:
        return dict([(k, 0.0 if k.startswith("NSD@") else None) for k in keys], defined=False)

    def directed(src, dst):
        chunk = max(1, int(pairs) // dst.shape[0])
        return torch.cat([torch.cdist(src[i:i + chunk], dst, compute_mode="donot_use_mm_for_euclid_dist").min(1)[0] for i in range(0, src.shape[0], chunk)])

    dp, dg = directed(a, b).double(), directed(b, a).double()
    both = torch.sort(torch.cat([dp, dg]))[0]
    n = n_p + n_g
    fl, rem = divmod(percentile * (n - 1), 100)
    lo, hi = float(both[fl]), float(both[min(fl + 1, n - 1)])
    out = {"HD": float(both[-1]), keys[1]: lo + (rem / 100.0) * (hi - lo), "ASSD": 0.5 * (float(dp.mean()) + float(dg.mean()))}
    for t, k in zip(tolerances, keys[3:]):
        out[k] = float(int((dp <= t).sum()) + int((dg <= t).sum())) / n
    out["defined"] = True
    return out


class SurfaceMeter(object):
    """Dataset aggregation of surface_image_stats: HD, HD<percentile> and ASSD are means over the images where they are defined (0 when there is
    none), NSD a mean over all images; `undefined` counts the images with exactly one empty mask."""

    def __init__(self, percentile=95, tolerances=(2.0,)):
        self.percentile, self.tolerances = _surface_check(percentile, tuple(tolerances), "SurfaceMeter")
        self.keys = surface_keys(self.percentile, self.tolerances)
        self.reset()

    def reset(self):
        self.sums = {k: 0.0 for k in self.keys}
        self.count = 0
        self.undefined = 0

    def update(self, stats):
        self.count += 1
        if not stats["defined"]:
            self.undefined += 1
        for k in self.keys:
            if k.startswith("NSD@") or stats["defined"]:
                self.sums[k] += float(stats[k])

    def as_dict(self):
        n_all, n_def = float(max(self.count, 1)), float(max(self.count - self.undefined, 1))
        out = {k: self.sums[k] / (n_all if k.startswith("NSD@") else n_def) for k in self.keys}
        out["images"] = self.count
        out["undefined"] = self.undefined
        return out

    def summary(self, logger):
        r = self.as_dict()
        logger.info("Surface metric, val result over {} images ({} undefined): HD/{} {:.4f}/{:.4f}, ASSD {:.4f}.".format(
            r["images"], r["undefined"], self.keys[1], r["HD"], r[self.keys[1]], r["ASSD"]))
        if self.tolerances:
            logger.info("Surface metric, val result: " + ", ".join("{} {:.4f}".format(k, r[k]) for k in self.keys[3:]) + ".")


# ----------------------------------------------------------------------------- lesion-wise metrics and mask clean-up (TEST.LESION_METRICS, TEST.MASK_*)
LESION_INTS = 12                        # MI_LESION_INTS of include/mi355seg.h, where the definition stands
LESION_FIELDS = ("pred_pixels", "kept_pixels", "lesion_pixels", "pred_components", "kept_components", "lesions", "true_positives", "detected",
                 "largest_pred", "largest_lesion", "overlap_pixels", "removed_components")
LESION_DEFAULTS = {"LESION_METRICS": False, "LESION_CONNECTIVITY": 8, "LESION_OVERLAP": 0.0, "MASK_MIN_AREA": 0, "MASK_KEEP_LARGEST": False}


def _lesion_check(connectivity, overlap, min_area, keep_largest, names=("connectivity", "overlap", "min_area", "keep_largest")):
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
        raise ValueError("%s %r must be 4 or 8" % (names[0], connectivity))
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float, np.integer, np.floating)) or not 0.0 <= overlap <= 1.0:
        raise ValueError("%s %r must be a number in [0, 1]" % (names[1], overlap))
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or min_area < 0:
        raise ValueError("%s %r must be an integer >= 0" % (names[2], min_area))
    if not isinstance(keep_largest, bool):
        raise ValueError("%s %r must be True or False" % (names[3], keep_largest))
    return int(connectivity), float(overlap), int(min_area), keep_largest


def lesion_settings(cfg):
    """None while TEST.LESION_METRICS is False, TEST.MASK_MIN_AREA 0 and TEST.MASK_KEEP_LARGEST False (none a reference key; absent = these
    defaults), else (metrics, connectivity, overlap, min_area, keep_largest): LESION_METRICS, LESION_CONNECTIVITY (4 or 8), LESION_OVERLAP (a
    share in [0, 1]), MASK_MIN_AREA (pixels, >= 0), MASK_KEEP_LARGEST.  Every key is checked whether or not the feature is on."""
    test = cfg.TEST
    v = {k: (test[k] if k in test else d) for k, d in LESION_DEFAULTS.items()}
    if not isinstance(v["LESION_METRICS"], bool):
        raise ValueError("TEST.LESION_METRICS %r must be True or False" % (v["LESION_METRICS"],))
    rest = _lesion_check(v["LESION_CONNECTIVITY"], v["LESION_OVERLAP"], v["MASK_MIN_AREA"], v["MASK_KEEP_LARGEST"],
                         ("TEST.LESION_CONNECTIVITY", "TEST.LESION_OVERLAP", "TEST.MASK_MIN_AREA", "TEST.MASK_KEEP_LARGEST"))
    if not (v["LESION_METRICS"] or rest[2] > 0 or rest[3]):
        return None
    return (v["LESION_METRICS"],) + rest


def require_no_lesion(cfg, who):
    """Components are labelled on PranetTester's binary masks: testers of multi-class models refuse the keys rather than ignore them."""
    if lesion_settings(cfg) is not None:
        raise NotImplementedError("%s: TEST.LESION_METRICS / TEST.MASK_MIN_AREA / TEST.MASK_KEEP_LARGEST - lesion-wise metrics and component "
                                  "filtering exist for PranetTester only; leave them at False / 0 / False" % (who,))


def lesion_image_stats(ints):
    """One image's row of mi_lesion_score's ints [12] (or the same numbers counted elsewhere) as a dict of Python ints under LESION_FIELDS, plus
    false_positives (kept components that are no true positive) and missed (lesions not detected).  The definitions: include/mi355seg.h."""
    ints = np.asarray(ints.cpu() if isinstance(ints, torch.Tensor) else ints).astype(np.int64)
    if ints.shape != (LESION_INTS,):
        raise ValueError("lesion_image_stats: ints must be [%d], got %s" % (LESION_INTS, ints.shape))
    s = {k: int(v) for k, v in zip(LESION_FIELDS, ints)}
    if ((ints < 0).any() or s["removed_components"] != s["pred_components"] - s["kept_components"] or s["true_positives"] > s["kept_components"]
            or s["detected"] > s["lesions"] or s["kept_pixels"] > s["pred_pixels"] or s["overlap_pixels"] > min(s["kept_pixels"], s["lesion_pixels"])):
        raise ValueError("lesion_image_stats: the integers %r contradict each other" % (ints.tolist(),))
    s["false_positives"] = s["kept_components"] - s["true_positives"]
    s["missed"] = s["lesions"] - s["detected"]
    return s


def _ratio_or_none(num, den):
    return float(num) / float(den) if den else None


class LesionMeter(object):
    """Dataset aggregation of lesion_image_stats.  Sums over the images, then lesion recall = detected / lesions, component precision = true
    positives / kept components, their F1, false positives per image; the images with a lesion and none detected, the images without a lesion and
    a (kept) prediction; what the filter removed.  A ratio whose denominator is 0 is None, not 0 or 1."""
    SUMS = ("lesions", "detected", "kept_components", "true_positives", "false_positives", "removed_components")

    def __init__(self):
        self.reset()

    def reset(self):
        self.sums = {k: 0 for k in self.SUMS}
        self.removed_pixels = 0
        self.count = 0
        self.images_missed = 0
        self.images_false_alarm = 0

    def update(self, stats):
        self.count += 1
        for k in self.SUMS:
            self.sums[k] += int(stats[k])
        self.removed_pixels += int(stats["pred_pixels"]) - int(stats["kept_pixels"])
        self.images_missed += 1 if stats["lesions"] > 0 and stats["detected"] == 0 else 0
        self.images_false_alarm += 1 if stats["lesions"] == 0 and stats["kept_components"] > 0 else 0

    def as_dict(self):
        s = self.sums
        recall, precision = _ratio_or_none(s["detected"], s["lesions"]), _ratio_or_none(s["true_positives"], s["kept_components"])
        f1 = None if recall is None or precision is None or recall + precision == 0 else 2.0 * recall * precision / (recall + precision)
        out = {"images": self.count, "lesion_recall": recall, "component_precision": precision, "lesion_f1": f1,
               "false_positives_per_image": _ratio_or_none(s["false_positives"], self.count), "images_missed": self.images_missed,
               "images_false_alarm": self.images_false_alarm, "removed_pixels": self.removed_pixels}
        out.update(s)
        return out

    def summary(self, logger):
        r = self.as_dict()

        def f(v):
            return "n/a" if v is None else "{:.4f}".format(v)

        logger.info("Lesion metric, val result over {} images: recall {} ({}/{} lesions), precision {} ({}/{} components), F1 {}.".format(
            r["images"], f(r["lesion_recall"]), r["detected"], r["lesions"], f(r["component_precision"]), r["true_positives"], r["kept_components"],
            f(r["lesion_f1"])))
        logger.info("Lesion metric, val result: false positives per image {}, images missed {}, false alarms {}, removed components {}.".format(
            f(r["false_positives_per_image"]), r["images_missed"], r["images_false_alarm"], r["removed_components"]))


def literal_lesion_stats(pred, label, cls=1, connectivity=8, min_area=0, keep_largest=False, overlap=0.0, max_rounds=None):
    """What a user would write without mi_lesion_score, from torch ops on the inputs' device (pred, label [H,W]): every foreground pixel starts
    with its own linear index, the smallest index of the neighbourhood is propagated by max_pool2d on the negated indices until nothing changes
    (as many rounds as the longest path inside a component), areas and hits by bincount.  Returns (the 12 integers as a list, filtered uint8
    [H,W]).  A second derivation for tests and the yardstick of tools/lesion_bench.py; never on a product path.  max_rounds: give up with
    RuntimeError after that many rounds (the bench's guard against a spiral of a million pixels)."""
    connectivity, overlap, min_area, keep_largest = _lesion_check(connectivity, overlap, min_area, keep_largest)
    permille = int(round(1000 * overlap))
    H, W = pred.shape
    n = H * W
    idx = torch.arange(n, dtype=torch.float64, device=pred.device).view(1, 1, H, W)
    ninf = torch.full_like(idx, float("-inf"))
    pool = torch.nn.functional.max_pool2d

    def roots(fg):
        cur = torch.where(fg.view(1, 1, H, W), -idx, ninf)
        rounds = 0
        while True:
            rounds += 1
            if max_rounds is not None and rounds > max_rounds:
                raise RuntimeError("literal_lesion_stats: no fixed point after %d rounds" % max_rounds)
            if connectivity == 8:
                nxt = pool(cur, 3, 1, 1)
            else:
                nxt = torch.maximum(pool(cur, (3, 1), 1, (1, 0)), pool(cur, (1, 3), 1, (0, 1)))
            nxt = torch.where(fg.view(1, 1, H, W), nxt, ninf)
            if torch.equal(nxt, cur):
                return torch.where(fg, (-cur).view(H, W), torch.zeros((), dtype=torch.float64, device=pred.device)).long()
            cur = nxt

    P, G = pred == cls, label == cls
    rp, rg = roots(P), roots(G)
    area_p, area_g = torch.bincount(rp[P], minlength=n), torch.bincount(rg[G], minlength=n)
    keep = (area_p > 0) & (area_p >= min_area)
    if keep_largest and bool(keep.any()):
        top = torch.where(keep, area_p, torch.zeros_like(area_p))
        first = int((top == top.max()).nonzero()[0])                       # a tie: the smallest root
        keep = torch.zeros_like(keep)
        keep[first] = True
    F = P & keep[rp]
    hit_p, hit_g = torch.bincount(rp[F & G], minlength=n), torch.bincount(rg[G & F], minlength=n)
    tp = keep & (hit_p >= 1) & (1000 * hit_p >= permille * area_p)
    det = (area_g > 0) & (hit_g >= 1) & (1000 * hit_g >= permille * area_g)
    n_p, n_kept = int((area_p > 0).sum()), int(keep.sum())
    ints = [int(P.sum()), int(F.sum()), int(G.sum()), n_p, n_kept, int((area_g > 0).sum()), int(tp.sum()), int(det.sum()), int(area_p.max()),
            int(area_g.max()), int((F & G).sum()), n_p - n_kept]
    other = torch.full((), 1 if cls == 0 else 0, dtype=torch.uint8, device=pred.device)
    return ints, torch.where(F, torch.full((), cls, dtype=torch.uint8, device=pred.device), other)


# ----------------------------------------------------------------------------- io / logging
def soft_label_cross_entropy(pred, soft_label, pixel_weights=None):
    """utility.py:172-177 on materialised [N,C,H,W] tensors (API parity: AsppFada uses the fused kernel
    `PixelDiscriminator.soft_loss`, which never builds the full-resolution operands)."""
    loss = -soft_label.float() * torch.nn.functional.log_softmax(pred, dim=1)
    if pixel_weights is None:
        return torch.mean(torch.sum(loss, dim=1))
    return torch.mean(pixel_weights * torch.sum(loss, dim=1))


class _GeneralizedDiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, eps, weight_type, ignore_label):
        from .. import kernels as K
        nhwc = output.permute(0, 2, 3, 1).contiguous()          # (GCPADecoder's outputs ARE NHWC memory: no copy)
        # the fused kernel at h == H, w == W: every interpolation weight is 0, the upsample is the identity
        out, d, _ = K.upsample_gdl(nhwc, target.contiguous(), want_grad=ctx.needs_input_grad[0], ignore_index=ignore_label, weight_type=weight_type,
                                   eps=eps, align_corners=False)
        ctx.d = d
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, gout, _gcounts):
        d, ctx.d = ctx.d, None
        return (d * gout).permute(0, 3, 1, 2), None, None, None, None


def GeneralizedDiceLoss(output, target, eps=1e-5, weight_type='square', ignore_label=255, with_counts=False):
    """utility.py:399-447, label form, on the HIP kernels (mi_upsample_gdl): output [N,C,H,W] fp32 logits on the GPU, target [N,H,W] labels.
    Unlike the reference it leaves `target` as it is (utility.py:421 overwrites its ignored entries with C), and labels outside [0, C) that are
    not ignore_label are left out and counted where F.one_hot would raise: with_counts=True (not in the reference) returns (loss, counts) with
    counts the call's own float32 [4] device tensor loss, valid pixels, such labels, 0 (kernels.check_labels).  The one-hot [N,C,H,W] target
    form and CPU tensors are refused."""
    if weight_type not in ("square", "identity", "sqrt"):
        raise ValueError('Check out the weight_type: ', weight_type)
    if output.dim() != 4:
        raise ValueError("GeneralizedDiceLoss: output must be [N,C,H,W] logits, got %s" % (tuple(output.shape),))
    if target.dim() != 3:
        raise NotImplementedError("GeneralizedDiceLoss: only the label form target [N,H,W] is implemented (got %s: the one-hot [N,C,H,W] form is not)"
                                  % (tuple(target.shape),))
    if not (output.is_cuda and target.is_cuda):
        raise NotImplementedError("GeneralizedDiceLoss runs on the MI355X only (got %s / %s tensors): no CPU path exists" % (output.device, target.device))
    if tuple(target.shape) != (output.shape[0],) + tuple(output.shape[2:]):
        raise ValueError("GeneralizedDiceLoss: target %s does not match output %s" % (tuple(target.shape), tuple(output.shape)))
    loss, counts = _GeneralizedDiceFn.apply(output.float(), target.long(), float(eps), weight_type, int(ignore_label))
    return (loss, counts) if with_counts else loss


def LovaszSoftmax(output, target, ignore_label=255, bins=None):
    """Lovasz-Softmax (Berman, Triki, Blaschko, CVPR 2018; classes present, over the whole batch) written with torch ops on materialised tensors:
    output [N,C,H,W] logits (fp32, or fp64 kept as it is), target [N,H,W] labels; autograd does the backward.  Any device.  bins=None sorts the errors
    of every present class (the paper's form); bins=B orders them by the cell min(B - 1, floor(e * B)) instead - inside a cell the foreground pixels
    first, then the background pixels with their Jaccard increments averaged - which is what the fused heads compute with B = 1024
    (mi_upsample_lovasz) and lies within 1 / B below the sorted loss.  Labels outside [0, C) are left out like ignore_label; no valid pixel: nan.
    The literal form: it exists for comparisons (tools/gald_bench.py --literal, the tests), the trainers run the fused head."""
    if output.dim() != 4 or target.dim() != 3 or tuple(target.shape) != (output.shape[0],) + tuple(output.shape[2:]):
        raise ValueError("LovaszSoftmax: output [N,C,H,W] logits and target [N,H,W] labels, got %s and %s" % (tuple(output.shape), tuple(target.shape)))
    if bins is not None and (int(bins) != bins or bins < 1):
        raise ValueError("LovaszSoftmax: bins must be None (sorted) or a positive integer, got %r" % (bins,))
    C = output.shape[1]
    p = torch.softmax(output if output.dtype == torch.float64 else output.float(), dim=1).permute(0, 2, 3, 1).reshape(-1, C)
    y = target.reshape(-1).long()
    valid = (y != ignore_label) & (y >= 0) & (y < C)
    p, y = p[valid], y[valid]
    losses = []
    for c in range(C):
        fg = y == c
        if not bool(fg.any()):
            continue
        e = torch.where(fg, 1.0 - p[:, c], p[:, c])
        if bins is None:
            es, perm = torch.sort(e, descending=True)
            f = fg[perm].to(e.dtype)
            G = f.sum()
            jac = 1.0 - (G - f.cumsum(0)) / (G + (1.0 - f).cumsum(0))
            g = torch.cat([jac[:1], jac[1:] - jac[:-1]])
            losses.append((es * g).sum())
        else:
            cell = (e.detach() * bins).floor().long().clamp_(0, int(bins) - 1)
            F = torch.bincount(cell[fg], minlength=int(bins)).double()
            N = torch.bincount(cell[~fg], minlength=int(bins)).double()
            G = F.sum()
            a = F.flip(0).cumsum(0).flip(0) - F          # pixels in strictly higher cells
            n = N.flip(0).cumsum(0).flip(0) - N
            g_fg, g_bg = 1.0 / (G + n), (G - a - F) / ((G + n) * (G + n + N))
            losses.append((e * torch.where(fg, g_fg[cell], g_bg[cell]).to(e.dtype)).sum())
    if not losses:
        return output.sum() * float("nan")
    return torch.stack(losses).mean()


def load_json(path):
    with open(path, "r") as f:
        return json.load(f)


def dump_json(path, data):
    with open(path, "w") as f:
        json.dump(data, f)


def setup_logger(name, save_dir, distributed_rank=None):
    """utility.py:238-249 (same format string / handlers); creates save_dir, and only rank 0 writes the file."""
    os.makedirs(save_dir, exist_ok=True)
    logger = logging.getLogger(name)
    logger.setLevel(logging.INFO)
    logger.propagate = False
    if not logger.handlers:
        fmt = logging.Formatter("%(asctime)s [%(levelname)s] %(message)s")
        if not distributed_rank:
            fh = logging.FileHandler(os.path.join(save_dir, name + ".txt"))
            fh.setFormatter(fmt)
            logger.addHandler(fh)
        sh = logging.StreamHandler()
        sh.setFormatter(fmt)
        logger.addHandler(sh)
    return logger
