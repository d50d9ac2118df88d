"""ASPPTester: the reference's evaluation loop (core/testers/aspp_tester.py:10-83): inference() -> argmax ->
confusion matrix + IoU meters -> summary + aspp_confusion_matrix.json.  Device-agnostic host logic (the
reference hard-codes .cuda(), aspp_tester.py:57-58); metrics are integer bincounts on the device."""
import os

import numpy as np
import torch

from .metrics import (BOUNDARY_MAPS, BOUNDARY_MAX_WIDTH, CURVE_BINS, PSEUDO_BINS, AverageMeter, boundary_accumulate, boundary_settings,
                      boundary_summary, boundary_width, class_threshold_settings, class_thresholds, classwise_pseudo_labels, classwise_settings,
                      confusion_matrix, crf_channel_scale, crf_refine_output, crf_settings, curves_accumulate, curves_settings, curves_summary,
                      dump_json, inference, intersectionAndUnionGPU, literal_histogram, literal_pseudo, multi_scale_inference, predict_and_score,
                      require_no_lesion, require_no_polyp_metrics, require_no_surface, score_settings, slide_inference, slide_plan, slide_settings,
                      strip_prefix_if_present, threshold_table, tta_settings)
from .modules import build_classifier, build_feature_extractor


class ASPPTester:
    build_feature_extractor = staticmethod(build_feature_extractor)
    build_classifier = staticmethod(build_classifier)

    def __init__(self, cfg, device, test_loader, logger, palette, trainid2name, saveres=False):
        self.cfg = cfg
        self.logger = logger
        self.test_loader = test_loader
        self.device = device
        self.palette = palette
        self.trainid2name = trainid2name
        self.saveres = saveres
        classwise_settings(cfg)                            # a stray TEST.PSEUDO_PORTION is refused before anything is built
        require_no_polyp_metrics(cfg, "ASPPTester")
        require_no_surface(cfg, "ASPPTester")
        require_no_lesion(cfg, "ASPPTester")
        self.crf = crf_settings(cfg)                       # TEST.CRF: None, or the parameters of kernels.crf_refine (a stray CRF_* key is refused)
        self.crf_scale = crf_channel_scale(cfg) if self.crf is not None else None
        self.slide = slide_settings(cfg)                   # TEST.SLIDE: None, or (crop, stride), each (h, w) (a stray SLIDE_* key is refused)
        self.boundary = boundary_settings(cfg)             # TEST.BOUNDARY: None, or the band widths (empty = 2 % of the label's diagonal)
        self.curves = curves_settings(cfg)                 # TEST.CURVES: None, or (ece_bins, target precision) (a stray CURVES_* key is refused)
        self.class_table = class_threshold_settings(cfg)   # TEST.PSEUDO_CLASS_THRESHOLDS: None, or one pseudo-label threshold per class
        self.feature_extractor = self.build_feature_extractor(cfg)
        self.feature_extractor.to(device)
        self.classifier = self.build_classifier(cfg)
        self.classifier.to(device)
        # Evaluation reproduces the reference's fp32 masks (BASELINE: argmax identical, mIoU equal): TEST.PRECISION "fp32"
        # (default) selects the exact-fp32 schedule, "bf16" the 4x faster training engine.
        precision = cfg.TEST.PRECISION if "PRECISION" in cfg.TEST else "fp32"
        for m in (self.feature_extractor, self.classifier):
            if hasattr(m, "set_precision") and device.type == "cuda":
                m.set_precision(precision)

    def _load_checkpoint(self):
        self.logger.info("Loading checkpoint from {}".format(self.cfg.resume))
        checkpoint = torch.load(self.cfg.resume, map_location=self.device)
        self.feature_extractor.load_state_dict(strip_prefix_if_present(checkpoint["feature_extractor"], "module."))
        self.classifier.load_state_dict(strip_prefix_if_present(checkpoint["classifier"], "module."))

    def save_distill(self, output, name):
        """aspp_tester.py:33-45: palette PNG of the argmax mask under PSEUDO_DIR/inference/<dataset>."""
        self.save_mask(output.cpu().numpy().squeeze().argmax(0).astype(np.uint8), name)

    def save_mask(self, mask, name):
        """The file save_distill writes, from a [H,W] uint8 mask (tensor or array) that is already an argmax / pseudo-label map."""
        from PIL import Image
        folder = os.path.join(self.cfg.PSEUDO_DIR, "inference", self.cfg.DATASETS.TEST)
        os.makedirs(folder, exist_ok=True)
        if isinstance(mask, torch.Tensor):
            mask = mask.cpu().numpy()
        mask = Image.fromarray(np.ascontiguousarray(mask, dtype=np.uint8))
        mask.putpalette(list(self.palette))
        mask.save(os.path.join(folder, name[0] + ".png"))

    def _literal_output(self, x, y, single, scales, flip):
        if self.slide is not None:
            output = slide_inference(self.feature_extractor, self.classifier, x, y, self.slide[0], self.slide[1], flip=flip)
        elif single:
            output = inference(self.feature_extractor, self.classifier, x, y, flip=False)     # [1,K,H,W]
        else:
            # the call aspp_tester.py:61 keeps commented out
            output = multi_scale_inference(self.feature_extractor, self.classifier, x, y, flip=flip, scales=list(scales))
        if self.crf is None:
            return output
        # TEST.CRF: everything downstream (argmax, thresholds, histogram, metrics, masks) works on the refined probabilities
        return crf_refine_output(output, x, tuple(y.shape[-2:]), self.crf_scale, self.crf)

    def test(self):
        num_classes = self.cfg.MODEL.NUM_CLASSES
        self.feature_extractor.eval()
        self.classifier.eval()
        self.meter = AverageMeter()
        cmt = torch.zeros(num_classes, num_classes, dtype=torch.int64)
        scales, flip = tta_settings(self.cfg)
        single = scales == (1.0,) and not flip
        fused, threshold = score_settings(self.cfg)
        classwise, portion, cap = classwise_settings(self.cfg)
        # one kernel after the logits (argmax, threshold, counts) instead of the probability map and the torch-op metrics: same integers, same files
        fused = fused and self.device.type == "cuda" and hasattr(self.classifier, "predict_mask_multi")
        if self.crf is not None:
            # the refinement needs the probability map the fused tail never writes: the literal path, whatever TEST.FUSED_SCORE says
            fused = False
            self.logger.info("TEST.CRF: {iters} mean-field iterations, window {window} x dilation {dilation}; scoring takes the literal path "
                             "on the refined map.".format(**self.crf))
        # TEST.PSEUDO_CLASSWISE: this loop is pass 1 - the metrics as ever, no masks, and the confidence histogram of the whole set on the device
        hist = torch.zeros(num_classes, PSEUDO_BINS, dtype=torch.int64, device=self.device) if classwise else None
        grid = None
        self.boundary_hist = self.boundary_size = None     # TEST.BOUNDARY: one int64 [5, K, D + 1] buffer on the device for the whole set
        # TEST.CURVES: int64 pr [K, 256, 2] and cal [ece_bins, 3] on the device for the whole set; every picture adds to them
        curves = None
        if self.curves is not None:
            curves = (torch.zeros(num_classes, CURVE_BINS, 2, dtype=torch.int64, device=self.device),
                      torch.zeros(self.curves[0], 3, dtype=torch.int64, device=self.device))
            self.logger.info("TEST.CURVES: precision-recall curves over {} thresholds per class, calibration over {} bins.".format(
                CURVE_BINS, self.curves[0]))
        table = self.class_table
        extra = {}                                         # keywords of predict_and_score that only these two keys add
        if curves is not None:
            extra["curves"] = curves
        if table is not None and self.saveres:
            extra["class_threshold"] = table
        for x, y, name in self.test_loader:
            x = x.to(self.device, non_blocking=True)
            y = y.to(self.device, non_blocking=True).long()
            if self.slide is not None and grid != tuple(x.shape[-2:]):
                grid = tuple(x.shape[-2:])
                rows, cols, (wh, ww) = slide_plan(grid, *self.slide)
                self.logger.info("TEST.SLIDE: {} x {} windows of {} x {}, stride {} over {} x {} pictures.".format(
                    len(rows), len(cols), wh, ww, " x ".join(str(s) for s in (self.slide[1][:1] if self.slide[1][0] == self.slide[1][1] else self.slide[1])), grid[0], grid[1]))
            if fused:
                r = predict_and_score(self.feature_extractor, self.classifier, x, y, flip=flip, scales=scales, num_classes=num_classes,
                                      ignore_index=self.cfg.INPUT.IGNORE_LABEL, threshold=0.0 if classwise else threshold, hist=hist,
                                      slide=self.slide, **extra)
                if self.saveres and not classwise:
                    self.save_mask(r.pred if r.pseudo is None else r.pseudo, name)
                if self.boundary is not None:
                    self._boundary_count(r.pred, y[0])
                cmt = cmt + r.cmt
                self.meter.update(*[t.numpy() for t in (r.intersection, r.union, r.target, r.output)])
                continue
            output = self._literal_output(x, y, single, scales, flip)
            pred = output.max(1)[1]
            if curves is not None:
                curves_accumulate(output, y[:1], num_classes, curves)
            if classwise:
                hist += literal_histogram(output, num_classes)
            elif self.saveres and table is not None:
                self.save_mask(literal_pseudo(output, table), name)
            elif self.saveres and threshold == 0:
                self.save_distill(output, name)
            elif self.saveres:
                top = output.max(1)
                self.save_mask(torch.where(top[0] >= threshold, pred, torch.full_like(pred, 255))[0], name)
            y0 = y[:1]                                    # inference() keeps image 0 only (utility.py:190)
            if self.boundary is not None:
                self._boundary_count(pred[0].to(torch.uint8), y0[0])
            cmt = cmt + confusion_matrix(self.cfg, torch.flatten(pred), torch.flatten(y0))
            inter, union, target, res = intersectionAndUnionGPU(pred, y0, num_classes, self.cfg.INPUT.IGNORE_LABEL)
            self.meter.update(*[t.cpu().numpy() for t in (inter, union, target, res)])
        self.meter.summary(self.logger, num_classes)
        os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
        dump_json(os.path.join(self.cfg.OUTPUT_DIR, "aspp_confusion_matrix.json"),
                  {"cmt": cmt.tolist(), "classes": list(self.trainid2name.values())})
        if self.boundary is not None:
            self._boundary_report()
        if curves is not None:
            self._curves_report(curves)
        if classwise:
            self._classwise_masks(hist, portion, cap, fused, single, scales, flip)
        return cmt

    def _boundary_count(self, pred, label):
        """TEST.BOUNDARY, one picture: the mask the evaluation already has (uint8 [H,W]) and label 0 into the set's histograms.  The widths are
        fixed at the first label: the configured ones, or the 2 % width of its size."""
        size = tuple(label.shape[-2:])
        if self.boundary_hist is None:
            self.boundary_size = size
            self.boundary_widths = self.boundary if self.boundary else (boundary_width(size),)
            if self.boundary_widths[-1] > BOUNDARY_MAX_WIDTH:
                raise ValueError("TEST.BOUNDARY_WIDTHS (): 2 % of the diagonal of a {} x {} label is {} pixels, more than {}; set the widths".format(
                    size[0], size[1], self.boundary_widths[-1], BOUNDARY_MAX_WIDTH))
            self.boundary_hist = torch.zeros(BOUNDARY_MAPS, self.cfg.MODEL.NUM_CLASSES, self.boundary_widths[-1] + 1, dtype=torch.int64,
                                             device=label.device)
            self.logger.info("TEST.BOUNDARY: Boundary IoU and trimap IoU at band widths {}.".format(", ".join(str(d) for d in self.boundary_widths)))
        elif not self.boundary and size != self.boundary_size:
            raise ValueError("TEST.BOUNDARY_WIDTHS (): the band width is 2 % of the first label's diagonal ({} x {}), and this label is {} x {}; "
                             "set TEST.BOUNDARY_WIDTHS for a set of mixed sizes".format(*(self.boundary_size + size)))
        boundary_accumulate(pred, label, self.cfg.MODEL.NUM_CLASSES, self.cfg.INPUT.IGNORE_LABEL, self.boundary_widths[-1], self.boundary_hist)

    def _boundary_report(self):
        """After the loop of TEST.BOUNDARY: one device-to-host copy, one line per width and class, OUTPUT_DIR/aspp_boundary_metrics.json."""
        if self.boundary_hist is None:
            return
        self.boundary_hist = hist = self.boundary_hist.cpu()
        self.boundary_metrics = table = boundary_summary(hist, self.boundary_widths, list(self.trainid2name.values()))
        for i, d in enumerate(table["widths"]):
            self.logger.info("Boundary metric, width {}: mean Boundary IoU/trimap IoU {}/{}.".format(
                d, *("n/a" if v is None else "{:.4f}".format(v) for v in (table["mean_boundary_iou"][i], table["mean_trimap_iou"][i]))))
            for c, cls in enumerate(table["classes"]):
                self.logger.info("Boundary metric, width {}, class {} ({}): Boundary IoU/trimap IoU {}/{}.".format(
                    d, c, cls, *("n/a" if v is None else "{:.4f}".format(v) for v in (table["boundary_iou"][i][c], table["trimap_iou"][i][c]))))
        table = dict(table, max_width=int(hist.shape[2] - 1), hist=hist.tolist())
        dump_json(os.path.join(self.cfg.OUTPUT_DIR, "aspp_boundary_metrics.json"), table)

    def _curves_report(self, curves):
        """After the loop of TEST.CURVES: one device-to-host copy, one line per class and one for the set, OUTPUT_DIR/aspp_curves.json with the raw
        histograms, the summary (metrics.curves_summary) and the settings."""
        both = torch.cat([curves[0].flatten(), curves[1].flatten()]).cpu()
        n = curves[0].numel()
        self.curves_pr, self.curves_cal = pr, cal = both[:n].reshape(curves[0].shape), both[n:].reshape(curves[1].shape)
        self.curves_metrics = table = curves_summary(pr, cal, list(self.trainid2name.values()), self.curves[1])

        def show(v, spec="{:.4f}"):
            return "n/a" if v is None else spec.format(v)

        for c, cls in enumerate(table["classes"]):
            self.logger.info("Curves, class {} ({}): AP {}, best F1 {} at threshold {}, precision {} from threshold {} with recall {}.".format(
                c, cls, show(table["ap"][c]), show(table["best_f1"][c]), show(table["best_f1_threshold"][c]), table["target_precision"],
                show(table["threshold_at_precision"][c]), show(table["recall_at_precision"][c])))
        calib = table["calibration"]
        self.logger.info("Curves: mAP {}, ECE {}, MCE {}, accuracy {}, mean confidence {}.".format(
            show(table["map"]), show(calib["ece"]), show(calib["mce"]), show(calib["overall_accuracy"]), show(calib["mean_confidence"])))
        table = dict(table, ece_bins=self.curves[0], pr=pr.tolist(), cal=cal.tolist())
        dump_json(os.path.join(self.cfg.OUTPUT_DIR, "aspp_curves.json"), table)

    def _classwise_masks(self, hist, portion, cap, fused, single, scales, flip):
        """After pass 1 of TEST.PSEUDO_CLASSWISE: the thresholds from the histogram (one device-to-host copy), their table to the logger and to
        PSEUDO_DIR/inference/<dataset>/class_thresholds.json, and - with --saveres - pass 2 over the loader, which writes the masks with the
        table and does nothing else (the 1/8-resolution logits of pass 1 are not kept: a second backbone pass is cheap next to PNG encoding)."""
        num_classes = self.cfg.MODEL.NUM_CLASSES
        hist = hist.cpu()
        self.class_hist = hist
        self.class_thresholds = thresholds = class_thresholds(hist, portion, cap)
        names = list(self.trainid2name.values())
        names = names if len(names) == num_classes else None
        table = threshold_table(hist, thresholds, names)
        table.update(portion=portion, cap=cap)
        for c in range(num_classes):
            self.logger.info("Class-wise pseudo-labels, class {} ({}): {} pixels, threshold {:.6f}, kept {:.4f}.".format(
                c, table["classes"][c], table["pixels"][c], table["thresholds"][c], table["kept"][c]))
        folder = os.path.join(self.cfg.PSEUDO_DIR, "inference", self.cfg.DATASETS.TEST)
        os.makedirs(folder, exist_ok=True)
        dump_json(os.path.join(folder, "class_thresholds.json"), table)
        if not self.saveres:
            return
        for x, y, name in self.test_loader:
            x = x.to(self.device, non_blocking=True)
            y = y.to(self.device, non_blocking=True).long()
            if fused:
                mask = classwise_pseudo_labels(self.feature_extractor, self.classifier, x, y, flip=flip, scales=scales, num_classes=num_classes,
                                               class_threshold=thresholds, slide=self.slide)
            else:
                mask = literal_pseudo(self._literal_output(x, y, single, scales, flip), thresholds)
            self.save_mask(mask, name)
