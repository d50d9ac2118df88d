"""Config surface of the reference (`from core.configs import cfg`), re-implemented without yacs.

Reference: core/configs/defaults.py:5-91 builds a yacs CfgNode; scripts call
cfg.merge_from_file(yaml) / cfg.merge_from_list([K, V, ...]) / cfg.freeze()
(train_src.py:58-60, test.py:67-69).  yacs is not installed in this image, so this is a
small clone with the behaviours the scripts rely on: attribute access, YAML merge with
literal_eval of string leaves ('5e-4' -> float, 'None' -> None), type checking with
list<->tuple coercion, unknown-key rejection, freeze.
"""
import copy
from ast import literal_eval

import yaml

_VALID = (tuple, list, str, int, float, bool, type(None))
_RANGES = {"TEST.PSEUDO_THRESHOLD": (0.0, 1.0), "TEST.PSEUDO_PORTION": (0.0, 1.0), "SOLVER.TVERSKY_ALPHA": (0.0, 1.0), "SOLVER.LABEL_SMOOTHING": (0.0, 1.0),
           "SOLVER.OHEM_THRESH": (0.0, 1.0), "SOLVER.OHEM_MIN_KEPT": (1, float("inf")), "SOLVER.FOCAL_GAMMA": (0.0, 8.0),
           "SOLVER.EMA_ALPHA": (0.0, 1.0), "SOLVER.MIX_THRESHOLD": (0.0, 1.0), "SOLVER.LOVASZ_CE": (0.0, float("inf")),
           "SOLVER.BOUNDARY_WEIGHT": (0.0, float("inf"))}      # closed intervals a merged value has to lie in
_CHOICES = {"SOLVER.LOSS": ("ce", "gdl", "tversky", "ohem", "lovasz"), "SOLVER.GDL_WEIGHT": ("square", "identity", "sqrt")}      # the only values a merged key may take


class CfgNode(dict):
    IMMUTABLE = "__immutable__"

    def __init__(self, init=None):
        super().__init__()
        self.__dict__[CfgNode.IMMUTABLE] = False
        for k, v in (init or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) and not isinstance(v, CfgNode) else v

    # attribute access -------------------------------------------------------------------------
    def __getattr__(self, name):
        if name in self:
            return self[name]
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if self.is_frozen():
            raise AttributeError("Attempted to set {} to {}, but CfgNode is immutable".format(name, value))
        if name in self.__dict__:
            raise AttributeError("Invalid attempt to modify internal CfgNode state: {}".format(name))
        self[name] = value

    def is_frozen(self):
        return self.__dict__[CfgNode.IMMUTABLE]

    def _set_frozen(self, flag):
        self.__dict__[CfgNode.IMMUTABLE] = flag
        for v in self.values():
            if isinstance(v, CfgNode):
                v._set_frozen(flag)

    def freeze(self):
        self._set_frozen(True)

    def defrost(self):
        self._set_frozen(False)

    def clone(self):
        return copy.deepcopy(self)

    def __deepcopy__(self, memo):
        out = CfgNode()
        for k, v in self.items():
            dict.__setitem__(out, k, copy.deepcopy(v, memo))
        out.__dict__[CfgNode.IMMUTABLE] = self.is_frozen()
        return out

    # merging ----------------------------------------------------------------------------------
    @staticmethod
    def _decode(v):
        """yacs semantics: strings go through literal_eval when they parse ('5e-4', 'None', '[1, 2]')."""
        if isinstance(v, dict):
            return v
        if not isinstance(v, str):
            return v
        try:
            return literal_eval(v)
        except (ValueError, SyntaxError):
            return v

    @staticmethod
    def _coerce(new, old, key):
        if key in _RANGES and isinstance(new, (int, float)) and not isinstance(new, bool) and not _RANGES[key][0] <= new <= _RANGES[key][1]:
            raise ValueError("Value {} of config key {} lies outside [{}, {}]".format(new, key, *_RANGES[key]))
        if key in _CHOICES and new not in _CHOICES[key]:
            raise ValueError("Value {!r} of config key {} is not one of {}".format(new, key, ", ".join(_CHOICES[key])))
        if old is None or new is None or type(new) is type(old):
            return new
        for a, b in ((list, tuple), (tuple, list)):
            if isinstance(new, a) and isinstance(old, b):
                return b(new)
        if isinstance(old, float) and isinstance(new, int) and not isinstance(new, bool):
            return float(new)
        raise ValueError("Type mismatch ({} vs. {}) with values ({} vs. {}) for config key: {}".format(
            type(old), type(new), old, new, key))

    def _merge(self, other, path):
        for k, v in other.items():
            full = ".".join(path + [k])
            if k not in self:
                raise KeyError("Non-existent config key: {}".format(full))
            v = self._decode(copy.deepcopy(v))
            if isinstance(self[k], CfgNode):
                if not isinstance(v, dict):
                    raise ValueError("Config key {} expects a mapping".format(full))
                self[k]._merge(v, path + [k])
            else:
                if not isinstance(v, _VALID):
                    raise ValueError("Key {} with value {} is not a valid type".format(full, type(v)))
                dict.__setitem__(self, k, self._coerce(v, self[k], full))

    def merge_from_file(self, path):
        if self.is_frozen():
            raise AttributeError("CfgNode is immutable")
        with open(path, "r") as f:
            loaded = yaml.safe_load(f) or {}
        self._merge(loaded, [])

    def merge_from_other_cfg(self, other):
        self._merge(other, [])

    def merge_from_list(self, opts):
        if self.is_frozen():
            raise AttributeError("CfgNode is immutable")
        opts = list(opts or [])
        if len(opts) % 2:
            raise AssertionError("Override list has odd length: {}; it must be a list of pairs".format(opts))
        for full, v in zip(opts[0::2], opts[1::2]):
            node = self
            parts = full.split(".")
            for p in parts[:-1]:
                if p not in node:
                    raise KeyError("Non-existent key: {}".format(full))
                node = node[p]
            leaf = parts[-1]
            if leaf not in node:
                raise KeyError("Non-existent key: {}".format(full))
            dict.__setitem__(node, leaf, self._coerce(self._decode(v), node[leaf], full))

    def __str__(self):
        def fmt(node, indent):
            lines = []
            for k in sorted(node):
                v = node[k]
                if isinstance(v, CfgNode):
                    lines.append(" " * indent + "{}:".format(k))
                    lines.extend(fmt(v, indent + 2))
                else:
                    lines.append(" " * indent + "{}: {}".format(k, v))
            return lines

        return "\n".join(fmt(self, 0))

    __repr__ = __str__


def default_tree():
    """Same keys / default values as reference core/configs/defaults.py:7-91 (the YAML surface)."""
    return {
        "MODEL": {"NAME": "deeplab_resnet101", "NUM_CLASSES": 2, "DEVICE": "cuda", "WEIGHTS": "", "FREEZE_BN": False},
        "INPUT": {
            "TRAINSIZE": 352, "SOURCE_INPUT_SIZE_TRAIN": (1280, 720), "TARGET_INPUT_SIZE_TRAIN": (1024, 512),
            "INPUT_SIZE_TEST": (1024, 512), "INPUT_SCALES_TRAIN": (1.0, 1.0), "IGNORE_LABEL": 255,
            "PIXEL_MEAN": [0.485, 0.456, 0.406], "PIXEL_STD": [0.229, 0.224, 0.225], "TO_BGR255": False,
            "BRIGHTNESS": 0.0, "CONTRAST": 0.0, "SATURATION": 0.0, "HUE": 0.0, "HORIZONTAL_FLIP_PROB_TRAIN": 0.0,
        },
        "AUG": {"NAME": "attn", "BLUR_PROB": 0.7, "ROTATE_PROB": 0.7, "JITTER_PROB": 0.7, "FLIP_PROB": 0.7, "PROB": 0.7,
                "COLLATE": "attn"},
        "DATASETS": {"DATASET_DIR": "", "SOURCE_TRAIN": "", "TARGET_TRAIN": "", "VALIDATION": "", "TEST": "", "CROSS_VAL": 0},
        "SOLVER": {
            "EPOCHS": 5, "MAX_ITER": 16000, "STOP_ITER": 10000, "LR_METHOD": "poly", "BASE_LR": 0.02, "BASE_LR_D": 0.008,
            "LR_POWER": 0.9, "MOMENTUM": 0.9, "WEIGHT_DECAY": 0.0005, "WEIGHT_DECAY_BIAS": 0, "DECAY_RATE": 0.1,
            "DECAY_EPOCH": 50, "GAMMA": 0.1, "CHECKPOINT_PERIOD": 5, "BATCH_SIZE": 8, "BATCH_SIZE_VAL": 1,
            # not in the reference: LOSS "ce" = the trainers' cross-entropy, "gdl" = GeneralizedDiceLoss (utility.py:399-447) on GALD's four heads
            # (GALDTrainer only: the lines gald_trainer.py:70-73 toggles); GDL_WEIGHT = its weight_type, "square" | "identity" | "sqrt"
            # "tversky" = MultiscaleLoss(CompoundLoss([TverskyLoss(TVERSKY_ALPHA), BinaryCrossEntropyLoss()])) (attn/loss.py, as attn_trainer.py combines
            # them) on PraNet's four side outputs (PraNetTrainer only, whose "ce" is its own structure loss)
            "LOSS": "ce", "GDL_WEIGHT": "square", "TVERSKY_ALPHA": 0.7,
            # not in the reference either: BOUNDARY_WEIGHT (>= 0) times the boundary loss of Kervadec et al. (MIDL 2019), mean(sigmoid(z) * phi) with phi the
            # signed distance map of (gts >= 0.5) in pixels (mi_signed_distance, once per step on the device), added inside each of the four fused heads of
            # LOSS "tversky" (PraNetTrainer only; mi_upsample_tversky_bce_sdf).  phi is in pixels, so useful weights are small (0.01); 0 = off, the step
            # launches what it launched before the key existed.  Under any other LOSS or trainer a weight above 0 is refused (plugin.require_loss).
            "BOUNDARY_WEIGHT": 0.0,
            # not in the reference either: CLASS_WEIGHTS (empty, or one non-negative factor per class: tools/class_weights.py prints them) and
            # LABEL_SMOOTHING in [0, 1] are CrossEntropyLoss's weight= and label_smoothing= for LOSS "ce" of ASPPTrainer, GALDTrainer and both FADA
            # combos, inside the fused upsample + cross-entropy heads (mi_upsample_ce_w); any other loss or trainer refuses them (plugin.ce_options)
            "CLASS_WEIGHTS": (), "LABEL_SMOOTHING": 0.0,
            # LOSS "ohem" (ASPPTrainer, GALDTrainer) = online hard example mining, the criterion GALDNet, CCNet, OCNet and HRNet-Seg were published with:
            # cross-entropy over the pixels whose probability of the true class is at most max(OHEM_THRESH, the OHEM_MIN_KEPT-th smallest of the call),
            # inside the fused heads (mi_upsample_ce_ohem).  OHEM_MIN_KEPT counts full-resolution pixels of one head, one batch, one rank.  The two keys
            # changed under any other LOSS are refused (plugin.ohem_options), as is "ohem" together with CLASS_WEIGHTS / LABEL_SMOOTHING.
            "OHEM_THRESH": 0.7, "OHEM_MIN_KEPT": 100000,
            # not in the reference either: FOCAL_GAMMA in [0, 8] (0 = off) turns LOSS "ce" of ASPPTrainer, GALDTrainer and both FADA combos into the
            # focal loss -w_y (1 - p_y)^FOCAL_GAMMA log p_y inside the fused heads (mi_upsample_ce_focal): OHEM's smooth counterpart.  It composes with
            # CLASS_WEIGHTS; any other LOSS ("ohem" included), LABEL_SMOOTHING > 0 and PraNetTrainer refuse it (plugin.focal_options)
            "FOCAL_GAMMA": 0.0,
            # LOSS "lovasz" (ASPPTrainer, GALDTrainer) = Lovasz-Softmax (Berman et al., CVPR 2018; classes present, over the batch), the surrogate of the
            # Jaccard index itself, on a 1024-cell order inside the fused heads (mi_upsample_lovasz), plus LOVASZ_CE (>= 0) times the plain cross-entropy of
            # the same head: 1.0 is the sum people train with, 0 the Lovasz term alone (it trains poorly from scratch).  LOVASZ_CE changed under any other
            # LOSS is refused (plugin.lovasz_options); "lovasz" refuses CLASS_WEIGHTS, LABEL_SMOOTHING, FOCAL_GAMMA and the OHEM keys.
            "LOVASZ_CE": 1.0,
            # not in the reference either: the online form of pseudo-labelling + self-distillation, AsppClassMix (host/self_train.py; train_adv.py --model
            # aspp_classmix): EMA_ALPHA in [0, 1] is the ceiling of the mean teacher's decay, a = min(1 - 1 / (it + 1), EMA_ALPHA) in iteration it (from 0:
            # the first update copies the student); MIX_THRESHOLD in [0, 1] keeps a target pixel's pseudo-label where the teacher's winning probability
            # reaches it (0.968: DACS's value) and ignores the pixel below, inside the mixing kernel (mi_classmix).  Either key changed under any other
            # trainer or combo is refused (plugin.self_train_options)
            "EMA_ALPHA": 0.99, "MIX_THRESHOLD": 0.968,
        },
        # not in the reference: PRECISION fp32 = exact evaluation path, bf16 = training engine; SCALES / FLIP other than these defaults make
        # ASPPTester call multi_scale_inference (utility.py:193-209) instead of inference(flip=False); FUSED_SCORE True = argmax, threshold and
        # metric counts in the evaluation tail's kernel (False = the probability map and torch ops: same numbers and files);
        # PSEUDO_THRESHOLD in [0, 1]: saved masks hold 255 where the winning probability is below it (0 = the reference's plain argmax);
        # PSEUDO_CLASSWISE True = class-balanced pseudo-labels (CBST; the BDL / FADA self-distillation rule): one threshold per class, the
        # PSEUDO_PORTION quantile (0.5 = the median) of the confidences of the pixels predicted as that class over the whole test set, capped at
        # PSEUDO_THRESHOLD (0 = no cap); ASPPTester takes them from a histogram the evaluation tail accumulates, then writes the masks in a second
        # pass (metrics.classwise_settings; PSEUDO_PORTION changed while PSEUDO_CLASSWISE is False is refused);
        # POLYP_METRICS True (PranetTester only; the other testers refuse it) = besides the intersection / union lines, the polyp-segmentation
        # metrics PraNet is published with - mean Dice / IoU over 256 thresholds, F-beta, S-measure, E-measure, MAE - from one fused evaluation
        # tail (mi_polyp_score), logged and written to OUTPUT_DIR/pranet_polyp_metrics.json; labels must be 0 / 1;
        # SURFACE_METRICS True (PranetTester only; the other testers refuse it) = the surface-distance metrics of the medical segmentation
        # literature in medpy's conventions - Hausdorff distance, its SURFACE_PERCENTILE-th percentile (an integer in 1..100; HD95), average
        # symmetric surface distance, and surface Dice at each of SURFACE_TOLERANCES (at most 8 pixel distances >= 0) - measured exactly on the
        # device (mi_surface_score), logged and written to OUTPUT_DIR/pranet_surface_metrics.json; labels other than 1 are background
        # (metrics.surface_settings);
        # LESION_METRICS True (PranetTester only; the other testers refuse it) = lesion-wise detection rates from the connected components of the
        # mask and of the label (LESION_CONNECTIVITY 4 or 8), counted on the device (mi_lesion_score): a lesion is detected, and a predicted
        # component a true positive, when the other mask covers at least the share LESION_OVERLAP in [0, 1] of it (0 = any shared pixel) - lesion
        # recall, component precision, their F1, false positives per image - logged and written to OUTPUT_DIR/pranet_lesion_metrics.json.
        # MASK_MIN_AREA > 0 drops the predicted components of fewer pixels, MASK_KEEP_LARGEST True keeps only the largest of the rest, before
        # the intersection / union lines, the surface metrics and the lesion counts see the mask (the polyp metrics are measured on the soft map
        # and are not filtered); either filter key works with or without LESION_METRICS; labels other than 1 are background
        # (metrics.lesion_settings);
        # CRF True (ASPPTester only; the other testers refuse it) = the third part of DeepLabV2 as published, in its locally connected form: the
        # full-resolution probability map is refined by CRF_ITER mean-field iterations over a CRF_WINDOW x CRF_WINDOW window dilated by
        # CRF_DILATION, with a position kernel (weight CRF_POS_W, sigma CRF_POS_XY pixels) and a bilateral kernel (weight CRF_BI_W, sigmas
        # CRF_BI_XY pixels and CRF_BI_RGB in 0..255 colour units), in one HIP kernel family (mi_crf_refine) between the evaluation tail and the
        # argmax; the tester then takes the literal scoring path whatever FUSED_SCORE says.  The defaults are the customary dense-CRF values
        # (3 / 3, 10 / 80 / 13, 5 iterations); they are NOT tuned on any dataset here.  A CRF_* key changed while CRF is False is refused
        # (metrics.crf_settings);
        # SLIDE True (ASPPTester only; the other testers refuse it) = sliding-window evaluation, the protocol DeepLab and PSPNet report Cityscapes
        # under: the picture stays at INPUT_SIZE_TEST, windows of SLIDE_CROP (width, height; the size the net was trained on) are slid over it
        # with SLIDE_STRIDE, each is evaluated as inference() evaluates a picture (with FLIP: averaged with its mirror) and the windows'
        # probabilities are averaged where they overlap - on the fused path in one kernel after the windows' backbone passes
        # (mi_upsample_predict_score_slide).  SCALES must stay (1.0,); a SLIDE_* key changed while SLIDE is False is refused
        # (metrics.slide_settings);
        # BOUNDARY True (ASPPTester only; the other testers refuse it) = besides the region metrics, Boundary IoU (Cheng et al., CVPR 2021) and
        # DeepLab's trimap IoU per class: both restricted to the band of BOUNDARY_WIDTHS pixels (3 x 3 erosions) inside each class's contours,
        # counted on the mask the evaluation already has by one HIP kernel pair per picture (mi_boundary_score), whatever SCALES, FLIP, CRF, SLIDE
        # or the thresholds are; logged and written to OUTPUT_DIR/aspp_boundary_metrics.json.  BOUNDARY_WIDTHS () = 2 % of the label's diagonal
        # (46 at 1024 x 2048; every label must then have the first one's size), else strictly increasing integers in 1..64.  BOUNDARY_WIDTHS
        # changed while BOUNDARY is False is refused (metrics.boundary_settings);
        # CURVES True (ASPPTester only; the other testers refuse it) = what a confidence is worth on a labelled split: per class the
        # precision-recall curve over 256 probability thresholds (average precision, best F1, and the lowest threshold >= 0.5 whose
        # pseudo-labels reach the precision CURVES_PRECISION, with the recall kept there) and the calibration of the winning probability over
        # CURVES_ECE_BINS (1..64) bins (ECE, MCE, accuracy, mean confidence).  Integer histograms of the values the evaluation tail holds in
        # registers, counted by one more launch per picture (mi_upsample_curves / mi_upsample_curves_slide), or from the map on the literal
        # path (FUSED_SCORE False, CRF: then of the refined map); logged and written to OUTPUT_DIR/aspp_curves.json.  A CURVES_* key changed
        # while CURVES is False is refused (metrics.curves_settings);
        # PSEUDO_CLASS_THRESHOLDS = NUM_CLASSES thresholds in [0, 1] (() = off): with --saveres the pseudo-label masks keep a pixel where the
        # winning probability reaches its class's threshold, in a single pass - for instance the "pseudo_class_thresholds" of an
        # aspp_curves.json counted on a labelled split.  Refused together with PSEUDO_CLASSWISE or a non-zero PSEUDO_THRESHOLD
        # (metrics.class_threshold_settings)
        "TEST": {"BATCH_SIZE": 1, "PRECISION": "fp32", "SCALES": (1.0,), "FLIP": False, "FUSED_SCORE": True, "PSEUDO_THRESHOLD": 0.0,
                 "PSEUDO_CLASSWISE": False, "PSEUDO_PORTION": 0.5, "POLYP_METRICS": False,
                 "SURFACE_METRICS": False, "SURFACE_PERCENTILE": 95, "SURFACE_TOLERANCES": (2.0,),
                 "LESION_METRICS": False, "LESION_CONNECTIVITY": 8, "LESION_OVERLAP": 0.0, "MASK_MIN_AREA": 0, "MASK_KEEP_LARGEST": False,
                 "CRF": False, "CRF_ITER": 5, "CRF_WINDOW": 7, "CRF_DILATION": 4, "CRF_POS_W": 3.0, "CRF_POS_XY": 3.0, "CRF_BI_W": 10.0,
                 "CRF_BI_XY": 80.0, "CRF_BI_RGB": 13.0,
                 "SLIDE": False, "SLIDE_CROP": (769, 769), "SLIDE_STRIDE": (513, 513),
                 "BOUNDARY": False, "BOUNDARY_WIDTHS": (),
                 "CURVES": False, "CURVES_ECE_BINS": 15, "CURVES_PRECISION": 0.9, "PSEUDO_CLASS_THRESHOLDS": ()},
        "OUTPUT_DIR": ".",
        "resume": "",
        "PSEUDO_DIR": "",
    }


_C = CfgNode(default_tree())
cfg = _C   # `from core.configs import cfg` (reference core/configs/__init__.py:1)
