"""The reference's plugin API: base/base_trainer.py:7-53 (BaseTrainer) and base/base_model.py:6-30
(BaseModel), same constructor arguments, attributes and abstract methods."""
import logging
import time

import numpy as np
import torch
import torch.nn as nn

from ..kernels import FOCAL_GAMMA_MAX          # SOLVER.FOCAL_GAMMA's range in host/config.py is mi_upsample_ce_focal's
from .metrics import setup_logger


_LOSS_HOME = {"lovasz": "the Lovasz-Softmax loss ('lovasz') is wired into the fused heads of ASPPTrainer (configs/deeplabv2_r101_src_lovasz.yaml) and "
                        "GALDTrainer (configs/gald_src_lovasz.yaml); the FADA combos, AsppClassMix and PraNet do not train with it",
              "gdl": "the generalized Dice loss ('gdl') is wired into GALD: GALDTrainer (configs/gald_src_dice.yaml)",
              "ohem": "online hard example mining ('ohem') is wired into the fused cross-entropy heads of ASPPTrainer (configs/deeplabv2_r101_src_ohem.yaml) "
                      "and GALDTrainer (configs/gald_src_ohem.yaml)",
              "tversky": "the Tversky + BCE loss ('tversky') is wired into PraNet: PraNetTrainer (configs/pranet_src_polyp_tversky.yaml)"}


def require_loss(cfg, who, supported=("ce",)):
    """SOLVER.LOSS (not in the reference) names the segmentation criterion; GALDTrainer and PraNetTrainer each know one besides their default."""
    loss = getattr(getattr(cfg, "SOLVER", None), "LOSS", "ce")
    if loss not in supported:
        raise NotImplementedError("{} trains with SOLVER.LOSS {} only (got {!r}); {}".format(
            who, " / ".join(repr(s) for s in supported), loss, _LOSS_HOME.get(loss, "no trainer implements it")))
    weight = getattr(getattr(cfg, "SOLVER", None), "BOUNDARY_WEIGHT", 0.0)
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= weight < float("inf"):      # (a merged value was checked there; this one was assigned)
        raise ValueError("SOLVER.BOUNDARY_WEIGHT {!r} must be a finite number >= 0".format(weight))
    if weight > 0.0 and "tversky" not in supported:
        raise NotImplementedError("SOLVER.BOUNDARY_WEIGHT (the boundary loss) is wired into the fused Tversky + BCE heads of PraNetTrainer "
                                  "(configs/pranet_src_kvasir_boundary.yaml); {} does not know it".format(who))
    if weight > 0.0 and loss != "tversky":
        raise ValueError("SOLVER.BOUNDARY_WEIGHT {!r} needs SOLVER.LOSS 'tversky' (got {!r} for {}): the boundary term lives in the fused Tversky + BCE "
                         "heads".format(weight, loss, who))
    return loss


def ce_options(cfg, who, device=None):
    """SOLVER.CLASS_WEIGHTS / SOLVER.LABEL_SMOOTHING (not in the reference) as (weights, smoothing) for the trainer `who`: torch.nn.CrossEntropyLoss's
    weight= as a [NUM_CLASSES] fp32 tensor on `device`, or None when the key is empty, and its label_smoothing=.  Both belong to SOLVER.LOSS "ce" of the
    trainers whose "ce" is the cross-entropy; everything else refuses them instead of ignoring them."""
    solver = getattr(cfg, "SOLVER", None)
    weights = tuple(getattr(solver, "CLASS_WEIGHTS", ()) or ())
    smoothing = float(getattr(solver, "LABEL_SMOOTHING", 0.0))
    if not weights and smoothing == 0.0:
        return None, 0.0
    loss = getattr(solver, "LOSS", "ce")
    if loss == "ohem":
        raise NotImplementedError("SOLVER.LOSS 'ohem' cannot be combined with SOLVER.CLASS_WEIGHTS / SOLVER.LABEL_SMOOTHING yet ({}): the mining "
                                  "entry runs the plain cross-entropy".format(who))
    if loss != "ce":
        raise NotImplementedError("SOLVER.CLASS_WEIGHTS / SOLVER.LABEL_SMOOTHING belong to SOLVER.LOSS 'ce' (got {!r} for {})".format(loss, who))
    if who == "PraNetTrainer":
        raise NotImplementedError("PraNetTrainer's SOLVER.LOSS 'ce' is its structure loss (weighted BCE + IoU), which has neither class weights nor "
                                  "label smoothing; SOLVER.CLASS_WEIGHTS / SOLVER.LABEL_SMOOTHING are for ASPPTrainer, GALDTrainer and the FADA combos")
    if not 0.0 <= smoothing <= 1.0:          # (a value merged into the config was checked there; this one was assigned)
        raise ValueError("SOLVER.LABEL_SMOOTHING {} lies outside [0, 1]".format(smoothing))
    if not weights:
        return None, smoothing
    nc = int(cfg.MODEL.NUM_CLASSES)
    if len(weights) != nc:
        raise ValueError("SOLVER.CLASS_WEIGHTS has {} entries, MODEL.NUM_CLASSES is {} (one weight per class, or none)".format(len(weights), nc))
    vals = [float(v) for v in weights]
    for i, v in enumerate(vals):
        if not np.isfinite(v) or v < 0.0:
            raise ValueError("SOLVER.CLASS_WEIGHTS[{}] = {} (every weight must be finite and not negative)".format(i, v))
    return torch.tensor(vals, dtype=torch.float32, device=device), smoothing


OHEM_DEFAULTS = (0.7, 100000)          # SOLVER.OHEM_THRESH, SOLVER.OHEM_MIN_KEPT of host/config.py (GALDNet's published values)


def ohem_options(cfg, who):
    """SOLVER.OHEM_THRESH / SOLVER.OHEM_MIN_KEPT (not in the reference) as (thresh, min_kept) when SOLVER.LOSS is "ohem", else None.  The keys changed
    while SOLVER.LOSS is something else are refused instead of ignored."""
    solver = getattr(cfg, "SOLVER", None)
    thresh = getattr(solver, "OHEM_THRESH", OHEM_DEFAULTS[0])
    min_kept = getattr(solver, "OHEM_MIN_KEPT", OHEM_DEFAULTS[1])
    loss = getattr(solver, "LOSS", "ce")
    if loss != "ohem":
        if (thresh, min_kept) != OHEM_DEFAULTS:
            raise NotImplementedError("SOLVER.OHEM_THRESH / SOLVER.OHEM_MIN_KEPT belong to SOLVER.LOSS 'ohem' (got {!r} for {})".format(loss, who))
        return None
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or not 0.0 <= thresh <= 1.0:          # (a merged value was checked there; this one was assigned)
        raise ValueError("SOLVER.OHEM_THRESH {!r} lies outside [0, 1]".format(thresh))
    if isinstance(min_kept, bool) or not isinstance(min_kept, int) or min_kept < 1:
        raise ValueError("SOLVER.OHEM_MIN_KEPT {!r} must be an integer >= 1".format(min_kept))
    return float(thresh), int(min_kept)


def focal_options(cfg, who):
    """SOLVER.FOCAL_GAMMA (not in the reference) as a float for the trainer `who`: 0 = off, > 0 = the focal loss -w_y (1 - p_y)^gamma log p_y in place of
    SOLVER.LOSS "ce" inside the fused heads.  It composes with SOLVER.CLASS_WEIGHTS; whatever else it cannot modulate refuses it instead of ignoring it."""
    solver = getattr(cfg, "SOLVER", None)
    gamma = getattr(solver, "FOCAL_GAMMA", 0.0)
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not 0.0 <= gamma <= FOCAL_GAMMA_MAX:      # (a merged value was checked there; this one was assigned)
        raise ValueError("SOLVER.FOCAL_GAMMA {!r} lies outside [0, {:g}]".format(gamma, FOCAL_GAMMA_MAX))
    gamma = float(gamma)
    if gamma == 0.0:
        return 0.0
    loss = getattr(solver, "LOSS", "ce")
    if loss == "ohem":
        raise NotImplementedError("SOLVER.FOCAL_GAMMA cannot be combined with SOLVER.LOSS 'ohem' ({}): the mining entry runs the plain cross-entropy; "
                                  "focal loss is its smooth counterpart under SOLVER.LOSS 'ce'".format(who))
    if loss != "ce":
        raise NotImplementedError("SOLVER.FOCAL_GAMMA belongs to SOLVER.LOSS 'ce' (got {!r} for {})".format(loss, who))
    if float(getattr(solver, "LABEL_SMOOTHING", 0.0)) > 0.0:
        raise NotImplementedError("SOLVER.FOCAL_GAMMA cannot be combined with SOLVER.LABEL_SMOOTHING ({}): the focal entry modulates the cross-entropy "
                                  "of the hard labels (SOLVER.CLASS_WEIGHTS are fine)".format(who))
    if who == "PraNetTrainer":
        raise NotImplementedError("PraNetTrainer's SOLVER.LOSS 'ce' is its structure loss (weighted BCE + IoU), which SOLVER.FOCAL_GAMMA does not modulate; "
                                  "the key is for ASPPTrainer, GALDTrainer and the FADA combos")
    return gamma


LOVASZ_CE_DEFAULT = 1.0          # SOLVER.LOVASZ_CE of host/config.py


def lovasz_options(cfg, who):
    """SOLVER.LOVASZ_CE (not in the reference) as a float when SOLVER.LOSS is "lovasz" - the step's loss is Lovasz-Softmax + LOVASZ_CE * cross-entropy,
    0 = the Lovasz head alone - else None.  The key changed while SOLVER.LOSS is something else is refused instead of ignored.  (CLASS_WEIGHTS,
    LABEL_SMOOTHING, FOCAL_GAMMA and the OHEM keys under "lovasz" are refused by their own option readers: each belongs to another LOSS.)"""
    solver = getattr(cfg, "SOLVER", None)
    weight = getattr(solver, "LOVASZ_CE", LOVASZ_CE_DEFAULT)
    loss = getattr(solver, "LOSS", "ce")
    if loss != "lovasz":
        if weight != LOVASZ_CE_DEFAULT:
            raise NotImplementedError("SOLVER.LOVASZ_CE belongs to SOLVER.LOSS 'lovasz' (got {!r} for {})".format(loss, who))
        return None
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= weight < float("inf"):      # (a merged value was checked there; this one was assigned)
        raise ValueError("SOLVER.LOVASZ_CE {!r} must be a finite number >= 0".format(weight))
    return float(weight)


SELF_TRAIN_DEFAULTS = (0.99, 0.968)          # SOLVER.EMA_ALPHA, SOLVER.MIX_THRESHOLD of host/config.py (DACS's values)


def self_train_options(cfg, who, self_training=False):
    """SOLVER.EMA_ALPHA / SOLVER.MIX_THRESHOLD (not in the reference) as (alpha, threshold) for the student trainer of AsppClassMix (host/self_train.py),
    else None.  The keys changed under any other trainer or combo are refused instead of ignored."""
    solver = getattr(cfg, "SOLVER", None)
    alpha = getattr(solver, "EMA_ALPHA", SELF_TRAIN_DEFAULTS[0])
    thresh = getattr(solver, "MIX_THRESHOLD", SELF_TRAIN_DEFAULTS[1])
    if not self_training:
        if (alpha, thresh) != SELF_TRAIN_DEFAULTS:
            raise NotImplementedError("SOLVER.EMA_ALPHA / SOLVER.MIX_THRESHOLD belong to the mean-teacher + ClassMix combo (train_adv.py --model aspp_classmix); "
                                      "{} does not know them".format(who))
        return None
    for key, v in (("EMA_ALPHA", alpha), ("MIX_THRESHOLD", thresh)):          # (a merged value was checked there; this one was assigned)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
            raise ValueError("SOLVER.{} {!r} lies outside [0, 1]".format(key, v))
    return float(alpha), float(thresh)


class BaseTrainer:
    SELF_TRAINING = False     # True: the trainer is the student of a self-training combo, which reads SOLVER.EMA_ALPHA / SOLVER.MIX_THRESHOLD
    LOSSES = ("ce",)          # the criteria the trainer implements, as SOLVER.LOSS values
    MINED = ()                # SOLVER.LOSS values that are a LOSSES entry over mined pixels ("ohem" = "ce" over the hard pixels): accepted like LOSSES
    COMPOUND = ()             # SOLVER.LOSS values that add a term to a weighted LOSSES entry ("lovasz" = Lovasz-Softmax + LOVASZ_CE x "ce"): accepted like LOSSES

    def __init__(self, name, cfg, train_loader, local_rank, logger=None):
        require_loss(cfg, type(self).__name__, self.LOSSES + self.MINED + self.COMPOUND)
        who = "PraNetTrainer" if any(c.__name__ == "PraNetTrainer" for c in type(self).__mro__) else type(self).__name__
        weights, self.ce_smoothing = ce_options(cfg, who)          # CrossEntropyLoss(weight=, label_smoothing=): refused early where they do not apply
        self.ohem = ohem_options(cfg, who)                          # (thresh, min_kept) under SOLVER.LOSS "ohem", else None
        self.focal_gamma = focal_options(cfg, who)                  # SOLVER.FOCAL_GAMMA: > 0 = the focal loss in place of "ce", 0 = off
        self.lovasz = lovasz_options(cfg, who)                      # SOLVER.LOVASZ_CE under SOLVER.LOSS "lovasz", else None
        self.self_train = self_train_options(cfg, who, self.SELF_TRAINING)      # (EMA_ALPHA, MIX_THRESHOLD) for AsppClassMix's student, else None
        self.cfg = cfg
        self.logger = setup_logger(name + "_train", cfg.OUTPUT_DIR, local_rank) if logger is None else logger
        self.train_loader = train_loader
        self.local_rank = local_rank
        self.start_epoch = 1
        self.distributed = False
        self.lr_data = list()
        self.loss_data = list()
        if torch.cuda.is_available():
            self.with_cuda = True
            device = "cuda"
            if torch.cuda.device_count() > 1:
                self.distributed = True
            torch.cuda.empty_cache()
        else:
            self.logger.warning("Warning: There's no CUDA support on this machine, training is performed on CPU.")
            self.with_cuda = False
            device = "cpu"
        self.device = torch.device(device)
        self.ce_weights = None if weights is None else weights.to(self.device)          # created once, on the trainer's device
        # keywords for the fused heads' .loss() / .losses(); empty at the defaults, so those calls stay exactly what they were
        self.ce_kwargs = {"class_weights": self.ce_weights, "label_smoothing": self.ce_smoothing} if (weights is not None or self.ce_smoothing) else {}
        if self.ohem is not None:
            self.ce_kwargs = {"ohem": self.ohem}
        if self.focal_gamma > 0.0:          # (focal_options refused smoothing and "ohem"): the weights, if any, without label_smoothing
            self.ce_kwargs = {"focal_gamma": self.focal_gamma}
            if self.ce_weights is not None:
                self.ce_kwargs["class_weights"] = self.ce_weights
        if self.lovasz is not None:         # (the other readers refused their keys under "lovasz")
            self.ce_kwargs = {"lovasz": self.lovasz}
        self.init_params()
        if cfg.resume:
            self.logger.info("Loading checkpoint from {}".format(self.cfg.resume))
            self._load_checkpoint()

    def init_params(self):
        raise NotImplementedError

    def _train_epoch(self, epoch):
        raise NotImplementedError

    def _val_epoch(self, epoch):
        raise NotImplementedError

    def _save_checkpoint(self, epoch, save_path):
        raise NotImplementedError

    def _load_checkpoint(self):
        raise NotImplementedError

    def train(self):
        """Generic epoch loop (base_trainer.py:70-96); ASPPTrainer overrides it like the reference does."""
        best = None
        for epoch in range(self.start_epoch, self.epochs + 1):
            tic = time.time()
            train_log = self._train_epoch(epoch)
            self.logger.info("Epoch {} done in {:.1f}s: {}".format(epoch, time.time() - tic, train_log))
            if epoch % self.val_interval == 0 or epoch == self.epochs:
                val_log = self._val_epoch(epoch)
                score = val_log.get("val_f1")
                if best is None or (score is not None and score > best):
                    self.log = {**train_log, **val_log}
                    self._save_checkpoint(epoch, None)
                    best = score


class BaseModel(nn.Module):
    def __init__(self, config):
        super(BaseModel, self).__init__()
        self.config = config
        self.logger = logging.getLogger(self.__class__.__name__)

    def forward(self, *input):
        raise NotImplementedError

    def summary(self):
        params = sum(np.prod(p.size()) for p in self.parameters() if p.requires_grad)
        self.logger.info("Trainable parameters: {}".format(params))
        self.logger.info(self)
