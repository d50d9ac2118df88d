"""FADA adversarial adaptation of the GALD model (HarDNet-68 encoder + GCPA decoder) on the MI355X engine.

Reference surface mirrored here (same constructor, attributes, checkpoint keys and chart file):
  GaldFada                      core/combos/gald_fada.py:13-203
  (its parts)                   GALDTrainer (host/gald.py), FADAAdapter + PixelDiscriminator (host/fada.py)

One iteration (gald_fada.py:69-136): source pass with the cross-entropy on out2 / T alone, soft labels clip(softmax(out2 / T), 0.9) from the
source and the target logits, the discriminator on HarDNet's 1/32-resolution output (1024 channels) for the target's adversarial loss, the
generator's Adam steps, then the discriminator's two losses and its Adam step.  The fused path never writes a [B,C,H,W] tensor: the source
loss is the upsample + cross-entropy kernel on linear2 / T, and each soft-label cross-entropy rebuilds the soft labels per pixel from linear2
(1/4 resolution, align_corners=False) while it upsamples the discriminator's logits (1/32, align_corners=True) - mi_upsample_softce_2grid.
The two domains differ in crop size and GALD normalises with batch statistics, so source and target run through the encoder separately, as
in the reference (AsppFada's one-batch trick needs frozen BatchNorm and equal crops).
"""
import datetime
import os
import time

import torch
import torch.nn.functional as F

from .fada import FADAAdapter, PixelDiscriminator
from .gald import GALDTrainer, take_bad_labels
from .metrics import MetricLogger, adjust_learning_rate, dump_json, setup_logger, soft_label_cross_entropy
from .plugin import require_loss


class GaldFada:
    """gald_fada.py:13-203: checkpoints `GaldFada-{epoch}.pth`, chart `gald_fada_chart_params.json`.  Single GPU: under WORLD_SIZE > 1 every
    rank trains its encoder and decoder on its own, as GALDTrainer does (the discriminator keeps FADAAdapter's gradient exchange)."""
    trainer_cls = GALDTrainer
    adapter_cls = FADAAdapter
    TEMPERATURE = 1.8
    FUSED = True        # False: the literal order of operations on materialised tensors (the in-repo A/B of the fused kernels)

    def __init__(self, name, cfg, src_train_loader, tgt_train_loader, local_rank):
        require_loss(cfg, type(self).__name__)          # its source loss is GCPADecoder.loss: cross-entropy on out2
        self.cfg = cfg
        self.logger = setup_logger(name + "_train", cfg.OUTPUT_DIR, local_rank)
        self.gald = self.trainer_cls(name, cfg, src_train_loader, local_rank, self.logger)
        self.fada = self.adapter_cls(cfg, tgt_train_loader, self.gald.device)
        if cfg.resume:
            self.fada._load_checkpoint(self.gald.checkpoint, self.logger)
        # linear5/4/3 (and the never-run dconv3 / ImageNet head) get no gradient here: torch's Adam skips a parameter whose .grad is None, so
        # after resuming from Gald-N.pth their non-zero moments must not keep moving them
        for opt in (self.gald.optimizer_enc, self.gald.optimizer_dec):
            opt.skip_unwritten = True
        self.lr_data, self.D_lr_data = [], []
        self.loss_seg_data, self.loss_adv_tgt_data, self.loss_D_src_data, self.loss_D_tgt_data = [], [], [], []
        self.iteration = 0

    def _save_checkpoint(self, adv_epoch, save_path):
        g, f = self.gald, self.fada
        torch.save({
            "adv_epoch": adv_epoch, "iteration": self.iteration, "encoder": g.encoder.state_dict(), "decoder": g.decoder.state_dict(),
            "optimizer_enc": g.optimizer_enc.state_dict(), "optimizer_dec": g.optimizer_dec.state_dict(),
            "model_D": f.model_D.state_dict(), "optimizer_D": f.optimizer_D.state_dict()}, save_path)

    @staticmethod
    def _reduce(part):
        if getattr(part, "reducer", None) is not None:
            part.reducer.finish()

    # -- one iteration, gald_fada.py:69-136 -----------------------------------------------------------------------------------------
    def train_step(self, src_input, src_label, tgt_input, max_iter):
        g, f = self.gald, self.fada
        enc, dec, D = g.encoder, g.decoder, f.model_D
        self.iteration += 1                                     # :69, before the learning rates (aspp_fada's order, not GALDTrainer's)
        lr = adjust_learning_rate(self.cfg.SOLVER.LR_METHOD, self.cfg.SOLVER.BASE_LR, self.iteration, max_iter, power=self.cfg.SOLVER.LR_POWER)
        lr_d = adjust_learning_rate(self.cfg.SOLVER.LR_METHOD, self.cfg.SOLVER.BASE_LR_D, self.iteration, max_iter, power=self.cfg.SOLVER.LR_POWER)
        for grp in g.optimizer_enc.param_groups:
            grp["lr"] = lr
        for grp in g.optimizer_dec.param_groups:
            grp["lr"] = lr * 10
        for grp in f.optimizer_D.param_groups:
            grp["lr"] = lr_d
        g.optimizer_enc.zero_grad()
        g.optimizer_dec.zero_grad()
        f.optimizer_D.zero_grad()
        dev = g.device
        src_input = src_input.to(dev, non_blocking=True)
        src_label = src_label.to(dev, non_blocking=True).long()
        tgt_input = tgt_input.to(dev, non_blocking=True)
        src_size, tgt_size = tuple(src_input.shape[-2:]), tuple(tgt_input.shape[-2:])
        T = self.TEMPERATURE
        ignore = self.cfg.INPUT.IGNORE_LABEL
        fused = self.FUSED and hasattr(dec, "loss") and hasattr(D, "soft_loss_grids")
        if fused:
            src_feats = enc(src_input)
            loss_seg = dec.loss(src_input, src_feats, src_label, ignore, temperature=T, **g.ce_kwargs)          # :80-88, out2 alone
            src_low = dec.last_low                              # linear2 [B,K,H/4,W/4] (detached) -> the source soft labels, inside the kernel
            loss_seg.backward()
            tgt_feats = enc(tgt_input)
            tgt_low = dec.low2(tgt_input, tgt_feats)            # :94-96: train-mode BatchNorm, no tape (its out2 feeds detached soft labels only)
            d_params = list(D.parameters())
            for p in d_params:                                  # their gradients from this loss are zeroed before use (:112)
                p.requires_grad_(False)
            try:
                loss_adv_tgt = D.soft_loss_grids(tgt_feats[3], tgt_low, 0, tgt_size, weight=0.001, temperature=T)
                loss_adv_tgt.backward()                         # reaches the encoder through feats[3] only
            finally:
                for p in d_params:
                    p.requires_grad_(True)
            g.optimizer_enc.step()
            g.optimizer_dec.step()
            f.optimizer_D.zero_grad()
            loss_D_src = D.soft_loss_grids(src_feats[3].detach(), src_low, 0, src_size, weight=0.5, temperature=T)
            loss_D_src.backward()
            loss_D_tgt = D.soft_loss_grids(tgt_feats[3].detach(), tgt_low, 1, tgt_size, weight=0.5, temperature=T)
            loss_D_tgt.backward()
            self._reduce(f)
            f.optimizer_D.step()
        else:                                                   # gald_fada.py:79-127 as written
            if getattr(g, "focal_gamma", 0.0) > 0.0:
                raise NotImplementedError("SOLVER.FOCAL_GAMMA runs inside the fused head (decoder.loss); the literal path does not know it")
            src_feats = enc(src_input)
            src_output = dec(src_input, src_feats)[-1].div(T)
            loss_seg = F.cross_entropy(src_output, src_label, ignore_index=ignore, weight=g.ce_weights, label_smoothing=g.ce_smoothing)
            loss_seg.backward()
            src_soft = F.softmax(src_output, dim=1).detach()
            src_soft[src_soft > 0.9] = 0.9
            tgt_feats = enc(tgt_input)
            tgt_output = dec(tgt_input, tgt_feats)[-1].div(T)
            tgt_soft = F.softmax(tgt_output, dim=1).detach()
            tgt_soft[tgt_soft > 0.9] = 0.9
            loss_adv_tgt = 0.001 * soft_label_cross_entropy(D(tgt_feats[3], tgt_size), torch.cat((tgt_soft, torch.zeros_like(tgt_soft)), dim=1))
            loss_adv_tgt.backward()
            g.optimizer_enc.step()
            g.optimizer_dec.step()
            f.optimizer_D.zero_grad()
            loss_D_src = 0.5 * soft_label_cross_entropy(D(src_feats[3].detach(), src_size), torch.cat((src_soft, torch.zeros_like(src_soft)), dim=1))
            loss_D_src.backward()
            loss_D_tgt = 0.5 * soft_label_cross_entropy(D(tgt_feats[3].detach(), tgt_size), torch.cat((torch.zeros_like(tgt_soft), tgt_soft), dim=1))
            loss_D_tgt.backward()
            self._reduce(f)
            f.optimizer_D.step()
        return dict(loss_seg=loss_seg.detach(), loss_adv_tgt=loss_adv_tgt.detach(), loss_D_src=loss_D_src.detach(),
                    loss_D_tgt=loss_D_tgt.detach(), lr=lr, lr_d=lr_d)

    def _check_labels(self):
        """Labels outside [0, K) that are not ignore_index: counted by the fused cross-entropy (torch's would device-assert), raised here."""
        bad = take_bad_labels(self.gald.decoder)
        if bad:
            raise ValueError("train labels: %d label values lie outside [0, %d) and are not ignore_index - torch.nn.CrossEntropyLoss "
                             "(gald_fada.py:88) would raise a device assert; map the label ids to train ids first" % (bad, self.cfg.MODEL.NUM_CLASSES))

    def train(self):
        save_to_disk = self.gald.local_rank == 0
        n_it = min(len(self.gald.train_loader), len(self.fada.tgt_train_loader))
        self.iteration = (self.fada.start_adv_epoch - 1) * n_it
        max_iter = self.cfg.SOLVER.EPOCHS * n_it
        self.logger.info("#" * 20 + " Start Adversarial Training " + "#" * 20)
        meters = MetricLogger(delimiter="  ")
        self.gald.encoder.train()
        self.gald.decoder.train()
        self.fada.model_D.train()
        start, end = time.time(), time.time()
        for epoch in range(self.fada.start_adv_epoch, self.cfg.SOLVER.EPOCHS + 1):
            for (src_input, src_label, _), (tgt_input, _, _) in zip(self.gald.train_loader, self.fada.tgt_train_loader):
                data_time = time.time() - end
                r = self.train_step(src_input, src_label, tgt_input, max_iter)
                vals = {k: float(r[k]) for k in ("loss_seg", "loss_adv_tgt", "loss_D_src", "loss_D_tgt")}
                self._check_labels()                            # (the losses were fetched above: the step is complete on the device)
                meters.update(loss_seg=vals["loss_seg"], loss_adv_tgt=vals["loss_adv_tgt"], loss_D=vals["loss_D_src"] + vals["loss_D_tgt"],
                              loss_D_src=vals["loss_D_src"], loss_D_tgt=vals["loss_D_tgt"])
                meters.update(time=time.time() - end, data=data_time)
                end = time.time()
                self.lr_data.append(r["lr"])
                self.D_lr_data.append(r["lr_d"])
                self.loss_seg_data.append(vals["loss_seg"])
                self.loss_adv_tgt_data.append(vals["loss_adv_tgt"])
                self.loss_D_src_data.append(vals["loss_D_src"])
                self.loss_D_tgt_data.append(vals["loss_D_tgt"])
                if self.iteration % 20 == 0 or self.iteration == max_iter:
                    eta = str(datetime.timedelta(seconds=int(meters.time.global_avg * (max_iter - self.iteration))))
                    mem = torch.cuda.max_memory_allocated() / 1024.0 / 1024.0 if self.gald.device.type == "cuda" else 0.0
                    self.logger.info(meters.delimiter.join(["Epoch: {epoch}", "eta: {eta}", "iter: {iter}", "{meters}", "lr: {lr:.6f}",
                                                            "max mem: {memory:.0f}"]).format(
                        epoch=epoch, eta=eta, iter=self.iteration, meters=str(meters), lr=r["lr"], memory=mem))
            if epoch % self.cfg.SOLVER.CHECKPOINT_PERIOD == 0 and save_to_disk:
                os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
                self._save_checkpoint(epoch, os.path.join(self.cfg.OUTPUT_DIR, "GaldFada-{}.pth".format(epoch)))
        total = time.time() - start
        self.logger.info("Total training time: {} ({:.4f} s / epoch)".format(str(datetime.timedelta(seconds=total)),
                                                                             total / max(self.cfg.SOLVER.EPOCHS, 1)))
        os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
        dump_json(os.path.join(self.cfg.OUTPUT_DIR, "gald_fada_chart_params.json"), {
            "learning rate": self.lr_data, "discriminator learning rate": self.D_lr_data, "segmentation loss": self.loss_seg_data,
            "target adversarial loss": self.loss_adv_tgt_data, "source discriminator loss": self.loss_D_src_data,
            "target discriminator loss": self.loss_D_tgt_data})
