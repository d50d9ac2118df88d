"""Mean-teacher self-training with ClassMix around the DeepLabV2 path (not in the reference): the online form of the reference's last two
adaptation stages - pseudo-labels written by `test.py --saveres`, then self-distillation on those files - as DACS and DAFormer run it.

One iteration: an EMA teacher labels the target batch inside the step, ClassMix pastes half of each source image's classes onto the target image
of the same index, and the student (an ASPPTrainer) trains on the source and the mixed images as one batch.  No second run over the target set, no
pseudo-label files, no stale labels.

On the device (csrc/classmix.hip): the class selection (mi_label_classes + the per-workgroup selection of mi_classmix), the pseudo-label and mixing
pass (mi_classmix: the evaluation tail's per-pixel arithmetic, so the [B,K,H,W] probability map is never written) and the teacher's EMA update
(mi_ema_update).  The teacher's forward is the bf16 engine with frozen BatchNorm in eval(); its operands are re-packed by the one-launch pack after
every update.  AsppClassMix mirrors AsppFada's shape: same constructor, train_step, train, _save_checkpoint and the FUSED switch.
"""
import datetime
import os
import time

import torch
import torch.nn.functional as F

from .. import kernels as K
from .metrics import MetricLogger, adjust_learning_rate, dump_json, setup_logger, strip_prefix_if_present
from .plugin import require_loss
from .trainer import ASPPTrainer


class ClassMixStudent(ASPPTrainer):
    """The student: an ASPPTrainer that reads SOLVER.EMA_ALPHA / SOLVER.MIX_THRESHOLD for its combo (plugin.self_train_options)."""
    SELF_TRAINING = True


def ema_alpha(it, ceiling):
    """The teacher's decay in iteration `it` (counted from 0): min(1 - 1 / (it + 1), SOLVER.EMA_ALPHA).  0 in the first iteration - the update
    copies the student -, 1/2, 2/3, ... until the ceiling takes over."""
    return min(1.0 - 1.0 / (it + 1), float(ceiling))


def draw_priorities(iteration, rank, batch, num_classes):
    """priority [batch, num_classes] uint8 on the host, every row a permutation of 0..num_classes-1, from a torch.Generator seeded from the
    iteration and the rank: what ClassMix's class selection (the ceil(n/2) present classes of smallest priority) is random in."""
    g = torch.Generator()
    g.manual_seed(int(iteration) * 65537 + int(rank))
    return torch.stack([torch.randperm(num_classes, generator=g) for _ in range(batch)]).to(torch.uint8)


class AsppClassMix:
    """Source cross-entropy + cross-entropy on the ClassMix images labelled by an EMA teacher, one student step per iteration; checkpoints
    `AsppClassMix-{epoch}.pth` (the student under the usual keys: test.py evaluates it unchanged), `aspp_classmix_chart_params.json`."""
    trainer_cls = ClassMixStudent
    FUSED = True        # False: the literal composition from torch ops (F.interpolate, softmax, max, torch.where, mul_ / add_) on materialised tensors
    KEEP_MIX = False    # True: train_step leaves the mixed images and labels of its iteration in `last_mix` (the A/B of the two paths looks at them)

    def __init__(self, name, cfg, src_train_loader, tgt_train_loader, local_rank):
        who = type(self).__name__
        require_loss(cfg, who)          # the loss of both halves is the student's cross-entropy (with its weights / smoothing / focal keywords)
        if not cfg.MODEL.FREEZE_BN:
            raise NotImplementedError("{} needs MODEL.FREEZE_BN True: the source and the mixed images run through the student as ONE batch, which is the two "
                                      "passes only while BatchNorm treats every sample on its own, and the teacher runs in eval()".format(who))
        self.cfg = cfg
        self.logger = setup_logger(name + "_train", cfg.OUTPUT_DIR, local_rank)
        self.aspp = self.trainer_cls(name, cfg, src_train_loader, local_rank, self.logger)
        self.tgt_train_loader = tgt_train_loader
        self.alpha, self.threshold = self.aspp.self_train
        self.start_epoch = 1
        self.iteration = 0
        self._build_teacher()
        if cfg.resume:
            self._load_checkpoint(self.aspp.checkpoint)
        self.lr_data, self.loss_data, self.kept_data, self.pasted_data = [], [], [], []

    # -- the teacher: a second backbone + head with flat stores of its own, initialised from the student AFTER `resume` has been applied
    def _build_teacher(self):
        a = self.aspp
        self.teacher_feature_extractor = a.build_feature_extractor(self.cfg).to(a.device)
        self.teacher_classifier = a.build_classifier(self.cfg).to(a.device)
        for t, s in ((self.teacher_feature_extractor, a.feature_extractor), (self.teacher_classifier, a.classifier)):
            if hasattr(t, "ensure_flat") and a.device.type == "cuda":
                t.ensure_flat()
            t.load_state_dict(s.state_dict())          # copies into the teacher's own storage
            t.requires_grad_(False)
            t.eval()
        self._ema_a = torch.zeros(1, dtype=torch.float32, device=a.device)          # the decay, read by mi_ema_update from device memory

    def _load_checkpoint(self, checkpoint):
        """A checkpoint of this combo restores the teacher and the position; any other (a source-only Aspp-{epoch}.pth) leaves the teacher the
        student's copy and the schedule at iteration 0."""
        if "teacher_feature_extractor" not in checkpoint:
            return
        self.logger.info("Loading the teacher from {}".format(self.cfg.resume))
        self.teacher_feature_extractor.load_state_dict(strip_prefix_if_present(checkpoint["teacher_feature_extractor"], "module."))
        self.teacher_classifier.load_state_dict(strip_prefix_if_present(checkpoint["teacher_classifier"], "module."))
        self._teacher_changed()
        self.iteration = int(checkpoint.get("iteration", 0))
        if "mix_epoch" in checkpoint:
            self.start_epoch = checkpoint["mix_epoch"] + 1

    def _save_checkpoint(self, epoch, save_path):
        clone = lambda sd: {k: v.detach().clone() for k, v in sd.items()}          # un-share the flat storage
        a = self.aspp
        torch.save({
            "mix_epoch": epoch, "iteration": self.iteration,
            "feature_extractor": clone(a.feature_extractor.state_dict()), "classifier": clone(a.classifier.state_dict()),
            "optimizer_fea": a.optimizer_fea.state_dict(), "optimizer_cls": a.optimizer_cls.state_dict(),
            "teacher_feature_extractor": clone(self.teacher_feature_extractor.state_dict()),
            "teacher_classifier": clone(self.teacher_classifier.state_dict())}, save_path)

    def _teacher_changed(self):
        """The teacher's weights were written through raw pointers (mi_ema_update) or load_state_dict: bump its stores' generations and re-pack its
        bf16 operands now, with the existing one-launch pack (StageEngine.prepare) and the head's pack."""
        for m in (self.teacher_feature_extractor, self.teacher_classifier):
            store = getattr(m, "_store", None)
            if store is None:
                return
            store.generation += 1
        self.teacher_feature_extractor._engine.eval_mode = True
        self.teacher_feature_extractor._engine.prepare(False)
        self.teacher_classifier._engine.prepare(False)

    def _teacher_low(self, tgt_input):
        """The teacher's low-resolution logits [B,h,w,K] fp32 NHWC of the target batch: eval(), bf16 engine, no autograd."""
        with torch.no_grad():
            feat = self.teacher_feature_extractor(tgt_input)
            cls = self.teacher_classifier
            if not hasattr(cls, "_engine"):          # foreign modules (FUSED = False only: the fused kernels refuse what is not on the GPU)
                return cls(feat).permute(0, 2, 3, 1).contiguous().float()
            cls.ensure_flat()
            cls._engine.prepare(False)
            return cls._engine.forward(cls._nhwc(feat))

    def _ema_step(self, it):
        a = ema_alpha(it, self.alpha)
        pairs = ((self.teacher_feature_extractor, self.aspp.feature_extractor), (self.teacher_classifier, self.aspp.classifier))
        if self.FUSED and all(getattr(m, "_store", None) is not None for pair in pairs for m in pair):
            self._ema_a.copy_(torch.tensor([a], dtype=torch.float32).pin_memory(), non_blocking=True)
            for t, s in pairs:
                if t._store.total != s._store.total:
                    raise RuntimeError("teacher and student stores differ in layout ({} vs {} floats)".format(t._store.total, s._store.total))
                K.ema_update(t._store.data, s._store.data, self._ema_a)
        else:
            a32 = torch.tensor(a, dtype=torch.float32)
            b32 = (torch.tensor(1.0, dtype=torch.float32) - a32).item()          # the fp32 difference, as the kernel takes it
            with torch.no_grad():
                for t, s in pairs:
                    for pt, ps in zip(t.parameters(), s.parameters()):
                        pt.mul_(a32.item()).add_(ps.detach(), alpha=b32)
        self._teacher_changed()

    def _mix_literal(self, src_input, src_label, tgt_input, low, prio, batch, labels):
        """FUSED = False: the same selection, pseudo-labels and mixing from torch ops on materialised tensors (a [B,K,H,W] probability map)."""
        B, _, H, W = src_input.shape
        nc, ignore = low.shape[-1], self.cfg.INPUT.IGNORE_LABEL
        with torch.no_grad():
            prob = F.softmax(F.interpolate(low.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True), dim=1)
            conf, pseudo = prob.max(1)
            kept = conf >= self.threshold
            pseudo = torch.where(kept, pseudo, torch.full_like(pseudo, ignore))
            valid = (src_label >= 0) & (src_label < nc)
            safe = torch.where(valid, src_label, torch.zeros_like(src_label)).reshape(B, -1)
            hist = torch.zeros((B, nc), dtype=torch.int64, device=src_label.device).scatter_add_(1, safe, valid.reshape(B, -1).long())
            present = hist > 0
            key = torch.where(present, prio.long(), torch.full_like(prio, 255).long())
            rank = key.argsort(1).argsort(1)                                         # a class's rank among the present ones (priorities are permutations)
            chosen = present & (rank < (present.sum(1, keepdim=True) + 1) // 2)
            pasted = valid & chosen.gather(1, safe).reshape(B, H, W)
            batch[B:].copy_(torch.where(pasted.unsqueeze(1), src_input, tgt_input))
            labels[B:].copy_(torch.where(pasted, src_label, pseudo))
            return torch.stack((pasted.reshape(B, -1).sum(1), (kept & ~pasted).reshape(B, -1).sum(1)), 1)

    # -- one iteration -------------------------------------------------------------------------------------------------------------------------
    def train_step(self, src_input, src_label, tgt_input, max_iter):
        a, cfg = self.aspp, self.cfg
        if tuple(src_input.shape) != tuple(tgt_input.shape):
            raise ValueError("AsppClassMix pastes source pixels onto the target image of the same index: source and target batches must have one shape "
                             "(got {} and {}; set INPUT.SOURCE_INPUT_SIZE_TRAIN = INPUT.TARGET_INPUT_SIZE_TRAIN and equal batch halves)".format(
                                 tuple(src_input.shape), tuple(tgt_input.shape)))
        a._throttle()                 # at most two iterations in flight (host/trainer.py RUN_AHEAD)
        it = self.iteration
        lr = adjust_learning_rate(cfg.SOLVER.LR_METHOD, cfg.SOLVER.BASE_LR, it, max_iter, power=cfg.SOLVER.LR_POWER)
        for g in a.optimizer_fea.param_groups:
            g["lr"] = lr
        for g in a.optimizer_cls.param_groups:
            g["lr"] = lr * 10
        dev = a.device
        src_input = src_input.to(dev, non_blocking=True).float().contiguous()
        src_label = src_label.to(dev, non_blocking=True).long().contiguous()
        tgt_input = tgt_input.to(dev, non_blocking=True).float().contiguous()
        B, _, H, W = src_input.shape
        nc = cfg.MODEL.NUM_CLASSES
        low = self._teacher_low(tgt_input)
        # priorities: drawn on the host, copied from pinned memory (the caching host allocator keeps the block until the copy has run): no sync
        prio = draw_priorities(it, getattr(a, "rank", 0), B, nc)
        if dev.type == "cuda":
            prio = prio.pin_memory().to(dev, non_blocking=True)
        batch = torch.empty((2 * B, 3, H, W), dtype=torch.float32, device=dev)        # [source | mixed]: ONE student batch (BatchNorm is frozen)
        labels = torch.empty((2 * B, H, W), dtype=torch.int64, device=dev)
        batch[:B].copy_(src_input)
        labels[:B].copy_(src_label)
        if self.FUSED:
            present = K.label_classes(src_label, nc)
            counts = K.classmix(src_input, tgt_input, src_label, low, present, prio, self.threshold, cfg.INPUT.IGNORE_LABEL,
                                out_img=batch[B:], out_label=labels[B:]).counts
        else:
            counts = self._mix_literal(src_input, src_label, tgt_input, low, prio, batch, labels)
        a.optimizer_fea.zero_grad()
        a.optimizer_cls.zero_grad()
        feat, fmask = a._feature(batch)
        if hasattr(a.classifier, "loss"):
            loss = a.classifier.loss(feat, labels, cfg.INPUT.IGNORE_LABEL, **a.ce_kwargs, **fmask)      # the mean over the valid pixels of both halves
        else:                         # foreign modules, as ASPPTrainer.train_step treats them
            loss = F.cross_entropy(a.classifier(feat, labels.shape[-2:]), labels, ignore_index=cfg.INPUT.IGNORE_LABEL)
        loss.backward()
        if a.reducer is not None:
            a.reducer.finish()
        a.optimizer_fea.step()
        a.optimizer_cls.step()
        self._ema_step(it)
        self.iteration += 1
        if self.KEEP_MIX:
            self.last_mix = (batch[B:], labels[B:])
        return dict(loss=loss.detach(), counts=counts, lr=lr)

    def train(self):
        a = self.aspp
        save_to_disk = a.local_rank == 0 and getattr(a, "rank", 0) == 0
        n_it = min(len(a.train_loader), len(self.tgt_train_loader))
        if self.iteration == 0:
            self.iteration = (self.start_epoch - 1) * n_it
        max_iter = self.cfg.SOLVER.EPOCHS * n_it
        self.logger.info("#" * 20 + " Start Mean-Teacher ClassMix Training " + "#" * 20)
        meters = MetricLogger(delimiter="  ")
        a.feature_extractor.train()
        a.classifier.train()
        start, end = time.time(), time.time()
        pending = []          # (device loss, device counts, pixels, lr) not yet fetched

        def flush():
            for l, c, px, lr in pending:          # the only place the loss and the two ratios are read back
                v, (pasted, kept) = float(l), c.sum(0).tolist()
                kept_ratio, pasted_ratio = kept / max(px - pasted, 1), pasted / max(px, 1)
                meters.update(loss_seg=v, kept=kept_ratio, pasted=pasted_ratio)
                self.loss_data.append(v)
                self.lr_data.append(lr)
                self.kept_data.append(kept_ratio)
                self.pasted_data.append(pasted_ratio)
            pending.clear()

        for epoch in range(self.start_epoch, self.cfg.SOLVER.EPOCHS + 1):
            for loader in (a.train_loader, self.tgt_train_loader):      # DistributedSampler: new order per epoch
                sampler = getattr(loader, "sampler", None)
                if hasattr(sampler, "set_epoch"):
                    sampler.set_epoch(epoch)
            for (src_input, src_label, _), (tgt_input, _, _) in zip(a.train_loader, self.tgt_train_loader):
                data_time = time.time() - end
                r = self.train_step(src_input, src_label, tgt_input, max_iter)
                pending.append((r["loss"], r["counts"], src_label.numel(), r["lr"]))
                log_now = self.iteration % 20 == 0 or self.iteration == max_iter
                if log_now:
                    flush()
                meters.update(time=time.time() - end, data=data_time)
                end = time.time()
                if log_now and getattr(a, "rank", 0) == 0:
                    eta = str(datetime.timedelta(seconds=int(meters.time.global_avg * (max_iter - self.iteration))))
                    mem = torch.cuda.max_memory_allocated() / 1024.0 / 1024.0 if a.device.type == "cuda" else 0.0
                    self.logger.info(meters.delimiter.join(["Epoch: {epoch}", "eta: {eta}", "iter: {iter}", "{meters}", "lr: {lr:.6f}",
                                                            "ema: {ema:.4f}", "max mem: {memory:.0f}"]).format(
                        epoch=epoch, eta=eta, iter=self.iteration, meters=str(meters), lr=r["lr"], ema=ema_alpha(self.iteration - 1, self.alpha),
                        memory=mem))
            flush()
            if epoch % self.cfg.SOLVER.CHECKPOINT_PERIOD == 0 and save_to_disk:
                os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
                self._save_checkpoint(epoch, os.path.join(self.cfg.OUTPUT_DIR, "AsppClassMix-{}.pth".format(epoch)))
        total = time.time() - start
        self.logger.info("Total training time: {} ({:.4f} s / epoch)".format(str(datetime.timedelta(seconds=total)),
                                                                             total / max(self.cfg.SOLVER.EPOCHS, 1)))
        if save_to_disk:
            os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
            dump_json(os.path.join(self.cfg.OUTPUT_DIR, "aspp_classmix_chart_params.json"), {
                "learning rate": self.lr_data, "loss": self.loss_data, "kept pseudo-label ratio": self.kept_data, "pasted ratio": self.pasted_data})
