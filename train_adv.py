"""Adversarial (FADA) training entry point: same flags as the reference's train_adv.py:62-105
(`-cfg FILE [--local_rank N] KEY VAL ...`) plus `--model` (the reference hard-codes main("gald_fada", ...) at :105 although
the DeepLab YAMLs need "aspp_fada"; `--model gald_fada -cfg configs/gald_adv.yaml` is the reference's default run; `--model aspp_classmix
-cfg configs/deeplabv2_r101_classmix.yaml` is the mean-teacher + ClassMix self-training of host/self_train.py, fed by the same two loaders).  Source and target loaders each carry BATCH_SIZE // 2 images (train_adv.py:29,39),
the target set is repeated 9x (:17).  Under torchrun (WORLD_SIZE > 1) it runs data-parallel over RCCL."""
import argparse
import os

import torch
import torch.distributed as dist
from torch.utils.data import ConcatDataset

from core.combos.aspp_fada import AsppFada
from core.configs import cfg
from core.datasets.build import build_collate_fn, build_dataset
from rnd_semantic_segmentation_amd.host.datasets import has_device_transform, run_trainer, wrap_loader


def main(name, cfg, local_rank):
    world = dist.get_world_size() if dist.is_initialized() else 1
    src = build_dataset(cfg, mode="train", is_source=True)
    tgt = ConcatDataset([build_dataset(cfg, mode="train", is_source=False)] * 9)
    per_rank = max(1, cfg.SOLVER.BATCH_SIZE // 2 // world)

    def loader(data, collate):
        sampler = torch.utils.data.distributed.DistributedSampler(data, shuffle=True, drop_last=True) if world > 1 else None
        # (datasets read from disk: 8 decode workers per loader, 16 per process; the transform runs on the GPU)
        return wrap_loader(data, batch_size=per_rank, shuffle=sampler is None, num_workers=8 if has_device_transform(data) else 4, pin_memory=True,
                           collate_fn=collate, sampler=sampler, drop_last=True)

    if name == "aspp_fada":
        combo = AsppFada
    elif name == "gald_fada":                                # what the reference's train_adv.py:105 runs (HarDNet-68 + GCPA decoder + FADA)
        from rnd_semantic_segmentation_amd.host.gald_fada import GaldFada
        combo = GaldFada
    elif name == "aspp_classmix":                            # not in the reference: online pseudo-labels from an EMA teacher + ClassMix
        from rnd_semantic_segmentation_amd.host.self_train import AsppClassMix
        combo = AsppClassMix
    else:
        raise NotImplementedError("combo %r: 'aspp_fada' (DeepLabV2-ResNet + ASPP + FADA), 'gald_fada' (GALD + FADA) and 'aspp_classmix' (DeepLabV2 + mean "
                                  "teacher + ClassMix) are on the MI355X hot path" % name)
    src_loader, tgt_loader = loader(src, build_collate_fn(cfg)), loader(tgt, None)
    run_trainer(combo(name, cfg, src_loader, tgt_loader, local_rank), src_loader, tgt_loader)


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="MI355X Semantic Segmentation Adversarial Training")
    parser.add_argument("-cfg", "--config-file", default="", metavar="FILE", help="path to config file", type=str)
    parser.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)))
    parser.add_argument("--model", default="aspp_fada", help="combo to run (the reference edits a literal instead)")
    parser.add_argument("opts", help="Modify config options using the command-line", default=None, nargs=argparse.REMAINDER)
    args = parser.parse_args()
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        torch.cuda.set_device(args.local_rank)
        dist.init_process_group(backend="nccl", init_method="env://")     # "nccl" is RCCL on ROCm
    cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts)
    cfg.freeze()
    main(args.model, cfg, args.local_rank)
