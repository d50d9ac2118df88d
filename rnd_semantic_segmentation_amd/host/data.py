"""Dataset surface: `build_dataset(cfg, mode, is_source)` / `build_collate_fn(cfg)` with the reference's
signatures (core/datasets/build.py:5-30).

GTA5 / Cityscapes are read from disk when DATASETS.DATASET_DIR holds them (host/datasets.py decodes, csrc/augment.hip runs the `aspp`
transform on the batch).  So is Kvasir-SEG (DATASET_DIR/kvasir): the polyp_* names with AUG.NAME "pra" (PraNet; csrc/augment_pra.hip runs
the `pra` transform), the kvasir_* names with AUG.NAME "aspp" (two-class DeepLab).  Everything else - a synthetic dataset name, a polyp /
kvasir name under any other AUG.NAME, a dataset directory that does not exist - is backed by a synthetic generator, on which
BASELINE.json's configs are defined.
Both keep the TENSOR CONTRACT of the loader
(core/datasets/transform.py:31-46, cityscapes.py:137-151, defaults.py:21-24):
    image  float32 [3,H,W], RGB/255 then (x-mean)/std   (here: unit-variance noise of that shape)
    label  float32 [H,W] with train-ids 0..K-1 and 255 = ignore
    name   str
"""
import os

import torch
from torch.utils.data import Dataset

from . import synth


class SyntheticSegmentation(Dataset):
    def __init__(self, cfg, mode="train", is_source=True, length=None):
        self.num_classes = cfg.MODEL.NUM_CLASSES
        if mode == "train":
            w, h = cfg.INPUT.SOURCE_INPUT_SIZE_TRAIN if is_source else cfg.INPUT.TARGET_INPUT_SIZE_TRAIN
        else:
            w, h = cfg.INPUT.INPUT_SIZE_TEST
        self.size = (int(h), int(w))
        env = os.environ.get("MI_SYNTH_LEN")
        self.length = int(length if length is not None else (env if env else (64 if mode == "train" else 4)))
        self.seed0 = {"train": 1000, "val": 2000, "test": 3000}[mode] + (0 if is_source else 500)

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        h, w = self.size
        img = synth.synth_image(1, h, w, seed=self.seed0 + i)[0]
        lab = synth.synth_label(1, h, w, self.num_classes, seed=self.seed0 + i)[0]
        return torch.from_numpy(img), torch.from_numpy(lab), "synthetic_%06d" % i


class SyntheticPolyp(Dataset):
    """The polyp_train / polyp_val contract the PraNet trainer and tester consume (pranet_trainer.py:39-43, pranet_tester.py:27-34):
    image float32 [3,S,S] mean/std normalised, mask float32 [1,S,S] with values in {0, 1} (one or two smooth blobs), name.
    S = INPUT.TRAINSIZE in train mode (the reference's pra_trans resizes to it, augment.py:55-86), INPUT.INPUT_SIZE_TEST otherwise."""

    def __init__(self, cfg, mode="train", length=None):
        if mode == "train":
            self.size = (int(cfg.INPUT.TRAINSIZE), int(cfg.INPUT.TRAINSIZE))
        else:
            w, h = cfg.INPUT.INPUT_SIZE_TEST
            self.size = (int(h), int(w))
        env = os.environ.get("MI_SYNTH_LEN")
        self.length = int(length if length is not None else (env if env else (64 if mode == "train" else 4)))
        self.seed0 = {"train": 5000, "val": 6000, "test": 7000}[mode]

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        h, w = self.size
        img, mask = synth.synth_polyp(1, h, w, seed=self.seed0 + i)
        return torch.from_numpy(img[0]), torch.from_numpy(mask[0]), "synthetic_polyp_%06d" % i


def build_collate_fn(cfg):
    """core/datasets/build.py:5-13.  The reference's collate functions (core/datasets/func.py: attn_collate_fn, the missing pranet_collate_fn)
    turn numpy HWC images from disk into tensors; the synthetic datasets here already yield the tensors of the loader contract, so the
    default collation applies for every value of AUG.COLLATE ("attn" is the default of defaults.py and what the PraNet YAML inherits).  The
    datasets read from disk are batched by host/datasets.DeviceAugmentLoader, which brings its own collation."""
    return None


def real_dataset_root(cfg, name):
    """The directory a dataset name reads, when it is read from disk; None for every name and configuration that gets the synthetic data.
    GTA5 / Cityscapes: when the directory exists.  polyp_*: when it exists and AUG.NAME is "pra"; kvasir_*: when it exists and AUG.NAME is "aspp"."""
    from .datasets import DatasetCatalog
    name = str(name)
    if not cfg.DATASETS.DATASET_DIR:
        return None
    if "polyp" in name or "kvasir" in name:
        if cfg.AUG.NAME != ("pra" if "polyp" in name else "aspp"):
            return None
    elif not ("gta5" in name or "cityscapes" in name):
        return None
    root = DatasetCatalog.root(cfg, name)
    return root if root is not None and os.path.isdir(root) else None


def build_dataset(cfg, mode="train", is_source=True):
    assert mode in ["train", "val", "test"]
    name = cfg.DATASETS.SOURCE_TRAIN if (mode == "train" and is_source) else (cfg.DATASETS.TARGET_TRAIN if mode == "train" else cfg.DATASETS.TEST)
    polyp = "polyp" in str(name) or "kvasir" in str(name)       # dataset_path_catalog.py:36-51,99-106
    if real_dataset_root(cfg, name) is None:
        return SyntheticPolyp(cfg, mode) if polyp else SyntheticSegmentation(cfg, mode, is_source)
    if not polyp and cfg.AUG.NAME != "aspp":
        raise ValueError("AUG.NAME %r: datasets read from disk are transformed by the 'aspp' transform only (the reference's other transforms need "
                         "albumentations); set AUG.NAME to 'aspp' or point DATASETS.DATASET_DIR away from %s" % (cfg.AUG.NAME, real_dataset_root(cfg, name)))
    from .augment import AugmentSpec
    from .datasets import DatasetCatalog
    from .pra_augment import PraSpec
    split = mode if mode != "test" else str(cfg.DATASETS.TEST).split("_")[-1]          # build.py:28
    spec = PraSpec.from_cfg(cfg, mode) if "polyp" in str(name) else AugmentSpec.from_cfg(cfg, mode, is_source)
    return DatasetCatalog.get(cfg, name, split, num_classes=cfg.MODEL.NUM_CLASSES, transform=spec, cross_val=cfg.DATASETS.CROSS_VAL)
