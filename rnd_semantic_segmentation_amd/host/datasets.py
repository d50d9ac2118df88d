"""GTA5 / Cityscapes from disk: the reference's dataset classes (core/datasets/gta5.py, cityscapes.py) and DatasetCatalog
(dataset_path_catalog.py) with their constructor signatures, decoding only.

The reference's __getitem__ runs the whole `aspp` transform on the CPU through PIL.  Here a dataset whose `transform` is a
host/augment.AugmentSpec (what build_dataset passes) returns what the DEVICE transform consumes - the decoded uint8 [H,W,3] image, the raw
uint8 [H,W] label ids and the name - and the DeviceAugmentLoader runs csrc/augment.hip on the batch.  A callable `transform` is still
honoured as in the reference: it receives (PIL RGB image, PIL mode-F label with the ids already mapped) and its result is returned.
Kvasir-SEG in folds (core/datasets/kvasir.py) is read the same way: KvasirFoldDataset with a host/pra_augment.PraSpec for PraNet (the `pra`
transform, csrc/augment_pra.hip), KvasirDataSet as a two-class set for the `aspp` transform.
PIL is imported when a dataset is constructed, not with this module.
"""
import os
from glob import glob

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import augment, pra_augment

# label id -> train id (data of the Cityscapes label definition; every other id is IGNORE), and the class names
TRAINID_19 = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 31: 16, 32: 17, 33: 18}
TRAINID_16 = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 23: 9, 24: 10, 25: 11, 26: 12, 28: 13, 32: 14, 33: 15}
NAMES_19 = ["road", "sidewalk", "building", "wall", "fence", "pole", "light", "sign", "vegetation", "terrain", "sky", "person", "rider", "car", "truck", "bus",
            "train", "motocycle", "bicycle"]
NAMES_16 = ["road", "sidewalk", "building", "wall", "fence", "pole", "light", "sign", "vegetation", "sky", "person", "rider", "car", "bus", "motocycle", "bicycle"]


def id_table(mapping, ignore_label=255):
    """uint8[256]: label id -> train id, everything else -> ignore_label (what the reference does with a float32 copy and one pass per id)."""
    t = np.full(256, ignore_label, np.uint8)
    for k, v in mapping.items():
        t[k] = v
    return t


class _DecodedSegmentation(Dataset):
    """Shared __getitem__: decode, then either hand the raw arrays on (device transform) or run a callable transform as the reference does."""

    def _setup(self, transform, ignore_label, debug):
        import PIL.Image  # noqa: F401  (fail here, not in a worker, when PIL is missing)
        self.transform = transform
        self.ignore_label = ignore_label
        self.debug = debug
        self.image_paths = []

    @property
    def device_transform(self):
        return isinstance(self.transform, (augment.AugmentSpec, pra_augment.PraSpec))

    def __len__(self):
        return len(self.image_paths)

    def _paths(self, index):
        raise NotImplementedError

    def __getitem__(self, index):
        from PIL import Image
        if self.debug:
            index = 0
        img_path, label_path, name = self._paths(index)
        image = Image.open(img_path).convert("RGB")
        ids = np.array(Image.open(label_path))
        if ids.ndim != 2:
            raise ValueError("%s: a single-channel label image is expected, got shape %s" % (label_path, ids.shape))
        wide = ids.dtype != np.uint8                                # 16-bit / 32-bit label files: an id outside 0..255 is in no table
        outside = ((ids < 0) | (ids > 255)) if wide else None
        if self.device_transform:
            if wide:
                void = np.flatnonzero(self.id_table == self.ignore_label)
                if outside.any() and void.size == 0:
                    raise ValueError("%s: label ids outside 0..255 and no id that maps to ignore_label" % label_path)
                ids = np.where(outside, void[0] if void.size else 0, ids).astype(np.uint8)
            return torch.from_numpy(np.array(image, dtype=np.uint8)), torch.from_numpy(np.ascontiguousarray(ids)), name
        label = self.id_table[np.where(outside, 0, ids).astype(np.uint8) if wide else ids].astype(np.float32)
        if wide:
            label[outside] = self.ignore_label
        label = Image.fromarray(label)
        if self.transform is not None:
            image, label = self.transform(image, label)
        return image, label, name


class GTA5FoldDataSet(_DecodedSegmentation):
    """core/datasets/gta5.py:15-91: folds are the sub-directories of data_root; train = folds whose name does not contain str(cross_val),
    every other mode = those that do; <fold>/images/*.png with <fold>/labels/<same name>."""

    def __init__(self, cfg, data_root, mode="train", cross_val=0, transform=None, debug=False, ignore_label=255):
        super().__init__()
        self._setup(transform, ignore_label, debug)
        self.cfg = cfg
        self.data_root = data_root
        self.mode = mode
        self.num_class = cfg.MODEL.NUM_CLASSES
        for fold in sorted(glob(data_root + "/*/")):
            inside = str(cross_val) in os.path.basename(fold[:-1])
            if inside != (mode == "train"):
                self.image_paths += glob(os.path.join(fold, "images") + "/*.png")
        # sorted: the reference keeps glob's order, which is the directory's (file system dependent) - an unsorted list makes the sample an
        # index names, and with it every seeded run, irreproducible from one machine to the next
        self.image_paths.sort()
        self.id_to_trainid = dict(TRAINID_19)
        self.trainid2name = dict(enumerate(NAMES_19))
        self.id_table = id_table(self.id_to_trainid, ignore_label)

    def _paths(self, index):
        path = self.image_paths[index]
        img_name = os.path.basename(path)
        return path, os.path.join(os.path.dirname(os.path.dirname(path)), "labels", img_name), img_name[:-4]


class cityscapesDataSet(_DecodedSegmentation):
    """core/datasets/cityscapes.py:13-151: leftImg8bit/<mode>/*/*.png with gtFine/<mode>/<city>/<stem>_gtFine_labelIds.png; the 19-class id
    table, the 16-class one for num_classes == 16."""

    def __init__(self, data_root, num_classes=19, mode="train", transform=None, ignore_label=255, debug=False):
        super().__init__()
        self._setup(transform, ignore_label, debug)
        self.mode = mode
        self.NUM_CLASS = num_classes
        self.data_root = data_root
        for city in sorted(glob(os.path.join(data_root, "leftImg8bit/%s" % mode) + "/*/")):
            self.image_paths += glob(city + "/*.png")
        self.image_paths.sort()                                  # (see GTA5FoldDataSet: glob's order is not reproducible)
        sixteen = num_classes == 16
        self.id_to_trainid = dict(TRAINID_16 if sixteen else TRAINID_19)
        self.trainid2name = dict(enumerate(NAMES_16 if sixteen else NAMES_19))
        self.id_table = id_table(self.id_to_trainid, ignore_label)

    def _paths(self, index):
        path = self.image_paths[index]
        img_name = os.path.basename(path)
        city = os.path.basename(os.path.dirname(path))
        label = os.path.join(self.data_root, "gtFine", self.mode, city, img_name.split("_leftImg8bit")[0] + "_gtFine_labelIds.png")
        return path, label, img_name[:-4]


class cityscapesSelfDistillDataSet(cityscapesDataSet):
    """core/datasets/cityscapes.py:153-182: the label is label_dir/<image name> (a pseudo-label PNG holding train ids): ids 0..K-1 are kept,
    everything else becomes ignore_label."""

    def __init__(self, data_root, label_dir, num_classes=19, mode="train", transform=None, ignore_label=255, debug=False):
        super().__init__(data_root, num_classes, mode, transform, ignore_label, debug)
        self.label_dir = label_dir
        self.id_table = id_table({k: k for k in self.trainid2name}, ignore_label)

    def _paths(self, index):
        path = self.image_paths[index]
        img_name = os.path.basename(path)
        return path, os.path.join(self.label_dir, img_name), img_name[:-4]


def _fold_images(data_root, mode, cross_val):
    """<fold>/images/*.png of the folds a mode reads: train = folds whose name does not contain str(cross_val), every other mode = those
    that do; sorted (see GTA5FoldDataSet)."""
    paths = []
    for fold in sorted(glob(data_root + "/*/")):
        inside = str(cross_val) in os.path.basename(fold[:-1])
        if inside != (mode == "train"):
            paths += glob(os.path.join(fold, "images") + "/*.png")
    return sorted(paths)


class KvasirFoldDataset(_DecodedSegmentation):
    """core/datasets/kvasir.py:11-64: Kvasir-SEG in folds, <fold>/images/*.png with <fold>/masks/<same name>, for PraNet.  With a
    host/pra_augment.PraSpec as `transform` it returns the decoded uint8 [H,W,3] image, the uint8 [H,W] grey mask (convert("L")) and the
    name, and the `pra` transform runs on the device; a callable transform receives (PIL RGB image, PIL L mask)."""

    def __init__(self, cfg, data_root, mode="train", cross_val=0, transform=None, debug=False):
        super().__init__()
        self._setup(transform, None, debug)
        self.cfg = cfg
        self.data_root = data_root
        self.mode = mode
        self.image_paths = _fold_images(data_root, mode, cross_val)
        self.id_table = pra_augment.MASK_TABLE                   # grey level -> {0, 1}: what the loader passes to the plans

    def _paths(self, index):
        path = self.image_paths[index]
        img_name = os.path.basename(path)
        return path, os.path.join(os.path.dirname(os.path.dirname(path)), "masks", img_name), img_name[:-4]

    def __getitem__(self, index):
        from PIL import Image
        if self.debug:
            index = 0
        img_path, mask_path, name = self._paths(index)
        image = Image.open(img_path).convert("RGB")
        mask = Image.open(mask_path).convert("L")
        if mask.size != image.size:
            raise ValueError("%s: the mask is %dx%d, its image %dx%d" % (mask_path, mask.size[0], mask.size[1], image.size[0], image.size[1]))
        if self.device_transform:
            return torch.from_numpy(np.array(image, dtype=np.uint8)), torch.from_numpy(np.array(mask, dtype=np.uint8)), name
        if self.transform is not None:
            image, mask = self.transform(image, mask)
        return image, mask, name


class KvasirDataSet(_DecodedSegmentation):
    """core/datasets/kvasir.py:66-117: the same tree as a two-class segmentation set for the `aspp` transform (the reference's two-class
    DeepLab YAML): mask values 0 and 1 are the classes, everything else is ignore_label."""

    def __init__(self, data_root, num_classes=2, mode="train", cross_val=0, transform=None, ignore_label=255, debug=False):
        super().__init__()
        self._setup(transform, ignore_label, debug)
        self.data_root = data_root
        self.mode = mode
        self.image_paths = _fold_images(data_root, mode, cross_val)
        self.id_to_trainid = {0: 0, 1: 1}
        self.id_table = id_table(self.id_to_trainid, ignore_label)

    _paths = KvasirFoldDataset._paths


class DatasetCatalog(object):
    """core/datasets/dataset_path_catalog.py: dataset name -> directory under DATASETS.DATASET_DIR, routed by substring of the name."""
    DATASETS = {
        "gta5_train": {"data_dir": "gta5", "data_list": "gta5_train_list.txt"},
        "gta5_val": {"data_dir": "gta5", "data_list": "gta5_train_list.txt"},
        "synthia_train": {"data_dir": "synthia", "data_list": "synthia_train_list.txt"},
        "cityscapes_train": {"data_dir": "cityscapes", "data_list": "cityscapes_train_list.txt"},
        "cityscapes_self_distill_train": {"data_dir": "cityscapes", "data_list": "cityscapes_train_list.txt",
                                          "label_dir": "cityscapes/soft_labels/inference/cityscapes_train"},
        "cityscapes_val": {"data_dir": "cityscapes", "data_list": "cityscapes_val_list.txt"},
        "kvasir_train": {"data_dir": "kvasir", "data_list": ""},
        "kvasir_val": {"data_dir": "kvasir", "data_list": ""},
        "polyp_train": {"data_dir": "kvasir", "data_list": ""},
        "polyp_val": {"data_dir": "kvasir", "data_list": ""},
        "bli_train": {"data_dir": "BLI/train", "data_list": ""},
        "bli_val": {"data_dir": "BLI/test", "data_list": ""},
    }

    @staticmethod
    def root(cfg, name):
        """The directory a dataset name reads, or None for a name the catalog does not know."""
        attrs = DatasetCatalog.DATASETS.get(name)
        return None if attrs is None else os.path.join(cfg.DATASETS.DATASET_DIR, attrs["data_dir"])

    @staticmethod
    def get(cfg, name, mode, num_classes, transform=None, cross_val=None):
        data_dir = cfg.DATASETS.DATASET_DIR
        if "gta5" in name:
            return GTA5FoldDataSet(cfg, os.path.join(data_dir, DatasetCatalog.DATASETS[name]["data_dir"]), mode=mode, cross_val=cross_val, transform=transform)
        if "cityscapes" in name:
            attrs = DatasetCatalog.DATASETS[name]
            root = os.path.join(data_dir, attrs["data_dir"])
            if "distill" in name:
                return cityscapesSelfDistillDataSet(root, os.path.join(data_dir, attrs["label_dir"]), num_classes=num_classes, mode=mode, transform=transform)
            return cityscapesDataSet(root, num_classes=num_classes, mode=mode, transform=transform)
        if "polyp" in name:
            return KvasirFoldDataset(cfg, os.path.join(data_dir, DatasetCatalog.DATASETS[name]["data_dir"]), mode=mode, cross_val=cross_val, transform=transform)
        if "kvasir" in name:
            return KvasirDataSet(os.path.join(data_dir, DatasetCatalog.DATASETS[name]["data_dir"]), num_classes=num_classes, mode=mode, cross_val=cross_val,
                                 transform=transform)
        if any(k in name for k in ("synthia", "bli")):
            raise RuntimeError("Dataset %r is not read from disk by this project (GTA5, Cityscapes and Kvasir are; the reference's Synthia class "
                               "does not exist and its BLI transform needs albumentations)" % name)
        raise RuntimeError("Dataset not available: {}".format(name))


# ---- the loader -------------------------------------------------------------------------------------------------------------------------------
def list_collate(batch):
    """Keeps the samples as they are: images of a batch may differ in size, and the batch is formed on the device."""
    return list(batch)


MAX_WORKERS = 16          # decode workers per process, in total


class _EpochBatches:
    """Batch sampler of the inner loader: replays the index batches the wrapper drew for the current epoch."""

    def __init__(self):
        self.batches = []

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


class DeviceAugmentLoader:
    """A torch DataLoader whose workers decode, around the device transform.  Iterating yields the (image, label, names) batches of the loader
    contract - float32 [B,3,h,w], float32 [B,lh,lw], list of str - as device tensors, produced by mi_augment_batch (an AugmentSpec) or
    mi_augment_pra_batch (a PraSpec) on a side stream, one
    batch in flight ahead of the consumer.  The worker processes never touch HIP.

    The plan of a sample is seeded by (seed, epoch, dataset index); the epoch is `start_epoch` plus the number of __iter__ calls made so far,
    and the dataset indices are the sampler's, drawn here (the inner loader is fed the same indices through a batch sampler)."""

    def __init__(self, dataset, batch_size=1, shuffle=False, sampler=None, num_workers=4, drop_last=False, device="cuda", seed=0, start_epoch=0,
                 prefetch_factor=2):
        if not has_device_transform(dataset):
            raise ValueError("DeviceAugmentLoader needs a dataset built with a device transform (build_dataset with AUG.NAME 'aspp' or 'pra')")
        self.dataset = dataset
        self.base = base_dataset(dataset)
        self.spec = self.base.transform
        self.batch_size = int(batch_size)
        self.drop_last = bool(drop_last)
        if sampler is None:
            sampler = torch.utils.data.RandomSampler(dataset) if shuffle else torch.utils.data.SequentialSampler(dataset)
        self.sampler = sampler
        self.batch_sampler = torch.utils.data.BatchSampler(sampler, self.batch_size, self.drop_last)
        self.num_workers = max(0, min(int(num_workers), MAX_WORKERS))
        self.device = torch.device(device)
        self.seed = int(seed)
        self.epoch = int(start_epoch)
        self.prefetch_factor = prefetch_factor
        self._augmenter = None
        self._stream = None
        self._inner = None
        self._replay = _EpochBatches()

    def __len__(self):
        return len(self.batch_sampler)

    def set_start_epoch(self, epoch):
        """For a resumed run: the trainer's start epoch, so that epoch e of the resumed run draws the plans epoch e of the first run drew."""
        self.epoch = int(epoch)

    def plans_for(self, indices, sizes, epoch):
        sample = pra_augment.sample_pra_plan if isinstance(self.spec, pra_augment.PraSpec) else augment.sample_plan
        return [sample(self.spec, h, w, self.seed, epoch, i, self.base.id_table) for i, (h, w) in zip(indices, sizes)]

    def _launch(self, indices, samples, epoch):
        images = [s[0].numpy() for s in samples]
        labels = [s[1].numpy() for s in samples]
        plans = self.plans_for(indices, [im.shape[:2] for im in images], epoch)
        img, lab = self._augmenter(images, labels, plans, stream=self._stream)
        ev = torch.cuda.Event()
        ev.record(self._stream)
        return img, lab, [s[2] for s in samples], ev

    def __iter__(self):
        if self.device.type != "cuda":
            raise RuntimeError("the aspp / pra transforms run on the GPU (csrc/augment.hip, csrc/augment_pra.hip); there is no CPU path")
        if self._augmenter is None:
            self._augmenter = augment.DeviceAugmenter(self.device, slots=3)
            self._stream = torch.cuda.Stream(self.device)
        epoch = self.epoch
        self.epoch += 1
        batches = [list(b) for b in self.batch_sampler]          # the sampler is consumed once: the inner loader replays these indices
        self._replay.batches = batches
        if self._inner is None:
            # the workers are started once and kept: forking a process that holds pinned staging buffers and the HIP runtime's mappings
            # costs ~0.15 s per worker (measured: 16 workers, 2 s at the start of every epoch), and they only ever decode
            kw = {"prefetch_factor": self.prefetch_factor, "persistent_workers": True} if self.num_workers > 0 else {}
            self._inner = DataLoader(self.dataset, batch_sampler=self._replay, num_workers=self.num_workers, collate_fn=list_collate, **kw)
        inner = self._inner
        ahead = None
        for indices, samples in zip(batches, inner):
            nxt = self._launch(indices, samples, epoch)
            if ahead is not None:
                yield self._hand_over(ahead)
            ahead = nxt
        if ahead is not None:
            yield self._hand_over(ahead)

    def _hand_over(self, item):
        img, lab, names, ev = item
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        img.record_stream(cur)
        lab.record_stream(cur)
        return img, lab, names


def base_dataset(dataset):
    """The dataset behind a ConcatDataset of repeats (train_adv.py repeats the target set 9 times)."""
    while isinstance(dataset, torch.utils.data.ConcatDataset):
        dataset = dataset.datasets[0]
    return dataset


def has_device_transform(dataset):
    if isinstance(dataset, torch.utils.data.ConcatDataset):
        return all(has_device_transform(d) for d in dataset.datasets) and len({id(base_dataset(d)) for d in dataset.datasets}) == 1
    return bool(getattr(dataset, "device_transform", False))


def wrap_loader(dataset, start_epoch=0, **loader_kwargs):
    """The scripts' loader: a DeviceAugmentLoader for a dataset read from disk, the plain DataLoader (today's behaviour) for the synthetic ones."""
    if has_device_transform(dataset):
        loader_kwargs.pop("pin_memory", None)
        loader_kwargs.pop("collate_fn", None)
        return DeviceAugmentLoader(dataset, start_epoch=start_epoch, **loader_kwargs)
    return DataLoader(dataset, **loader_kwargs)


def run_trainer(trainer, *loaders):
    """trainer.train() with the loaders' plan epoch set from the trainer's start epoch (1 unless a checkpoint was resumed; the FADA combos keep
    theirs as fada.start_adv_epoch), so that a resumed run draws in epoch e the plans an uninterrupted run draws in epoch e."""
    start = getattr(getattr(trainer, "fada", None), "start_adv_epoch", None)
    if start is None:
        start = getattr(trainer, "start_epoch", 1)
    for loader in loaders:
        if hasattr(loader, "set_start_epoch"):
            loader.set_start_epoch(int(start) - 1)
    return trainer.train()
