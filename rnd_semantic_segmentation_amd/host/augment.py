"""The `aspp` input transform (reference core/components/augment.py:87-120, core/datasets/transform.py) split in two:

 * the PLAN, here, pure Python / numpy: one record per sample with everything random (ColorJitter order and factors, RandomScale,
   RandomCrop offset, flip) and everything derived from it (scaled size, padding, the windows of the image that the output shows, the
   fixed-point coefficient tables of PIL's two bicubic passes, computed in float64);
 * the ARITHMETIC, csrc/augment.hip (mi_augment_batch), which executes the plans of a batch on decoded uint8 images and gives PIL's bits.

A plan is sampled from a generator seeded by (base seed, epoch, sample index): it does not depend on worker count, rank or batch
composition.  torchvision's own random stream is not reproduced (it differs between torchvision versions); the supports of the
distributions are the reference's.
"""
import ctypes
import functools
import math

import numpy as np

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 1, 2, 3, 4
OP_NAMES = {OP_BRIGHTNESS: "brightness", OP_CONTRAST: "contrast", OP_SATURATION: "saturation", OP_HUE: "hue"}
PRECISION_BITS = 22          # PIL Resample.c: coefficients as fixed point with 22 fraction bits


# ---- PIL's resampling coefficients (Resample.c precompute_coeffs + normalize_coeffs_8bpc) ------------------------------------------
def _bicubic_kernel(x, a=-0.5):
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _triangle_kernel(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


FILTERS = {"bicubic": (_bicubic_kernel, 2.0), "bilinear": (_triangle_kernel, 1.0)}      # PIL Resample.c: (filter, support)


def bicubic_tables(in_size, out_size):
    """resample_tables with the bicubic filter (the `aspp` transform's)."""
    return resample_tables(in_size, out_size, "bicubic")


@functools.lru_cache(maxsize=64)
def resample_tables(in_size, out_size, filter="bicubic"):
    """(coef int32 [k][out_size] tap-major, bound int32 [out_size][2] = {first source index, taps}, k) of one pass in_size -> out_size with
    PIL's BICUBIC or BILINEAR filter.  float64 throughout; the weights of an output are summed in tap order and divided by that sum, as PIL
    does."""
    kernel, filter_support = FILTERS[filter]
    in_size, out_size = int(in_size), int(out_size)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = filter_support * fs
    k = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    x0 = np.maximum((center - support + 0.5).astype(np.int64), 0)            # astype truncates toward zero like C's (int)
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - x0
    j = np.arange(k, dtype=np.float64)[:, None]
    w = kernel((j + x0[None, :] - center[None, :] + 0.5) * (1.0 / fs))
    w = np.where(np.arange(k)[:, None] < n[None, :], w, 0.0)
    total = np.zeros(out_size, np.float64)
    for t in range(k):                                                       # in tap order: the sum's rounding is part of the result
        total = total + w[t]
    w = np.where(total[None, :] != 0.0, w / np.where(total == 0.0, 1.0, total)[None, :], w)
    fixed = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)   # truncation toward zero
    coef = np.ascontiguousarray(fixed.astype(np.int32))
    bound = np.ascontiguousarray(np.stack([x0, n], 1).astype(np.int32))
    coef.setflags(write=False)
    bound.setflags(write=False)
    return coef, bound, k


# ---- what a configuration asks for ------------------------------------------------------------------------------------------------------------
class AugmentSpec:
    """aspp_trans of one (cfg, mode, is_source): output size and which random decisions exist."""

    def __init__(self, out_size, train, jitter=(0.0, 0.0, 0.0, 0.0), scales=(1.0, 1.0), flip_prob=0.0, to_bgr255=False,
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.out_h, self.out_w = int(out_size[0]), int(out_size[1])
        self.train = bool(train)
        self.brightness, self.contrast, self.saturation, self.hue = [float(v) for v in jitter]
        self.scales = (float(scales[0]), float(scales[1]))
        self.flip_prob = float(flip_prob)
        self.to_bgr255 = bool(to_bgr255)
        self.mean = tuple(float(v) for v in mean)
        self.std = tuple(float(v) for v in std)
        if not 0.0 <= self.hue <= 0.5 or min(self.brightness, self.contrast, self.saturation) < 0:
            raise ValueError("ColorJitter: brightness / contrast / saturation must be >= 0 and hue in [0, 0.5]")

    @classmethod
    def from_cfg(cls, cfg, mode="train", is_source=True):
        I = cfg.INPUT
        if mode == "train":
            w, h = I.SOURCE_INPUT_SIZE_TRAIN if is_source else I.TARGET_INPUT_SIZE_TRAIN
            jitter = (I.BRIGHTNESS, I.CONTRAST, I.SATURATION, I.HUE) if is_source else (0.0, 0.0, 0.0, 0.0)      # ColorJitter: source only
            return cls((h, w), True, jitter, I.INPUT_SCALES_TRAIN, I.HORIZONTAL_FLIP_PROB_TRAIN, I.TO_BGR255, I.PIXEL_MEAN, I.PIXEL_STD)
        w, h = I.INPUT_SIZE_TEST
        return cls((h, w), False, to_bgr255=I.TO_BGR255, mean=I.PIXEL_MEAN, std=I.PIXEL_STD)

    @property
    def fixed_resize(self):
        return not self.train or (self.scales[0] == self.scales[1] and self.scales[0] == 1)


IDENTITY_TABLE = np.arange(256, dtype=np.uint8)


class Plan:
    """Everything mi_augment_batch needs to know about one sample, and nothing random left to decide."""

    FIELDS = ("H", "W", "sh", "sw", "pad_y", "pad_x", "crop_y", "crop_x", "flip", "out_h", "out_w", "lab_sh", "lab_sw", "lab_h", "lab_w", "to_bgr255")

    def __init__(self, H, W, ops, sh, sw, pad_y, pad_x, crop_y, crop_x, flip, out_h, out_w, to_bgr255, mean, std, label_table=None,
                 lab_sh=None, lab_sw=None, lab_h=None, lab_w=None):
        self.H, self.W = int(H), int(W)
        self.ops = [(int(c), float(f)) for c, f in ops]                       # in execution order
        self.sh, self.sw = int(sh), int(sw)
        self.pad_y, self.pad_x = int(pad_y), int(pad_x)                       # added on BOTH sides of the axis
        self.crop_y, self.crop_x = int(crop_y), int(crop_x)                   # offset into the padded image
        self.flip = int(bool(flip))
        self.out_h, self.out_w = int(out_h), int(out_w)
        self.to_bgr255 = int(bool(to_bgr255))
        self.mean = np.asarray(mean, np.float64)
        self.std = np.asarray(std, np.float64)
        self.label_table = np.asarray(IDENTITY_TABLE if label_table is None else label_table, np.uint8)
        # the label follows the image's geometry in train mode; in test mode it keeps its own size (Resize(resize_label=False))
        self.lab_sh, self.lab_sw = int(self.sh if lab_sh is None else lab_sh), int(self.sw if lab_sw is None else lab_sw)
        self.lab_h, self.lab_w = int(self.out_h if lab_h is None else lab_h), int(self.out_w if lab_w is None else lab_w)
        assert len(self.ops) <= 4 and len({c for c, _ in self.ops}) == len(self.ops) and all(c in OP_NAMES for c, _ in self.ops)
        assert self.label_table.shape == (256,) and self.mean.shape == (3,) and self.std.shape == (3,)
        assert 0 <= self.crop_y <= self.sh + 2 * self.pad_y - self.out_h and 0 <= self.crop_x <= self.sw + 2 * self.pad_x - self.out_w, "crop outside the padded image"

    # derived ---------------------------------------------------------------------------------------------------------------------------------
    @property
    def off_y(self):
        return self.crop_y - self.pad_y

    @property
    def off_x(self):
        return self.crop_x - self.pad_x

    @property
    def hue_shift(self):
        """torchvision adjust_hue: uint8(hue_factor * 255) added to H modulo 256; the conversion truncates toward zero."""
        for c, f in self.ops:
            if c == OP_HUE:
                return int(f * 255) % 256
        return 0

    def windows(self):
        """(cy0, cy1, cx0, cx1, ry0, ry1, rx0, rx1): the part of the resampled image the output shows, and the source rows / columns it needs."""
        cy0, cy1 = max(self.off_y, 0), min(self.off_y + self.out_h, self.sh)
        cx0, cx1 = max(self.off_x, 0), min(self.off_x + self.out_w, self.sw)
        if cy0 >= cy1 or cx0 >= cx1:
            return (0,) * 8
        ry0, ry1, rx0, rx1 = cy0, cy1, cx0, cx1
        if self.sh != self.H:
            b = bicubic_tables(self.H, self.sh)[1]
            ry0, ry1 = int(b[cy0, 0]), int(b[cy1 - 1, 0] + b[cy1 - 1, 1])
        if self.sw != self.W:
            b = bicubic_tables(self.W, self.sw)[1]
            rx0, rx1 = int(b[cx0, 0]), int(b[cx1 - 1, 0] + b[cx1 - 1, 1])
        return cy0, cy1, cx0, cx1, ry0, ry1, rx0, rx1

    # fixtures --------------------------------------------------------------------------------------------------------------------------------
    def to_arrays(self):
        ops = np.zeros((4, 2), np.float64)
        for i, (c, f) in enumerate(self.ops):
            ops[i] = (c, f)
        return {"geom": np.array([getattr(self, k) for k in self.FIELDS], np.int64), "ops": ops, "n_ops": np.array(len(self.ops)),
                "mean": self.mean, "std": self.std, "label_table": self.label_table}

    @classmethod
    def from_arrays(cls, a):
        g = dict(zip(cls.FIELDS, [int(v) for v in a["geom"]]))
        ops = [(int(c), float(f)) for c, f in a["ops"][:int(a["n_ops"])]]
        return cls(g["H"], g["W"], ops, g["sh"], g["sw"], g["pad_y"], g["pad_x"], g["crop_y"], g["crop_x"], g["flip"], g["out_h"], g["out_w"],
                   g["to_bgr255"], a["mean"], a["std"], a["label_table"], g["lab_sh"], g["lab_sw"], g["lab_h"], g["lab_w"])


def plan_rng(seed, epoch, index):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed) & 0xFFFFFFFF, int(epoch), int(index)])))


def sample_plan(spec, H, W, seed=0, epoch=0, index=0, label_table=None):
    """The random decisions of aspp_trans for one image of size H x W, in the reference's order: ColorJitter (torchvision: a random order of
    the four ops, a parameter of 0 disables its op, brightness / contrast / saturation uniform in [max(0, 1 - p), 1 + p], hue in [-p, p]),
    Resize | RandomScale + RandomCrop(pad_if_needed), RandomHorizontalFlip."""
    rng = plan_rng(seed, epoch, index)
    h, w = spec.out_h, spec.out_w
    if not spec.train:                        # Resize((h, w), resize_label=False)
        return Plan(H, W, [], h, w, 0, 0, 0, 0, 0, h, w, spec.to_bgr255, spec.mean, spec.std, label_table, lab_sh=H, lab_sw=W, lab_h=H, lab_w=W)
    ops = []
    order = rng.permutation(4)
    amount = {OP_BRIGHTNESS: spec.brightness, OP_CONTRAST: spec.contrast, OP_SATURATION: spec.saturation, OP_HUE: spec.hue}
    factor = {}
    for code in (OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE):
        p = amount[code]
        if p > 0:
            lo, hi = (-p, p) if code == OP_HUE else (max(0.0, 1.0 - p), 1.0 + p)
            factor[code] = float(rng.uniform(lo, hi))
    for i in order:
        code = (OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE)[int(i)]
        if code in factor:
            ops.append((code, factor[code]))
    if spec.fixed_resize:
        sh, sw, pad_y, pad_x, crop_y, crop_x = h, w, 0, 0, 0, 0
    else:
        s = spec.scales[0] + (spec.scales[1] - spec.scales[0]) * float(rng.random())
        sh, sw = int(H * s), int(W * s)
        if sh < 1 or sw < 1:
            raise ValueError("INPUT_SCALES_TRAIN %r leaves nothing of a %dx%d image" % (spec.scales, H, W))
        # torchvision pads a two-number padding on both sides of the axis: a too narrow image grows by 2 * (w - width)
        pad_x = w - sw if sw < w else 0
        pad_y = h - sh if sh < h else 0
        ph, pw = sh + 2 * pad_y, sw + 2 * pad_x
        if (ph, pw) == (h, w):
            crop_y, crop_x = 0, 0
        else:
            crop_y, crop_x = int(rng.integers(0, ph - h + 1)), int(rng.integers(0, pw - w + 1))
    flip = spec.flip_prob > 0 and float(rng.random()) < spec.flip_prob
    return Plan(H, W, ops, sh, sw, pad_y, pad_x, crop_y, crop_x, flip, h, w, spec.to_bgr255, spec.mean, spec.std, label_table)


# ---- executing plans on the device ------------------------------------------------------------------------------------------------------------
def _round16(n):
    return (int(n) + 15) & ~15


class DeviceAugmenter:
    """Stages a batch (descriptor table, coefficient tables, decoded images, label ids) in one pinned buffer, copies it to the device in
    one transfer and runs mi_augment_batch.  `slots` staging buffers are cycled so that a batch can be prepared while the previous one is
    still being consumed."""

    def __init__(self, device, slots=2):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.slots = [{"pinned": None, "dev": None, "event": None} for _ in range(slots)]
        self.turn = 0

    def _buffers(self, slot, staged, total):
        torch = self.torch
        if slot["event"] is not None:
            slot["event"].synchronize()                      # the previous batch of this slot has been copied and transformed
        if slot["pinned"] is None or slot["pinned"].numel() < staged:
            slot["pinned"] = torch.empty(_round16(staged * 5 // 4), dtype=torch.uint8, pin_memory=True)
        if slot["dev"] is None or slot["dev"].numel() < total:
            slot["dev"] = torch.empty(_round16(total * 5 // 4), dtype=torch.uint8, device=self.device)
        return slot["pinned"], slot["dev"]

    def __call__(self, images, labels, plans, stream=None):
        """images: uint8 [H,W,3] arrays / CPU tensors, labels: uint8 [H,W] or None per sample, plans: Plan per sample.  Returns
        (float32 [B,3,h,w], float32 [B,lh,lw] or None) on the device; with `stream`, the work is enqueued there and the caller orders its
        own stream behind the returned tensors (see DeviceAugmentLoader).  A batch of host/pra_augment.PraPlan runs the `pra` transform
        (mi_augment_pra_batch) through the same slots."""
        from .. import _lib, kernels
        from . import pra_augment
        if isinstance(plans[0], pra_augment.PraPlan):
            return pra_augment.run_batch(self, images, labels, plans, stream)
        torch = self.torch
        B = len(plans)
        p0 = plans[0]
        if any((p.out_h, p.out_w, p.lab_h, p.lab_w) != (p0.out_h, p0.out_w, p0.lab_h, p0.lab_w) for p in plans):
            raise ValueError("the samples of a batch must agree in output size (test mode keeps each label at its own size: use TEST.BATCH_SIZE 1 for images of different sizes)")
        images = [np.asarray(im) for im in images]
        labels = [None if lb is None else np.asarray(lb) for lb in labels]
        have_label = all(lb is not None for lb in labels)
        tsize = ctypes.sizeof(_lib.MiAugSample)
        off = _round16(B * tsize)
        layout, tables = [], {}
        for im, lb, p in zip(images, labels, plans):
            if im.dtype != np.uint8 or im.shape != (p.H, p.W, 3) or (lb is not None and (lb.dtype != np.uint8 or lb.shape != (p.H, p.W))):
                raise ValueError("augment: image uint8 [%d,%d,3] and label uint8 [%d,%d] expected, got %s / %s" % (p.H, p.W, p.H, p.W, im.shape, None if lb is None else lb.shape))
            e = {}
            for axis, (a, b) in (("h", (p.W, p.sw)), ("v", (p.H, p.sh))):
                if a != b and (a, b) not in tables:
                    coef, bound, k = bicubic_tables(a, b)
                    tables[(a, b)] = (off, off + _round16(coef.nbytes), k, coef, bound)
                    off += _round16(coef.nbytes) + _round16(bound.nbytes)
                e[axis] = tables.get((a, b)) if a != b else None
            e["img"] = off
            off += _round16(im.nbytes)
            if lb is not None and have_label:
                e["lab"] = off
                off += _round16(lb.nbytes)
            layout.append(e)
        staged = off
        for e, p in zip(layout, plans):                     # device-only scratch behind the staged part
            cy0, cy1, cx0, cx1, ry0, ry1, rx0, rx1 = p.windows()
            e["win"] = (cy0, cy1, cx0, cx1, ry0, ry1, rx0, rx1)
            e["tstride"] = 12 * ((cx1 - cx0 + 3) // 4)
            if p.ops:
                e["jit"] = off
                off += _round16(p.H * p.W * 3)
            if p.sw != p.W and cx1 > cx0:
                e["tmp"] = off
                off += _round16((ry1 - ry0) * e["tstride"])
        slot = self.slots[self.turn]
        self.turn = (self.turn + 1) % len(self.slots)
        pinned, dev = self._buffers(slot, staged, off)
        host = pinned.numpy()
        base = dev.data_ptr()
        table = (_lib.MiAugSample * B).from_buffer(host)     # the descriptors are written in place in the pinned buffer
        for i, (e, im, lb, p) in enumerate(zip(layout, images, labels, plans)):
            d = table[i]
            ctypes.memset(ctypes.byref(d), 0, tsize)
            d.img = base + e["img"]
            host[e["img"]:e["img"] + im.nbytes] = im.reshape(-1)
            if "lab" in e:
                d.lab = base + e["lab"]
                host[e["lab"]:e["lab"] + lb.nbytes] = lb.reshape(-1)
            d.jit = base + e["jit"] if "jit" in e else None
            d.tmp = base + e["tmp"] if "tmp" in e else None
            if e["h"] is not None:
                d.hcoef, d.hbound, d.hk = base + e["h"][0], base + e["h"][1], e["h"][2]
            if e["v"] is not None:
                d.vcoef, d.vbound, d.vk = base + e["v"][0], base + e["v"][1], e["v"][2]
            d.H, d.W, d.sh, d.sw = p.H, p.W, p.sh, p.sw
            d.off_y, d.off_x, d.flip = p.off_y, p.off_x, p.flip
            d.cy0, d.cy1, d.cx0, d.cx1, d.ry0, d.ry1, d.rx0, d.rx1 = e["win"]
            d.tstride = e["tstride"]
            d.lab_sh, d.lab_sw = p.lab_sh, p.lab_sw
            d.n_ops, d.hue_shift = len(p.ops), p.hue_shift
            for k, (c, f) in enumerate(p.ops):
                d.op[k], d.factor[k] = c, f                  # the factor is rounded to fp32 here, as PIL's C takes it
            d.to_bgr255 = p.to_bgr255
            for k in range(3):
                d.mean[k], d.std[k] = p.mean[k], p.std[k]    # rounded to fp32 as torch.tensor(mean) does
            ctypes.memmove(d.lab_table, p.label_table.ctypes.data, 256)
        for c_off, b_off, _, coef, bound in tables.values():
            host[c_off:c_off + coef.nbytes] = coef.view(np.uint8).reshape(-1)
            host[b_off:b_off + bound.nbytes] = bound.view(np.uint8).reshape(-1)
        del table
        ctx = torch.cuda.stream(stream) if stream is not None else _NullContext()
        with torch.cuda.device(self.device), ctx:
            dev[:staged].copy_(pinned[:staged], non_blocking=True)
            out_img = torch.empty((B, 3, p0.out_h, p0.out_w), dtype=torch.float32, device=self.device)
            out_lab = torch.empty((B, p0.lab_h, p0.lab_w), dtype=torch.float32, device=self.device) if have_label else None
            kernels.augment_batch(dev, pinned, B, out_img, out_lab)
            slot["event"] = torch.cuda.Event()
            slot["event"].record()
        return out_img, out_lab


class _NullContext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
