"""The `pra` input transform (PraNet's polyp transform: the operations, probabilities and ranges of the reference's
core/components/augment.py:55-85, the arithmetic defined on PIL; the contract is in DESIGN.md), split like the `aspp` one of host/augment.py:

 * the PLAN, here: one record per sample with everything random (the draws of PraDraws) and everything derived from it - the composed
   symmetry of the square, the window, the three 256-byte colour tables, the hue shift, PIL's bilinear coefficient tables and nearest
   index tables;
 * the ARITHMETIC, csrc/augment_pra.hip (mi_augment_pra_batch), which executes the plans of a batch on decoded uint8 images and grey masks
   and gives PIL's bits.  The kernels decide nothing.

A plan is sampled from host/augment.plan_rng: it depends on (base seed, epoch, dataset index) only.
"""
import collections
import ctypes
import functools

import numpy as np

from .augment import _NullContext, _round16, plan_rng, resample_tables

# ---- the eight symmetries of the square -----------------------------------------------------------------------------------------------------------
# sym = 4 * transpose + 2 * flip_rows + flip_cols: pixel (y, x) of the transformed frame is source pixel (fr(a), fc(b)) with
# (a, b) = (x, y) when transposed, else (y, x); fr(a) = H-1-a when flip_rows, fc(b) = W-1-b when flip_cols.  As a signed permutation matrix
# M (source = M . transformed, a negative entry meaning "counted from the far end"): row 0 picks x when transposed, its sign is flip_rows,
# the sign of row 1 is flip_cols.
_ROT90 = np.array([[0, 1], [-1, 0]])            # np.rot90(m, 1)[y][x] == m[x][W-1-y]
_FLIP = {0: np.array([[-1, 0], [0, 1]]), 1: np.array([[1, 0], [0, -1]]), -1: np.array([[-1, 0], [0, -1]])}      # cv2 codes: 0 rows, 1 columns, -1 both
_TRANSPOSE = np.array([[0, 1], [1, 0]])
CROP_NOT_DRAWN, CROP_RANDOM, CROP_CENTER, CROP_TOO_SMALL = 0, 1, 2, 3


def compose_symmetry(k=0, d=None, transpose=False):
    """np.rot90(., k), then the flip d (None: no flip), then the transpose, as one element."""
    m = np.linalg.matrix_power(_ROT90, int(k) % 4)
    if d is not None:
        m = m @ _FLIP[int(d)]
    if transpose:
        m = m @ _TRANSPOSE
    t = int(m[0, 1] != 0)
    return 4 * t + 2 * int(m[0].sum() < 0) + int(m[1].sum() < 0)


def apply_symmetry(a, sym):
    """numpy statement of a symmetry code on an [H,W,...] array."""
    if sym & 2:
        a = a[::-1]
    if sym & 1:
        a = a[:, ::-1]
    return np.swapaxes(a, 0, 1) if sym & 4 else a


def shift_table(shift):
    """HueSaturationValue's saturation / value table."""
    return np.clip(np.arange(256, dtype=np.float32) + np.float32(shift), 0, 255).astype(np.uint8)


def brightness_contrast_table(alpha, beta):
    return np.clip(np.arange(256, dtype=np.float32) * np.float32(alpha) + np.float32(beta * 255.0), 0, 255).astype(np.uint8)


def hue_shift_of(shift):
    """A hue shift on cv2's 0..179 scale as an addend modulo 256 on PIL's 0..255 hue."""
    return int(round(shift * 256 / 180)) % 256


@functools.lru_cache(maxsize=64)
def nearest_table(in_size, out_size):
    """int32 [out_size]: the source index of every output of PIL's NEAREST resize (Geometry.c ImagingScaleAffine: the coordinate starts
    at half a step and is advanced by repeated addition in float64, then truncated)."""
    step = float(in_size) / float(out_size)
    idx = np.empty(int(out_size), np.int32)
    pos = 0.0 + step * 0.5
    for o in range(int(out_size)):
        idx[o] = min(int(pos), int(in_size) - 1)
        pos += step
    idx.setflags(write=False)
    return idx


MASK_TABLE = (np.arange(256) >= 128).astype(np.uint8)            # grey level -> {0, 1}


# ---- what a configuration asks for ------------------------------------------------------------------------------------------------------------
class PraSpec:
    """pra_trans of one (cfg, mode): output size, crop size, whether anything is random."""

    def __init__(self, out_size, train, crop=220, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.out_h, self.out_w = int(out_size[0]), int(out_size[1])
        self.train = bool(train)
        self.crop = int(crop)
        self.mean = tuple(float(v) for v in mean)
        self.std = tuple(float(v) for v in std)
        if self.crop < 1 or self.out_h < 1 or self.out_w < 1:
            raise ValueError("pra transform: crop and output size must be positive")

    @classmethod
    def from_cfg(cls, cfg, mode="train"):
        I = cfg.INPUT
        if mode == "train":
            return cls((I.TRAINSIZE, I.TRAINSIZE), True, mean=I.PIXEL_MEAN, std=I.PIXEL_STD)
        w, h = I.INPUT_SIZE_TEST
        return cls((h, w), False, mean=I.PIXEL_MEAN, std=I.PIXEL_STD)


# every gate has p = 0.5; every value is drawn whether or not its gate fires, so the stream a sample consumes does not depend on its gates
PraDraws = collections.namedtuple("PraDraws", "rot k flip d hsv hue sat val bc alpha beta transpose crop center u1 u2")
GATES = ("rot", "flip", "hsv", "bc", "transpose", "crop")


def draw_pra(seed=0, epoch=0, index=0):
    """The random decisions of the train transform in the contract's order."""
    rng = plan_rng(seed, epoch, index)
    gate = lambda: bool(rng.random() < 0.5)
    rot, k = gate(), int(rng.integers(0, 4))
    flip, d = gate(), int(rng.integers(-1, 2))
    hsv, hue, sat, val = gate(), float(rng.uniform(-20, 20)), float(rng.uniform(-30, 30)), float(rng.uniform(-20, 20))
    bc, alpha, beta = gate(), 1.0 + float(rng.uniform(-0.2, 0.2)), float(rng.uniform(-0.2, 0.2))
    transpose = gate()
    crop, center, u1, u2 = gate(), gate(), float(rng.random()), float(rng.random())
    return PraDraws(rot, k, flip, d, hsv, hue, sat, val, bc, alpha, beta, transpose, crop, center, u1, u2)


class PraPlan:
    """Everything mi_augment_pra_batch needs to know about one sample, and nothing random left to decide."""

    FIELDS = ("H", "W", "sym", "crop", "y0", "x0", "wh", "ww", "out_h", "out_w", "hsv", "hue_shift", "bc")
    COLOUR = ("sat_shift", "val_shift", "alpha", "beta")

    def __init__(self, H, W, sym, crop, y0, x0, wh, ww, out_h, out_w, hsv=0, hue_shift=0, bc=0, sat_shift=0.0, val_shift=0.0, alpha=1.0, beta=0.0,
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), mask_table=None):
        self.H, self.W, self.sym, self.crop = int(H), int(W), int(sym), int(crop)
        self.y0, self.x0, self.wh, self.ww = int(y0), int(x0), int(wh), int(ww)
        self.out_h, self.out_w = int(out_h), int(out_w)
        self.hsv, self.hue_shift, self.bc = int(bool(hsv)), int(hue_shift), int(bool(bc))
        self.sat_shift, self.val_shift, self.alpha, self.beta = float(sat_shift), float(val_shift), float(alpha), float(beta)
        self.mean = np.asarray(mean, np.float64)
        self.std = np.asarray(std, np.float64)
        self.mask_table = np.asarray(MASK_TABLE if mask_table is None else mask_table, np.uint8)
        self.to_bgr255 = 0                                       # (what tests/_augment_ref.to_tensor_normalize reads)
        th, tw = self.frame
        assert 0 <= self.sym <= 7 and 0 <= self.hue_shift <= 255 and self.crop in (CROP_NOT_DRAWN, CROP_RANDOM, CROP_CENTER, CROP_TOO_SMALL)
        assert self.wh > 0 and self.ww > 0 and 0 <= self.y0 <= th - self.wh and 0 <= self.x0 <= tw - self.ww, "window outside the transformed frame"
        assert self.mask_table.shape == (256,) and self.mean.shape == (3,) and self.std.shape == (3,)

    @property
    def frame(self):
        """(H', W'): the size after the symmetry."""
        return (self.W, self.H) if self.sym & 4 else (self.H, self.W)

    # the three 256-byte tables the kernel looks colours up in
    @property
    def lut_s(self):
        return shift_table(self.sat_shift)

    @property
    def lut_v(self):
        return shift_table(self.val_shift)

    @property
    def lut_bc(self):
        return brightness_contrast_table(self.alpha, self.beta)

    def to_arrays(self):
        return {"geom": np.array([getattr(self, k) for k in self.FIELDS], np.int64), "colour": np.array([getattr(self, k) for k in self.COLOUR], np.float64),
                "mean": self.mean, "std": self.std, "mask_table": self.mask_table}

    @classmethod
    def from_arrays(cls, a):
        kw = dict(zip(cls.FIELDS, [int(v) for v in a["geom"]]))
        kw.update(zip(cls.COLOUR, [float(v) for v in a["colour"]]))
        return cls(mean=a["mean"], std=a["std"], mask_table=a["mask_table"], **kw)


def plan_from_draws(spec, H, W, draws, mask_table=None):
    """The plan the draws give for an image of size H x W: the three geometric draws composed, the crop resolved against the frame."""
    sym = compose_symmetry(draws.k if draws.rot else 0, draws.d if draws.flip else None, draws.transpose)
    th, tw = (W, H) if sym & 4 else (H, W)
    c = spec.crop
    crop, y0, x0, wh, ww = CROP_NOT_DRAWN, 0, 0, th, tw
    if draws.crop:
        if min(th, tw) < c:
            crop = CROP_TOO_SMALL                                # albumentations would raise; the frame is resized whole
        elif draws.center:
            crop, y0, x0, wh, ww = CROP_CENTER, (th - c) // 2, (tw - c) // 2, c, c
        else:
            crop, y0, x0, wh, ww = CROP_RANDOM, int((th - c) * draws.u1), int((tw - c) * draws.u2), c, c
    return PraPlan(H, W, sym, crop, y0, x0, wh, ww, spec.out_h, spec.out_w, draws.hsv, hue_shift_of(draws.hue) if draws.hsv else 0, draws.bc,
                   draws.sat if draws.hsv else 0.0, draws.val if draws.hsv else 0.0, draws.alpha if draws.bc else 1.0, draws.beta if draws.bc else 0.0,
                   spec.mean, spec.std, mask_table)


def sample_pra_plan(spec, H, W, seed=0, epoch=0, index=0, mask_table=None):
    if not spec.train:                                           # Resize + Normalize (the reference's Transpose there is a bug and is dropped)
        return PraPlan(H, W, 0, CROP_NOT_DRAWN, 0, 0, H, W, spec.out_h, spec.out_w, mean=spec.mean, std=spec.std, mask_table=mask_table)
    return plan_from_draws(spec, H, W, draw_pra(seed, epoch, index), mask_table)


# ---- executing plans on the device ------------------------------------------------------------------------------------------------------------
def run_batch(augmenter, images, masks, plans, stream=None):
    """DeviceAugmenter.__call__ for PraPlans: the batch (descriptor table, coefficient and index tables, decoded images, masks) staged in one
    pinned buffer of the augmenter's slot, one copy, mi_augment_pra_batch.  Returns (float32 [B,3,h,w], float32 [B,h,w] or None)."""
    from .. import _lib, kernels
    torch = augmenter.torch
    B = len(plans)
    p0 = plans[0]
    if any((p.out_h, p.out_w) != (p0.out_h, p0.out_w) for p in plans):
        raise ValueError("the samples of a batch must agree in output size")
    images = [np.asarray(im) for im in images]
    masks = [None if m is None else np.asarray(m) for m in masks]
    have_mask = all(m is not None for m in masks)
    tsize = ctypes.sizeof(_lib.MiPraSample)
    off = _round16(B * tsize)
    layout, tables = [], {}

    def table(key, arrays):
        nonlocal off
        if key not in tables:
            offs = []
            for a in arrays:
                offs.append(off)
                off += _round16(a.nbytes)
            tables[key] = (offs, arrays)
        return tables[key][0]

    for im, m, p in zip(images, masks, plans):
        if im.dtype != np.uint8 or im.shape != (p.H, p.W, 3) or (m is not None and (m.dtype != np.uint8 or m.shape != (p.H, p.W))):
            raise ValueError("augment: image uint8 [%d,%d,3] and mask uint8 [%d,%d] expected, got %s / %s" % (p.H, p.W, p.H, p.W, im.shape, None if m is None else m.shape))
        e = {}
        for axis, (a, b) in (("h", (p.ww, p.out_w)), ("v", (p.wh, p.out_h))):
            e[axis] = None
            if a != b:
                coef, bound, k = resample_tables(a, b, "bilinear")
                e[axis] = table(("coef", a, b), (coef, bound)) + [k]
        if have_mask:
            e["ny"], e["nx"] = table(("near", p.wh, p.out_h), (nearest_table(p.wh, p.out_h),))[0], table(("near", p.ww, p.out_w), (nearest_table(p.ww, p.out_w),))[0]
        e["img"] = off
        off += _round16(im.nbytes)
        if have_mask:
            e["mask"] = off
            off += _round16(m.nbytes)
        layout.append(e)
    staged = off
    for e, p in zip(layout, plans):                              # device-only scratch behind the staged part
        e["wstride"], e["tstride"] = 12 * ((p.ww + 3) // 4), 12 * ((p.out_w + 3) // 4)
        e["win"] = off
        off += _round16(p.wh * e["wstride"])
        if e["h"] is not None:
            e["tmp"] = off
            off += _round16(p.wh * e["tstride"])
    slot = augmenter.slots[augmenter.turn]
    augmenter.turn = (augmenter.turn + 1) % len(augmenter.slots)
    pinned, dev = augmenter._buffers(slot, staged, off)
    host = pinned.numpy()
    base = dev.data_ptr()
    records = (_lib.MiPraSample * B).from_buffer(host)           # the descriptors are written in place in the pinned buffer
    for i, (e, im, m, p) in enumerate(zip(layout, images, masks, plans)):
        d = records[i]
        ctypes.memset(ctypes.byref(d), 0, tsize)
        d.img = base + e["img"]
        host[e["img"]:e["img"] + im.nbytes] = im.reshape(-1)
        if "mask" in e:
            d.mask, d.ny, d.nx = base + e["mask"], base + e["ny"], base + e["nx"]
            host[e["mask"]:e["mask"] + m.nbytes] = m.reshape(-1)
        d.win = base + e["win"]
        d.tmp = base + e["tmp"] if "tmp" in e else None
        if e["h"] is not None:
            d.hcoef, d.hbound, d.hk = base + e["h"][0], base + e["h"][1], e["h"][2]
        if e["v"] is not None:
            d.vcoef, d.vbound, d.vk = base + e["v"][0], base + e["v"][1], e["v"][2]
        d.H, d.W, d.sym, d.y0, d.x0, d.wh, d.ww = p.H, p.W, p.sym, p.y0, p.x0, p.wh, p.ww
        d.wstride, d.tstride = e["wstride"], e["tstride"]
        d.hsv, d.hue_shift, d.bc = p.hsv, p.hue_shift, p.bc
        for k in range(3):
            d.mean[k], d.std[k] = p.mean[k], p.std[k]            # rounded to fp32 as torch.tensor(mean) does
        for name in ("lut_s", "lut_v", "lut_bc", "mask_table"):
            ctypes.memmove(getattr(d, name), np.ascontiguousarray(getattr(p, name)).ctypes.data, 256)
    for offs, arrays in tables.values():
        for o, a in zip(offs, arrays):
            host[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
    del records
    ctx = torch.cuda.stream(stream) if stream is not None else _NullContext()
    with torch.cuda.device(augmenter.device), ctx:
        dev[:staged].copy_(pinned[:staged], non_blocking=True)
        out_img = torch.empty((B, 3, p0.out_h, p0.out_w), dtype=torch.float32, device=augmenter.device)
        out_mask = torch.empty((B, p0.out_h, p0.out_w), dtype=torch.float32, device=augmenter.device) if have_mask else None
        kernels.augment_pra_batch(dev, pinned, B, out_img, out_mask)
        slot["event"] = torch.cuda.Event()
        slot["event"].record()
    return out_img, out_mask
