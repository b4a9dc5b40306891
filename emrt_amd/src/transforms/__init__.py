"""Image / label transforms of the EMRT data pipeline, cv2-free (reference: src/transforms/transforms.py:24-88 Compose,
:91-110 RandomHorizontalFlip, :113-132 RandomVerticalFlip, :136-206 Resize, :209-270 ResizeStepScaling, :273-318 Normalize, :391-478
RandomPaddingCrop, :588-681 RandomDistort; src/transforms/__init__.py:4-57 get_transforms).

Arrays are HWC float32 RGB (the reference reads BGR with cv2 and converts to RGB; here PIL reads RGB directly), labels
HW uint8.  Bilinear / nearest resizing are restated in numpy with cv2's conventions (INTER_LINEAR: half-pixel centres,
no antialiasing; INTER_NEAREST: floor(dst * scale)).  Random draws use the same `np.random` / `random` calls as the
reference, so a seeded run makes the same decisions.
"""
import random
from collections import namedtuple

import numpy as np
from PIL import Image, ImageEnhance


def read_image(path):
    """-> HWC float32 RGB, 0..255 (cv2.imread + BGR2RGB in the reference, transforms.py:55,71)."""
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float32)


def read_label(path):
    """-> HW uint8 class indices; palette PNGs give their indices (transforms.py:62)."""
    return np.asarray(Image.open(path).convert("P"), dtype=np.uint8)


def resize_bilinear(img, w, h):
    """cv2.resize(img, (w, h), INTER_LINEAR) for HWC float arrays."""
    H, W = img.shape[:2]
    if (H, W) == (h, w):
        return img
    ys = np.clip((np.arange(h, dtype=np.float64) + 0.5) * (H / h) - 0.5, 0, None)
    xs = np.clip((np.arange(w, dtype=np.float64) + 0.5) * (W / w) - 0.5, 0, None)
    y0 = np.minimum(ys.astype(np.int64), H - 1)
    x0 = np.minimum(xs.astype(np.int64), W - 1)
    y1 = np.minimum(y0 + 1, H - 1)
    x1 = np.minimum(x0 + 1, W - 1)
    wy = (ys - y0).astype(np.float32)[:, None, None]
    wx = (xs - x0).astype(np.float32)[None, :, None]
    a = img.reshape(H, W, -1)
    top = a[y0][:, x0] * (1 - wx) + a[y0][:, x1] * wx
    bot = a[y1][:, x0] * (1 - wx) + a[y1][:, x1] * wx
    out = top * (1 - wy) + bot * wy
    return out.reshape((h, w) + img.shape[2:]).astype(img.dtype)


def resize_nearest(lab, w, h):
    """cv2.resize(label, (w, h), INTER_NEAREST)."""
    H, W = lab.shape[:2]
    if (H, W) == (h, w):
        return lab
    ys = np.minimum((np.arange(h) * (H / h)).astype(np.int64), H - 1)
    xs = np.minimum((np.arange(w) * (W / w)).astype(np.int64), W - 1)
    return lab[ys][:, xs]


class Compose:
    def __init__(self, transforms, to_rgb=True):
        if not isinstance(transforms, list):
            raise TypeError("The transforms must be a list!")
        self.transforms = transforms
        self.to_rgb = to_rgb

    def __call__(self, img, label=None):
        if isinstance(img, str):
            img = read_image(img)
        if isinstance(label, str):
            label = read_label(label)
        if img is None:
            raise ValueError("Can't read The image file {}!".format(img))
        for op in self.transforms:
            outputs = op(img, label)
            img = outputs[0]
            if len(outputs) == 2:
                label = outputs[1]
        return np.ascontiguousarray(np.transpose(img, (2, 0, 1))), label


class RandomHorizontalFlip:
    def __init__(self, prob=0.5):
        self.prob = prob

    def draw(self):
        """The flip decision: one Python `random.random()` (the CPU chain and DevicePlan.plan both draw it here)."""
        return random.random() < self.prob

    def __call__(self, img, label=None):
        if self.draw():
            img = img[:, ::-1, :]
            if label is not None:
                label = label[:, ::-1]
        return (img,) if label is None else (img, label)


class RandomVerticalFlip:
    """transforms.py:113-132: rows mirrored with probability `prob`, image and label alike."""

    def __init__(self, prob=0.1):
        self.prob = prob

    def draw(self):
        """The flip decision: one Python `random.random()` (the CPU chain and DevicePlan.plan both draw it here)."""
        return random.random() < self.prob

    def __call__(self, img, label=None):
        if self.draw():
            img = img[::-1, :, :]
            if label is not None:
                label = label[::-1, :]
        return (img,) if label is None else (img, label)


class RandomRot90:
    """Not in the reference: with probability `prob` the sample is turned by k quarter turns, k uniform over 1, 2, 3, counter-clockwise in array
    coordinates -- np.rot90(img, k, axes=(0, 1)), image and label alike.  The only exact rotation: no resampling, no padding, no label
    interpolation.  Square samples only (DATA.AUGMENT.ROT90_PROB)."""

    def __init__(self, prob=0.75):
        self.prob = prob

    def draw(self):
        """The turn k in 0..3: one Python `random.random()` and, only if that passes, one `random.randrange(3)` for k - 1 (the CPU chain and
        DevicePlan.plan both draw it here)."""
        if random.random() < self.prob:
            return 1 + random.randrange(3)
        return 0

    def __call__(self, img, label=None):
        k = self.draw()
        if k:
            if img.shape[0] != img.shape[1]:
                raise ValueError("RandomRot90: a quarter turn needs a square sample, got %dx%d (h x w)" % (img.shape[0], img.shape[1]))
            img = np.rot90(img, k, axes=(0, 1))
            if label is not None:
                label = np.rot90(label, k, axes=(0, 1))
        return (img,) if label is None else (img, label)


class RandomDistort:
    """transforms.py:588-681 with functional.py:76-96: brightness, contrast and saturation through PIL's ImageEnhance on the image truncated to
    uint8, in a shuffled order, each with its own probability and a factor drawn from [1 - range, 1 + range].  The label is untouched.

    Hue is refused: functional.hue adds a float to a uint8 HSV plane, a cast that is undefined for negative values (numpy warns), so there is
    nothing exact to reproduce; the HSV round trip alone changes pixels, so hue_prob > 0 is refused whatever hue_range is.  Pass
    hue_prob=0.  Hue keeps its place in the shuffle and its probability draw is still consumed, so a seeded run leaves `random` / `np.random`
    where the reference leaves them with hue_prob=0."""

    OPS = ("brightness", "contrast", "saturation", "hue")
    _ENHANCE = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}

    def __init__(self, brightness_range=0.5, brightness_prob=0.5, contrast_range=0.5, contrast_prob=0.5, saturation_range=0.5,
                 saturation_prob=0.5, hue_range=18, hue_prob=0.5):
        if hue_prob > 0:
            raise ValueError("RandomDistort: hue is not supported (hue_prob=%r, hue_range=%r): the reference's hue shift casts a negative float "
                             "to uint8, which has no defined result; pass hue_prob=0" % (hue_prob, hue_range))
        self.brightness_range, self.brightness_prob = brightness_range, brightness_prob
        self.contrast_range, self.contrast_prob = contrast_range, contrast_prob
        self.saturation_range, self.saturation_prob = saturation_range, saturation_prob
        self.hue_range, self.hue_prob = hue_range, hue_prob

    def draw(self):
        """The decisions, with the reference's draws: random.shuffle of the four ops, then per op in shuffled order np.random.uniform(0, 1) < prob
        and, only if that passes, np.random.uniform(lower, upper).  -> [(op name, factor)] of the applied ops, in application order."""
        ops = list(self.OPS)
        random.shuffle(ops)
        applied = []
        for name in ops:
            if np.random.uniform(0, 1) < getattr(self, name + "_prob"):
                r = getattr(self, name + "_range")
                applied.append((name, np.random.uniform(1 - r, 1 + r)))       # (hue never gets here: its probability is 0)
        return applied

    @classmethod
    def apply(cls, img, ops):
        """img HWC float -> uint8 (truncation) -> PIL -> the ops of draw() in order -> float32."""
        im = Image.fromarray(img.astype("uint8"))
        for name, factor in ops:
            im = cls._ENHANCE[name](im).enhance(factor)
        return np.asarray(im).astype("float32")

    def __call__(self, img, label=None):
        img = self.apply(img, self.draw())
        return (img,) if label is None else (img, label)


class Resize:
    """transforms.py:136-206: target_size (w, h) or int; keep_ori_size returns the input untouched."""

    def __init__(self, target_size=520, interp="LINEAR", keep_ori_size=False):
        self.target_size, self.interp, self.keep_ori_size = target_size, interp, keep_ori_size

    def __call__(self, img, label=None):
        if not self.keep_ori_size and self.target_size is not None:
            ts = self.target_size
            w, h = (ts, ts) if isinstance(ts, int) else (ts[0], ts[1])
            img = resize_bilinear(img, w, h)
            if label is not None:
                label = resize_nearest(label, w, h)
        return (img,) if label is None else (img, label)


class ResizeStepScaling:
    def __init__(self, min_scale_factor=0.75, max_scale_factor=1.25, scale_step_size=0.25):
        if min_scale_factor > max_scale_factor:
            raise ValueError("min_scale_factor must be less than max_scale_factor, but they are {} and {}.".format(min_scale_factor, max_scale_factor))
        self.min_scale_factor, self.max_scale_factor, self.scale_step_size = min_scale_factor, max_scale_factor, scale_step_size

    def draw(self):
        """The scale factor, with the reference's draws: none when min == max, np.random.uniform when the step is 0, else a shuffle."""
        if self.min_scale_factor == self.max_scale_factor:
            return self.min_scale_factor
        if self.scale_step_size == 0:
            return np.random.uniform(self.min_scale_factor, self.max_scale_factor)
        num_steps = int((self.max_scale_factor - self.min_scale_factor) / self.scale_step_size + 1)
        scale_factors = np.linspace(self.min_scale_factor, self.max_scale_factor, num_steps).tolist()
        np.random.shuffle(scale_factors)
        return scale_factors[0]

    @staticmethod
    def resized(scale_factor, h, w):
        """-> (h, w) of an h x w image scaled by scale_factor (Python round, as the reference)."""
        return int(round(scale_factor * h)), int(round(scale_factor * w))

    def __call__(self, img, label=None):
        h, w = self.resized(self.draw(), img.shape[0], img.shape[1])
        img = resize_bilinear(img, w, h)
        if label is not None:
            label = resize_nearest(label, w, h)
        return (img,) if label is None else (img, label)


class Normalize:
    def __init__(self, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        if not (isinstance(mean, (list, tuple)) and isinstance(std, (list, tuple))):
            raise ValueError("{}: input type is invalid. It should be list or tuple".format(self))
        if any(s == 0 for s in std):
            raise ValueError("{}: std is invalid!".format(self))
        self.mean, self.std = mean, std

    def __call__(self, img, label=None):
        mean = np.asarray(self.mean, dtype=np.float64).reshape(1, 1, -1)
        stdinv = 1.0 / np.asarray(self.std, dtype=np.float64).reshape(1, 1, -1)
        img = ((img.astype(np.float32) - mean) * stdinv).astype(np.float32)      # functional.imnormalize_
        return (img,) if label is None else (img, label)


class RandomPaddingCrop:
    def __init__(self, crop_size=(512, 512), img_padding_value=(123.675, 116.28, 103.53), label_padding_value=255):
        if isinstance(crop_size, (list, tuple)):
            if len(crop_size) != 2:
                raise ValueError("Type of `crop_size` is list or tuple. It should include 2 elements, but it is {}".format(crop_size))
        elif not isinstance(crop_size, int):
            raise TypeError("The type of `crop_size` is invalid. It should be list or tuple, but it is {}".format(type(crop_size)))
        self.crop_size, self.img_padding_value, self.label_padding_value = crop_size, img_padding_value, label_padding_value

    def size(self):
        """-> (crop height, crop width); crop_size is (w, h) or an int."""
        if isinstance(self.crop_size, int):
            return self.crop_size, self.crop_size
        return self.crop_size[1], self.crop_size[0]

    def draw(self, ih, iw):
        """Crop offsets (h_off, w_off) into an ih x iw image once padded bottom / right to the crop size, with the reference's two
        np.random.randint calls; None (no draw) when the image already has the crop size.  The draws happen whenever the size differs,
        even when padding then makes it equal to the crop."""
        chh, cw = self.size()
        if ih == chh and iw == cw:
            return None
        ih, iw = max(ih, chh), max(iw, cw)
        if chh > 0 and cw > 0:
            h_off = np.random.randint(ih - chh + 1)
            w_off = np.random.randint(iw - cw + 1)
            return h_off, w_off
        return None

    def __call__(self, img, label=None):
        chh, cw = self.size()
        ih, iw = img.shape[0], img.shape[1]
        offsets = self.draw(ih, iw)
        if not (ih == chh and iw == cw):
            ph, pw = max(chh - ih, 0), max(cw - iw, 0)
            if ph > 0 or pw > 0:            # bottom / right padding (cv2.copyMakeBorder BORDER_CONSTANT)
                padded = np.empty((ih + ph, iw + pw, img.shape[2]), dtype=img.dtype)
                padded[...] = np.asarray(self.img_padding_value, dtype=img.dtype)
                padded[:ih, :iw] = img
                img = padded
                if label is not None:
                    pl = np.full((ih + ph, iw + pw), self.label_padding_value, dtype=label.dtype)
                    pl[:ih, :iw] = label
                    label = pl
                ih, iw = img.shape[0], img.shape[1]
            if offsets is not None:
                h_off, w_off = offsets
                img = img[h_off:chh + h_off, w_off:w_off + cw, :]
                if label is not None:
                    label = label[h_off:chh + h_off, w_off:w_off + cw]
        return (img,) if label is None else (img, label)


_MEAN, _STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


# One sample's decisions for the device kernel (emrt_augment_tiles): source H x W, resized h x w, crop offsets into the resized image padded
# bottom / right to the crop size, horizontal flip after the crop.
SamplePlan = namedtuple("SamplePlan", "H W h w off_y off_x flip")
# ... of a chain with RandomVerticalFlip / RandomDistort (emrt_aug_tiles of the second library): SamplePlan's fields, the vertical flip, and the
# applied colour ops [(op name, factor)] in application order.
AugSamplePlan = namedtuple("AugSamplePlan", "H W h w off_y off_x flip vflip ops")
# ... of a chain with RandomRot90: `base` is the SamplePlan / AugSamplePlan of the same chain without it, `turn` the quarter turns (0..3) of the
# post-pass (emrt_rot_batch of libemrt_hip_rot.so) over the batch that the base plans produce.
RotPlan = namedtuple("RotPlan", "base turn")


class DevicePlan:
    """A training transform list compiled for the fused device kernel (emrt_amd.functional.augment_tiles).  Two chains are supported, the
    ones get_transforms ships: [ResizeStepScaling, RandomPaddingCrop, RandomHorizontalFlip, Normalize] (Potsdam, Vaihingen) and
    [Normalize] (LoveDA: output size = source size).  Any other op or order raises, naming the op: nothing is skipped or left to the CPU.
    The first chain may carry RandomVerticalFlip and / or RandomDistort, in that order, between RandomHorizontalFlip and Normalize
    (DATA.AUGMENT): `extended` is then True, plan() returns an AugSamplePlan and the loaders call the second library (functional.aug_tiles).
    RandomRot90 may follow those, before RandomDistort: plan() then returns RotPlan(base, turn) with the plan above as `base`, and the loaders
    turn the finished batch (functional.rot_batch); `extended` keeps its meaning.

    plan(H, W) draws one sample's random decisions with the draw helpers the CPU transforms themselves call (ResizeStepScaling.draw,
    RandomPaddingCrop.draw, RandomHorizontalFlip.draw, RandomVerticalFlip.draw, RandomRot90.draw, RandomDistort.draw), in the chain's order and under its
    conditions, so a seeded run makes the same decisions on either path and leaves np.random / random in the same state."""

    _HEAD = (ResizeStepScaling, RandomPaddingCrop, RandomHorizontalFlip)
    CHAINS = (_HEAD + (Normalize,), (Normalize,), _HEAD + (RandomVerticalFlip, Normalize), _HEAD + (RandomDistort, Normalize),
              _HEAD + (RandomVerticalFlip, RandomDistort, Normalize),
              _HEAD + (RandomRot90, Normalize), _HEAD + (RandomVerticalFlip, RandomRot90, Normalize), _HEAD + (RandomRot90, RandomDistort, Normalize),
              _HEAD + (RandomVerticalFlip, RandomRot90, RandomDistort, Normalize))

    def __init__(self, transforms):
        transforms = list(transforms)
        kinds = tuple(type(t) for t in transforms)
        if kinds not in self.CHAINS:
            best = max(self.CHAINS, key=lambda c: sum(1 for a, b in zip(c, kinds) if a is b))
            i = next((i for i, (a, b) in enumerate(zip(best, kinds)) if a is not b), min(len(best), len(kinds)))
            what = ("%s at position %d" % (type(transforms[i]).__name__, i)) if i < len(transforms) else "the chain ends early"
            raise ValueError("device transforms: %s is not supported; the device path runs [%s] or [%s] exactly, got [%s] (RandomVerticalFlip and "
                             "RandomDistort may follow RandomHorizontalFlip, in that order)" % (
                what, ", ".join(c.__name__ for c in self.CHAINS[0]), ", ".join(c.__name__ for c in self.CHAINS[1]),
                ", ".join(type(t).__name__ for t in transforms)))
        norm = transforms[-1]
        if len(norm.mean) != 3 or len(norm.std) != 3:
            raise ValueError("device transforms: Normalize needs 3 channels, got mean %r std %r" % (norm.mean, norm.std))
        self.mean = np.asarray(norm.mean, dtype=np.float64)
        self.stdinv = 1.0 / np.asarray(norm.std, dtype=np.float64)          # as Normalize computes it
        self.scaling = self.crop = self.flip = self.vflip = self.rot = self.distort = None
        self.img_pad, self.label_pad = np.zeros(3, np.float32), 255
        if len(transforms) >= 4:
            self.scaling, self.crop, self.flip = transforms[:3]
            for t in transforms[3:-1]:
                if isinstance(t, RandomVerticalFlip):
                    self.vflip = t
                elif isinstance(t, RandomRot90):
                    self.rot = t
                else:
                    self.distort = t
            chh, cw = self.crop.size()
            if chh <= 0 or cw <= 0:
                raise ValueError("device transforms: RandomPaddingCrop size must be positive, got %r" % (self.crop.crop_size,))
            if self.rot is not None:
                if chh != cw:
                    raise ValueError("device transforms: RandomRot90 needs a square crop, got %dx%d (h x w)" % (chh, cw))
                if not 0.0 <= float(self.rot.prob) <= 1.0:
                    raise ValueError("device transforms: RandomRot90 prob must lie in [0, 1], got %r" % (self.rot.prob,))
            pad = np.asarray(self.crop.img_padding_value, dtype=np.float32).reshape(-1)
            if pad.size != 3:
                raise ValueError("device transforms: img_padding_value needs 3 channels, got %r" % (self.crop.img_padding_value,))
            self.img_pad = pad
            self.label_pad = int(self.crop.label_padding_value)
            if not 0 <= self.label_pad <= 255:
                raise ValueError("device transforms: label_padding_value must be 0..255, got %r" % (self.crop.label_padding_value,))
            if self.distort is not None:
                if not all(0 <= float(v) < 256 for v in pad):
                    raise ValueError("device transforms: RandomDistort truncates to uint8; img_padding_value must lie in [0, 256), got %r" % (
                        self.crop.img_padding_value,))
                for name in RandomDistort.OPS[:3]:
                    r, p = getattr(self.distort, name + "_range"), getattr(self.distort, name + "_prob")
                    if not (0 <= r <= 1 and 0 <= p <= 1):
                        raise ValueError("device transforms: RandomDistort %s_range and %s_prob must lie in [0, 1], got %r and %r" % (name, name, r, p))

    @property
    def extended(self):
        """The chain holds RandomVerticalFlip or RandomDistort: it runs on the second library's entry points."""
        return self.vflip is not None or self.distort is not None

    def out_size(self, H, W):
        """-> (OH, OW) of a sample whose source is H x W."""
        return (H, W) if self.crop is None else self.crop.size()

    def plan(self, H, W):
        """Draw one H x W sample's decisions -> SamplePlan (AugSamplePlan for an extended chain; RotPlan around either for a chain with
        RandomRot90, whose turn is drawn in chain order, between the vertical flip and the distortion)."""
        if self.scaling is None:
            return SamplePlan(H, W, H, W, 0, 0, 0)
        h, w = ResizeStepScaling.resized(self.scaling.draw(), H, W)
        off = self.crop.draw(h, w) or (0, 0)
        flip = self.flip.draw()
        vflip = self.vflip.draw() if self.vflip is not None else False
        turn = self.rot.draw() if self.rot is not None else 0
        if not self.extended:
            base = SamplePlan(H, W, h, w, int(off[0]), int(off[1]), int(flip))
        else:
            ops = self.distort.draw() if self.distort is not None else []
            base = AugSamplePlan(H, W, h, w, int(off[0]), int(off[1]), int(flip), int(vflip), tuple((n, float(f)) for n, f in ops))
        return base if self.rot is None else RotPlan(base, int(turn))


def _augment(config, name, chain):
    """DATA.AUGMENT on a dataset's chain: RandomVerticalFlip and RandomDistort (hue off) go after the flip and before Normalize, the order of
    the reference's ADE20K chain; RandomRot90 (ROT90_PROB; not in the reference) goes between the two.  A chain without RandomHorizontalFlip
    (LoveDA's) has no place for them: the key is refused by name.  ROT90_PROB with a non-square DATA.CROP_SIZE is refused by name too."""
    aug = config.DATA.AUGMENT
    wanted = [k for k, on in (("DATA.AUGMENT.VFLIP_PROB", aug.VFLIP_PROB > 0), ("DATA.AUGMENT.DISTORT.ENABLE", bool(aug.DISTORT.ENABLE)),
                              ("DATA.AUGMENT.ROT90_PROB", aug.ROT90_PROB > 0)) if on]
    if not wanted:
        return chain
    at = next((i for i, t in enumerate(chain) if isinstance(t, RandomHorizontalFlip)), None)
    if at is None:
        raise ValueError("%s is set, but the %s chain is [%s]: the extra augmentations follow RandomHorizontalFlip, which it does not have" % (
            wanted[0], name, ", ".join(type(t).__name__ for t in chain)))
    extra = []
    if aug.VFLIP_PROB > 0:
        extra.append(RandomVerticalFlip(prob=aug.VFLIP_PROB))
    if aug.ROT90_PROB > 0:
        check_rot90(config)
        extra.append(RandomRot90(prob=aug.ROT90_PROB))
    if aug.DISTORT.ENABLE:
        d = aug.DISTORT
        extra.append(RandomDistort(brightness_range=d.BRIGHTNESS_RANGE, brightness_prob=d.BRIGHTNESS_PROB, contrast_range=d.CONTRAST_RANGE,
                                   contrast_prob=d.CONTRAST_PROB, saturation_range=d.SATURATION_RANGE, saturation_prob=d.SATURATION_PROB,
                                   hue_prob=0))
    return chain[:at + 1] + extra + chain[at + 1:]


def check_rot90(config):
    """DATA.AUGMENT.ROT90_PROB > 0 needs a square DATA.CROP_SIZE and a probability in [0, 1]: refused by name otherwise (the chain builder and
    train.py's start-up both call this)."""
    p, crop = config.DATA.AUGMENT.ROT90_PROB, tuple(config.DATA.CROP_SIZE)
    if not 0 <= p <= 1:
        raise ValueError("DATA.AUGMENT.ROT90_PROB must lie in [0, 1], got %r" % (p,))
    if p > 0 and (len(crop) != 2 or crop[0] != crop[1]):
        raise ValueError("DATA.AUGMENT.ROT90_PROB is set, but DATA.CROP_SIZE is %r: a quarter turn needs a square crop (w == h)" % (crop,))


def get_transforms(config):
    """Training transforms per dataset (src/transforms/__init__.py:4-57; only the datasets the EMRT yamls use)."""
    name = config.DATA.DATASET
    if name in ("Potsdam", "Vaihingen"):
        return _augment(config, name, [
            ResizeStepScaling(0.5, 2.0, 0.25),
            RandomPaddingCrop(crop_size=tuple(config.DATA.CROP_SIZE), img_padding_value=(0, 0, 0), label_padding_value=255),
            RandomHorizontalFlip(prob=0.5),
            Normalize(mean=_MEAN, std=_STD)])
    if name == "LoveDA":
        return _augment(config, name, [Normalize(mean=_MEAN, std=_STD)])
    raise NotImplementedError("{} dataset is not supported".format(name))


def get_val_transforms(config):
    """train.py:89-91 / val.py:95-97."""
    return [Resize(target_size=config.VAL.IMAGE_BASE_SIZE, keep_ori_size=config.VAL.KEEP_ORI_SIZE),
            Normalize(mean=list(config.VAL.MEAN), std=list(config.VAL.STD))]
