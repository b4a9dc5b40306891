"""PIL's ImageEnhance.Brightness / Contrast / Color restated in plain numpy (no PIL, no library import): what the device kernels of
csrc/augment_ext are held to, and itself held to PIL in tests/test_augment_ext_cpu.py.

  L     = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16                            (Image.convert("L"))
  blend = d + f * (x - d) in float32, f rounded to float32, the product rounded before the sum (no fused multiply-add);
          0 <= f <= 1: truncated to uint8; otherwise 0 where t <= 0, 255 where t >= 255, truncated between  (Image.blend)
  d     = 0 (brightness); int(sum(L) / count + 0.5) over the whole image the op sees (contrast); the pixel's own L (saturation)
"""
import numpy as np

OPS = ("brightness", "contrast", "saturation")


def luminance(img):
    """uint8 HWC RGB -> int64 HW."""
    a = img.astype(np.int64)
    return (a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16


def blend(d, x, f):
    """d, x: integer arrays 0..255 (broadcastable); f: the factor -> uint8."""
    f = np.float32(f)
    d32 = np.asarray(d).astype(np.float32)
    prod = (f * (np.asarray(x).astype(np.float32) - d32)).astype(np.float32)
    t = (d32 + prod).astype(np.float32)
    if 0 <= f <= 1:
        return t.astype(np.int64).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64)))
    return out.astype(np.uint8)


def contrast_mean(img):
    l = luminance(img)
    return int(int(l.sum()) / l.size + 0.5)


def enhance(img, op, f):
    """One op on a uint8 HWC RGB image -> uint8 HWC."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    if op == "brightness":
        d = np.zeros((1, 1, 1), np.int64)
    elif op == "contrast":
        d = np.full((1, 1, 1), contrast_mean(img), np.int64)
    elif op == "saturation":
        d = luminance(img)[..., None]
    else:
        raise ValueError(op)
    return blend(d, img.astype(np.int64), f)


def distort(img, ops):
    """RandomDistort.apply restated: float HWC -> uint8 (truncation) -> the ops [(name, factor)] in order -> float32."""
    x = img.astype(np.uint8)
    for name, f in ops:
        x = enhance(x, name, f)
    return x.astype(np.float32)
