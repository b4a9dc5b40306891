"""Window-level test-time augmentation restated in numpy / float64: the variants of a window, their inverses, the normalised
variant batch, the softmax sums and hit counts of a list of windows, and the error bound the kernels are held to.  Shared by
tests/test_tta_cpu.py and tests/test_gpu_tta.py; nothing here touches a device or the package."""
import numpy as np

MODES = {"none": [0], "hflip": [0, 1], "flips": [0, 1, 2, 3], "d4": [0, 1, 2, 3, 4, 5, 6, 7]}


def variant(a, code):
    """[..., h, w] -> the variant `code` = t * 4 + fv * 2 + fh: rows reversed if fv, columns reversed if fh, then transposed if t"""
    if code & 2:
        a = a[..., ::-1, :]
    if code & 1:
        a = a[..., :, ::-1]
    if code & 4:
        a = np.swapaxes(a, -1, -2)
    return a


def inverse(m, code):
    """what undoes variant(., code) on a map made from the variant: transposed if t, then the same reversals"""
    if code & 4:
        m = np.swapaxes(m, -1, -2)
    if code & 2:
        m = m[..., ::-1, :]
    if code & 1:
        m = m[..., :, ::-1]
    return m


def crop_variants(scene_u8, org, codes, ch, cw, mean, std):
    """uint8 [H, W, 3], origins (y, x) -> float64 [n * G, 3, ch, cw], variant g of window j at j * G + g; (u8 - mean) * (1 / std) in float64,
    transforms.Normalize's arithmetic (the kernel rounds this once to fp32: compare with .astype(np.float32))"""
    mean = np.asarray(mean, dtype=np.float64).reshape(3, 1, 1)
    stdinv = (1.0 / np.asarray(std, dtype=np.float64)).reshape(3, 1, 1)
    out = []
    for y, x in org:
        win = (np.transpose(scene_u8[y:y + ch, x:x + cw].astype(np.float64), (2, 0, 1)) - mean) * stdinv
        out += [variant(win, k) for k in codes]
    return np.ascontiguousarray(np.stack(out))


def softmax(z, axis):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def cover(H, W, org, ch, cw):
    """int64 [H, W]: how many of the windows cover a pixel"""
    k = np.zeros((H, W), dtype=np.int64)
    for y, x in org:
        k[y:y + ch, x:x + cw] += 1
    return k


def accumulate(logits, org, codes, H, W, final=None, count=None):
    """logits [n * G, C, ch, cw] (any float dtype) of the variants of the windows at `org` -> (final float64 [C, H, W], count float64 [H, W]):
    final += the softmax of every variant's logits, turned back; count += G per covering window.  Adds to the arrays given, else starts at 0."""
    logits = np.asarray(logits, dtype=np.float64)
    G, C, ch, cw = len(codes), logits.shape[1], logits.shape[2], logits.shape[3]
    assert logits.shape[0] == len(org) * G
    final = np.zeros((C, H, W)) if final is None else final
    count = np.zeros((H, W)) if count is None else count
    for j, (y, x) in enumerate(org):
        for g, k in enumerate(codes):
            final[:, y:y + ch, x:x + cw] += softmax(inverse(logits[j * G + g], k), axis=0)
        count[y:y + ch, x:x + cw] += G
    return final, count


def bound(K, G, C):
    """Absolute bound on an fp32 sum of K * G softmax terms of C classes against float64: per term expf and the reciprocal at a few ulp and a
    C-term denominator, (C + 8) * 2^-24 * 2 relative on a value <= 1, and K * G additions of partial sums -- together K * G * (C + 8) * 2^-23."""
    return K * G * (C + 8) * 2.0 ** -23
