"""Multi-scale window-level test-time augmentation restated in numpy / float64: the integer tap rule, the resampled variant batch,
the softmax sums and hit counts of a list of footprints, the footprint grids, the inputs of the GPU cases (so that the CPU tests can judge them
from the reference alone) and the error bounds the kernels are held to.  Variants and softmax are tests/tta_reference.py's.  Shared by
tests/test_ms_tta_cpu.py and tests/test_gpu_ms_tta.py; nothing here touches a device or the package."""
import numpy as np

from tests import tta_reference as R

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
MODES = R.MODES


# ---- the resampling rule ---------------------------------------------------------------------------------------------------------------------
def taps(n_out, n_src):
    """-> (i0, i1 int64 [n_out], w float64 [n_out]): output index i reads i0 and i1 with weight w on i1.  The indices are exact (integers);
    w is the rational (num - i0 den) / den to float64's 2^-53, where the kernel rounds it to fp32."""
    i = np.arange(n_out, dtype=np.int64)
    num, den = (2 * i + 1) * n_src - n_out, 2 * n_out
    i0 = np.where(num <= 0, 0, num // den)
    edge = (num <= 0) | (i0 >= n_src - 1)
    i0 = np.minimum(i0, n_src - 1)
    w = np.where(edge, 0.0, (num - i0 * den) / float(den))
    return i0, np.minimum(i0 + 1, n_src - 1), w


def resample(a, oh, ow):
    """[..., h, w] -> float64 [..., oh, ow]: bilinear, align_corners = False, by the tap rule; top = a + wx (b - a), v = top + wy (bot - top)"""
    a = np.asarray(a, dtype=np.float64)
    y0, y1, wy = taps(oh, a.shape[-2])
    x0, x1, wx = taps(ow, a.shape[-1])
    r0, r1 = a[..., y0, :], a[..., y1, :]
    top = r0[..., x0] + wx * (r0[..., x1] - r0[..., x0])
    bot = r1[..., x0] + wx * (r1[..., x1] - r1[..., x0])
    return top + wy[:, None] * (bot - top)


def tap_max(a, oh, ow):
    """[h, w] -> [oh, ow]: the largest of a at the four taps of every output pixel"""
    y0, y1, _ = taps(oh, a.shape[-2])
    x0, x1, _ = taps(ow, a.shape[-1])
    return np.maximum(np.maximum(a[y0][:, x0], a[y0][:, x1]), np.maximum(a[y1][:, x0], a[y1][:, x1]))


# ---- footprints ------------------------------------------------------------------------------------------------------------------------------
def window_grid(h, w, crop, stride):
    """the sliding-window origins (y, x) of an h x w image for crop / stride given as (w, h): rows then columns, the last of a row or column
    shifted back inside (what infer.window_grid lays out)"""
    (cw, ch), (sw, sh) = crop, stride
    rows, cols = max(h - ch + sh - 1, 0) // sh + 1, max(w - cw + sw - 1, 0) // sw + 1
    out = []
    for r in range(rows):
        for c in range(cols):
            y, x = r * sh, c * sw
            if y >= h or x >= w:
                continue
            out.append((max(min(y + ch, h) - ch, 0), max(min(x + cw, w) - cw, 0)))
    return out


def footprints(H, W, crop, stride, s):
    """-> ((fw, fh), (sw, sh), [(y, x)]): f = int(c / s + 0.5), stride min(f, max(1, int(t / s + 0.5))), origins in grid order"""
    size = tuple(int(c / s + 0.5) for c in crop)
    step = tuple(min(f, max(1, int(t / s + 0.5))) for f, t in zip(size, stride))
    assert H >= size[1] and W >= size[0]
    return size, step, window_grid(H, W, size, step)


# ---- the two kernels -------------------------------------------------------------------------------------------------------------------------
def crop_variants_ms(scene_u8, org, codes, fh, fw, ch, cw, mean=MEAN, std=STD):
    """uint8 [H, W, 3], footprint origins (y, x) -> float64 [n * G, 3, ch, cw], variant g of footprint j at j * G + g: the footprint's bytes
    resampled to ch x cw, then (v - mean) * (1 / std)"""
    mean = np.asarray(mean, dtype=np.float64).reshape(3, 1, 1)
    stdinv = (1.0 / np.asarray(std, dtype=np.float64)).reshape(3, 1, 1)
    out = []
    for y, x in org:
        win = (resample(np.transpose(scene_u8[y:y + fh, x:x + fw].astype(np.float64), (2, 0, 1)), ch, cw) - mean) * stdinv
        out += [R.variant(win, k) for k in codes]
    return np.ascontiguousarray(np.stack(out))


def accumulate_ms(logits, org, codes, H, W, fh, fw, final=None, count=None, bound=None):
    """logits [n * G, C, ch, cw] of the variants of the footprints at `org` -> (final float64 [C, H, W], count float64 [H, W], bound float64
    [H, W]): final += the softmax of every variant's logits, turned back and resampled to the footprint; count += G per covering footprint;
    bound += acc_term_bound per term.  Adds to the arrays given, else starts at 0."""
    logits = np.asarray(logits, dtype=np.float64)
    G, C = len(codes), logits.shape[1]
    assert logits.shape[0] == len(org) * G
    final = np.zeros((C, H, W)) if final is None else final
    count = np.zeros((H, W)) if count is None else count
    bound = np.zeros((H, W)) if bound is None else bound
    for j, (y, x) in enumerate(org):
        for g, k in enumerate(codes):
            m = R.inverse(logits[j * G + g], k)
            final[:, y:y + fh, x:x + fw] += R.softmax(resample(m, fh, fw), axis=0)
            bound[y:y + fh, x:x + fw] += acc_term_bound(C, tap_max(np.abs(m).max(0), fh, fw))
        count[y:y + fh, x:x + fw] += G
    return final, count, bound


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------------
def crop_bound(ref, std=STD):
    """Absolute bound per value of the fp32 crop against float64 `ref` [..., 3, h, w]: 8 * 255 * 2^-24 * stdinv_c + 2^-24 * |ref|.
    Seven fp32 roundings at magnitude <= 255 lie on the path and one is spare for the compiler's choice of contraction: a horizontal lerp has
    three (the weight, the product, the sum); the vertical lerp inherits at most 3, as the convex mix of top and bot, and adds four of its own
    (the difference, the weight, the product, the sum).  Each is at most 255 * 2^-24 on the blend and is scaled by stdinv_c; the last term is
    the cast of the normalised value to fp32."""
    stdinv = (1.0 / np.asarray(std, dtype=np.float64)).reshape(3, 1, 1)
    return 8 * 255 * 2.0 ** -24 * stdinv + 2.0 ** -24 * np.abs(ref)


def acc_term_bound(C, m):
    """Absolute bound of ONE softmax term of the fp32 sums: (C + 8) * 2^-23 + m * 2^-20, m the largest |logit| among the term's four taps over
    all classes.  (C + 8) * 2^-23 is tta_reference.bound's per-term figure (expf, the reciprocal, a C-term denominator, the addition to the
    sum).  The blended logits are off by at most 8 * m * 2^-24 = m * 2^-21 (the eight roundings of crop_bound, at magnitude <= m), and a
    softmax moves by at most twice the largest shift of its logits: m * 2^-20."""
    return (C + 8) * 2.0 ** -23 + m * 2.0 ** -20


def undecided(final, bound):
    """share of the pixels whose two largest sums lie within twice the per-pixel bound: where a class index is not compared"""
    top = np.sort(final, axis=0)
    return float(((top[-1] - top[-2]) <= 2 * bound).mean())


# ---- the inputs of the GPU cases (tests/test_gpu_ms_tta.py runs them; tests/test_ms_tta_cpu.py judges the share left undecided) ---------------------
SCALES = [0.5, 0.8, 1.0, 1.6, 2.0]          # crop 16 -> footprints 32, 20, 16, 10, 8
ACC_MAP, ACC_CROP, ACC_STRIDE = (37, 41), (16, 16), (13, 14)          # 4, 6, 9, 20 and 36 footprints; 4 over a pixel at most, at every scale
ACC_CLASSES, ACC_MODES = [1, 6, 19], ["none", "flips", "d4"]


def acc_case(C, s, mode):
    """-> (org, fh, fw, logits fp32 [n * G, C, 16, 16], final0 fp32 [C, H, W], count0 fp32 [H, W]): logits N(0, 1) * 3 with 0.2 % of the entries
    at +-40 (a softmax without the max subtraction overflows there; a scaling that saturates every softmax would leave the class undecided
    wherever few terms meet), sums and counts pre-filled"""
    H, W = ACC_MAP
    (fw, fh), _, org = footprints(H, W, ACC_CROP, ACC_STRIDE, s)
    G = len(MODES[mode])
    rng = np.random.RandomState(6300 + 100 * C + int(round(s * 10)) + 1000 * G)
    logits = (rng.standard_normal((len(org) * G, C, ACC_CROP[1], ACC_CROP[0])) * 3).astype(np.float32)
    flat = logits.reshape(-1)
    hot = rng.choice(flat.size, max(2, int(0.002 * flat.size)), replace=False)
    flat[hot[::2]], flat[hot[1::2]] = 40.0, -40.0
    final0 = (rng.random_sample((C, H, W)) * 0.75 + 0.25).astype(np.float32)
    count0 = rng.randint(1, 4, (H, W)).astype(np.float32)
    return org, fh, fw, logits, final0, count0


PIPE_NCLS, PIPE_CROP, PIPE_STRIDE, PIPE_MAX_BATCH = 6, (32, 32), (24, 24), 16
PIPE_SIZES, PIPE_SCALES, PIPE_MODES, PIPE_SEED = [(72, 88), (64, 50)], (0.75, 1.0, 1.5), ["none", "d4"], 64


def stub_params(equivariant, ncls=PIPE_NCLS, crop=32):
    """-> (mix [ncls, 3], ramp [ncls, crop, crop] or None, both fp32).  The stub model's logits are mix applied to the window pixel by pixel plus
    the ramp: with the ramp they are neither equivariant under the variants nor invariant under scale, so a wrong inverse or a wrong tap moves
    the sums."""
    rng = np.random.RandomState(6400)
    mix = (rng.standard_normal((ncls, 3)) * 1.5).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(crop, dtype=np.float32), np.arange(crop, dtype=np.float32), indexing="ij")
    ramp = np.stack([(k + 1) * 0.05 * ys - (ncls - k) * 0.03 * xs + 0.002 * k * ys * xs / crop for k in range(ncls)]).astype(np.float32)
    return mix, (None if equivariant else ramp)


def stub_logits(batch, mix, ramp):
    """the stub on a float64 batch [n, 3, h, w] -> float64 [n, ncls, h, w]"""
    out = np.einsum("kc,nchw->nkhw", mix.astype(np.float64), batch)
    return out if ramp is None else out + ramp.astype(np.float64)


CONST_LOGITS = [0.3, -1.2, 2.1, 0.9, -0.4, 1.7]          # the stub that is exactly equivariant AND scale-invariant: the same logits at every pixel


def pipeline_reference(scene_u8, crop, stride, scales, codes, max_batch, model, logits=None):
    """The float64 sums, counts and per-pixel bound of one scene: the scales in the order given, the footprints in grid order, max_batch // G per
    model call.  `model` maps a float64 batch to logits; with `logits` (a list of recorded arrays, consumed from the front) the recorded logits
    of the device's own model calls are accumulated instead and `model` is not called."""
    H, W = scene_u8.shape[:2]
    G, per = len(codes), max_batch // len(codes)
    final = count = bound = None
    for s in scales:
        (fw, fh), _, org = footprints(H, W, crop, stride, s)
        for i in range(0, len(org), per):
            chunk = org[i:i + per]
            if logits is None:
                lg = model(crop_variants_ms(scene_u8, chunk, codes, fh, fw, crop[1], crop[0]))
            else:
                lg = logits.pop(0)
                assert lg.shape[0] == len(chunk) * G
            final, count, bound = accumulate_ms(lg, chunk, codes, H, W, fh, fw, final, count, bound)
    return final, count, bound
