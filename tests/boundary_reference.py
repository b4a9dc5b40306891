"""The numpy host model of boundary-aware scene evaluation (include/emrt_hip_bnd.h), written as the definition reads: a brute-force
loop over the offsets of the structuring element, not the row-then-column decomposition of the kernels.  The tests compare the kernels (GPU) and
the scipy erosion formulation (CPU) against it; tools/bench_boundary.py times it."""
import numpy as np

MAX_RADIUS = 32
SHAPES = {"disk": 0, "square": 1}


def half_widths(r, shape):
    """w(dy) for dy = -r..r, in integers: r for the square, the largest w with w * w + dy * dy <= r * r for the disk"""
    if shape not in SHAPES:
        raise ValueError("shape must be one of %s, got %r" % (", ".join(SHAPES), shape))
    if shape == "square":
        return [r] * (2 * r + 1)
    out = []
    for dy in range(-r, r + 1):
        w = 0
        while (w + 1) * (w + 1) + dy * dy <= r * r:
            w += 1
        out.append(w)
    return out


def structure(r, shape):
    """the structuring element as a bool [2r + 1, 2r + 1] array (what scipy.ndimage.binary_erosion takes)"""
    S = np.zeros((2 * r + 1, 2 * r + 1), dtype=bool)
    for i, w in enumerate(half_widths(r, shape)):
        S[i, r - w:r + w + 1] = True
    return S


def band(M, r, shape):
    """bool [H, W]: some in-image neighbour (y + dy, x + dx), |dx| <= w(dy), holds another value than M[y, x]"""
    M = np.asarray(M)
    H, W = M.shape
    out = np.zeros((H, W), dtype=bool)
    for dy, w in zip(range(-r, r + 1), half_widths(r, shape)):
        if abs(dy) >= H:
            continue
        for dx in range(-min(w, W - 1), min(w, W - 1) + 1):
            here = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
            there = (slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))
            out[here] |= M[here] != M[there]
    return out


def runs(M, r):
    """uint8 [H, W]: min(r, the largest k such that every in-image pixel of [x - k, x + k] in row y equals M[y, x]) -- what emrt_bnd_runs writes"""
    M = np.asarray(M)
    H, W = M.shape
    out = np.zeros((H, W), dtype=np.uint8)
    alive = np.ones((H, W), dtype=bool)
    for k in range(1, r + 1):
        if k < W:
            alive[:, k:] &= M[:, k:] == M[:, :-k]
            alive[:, :-k] &= M[:, :-k] == M[:, k:]
        out[alive] = k
    return out


def areas(pred, label, ncls, ignore, select):
    """int64 [3, ncls]: intersect / prediction / label pixel counts over the pixels with label != ignore, each restricted by its own mask of
    `select` (three bool arrays); values outside [0, ncls) are counted nowhere"""
    pred, label = np.asarray(pred).astype(np.int64).reshape(-1), np.asarray(label).astype(np.int64).reshape(-1)
    keep = label != ignore
    out = np.zeros((3, ncls), dtype=np.int64)
    for row, (values, mask) in enumerate(zip((pred, pred, label), select)):
        ok = keep & np.asarray(mask).reshape(-1) & (values >= 0) & (values < ncls)
        if row == 0:
            ok &= pred == label
        out[row] = np.bincount(values[ok], minlength=ncls)
    return out


def counts(pred, label, ncls, ignore, r, shape, band_pred=None, band_label=None):
    """int64 [2, 3, ncls], what emrt_bnd_areas adds for one scene: [0] the areas over the pixels outside the label's band (the ISPRS eroded
    protocol), [1] the three areas of Boundary IoU"""
    pred, label = np.asarray(pred), np.asarray(label)
    bp = band(pred, r, shape) if band_pred is None else np.asarray(band_pred).astype(bool)
    bl = band(label, r, shape) if band_label is None else np.asarray(band_label).astype(bool)
    return np.stack([areas(pred, label, ncls, ignore, (~bl, ~bl, ~bl)), areas(pred, label, ncls, ignore, (bl & bp, bp, bl))])
