"""The class-aware tile sampler (include/emrt_hip_sampler.h) restated in Python: the row counts by np.bincount, the class
probabilities and thresholds, and the redraw of emrt_smp_class_redraw.  Philox4x32-10 and the 64-bit draw are the restatement
tests/test_scene_sampler_cpu.py already holds to the Random123 known answers.  tests/test_class_sampler_cpu.py checks what this restatement
promises (the distribution, the window around the anchor); tests/test_gpu_class_sampler.py holds the kernels to it bit for bit."""
import math

import numpy as np

from tests.test_scene_sampler_cpu import M32, below, philox4x32_10

TWO32 = 1 << 32


def mapped(labels, lut=None):
    """The label maps as the kernels see them: after the 256-entry lookup table, when there is one."""
    return [np.asarray(lab) if lut is None else np.asarray(lut, dtype=np.uint8)[np.asarray(lab)] for lab in labels]


def row_counts(labels, n_classes, lut=None):
    """int64 [R][n_classes]: pixels of every class in every row of every label map, in bank order; values >= n_classes are not counted."""
    return np.asarray([np.bincount(row, minlength=256)[:n_classes] for lab in mapped(labels, lut) for row in lab], dtype=np.int64)


def probabilities(totals, temperature=0.1, class_probs=None):
    """P(c) proportional to exp((1 - f_c) / T), f_c = the class's share of the counted pixels, or to class_probs[c]; 0 for a class without a pixel."""
    n = np.asarray(totals, dtype=np.int64)
    f = n.astype(np.float64) / float(n.sum())
    w = np.exp((1.0 - f) / float(temperature)) if class_probs is None else np.asarray(class_probs, dtype=np.float64)
    w = np.where(n > 0, w, 0.0)
    return w / w.sum()


def thresholds(p):
    """[int]: floor(2^32 * running sum of p) in float64; exactly 2^32 from the last class with a non-zero probability on."""
    acc, thr = np.float64(0.0), []
    for v in np.asarray(p, dtype=np.float64):
        acc = acc + v
        thr.append(min(int(math.floor(acc * 4294967296.0)), TWO32))
    last = max(c for c, v in enumerate(p) if v > 0)
    return [t if c < last else TWO32 for c, t in enumerate(thr)]


def pick_class(word, thr):
    """The class a 32-bit word picks: the number of thresholds it reaches, at most the first class whose threshold is 2^32."""
    return min(sum(word >= t for t in thr), thr.index(TWO32))


def redraw(rows, key, step, rank, labels, tile, n_classes, thr, prob, lut=None, counts=None):
    """emrt_smp_class_redraw on the draw table `rows` (B rows of 10 or 18 columns) -> (the new table, one entry per sample: None where the row
    was left alone, else (cls, scene, y, x, dy, dx) with (y, x) the anchor pixel).  `counts`: an index other than this bank's own (a stale one);
    a pixel it promises and the row does not hold leaves the row alone."""
    th, tw = tile
    maps = mapped(labels, lut)
    cnt = row_counts(labels, n_classes, lut) if counts is None else np.asarray(counts, dtype=np.int64)
    R = sum(m.shape[0] for m in maps)
    assert cnt.shape == (R, n_classes)
    cum = np.zeros((n_classes, R + 1), dtype=np.int64)
    cum[:, 1:] = np.cumsum(cnt.T, axis=1)
    row_start = [0]
    for m in maps:
        row_start.append(row_start[-1] + m.shape[0])
    thr = [int(t) for t in thr]
    B, k2 = len(rows), (key & M32, (key >> 32) & M32)
    out, info = [list(r) for r in rows], []
    for b in range(B):
        ctr = [step & M32, (step >> 32) & M32, (rank * B + b) & M32]
        r8, r9 = philox4x32_10(ctr + [8], k2), philox4x32_10(ctr + [9], k2)
        info.append(None)
        if not r8[0] * 2.0 ** -32 < prob:
            continue
        cls = pick_class(r8[1], thr)
        n_cls = int(cum[cls][R])
        if n_cls <= 0:
            continue
        k = below(r8[2], r8[3], n_cls)
        Ri = int(np.searchsorted(cum[cls][:R], k, side="right")) - 1          # the last row whose prefix is <= k (cum[cls][0] is 0)
        j = k - int(cum[cls][Ri])
        s = max(i for i in range(len(maps)) if row_start[i] <= Ri)
        y = Ri - row_start[s]
        H, W = maps[s].shape
        xs = np.flatnonzero(maps[s][y] == cls)
        if j < 0 or j >= len(xs):
            continue
        x = int(xs[j])
        dy, dx = (r9[0] * th) >> 32, (r9[1] * tw) >> 32
        out[b][0:3] = [s, min(max(y - dy, 0), H - th), min(max(x - dx, 0), W - tw)]
        info[b] = (cls, s, y, x, dy, dx)
    return out, info


def rare_class_labels(sizes, seed=0, shift=0):
    """Label maps of the sampler's tests: classes 0 and 1 as noise (about 70 % / 25 %), 5 % ignored (255), class 2 on exactly three pixels -- (0, 0)
    of the first scene, the last pixel of the last scene, and column W - 1 - 64 of the last scene's middle row -- and class 3 absent.  shift 1:
    the same maps as LoveDA stores them (every class one higher, 0 = ignore; 255 stays), to be read through label_lut(1)."""
    rng = np.random.RandomState(seed)
    labs = []
    for H, W in sizes:
        u = rng.rand(H, W)
        labs.append(np.where(u < 0.70, 0, np.where(u < 0.95, 1, 255)).astype(np.uint8))
    H, W = sizes[-1]
    labs[0][0, 0] = 2
    labs[-1][H - 1, W - 1] = 2
    labs[-1][H // 2, W - 1 - 64 if W > 64 else W // 2] = 2
    if shift:
        labs = [np.where(lab == 255, rng.choice(np.asarray([0, 255], np.uint8), lab.shape), lab + np.uint8(shift)).astype(np.uint8) for lab in labs]
    return labs


def write_bank(root, sizes, labels, seed=0):
    """<root>/images/scene_<i>.tif (noise) + <root>/labels/scene_<i>.png (the given maps) -> [(img, lab)]."""
    import os
    from PIL import Image
    rng = np.random.RandomState(seed + 1)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "labels"), exist_ok=True)
    out = []
    for i, ((H, W), lab) in enumerate(zip(sizes, labels)):
        img = rng.randint(0, 256, (H, W, 3), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(root, "images", "scene_%d.tif" % i))
        Image.fromarray(lab).save(os.path.join(root, "labels", "scene_%d.png" % i))
        out.append((img, lab))
    return out
