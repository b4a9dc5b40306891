"""Whole-scene prediction: a uint8 RGB scene of any size -> class indices, colour mask, overlay and per-class areas, all on the device
(DESIGN.md 16).  What the reference's predict.py does with one window per model call, a host argmax and a per-class colouring loop in numpy:

    crop + normalise windows from the uint8 scene   emrt_scene_crop_windows_u8 (transforms.Normalize's arithmetic, bit for bit)
    model                                           one call per `max_batch` windows, in infer.window_grid order: slide_inference's logits
    accumulate sums and hit counts                  emrt_window_accumulate
    finish                                          emrt_scene_finish: divide, argmax, palette, overlay, areas in one pass over the sums

Nothing is resized: a scene is predicted at its own resolution with the configured crop and stride.  With `scales`, the softmax sums of
infer.ms_accumulate (multi-scale + horizontal flip) are finished instead.

SceneEvaluator runs the same windows over the scenes of a resident validation bank (datasets.SceneBank) and counts the metric areas
against the bank's uint8 label maps where they lie: emrt_window_normalise, emrt_argmax_nchw and emrt_segmentation_areas stand where the finish stands.

Both take `tta`: "hflip", "flips" or "d4" puts every window through the model in 2, 4 or 8 flipped / turned variants and averages
the class probabilities of all variants of all covering windows -- two launches of libemrt_hip_tta.so around the model call stand where the crop
and the accumulation stand; "none" (the default) issues what it always issued and never loads that library.

Both take `tta_scales`, with any `tta`: a sequence of scales in [0.25, 4].  At scale s a window is resampled from a footprint of
crop / s native pixels where it is cropped from the uint8 scene, and its logits are resampled back where they are accumulated -- two launches of
libemrt_hip_mstta.so per model call, no scaled scene and no fp32 scene; the result is the mean class probability over every scale, covering
footprint and variant.  None (the default) takes the paths above untouched and never loads that library.

SceneEvaluator takes `boundary`: a radius r in 1..32 adds, per scene, the launches of libemrt_hip_bnd.so that mark the pixels within r
of another class in the prediction and in the label map and count the ISPRS eroded-boundary areas and the Boundary IoU areas from them.  None
(the default) issues what it always issued and never loads that library.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import infer
from ... import _lib
from ... import functional as Fn
from ...runtime import ctx

MAX_WINDOWS = 64          # csrc/common.hpp EMRT_MAX_WINDOWS: origins of one launch

# index uint8 [H, W], color uint8 [H, W, 3], overlay uint8 [H, W, 3] or None, areas int64 [ncls] (pixels per class); predict_tiles adds a
# leading tile dimension to the first three
SceneResult = namedtuple("SceneResult", "index color overlay areas")


def _origins(org):
    arr = (ctypes.c_int * (2 * len(org)))(*[v for yx in org for v in yx])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def check_windows(crop_size, stride_size):
    """-> (crop, stride) as int (w, h) pairs; a stride larger than the crop is refused"""
    crop, stride = tuple(int(v) for v in crop_size), tuple(int(v) for v in stride_size)
    if len(crop) != 2 or len(stride) != 2 or min(crop + stride) < 1:
        raise ValueError("crop_size and stride_size are positive (w, h) pairs, got %r and %r" % (crop_size, stride_size))
    if stride[0] > crop[0] or stride[1] > crop[1]:
        raise ValueError("stride %r is larger than the crop %r: the windows would leave uncovered stripes (NaN logits in the reference)"
                         % (stride, crop))
    return crop, stride


def check_normalise(mean, std):
    """-> (mean, 1 / std) as lists of Python floats, as transforms.Normalize computes them"""
    if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
        raise ValueError("mean / std need 3 channels and a non-zero std, got %r / %r" % (mean, std))
    return [float(v) for v in np.asarray(mean, dtype=np.float64)], [float(v) for v in 1.0 / np.asarray(std, dtype=np.float64)]


def crop_windows(scene, H, W, org, ch, cw, mean, stdinv):
    """windows at `org` of the uint8 [H, W, 3] scene -> normalised fp32 [n, 3, ch, cw] (+ the origins' pointer and the array that owns it)"""
    c = ctx()
    arr, ptr = _origins(org)
    batch = c.empty((len(org), 3, ch, cw), torch.float32)
    Fn._L().call("emrt_scene_crop_windows_u8", Fn.P(scene), Fn.P(batch), ptr, len(org), H, W, ch, cw, *mean, *stdinv, c.stream)
    return batch, ptr, arr


# Test-time augmentation of a window: mode -> variant codes, t * 4 + fv * 2 + fh (include/emrt_hip_tta.h): the window with its rows
# reversed if fv and its columns reversed if fh, then transposed if t.  "d4" is the eight flips and quarter turns of a square window.
TTA_MODES = {"none": (0,), "hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def check_tta(tta, crop, max_batch, scales):
    """-> the variant codes of mode `tta` for windows of `crop` (w, h); what cannot run is refused here, before anything is loaded"""
    if tta not in TTA_MODES:
        raise ValueError("tta must be one of %s, got %r" % (", ".join(TTA_MODES), tta))
    codes = TTA_MODES[tta]
    if len(codes) > 1:
        if scales is not None:
            raise ValueError("tta=%r cannot be combined with scales: multi-scale inference keeps its own horizontal flip" % tta)
        if any(k & 4 for k in codes) and crop[0] != crop[1]:
            raise ValueError("tta=%r turns windows by 90 degrees and needs a square crop, got %dx%d (w x h)" % (tta, crop[0], crop[1]))
        if max_batch < len(codes):
            raise ValueError("tta=%r makes %d variants of a window and needs max_batch >= %d, got %d" % (tta, len(codes), len(codes), max_batch))
    return codes


def accumulate_windows_tta(model, scene, H, W, org, crop, ncls, max_batch, mean, stdinv, final, count, codes):
    """The windows at `org` in that order, max_batch // G per model call, each with its G = len(codes) variants (variant g of window j is image
    j * G + g of the call): emrt_tta_crop_windows_u8 makes them from the uint8 scene, emrt_tta_window_accumulate adds the softmax of every
    variant's logits, turned back, to `final` [1, ncls, H, W] and G per covering window to `count` [1, 1, H, W]."""
    T, c = _lib.tta_lib(), ctx()
    w_crop, h_crop = crop
    G = len(codes)
    karr = (ctypes.c_int * G)(*codes)
    kptr = ctypes.cast(karr, ctypes.c_void_p)
    per = max_batch // G
    for i in range(0, len(org), per):
        chunk = org[i:i + per]
        _keep, ptr = _origins(chunk)
        batch = c.empty((len(chunk) * G, 3, h_crop, w_crop), torch.float32)
        T.call("emrt_tta_crop_windows_u8", Fn.P(scene), Fn.P(batch), ptr, len(chunk), kptr, G, H, W, h_crop, w_crop, *mean, *stdinv, c.stream)
        logits = model(batch)[0]
        assert logits.dtype == torch.float32 and logits.is_contiguous() and tuple(logits.shape) == (len(chunk) * G, ncls, h_crop, w_crop)
        T.call("emrt_tta_window_accumulate", Fn.P(logits), Fn.P(final), Fn.P(count), ptr, len(chunk), kptr, G, ncls, H, W, h_crop, w_crop, c.stream)


# Scale as one more axis of that augmentation: at scale s a window of the crop is resampled from a FOOTPRINT of crop / s native
# pixels where it is cropped, and its logits are resampled back where they are accumulated (include/emrt_hip_mstta.h).
TTA_SCALE_RANGE = (0.25, 4.0)
MAX_EDGE = 2048           # include/emrt_hip_mstta.h EMRT_MST_MAX_EDGE: footprint and window edges of one launch


def footprint(crop, stride, s):
    """-> ((fw, fh), (sw, sh)): the native pixels a crop-sized window covers at scale s, f = int(c / s + 0.5) per axis, and the stride its
    footprints are laid out with, min(f, max(1, int(t / s + 0.5))): size and stride scale together.  At s = 1 these are crop and stride."""
    s = float(s)
    size = tuple(int(c / s + 0.5) for c in crop)
    for c, f in zip(crop, size):
        if not (1 <= f <= MAX_EDGE and 1 <= c <= MAX_EDGE and f <= 4 * c and c <= 4 * f):
            raise ValueError("scale %g turns a crop edge of %d into a footprint of %d pixels: both must be 1..%d and within 4 times of each other"
                             % (s, c, f, MAX_EDGE))
    return size, tuple(min(f, max(1, int(t / s + 0.5))) for f, t in zip(size, stride))


def check_tta_scales(tta_scales, scales):
    """-> None, or the scales as a tuple of floats in the order given; an empty or non-sequence value, a scale outside [0.25, 4], a repeated
    scale and the combination with `scales` (the reference's multi-scale pass) are refused"""
    if tta_scales is None:
        return None
    if isinstance(tta_scales, (str, bytes)) or not hasattr(tta_scales, "__len__") or not hasattr(tta_scales, "__iter__") or len(tta_scales) == 0:
        raise ValueError("tta_scales must be a non-empty sequence of scales, got %r" % (tta_scales,))
    try:
        out = tuple(float(s) for s in tta_scales)
    except (TypeError, ValueError):
        raise ValueError("tta_scales must be a non-empty sequence of scales, got %r" % (tta_scales,))
    for s in out:
        if not TTA_SCALE_RANGE[0] <= s <= TTA_SCALE_RANGE[1]:          # (a NaN fails this too)
            raise ValueError("tta_scales must lie in [%g, %g], got %r" % (TTA_SCALE_RANGE + (s,)))
    if len(set(out)) != len(out):
        raise ValueError("tta_scales repeats a scale: %r" % (out,))
    if scales is not None:
        raise ValueError("tta_scales cannot be combined with scales: the reference's multi-scale pass resizes the whole scene itself")
    return out


def refuse_scales_with_config(args, config):
    """For the command lines: VAL.MULTI_SCALES_VAL is known only once the yaml is read, and --tta_scales is refused with it as with
    --multi_scales: a message on stderr and exit status 2, as argparse refuses."""
    if getattr(args, "tta_scales", None) is not None and config.VAL.MULTI_SCALES_VAL:
        import sys
        sys.stderr.write("error: --tta_scales cannot be combined with VAL.MULTI_SCALES_VAL of the config: choose the window-level scales or the "
                         "reference's whole-scene pass\n")
        raise SystemExit(2)


def footprint_grids(H, W, crop, stride, tta_scales, what="scene"):
    """-> [(s, fh, fw, [(y, x)])] in the order of tta_scales: per scale the footprint and the origins of infer.window_grid over footprints, in
    its order.  A scene smaller than a footprint is refused (nothing is padded), before anything is launched for any scale."""
    grids = []
    for s in tta_scales:
        (fw, fh), fstride = footprint(crop, stride, s)
        if H < fh or W < fw:
            raise ValueError("%s %dx%d (h x w) is smaller than the %dx%d footprint of the %dx%d crop at scale %g: nothing is resized or padded"
                             % (what, H, W, fh, fw, crop[1], crop[0], s))
        grids.append((s, fh, fw, [(a, b) for (a, b, _, _) in infer.window_grid(H, W, (fw, fh), fstride)]))
    return grids


def accumulate_windows_ms(model, scene, H, W, crop, stride, ncls, max_batch, mean, stdinv, final, count, codes, tta_scales, what="scene"):
    """accumulate_windows_tta with scale as one more axis: the scales in the order given, per scale the footprints of footprint_grids in grid
    order, max_batch // G per model call, each with its G = len(codes) variants.  emrt_mst_crop_windows_u8 resamples the windows from the uint8
    scene, emrt_mst_window_accumulate resamples every variant's logits back to the footprint, turned back, and adds their softmax to `final`
    [1, ncls, H, W] and G per covering footprint to `count` [1, 1, H, W]: the mean class probability over scales, footprints and variants."""
    grids = footprint_grids(H, W, crop, stride, tta_scales, what)
    M, c = _lib.mst_lib(), ctx()
    w_crop, h_crop = crop
    G = len(codes)
    karr = (ctypes.c_int * G)(*codes)
    kptr = ctypes.cast(karr, ctypes.c_void_p)
    per = max_batch // G
    for _s, fh, fw, org in grids:
        for i in range(0, len(org), per):
            chunk = org[i:i + per]
            _keep, ptr = _origins(chunk)
            batch = c.empty((len(chunk) * G, 3, h_crop, w_crop), torch.float32)
            M.call("emrt_mst_crop_windows_u8", Fn.P(scene), Fn.P(batch), ptr, len(chunk), kptr, G, H, W, fh, fw, h_crop, w_crop, *mean, *stdinv, c.stream)
            logits = model(batch)[0]
            assert logits.dtype == torch.float32 and logits.is_contiguous() and tuple(logits.shape) == (len(chunk) * G, ncls, h_crop, w_crop)
            M.call("emrt_mst_window_accumulate", Fn.P(logits), Fn.P(final), Fn.P(count), ptr, len(chunk), kptr, G, ncls, H, W, fh, fw, h_crop, w_crop,
                   c.stream)


def accumulate_windows(model, scene, H, W, crop, stride, ncls, max_batch, mean, stdinv, final, count, codes=(0,)):
    """The single-scale pass both classes share: the windows of infer.window_grid(H, W, crop, stride) in that order, max_batch per model call
    (chunked exactly as infer.slide_inference: the same logits, bit for bit), cropped and normalised from the uint8 scene, their logits added to
    `final` [1, ncls, H, W] and their hits to `count` [1, 1, H, W]; both fp32 and zeroed by the caller.  With more than one variant code
    (check_tta) the sums are those of accumulate_windows_tta instead: class probabilities, not logits."""
    L, c = Fn._L(), ctx()
    w_crop, h_crop = crop
    wins = infer.window_grid(H, W, crop, stride)
    if len(codes) > 1:
        return accumulate_windows_tta(model, scene, H, W, [(a, b) for (a, b, _, _) in wins], crop, ncls, max_batch, mean, stdinv, final, count, codes)
    for i in range(0, len(wins), max_batch):
        chunk = wins[i:i + max_batch]
        batch, ptr, _keep = crop_windows(scene, H, W, [(a, b) for (a, b, _, _) in chunk], h_crop, w_crop, mean, stdinv)
        logits = model(batch)[0]
        assert logits.dtype == torch.float32 and logits.is_contiguous()
        L.call("emrt_window_accumulate", Fn.P(logits), Fn.P(final), Fn.P(count), ptr, len(chunk), ncls, H, W, h_crop, w_crop, c.stream)


class ScenePredictor:
    """p = ScenePredictor(model, num_classes, crop_size, stride_size, palette, mean, std, overlay=None, max_batch=32, scales=None, tta="none")
    p(scene_u8)            torch.uint8 [H, W, 3] RGB on the device -> SceneResult
    p.predict_tiles(t_u8)  torch.uint8 [n, h, w, 3] with h x w == crop: one model call per max_batch tiles -> SceneResult with [n, ...] maps

    crop_size / stride_size are (w, h) as in the configs (VAL.CROP_SIZE, VAL.STRIDE_SIZE); palette uint8 [num_classes, 3] RGB; mean / std as
    transforms.Normalize takes them; overlay = alpha in [0, 1] (the colour's weight over the scene) or None; tta = a key of TTA_MODES: with
    G > 1 variants a model call carries max_batch // G windows; tta_scales = None or a sequence of scales in [0.25, 4] (check_tta_scales), with
    any tta, not with `scales` and not for predict_tiles."""

    def __init__(self, model, num_classes, crop_size, stride_size, palette, mean, std, overlay=None, max_batch=32, scales=None,
                 flip_horizontal=True, tta="none", tta_scales=None):
        self.model, self.ncls = model, int(num_classes)
        self.crop, self.stride = check_windows(crop_size, stride_size)
        pal = np.ascontiguousarray(np.asarray(palette))
        if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] != self.ncls:
            raise ValueError("palette must be uint8 [%d, 3] (one RGB colour per class), got %s %s" % (self.ncls, pal.dtype, pal.shape))
        if not 1 <= self.ncls <= 256:
            raise ValueError("num_classes must be 1..256 (the index map is uint8), got %d" % self.ncls)
        self._pal = (ctypes.c_ubyte * pal.size)(*pal.reshape(-1).tolist())
        self.mean, self.stdinv = check_normalise(mean, std)
        if overlay is not None and not 0.0 <= float(overlay) <= 1.0:
            raise ValueError("overlay alpha must be in [0, 1], got %r" % (overlay,))
        self.alpha = None if overlay is None else float(overlay)
        if not 1 <= int(max_batch) <= MAX_WINDOWS:
            raise ValueError("max_batch must be 1..%d, got %r" % (MAX_WINDOWS, max_batch))
        self.max_batch = int(max_batch)
        self.scales = None if scales is None else tuple(scales)
        self.flip_horizontal = flip_horizontal
        self.tta_scales = check_tta_scales(tta_scales, self.scales)
        self.tta, self.codes = tta, check_tta(tta, self.crop, self.max_batch, self.scales)

    # ---- kernels ---------------------------------------------------------------------------------------------------
    def _crop(self, scene, H, W, org, ch, cw):
        """windows at `org` of the uint8 [H, W, 3] scene -> normalised fp32 [n, 3, ch, cw]"""
        return crop_windows(scene, H, W, org, ch, cw, self.mean, self.stdinv)

    def _finish(self, values, count, scene, out, j0, N, H, W, tall=False):
        """values [N, ncls, H, W] (+ count) -> maps j0 .. j0 + N of `out`; the areas are added to out.areas.  tall: the N maps are one scene of
        N * H rows (values [1, ncls, N * H, W])"""
        overlay = None if out.overlay is None else out.overlay[j0:j0 + N]
        shape = (1, self.ncls, N * H, W) if tall else (N, self.ncls, H, W)
        Fn._L().call("emrt_scene_finish", Fn.P(values), Fn.P(count), ctypes.cast(self._pal, ctypes.c_void_p),
                     None if overlay is None else Fn.P(scene), 0.0 if self.alpha is None else self.alpha, Fn.P(out.index[j0:j0 + N]),
                     Fn.P(out.color[j0:j0 + N]), Fn.P(overlay), Fn.P(out.areas), *shape, ctx().stream)

    def _outputs(self, n, H, W):
        c = ctx()
        return SceneResult(c.empty((n, H, W), torch.uint8), c.empty((n, H, W, 3), torch.uint8),
                           None if self.alpha is None else c.empty((n, H, W, 3), torch.uint8), c.zeros((self.ncls,), torch.int64))

    @staticmethod
    def _check_u8(t, dims, what):
        if t.dtype != torch.uint8 or t.dim() != dims or t.shape[-1] != 3:
            raise ValueError("%s must be torch.uint8 %s RGB, got %s %s" % (what, "[H, W, 3]" if dims == 3 else "[n, h, w, 3]", t.dtype, tuple(t.shape)))
        return t.contiguous()

    # ---- one scene ---------------------------------------------------------------------------------------------------
    def __call__(self, scene_u8):
        scene = self._check_u8(scene_u8, 3, "scene")
        H, W = int(scene.shape[0]), int(scene.shape[1])
        w_crop, h_crop = self.crop
        if self.tta_scales is not None:
            footprint_grids(H, W, self.crop, self.stride, self.tta_scales)          # a scene smaller than a footprint is refused before anything is allocated
        elif H < h_crop or W < w_crop:
            raise ValueError("scene %dx%d (h x w) is smaller than the crop %dx%d: nothing is resized or padded" % (H, W, h_crop, w_crop))
        c = ctx()
        out = self._outputs(1, H, W)
        if self.tta_scales is not None:
            final = c.zeros((1, self.ncls, H, W), torch.float32)
            count = c.zeros((1, 1, H, W), torch.float32)
            accumulate_windows_ms(self.model, scene, H, W, self.crop, self.stride, self.ncls, self.max_batch, self.mean, self.stdinv, final, count,
                                  self.codes, self.tta_scales)
            self._finish(final, count, scene, out, 0, 1, H, W)
        elif self.scales is not None:
            img, _, _ = self._crop(scene, H, W, [(0, 0)], H, W)          # the whole scene as normalised fp32 CHW: one window
            final = infer.ms_accumulate(self.model, img[0], (H, W), True, None, self.stride, self.crop, self.ncls, scales=list(self.scales),
                                        flip_horizontal=self.flip_horizontal)
            self._finish(final, None, scene, out, 0, 1, H, W)
        else:
            final = c.zeros((1, self.ncls, H, W), torch.float32)
            count = c.zeros((1, 1, H, W), torch.float32)
            accumulate_windows(self.model, scene, H, W, self.crop, self.stride, self.ncls, self.max_batch, self.mean, self.stdinv, final, count,
                               self.codes)
            self._finish(final, count, scene, out, 0, 1, H, W)
        return SceneResult(out.index[0], out.color[0], None if out.overlay is None else out.overlay[0], out.areas)

    # ---- a stack of crop-sized tiles -----------------------------------------------------------------------------
    def predict_tiles(self, tiles_u8):
        """The stack is one tall scene [n * h][w][3] whose windows are the tiles; the model's logits are finished directly (a batch
        dimension, no count), max_batch tiles per model call, results in tile order.  With tta, max_batch // G tiles per model call are one tall
        scene of their own: its sums and counts (accumulate_windows_tta) are finished."""
        if self.tta_scales is not None:
            raise ValueError("predict_tiles does not take tta_scales: tiles are crop-sized, and the footprint of a scale below 1 does not fit in one")
        tiles = self._check_u8(tiles_u8, 4, "tiles")
        n, h, w = (int(v) for v in tiles.shape[:3])
        if (w, h) != self.crop:
            raise ValueError("tiles are %dx%d (h x w), the crop is %dx%d: predict_tiles takes crop-sized tiles" % (h, w, self.crop[1], self.crop[0]))
        out = self._outputs(n, h, w)
        if len(self.codes) > 1:
            c, per = ctx(), self.max_batch // len(self.codes)
            for j0 in range(0, n, per):
                m = min(per, n - j0)
                final = c.zeros((1, self.ncls, m * h, w), torch.float32)
                count = c.zeros((1, 1, m * h, w), torch.float32)
                accumulate_windows_tta(self.model, tiles[j0:j0 + m], m * h, w, [(j * h, 0) for j in range(m)], self.crop, self.ncls, self.max_batch,
                                       self.mean, self.stdinv, final, count, self.codes)
                self._finish(final, count, tiles[j0:j0 + m], out, j0, m, h, w, tall=True)
            return out
        for j0 in range(0, n, self.max_batch):
            m = min(self.max_batch, n - j0)
            batch, _, _keep = self._crop(tiles, n * h, w, [(j * h, 0) for j in range(j0, j0 + m)], h, w)
            logits = self.model(batch)[0]
            assert logits.dtype == torch.float32 and logits.is_contiguous() and tuple(logits.shape) == (m, self.ncls, h, w)
            self._finish(logits, None, tiles[j0:j0 + m], out, j0, m, h, w)
        return out


BOUNDARY_MAX_RADIUS = 32          # include/emrt_hip_bnd.h EMRT_BND_MAX_RADIUS
BOUNDARY_SHAPES = {"disk": 0, "square": 1}          # include/emrt_hip_bnd.h EMRT_BND_DISK / EMRT_BND_SQUARE


def check_boundary(boundary, shape):
    """-> (radius or None, shape code); a radius that is no integer in 1..32 and an unknown shape are refused here, before anything is loaded"""
    if shape not in BOUNDARY_SHAPES:
        raise ValueError("boundary_shape must be one of %s, got %r" % (", ".join(BOUNDARY_SHAPES), shape))
    if boundary is None:
        return None, BOUNDARY_SHAPES[shape]
    if isinstance(boundary, bool) or not isinstance(boundary, (int, np.integer)):
        raise ValueError("boundary must be an integer radius in pixels, got %r" % (boundary,))
    if not 1 <= int(boundary) <= BOUNDARY_MAX_RADIUS:
        raise ValueError("boundary must be a radius in 1..%d, got %r" % (BOUNDARY_MAX_RADIUS, boundary))
    return int(boundary), BOUNDARY_SHAPES[shape]


class SceneEvaluator:
    """ev = SceneEvaluator(model, bank, num_classes, crop_size, stride_size, mean, std, ignore_index=255, max_batch=32, scales=None, tta="none")
    tot = ev.evaluate(rank=0, nranks=1)     int64 [3, ncls] on the device: intersect, prediction and label areas of this rank's scenes
    ev.per_scene                            int64 [n_scenes, 3, ncls] on the device: the same per scene, rows of other ranks' scenes zero

    `bank` is a datasets.SceneBank whose label maps are stored as they are to be counted (a validation bank: shift_on_upload=True).  Scene i of
    range(rank, len(bank), nranks) is predicted at its own size from the bank's uint8 view -- accumulate_windows, emrt_window_normalise,
    emrt_argmax_nchw: the prediction of infer.ss_inference on the CPU-normalised scene, bit for bit (with `scales`: infer.ms_accumulate on the
    normalised scene and the argmax, infer.ms_inference's) -- and emrt_segmentation_areas counts it against the uint8 label view into the scene's
    row.  Everything is enqueued on the current stream: no host copy of a pixel, no synchronisation.  Sums, counts, normalised logits and the
    prediction are allocated once per distinct scene shape and reused by every scene of that shape and by every later evaluation.
    crop_size / stride_size are (w, h) as in the configs (VAL.CROP_SIZE, VAL.STRIDE_SIZE); mean / std as transforms.Normalize takes them; tta as
    ScenePredictor takes it (the argmax is then that of the mean class probability), and tta_scales likewise.

    boundary=r (1..32), boundary_shape "disk" or "square": after each scene's emrt_segmentation_areas, emrt_bnd_runs and emrt_bnd_band mark the band of
    the prediction and of the label map (include/emrt_hip_bnd.h; one runs map and two bands per scene shape, reused like the rest) and emrt_bnd_areas
    counts into
    ev.boundary_per_scene                   int64 [n_scenes, 2, 3, ncls]: [0] the three areas outside the label's band (the ISPRS eroded protocol),
                                            [1] those of Boundary IoU; zeroed by evaluate(), rows of other ranks' scenes zero
    ev.boundary_totals()                    its sum over the scenes, int64 [2, 3, ncls]
    evaluate() and per_scene are what they are without it: the launches only read the prediction."""

    def __init__(self, model, bank, num_classes, crop_size, stride_size, mean, std, ignore_index=255, max_batch=32, scales=None,
                 flip_horizontal=True, tta="none", tta_scales=None, boundary=None, boundary_shape="disk"):
        self.boundary, self.boundary_shape = check_boundary(boundary, boundary_shape)
        self.model, self.bank, self.ncls = model, bank, int(num_classes)
        self.crop, self.stride = check_windows(crop_size, stride_size)
        self.scales = None if scales is None else tuple(scales)
        self.tta_scales = check_tta_scales(tta_scales, self.scales)
        for i, (H, W) in enumerate(bank.sizes):
            if self.tta_scales is not None:
                footprint_grids(H, W, self.crop, self.stride, self.tta_scales, "scene %d (%s)" % (i, bank.names[i]))
            elif H < self.crop[1] or W < self.crop[0]:
                raise ValueError("scene %d (%s) is %dx%d (h x w), smaller than the crop %dx%d: nothing is resized or padded"
                                 % (i, bank.names[i], H, W, self.crop[1], self.crop[0]))
        if not 1 <= self.ncls <= 256:
            raise ValueError("num_classes must be 1..256 (the label maps are uint8), got %d" % self.ncls)
        if not 1 <= int(max_batch) <= MAX_WINDOWS:
            raise ValueError("max_batch must be 1..%d, got %r" % (MAX_WINDOWS, max_batch))
        self.max_batch = int(max_batch)
        self.mean, self.stdinv = check_normalise(mean, std)
        self.ignore_index = int(ignore_index)
        self.flip_horizontal = flip_horizontal
        self.tta, self.codes = tta, check_tta(tta, self.crop, self.max_batch, self.scales)
        self.per_scene = torch.empty((len(bank), 3, self.ncls), dtype=torch.int64, device=bank.device)
        self._scratch = {}          # (H, W) -> (sums, counts, normalised logits, prediction)
        self.boundary_per_scene = None
        if self.boundary is not None:
            self.boundary_per_scene = torch.empty((len(bank), 2, 3, self.ncls), dtype=torch.int64, device=bank.device)
        self._bnd_scratch = {}      # (H, W) -> (runs, the prediction's band, the label's band), uint8 [H, W] each

    def _boundary_buffers(self, H, W):
        if (H, W) not in self._bnd_scratch:
            self._bnd_scratch[(H, W)] = tuple(torch.empty((H, W), dtype=torch.uint8, device=self.bank.device) for _ in range(3))
        return self._bnd_scratch[(H, W)]

    def _count_boundary(self, i, pred, label):
        """The bands of scene i's prediction (int32) and label map (uint8, where it lies in the bank) and the counts of both protocols: five
        launches on the current stream.  The runs map is shared: the stream orders the prediction's column pass before the label's row pass."""
        B, c = _lib.bnd_lib(), ctx()
        H, W = self.bank.sizes[i]
        run, band_pred, band_label = self._boundary_buffers(H, W)
        for m, kind, band in ((pred, 0, band_pred), (label, 2, band_label)):
            B.call("emrt_bnd_runs", Fn.P(m), kind, H, W, self.boundary, Fn.P(run), c.stream)
            B.call("emrt_bnd_band", Fn.P(m), kind, Fn.P(run), H, W, self.boundary, self.boundary_shape, Fn.P(band), c.stream)
        B.call("emrt_bnd_areas", Fn.P(pred), Fn.P(label), Fn.P(band_pred), Fn.P(band_label), H * W, self.ncls, self.ignore_index,
               Fn.P(self.boundary_per_scene[i]), c.stream)

    def boundary_totals(self):
        """int64 [2, 3, ncls]: boundary_per_scene summed over this rank's scenes"""
        if self.boundary is None:
            raise ValueError("this SceneEvaluator was made without boundary=: there are no boundary counts")
        return self.boundary_per_scene.sum(0)

    def _buffers(self, H, W):
        if (H, W) not in self._scratch:
            dev, single = self.bank.device, self.scales is None
            self._scratch[(H, W)] = (torch.empty((1, self.ncls, H, W), dtype=torch.float32, device=dev) if single else None,
                                     torch.empty((1, 1, H, W), dtype=torch.float32, device=dev) if single else None,
                                     torch.empty((1, self.ncls, H, W), dtype=torch.float32, device=dev) if single else None,
                                     torch.empty((1, 1, H, W), dtype=torch.int32, device=dev))
        return self._scratch[(H, W)]

    def predict(self, i):
        """Scene i -> its int32 [1, 1, H, W] prediction in the scratch of its shape (overwritten by the next scene of that shape)."""
        L, c = Fn._L(), ctx()
        scene, _ = self.bank.scene(i)
        H, W = self.bank.sizes[i]
        final, count, logits, pred = self._buffers(H, W)
        if self.scales is not None:
            img, _, _keep = crop_windows(scene, H, W, [(0, 0)], H, W, self.mean, self.stdinv)          # the whole scene as normalised fp32 CHW: one window
            logits = infer.ms_accumulate(self.model, img[0], (H, W), True, None, self.stride, self.crop, self.ncls, scales=list(self.scales),
                                         flip_horizontal=self.flip_horizontal)
        else:
            L.call("emrt_memset", Fn.P(final), 0, final.numel() * 4, c.stream)
            L.call("emrt_memset", Fn.P(count), 0, count.numel() * 4, c.stream)
            if self.tta_scales is not None:
                accumulate_windows_ms(self.model, scene, H, W, self.crop, self.stride, self.ncls, self.max_batch, self.mean, self.stdinv, final, count,
                                      self.codes, self.tta_scales, "scene %d (%s)" % (i, self.bank.names[i]))
            else:
                accumulate_windows(self.model, scene, H, W, self.crop, self.stride, self.ncls, self.max_batch, self.mean, self.stdinv, final, count,
                                   self.codes)
            L.call("emrt_window_normalise", Fn.P(final), Fn.P(count), Fn.P(logits), self.ncls, H, W, c.stream)
        L.call("emrt_argmax_nchw", Fn.P(logits), Fn.P(pred), 1, self.ncls, H, W, c.stream)
        return pred

    def evaluate(self, rank=0, nranks=1):
        L, c = Fn._L(), ctx()
        self.model.eval()
        L.call("emrt_memset", Fn.P(self.per_scene), 0, self.per_scene.numel() * 8, c.stream)
        if self.boundary is not None:
            L.call("emrt_memset", Fn.P(self.boundary_per_scene), 0, self.boundary_per_scene.numel() * 8, c.stream)
        for i in range(rank, len(self.bank), nranks):
            pred = self.predict(i)
            _, label = self.bank.scene(i)
            L.call("emrt_segmentation_areas", Fn.P(pred), Fn.P(label), 2, pred.numel(), self.ncls, self.ignore_index, Fn.P(self.per_scene[i]), c.stream)
            if self.boundary is not None:
                self._count_boundary(i, pred, label)
        return self.per_scene.sum(0)
