"""Whole-scene prediction: a uint8 RGB scene of any size -> class indices, colour mask, overlay and per-class areas, all on the device
(DESIGN.md 16).  What the reference's predict.py does with one window per model call, a host argmax and a per-class colouring loop in numpy:

    crop + normalise windows from the uint8 scene   emrt_scene_crop_windows_u8 (transforms.Normalize's arithmetic, bit for bit)
    model                                           one call per `max_batch` windows, in infer.window_grid order: slide_inference's logits
    accumulate sums and hit counts                  emrt_window_accumulate
    finish                                          emrt_scene_finish: divide, argmax, palette, overlay, areas in one pass over the sums

Nothing is resized: a scene is predicted at its own resolution with the configured crop and stride.  With `scales`, the softmax sums of
infer.ms_accumulate (multi-scale + horizontal flip) are finished instead.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import infer
from ... import functional as Fn
from ...runtime import ctx

MAX_WINDOWS = 64          # csrc/common.hpp EMRT_MAX_WINDOWS: origins of one launch

# index uint8 [H, W], color uint8 [H, W, 3], overlay uint8 [H, W, 3] or None, areas int64 [ncls] (pixels per class); predict_tiles adds a
# leading tile dimension to the first three
SceneResult = namedtuple("SceneResult", "index color overlay areas")


def _origins(org):
    arr = (ctypes.c_int * (2 * len(org)))(*[v for yx in org for v in yx])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


class ScenePredictor:
    """p = ScenePredictor(model, num_classes, crop_size, stride_size, palette, mean, std, overlay=None, max_batch=32, scales=None)
    p(scene_u8)            torch.uint8 [H, W, 3] RGB on the device -> SceneResult
    p.predict_tiles(t_u8)  torch.uint8 [n, h, w, 3] with h x w == crop: one model call per max_batch tiles -> SceneResult with [n, ...] maps

    crop_size / stride_size are (w, h) as in the configs (VAL.CROP_SIZE, VAL.STRIDE_SIZE); palette uint8 [num_classes, 3] RGB; mean / std as
    transforms.Normalize takes them; overlay = alpha in [0, 1] (the colour's weight over the scene) or None."""

    def __init__(self, model, num_classes, crop_size, stride_size, palette, mean, std, overlay=None, max_batch=32, scales=None,
                 flip_horizontal=True):
        self.model, self.ncls = model, int(num_classes)
        self.crop, self.stride = tuple(int(v) for v in crop_size), tuple(int(v) for v in stride_size)
        if len(self.crop) != 2 or len(self.stride) != 2 or min(self.crop + self.stride) < 1:
            raise ValueError("crop_size and stride_size are positive (w, h) pairs, got %r and %r" % (crop_size, stride_size))
        if self.stride[0] > self.crop[0] or self.stride[1] > self.crop[1]:
            raise ValueError("stride %r is larger than the crop %r: the windows would leave uncovered stripes (NaN logits in the reference)"
                             % (self.stride, self.crop))
        pal = np.ascontiguousarray(np.asarray(palette))
        if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] != self.ncls:
            raise ValueError("palette must be uint8 [%d, 3] (one RGB colour per class), got %s %s" % (self.ncls, pal.dtype, pal.shape))
        if not 1 <= self.ncls <= 256:
            raise ValueError("num_classes must be 1..256 (the index map is uint8), got %d" % self.ncls)
        self._pal = (ctypes.c_ubyte * pal.size)(*pal.reshape(-1).tolist())
        if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
            raise ValueError("mean / std need 3 channels and a non-zero std, got %r / %r" % (mean, std))
        self.mean = [float(v) for v in np.asarray(mean, dtype=np.float64)]
        self.stdinv = [float(v) for v in 1.0 / np.asarray(std, dtype=np.float64)]          # as Normalize computes it
        if overlay is not None and not 0.0 <= float(overlay) <= 1.0:
            raise ValueError("overlay alpha must be in [0, 1], got %r" % (overlay,))
        self.alpha = None if overlay is None else float(overlay)
        if not 1 <= int(max_batch) <= MAX_WINDOWS:
            raise ValueError("max_batch must be 1..%d, got %r" % (MAX_WINDOWS, max_batch))
        self.max_batch = int(max_batch)
        self.scales = None if scales is None else tuple(scales)
        self.flip_horizontal = flip_horizontal

    # ---- kernels ---------------------------------------------------------------------------------------------------
    def _crop(self, scene, H, W, org, ch, cw):
        """windows at `org` of the uint8 [H, W, 3] scene -> normalised fp32 [n, 3, ch, cw]"""
        c = ctx()
        arr, ptr = _origins(org)
        batch = c.empty((len(org), 3, ch, cw), torch.float32)
        Fn._L().call("emrt_scene_crop_windows_u8", Fn.P(scene), Fn.P(batch), ptr, len(org), H, W, ch, cw, *self.mean, *self.stdinv, c.stream)
        return batch, ptr, arr

    def _finish(self, values, count, scene, out, j0, N, H, W):
        """values [N, ncls, H, W] (+ count) -> maps j0 .. j0 + N of `out`; the areas are added to out.areas"""
        overlay = None if out.overlay is None else out.overlay[j0:j0 + N]
        Fn._L().call("emrt_scene_finish", Fn.P(values), Fn.P(count), ctypes.cast(self._pal, ctypes.c_void_p),
                     None if overlay is None else Fn.P(scene), 0.0 if self.alpha is None else self.alpha, Fn.P(out.index[j0:j0 + N]),
                     Fn.P(out.color[j0:j0 + N]), Fn.P(overlay), Fn.P(out.areas), N, self.ncls, H, W, ctx().stream)

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
        if H < h_crop or W < w_crop:
            raise ValueError("scene %dx%d (h x w) is smaller than the crop %dx%d: nothing is resized or padded" % (H, W, h_crop, w_crop))
        L, c = Fn._L(), ctx()
        out = self._outputs(1, H, W)
        if self.scales is not None:
            img, _, _ = self._crop(scene, H, W, [(0, 0)], H, W)          # the whole scene as normalised fp32 CHW: one window
            final = infer.ms_accumulate(self.model, img[0], (H, W), True, None, self.stride, self.crop, self.ncls, scales=list(self.scales),
                                        flip_horizontal=self.flip_horizontal)
            self._finish(final, None, scene, out, 0, 1, H, W)
        else:
            wins = infer.window_grid(H, W, self.crop, self.stride)
            final = c.zeros((1, self.ncls, H, W), torch.float32)
            count = c.zeros((1, 1, H, W), torch.float32)
            for i in range(0, len(wins), self.max_batch):          # chunked exactly as infer.slide_inference: the same logits, bit for bit
                chunk = wins[i:i + self.max_batch]
                batch, ptr, _keep = self._crop(scene, H, W, [(a, b) for (a, b, _, _) in chunk], h_crop, w_crop)
                logits = self.model(batch)[0]
                assert logits.dtype == torch.float32 and logits.is_contiguous()
                L.call("emrt_window_accumulate", Fn.P(logits), Fn.P(final), Fn.P(count), ptr, len(chunk), self.ncls, H, W, h_crop, w_crop, c.stream)
            self._finish(final, count, scene, out, 0, 1, H, W)
        return SceneResult(out.index[0], out.color[0], None if out.overlay is None else out.overlay[0], out.areas)

    # ---- a stack of crop-sized tiles -----------------------------------------------------------------------------
    def predict_tiles(self, tiles_u8):
        """The stack is one tall scene [n * h][w][3] whose windows are the tiles; the model's logits are finished directly (a batch
        dimension, no count), max_batch tiles per model call, results in tile order."""
        tiles = self._check_u8(tiles_u8, 4, "tiles")
        n, h, w = (int(v) for v in tiles.shape[:3])
        if (w, h) != self.crop:
            raise ValueError("tiles are %dx%d (h x w), the crop is %dx%d: predict_tiles takes crop-sized tiles" % (h, w, self.crop[1], self.crop[0]))
        out = self._outputs(n, h, w)
        for j0 in range(0, n, self.max_batch):
            m = min(self.max_batch, n - j0)
            batch, _, _keep = self._crop(tiles, n * h, w, [(j * h, 0) for j in range(j0, j0 + m)], h, w)
            logits = self.model(batch)[0]
            assert logits.dtype == torch.float32 and logits.is_contiguous() and tuple(logits.shape) == (m, self.ncls, h, w)
            self._finish(logits, None, tiles[j0:j0 + m], out, j0, m, h, w)
        return out
