"""Class palettes and PNG writers of `python -m emrt_amd.predict` (reference: src/utils/vis.py, predict.py; PIL instead of cv2).

The palettes are the colour codings the datasets publish, written as the RGB a viewer shows: the reference lists them in BGR and writes
them with cv2, whose imwrite takes BGR, so its files hold these same RGB values."""
import numpy as np
from PIL import Image

_ISPRS = [(255, 255, 255), (0, 0, 255), (0, 255, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0)]      # surfaces, building, low vegetation, tree, car, clutter
_PALETTES = {
    "Potsdam": _ISPRS,
    "Vaihingen": _ISPRS,
    "LoveDA": [(255, 255, 255), (255, 0, 0), (255, 255, 0), (0, 0, 255), (159, 129, 183), (0, 255, 0), (255, 195, 128)],
}


def get_palette(dataset_name):
    """-> uint8 [ncls, 3] RGB of DATA.DATASET's classes"""
    if dataset_name not in _PALETTES:
        raise ValueError("no palette for dataset %r (known: %s)" % (dataset_name, ", ".join(sorted(_PALETTES))))
    return np.array(_PALETTES[dataset_name], dtype=np.uint8)


def save_color_png(path, rgb):
    """uint8 [H, W, 3] RGB -> an RGB PNG (the colour mask, the overlay)"""
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("save_color_png takes uint8 [H, W, 3], got %s %s" % (rgb.dtype, rgb.shape))
    Image.fromarray(rgb, "RGB").save(path, format="PNG")


def save_index_png(path, index, palette):
    """uint8 [H, W] class indices -> an 8-bit palette PNG (mode P): the pixel values ARE the indices, the embedded palette shows them in the
    dataset's colours"""
    index, palette = np.ascontiguousarray(index), np.asarray(palette)
    if index.dtype != np.uint8 or index.ndim != 2:
        raise ValueError("save_index_png takes uint8 [H, W], got %s %s" % (index.dtype, index.shape))
    if palette.dtype != np.uint8 or palette.ndim != 2 or palette.shape[1] != 3 or palette.shape[0] > 256:
        raise ValueError("palette must be uint8 [ncls <= 256, 3], got %s %s" % (palette.dtype, palette.shape))
    im = Image.fromarray(index, "P")
    im.putpalette(palette.reshape(-1).tolist())
    im.save(path, format="PNG")
