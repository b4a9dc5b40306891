"""A small seeded scene tree for `train.py --data scenes` (emrt_amd.src.datasets.SceneBank):
    <root>/images/<n>.tif + <root>/labels/<n>.png ; with --val N also <root>/val_images/<n>.tif + <root>/val_labels/<n>.png

    python tools/make_fake_scenes.py [root] [--scenes 4] [--size 512 | --size 600x800] [--val 0] [--seed 0] [--learnable] [--rare-share 0.01 [--rare-class 5] [--rare-blob 32]]

Images are uint8 RGB, label maps uint8 class indices 0..5 with 1.5 % of the pixels set to 255 (ignore), as the *_convert_labels trees hold them.
default: uniform noise (plumbing and timing: nothing to learn).  --learnable: the scenes of tools/make_fake_potsdam.py, at scene size.
--rare-share S (noise scenes): class --rare-class covers about the share S of the pixels (e.g. 0.01) as --rare-blob x --rare-blob squares at random
places (overlaps make it slightly less) and the other five classes share the rest as noise, so the effect of DATA.SCENE_SAMPLING.MODE "class" can be
seen without a dataset: objects, not salt -- a window around a pixel of per-pixel noise holds no more of its class than any other window.  Without
the option the output is what it always was, byte for byte."""
import argparse
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("root", nargs="?", default="fake_scenes")
    p.add_argument("--scenes", type=int, default=4)
    p.add_argument("--size", default="512", help="S or HxW")
    p.add_argument("--val", type=int, default=0, help="validation scenes under val_images/ + val_labels/")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--learnable", action="store_true")
    p.add_argument("--rare-share", type=float, default=0.0, help="noise scenes: the share of the pixels painted as --rare-class (0: off)")
    p.add_argument("--rare-class", type=int, default=5)
    p.add_argument("--rare-blob", type=int, default=32, help="side of the squares the rare class is painted in")
    a = p.parse_args(argv)
    H, W = (int(v) for v in a.size.split("x")) if "x" in a.size else (int(a.size),) * 2
    if not 0.0 <= a.rare_share < 1.0 or not 0 <= a.rare_class <= 5 or (a.rare_share and a.learnable) or not 1 <= a.rare_blob <= min(H, W):
        raise SystemExit("--rare-share is a share in [0, 1) of a noise scene (not --learnable), --rare-class one of 0..5, --rare-blob at most the scene's side")
    rng = np.random.RandomState(a.seed)
    for img_dir, lab_dir, n in (("images", "labels", a.scenes), ("val_images", "val_labels", a.val)):
        if n <= 0:
            continue
        os.makedirs(os.path.join(a.root, img_dir), exist_ok=True)
        os.makedirs(os.path.join(a.root, lab_dir), exist_ok=True)
        for i in range(n):
            if a.learnable:
                if H != W:
                    raise SystemExit("--learnable draws square scenes; got %dx%d" % (H, W))
                from make_fake_potsdam import learnable_tile
                img, lab = learnable_tile(rng, H)
            else:
                img = rng.randint(0, 256, (H, W, 3), dtype=np.uint8)
                lab = rng.randint(0, 6, (H, W), dtype=np.uint8)
                if a.rare_share:
                    others = np.asarray([c for c in range(6) if c != a.rare_class], dtype=np.uint8)
                    lab = others[rng.randint(0, 5, (H, W))]
                    side = a.rare_blob
                    for _ in range(max(1, int(round(a.rare_share * H * W / (side * side))))):
                        y, x = rng.randint(0, H - side + 1), rng.randint(0, W - side + 1)
                        lab[y:y + side, x:x + side] = a.rare_class
                lab[rng.rand(H, W) < 0.015] = 255
            Image.fromarray(img).save(os.path.join(a.root, img_dir, "%d.tif" % i))
            Image.fromarray(lab).save(os.path.join(a.root, lab_dir, "%d.png" % i))
    print("[make_fake_scenes] %d scenes of %dx%d (+ %d validation) under %s" % (a.scenes, H, W, max(a.val, 0), a.root))


if __name__ == "__main__":
    main()
