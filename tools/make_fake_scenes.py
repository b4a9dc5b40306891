"""A small seeded scene tree for `train.py --data scenes` (emrt_amd.src.datasets.SceneBank):
    <root>/images/<n>.tif + <root>/labels/<n>.png ; with --val N also <root>/val_images/<n>.tif + <root>/val_labels/<n>.png

    python tools/make_fake_scenes.py [root] [--scenes 4] [--size 512 | --size 600x800] [--val 0] [--seed 0] [--learnable]

Images are uint8 RGB, label maps uint8 class indices 0..5 with 1.5 % of the pixels set to 255 (ignore), as the *_convert_labels trees hold them.
default: uniform noise (plumbing and timing: nothing to learn).  --learnable: the scenes of tools/make_fake_potsdam.py, at scene size."""
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
    a = p.parse_args(argv)
    H, W = (int(v) for v in a.size.split("x")) if "x" in a.size else (int(a.size),) * 2
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
                lab[rng.rand(H, W) < 0.015] = 255
            Image.fromarray(img).save(os.path.join(a.root, img_dir, "%d.tif" % i))
            Image.fromarray(lab).save(os.path.join(a.root, lab_dir, "%d.png" % i))
    print("[make_fake_scenes] %d scenes of %dx%d (+ %d validation) under %s" % (a.scenes, H, W, max(a.val, 0), a.root))


if __name__ == "__main__":
    main()
