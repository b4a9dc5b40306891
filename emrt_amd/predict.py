"""Prediction entry point (reference: semantic_segmentation/predict.py): colour maps of whole scenes.

    python -m emrt_amd.predict --config <yaml> --model_path <best_model.pdparams> [--input scene.tif dir/ ...] [--overlay 0.5] [--save_index]

Every image is predicted at its own resolution by the sliding window of VAL.CROP_SIZE / VAL.STRIDE_SIZE (nothing is resized; for the shipped
configs, whose tiles are cut to the crop size, that is what the reference computes).  The uint8 scene goes to the device once; windows are
cropped and normalised there, and one kernel turns the accumulated logits into the class index, the colour mask, the overlay and the per-class
areas (src/api/scene.py), so what comes back to the host is bytes.  PNGs are encoded by a few writer threads while the next scene runs.
"""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from .config import get_config, update_config
from .runtime import BF16, F16, F32
from .src.api.scene import TTA_MODES, ScenePredictor, check_tta_scales, refuse_scales_with_config
from .src.models import get_model
from .src.utils import vis

WRITERS = 4          # most PNG encoder threads


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="EMRT (MI355X HIP path) prediction: colour maps of whole scenes")
    p.add_argument("--config", dest="cfg", type=str,
                   default=os.path.join(os.path.dirname(__file__), "configs/EMRT/EMRT_256x256_160k_potsdam.yaml"))
    p.add_argument("--model_path", default=None, type=str, help="a .pdparams file or a checkpoint written by emrt_amd.train")
    p.add_argument("--multi_scales", action="store_true", help="multi-scale (VAL.SCALE_RATIOS) + horizontal-flip inference, infer.py:160-260")
    p.add_argument("--input", nargs="+", default=None, metavar="PATH",
                   help="image files and / or directories (read sorted, not recursively); default: the test split of DATA.DATASET under DATA.DATA_PATH")
    p.add_argument("--save_dir", default=None, help="default: <SAVE_DIR>/predict")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "fp16"])
    p.add_argument("--max_batch", default=32, type=int, help="windows per model call (1..64)")
    p.add_argument("--tta", default="none", choices=list(TTA_MODES),
                   help="test-time augmentation of every window at scale 1: hflip = 2 variants, flips = both flips and their product (4), "
                        "d4 = the 8 flips and quarter turns (square crop); the class probabilities of all variants are averaged. "
                        "A model call then carries max_batch // variants windows. Not with --multi_scales, which keeps its own flip")
    p.add_argument("--tta_scales", default=None, type=float, nargs="+", metavar="S",
                   help="window-level scales in [0.25, 4], e.g. 0.75 1.0 1.25, with any --tta: at scale S a window is resampled from CROP / S scene "
                        "pixels and its logits are resampled back; the class probabilities of all scales and variants are averaged. "
                        "Not with --multi_scales / VAL.MULTI_SCALES_VAL, the reference's whole-scene multi-scale pass")
    p.add_argument("--overlay", default=None, type=float, metavar="ALPHA",
                   help="also write <stem>_overlay.png = ALPHA * colour + (1 - ALPHA) * image, ALPHA in [0, 1]")
    p.add_argument("--save_index", action="store_true",
                   help="also write <stem>_index.png, an 8-bit palette PNG whose pixel values are the class indices. "
                        "Outputs are named after the source file's stem (<stem>.png is the colour mask), not after a running counter as in the reference")
    args = p.parse_args(argv)
    if args.tta != "none" and args.multi_scales:
        p.error("--tta %s cannot be combined with --multi_scales: multi-scale inference keeps its own horizontal flip" % args.tta)
    if args.tta_scales is not None:
        if args.multi_scales:
            p.error("--tta_scales cannot be combined with --multi_scales: choose the window-level scales or the reference's whole-scene pass")
        try:
            check_tta_scales(args.tta_scales, None)
        except ValueError as e:
            p.error("--tta_scales: %s" % e)
    return args


def input_files(paths):
    """--input: files as given, directories expanded to their files (sorted, not recursive)"""
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += [os.path.join(p, f) for f in sorted(os.listdir(p)) if os.path.isfile(os.path.join(p, f))]
        elif os.path.isfile(p):
            out.append(p)
        else:
            raise ValueError("--input: %s is neither a file nor a directory" % p)
    return out


def _write(save_dir, stem, palette, index, color, overlay):
    """One image's PNGs (a writer thread)."""
    paths = [os.path.join(save_dir, stem + ".png")]
    vis.save_color_png(paths[0], color)
    if overlay is not None:
        paths.append(os.path.join(save_dir, stem + "_overlay.png"))
        vis.save_color_png(paths[-1], overlay)
    if index is not None:
        paths.append(os.path.join(save_dir, stem + "_index.png"))
        vis.save_index_png(paths[-1], index, palette)
    return paths


def main(argv=None):
    args = parse_args(argv)
    config = update_config(get_config(), args)
    refuse_scales_with_config(args, config)
    palette = vis.get_palette(config.DATA.DATASET)
    ncls = config.DATA.NUM_CLASSES
    if args.input:
        files = input_files(args.input)
    else:
        from .src import datasets
        files = datasets.test_images(config)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    twice = sorted({s for s in stems if stems.count(s) > 1})
    if twice:
        raise ValueError("outputs are named after the source file's stem, and these stems occur more than once: %s" % ", ".join(twice))
    save_dir = args.save_dir or os.path.join(config.SAVE_DIR, "predict")
    os.makedirs(save_dir, exist_ok=True)

    model = get_model(config)
    if args.model_path:
        from .src.utils.checkpoint import load_entire_model
        load_entire_model(model, args.model_path)
    model.to_hip("cuda:0", {"bf16": BF16, "fp16": F16, "fp32": F32}[args.dtype])
    if args.dtype == "fp16":
        model.compute_aux_in_eval = False      # the auxiliary head is computed and thrown away in eval (paddle_EMRT.py:300-302, infer.py:66)
    model.eval()
    crop, stride = list(config.VAL.CROP_SIZE), list(config.VAL.STRIDE_SIZE)
    if stride == [320, 320] and crop[0] < 320:
        stride = crop          # the default stride left in place over a smaller crop, as emrt_amd.val treats it
    multi = args.multi_scales or config.VAL.MULTI_SCALES_VAL
    predictor = ScenePredictor(model, ncls, crop, stride, palette, list(config.VAL.MEAN), list(config.VAL.STD), overlay=args.overlay,
                               max_batch=args.max_batch, scales=list(config.VAL.SCALE_RATIOS) if multi else None, tta=args.tta,
                               tta_scales=args.tta_scales)
    written, jobs = [], []
    with ThreadPoolExecutor(max_workers=max(1, min(WRITERS, len(files)))) as pool:
        for f, stem in zip(files, stems):
            scene = torch.from_numpy(np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8).copy()).to("cuda:0")
            res = predictor(scene)
            areas = res.areas.cpu().numpy()          # (synchronises: the maps below are complete)
            jobs.append(pool.submit(_write, save_dir, stem, palette, res.index.cpu().numpy() if args.save_index else None, res.color.cpu().numpy(),
                                    None if res.overlay is None else res.overlay.cpu().numpy()))
            share = areas / max(1, int(areas.sum()))
            print("[PREDICT] {} {}x{}  class share: {}".format(os.path.basename(f), scene.shape[0], scene.shape[1],
                                                                " ".join("%d:%.4f" % (k, s) for k, s in enumerate(share))), flush=True)
        for j in jobs:
            written += j.result()          # (a writer's exception surfaces here)
    print("[PREDICT] Images: {}  files written: {}  -> {}".format(len(files), len(written), save_dir))
    return written


if __name__ == "__main__":
    main()
