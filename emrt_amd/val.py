"""Evaluation entry point (reference: semantic_segmentation/val.py:34-231, val_in_train.py:19-125).

    python -m emrt_amd.val --config <yaml> --model_path <iter_N_state.pt> [--data tiles.npz]
    python -m emrt_amd.val --config <yaml> --model_path <...> --data scenes [--data_path ROOT]

Single-scale sliding-window inference (src/api/infer.py) over a set of tiles, per-image area accumulation, one
all-reduce of the [3, ncls] int64 areas at the end when WORLD_SIZE > 1 (the reference all-gathers three tensors per
image, val.py:164-170), then mIoU / Acc / Kappa / per-class F1 exactly as val.py:197-209 prints them.

--data scenes evaluates the whole scenes of <DATA.DATA_PATH>/val_images + /val_labels at their own resolution: they are uploaded once as uint8
(datasets.SceneBank) and api.scene.SceneEvaluator cuts, normalises, predicts and counts them on the device; one more line per scene.  With --boundary R it also prints the ISPRS
metrics on ground truth whose class boundaries are eroded by R pixels and Boundary IoU at that distance.
"""
import argparse
import os
import time

import numpy as np
import torch

from .config import get_config, update_config
from .distributed import init_process_group
from .runtime import BF16, F16, F32
from .src.api import infer
from .src.api.scene import BOUNDARY_SHAPES, TTA_MODES, check_boundary, check_tta_scales, refuse_scales_with_config
from .src.models import get_model
from .src.utils import metrics


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="EMRT (MI355X HIP path) evaluation")
    p.add_argument("--config", dest="cfg", type=str,
                   default=os.path.join(os.path.dirname(__file__), "configs/EMRT/EMRT_256x256_160k_potsdam.yaml"))
    p.add_argument("--model_path", default=None, type=str)
    p.add_argument("--multi_scales", action="store_true", help="multi-scale (VAL.SCALE_RATIOS) + horizontal-flip inference, infer.py:160-260")
    p.add_argument("--data", default="synthetic", help="'synthetic', 'dataset' (DATA.DATASET under DATA.DATA_PATH), 'scenes' (the whole scenes of "
                   "DATA.DATA_PATH/val_images + /val_labels, resident on the GPU and evaluated at their own resolution) or a .npz")
    p.add_argument("--data_path", default=None, help="override DATA.DATA_PATH of the yaml")
    p.add_argument("--dtype", default="fp32", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--tta", default="none", choices=list(TTA_MODES),
                   help="with --data scenes: test-time augmentation of every window at scale 1 (hflip: 2 variants, flips: 4, d4: the 8 flips and "
                        "quarter turns of a square crop); the class probabilities of all variants are averaged. Not with --multi_scales")
    p.add_argument("--tta_scales", default=None, type=float, nargs="+", metavar="S",
                   help="with --data scenes: window-level scales in [0.25, 4], e.g. 0.75 1.0 1.25, with any --tta (DESIGN.md 23); the class "
                        "probabilities of all scales and variants are averaged. Not with --multi_scales / VAL.MULTI_SCALES_VAL")
    p.add_argument("--boundary", default=None, type=int, metavar="R",
                   help="with --data scenes: also report the metrics on ground truth whose class boundaries are eroded by R pixels (the ISPRS protocol "
                        "uses a disk of 3) and Boundary IoU at distance R; 1..32 (DESIGN.md 25)")
    p.add_argument("--boundary_shape", default="disk", choices=list(BOUNDARY_SHAPES),
                   help="the structuring element of --boundary: a disk (ISPRS) or a square (Chebyshev distance: R erosions by 3x3, as the Boundary IoU "
                        "reference code)")
    args = p.parse_args(argv)
    if args.boundary is not None:
        if args.data != "scenes":
            p.error("--boundary needs --data scenes: only whole scenes resident on the GPU are evaluated at their boundaries, --data %s is not" % args.data)
        try:
            check_boundary(args.boundary, args.boundary_shape)
        except ValueError as e:
            p.error("--boundary: %s" % e)
    elif args.boundary_shape != "disk":
        p.error("--boundary_shape needs --boundary")
    if args.tta_scales is not None:
        if args.data != "scenes":
            p.error("--tta_scales needs --data scenes: only whole scenes resident on the GPU are evaluated with test-time augmentation, --data %s is not"
                    % args.data)
        if args.multi_scales:
            p.error("--tta_scales cannot be combined with --multi_scales: choose the window-level scales or the reference's whole-scene pass")
        try:
            check_tta_scales(args.tta_scales, None)
        except ValueError as e:
            p.error("--tta_scales: %s" % e)
    if args.tta != "none" and args.data != "scenes":
        p.error("--tta %s needs --data scenes: only whole scenes resident on the GPU are evaluated with test-time augmentation, --data %s is not"
                % (args.tta, args.data))
    if args.tta != "none" and args.multi_scales:
        p.error("--tta %s cannot be combined with --multi_scales: multi-scale inference keeps its own horizontal flip" % args.tta)
    return args


class _OnDevice:
    """Sequence view: element i moved to the device when it is indexed (no-op for device tensors)."""

    def __init__(self, seq, dev):
        self.seq, self.dev = seq, dev

    def __len__(self):
        return len(self.seq)

    def __getitem__(self, i):
        return self.seq[i].to(self.dev, non_blocking=True)


class ValTiles:
    """Lazy validation set over a dataset object: item i is decoded when indexed (and kept on the HOST, pinned when possible, for
    the next evaluation), so a rank only ever decodes its own shard.  `which` = 0 -> image fp32 [3,h,w], 1 -> label int64 [h,w]."""

    def __init__(self, dataset, which, cache=None):
        self.ds, self.which = dataset, which
        self.cache = {} if cache is None else cache

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        if i not in self.cache:
            a, b = self.ds[i]
            img = torch.from_numpy(np.ascontiguousarray(a)).float()
            lab = torch.from_numpy(np.ascontiguousarray(b[0])).long()
            try:
                img, lab = img.pin_memory(), lab.pin_memory()
            except RuntimeError:        # no pinned allocator (CPU-only host): pageable memory works too
                pass
            self.cache[i] = (img, lab)
        return self.cache[i][self.which]


def evaluate(model, images, labels, config, rank=0, nranks=1, multi_scales=False):
    """images: sequence of fp32 [3,h,w] tensors, labels: sequence of int64 [h,w], on the host or on the device (a lazy sequence
    such as ValTiles decodes on access).  Only this rank's shard (rank, rank + nranks, ...) is ever touched, and a host image is
    moved to the device when its turn comes -- as the reference streams them through a DataLoader (val.py:95-104) -- instead of
    the whole validation set living in HBM next to the training graph's pools.  Returns the reference's metric tuple."""
    from .runtime import ctx
    model.eval()
    ncls = config.DATA.NUM_CLASSES
    dev = ctx().device
    tot = torch.zeros(3, ncls, dtype=torch.int64, device=dev)
    t0 = time.time()
    images, labels = _OnDevice(images, dev), _OnDevice(labels, dev)
    for i in range(rank, len(images), nranks):
        img, lab = images[i], labels[i]          # ONE host-to-device copy each per evaluation (indexing _OnDevice copies)
        if multi_scales:            # val.py:168-181: VAL.SCALE_RATIOS + horizontal flip
            pred = infer.ms_inference(model, [img], lab.shape[-2:], True, config.VAL.IMAGE_BASE_SIZE, config.VAL.STRIDE_SIZE,
                                      config.VAL.CROP_SIZE, ncls, scales=list(config.VAL.SCALE_RATIOS), flip_horizontal=True,
                                      flip_vertical=False, rescale_from_ori=config.VAL.RESCALE_FROM_ORI)
        else:
            pred = infer.ss_inference(model, [img], [lab.shape[-2:]], True, config.VAL.IMAGE_BASE_SIZE, config.VAL.STRIDE_SIZE,
                                      config.VAL.CROP_SIZE, ncls, config.VAL.RESCALE_FROM_ORI)[0]
        inter, pa, la = metrics.calculate_area(pred, lab, ncls, config.TRAIN.IGNORE_INDEX)
        tot[0] += inter
        tot[1] += pa
        tot[2] += la
    if nranks > 1:
        torch.distributed.all_reduce(tot)
    return (time.time() - t0,) + metric_tuple(tot)


def metric_tuple(tot):
    """int64 [3, ncls] intersect / prediction / label areas (after the all-reduce, if any) -> (mIoU, Acc, kappa, class IoU, class Acc, class F1,
    mean F1): what evaluate() returns after its time."""
    class_iou, miou = metrics.mean_iou(tot[0], tot[1], tot[2])
    acc, class_acc, class_rec = metrics.accuracy(tot[0], tot[1], tot[2])
    kap = metrics.kappa(tot[0], tot[1], tot[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        class_f1 = np.nan_to_num(2 * class_acc * class_rec / (class_acc + class_rec))
    return miou, acc, kap, class_iou, class_acc, class_f1, float(np.mean(class_f1))


def scene_evaluator(model, config, device, multi_scales=False, max_batch=32, tta="none", tta_scales=None, boundary=None, boundary_shape="disk"):
    """The validation bank of a scene tree (<DATA.DATA_PATH>/val_images + /val_labels, uploaded here, labels stored as a `val` Dataset shifts them)
    and the SceneEvaluator over it, from VAL.CROP_SIZE / STRIDE_SIZE / MEAN / STD and TRAIN.IGNORE_INDEX; VAL.SCALE_RATIOS when multi_scales; tta as
    SceneEvaluator takes it, and tta_scales, boundary and boundary_shape likewise."""
    from .src.api.scene import SceneEvaluator
    from .src.datasets import SceneBank
    bank = SceneBank(config.DATA.DATA_PATH, device, label_shift=1 if config.DATA.DATASET == "LoveDA" else 0, sub=("val_images", "val_labels"),
                     shift_on_upload=True)
    return SceneEvaluator(model, bank, config.DATA.NUM_CLASSES, config.VAL.CROP_SIZE, config.VAL.STRIDE_SIZE, list(config.VAL.MEAN), list(config.VAL.STD),
                          ignore_index=config.TRAIN.IGNORE_INDEX, max_batch=max_batch, scales=list(config.VAL.SCALE_RATIOS) if multi_scales else None, tta=tta,
                          tta_scales=tta_scales, boundary=boundary, boundary_shape=boundary_shape)


def evaluate_scenes(evaluator, rank=0, nranks=1):
    """evaluate() over a SceneEvaluator: this rank's scenes, one all-reduce of the areas when nranks > 1, the same tuple."""
    t0 = time.time()
    tot = evaluator.evaluate(rank, nranks)
    if nranks > 1:
        torch.distributed.all_reduce(tot)
    return (time.time() - t0,) + metric_tuple(tot)


def scene_lines(evaluator, nranks=1):
    """One line per scene, "name  mIoU  Acc", from evaluator.per_scene in ONE device-to-host copy (the rows of the other ranks' scenes are summed in
    first when nranks > 1: every row belongs to one rank, the others hold zeros there)."""
    per = evaluator.per_scene
    if nranks > 1:
        per = per.clone()
        torch.distributed.all_reduce(per)
    per = per.cpu()
    lines = []
    for name, (H, W), a in zip(evaluator.bank.names, evaluator.bank.sizes, per):
        with np.errstate(divide="ignore", invalid="ignore"):
            miou, acc = metrics.mean_iou(a[0], a[1], a[2])[1], metrics.accuracy(a[0], a[1], a[2])[0]
        lines.append("[EVAL] Scene {} ({}x{}): mIoU: {:.4f}  Acc: {:.4f}".format(name, H, W, miou, acc))
    return lines


def boundary_lines(evaluator, nranks=1):
    """The four lines of --boundary from evaluator.boundary_totals() (one more all-reduce when nranks > 1): the ISPRS metrics over the pixels
    outside the label's band with their class F1 scores, and mean Boundary IoU with its class values."""
    tot = evaluator.boundary_totals()
    if nranks > 1:
        torch.distributed.all_reduce(tot)
    tot = tot.cpu()
    what = "%s r=%d" % ([k for k, v in BOUNDARY_SHAPES.items() if v == evaluator.boundary_shape][0], evaluator.boundary)
    miou, acc, _, _, _, cf1, mf1 = metric_tuple(tot[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        cbiou, mbiou = metrics.mean_iou(tot[1][0], tot[1][1], tot[1][2])
    return ["[EVAL] Eroded ({}): mIoU: {:.4f}  Acc: {:.4f}  mF1: {:.4f}".format(what, miou, acc, mf1),
            "[EVAL] Eroded Class F1-score: " + str(np.round(cf1, 4)),
            "[EVAL] Boundary ({}): mBIoU: {:.4f}".format(what, mbiou),
            "[EVAL] Boundary Class BIoU: " + str(np.round(cbiou, 4))]


def main(argv=None):
    args = parse_args(argv)
    config = update_config(get_config(), args)
    refuse_scales_with_config(args, config)
    rank, local_rank, nranks = init_process_group()
    model = get_model(config)
    if args.model_path:                 # a .pdparams written by the reference / by train.py, or a torch checkpoint
        from .src.utils.checkpoint import load_entire_model
        load_entire_model(model, args.model_path)
    model.to_hip("cuda:%d" % local_rank, {"bf16": BF16, "fp16": F16, "fp32": F32}[args.dtype])
    if args.dtype == "fp16":
        model.compute_aux_in_eval = False      # the auxiliary head is computed and thrown away in eval (paddle_EMRT.py:300-302, infer.py:66)
    dev = torch.device("cuda", local_rank)
    if list(config.VAL.STRIDE_SIZE) == [320, 320] and list(config.VAL.CROP_SIZE)[0] < 320:
        config.VAL.STRIDE_SIZE = list(config.VAL.CROP_SIZE)   # default stride > crop leaves NaN stripes
    multi_scales = args.multi_scales or config.VAL.MULTI_SCALES_VAL
    ev = None
    if args.data == "scenes":           # whole validation scenes resident on the device, evaluated at their own resolution
        if getattr(args, "data_path", None):
            config.DATA.DATA_PATH = args.data_path
        ev = scene_evaluator(model, config, dev, multi_scales, tta=args.tta, tta_scales=args.tta_scales, boundary=args.boundary,
                             boundary_shape=args.boundary_shape)
        images = ev.bank.names
        if rank == 0:
            print("[EVAL] data: %d validation scenes resident on the GPU (%.1f MB)" % (len(ev.bank), ev.bank.nbytes / 1e6), flush=True)
    elif args.data == "synthetic":
        g = torch.Generator().manual_seed(0)
        h = w = config.VAL.IMAGE_BASE_SIZE or config.DATA.CROP_SIZE[0]
        images = [torch.randn(3, h, w, generator=g).to(dev) for _ in range(8)]
        labels = [torch.randint(0, config.DATA.NUM_CLASSES, (h, w), generator=g).to(dev) for _ in range(8)]
    elif args.data == "dataset":        # the reference's pipeline (val.py:95-104): DATA.DATASET under DATA.DATA_PATH, mode 'val'
        from .src.datasets import get_dataset
        from .src.transforms import get_val_transforms
        if getattr(args, "data_path", None):
            config.DATA.DATA_PATH = args.data_path
        ds = get_dataset(config, data_transform=get_val_transforms(config), mode="val")
        cache = {}
        images, labels = ValTiles(ds, 0, cache), ValTiles(ds, 1, cache)
    else:
        z = np.load(args.data)
        images = [torch.from_numpy(a).float().to(dev) for a in z["images"]]
        labels = [torch.from_numpy(a).long().to(dev) for a in z["labels"]]
    if ev is not None:
        cost, miou, acc, kap, ciou, cacc, cf1, mf1 = evaluate_scenes(ev, rank, nranks)
        lines = scene_lines(ev, nranks)
        if args.boundary is not None:
            lines += boundary_lines(ev, nranks)
    else:
        cost, miou, acc, kap, ciou, cacc, cf1, mf1 = evaluate(model, images, labels, config, rank, nranks, multi_scales=multi_scales)
        lines = []
    if rank == 0:
        print("[EVAL] Images: {}  mIoU: {:.4f}  Acc: {:.4f}  Kappa: {:.4f}  mF1: {:.4f}".format(len(images), miou, acc, kap, mf1))
        print("[EVAL] Class IoU: " + str(np.round(ciou, 4)))
        print("[EVAL] Class Acc: " + str(np.round(cacc, 4)))
        print("[EVAL] Class F1-score: " + str(np.round(cf1, 4)))
        for line in lines:
            print(line)
    return miou


if __name__ == "__main__":
    main()
