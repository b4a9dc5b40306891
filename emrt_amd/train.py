"""Training entry point with the reference's CLI and step order (semantic_segmentation/train.py:26-266).

    python -m emrt_amd.train --config emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam.yaml [--seed 1234]
    python -m emrt_amd.train --gpus 8 --config ...          # starts the 8 rank processes itself (one per GPU, RCCL)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m emrt_amd.train --config ...

Per iteration (train.py:141-159): forward -> MixSoftmaxCrossEntropyLoss -> backward (+ RCCL gradient all-reduce when
WORLD_SIZE > 1) -> Momentum step with global-norm clip -> poly LR step -> clear grads; every LOGGING_INFO_FREQ
iterations rank 0 prints the reference's log line (:177-181); every SAVE_FREQ_CHECKPOINT iterations a checkpoint
(model + optimizer state + iteration, so training can actually be resumed -- the reference never wired that, :103).
The dataset pipeline (cv2 / Potsdam readers) is outside this path: tiles come from --data synthetic (default: seeded
random tiles of DATA.CROP_SIZE, resident on the device) or from an .npz of pre-cut tiles (--data file.npz with arrays
`images` [N,3,H,W] float32 normalised and `labels` [N,H,W] int64).  --data dataset reads the reference's directory layout;
--device_transforms then runs its training transforms on the GPU (DeviceTileLoader) instead of in the reader threads.
--data scenes uploads the whole scenes of <DATA.DATA_PATH>/images + /labels once (SceneBank) and cuts every training tile out of device memory
inside the captured step (SceneSampler): no reader threads, no per-step copy; periodic evaluation reads <root>/val_images + /val_labels.
--eval_scenes native (with --data scenes) uploads those validation scenes once as well and evaluates them at their own resolution on the device
(api.scene.SceneEvaluator) instead of resizing each to VAL.IMAGE_BASE_SIZE on the host.
"""
import argparse
import os
import time
from collections import deque

import numpy as np
import torch

from .config import get_config, update_config
from .distributed import DistributedTileSampler, init_process_group
from .engine import TrainEngine
from .runtime import BF16, F32
from .src.models import get_model
from .src.models.losses import get_loss_function
from .src.models.solver import get_optimizer, get_scheduler


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="EMRT (MI355X HIP path) training")
    p.add_argument("--config", "--cfg", dest="cfg", type=str,
                   default=os.path.join(os.path.dirname(__file__), "configs/EMRT/EMRT_256x256_160k_potsdam.yaml"), help="The config file.")
    p.add_argument("--seed", dest="seed", default=1234, type=int, help="Set the random seed during training.")
    p.add_argument("--data", default="synthetic", help="'synthetic', 'dataset' (DATA.DATASET under DATA.DATA_PATH, the reference's "
                   "directory layout), 'scenes' (whole scenes under DATA.DATA_PATH/images + /labels, resident on the GPU; tiles are cut "
                   "there at random positions) or a .npz of pre-cut tiles")
    p.add_argument("--data_path", default=None, help="override DATA.DATA_PATH of the yaml")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--iters", type=int, default=None, help="override TRAIN.ITERS.  Under WarmupPolyLR a value at or below LR_SCHEDULER.WARM_UP_STEPS also shortens the "
                   "warmup to a quarter of it (none at all for 1 to 3), with a log line; the schedule follows the --iters of the run at hand, so resume with "
                   "the --iters the checkpoint was trained with to continue the same schedule")
    p.add_argument("--no-graph", action="store_true", help="launch kernels eagerly instead of replaying a captured hipGraph")
    p.add_argument("--resume", default=None, help="checkpoint written by this script")
    p.add_argument("--save_dir", default=None, help="override SAVE_DIR of the yaml (the reference's yamls point at the authors' disks)")
    p.add_argument("--pretrained_backbone", default=None, help="weights to start from (.pdparams or torch): whole model or ResNet backbone")
    p.add_argument("--no-eval", action="store_true", help="skip the periodic evaluation (train.py:187-195) and best_model.pdparams")
    p.add_argument("--gpus", type=int, default=0, help="without a launcher (no RANK / WORLD_SIZE in the environment): start this many rank "
                   "processes, one per GPU (the reference gets its ranks from paddle.distributed.launch, train.py:116-123)")
    p.add_argument("--device_transforms", action="store_true", help="--data dataset only: reader threads just decode tiles; the "
                   "training transforms run as one HIP kernel per batch on the GPU (DeviceTileLoader)")
    p.add_argument("--eval_scenes", default="resized", choices=["resized", "native"], help="--data scenes only: how the periodic evaluation sees the "
                   "validation scenes.  'resized': decoded on the host and resized to VAL.IMAGE_BASE_SIZE (the tile chain of get_val_transforms); "
                   "'native': resident on the GPU as uint8 and evaluated at their own resolution with VAL.CROP_SIZE / VAL.STRIDE_SIZE windows")
    p.add_argument("--val_tiles", type=int, default=16, help="--data synthetic / .npz without val arrays: how many held-out tiles to evaluate on")
    return p.parse_args(argv)


def shorten_warmup(config, iters, verbose=True):
    """--iters N at or below the yaml's WARM_UP_STEPS leaves WarmupPolyLR without a decay phase, and it refuses that (max_iters must exceed
    warmup_steps): the warmup then shrinks with the run, to a quarter of it, with a log line.  The other schedules accept any --iters and are left alone.
    For --iters 1 to 3 the quarter is 0: no warmup.  The shortened value is not stored in a checkpoint: a --resume rebuilds the schedule from the yaml and ITS
    --iters, so a different --iters gives a different warmup under the restored step counter."""
    sch = config.TRAIN.LR_SCHEDULER
    if sch.NAME != "WarmupPolyLR" or sch.WARM_UP_STEPS < iters:
        return False
    new = iters // 4
    if verbose:
        print("[train] --iters %d is not more than LR_SCHEDULER.WARM_UP_STEPS %d: warming up over %d steps instead" % (iters, sch.WARM_UP_STEPS, new), flush=True)
    sch.WARM_UP_STEPS = new
    return True


class _Steps:
    """Stands where the tile sampler stands in the training loop when the batches are drawn on the device (--data scenes): `n` steps per epoch."""

    def __init__(self, n):
        self.n = n

    def set_epoch(self, epoch):
        pass

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter([None] * self.n)


class TimeAverager:  # utils/timer.py:17-40
    def __init__(self):
        self.reset()

    def reset(self):
        self._cnt, self._total_time, self._total_samples = 0, 0.0, 0

    def record(self, usetime, num_samples=None):
        self._cnt += 1
        self._total_time += usetime
        if num_samples:
            self._total_samples += num_samples

    def get_average(self):
        return 0 if self._cnt == 0 else self._total_time / float(self._cnt)

    def get_ips_average(self):
        return 0 if not self._total_samples or self._cnt == 0 else float(self._total_samples) / self._total_time


def calculate_eta(remaining_step, speed):  # utils/timer.py:43-51
    remaining_time = int(max(remaining_step, 0) * speed)
    h, r = divmod(remaining_time, 3600)
    m, s = divmod(r, 60)
    return "{:0>2}:{:0>2}:{:0>2}".format(h, m, s)


def synthetic_tiles(n, crop, ncls, seed, device):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(n, 3, crop[1], crop[0], generator=g)
    labels = torch.randint(0, ncls, (n, crop[1], crop[0]), generator=g)
    labels[torch.rand(n, crop[1], crop[0], generator=g) < 0.02] = 255
    return images.to(device), labels.to(device)


def main(argv=None):
    args = parse_args(argv)
    if args.device_transforms and args.data == "scenes":
        raise SystemExit("[train] --device_transforms cannot be combined with --data scenes: it augments the decoded tiles of --data dataset; "
                         "--data scenes already runs the transforms on the GPU, on tiles cut from the resident scenes")
    if args.device_transforms and args.data != "dataset":
        raise SystemExit("[train] --device_transforms needs --data dataset (it augments decoded tiles; --data %s has none)" % args.data)
    if args.eval_scenes == "native" and args.data != "scenes":
        raise SystemExit("[train] --eval_scenes native needs --data scenes (it evaluates the scene tree's val_images/ + val_labels/; --data %s has none)" % args.data)
    if args.eval_scenes == "native" and args.no_eval:
        raise SystemExit("[train] --eval_scenes native cannot be combined with --no-eval: there is no evaluation to run on the scenes")
    launched = "WORLD_SIZE" in os.environ or "RANK" in os.environ
    if args.gpus > 1 and not launched:          # pure parent: no GPU call in this process, N fresh rank processes
        import sys
        from .distributed import spawn_ranks
        codes, _ = spawn_ranks(args.gpus, [sys.executable, "-m", "emrt_amd.train"] + list(sys.argv[1:] if argv is None else argv))
        raise SystemExit(1 if any(codes) else 0)
    if args.gpus and launched and int(os.environ.get("WORLD_SIZE", 1)) != args.gpus:
        raise SystemExit("[train] WORLD_SIZE=%s but --gpus %d" % (os.environ.get("WORLD_SIZE"), args.gpus))
    if os.environ.get("EMRT_ALL_RANKS_ON_GPU0"):      # test aid (with EMRT_DIST_BACKEND=gloo): every rank on device 0
        os.environ["LOCAL_RANK"] = "0"
    config = update_config(get_config(), args)
    if config.DATA.SCENE_SAMPLING.MODE not in ("uniform", "class"):
        raise SystemExit("[train] DATA.SCENE_SAMPLING.MODE must be 'uniform' or 'class', got %r" % (config.DATA.SCENE_SAMPLING.MODE,))
    if config.DATA.SCENE_SAMPLING.MODE == "class" and args.data != "scenes":
        raise SystemExit("[train] DATA.SCENE_SAMPLING.MODE 'class' needs --data scenes (the classes are drawn from the label maps of the resident "
                         "scenes; --data %s has none)" % args.data)
    try:          # said at start-up, before a process group or a model exists: DATA.AUGMENT.ROT90_PROB needs a square DATA.CROP_SIZE
        from .src.transforms import check_rot90
        check_rot90(config)
    except ValueError as e:
        raise SystemExit("[train] %s" % e)
    rank, local_rank, nranks = init_process_group()
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    if args.save_dir:
        config.SAVE_DIR = args.save_dir
    if args.data_path:
        config.DATA.DATA_PATH = args.data_path
    if args.data == "scenes" and not args.no_eval:      # said at start-up, not at the first checkpoint
        root = config.DATA.DATA_PATH
        if not (os.path.isdir(os.path.join(root, "val_images")) and os.path.isdir(os.path.join(root, "val_labels"))):
            raise SystemExit("[train] --data scenes: %s has no val_images/ and val_labels/ for the periodic evaluation; add them or pass --no-eval" % root)
    model = get_model(config)
    if config.MODEL.PRETRAINED:
        # MODEL.PRETRAINED / --pretrained_backbone (config.py:245-246): a whole-model file (.pdparams or torch) or an ImageNet
        # ResNet file as paddle.vision saves it (keys without the "backbone." prefix; detected from the key names)
        from .src.utils.checkpoint import load_pretrained_model, load_pdparams
        path = config.MODEL.PRETRAINED
        if path.endswith(".pdparams"):
            keys = load_pdparams(path).keys()
        else:       # a checkpoint of this script ({"model": state, ...}) or a bare torch state dict
            ck = torch.load(path, map_location="cpu")
            keys = ck.get("model", ck).keys()
        prefix = "" if any(k.startswith("backbone.") or k.startswith("model.") for k in keys) else "backbone."
        load_pretrained_model(model, path, prefix=prefix)
    model.to_hip("cuda:%d" % local_rank, BF16 if args.dtype == "bf16" else F32, seed=args.seed + rank)   # per-rank dropout streams
    model.train()
    iters = args.iters or config.TRAIN.ITERS
    if args.iters:
        config.TRAIN.ITERS = iters
        shorten_warmup(config, iters, verbose=rank == 0)
    lr_scheduler = get_scheduler(config)
    optimizer = get_optimizer(model, lr_scheduler, config)
    loss_func = get_loss_function(config)
    bs = config.DATA.BATCH_SIZE
    dev = torch.device("cuda", local_rank)
    loader = source = None
    if args.data == "scenes":           # whole scenes resident in device memory; every batch is cut and augmented inside the step
        from .src.datasets import SceneBank, SceneSampler
        from .src.transforms import get_transforms
        root = config.DATA.DATA_PATH
        tile = (config.DATA.CROP_SIZE[1], config.DATA.CROP_SIZE[0])        # CROP_SIZE is (w, h)
        bank = SceneBank(root, dev, label_shift=1 if config.DATA.DATASET == "LoveDA" else 0)
        source = SceneSampler(bank, get_transforms(config), bs, args.seed, rank, tile=tile, sampling=config.DATA.SCENE_SAMPLING,
                              num_classes=config.DATA.NUM_CLASSES)
        n_tiles = None
        if rank == 0:
            print("[train] data: %d scenes resident on the GPU (%.1f MB), %d tile origins, %d scale steps; tiles are drawn and cut on the device" % (
                len(bank), bank.nbytes / 1e6, source.total_origins, len(source.scales)), flush=True)
            if source.class_mode:
                print("[train] data: class-aware sampling, %.0f %% of the tiles are cut around a pixel of a drawn class (label index built in %.2f ms)" % (
                    100.0 * source.class_prob, source.index.build_ms), flush=True)
                for name, share, prob in source.class_table:
                    print("[train] data:   %-12s pixel share %8.4f %%   sampling probability %8.4f %%" % (name, 100.0 * share, 100.0 * prob), flush=True)
    elif args.data == "synthetic":
        images, labels = synthetic_tiles(max(4 * bs * nranks, 64), config.DATA.CROP_SIZE, config.DATA.NUM_CLASSES, args.seed, dev)
        n_tiles = images.shape[0]
    elif args.data == "dataset":        # the reference's pipeline: DATA.DATASET under DATA.DATA_PATH (train.py:79-86)
        from .src.datasets import get_dataset, DeviceTileLoader, TileLoader
        from .src.transforms import get_transforms
        dataset_train = get_dataset(config, data_transform=get_transforms(config), mode="train")
        n_tiles = len(dataset_train)
    else:
        z = np.load(args.data)
        images, labels = torch.from_numpy(z["images"]).float().to(dev), torch.from_numpy(z["labels"]).long().to(dev)
        n_tiles = images.shape[0]
    if source is not None:              # an "epoch" of the log line: as many tiles as the scenes hold side by side
        sampler = _Steps(max(1, -(-source.total_origins // (tile[0] * tile[1] * bs * nranks))))
    else:
        sampler = DistributedTileSampler(n_tiles, bs, rank, nranks, shuffle=True, drop_last=True, seed=args.seed)
    if args.data == "dataset":
        import copy
        workers = max(1, config.DATA.NUM_WORKERS)
        if args.device_transforms:
            loader = DeviceTileLoader(dataset_train, copy.copy(sampler), dev, workers=workers, prefetch=4).epochs()
            if rank == 0:
                print("[train] data: DeviceTileLoader, %d reader threads, transforms on the GPU" % workers, flush=True)
        else:
            loader = TileLoader(dataset_train, copy.copy(sampler), dev, workers=workers, prefetch=4).epochs()
    start_iter = 0
    if args.resume:
        ck = torch.load(args.resume, map_location="cpu")
        model.load_state_dict(ck["model"])
        optimizer.set_state_dict(ck["optimizer"])
        start_iter = ck["iter"]
    engine = TrainEngine(model, optimizer, loss_func, nranks, use_graph=not args.no_graph, batch_source=source)
    if rank == 0:
        # the shipped yamls carry the reference authors' own disks as SAVE_DIR: a run that cannot checkpoint must say so
        # at once, not after 160k iterations (train.py:197-220 writes there unconditionally)
        try:
            os.makedirs(config.SAVE_DIR, exist_ok=True)
            if not os.access(config.SAVE_DIR, os.W_OK):
                raise PermissionError(config.SAVE_DIR)
        except OSError as e:
            fallback = os.path.abspath(os.path.join("output", os.path.basename(os.path.normpath(config.SAVE_DIR)) or "emrt"))
            print("[WARNING] SAVE_DIR {!r} cannot be created or written ({}); checkpoints go to {!r} instead "
                  "(pass --save_dir to choose)".format(config.SAVE_DIR, e, fallback), flush=True)
            os.makedirs(fallback, exist_ok=True)        # failing here is fatal: no silent run without checkpoints
            config.SAVE_DIR = fallback
        print("train_cfg: {}\ntrain_model_name: {}\ntrain_datatset: {}".format(args.cfg, config.MODEL.NAME, config.DATA.DATASET))
    # ---- validation set for the periodic evaluation (train.py:88-100, 187-195; val_in_train.py:19-125) ---------------------
    val_images = val_labels = scene_eval = None
    if not args.no_eval:
        if args.eval_scenes == "native":
            pass                    # the evaluator is built below, once the stride is settled
        elif args.data in ("dataset", "scenes"):
            from .src.transforms import get_val_transforms
            if args.data == "scenes":
                from .src.datasets import SceneVal
                ds_val = SceneVal(get_val_transforms(config), config.DATA.DATA_PATH, config.DATA.NUM_CLASSES, bank.label_shift)
            else:
                ds_val = get_dataset(config, data_transform=get_val_transforms(config), mode="val")
            from .val import ValTiles       # decoded lazily, this rank's shard only, kept on the host between evaluations
            cache = {}
            val_images, val_labels = ValTiles(ds_val, 0, cache), ValTiles(ds_val, 1, cache)
        elif args.data != "synthetic" and "val_images" in z.files:
            val_images = [torch.from_numpy(a).float().to(dev) for a in z["val_images"]]
            val_labels = [torch.from_numpy(a).long().to(dev) for a in z["val_labels"]]
        else:       # held-out seeded tiles (synthetic) / the first tiles of the file
            vi, vl = (synthetic_tiles(args.val_tiles, config.DATA.CROP_SIZE, config.DATA.NUM_CLASSES, args.seed + 7919, dev)
                      if args.data == "synthetic" else (images[:args.val_tiles], labels[:args.val_tiles]))
            val_images, val_labels = list(vi), list(vl)
        if list(config.VAL.STRIDE_SIZE) == [320, 320] and list(config.VAL.CROP_SIZE)[0] < 320:
            config.VAL.STRIDE_SIZE = list(config.VAL.CROP_SIZE)   # the default stride > crop leaves NaN stripes
        if args.eval_scenes == "native":        # the validation scenes uploaded once, beside the training bank
            from .val import scene_evaluator
            scene_eval = scene_evaluator(model, config, dev)
            val_images = scene_eval.bank.names
            if rank == 0:
                print("[train] eval: %d validation scenes resident on the GPU (%.1f MB), evaluated at their own resolution" % (
                    len(scene_eval.bank), scene_eval.bank.nbytes / 1e6), flush=True)
    best_mean_iou, best_acc, best_model_iter = -1.0, -1.0, -1
    iters_per_epoch = max(len(sampler), 1)
    total_epoch = iters // iters_per_epoch
    reader_cost, batch_cost = TimeAverager(), TimeAverager()
    save_models = deque()
    avg_loss, cur_iter, epoch = 0.0, start_iter, 0
    batch_start = time.time()
    pending = []
    while cur_iter < iters:
        sampler.set_epoch(epoch)
        epoch += 1
        for idx in sampler:
            if cur_iter >= iters:
                break
            cur_iter += 1
            reader_cost.record(time.time() - batch_start)
            lr = optimizer.get_lr()
            if source is not None:
                loss_t = engine.step()      # the batch is drawn and cut inside the step
            else:
                if loader is not None:
                    bx, by = next(loader)       # decoded / augmented by the reader threads, already on the device
                else:
                    ib = torch.as_tensor(idx, device=dev)
                    bx, by = images[ib], labels[ib]
                loss_t = engine.step(bx, by)
            pending.append(loss_t.clone())          # no device->host sync per step (the reference syncs here, :160)
            batch_cost.record(time.time() - batch_start, num_samples=bs)
            if cur_iter % config.LOGGING_INFO_FREQ == 0:
                avg_loss = float(torch.stack(pending).mean().item())
                pending = []
                if rank == 0:
                    print("[TRAIN] Epochs: {}/{}, iter: {}/{}, loss: {:.4f}, lr: {:.8f}, batch_cost: {:.4f}, reader_cost: {:.5f}, ips: {:.4f} samples/sec | ETA {}".format(
                        (cur_iter - 1) // iters_per_epoch + 1, total_epoch + 1, cur_iter, iters, avg_loss, lr, batch_cost.get_average(),
                        reader_cost.get_average(), batch_cost.get_ips_average() * nranks, calculate_eta(iters - cur_iter, batch_cost.get_average())), flush=True)
                reader_cost.reset()
                batch_cost.reset()
            checkpoint_now = cur_iter % config.SAVE_FREQ_CHECKPOINT == 0 or cur_iter == iters
            mean_iou = None
            if checkpoint_now and val_images is not None:       # every rank takes part (train.py:187-195)
                from .val import evaluate, evaluate_scenes, scene_lines
                if scene_eval is not None:
                    val_time_cost, mean_iou, acc, kap, class_iou, class_acc, class_f1, mean_f1 = evaluate_scenes(scene_eval, rank, nranks)
                    lines = scene_lines(scene_eval, nranks)
                else:
                    val_time_cost, mean_iou, acc, kap, class_iou, class_acc, class_f1, mean_f1 = evaluate(model, val_images, val_labels, config, rank, nranks)
                    lines = []
                if rank == 0:
                    for line in lines:
                        print(line)
                    print("Val_time_cost:   {}".format(val_time_cost))
                    print("In this val: mIoU {:.4f},  Acc: {:.4f}, F1-Score:{:.4f}".format(mean_iou, acc, mean_f1))
                    print("Current best_mIoU: {:.4f},  Acc: {:.4f}, iter: {}".format(best_mean_iou, best_acc, best_model_iter), flush=True)
                model.train()
            if checkpoint_now and rank == 0:
                path = os.path.join(config.SAVE_DIR, "iter_{}_state.pt".format(cur_iter))
                torch.save({"model": {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()},
                            "optimizer": {k: ({n: t.cpu() for n, t in v.items()} if isinstance(v, dict) else v) for k, v in optimizer.state_dict().items()},
                            "iter": cur_iter}, path)
                # and the weights alone in the reference's own format (train.py:200-203: iter_{n}_model_state.pdparams)
                from .src.utils.checkpoint import save_pdparams
                pd_path = os.path.join(config.SAVE_DIR, "iter_{}_model_state.pdparams".format(cur_iter))
                save_pdparams(model.state_dict(), pd_path)
                save_models.append((path, pd_path))
                print("saving the weights of model to {}".format(pd_path))
                if len(save_models) > config.KEEP_CHECKPOINT_MAX > 0:      # both files of the oldest checkpoint (train.py:210-213)
                    for old in save_models.popleft():
                        os.remove(old)
                if mean_iou is not None and mean_iou > best_mean_iou:       # train.py:215-229
                    best_mean_iou, best_acc, best_model_iter = mean_iou, acc, cur_iter
                    save_pdparams(model.state_dict(), os.path.join(config.SAVE_DIR, "best_model.pdparams"))
                    print("\n[EVAL] The model with the best validation mIoU ({:.4f}) was saved at iter {}.".format(best_mean_iou, best_model_iter))
                    print("[EVAL] Images: {}  mIoU: {:.4f}  Acc: {:.4f}  Kappa: {:.4f}  mean_f1: {:.4f}".format(len(val_images), mean_iou, acc, kap, mean_f1))
                    print("[EVAL] Class IoU: " + str(np.round(class_iou, 4)))
                    print("[EVAL] Class Acc: " + str(np.round(class_acc, 4)))
                    print("[EVAL] Class F1-score: " + str(np.round(class_f1, 4)) + "\n", flush=True)
            batch_start = time.time()
    torch.cuda.synchronize()
    total = sum(int(np.prod(p.shape)) for p in model.parameters())
    if rank == 0:
        print("Total params: {}".format(total))
    return model


if __name__ == "__main__":
    main()
