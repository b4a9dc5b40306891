"""Tile datasets of the EMRT configs (reference: src/datasets/{dataset,potsdam,vaihingen,loveda}.py, __init__.py:10-69
get_dataset) plus a small prefetching batch loader that stages batches on the GPU.

Directory layouts are the reference's:
  Potsdam / Vaihingen (both map to the Potsdam class in the reference's factory, __init__.py:50-58):
      <root>/train/<n>.tif  + <root>/train_convert_labels/<n>.png ;  <root>/test/... + <root>/test_convert_labels/...
      labels are class indices 0..5, 255 = ignore
  LoveDA:  <root>/Train/images_png/<n>.png + <root>/Train/masks_png/<n>.png ; <root>/Val/...
      masks are 1..7 with 0 = ignore: shifted by -1, ignore -> 255 (loveda.py:58-70)
Whole scenes (train.py --data scenes; no counterpart in the reference): <root>/images/<name>.* + <root>/labels/<name>.* (uint8 class indices),
optionally <root>/val_images + <root>/val_labels: SceneBank keeps them in device memory, SceneSampler cuts the training tiles there.
"""
import collections
import contextlib
import ctypes
import os
import queue
import threading

import numpy as np
import torch
from PIL import Image

from ... import _lib
from ..transforms import Compose, DevicePlan


class Dataset:
    """dataset.py: file_list of [image_path, label_path]; train -> (CHW float32, HW), val -> (CHW float32, 1HW)."""
    label_shift = 0

    def __init__(self, transforms, dataset_root, mode, num_classes, img_dir, label_dir, label_name):
        mode = mode.lower()
        if mode not in ("train", "val"):
            raise ValueError("`mode` should be one of ('train', 'val'), but got {}.".format(mode))
        if transforms is None:
            raise ValueError("`transforms` is necessary, but it is None.")
        self.transforms, self.mode, self.num_classes, self.ignore_index = Compose(transforms), mode, num_classes, 255
        self.dataset_root = dataset_root
        files = sorted(os.listdir(img_dir), key=lambda x: int(os.path.splitext(x)[0]))
        self.file_list = [[os.path.join(img_dir, f), os.path.join(label_dir, label_name(f))] for f in files]

    def __len__(self):
        return len(self.file_list)

    def __getitem__(self, idx):
        image_path, label_path = self.file_list[idx]
        if self.mode == "val":
            img, _ = self.transforms(img=image_path)
            label = np.asarray(Image.open(label_path))
            if self.label_shift:
                label = label - np.uint8(1)          # uint8 wrap: class 0 (ignore) -> 255
            return img, label[np.newaxis, :, :]
        img, label = self.transforms(img=image_path, label=label_path)
        if self.label_shift:
            label = label - np.uint8(1)
            label[label == 254] = 255                # padding (255) shifted to 254: restore
        return img, label


class Potsdam(Dataset):
    def __init__(self, transforms, dataset_root=None, mode="train", num_classes=6):
        sub = "train" if mode.lower() == "train" else "test"
        super().__init__(transforms, dataset_root, mode, num_classes, os.path.join(dataset_root, sub),
                         os.path.join(dataset_root, sub + "_convert_labels"), lambda f: os.path.splitext(f)[0] + ".png")


class LoveDA(Dataset):
    label_shift = 1

    def __init__(self, transforms, dataset_root=None, mode="train", num_classes=7):
        sub = "Train" if mode.lower() == "train" else "Val"
        super().__init__(transforms, dataset_root, mode, num_classes, os.path.join(dataset_root, sub, "images_png"),
                         os.path.join(dataset_root, sub, "masks_png"), lambda f: f)


def get_dataset(config, data_transform, mode="train"):
    name = config.DATA.DATASET
    mode = "val" if mode in ("val", "test") else "train"
    if name in ("Potsdam", "Vaihingen"):
        return Potsdam(transforms=data_transform, dataset_root=config.DATA.DATA_PATH, num_classes=config.DATA.NUM_CLASSES, mode=mode)
    if name == "LoveDA":
        return LoveDA(transforms=data_transform, dataset_root=config.DATA.DATA_PATH, num_classes=config.DATA.NUM_CLASSES, mode=mode)
    raise NotImplementedError("{} dataset is not supported".format(name))


def test_images(config):
    """Image paths of the configured dataset's test split, in the order a `val` Dataset lists them (Potsdam / Vaihingen: <root>/test,
    LoveDA: <root>/Val/images_png) -- what `python -m emrt_amd.predict` predicts without --input.  No labels are needed or looked for."""
    name, root = config.DATA.DATASET, config.DATA.DATA_PATH
    if name in ("Potsdam", "Vaihingen"):
        img_dir = os.path.join(root, "test")
    elif name == "LoveDA":
        img_dir = os.path.join(root, "Val", "images_png")
    else:
        raise NotImplementedError("{} dataset is not supported".format(name))
    files = sorted(os.listdir(img_dir), key=lambda x: int(os.path.splitext(x)[0]))
    return [os.path.join(img_dir, f) for f in files]


class TileLoader:
    """Iteration-based training loader (utils/dataloader.py:22-49): `sampler` yields index lists (DistributedTileSampler);
    `workers` threads decode + augment tiles (PIL and numpy release the GIL for the heavy parts) into PINNED host batches;
    at most `prefetch` finished batches exist at any time (a worker takes a slot before it starts a batch and the consumer
    returns it when it pops one).  The host->device copy is issued by the CONSUMER thread on the training stream (torch's
    current stream there): every later kernel on that stream is ordered after the copy, and the caching allocator ties the
    device block to that stream, so a batch can never be recycled under a queued kernel (a reader thread's `.to(device)`
    would run on that thread's own NULL stream, with nothing ordering it against the training stream)."""

    def __init__(self, dataset, sampler, device, workers=4, prefetch=4):
        self.dataset, self.sampler, self.device, self.workers, self.prefetch = dataset, sampler, device, max(1, workers), max(1, prefetch)
        self.pin = torch.cuda.is_available() and torch.device(device).type == "cuda"

    def _batch(self, idx):
        """Decoded, augmented host batch (fp32 [B,3,H,W], int64 [B,H,W]), page-locked when it is going to a GPU."""
        items = [self.dataset[i] for i in idx]
        imgs = torch.from_numpy(np.stack([it[0] for it in items]))
        labs = torch.from_numpy(np.stack([it[1] for it in items]).astype(np.int64))
        if self.pin:
            imgs, labs = imgs.pin_memory(), labs.pin_memory()
        return imgs, labs

    def epochs(self, start_epoch=0):
        """Endless generator of device batches, reshuffling per epoch."""
        todo, done = queue.Queue(maxsize=self.prefetch * 2), {}
        cv, stop = threading.Condition(), threading.Event()
        slots = threading.Semaphore(self.prefetch)       # finished-but-unconsumed batches (+ the ones being built)
        turn = [0]                                        # batches are built in order: slot n is taken before slot n + 1

        def feed():
            ep, n = start_epoch, 0
            while not stop.is_set():
                self.sampler.set_epoch(ep)
                for idx in self.sampler:
                    while not stop.is_set():
                        try:
                            todo.put((n, idx), timeout=0.2)
                            break
                        except queue.Full:
                            continue
                    if stop.is_set():
                        return
                    n += 1
                ep += 1

        def work():
            while not stop.is_set():
                try:
                    n, idx = todo.get(timeout=0.2)
                except queue.Empty:
                    continue
                # wait for this batch's turn, then for a free slot: the batch the consumer is waiting for always gets one
                with cv:
                    while turn[0] != n and not stop.is_set():
                        cv.wait(timeout=0.2)
                while not stop.is_set() and not slots.acquire(timeout=0.2):
                    pass
                if stop.is_set():
                    return
                try:
                    job = self._plan(idx)           # still this batch's turn: decisions drawn in batch order, whatever the worker count
                except Exception as e:
                    job = e
                with cv:
                    turn[0] = n + 1
                    cv.notify_all()
                if stop.is_set():
                    return
                try:
                    b = job if isinstance(job, Exception) else self._batch(job)
                except Exception as e:               # handed to the consumer, which raises it (a dead worker would leave it waiting)
                    b = e
                with cv:
                    done[n] = b
                    cv.notify_all()

        threads = [threading.Thread(target=feed, daemon=True)] + [threading.Thread(target=work, daemon=True) for _ in range(self.workers)]
        for t in threads:
            t.start()
        try:
            n = 0
            while True:
                with cv:
                    while n not in done:
                        cv.wait(timeout=1.0)
                    b = done.pop(n)
                slots.release()
                n += 1
                if isinstance(b, Exception):
                    raise b
                yield self._deliver(b)
        finally:
            stop.set()

    def _plan(self, idx):
        """Work a worker does while it holds batch `idx`'s turn (DeviceTileLoader draws its random decisions here); -> what _batch takes."""
        return idx

    def _deliver(self, b):
        """Consumer thread, training stream (see the class docstring): the batch on the device."""
        imgs, labs = b
        return imgs.to(self.device, non_blocking=True), labs.to(self.device, non_blocking=True)


def label_lut(shift):
    """The label map of a dataset's `label_shift` as a 256-entry table (None = identity): LoveDA's `label - 1` in uint8 with the
    254 -> 255 repair of Dataset.__getitem__ (class 0 = ignore -> 255, padding 255 -> 254 -> 255)."""
    if not shift:
        return None
    lut = ((np.arange(256) - shift) & 255).astype(np.uint8)
    lut[lut == 254] = 255
    return lut


class DeviceTileLoader(TileLoader):
    """TileLoader with the training transforms on the GPU (train.py --device_transforms).  Same epochs() contract: endless
    (fp32 [B,3,OH,OW], int64 [B,OH,OW]) device batches, the same values the CPU loader makes from the same seeds.

    A worker, while it holds its batch's turn, reads each tile's size from the file header (no decode) and draws the sample's random
    decisions (DevicePlan.plan), so decisions are drawn in batch and sample order whatever the number of workers; it then decodes the tiles
    to uint8 with read_image's / read_label's PIL calls outside the turn and packs them into one pinned host buffer.  The consumer thread
    issues one host->device copy of that buffer and one emrt_augment_tiles launch (resize, pad, crop, flip, normalise; emrt_aug_tiles of the
    second library when the chain holds RandomVerticalFlip / RandomDistort), both on the training stream, into outputs from torch's caching allocator on that stream.  Never inside a graph capture: train.py calls it between
    steps."""

    def __init__(self, dataset, sampler, device, workers=4, prefetch=4):
        super().__init__(dataset, sampler, device, workers, prefetch)
        if dataset.mode != "train":
            raise ValueError("DeviceTileLoader runs the training transforms; got a %r dataset" % dataset.mode)
        self.device_plan = DevicePlan(dataset.transforms.transforms)
        self.lut = label_lut(dataset.label_shift)

    def _plan(self, idx):
        job = []
        for i in idx:
            image_path, label_path = self.dataset.file_list[i]
            with Image.open(image_path) as im:
                W, H = im.size
            job.append((image_path, label_path, self.device_plan.plan(H, W)))
        turns = None
        if self.device_plan.rot is not None:      # RotPlan(base, turn): the base plans go the usual way, the turns follow the batch to _deliver
            job, turns = [(ip, lp, p.base) for ip, lp, p in job], [p.turn for _, _, p in job]
        sizes = {self.device_plan.out_size(p.H, p.W) for _, _, p in job}
        if len(sizes) != 1:
            raise ValueError("DeviceTileLoader: the samples of a batch have different output sizes %s (np.stack needs one)" % sorted(sizes))
        return job if turns is None else (job, turns)

    def _batch(self, job):
        """Decoded uint8 sources of one batch packed into one (pinned) buffer -> (buffer, [(img_off, lab_off, SamplePlan)], (OH, OW)); with
        RandomRot90 in the chain the batch's turns are a fourth element."""
        if self.device_plan.rot is not None:
            job, turns = job
            return self._batch_of(job) + (turns,)
        return self._batch_of(job)

    def _batch_of(self, job):
        total = sum(4 * p.H * p.W for _, _, p in job)
        buf = torch.empty(total, dtype=torch.uint8, pin_memory=self.pin)
        a = buf.numpy()
        samples, off = [], 0
        for image_path, label_path, p in job:
            img = np.asarray(Image.open(image_path).convert("RGB"), dtype=np.uint8)       # read_image's calls, kept in uint8
            lab = np.asarray(Image.open(label_path).convert("P"), dtype=np.uint8)         # read_label's
            if img.shape != (p.H, p.W, 3) or lab.shape != (p.H, p.W):
                raise ValueError("DeviceTileLoader: %s is %s and %s is %s; header said %dx%d" % (
                    image_path, img.shape, label_path, lab.shape, p.H, p.W))
            a[off:off + img.size] = img.reshape(-1)
            a[off + img.size:off + img.size + lab.size] = lab.reshape(-1)
            samples.append((off, off + img.size, p))
            off += img.size + lab.size
        return buf, samples, self.device_plan.out_size(job[0][2].H, job[0][2].W)

    def _deliver(self, b):
        from ... import functional as F
        dp = self.device_plan
        buf, samples, out_size = b[:3]
        dev = torch.device(self.device)
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            src = buf.to(dev, non_blocking=True)
            if dp.extended:      # RandomVerticalFlip / RandomDistort in the chain: the second library's entry point
                out = F.aug_tiles(src, samples, out_size, dp.mean, dp.stdinv, dp.img_pad, dp.label_pad, self.lut, distort=dp.distort is not None)
            else:
                out = F.augment_tiles(src, samples, out_size, dp.mean, dp.stdinv, dp.img_pad, dp.label_pad, self.lut)
            if dp.rot is not None:      # RandomRot90 in the chain: the finished batch is turned in place (libemrt_hip_rot.so), on the same stream
                F.rot_batch(out[0], out[1], b[3])
            return out


# ---- whole scenes resident in device memory (train.py --data scenes) -----------------------------------------------------------

_SceneEntry = _lib.struct("EmrtSceneEntry")      # generated from include/emrt_hip.h


MAX_SCALES = 16           # csrc/augment.hip SCENE_MAX_SCALES: scale entries of one emrt_scene_draw launch
DRAW_COLS = 10            # a row of the draw table: scene, y0, x0, scale_index, h, w, off_y, off_x, flip, 0
AUG_DRAW_COLS = 18        # ... of emrt_aug_scene_draw (include/emrt_hip_augment.h: EMRT_AUG_DRAW_COLS), an extended chain's table


def _free_device_bytes(device):
    """Free memory of a GPU in bytes; None for a host `device` (the CPU tests: no limit is checked there)."""
    device = torch.device(device)
    if device.type != "cuda":
        return None
    return int(torch.cuda.mem_get_info(device)[0])


@contextlib.contextmanager
def _no_pixel_limit():
    """PIL refuses images above ~179 Mpixel as decompression bombs; an ISPRS scene mosaic may be larger and is the user's own file."""
    old, Image.MAX_IMAGE_PIXELS = Image.MAX_IMAGE_PIXELS, None
    try:
        yield
    finally:
        Image.MAX_IMAGE_PIXELS = old


def scene_files(img_dir, label_dir):
    """-> [(name, image path, label path)] in name order: every file of img_dir with the file of label_dir that has the same name, or the same
    stem when the extensions differ (a .tif scene with its .png class map).  A scene without a label map is an error, by name."""
    if not os.path.isdir(img_dir):
        raise FileNotFoundError("scenes: no directory %s" % img_dir)
    labels = {}
    for f in sorted(os.listdir(label_dir)) if os.path.isdir(label_dir) else []:
        labels.setdefault(os.path.splitext(f)[0], f)
    out = []
    for f in sorted(os.listdir(img_dir)):
        lab = f if os.path.exists(os.path.join(label_dir, f)) else labels.get(os.path.splitext(f)[0])
        if lab is None:
            raise FileNotFoundError("scenes: %s has no label map named %s.* under %s" % (os.path.join(img_dir, f), os.path.splitext(f)[0], label_dir))
        out.append((os.path.splitext(f)[0], os.path.join(img_dir, f), os.path.join(label_dir, lab)))
    if not out:
        raise ValueError("scenes: %s holds no images" % img_dir)
    return out


ClassIndex = collections.namedtuple("ClassIndex", "counts totals cum cum_dev row_start row_start_host row_start_dev build_ms")
ClassIndex.__doc__ = """SceneBank.class_index(): the label index of include/emrt_hip_sampler.h.  counts int32 [R][n_classes] and totals int64
[n_classes] (numpy); cum int64 [n_classes][R + 1] (numpy) and cum_dev its device copy; row_start int64 [n_scenes + 1] as numpy, as the ctypes
host mirror the entry points check, and on the device; build_ms the counting launch between device events (None off the GPU)."""


def class_probabilities(totals, temperature=0.1, class_probs=None):
    """The class distribution of DATA.SCENE_SAMPLING, float64 [n_classes].  totals: pixels per class in the bank.  P(c) is proportional to
    exp((1 - f_c) / temperature) with f_c = totals[c] / sum(totals), or to class_probs[c] when that list is given; a class without a pixel gets
    0 either way.  A bank without a countable pixel, and weights that leave nothing to draw, are refused."""
    n = np.asarray(totals, dtype=np.int64)
    if n.ndim != 1 or n.size < 1 or (n < 0).any():
        raise ValueError("scenes: class totals must be a non-empty list of non-negative counts, got %r" % (totals,))
    if int(n.sum()) == 0:
        raise ValueError("scenes: the bank holds no pixel of any of the %d classes (every label is ignored): class-aware sampling has "
                         "nothing to draw" % n.size)
    if class_probs is not None:
        w = np.asarray(class_probs, dtype=np.float64)
        if w.shape != n.shape or not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("scenes: SCENE_SAMPLING.CLASS_PROBS must be %d finite non-negative weights (DATA.NUM_CLASSES), got %r"
                             % (n.size, class_probs))
    else:
        t = float(temperature)
        if not (np.isfinite(t) and t >= 1.0 / 700.0):
            raise ValueError("scenes: SCENE_SAMPLING.TEMPERATURE must be finite and at least 1/700 (exp(1 / T) must stay finite), got %r" % (temperature,))
        f = n.astype(np.float64) / float(n.sum())
        w = np.exp((1.0 - f) / t)
    w = np.where(n > 0, w, 0.0)
    if not float(w.sum()) > 0.0:
        raise ValueError("scenes: SCENE_SAMPLING.CLASS_PROBS gives no weight to a class that has pixels in the bank")
    return w / w.sum()


def class_thresholds(probs):
    """uint64 [n_classes]: thr[c] = floor(2^32 * sum of probs[:c + 1]) in float64, and exactly 2^32 from the last class with a non-zero
    probability on.  A 32-bit word w picks the class `number of c with w >= thr[c]` (include/emrt_hip_sampler.h)."""
    p = np.asarray(probs, dtype=np.float64)
    thr = np.minimum(np.floor(np.cumsum(p) * 4294967296.0), 4294967296.0).astype(np.uint64)
    thr[int(np.flatnonzero(p > 0)[-1]):] = np.uint64(1 << 32)
    return thr


class SceneBank:
    """Whole training scenes in ONE uint8 device buffer: <root>/images/* (RGB) with the same-named uint8 class-index maps of <root>/labels/* (the
    format of the *_convert_labels trees).  Scene i is its HWC image at img_off[i] followed by its HW label map at lab_off[i].

    bank.buffer     uint8 [nbytes] on `device`
    bank.sizes      [(H, W)] per scene, bank.names their file stems, bank.offsets [(img_off, lab_off)]
    bank.tables(th, tw) -> the scene table and the cumulative table of tile origins, on the device and as the host mirrors the entry points
                    check (emrt_scene_draw / emrt_scene_sample)
    bank.scene(i)   -> (uint8 [H, W, 3], uint8 [H, W]): scene i and its label map as views of bank.buffer (no copy)
    label_shift     the dataset's label shift (LoveDA: 1), applied by the sampler through label_lut

    sub             the two directories under `root`; a validation bank is SceneBank(root, device, label_shift, sub=("val_images", "val_labels"),
                    shift_on_upload=True)
    shift_on_upload the label maps are stored as `label - np.uint8(label_shift)` with uint8 wrap, what Dataset.__getitem__ does in `val` mode
                    (LoveDA's class 0 becomes 255): an evaluator counts the stored bytes as they lie.  False: stored as decoded."""

    def __init__(self, root, device, label_shift=0, sub=("images", "labels"), shift_on_upload=False):
        self.root, self.device, self.label_shift = root, torch.device(device), int(label_shift)
        self.sub, self.shift_on_upload = tuple(sub), bool(shift_on_upload)
        files = scene_files(os.path.join(root, self.sub[0]), os.path.join(root, self.sub[1]))
        self.names, self.sizes, self.offsets = [], [], []
        total = 0
        with _no_pixel_limit():
            for name, ip, lp in files:          # headers only: sizes and modes are known before a byte is decoded or uploaded
                with Image.open(ip) as im, Image.open(lp) as lab:
                    if im.mode != "RGB":
                        raise ValueError("scenes: %s is a %s image; the bank holds 8-bit RGB scenes" % (ip, im.mode))
                    if lab.mode not in ("L", "P"):
                        raise ValueError("scenes: %s is a %s image; label maps are uint8 class indices (modes L or P)" % (lp, lab.mode))
                    if im.size != lab.size:
                        raise ValueError("scenes: %s is %dx%d but its label map %s is %dx%d" % (ip, im.size[1], im.size[0], lp, lab.size[1], lab.size[0]))
                    W, H = im.size
                self.names.append(name)
                self.sizes.append((H, W))
                self.offsets.append((total, total + 3 * H * W))
                total += 4 * H * W
            self.nbytes = total
            free = _free_device_bytes(self.device)
            if free is not None and total > free:
                raise MemoryError("scenes: the bank of %d scenes needs %d bytes, the device has %d bytes free" % (len(files), total, free))
            self.buffer = torch.empty(total, dtype=torch.uint8, device=self.device)
            for (name, ip, lp), (io, lo), (H, W) in zip(files, self.offsets, self.sizes):
                img = np.array(Image.open(ip).convert("RGB"), dtype=np.uint8)         # read_image's / read_label's calls, kept in uint8
                lab = np.array(Image.open(lp).convert("P"), dtype=np.uint8)
                if self.shift_on_upload and self.label_shift:
                    lab = lab - np.uint8(self.label_shift)          # uint8 wrap: class 0 (ignore) -> 255
                self.buffer[io:lo].copy_(torch.from_numpy(img.reshape(-1)))
                self.buffer[lo:lo + H * W].copy_(torch.from_numpy(lab.reshape(-1)))
        self._tables, self._index = {}, {}

    def __len__(self):
        return len(self.sizes)

    def scene(self, i):
        """Scene i and its label map, uint8 [H, W, 3] and uint8 [H, W]: views of bank.buffer."""
        (io, lo), (H, W) = self.offsets[i], self.sizes[i]
        return self.buffer[io:lo].view(H, W, 3), self.buffer[lo:lo + H * W].view(H, W)

    def origins(self, th, tw):
        """Tile origins per scene, (H - th + 1) * (W - tw + 1); a tile larger than a scene is an error naming both."""
        for i, (H, W) in enumerate(self.sizes):
            if th > H or tw > W:
                raise ValueError("scenes: the %dx%d tile is larger than scene %d (%s, %dx%d)" % (th, tw, i, self.names[i], H, W))
        return [(H - th + 1) * (W - tw + 1) for H, W in self.sizes]

    def tables(self, th, tw):
        """-> (scenes_dev uint8 tensor, cum_dev int64 tensor, scenes_host ctypes array, cum_host ctypes array) for a th x tw tile."""
        if (th, tw) not in self._tables:
            n = len(self)
            host = (_SceneEntry * n)(*[_SceneEntry(io, lo, H, W) for (io, lo), (H, W) in zip(self.offsets, self.sizes)])
            cum = np.concatenate([[0], np.cumsum(self.origins(th, tw), dtype=np.int64)]).astype(np.int64)
            cum_host = (ctypes.c_longlong * (n + 1))(*cum.tolist())
            scenes_dev = torch.from_numpy(np.frombuffer(bytes(host), dtype=np.uint8).copy()).to(self.device)
            cum_dev = torch.from_numpy(cum).to(self.device)
            self._tables[(th, tw)] = (scenes_dev, cum_dev, host, cum_host)
        return self._tables[(th, tw)]


    def class_index(self, n_classes, lut=None):
        """-> ClassIndex: pixels per class and row, counted once on the device (emrt_smp_row_counts of the third library, after the 256-byte
        `lut` when given; values >= n_classes are not counted), read back once, and its class-major prefix over the rows of the whole bank.
        Synchronises and uploads: call it before any capture (SceneSampler does, in its constructor)."""
        key = (int(n_classes), None if lut is None else bytes(bytearray(int(v) for v in lut)))
        if key not in self._index:
            from ... import functional as Fn
            from ...runtime import ctx
            n, ncls = len(self), int(n_classes)
            row_start = np.concatenate([[0], np.cumsum([H for H, _ in self.sizes], dtype=np.int64)]).astype(np.int64)
            R = int(row_start[-1])
            row_start_host = (ctypes.c_longlong * (n + 1))(*row_start.tolist())
            row_start_dev = torch.from_numpy(row_start).to(self.device)
            scenes_dev, _, scenes_host, _ = self.tables(1, 1)
            counts = torch.zeros((R, ncls), dtype=torch.int32, device=self.device)
            lut_host = None if lut is None else (ctypes.c_ubyte * 256)(*[int(v) for v in lut])
            on_gpu = self.device.type == "cuda"
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if on_gpu else None
            if on_gpu:
                ev[0].record()
            _lib.sampler_lib().call("emrt_smp_row_counts", Fn.P(self.buffer), self.nbytes, Fn.P(scenes_dev), ctypes.cast(scenes_host, ctypes.c_void_p),
                                    Fn.P(row_start_dev), ctypes.cast(row_start_host, ctypes.c_void_p), n,
                                    None if lut_host is None else ctypes.cast(lut_host, ctypes.c_void_p), ncls, Fn.P(counts), R, ctx().stream)
            if on_gpu:
                ev[1].record()
            host = counts.cpu().numpy()          # (the copy waits for the launch)
            cum = np.zeros((ncls, R + 1), dtype=np.int64)
            np.cumsum(host.T.astype(np.int64), axis=1, out=cum[:, 1:])
            self._index[key] = ClassIndex(host, cum[:, -1].copy(), cum, torch.from_numpy(cum).to(self.device), row_start, row_start_host,
                                          row_start_dev, ev[0].elapsed_time(ev[1]) if on_gpu else None)
        return self._index[key]


class SceneSampler:
    """The training batches of `--data scenes`: SceneSampler(bank, transforms, batch_size, seed, rank).fill(images, labels) enqueues two launches on
    the current stream -- emrt_scene_draw (every random decision of the batch, from the device step counter) and emrt_scene_sample (the transform
    chain on the drawn windows) -- and touches nothing else, so it can run inside a captured training step.

    `transforms` is one of the chains DevicePlan accepts.  With RandomVerticalFlip / RandomDistort in it (DATA.AUGMENT) the two calls are the second
    library's emrt_aug_scene_draw and emrt_aug_scene_sample (draw, memset of the luminance sums, statistics, apply; include/emrt_hip_augment.h), just as
    capturable; the other chains never touch that library.  Potsdam / Vaihingen: the source tile is the crop size, the scale table is
    ResizeStepScaling.resized(factor, th, tw) over its np.linspace factors (Python's round stays on the host).  [Normalize] alone (LoveDA): pass
    `tile` = (h, w); one scale entry of the tile's own size, no flip.  The bank's label_shift goes down as label_lut.
    The draws are a pure function of (seed, step counter, rank, sample): restoring the step counter continues the same data stream.

    `sampling` is the DATA.SCENE_SAMPLING config node (MODE, PROB, TEMPERATURE, CLASS_PROBS).  None or MODE "uniform": the launches above and
    nothing else.  MODE "class" (needs num_classes): the constructor builds the bank's label index (SceneBank.class_index) and the class
    thresholds and uploads them, and fill() puts ONE launch of the third library, emrt_smp_class_redraw (include/emrt_hip_sampler.h), between the
    draw and the sample launch: it moves a share PROB of the windows onto a pixel of a drawn class and leaves every other decision alone.
    sampler.class_table then holds (class, pixel share, sampling probability) per class; class_names, when given, name the log lines.

    With RandomRot90 in the chain (DATA.AUGMENT.ROT90_PROB) fill() appends ONE launch of libemrt_hip_rot.so, emrt_rot_scene_batch, after the sample
    launch on the same stream: it draws every sample's turn from Philox block 5 of the same key and counter and turns the batch in place;
    sampler.turns (int32 [B]) then holds the batch's turns.  The other chains never touch that library."""

    def __init__(self, bank, transforms, batch_size, seed, rank=0, tile=None, sampling=None, num_classes=None, class_names=None):
        self.bank, self.plan = bank, DevicePlan(list(transforms))
        dp = self.plan
        if dp.crop is not None:
            crop = dp.crop.size()
            if tile is not None and tuple(tile) != tuple(crop):
                raise ValueError("scenes: the source tile of this chain is its crop size %r, got tile %r" % (crop, tuple(tile)))
            self.tile = self.crop = (int(crop[0]), int(crop[1]))
            sc = dp.scaling
            if sc.min_scale_factor == sc.max_scale_factor:
                factors = [sc.min_scale_factor]
            elif sc.scale_step_size == 0:
                raise ValueError("scenes: ResizeStepScaling with scale_step_size 0 draws a continuous factor; the device sampler draws from a table of steps")
            else:
                factors = np.linspace(sc.min_scale_factor, sc.max_scale_factor, int((sc.max_scale_factor - sc.min_scale_factor) / sc.scale_step_size + 1)).tolist()
            self.scales = [type(sc).resized(f, *self.tile) for f in factors]
            self.flip_prob = float(dp.flip.prob)
        else:
            if tile is None:
                raise ValueError("scenes: a chain without RandomPaddingCrop needs the tile size, tile=(h, w)")
            self.tile = self.crop = (int(tile[0]), int(tile[1]))
            self.scales = [self.tile]
            self.flip_prob = 0.0
        if not 1 <= len(self.scales) <= MAX_SCALES:
            raise ValueError("scenes: %d scale steps; the device sampler takes 1 to %d" % (len(self.scales), MAX_SCALES))
        if min(min(s) for s in self.scales) < 1:
            raise ValueError("scenes: a scale step resizes the %r tile to nothing: %r" % (self.tile, self.scales))
        if not 0.0 <= self.flip_prob <= 1.0:
            raise ValueError("scenes: flip probability %r is outside [0, 1]" % self.flip_prob)
        self.batch_size, self.rank = int(batch_size), int(rank)
        if self.batch_size < 1 or self.rank < 0:
            raise ValueError("scenes: batch_size must be positive and rank non-negative, got %r and %r" % (batch_size, rank))
        self.key = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.total_origins = sum(bank.origins(*self.tile))
        self.lut = label_lut(bank.label_shift)
        self.draws = torch.zeros((self.batch_size, AUG_DRAW_COLS if dp.extended else DRAW_COLS), dtype=torch.int32, device=bank.device)
        self._tables = bank.tables(*self.tile)       # uploaded here: fill() may run under stream capture, where no host -> device copy can
        # the HOST arguments of the two launches, built once: constants of the run, safe to bake into a captured graph
        self._scale_hw = (ctypes.c_int * (2 * len(self.scales)))(*[int(v) for hw in self.scales for v in hw])
        self._mean = (ctypes.c_double * 3)(*[float(v) for v in dp.mean])
        self._stdinv = (ctypes.c_double * 3)(*[float(v) for v in dp.stdinv])
        self._pad = (ctypes.c_float * 3)(*[float(v) for v in dp.img_pad])
        self._lut = None if self.lut is None else (ctypes.c_ubyte * 256)(*[int(v) for v in self.lut])
        if dp.extended:          # the second library's draws and launches (include/emrt_hip_augment.h); its workspace is allocated here, once
            self.vflip_prob = float(dp.vflip.prob) if dp.vflip is not None else 0.0
            if not 0.0 <= self.vflip_prob <= 1.0:
                raise ValueError("scenes: vertical flip probability %r is outside [0, 1]" % self.vflip_prob)
            names = ("brightness", "contrast", "saturation")
            d = dp.distort
            self._ranges = (ctypes.c_double * 3)(*[float(getattr(d, n + "_range")) if d is not None else 0.0 for n in names])
            self._probs = (ctypes.c_double * 3)(*[float(getattr(d, n + "_prob")) if d is not None else 0.0 for n in names])
            self._ws_bytes = 8 * self.batch_size          # = emrt_aug_workspace_bytes(B); the entry point checks it
            self._ws = torch.zeros(self.batch_size, dtype=torch.int64, device=bank.device)
        self.rot_prob = float(dp.rot.prob) if dp.rot is not None else 0.0      # (DevicePlan has checked the square crop and the range)
        self.turns = torch.zeros(self.batch_size, dtype=torch.int32, device=bank.device) if dp.rot is not None else None
        mode = "uniform" if sampling is None else sampling["MODE"]
        if mode not in ("uniform", "class"):
            raise ValueError("scenes: SCENE_SAMPLING.MODE must be 'uniform' or 'class', got %r" % (mode,))
        self.class_mode, self.class_table = mode == "class", None
        if self.class_mode:
            self._init_class_mode(sampling, num_classes, class_names)

    def _init_class_mode(self, sampling, num_classes, class_names):
        """Everything the redraw launch needs, once: fill() may run under stream capture, where nothing can be counted, read back or uploaded."""
        if num_classes is None or not 1 <= int(num_classes) <= 256:
            raise ValueError("scenes: SCENE_SAMPLING.MODE 'class' needs num_classes in 1..256 (DATA.NUM_CLASSES), got %r" % (num_classes,))
        self.class_prob = float(sampling["PROB"])
        if not 0.0 <= self.class_prob <= 1.0:
            raise ValueError("scenes: SCENE_SAMPLING.PROB %r is outside [0, 1]" % (sampling["PROB"],))
        ncls, bank = int(num_classes), self.bank
        self.index = idx = bank.class_index(ncls, self.lut)
        self.class_probs = class_probabilities(idx.totals, sampling["TEMPERATURE"], sampling["CLASS_PROBS"])
        self.thresholds = class_thresholds(self.class_probs)
        share = idx.totals / float(idx.totals.sum())
        name = (lambda c: str(class_names[c])) if class_names is not None else (lambda c: "class %d" % c)
        self.class_table = [(name(c), float(share[c]), float(self.class_probs[c])) for c in range(ncls)]
        for c in range(ncls):
            if idx.totals[c] == 0:
                print("[scenes] %s has no pixel in the bank: its sampling probability is 0" % name(c), flush=True)
        self._thr_host = (ctypes.c_ulonglong * ncls)(*[int(v) for v in self.thresholds])
        self._thr_dev = torch.from_numpy(self.thresholds.view(np.int64).copy()).to(bank.device)          # (the same 64 bits)
        scenes_host = self._tables[2]
        # the HOST arguments of the redraw launch: the same objects in every call
        self._smp_host = (ctypes.cast(scenes_host, ctypes.c_void_p), ctypes.cast(idx.row_start_host, ctypes.c_void_p),
                          ctypes.cast(self._thr_host, ctypes.c_void_p), None if self._lut is None else ctypes.cast(self._lut, ctypes.c_void_p))
        self._num_classes = ncls

    def _redraw(self, Fn, c, key):
        """emrt_smp_class_redraw on self.draws: after the draw launch, before the sample launch, on the same stream."""
        scenes_dev = self._tables[0]
        scenes_host, rows_host, thr_host, lut = self._smp_host
        idx, (th, tw) = self.index, self.tile
        _lib.sampler_lib().call("emrt_smp_class_redraw", Fn.P(c.step_counter), Fn.P(self.bank.buffer), self.bank.nbytes, Fn.P(scenes_dev), scenes_host,
                                Fn.P(idx.row_start_dev), rows_host, len(self.bank), Fn.P(idx.cum_dev), Fn.P(self._thr_dev), thr_host,
                                self._num_classes, lut, key, self.rank, self.batch_size, th, tw, self.class_prob, Fn.P(self.draws),
                                int(self.draws.shape[1]), c.stream)

    @property
    def batch_shape(self):
        """(B, OH, OW) of the batches fill() writes."""
        return (self.batch_size,) + self.crop

    def fill(self, images, labels):
        """images fp32 [B, 3, OH, OW], labels int64 [B, OH, OW], contiguous, on the bank's device: the next batch, on the current stream."""
        from ... import functional as Fn
        from ...runtime import ctx
        B, (OH, OW), (th, tw) = self.batch_size, self.crop, self.tile
        if images.dtype != torch.float32 or tuple(images.shape) != (B, 3, OH, OW) or not images.is_contiguous():
            raise ValueError("scenes: images must be contiguous fp32 %r, got %s %r" % ((B, 3, OH, OW), images.dtype, tuple(images.shape)))
        if labels.dtype != torch.int64 or tuple(labels.shape) != (B, OH, OW) or not labels.is_contiguous():
            raise ValueError("scenes: labels must be contiguous int64 %r, got %s %r" % ((B, OH, OW), labels.dtype, tuple(labels.shape)))
        c = ctx()
        scenes_dev, cum_dev, scenes_host, cum_host = self._tables
        n = len(self.bank)
        key = self.key - (1 << 64) if self.key >= (1 << 63) else self.key         # the same 64 bits as a C long long
        if self.plan.extended:
            A = _lib.augment_lib()
            distort = int(self.plan.distort is not None)
            A.call("emrt_aug_scene_draw", Fn.P(c.step_counter), Fn.P(scenes_dev), Fn.P(cum_dev), ctypes.cast(scenes_host, ctypes.c_void_p),
                   ctypes.cast(cum_host, ctypes.c_void_p), n, self.bank.nbytes, key, self.rank, B, th, tw, OH, OW, self.flip_prob, self.vflip_prob,
                   distort, ctypes.cast(self._ranges, ctypes.c_void_p), ctypes.cast(self._probs, ctypes.c_void_p),
                   ctypes.cast(self._scale_hw, ctypes.c_void_p), len(self.scales), Fn.P(self.draws), c.stream)
            if self.class_mode:
                self._redraw(Fn, c, key)
            A.call("emrt_aug_scene_sample", Fn.P(self.bank.buffer), self.bank.nbytes, Fn.P(scenes_dev), ctypes.cast(scenes_host, ctypes.c_void_p), n,
                   Fn.P(self.draws), B, th, tw, OH, OW, distort, ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._stdinv, ctypes.c_void_p),
                   ctypes.cast(self._pad, ctypes.c_void_p), int(self.plan.label_pad),
                   None if self._lut is None else ctypes.cast(self._lut, ctypes.c_void_p), Fn.P(images), 3 * OH * OW, Fn.P(labels),
                   Fn.P(self._ws), self._ws_bytes, c.stream)
            self._rot(Fn, c, key, images, labels)
            return
        L = Fn._L()
        L.call("emrt_scene_draw", Fn.P(c.step_counter), Fn.P(scenes_dev), Fn.P(cum_dev), ctypes.cast(scenes_host, ctypes.c_void_p),
               ctypes.cast(cum_host, ctypes.c_void_p), n, self.bank.nbytes, key, self.rank, B, th, tw, OH, OW, self.flip_prob,
               ctypes.cast(self._scale_hw, ctypes.c_void_p), len(self.scales), Fn.P(self.draws), c.stream)
        if self.class_mode:
            self._redraw(Fn, c, key)
        L.call("emrt_scene_sample", Fn.P(self.bank.buffer), self.bank.nbytes, Fn.P(scenes_dev), ctypes.cast(scenes_host, ctypes.c_void_p), n,
               Fn.P(self.draws), B, th, tw, OH, OW, ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._stdinv, ctypes.c_void_p),
               ctypes.cast(self._pad, ctypes.c_void_p), int(self.plan.label_pad),
               None if self._lut is None else ctypes.cast(self._lut, ctypes.c_void_p), Fn.P(images), 3 * OH * OW, Fn.P(labels), c.stream)
        self._rot(Fn, c, key, images, labels)

    def _rot(self, Fn, c, key, images, labels):
        """emrt_rot_scene_batch on the batch the sample launch just wrote, on the same stream; nothing without RandomRot90 in the chain."""
        if self.plan.rot is None:
            return
        _lib.rot_lib().call("emrt_rot_scene_batch", Fn.P(c.step_counter), key, self.rank, self.batch_size, self.crop[0], self.rot_prob, Fn.P(images),
                            Fn.P(labels), Fn.P(self.turns), c.stream)


class SceneVal(Dataset):
    """The validation scenes of a scene tree, <root>/val_images/* with <root>/val_labels/*, as a `val` Dataset (what ValTiles / evaluate() take)."""

    def __init__(self, transforms, dataset_root, num_classes, label_shift=0):
        self.transforms, self.mode, self.num_classes, self.ignore_index = Compose(transforms), "val", num_classes, 255
        self.dataset_root, self.label_shift = dataset_root, label_shift
        self.file_list = [[ip, lp] for _, ip, lp in scene_files(os.path.join(dataset_root, "val_images"), os.path.join(dataset_root, "val_labels"))]

    def __getitem__(self, idx):
        with _no_pixel_limit():
            return super().__getitem__(idx)
