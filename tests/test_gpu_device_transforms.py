"""-m gpu: the fused augmentation kernel (csrc/augment.hip) and DeviceTileLoader against the CPU transform chain, bit for bit, and a
training run with --device_transforms end to end."""
import argparse
import math
import os
import random
import re
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from emrt_amd import functional as F
from emrt_amd.config import get_config, update_config
from emrt_amd.distributed import DistributedTileSampler
from emrt_amd.src import transforms as T
from emrt_amd.src.datasets import DeviceTileLoader, TileLoader, get_dataset, label_lut

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "emrt_amd/configs/EMRT")
SCALES = np.linspace(0.5, 2.0, 7).tolist()


def _chain(crop, pad=(0, 0, 0), label_pad=255):
    return [T.ResizeStepScaling(0.5, 2.0, 0.25), T.RandomPaddingCrop(crop_size=crop, img_padding_value=pad, label_padding_value=label_pad),
            T.RandomHorizontalFlip(prob=0.5), T.Normalize(mean=T._MEAN, std=T._STD)]


def _cpu(chain, img, lab, scale, off, flip):
    """The CPU chain on float32 / uint8 arrays with its draws forced to the given decisions."""
    chain[0].draw = lambda: scale
    chain[1].draw = lambda ih, iw: None if (ih, iw) == chain[1].size() else off
    chain[2].draw = lambda: bool(flip)
    return T.Compose(chain)(img.astype(np.float32), lab)


def _run(dp, tiles, plans, lut=None):
    """Pack uint8 tiles, stage them and run the kernel -> host (fp32 [B,3,OH,OW], int64 [B,OH,OW])."""
    chunks, samples, off = [], [], 0
    for (img, lab), p in zip(tiles, plans):
        chunks += [img.reshape(-1), lab.reshape(-1)]
        samples.append((off, off + img.size, p))
        off += img.size + lab.size
    src = torch.from_numpy(np.concatenate(chunks)).cuda()
    out, labels = F.augment_tiles(src, samples, dp.out_size(plans[0].H, plans[0].W), dp.mean, dp.stdinv, dp.img_pad, dp.label_pad, lut)
    torch.cuda.synchronize()
    return out.cpu(), labels.cpu()


@pytest.mark.parametrize("crop,pad,label_pad", [((256, 256), (0, 0, 0), 255), ((160, 96), (123.675, 116.28, 103.53), 7)])
def test_kernel_matches_cpu_chain_bit_for_bit(crop, pad, label_pad):
    """Every scale factor of the Potsdam chain, flip on and off, sources of 80x96 / 255x257 / 256^2 / 512^2 (padding below the crop,
    crops of the resized image above it), a square and a non-square crop, one batch of 56 samples (four launches of 16)."""
    g = np.random.RandomState(11)
    chain = _chain(crop, pad, label_pad)
    dp = T.DevicePlan(chain)
    OH, OW = crop[1], crop[0]
    tiles, plans, want = [], [], []
    for H, W in ((80, 96), (255, 257), (256, 256), (512, 512)):
        img = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
        lab = g.randint(0, 6, (H, W)).astype(np.uint8)
        lab[g.rand(H, W) < 0.05] = 255
        for scale in SCALES:
            h, w = T.ResizeStepScaling.resized(scale, H, W)
            for flip in (0, 1):
                off = (g.randint(max(h, OH) - OH + 1), g.randint(max(w, OW) - OW + 1))
                p = T.SamplePlan(H, W, h, w, int(off[0]) if (h, w) != (OH, OW) else 0, int(off[1]) if (h, w) != (OH, OW) else 0, flip)
                tiles.append((img, lab))
                plans.append(p)
                want.append(_cpu(_chain(crop, pad, label_pad), img, lab, scale, (p.off_y, p.off_x), flip))
    got_img, got_lab = _run(dp, tiles, plans)
    assert got_img.shape == (len(plans), 3, OH, OW) and got_lab.shape == (len(plans), OH, OW)
    for i, (wi, wl) in enumerate(want):
        assert torch.equal(got_img[i], torch.from_numpy(wi)), (plans[i], (got_img[i] - torch.from_numpy(wi)).abs().max().item())
        assert torch.equal(got_lab[i], torch.from_numpy(wl.astype(np.int64))), plans[i]
    assert any(p.h < OH for p in plans) and any(p.h > OH for p in plans)       # both padding and cropping were exercised


def test_kernel_matches_lovedas_chain_with_label_shift():
    """[Normalize] alone (output = source size) and LoveDA's label - 1 with the 254 -> 255 repair, through the lookup table."""
    g = np.random.RandomState(5)
    dp = T.DevicePlan([T.Normalize(mean=T._MEAN, std=T._STD)])
    tiles = [(g.randint(0, 256, (80, 96, 3)).astype(np.uint8), g.randint(0, 8, (80, 96)).astype(np.uint8)) for _ in range(3)]
    tiles[0][1][:4] = 255
    plans = [dp.plan(80, 96) for _ in tiles]
    got_img, got_lab = _run(dp, tiles, plans, label_lut(1))
    for i, (img, lab) in enumerate(tiles):
        wi, wl = T.Compose([T.Normalize(mean=T._MEAN, std=T._STD)])(img.astype(np.float32), lab)
        wl = wl - np.uint8(1)
        wl[wl == 254] = 255
        assert torch.equal(got_img[i], torch.from_numpy(wi)) and torch.equal(got_lab[i], torch.from_numpy(wl.astype(np.int64)))


def _tree(root, sizes):
    rng = np.random.RandomState(0)
    for sub in ("train", "test"):
        os.makedirs(os.path.join(root, sub))
        os.makedirs(os.path.join(root, sub + "_convert_labels"))
        for i, (h, w) in enumerate(sizes):
            Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, sub, "%d.tif" % i))
            Image.fromarray(rng.randint(0, 6, (h, w), dtype=np.uint8)).save(os.path.join(root, sub + "_convert_labels", "%d.png" % i))
    return root


def _batches(cls, ds, workers, n, seed=3):
    for t in threading.enumerate():                      # np.random / random are process-global: no reader thread of an earlier loader may draw
        if t.daemon and t.name.endswith(("(work)", "(feed)")):
            t.join(timeout=30)
    np.random.seed(seed)
    random.seed(seed)
    before = set(threading.enumerate())
    gen = cls(ds, DistributedTileSampler(len(ds), 4, 0, 1, shuffle=True, seed=2), "cuda:0", workers=workers, prefetch=3).epochs()
    out = [tuple(t.cpu() for t in next(gen)) for _ in range(n)]
    gen.close()
    for t in set(threading.enumerate()) - before:        # a prefetching worker finishes its draws before the next loader is seeded
        t.join(timeout=10)
    return out


def test_device_loader_matches_cpu_loader(tmp_path):
    """A small Potsdam tree of mixed source sizes, np.random and random seeded before each loader: DeviceTileLoader with 1 and with 4
    reader threads yields exactly the batches of the CPU TileLoader with 1, across an epoch boundary."""
    sizes = [(80, 96), (130, 70), (64, 64), (255, 257), (40, 100), (96, 80), (64, 64), (70, 130)]
    root = _tree(str(tmp_path / "p"), sizes)
    cfg = update_config(get_config(), argparse.Namespace(cfg=os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam.yaml")))
    cfg.DATA.DATA_PATH = root
    cfg.DATA.CROP_SIZE = [96, 64]
    ds = get_dataset(cfg, T.get_transforms(cfg), "train")
    want = _batches(TileLoader, ds, 1, 5)                  # 2 batches per epoch
    for workers in (1, 4):
        got = _batches(DeviceTileLoader, ds, workers, 5)
        for k, ((wi, wl), (gi, gl)) in enumerate(zip(want, got)):
            assert gi.shape == (4, 3, 64, 96) and gl.dtype == torch.int64
            assert torch.equal(gi, wi) and torch.equal(gl, wl), (workers, k, (gi - wi).abs().max().item())


def test_train_cli_with_device_transforms(tmp_path):
    """python -m emrt_amd.train --data dataset --device_transforms on a tiny tree: exit status 0, the device loader in the log, a finite
    loss on every logged step.  (Flips come from the unseeded Python random, so losses are not compared with a CPU-transform run.)"""
    root = _tree(str(tmp_path / "p"), [(80, 80)] * 6 + [(50, 70)] * 2)
    cfg = str(tmp_path / "tiny.yaml")
    with open(cfg, "w") as f:
        f.write('BASE: ["%s"]\n' % os.path.relpath(os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam.yaml"), str(tmp_path)))
        f.write('DATA: {CROP_SIZE: "(64, 64)", BATCH_SIZE: 2, NUM_WORKERS: 2}\n')
        f.write('MODEL: {ENCODER: {TYPE: "resnet18"}}\n')
        f.write("TRAIN: {ITERS: 6}\nSAVE_FREQ_CHECKPOINT: 1000\nLOGGING_INFO_FREQ: 1\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "emrt_amd.train", "--config", cfg, "--data", "dataset", "--data_path", root, "--device_transforms",
                        "--no-eval", "--save_dir", str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[train] data: DeviceTileLoader, 2 reader threads" in r.stdout
    losses = [float(m) for m in re.findall(r"\[TRAIN\].*?loss: ([^,]+),", r.stdout)]
    assert len(losses) == 6 and all(math.isfinite(v) for v in losses), r.stdout[-3000:]
