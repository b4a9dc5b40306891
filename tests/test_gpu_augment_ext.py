"""-m gpu: RandomVerticalFlip and RandomDistort on the device (csrc/augment_ext: emrt_aug_tiles, emrt_aug_scene_draw, emrt_aug_scene_sample).

  tiles    emrt_aug_tiles equals the CPU chain's own classes (PIL's ImageEnhance included) under the same decisions, bit for bit
  draws    the device table equals the Python restatement (tests/test_augment_ext_cpu.py: replay_aug); its geometry columns are emrt_scene_draw's
  scenes   every drawn tile equals the CPU functions on the host copy of its window and the tile-path entry point on a contiguous copy; with no
           vertical flip and no distortion the batch is emrt_scene_sample's
  engine   a captured ResNet-18 step cuts the predicted batch in every replay; the default chain never enters the second library
  loader   DeviceTileLoader with the augment yaml's chain yields the CPU TileLoader's batches

Every comparison is exact."""
import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                                   # noqa: E402
from emrt_amd import functional as Fn                                       # noqa: E402
from emrt_amd.config import get_config, update_config                       # noqa: E402
from emrt_amd.runtime import F32, ctx                                       # noqa: E402
from emrt_amd.src import transforms as T                                    # noqa: E402
from emrt_amd.src.datasets import DeviceTileLoader, SceneBank, SceneSampler, TileLoader, get_dataset, label_lut      # noqa: E402
from tests.test_augment_ext_cpu import OP_NAMES, aug_chain, replay_aug, row_ops      # noqa: E402
from tests.test_scene_sampler_cpu import potsdam_chain, potsdam_scales, replay, write_scene_tree      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "emrt_amd/configs/EMRT")
KEY = 1234
CROP = (64, 48)                 # (w, h): a non-square 48 x 64 crop
OH, OW = 48, 64
LO, HI, MID = 0.6, 1.4, 0.8731


@pytest.fixture
def device():
    ctx().init_device("cuda:0", F32)
    return "cuda:0"


def set_step(step):
    ctx().step_counter.fill_(step)


# ---- tile path ----------------------------------------------------------------------------------------------------------------------------------

def _cpu(chain, img, lab, scale, off, flip, vflip, ops):
    """The CPU chain on float32 / uint8 arrays with its draws forced to the given decisions."""
    chain[0].draw = lambda: scale
    chain[1].draw = lambda ih, iw: None if (ih, iw) == chain[1].size() else off
    chain[2].draw = lambda: bool(flip)
    for t in chain[3:-1]:
        if isinstance(t, T.RandomVerticalFlip):
            t.draw = lambda: bool(vflip)
        else:
            t.draw = lambda: list(ops)
    return T.Compose(chain)(img.astype(np.float32), lab)


def _run(dp, tiles, plans, lut=None):
    chunks, samples, off = [], [], 0
    for (img, lab), p in zip(tiles, plans):
        chunks += [img.reshape(-1), lab.reshape(-1)]
        samples.append((off, off + img.size, p))
        off += img.size + lab.size
    src = torch.from_numpy(np.concatenate(chunks)).cuda()
    out, labels = Fn.aug_tiles(src, samples, (OH, OW), dp.mean, dp.stdinv, dp.img_pad, dp.label_pad, lut, distort=dp.distort is not None)
    torch.cuda.synchronize()
    return out.cpu(), labels.cpu()


def _decisions():
    """[(source index, scale, flip, vflip, ops)]: the four flip combinations at every source and scale; each op alone at lower, upper, 1.0 and an
    interior factor; the six orders of the three ops (contrast first, middle and last)."""
    import itertools
    out = []
    for si in (0, 1):
        for scale in (0.5, 1.0, 2.0):
            for flip, vflip in ((0, 0), (1, 0), (0, 1), (1, 1)):
                out.append((si, scale, flip, vflip, ()))
    k = 0
    for op in OP_NAMES:
        for f in (LO, HI, 1.0, MID):
            out.append((k % 2, (0.5, 1.0, 2.0)[k % 3], k & 1, (k >> 1) & 1, ((op, f),)))      # scale 0.5: the padding enters the contrast mean
            k += 1
    for order in itertools.permutations(zip(OP_NAMES, (0.7, 1.3, 1.1))):
        out.append((k % 2, (0.5, 1.0, 2.0)[k % 3], 1, 1, tuple(order)))
        k += 1
    return out


@pytest.fixture(scope="module")
def tile_cases():
    """Sources 33 x 47 and 80 x 96, crop 48 x 64, pad (0, 0, 0) / 255: (tiles, plans, wanted arrays), the CPU reference computed once."""
    g = np.random.RandomState(7)
    srcs = []
    for H, W in ((33, 47), (80, 96)):
        lab = g.randint(0, 8, (H, W)).astype(np.uint8)
        lab[g.rand(H, W) < 0.05] = 255
        srcs.append((g.randint(0, 256, (H, W, 3)).astype(np.uint8), lab))
    tiles, plans, want = [], [], []
    for si, scale, flip, vflip, ops in _decisions():
        img, lab = srcs[si]
        H, W = lab.shape
        h, w = T.ResizeStepScaling.resized(scale, H, W)
        off = (int(g.randint(max(h, OH) - OH + 1)), int(g.randint(max(w, OW) - OW + 1)))
        tiles.append((img, lab))
        plans.append(T.AugSamplePlan(H, W, h, w, off[0], off[1], flip, vflip, ops))
        want.append(_cpu(aug_chain(CROP), img, lab, scale, off, flip, vflip, ops))
    return tiles, plans, want


def test_tile_path_matches_the_cpu_chain_bit_for_bit(device, tile_cases):
    """One batch of all 42 decisions: three chunks of at most 16, the first without contrast (no statistics launch), the other two mixing samples
    with and without it; a second call is identical."""
    tiles, plans, want = tile_cases
    assert len(plans) == 42 and any(p.h < OH for p in plans) and any(p.h > OH for p in plans)
    dp = T.DevicePlan(aug_chain(CROP))
    got_img, got_lab = _run(dp, tiles, plans)
    for i, (wi, wl) in enumerate(want):
        assert torch.equal(got_img[i], torch.from_numpy(wi)), (plans[i], (got_img[i] - torch.from_numpy(wi)).abs().max().item())
        assert torch.equal(got_lab[i], torch.from_numpy(wl.astype(np.int64))), plans[i]
    again_img, again_lab = _run(dp, tiles, plans)
    assert torch.equal(again_img, got_img) and torch.equal(again_lab, got_lab)


def test_tile_path_batch_of_17_and_label_lut(device, tile_cases):
    """17 samples (one past AUG_CHUNK) mixing samples with and without contrast, through LoveDA's label table."""
    tiles, plans, want = tile_cases
    pick = [0, 24, 25, 28, 29, 5, 30, 36, 37, 9, 38, 39, 40, 41, 13, 32, 31]
    assert len(pick) == 17 and {any(o == "contrast" for o, _ in plans[i].ops) for i in pick} == {True, False}
    assert any(o == "contrast" for o, _ in plans[pick[16]].ops)          # the second launch's only sample sums into sums[16]
    dp = T.DevicePlan(aug_chain(CROP))
    lut = label_lut(1)
    got_img, got_lab = _run(dp, [tiles[i] for i in pick], [plans[i] for i in pick], lut)
    for j, i in enumerate(pick):
        wi, wl = want[i]
        assert torch.equal(got_img[j], torch.from_numpy(wi)), plans[i]
        assert torch.equal(got_lab[j], torch.from_numpy(lut[wl].astype(np.int64))), plans[i]


def test_tile_path_without_distort_does_not_truncate(device, tile_cases):
    """[..., HFlip, VFlip, Normalize]: no RandomDistort in the chain, so the resized float pixels are normalised as they are; a padding value
    that is no integer and a label padding of 7."""
    tiles, plans, _ = tile_cases
    pad, label_pad = (123.675, 116.28, 103.53), 7
    chain = lambda: aug_chain(CROP, distort=False, pad=pad, label_pad=label_pad)
    dp = T.DevicePlan(chain())
    assert dp.extended and dp.distort is None
    sel = list(range(24))
    got_img, got_lab = _run(dp, [tiles[i] for i in sel], [plans[i] for i in sel])
    for j, i in enumerate(sel):
        p = plans[i]
        scale = {(16, 24): 0.5, (33, 47): 1.0, (66, 94): 2.0, (40, 48): 0.5, (80, 96): 1.0, (160, 192): 2.0}[(p.h, p.w)]
        wi, wl = _cpu(chain(), tiles[i][0], tiles[i][1], scale, (p.off_y, p.off_x), p.flip, p.vflip, ())
        assert torch.equal(got_img[j], torch.from_numpy(wi)) and torch.equal(got_lab[j], torch.from_numpy(wl.astype(np.int64))), p


# ---- scene path ---------------------------------------------------------------------------------------------------------------------------------

SCENES = [(70, 90), (66, 95), (81, 88)]
TILE = (24, 40)
RANGES, PROBS = [0.4, 0.4, 0.4], [0.5, 0.5, 0.5]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("augscenes"))
    return root, write_scene_tree(root, SCENES)


def drawn(sampler):
    B, oh, ow = sampler.batch_shape
    images = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=sampler.bank.device)
    labels = torch.empty((B, oh, ow), dtype=torch.int64, device=sampler.bank.device)
    sampler.fill(images, labels)
    torch.cuda.synchronize()
    return sampler.draws.cpu().tolist(), images.cpu(), labels.cpu()


def host_tile(arrays, row, tile, crop, distort=True):
    """One row of the extended draw table applied to the host copy of its window with the CPU chain's own functions."""
    scene, y0, x0, _, h, w, off_y, off_x, flip, vflip = row[:10]
    (th, tw), (oh, ow) = tile, crop
    img, lab = arrays[scene]
    img = img[y0:y0 + th, x0:x0 + tw].astype(np.float32)
    lab = lab[y0:y0 + th, x0:x0 + tw]
    img, lab = T.resize_bilinear(img, w, h), T.resize_nearest(lab, w, h)
    img, lab = _Forced(off_y, off_x, (ow, oh))(img, lab)
    if flip:
        img, lab = img[:, ::-1], lab[:, ::-1]
    if vflip:
        img, lab = img[::-1], lab[::-1]
    if distort:
        img = T.RandomDistort.apply(img, row_ops(row))
    img = T.Normalize(mean=T._MEAN, std=T._STD)(img)[0]
    return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))), torch.from_numpy(np.ascontiguousarray(lab).astype(np.int64))


class _Forced(T.RandomPaddingCrop):
    """RandomPaddingCrop with its offsets given."""

    def __init__(self, off_y, off_x, crop_size):
        super().__init__(crop_size=crop_size, img_padding_value=(0, 0, 0), label_padding_value=255)
        self._off = (off_y, off_x)

    def draw(self, ih, iw):
        return None if (ih, iw) == self.size() else self._off


def _aug_sampler(bank, crop_hw, B=8, key=KEY, rank=0):
    return SceneSampler(bank, aug_chain((crop_hw[1], crop_hw[0])), B, key, rank)


@pytest.mark.parametrize("rank,key", [(0, KEY), (3, 0xFEDCBA9876543210)])
def test_draw_table_equals_the_restatement_and_scene_draws_geometry(tree, device, rank, key):
    root, _ = tree
    bank = SceneBank(root, device)
    s = _aug_sampler(bank, TILE, key=key, rank=rank)
    plain = SceneSampler(bank, potsdam_chain(TILE), 8, key, rank)
    scales = potsdam_scales(TILE)
    assert s.scales == scales and s.draws.shape == (8, 18)
    for step in (0, 1, 2, (1 << 32) + 5):
        set_step(step)
        got, _, _ = drawn(s)
        want = replay_aug(key, step, rank, 8, SCENES, TILE, TILE, scales, 0.5, 0.5, True, RANGES, PROBS)
        assert got == want, (step, rank, got, want)
        old, _, _ = drawn(plain)
        assert [r[:9] for r in got] == [r[:9] for r in old] == [r[:9] for r in replay(key, step, rank, 8, SCENES, TILE, TILE, scales, 0.5)]


def test_scene_tiles_equal_the_cpu_functions_and_the_tile_path(tree, device):
    """Six steps of 8 tiles: each equals the CPU functions on the host copy of its window, and emrt_aug_tiles on a contiguous copy."""
    root, arrays = tree
    bank = SceneBank(root, device)
    s = _aug_sampler(bank, TILE)
    seen_ops, seen_flips = set(), set()
    for step in range(6):
        set_step(step)
        rows, images, labels = drawn(s)
        assert rows == replay_aug(KEY, step, 0, 8, SCENES, TILE, TILE, s.scales, 0.5, 0.5, True, RANGES, PROBS)
        chunks, samples, off = [], [], 0
        for b, r in enumerate(rows):
            wi, wl = host_tile(arrays, r, TILE, TILE)
            assert torch.equal(images[b], wi), (step, r, (images[b] - wi).abs().max().item())
            assert torch.equal(labels[b], wl), (step, r)
            scene, y0, x0, _, h, w, off_y, off_x, flip, vflip = r[:10]
            img, lab = arrays[scene]
            ci = np.ascontiguousarray(img[y0:y0 + TILE[0], x0:x0 + TILE[1]])
            cl = np.ascontiguousarray(lab[y0:y0 + TILE[0], x0:x0 + TILE[1]])
            chunks += [ci.reshape(-1), cl.reshape(-1)]
            samples.append((off, off + ci.size, T.AugSamplePlan(TILE[0], TILE[1], h, w, off_y, off_x, flip, vflip, tuple(row_ops(r)))))
            off += ci.size + cl.size
            seen_ops.add(tuple(o for o, _ in row_ops(r)))
            seen_flips.add((flip, vflip))
        dp = s.plan
        ti, tl = Fn.aug_tiles(torch.from_numpy(np.concatenate(chunks)).cuda(), samples, TILE, dp.mean, dp.stdinv, dp.img_pad, dp.label_pad, None)
        torch.cuda.synchronize()
        assert torch.equal(ti.cpu(), images) and torch.equal(tl.cpu(), labels), step
    assert seen_flips == {(0, 0), (0, 1), (1, 0), (1, 1)} and any("contrast" in o for o in seen_ops) and () in seen_ops


def test_no_vflip_no_distort_equals_scene_sample(tree, device):
    """The new entry points with vflip_prob = 0 and distort = 0 write emrt_scene_sample's batch."""
    root, _ = tree
    bank = SceneBank(root, device)
    plain = SceneSampler(bank, potsdam_chain(TILE), 8, KEY, 0)
    A = _lib.augment_lib()
    scenes_dev, cum_dev, scenes_host, cum_host = bank.tables(*TILE)
    c = ctx()
    zeros = (ctypes.c_double * 3)(0, 0, 0)
    draws = torch.zeros((8, 18), dtype=torch.int32, device=device)
    images = torch.empty((8, 3) + TILE, dtype=torch.float32, device=device)
    labels = torch.empty((8,) + TILE, dtype=torch.int64, device=device)
    for step in (0, 3):
        set_step(step)
        _, want_i, want_l = drawn(plain)
        A.call("emrt_aug_scene_draw", Fn.P(c.step_counter), Fn.P(scenes_dev), Fn.P(cum_dev), ctypes.cast(scenes_host, ctypes.c_void_p),
               ctypes.cast(cum_host, ctypes.c_void_p), len(bank), bank.nbytes, KEY, 0, 8, TILE[0], TILE[1], TILE[0], TILE[1], 0.5, 0.0, 0, zeros, zeros,
               ctypes.cast(plain._scale_hw, ctypes.c_void_p), len(plain.scales), Fn.P(draws), c.stream)
        A.call("emrt_aug_scene_sample", Fn.P(bank.buffer), bank.nbytes, Fn.P(scenes_dev), ctypes.cast(scenes_host, ctypes.c_void_p), len(bank),
               Fn.P(draws), 8, TILE[0], TILE[1], TILE[0], TILE[1], 0, ctypes.cast(plain._mean, ctypes.c_void_p),
               ctypes.cast(plain._stdinv, ctypes.c_void_p), ctypes.cast(plain._pad, ctypes.c_void_p), 255, None, Fn.P(images), 3 * TILE[0] * TILE[1],
               Fn.P(labels), None, 0, c.stream)
        torch.cuda.synchronize()
        assert torch.equal(images.cpu(), want_i) and torch.equal(labels.cpu(), want_l), step
        assert all(r[9] == 0 and r[11] == 0 for r in draws.cpu().tolist())


# ---- engine -------------------------------------------------------------------------------------------------------------------------------------

ENGINE_SIZES = [(96, 80), (96, 80)]


class _Spy:
    """Counts the calls that reach the second library."""

    def __init__(self, inner):
        self.inner, self.names = inner, []

    def call(self, name, *args):
        self.names.append(name)
        return self.inner.call(name, *args)

    def query(self, name, *args):
        self.names.append(name)
        return self.inner.query(name, *args)


def _engine(root, state, use_graph, chain):
    from emrt_amd.engine import TrainEngine
    from emrt_amd.src.models import get_model
    from emrt_amd.src.models.losses import get_loss_function
    from emrt_amd.src.models.solver import get_optimizer, get_scheduler
    from tests.test_gpu_model import make_config
    cfg = make_config("resnet18", iters=1000)
    model = get_model(cfg)
    model.load_state_dict(state)
    model.to_hip("cuda:0", F32)
    model.set_dropout(0.0)
    model.eval()
    model(torch.zeros(2, 3, 64, 64, device="cuda:0"))      # the shape-keyed constants are uploaded outside the capture
    model.train()
    opt = get_optimizer(model, get_scheduler(cfg), cfg)
    set_step(0)
    source = SceneSampler(SceneBank(root, "cuda:0"), chain, 2, KEY, 0)
    return model, TrainEngine(model, opt, get_loss_function(cfg), 1, use_graph=use_graph, warmup_eager=0, batch_source=source)


def test_captured_step_cuts_the_predicted_augmented_batch(tmp_path, monkeypatch):
    """ResNet-18, batch 2, 64 x 64, fp32, 3 steps eager and captured from the same weights: after every step the engine's batch is the one rebuilt
    on the host from the restated draws at that step's counter (the graph was captured at counter 0), and the losses agree."""
    root = str(tmp_path / "s")
    arrays = write_scene_tree(root, ENGINE_SIZES)
    scales = potsdam_scales((64, 64))
    torch.manual_seed(3)
    from oracle.emrt_torch import EMRT as OracleEMRT
    state = {k: v.clone() for k, v in OracleEMRT(6, "resnet18").state_dict().items()}
    losses = {}
    for mode in ("eager", "graph"):
        model, eng = _engine(root, state, mode == "graph", aug_chain((64, 64)))
        losses[mode] = []
        for step in range(3):
            losses[mode].append(eng.step().item())
            torch.cuda.synchronize()
            rows = replay_aug(KEY, step, 0, 2, ENGINE_SIZES, (64, 64), (64, 64), scales, 0.5, 0.5, True, RANGES, PROBS)
            assert eng.batch_source.draws.cpu().tolist() == rows, (mode, step)
            for b, r in enumerate(rows):
                wi, wl = host_tile(arrays, r, (64, 64), (64, 64))
                assert torch.equal(eng.images[b].cpu(), wi) and torch.equal(eng.labels[b].cpu(), wl), (mode, step, r)
        if mode == "graph":
            assert eng.graph_a is not None and eng.graph_a.n_graphs == 1 and eng.calls == 3
        del eng, model
    print("augmented scene steps, eager %s captured %s" % (["%.6f" % v for v in losses["eager"]], ["%.6f" % v for v in losses["graph"]]))
    assert all(math.isfinite(v) and v > 0 for v in losses["eager"] + losses["graph"])
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) / max(1.0, abs(a)) < 1e-3, losses
    # the default chain: nothing reaches the second library
    spy = _Spy(_lib.augment_lib())
    monkeypatch.setattr(_lib, "_AUG_LIB", spy)
    plain = SceneSampler(SceneBank(root, "cuda:0"), potsdam_chain((64, 64)), 2, KEY, 0)
    drawn(plain)
    assert spy.names == []
    drawn(SceneSampler(SceneBank(root, "cuda:0"), aug_chain((64, 64)), 2, KEY, 0))
    assert spy.names == ["emrt_aug_scene_draw", "emrt_aug_scene_sample"]


# ---- loader -------------------------------------------------------------------------------------------------------------------------------------

def test_device_loader_matches_cpu_loader_with_the_augment_yaml(tmp_path):
    """Eight Potsdam tiles of mixed sizes under the augment yaml's chain: DeviceTileLoader with 1 and 4 reader threads yields the batches of the
    CPU TileLoader (PIL's ImageEnhance) from the same seeds, one epoch and the first batch of the next."""
    from tests.test_gpu_device_transforms import _batches, _tree
    sizes = [(80, 96), (130, 70), (64, 64), (255, 257), (40, 100), (96, 80), (64, 64), (70, 130)]
    root = _tree(str(tmp_path / "p"), sizes)
    cfg = update_config(get_config(), argparse.Namespace(cfg=os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam_augment.yaml")))
    cfg.DATA.DATA_PATH = root
    cfg.DATA.CROP_SIZE = [96, 64]
    chain = T.get_transforms(cfg)
    assert [type(t).__name__ for t in chain][3:5] == ["RandomVerticalFlip", "RandomDistort"]
    ds = get_dataset(cfg, chain, "train")
    want = _batches(TileLoader, ds, 1, 3)
    for workers in (1, 4):
        got = _batches(DeviceTileLoader, ds, workers, 3)
        for k, ((wi, wl), (gi, gl)) in enumerate(zip(want, got)):
            assert gi.shape == (4, 3, 64, 96) and gl.dtype == torch.int64
            assert torch.equal(gi, wi) and torch.equal(gl, wl), (workers, k, (gi - wi).abs().max().item())
