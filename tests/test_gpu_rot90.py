"""-m gpu: the quarter turn of the training augmentation on the device (csrc/rot_ext: emrt_rot_batch, emrt_rot_scene_batch).
Everything is compared bit for bit, through int32 / int64 views.

  kernel    emrt_rot_batch against torch.rot90 of the host copy: every n that takes another path through the 32 x 32 tiling, random bits with NaN
            payloads, labels with 255, labels = NULL, a batch above a chunk; images, labels and turns sit inside sentinel-filled allocations whose
            margins stay untouched
  tiles     a seeded DeviceTileLoader equals the CPU TileLoader under the four new chains
  scenes    turns_out equals the restated block-5 draw; the batch with ROT90_PROB 0.75 is the batch with ROT90_PROB 0 turned on the host
  capture   three captured steps hold the predicted batches, captured and eager losses agree, a fresh engine at counter 2 cuts the third batch"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                                   # noqa: E402
from emrt_amd import functional as Fn                                       # noqa: E402
from emrt_amd.runtime import F32, ctx                                       # noqa: E402
from emrt_amd.src import transforms as T                                    # noqa: E402
from emrt_amd.src.datasets import DeviceTileLoader, SceneBank, SceneSampler, TileLoader, get_dataset      # noqa: E402
from tests.test_rot90_cpu import KEY, _cfg, rot_chain, rot_turns            # noqa: E402
from tests.test_scene_sampler_cpu import SIZES, potsdam_chain, potsdam_scales, replay, write_scene_tree      # noqa: E402

MARGIN = 1024                      # sentinel elements on either side of every buffer
SENTINEL_32, SENTINEL_64, SENTINEL_TURN = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
NAN_PATTERNS = [0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFFFFFFF - (1 << 32), 0xFF800001 - (1 << 32), 0x7FFFFFFF]      # quiet, payload, signalling, negative


@pytest.fixture
def device():
    ctx().init_device("cuda:0", F32)
    return "cuda:0"


def set_step(step):
    ctx().step_counter.fill_(step)


def _payload(B, n, seed):
    """Host int32 [B, 3, n, n] of random bits with the NaN patterns planted, and int64 [B, n, n] labels of random values with 255."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(-(1 << 31), (1 << 31) - 1, (B, 3, n, n), generator=g, dtype=torch.int64).to(torch.int32)
    flat = img.view(-1)
    at = torch.randperm(flat.numel(), generator=g)[:min(flat.numel(), 4 * len(NAN_PATTERNS))]
    flat[at] = torch.tensor(NAN_PATTERNS, dtype=torch.int32).repeat(4)[:at.numel()]
    lab = torch.randint(-(1 << 62), 1 << 62, (B, n, n), generator=g, dtype=torch.int64)
    lab[torch.rand(B, n, n, generator=g) < 0.3] = 255
    return img, lab


def _turned(x, turns):
    """torch.rot90 of each sample of the host copy by its turn, over the last two dimensions."""
    return torch.stack([torch.rot90(x[b], int(k), dims=(-2, -1)) for b, k in enumerate(turns)])


def _rot_batch_in_margins(B, n, turns, with_labels=True, seed=0):
    """emrt_rot_batch on buffers that sit inside sentinel-filled allocations -> (images int32, labels int64 or None) on the host, after the margins
    of all three allocations were found unchanged."""
    img, lab = _payload(B, n, seed)
    big_i = torch.full((2 * MARGIN + img.numel(),), SENTINEL_32, dtype=torch.int32, device="cuda")
    big_l = torch.full((2 * MARGIN + lab.numel(),), SENTINEL_64, dtype=torch.int64, device="cuda")
    di, dl = big_i[MARGIN:MARGIN + img.numel()], big_l[MARGIN:MARGIN + lab.numel()]
    di.copy_(img.view(-1))
    dl.copy_(lab.view(-1))
    host = (ctypes.c_int * (B + 2 * 16))(*([SENTINEL_TURN] * 16 + [int(k) for k in turns] + [SENTINEL_TURN] * 16))
    tptr = ctypes.c_void_p(ctypes.addressof(host) + 16 * ctypes.sizeof(ctypes.c_int))
    _lib.rot_lib().call("emrt_rot_batch", ctypes.c_void_p(di.data_ptr()), ctypes.c_void_p(dl.data_ptr()) if with_labels else None, tptr, B, n,
                        ctx().stream)
    torch.cuda.synchronize()
    for big, sentinel, count in ((big_i, SENTINEL_32, img.numel()), (big_l, SENTINEL_64, lab.numel())):
        h = big.cpu()
        assert bool((h[:MARGIN] == sentinel).all()) and bool((h[MARGIN + count:] == sentinel).all()), (B, n, "a margin was written")
    assert list(host[:16]) == [SENTINEL_TURN] * 16 and list(host[16 + B:]) == [SENTINEL_TURN] * 16 and list(host[16:16 + B]) == [int(k) for k in turns]
    return img, lab, di.cpu().view(B, 3, n, n), dl.cpu().view(B, n, n)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 97, 256])
def test_rot_batch_equals_torch_rot90_bit_for_bit(device, n):
    """Odd and even n, one tile, the tile edge +- 1 (the domain of n = 63..65 is 32 x 31, 32 x 32, 33 x 32: one tile, one tile, a second row of
    one line), partial edge tiles, the fixed centre pixel, and 256 (the training crop: 16 tiles a plane); B = 5 with every turn."""
    turns = [0, 1, 2, 3, 1]
    img, lab, got_i, got_l = _rot_batch_in_margins(5, n, turns, seed=n)
    assert torch.equal(got_i, _turned(img, turns)) and torch.equal(got_l, _turned(lab, turns))
    assert torch.equal(got_i[0], img[0]) and torch.equal(got_l[0], lab[0])          # turn 0: untouched
    if n > 1:
        assert not torch.equal(got_i[1], img[1])


def test_rot_batch_without_labels_and_above_a_chunk(device):
    """labels = NULL: the images are turned and the label buffer keeps every bit.  B = 70 is a chunk of 64 and one of 6; B = 130 has a middle
    chunk whose turns are all 0 (no launch for it)."""
    turns = [0, 1, 2, 3, 1]
    img, lab, got_i, got_l = _rot_batch_in_margins(5, 33, turns, with_labels=False, seed=1)
    assert torch.equal(got_i, _turned(img, turns)) and torch.equal(got_l, lab)
    g = np.random.RandomState(2)
    turns = g.randint(0, 4, 70).tolist()
    assert set(turns[64:]) > {0} and len(set(turns[:64])) == 4
    img, lab, got_i, got_l = _rot_batch_in_margins(70, 5, turns, seed=2)
    assert torch.equal(got_i, _turned(img, turns)) and torch.equal(got_l, _turned(lab, turns))
    turns = [3] * 64 + [0] * 64 + [2, 1]
    img, lab, got_i, got_l = _rot_batch_in_margins(130, 4, turns, seed=3)
    assert torch.equal(got_i, _turned(img, turns)) and torch.equal(got_l, _turned(lab, turns))


def test_functional_rot_batch_turns_in_place(device):
    img, lab = _payload(3, 24, 9)
    di, dl = img.view(torch.float32).cuda(), lab.cuda()
    oi, ol = Fn.rot_batch(di, dl, [1, 0, 3])
    torch.cuda.synchronize()
    assert oi.data_ptr() == di.data_ptr() and ol.data_ptr() == dl.data_ptr()
    assert torch.equal(di.cpu().view(torch.int32), _turned(img, [1, 0, 3])) and torch.equal(dl.cpu(), _turned(lab, [1, 0, 3]))
    with pytest.raises(_lib.EmrtHipError, match=r"turns\[1\] is 4"):
        Fn.rot_batch(di, dl, [1, 4, 3])
    with pytest.raises(ValueError, match="contiguous fp32"):
        Fn.rot_batch(di[:, :, :, :12], None, [0, 0, 0])


# ---- the tile path ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vflip,distort", [(False, False), (True, False), (False, True), (True, True)])
def test_device_loader_matches_cpu_loader_under_the_new_chains(tmp_path, monkeypatch, vflip, distort):
    """Eight Potsdam tiles of mixed sizes, a 24 x 24 crop, ROT90_PROB 0.75 with / without the vertical flip and the distortion (contrast at
    probability 1: its degenerate is a sum over the whole tile): DeviceTileLoader yields the batches of the CPU TileLoader (np.rot90, PIL's
    ImageEnhance) from the same seeds, bit for bit, one epoch and the first batch of the next."""
    from tests.test_gpu_device_transforms import _batches, _tree
    sizes = [(80, 96), (30, 70), (24, 24), (55, 57), (40, 100), (96, 80), (64, 64), (70, 30)]
    root = _tree(str(tmp_path / "p"), sizes)
    cfg = _cfg()
    cfg.DATA.DATA_PATH = root
    cfg.DATA.CROP_SIZE = [24, 24]
    cfg.DATA.AUGMENT.ROT90_PROB = 0.75
    cfg.DATA.AUGMENT.VFLIP_PROB = 0.5 if vflip else 0.0
    cfg.DATA.AUGMENT.DISTORT.ENABLE = distort
    cfg.DATA.AUGMENT.DISTORT.CONTRAST_PROB = 1.0
    chain = T.get_transforms(cfg)
    assert [type(t).__name__ for t in chain][3:-1] == ["RandomVerticalFlip"] * vflip + ["RandomRot90"] + ["RandomDistort"] * distort
    ds = get_dataset(cfg, chain, "train")
    want = _batches(TileLoader, ds, 1, 3)
    seen, real = [], Fn.rot_batch
    monkeypatch.setattr(Fn, "rot_batch", lambda images, labels, turns: (seen.extend(turns), real(images, labels, turns))[1])
    for workers in (1, 4):
        got = _batches(DeviceTileLoader, ds, workers, 3)
        for k, ((wi, wl), (gi, gl)) in enumerate(zip(want, got)):
            assert gi.shape == (4, 3, 24, 24) and gl.dtype == torch.int64
            assert torch.equal(gi.view(torch.int32), wi.view(torch.int32)) and torch.equal(gl, wl), (workers, k, (gi - wi).abs().max().item())
    assert len(seen) == 24 and set(seen) <= {0, 1, 2, 3} and any(seen), seen          # (3 batches of 4, twice: the post-pass ran, and turned)


# ---- the scene path -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("scenes"))
    return root, write_scene_tree(root, SIZES)


def drawn(sampler):
    """One fill on fresh buffers -> (images, labels) on the host."""
    B, OH, OW = sampler.batch_shape
    images = torch.empty((B, 3, OH, OW), dtype=torch.float32, device=sampler.bank.device)
    labels = torch.empty((B, OH, OW), dtype=torch.int64, device=sampler.bank.device)
    sampler.fill(images, labels)
    torch.cuda.synchronize()
    return images.cpu(), labels.cpu()


CLASS_NODE = {"MODE": "class", "PROB": 0.5, "TEMPERATURE": 0.1, "CLASS_PROBS": None}


@pytest.mark.parametrize("kind", ["plain", "extended", "class"])
@pytest.mark.parametrize("rank", [0, 3])
def test_scene_batch_is_the_unturned_batch_turned_by_the_restated_draw(tree, device, kind, rank):
    """Steps 0, 1, 2 and 2^32 + 5 (the counter's high word), ranks 0 and 3, B = 8, a 32 x 32 crop: turns_out equals the Python restatement of the
    block-5 draw, and the batch equals the batch of the same chain without RandomRot90 -- every other Philox block is untouched, so every other
    decision is equal -- turned on the host by those turns.  Plain chain; extended chain with contrast at probability 1; class mode."""
    root, _ = tree
    bank = SceneBank(root, device)
    if kind == "extended":
        with_rot = rot_chain((32, 32), vflip=0.5, distort=True, prob=1.0)
        without = [t for t in rot_chain((32, 32), vflip=0.5, distort=True, prob=1.0) if not isinstance(t, T.RandomRot90)]
    else:
        with_rot = rot_chain((32, 32), vflip=None, distort=False)
        without = potsdam_chain((32, 32))
    kw = dict(sampling=CLASS_NODE, num_classes=6) if kind == "class" else {}
    s, base = SceneSampler(bank, with_rot, 8, KEY, rank, **kw), SceneSampler(bank, without, 8, KEY, rank, **kw)
    assert s.class_mode == (kind == "class") and s.plan.extended == (kind == "extended") and base.turns is None
    seen = set()
    for step in (0, 1, 2, (1 << 32) + 5):
        set_step(step)
        want_turns = rot_turns(KEY, step, rank, 8, 0.75)
        gi, gl = drawn(s)
        assert s.turns.cpu().tolist() == want_turns, (step, rank)
        bi, bl = drawn(base)
        assert torch.equal(s.draws.cpu(), base.draws.cpu())
        assert torch.equal(gi.view(torch.int32), _turned(bi.view(torch.int32), want_turns)) and torch.equal(gl, _turned(bl, want_turns)), (step, rank)
        again_i, again_l = drawn(s)
        assert torch.equal(again_i.view(torch.int32), gi.view(torch.int32)) and torch.equal(again_l, gl)
        assert int(ctx().step_counter.item()) == step
        seen |= set(want_turns)
    assert seen == {0, 1, 2, 3}


def test_scene_batch_follows_the_64_bit_key_and_the_probability(tree, device):
    root, _ = tree
    bank = SceneBank(root, device)
    key = 0xFEDCBA9876543210
    set_step(9)
    for prob in (0.0, 0.3, 1.0):
        s = SceneSampler(bank, rot_chain((32, 32), vflip=None, distort=False, rot=prob), 8, key, 1) if prob else None
        if s is None:          # probability 0 through the entry point itself (the chain builder leaves the op out)
            s = SceneSampler(bank, rot_chain((32, 32), vflip=None, distort=False, rot=0.5), 8, key, 1)
            s.rot_prob = 0.0
        drawn(s)
        assert s.turns.cpu().tolist() == rot_turns(key, 9, 1, 8, prob), prob


# ---- capture ------------------------------------------------------------------------------------------------------------------------------------

ENGINE_SIZES = [(96, 80), (96, 80)]


def _engine(root, state, use_graph, start_step=0):
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
    set_step(start_step)
    source = SceneSampler(SceneBank(root, "cuda:0"), rot_chain((64, 64), vflip=None, distort=False), 2, KEY, 0)
    return model, TrainEngine(model, opt, get_loss_function(cfg), 1, use_graph=use_graph, warmup_eager=0, batch_source=source)


def test_captured_step_turns_the_predicted_batch_and_resumes(tmp_path):
    """The check of tests/test_gpu_scene_sampler.py with the key on: ResNet-18, batch 2, 64 x 64 out of two 96 x 80 scenes, 3 steps eager and
    captured from the same weights.  After every step the engine's batch is the one rebuilt on the host from the replay at that step's counter,
    turned by the restated block-5 draw (the graph was captured at counter 0: steps 1 and 2 prove that a replay reads the counter on the device).
    A fresh engine whose counter is set to 2 cuts the third batch."""
    from tests.test_gpu_scene_sampler import host_batch
    root = str(tmp_path / "s")
    arrays = write_scene_tree(root, ENGINE_SIZES)
    scales = potsdam_scales((64, 64))
    torch.manual_seed(3)
    from oracle.emrt_torch import EMRT as OracleEMRT
    state = {k: v.clone() for k, v in OracleEMRT(6, "resnet18").state_dict().items()}
    all_turns = [rot_turns(KEY, step, 0, 2, 0.75) for step in range(3)]
    assert any(k for t in all_turns for k in t), all_turns          # the three batches hold a turned sample
    losses, third = {}, None
    for mode in ("eager", "graph"):
        model, eng = _engine(root, state, use_graph=(mode == "graph"))
        losses[mode] = []
        for step in range(3):
            assert int(ctx().step_counter.item()) == step
            losses[mode].append(eng.step().item())
            torch.cuda.synchronize()
            rows = replay(KEY, step, 0, 2, ENGINE_SIZES, (64, 64), (64, 64), scales, 0.5)
            assert eng.batch_source.draws.cpu().tolist() == rows and eng.batch_source.turns.cpu().tolist() == all_turns[step], (mode, step)
            want_i, want_l = host_batch(arrays, rows, (64, 64), (64, 64))
            want_i, want_l = _turned(want_i, all_turns[step]), _turned(want_l, all_turns[step])
            assert torch.equal(eng.images.cpu(), want_i) and torch.equal(eng.labels.cpu(), want_l), (mode, step)
            third = (want_i, want_l)
        if mode == "graph":
            assert eng.graph_a is not None and eng.graph_a.n_graphs == 1 and eng.calls == 3
        del eng, model
    print("turned scene steps, turns %r, eager %s captured %s" % (all_turns, ["%.6f" % v for v in losses["eager"]], ["%.6f" % v for v in losses["graph"]]))
    assert all(math.isfinite(v) and v > 0 for v in losses["eager"] + losses["graph"])
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) / max(1.0, abs(a)) < 1e-3, losses
    model, eng = _engine(root, state, use_graph=True, start_step=2)
    eng.step()
    torch.cuda.synchronize()
    assert torch.equal(eng.images.cpu(), third[0]) and torch.equal(eng.labels.cpu(), third[1])
    assert int(ctx().step_counter.item()) == 3
