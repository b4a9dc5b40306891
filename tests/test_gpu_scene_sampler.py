"""-m gpu: the device-side tile sampler (csrc/augment.hip: emrt_scene_draw, emrt_scene_sample) behind `train.py --data scenes`.

  draws    the device table equals the pure-Python restatement of the draw procedure (tests/test_scene_sampler_cpu.py: replay) exactly
  sample   every drawn tile equals the CPU transform functions applied to the host copy of its window, bit for bit, and equals the existing
           emrt_augment_tiles kernel on a contiguous copy of the window
  engine   TrainEngine(batch_source=...) cuts a new batch in every replay of the captured step (the counter is read on the device), the
           captured and the eager run agree, and restoring the step counter resumes the same data stream
  CLI      train.main --data scenes runs and checkpoints

One bank for all of it: three scenes of 40x56, 33x47 and 64x64, as in the CPU distribution check."""
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import functional as Fn                                       # noqa: E402
from emrt_amd.runtime import F32, ctx                                       # noqa: E402
from emrt_amd.src import transforms as T                                    # noqa: E402
from emrt_amd.src.datasets import SceneBank, SceneSampler, label_lut        # noqa: E402
from tests.test_scene_sampler_cpu import SIZES, potsdam_chain, potsdam_scales, replay, write_scene_tree      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "emrt_amd/configs/EMRT")
KEY = 1234


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """(root, [(img uint8 HWC, lab uint8 HW)]) of the three-scene bank; labels 0..5 and 255."""
    root = str(tmp_path_factory.mktemp("scenes"))
    return root, write_scene_tree(root, SIZES)


@pytest.fixture
def device():
    ctx().init_device("cuda:0", F32)
    return "cuda:0"


def set_step(step):
    ctx().step_counter.fill_(step)


def drawn(sampler):
    """One fill on fresh buffers -> (draw rows, images, labels) on the host."""
    B, OH, OW = sampler.batch_shape
    images = torch.empty((B, 3, OH, OW), dtype=torch.float32, device=sampler.bank.device)
    labels = torch.empty((B, OH, OW), dtype=torch.int64, device=sampler.bank.device)
    sampler.fill(images, labels)
    torch.cuda.synchronize()
    return sampler.draws.cpu().tolist(), images.cpu(), labels.cpu()


def host_tile(arrays, row, tile, crop, pad, label_pad, lut):
    """One row of the draw table applied to the host copy of its window with the CPU chain's own functions:
    resize_bilinear / resize_nearest -> pad bottom / right -> crop -> flip -> Normalize (+ the label lookup table)."""
    scene, y0, x0, _, h, w, off_y, off_x, flip, _ = row
    (th, tw), (OH, OW) = tile, crop
    img, lab = arrays[scene]
    img = img[y0:y0 + th, x0:x0 + tw].astype(np.float32)
    lab = lab[y0:y0 + th, x0:x0 + tw]
    img, lab = T.resize_bilinear(img, w, h), T.resize_nearest(lab, w, h)
    ph, pw = max(OH - h, 0), max(OW - w, 0)
    if ph or pw:
        pi = np.empty((h + ph, w + pw, 3), dtype=np.float32)
        pi[...] = np.asarray(pad, dtype=np.float32)
        pi[:h, :w] = img
        pl = np.full((h + ph, w + pw), label_pad, dtype=np.uint8)
        pl[:h, :w] = lab
        img, lab = pi, pl
    img, lab = img[off_y:off_y + OH, off_x:off_x + OW], lab[off_y:off_y + OH, off_x:off_x + OW]
    if flip:
        img, lab = img[:, ::-1], lab[:, ::-1]
    img = T.Normalize(mean=T._MEAN, std=T._STD)(img)[0]
    if lut is not None:
        lab = lut[lab]
    return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))), torch.from_numpy(np.ascontiguousarray(lab).astype(np.int64))


def host_batch(arrays, rows, tile, crop, pad=(0, 0, 0), label_pad=255, lut=None):
    tiles = [host_tile(arrays, r, tile, crop, pad, label_pad, lut) for r in rows]
    return torch.stack([t[0] for t in tiles]), torch.stack([t[1] for t in tiles])


def covering_steps(sizes, tile, crop, scales, prob, B=8, need=None):
    """The first steps whose replayed draws, together, hold every (scale index, flip) pair."""
    need = set(need or {(k, f) for k in range(len(scales)) for f in ((0, 1) if prob > 0 else (0,))})
    steps = []
    for step in range(200):
        got = {(r[3], r[8]) for r in replay(KEY, step, 0, B, sizes, tile, crop, scales, prob)} & need
        if got:
            steps.append(step)
            need -= got
        if not need:
            return steps
    raise AssertionError("200 steps do not cover %r" % sorted(need))


# ---- draws --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rank", [0, 3])
def test_draws_equal_the_replay_exactly(tree, device, rank):
    """Steps 0, 1, 2 and 2^32 + 5 (the counter's high word), ranks 0 and 3, B = 8; a second launch at the same step is bit-identical."""
    root, _ = tree
    bank = SceneBank(root, device)
    s = SceneSampler(bank, potsdam_chain((32, 32)), 8, KEY, rank)
    for step in (0, 1, 2, (1 << 32) + 5):
        set_step(step)
        got, _, _ = drawn(s)
        want = replay(KEY, step, rank, 8, SIZES, (32, 32), (32, 32), potsdam_scales((32, 32)), 0.5)
        assert got == want, (step, rank, got, want)
        again, _, _ = drawn(s)
        assert again == got
        assert int(ctx().step_counter.item()) == step          # the sampler reads the counter, it does not advance it


def test_draws_follow_the_64_bit_key(tree, device):
    root, _ = tree
    bank = SceneBank(root, device)
    key = 0xFEDCBA9876543210                                    # both key words in use, top bit set (travels as a negative long long)
    s = SceneSampler(bank, potsdam_chain((32, 32)), 8, key, 1)
    set_step(9)
    got, _, _ = drawn(s)
    assert got == replay(key, 9, 1, 8, SIZES, (32, 32), (32, 32), potsdam_scales((32, 32)), 0.5)


# ---- sample kernel ------------------------------------------------------------------------------------------------------------------------------

def _check_against_host(s, arrays, steps, tile, crop, lut=None):
    seen = set()
    for step in steps:
        set_step(step)
        rows, images, labels = drawn(s)
        assert rows == replay(KEY, step, 0, s.batch_size, SIZES, tile, crop, s.scales, s.flip_prob)
        want_i, want_l = host_batch(arrays, rows, tile, crop, lut=lut)
        for b, r in enumerate(rows):
            assert torch.equal(images[b], want_i[b]), (step, r, (images[b] - want_i[b]).abs().max().item())
            assert torch.equal(labels[b], want_l[b]), (step, r)
            seen.add((r[3], r[8]))
    return seen


def test_sample_kernel_matches_the_cpu_chain_bit_for_bit(tree, device):
    """32 x 32 tile and crop: every scale index (16 .. 64: padding below the crop, offsets above it) with both flips."""
    root, arrays = tree
    s = SceneSampler(SceneBank(root, device), potsdam_chain((32, 32)), 8, KEY, 0)
    steps = covering_steps(SIZES, (32, 32), (32, 32), s.scales, 0.5)
    seen = _check_against_host(s, arrays, steps, (32, 32), (32, 32))
    assert seen == {(k, f) for k in range(7) for f in (0, 1)}


def test_sample_kernel_non_square_tile(tmp_path, device):
    """A 24 x 40 tile and crop out of the 40 x 56 scene: 17 x 17 origins, rows and columns of different lengths everywhere."""
    sub = str(tmp_path / "one")
    one = write_scene_tree(sub, SIZES[:1])
    s = SceneSampler(SceneBank(sub, device), potsdam_chain((24, 40)), 8, KEY, 0)
    assert s.tile == (24, 40) and s.total_origins == 17 * 17
    sizes = SIZES[:1]
    seen = set()
    for step in covering_steps(sizes, (24, 40), (24, 40), s.scales, 0.5):
        set_step(step)
        rows, images, labels = drawn(s)
        assert rows == replay(KEY, step, 0, 8, sizes, (24, 40), (24, 40), s.scales, 0.5)
        want_i, want_l = host_batch(one, rows, (24, 40), (24, 40))
        assert torch.equal(images, want_i) and torch.equal(labels, want_l), step
        seen |= {(r[3], r[8]) for r in rows}
    assert seen == {(k, f) for k in range(7) for f in (0, 1)}


def test_sample_kernel_lovedas_chain(tmp_path, device):
    """[Normalize] alone with LoveDA's label shift: label values 0 (ignore -> 255), 1..7 and 255 (stays 255) are all present."""
    root = str(tmp_path / "loveda")
    arrays = write_scene_tree(root, SIZES, label_values=[0, 1, 2, 3, 4, 5, 6, 7])
    assert all((lab == 0).any() and (lab == 255).any() for _, lab in arrays)
    s = SceneSampler(SceneBank(root, device, label_shift=1), [T.Normalize(mean=T._MEAN, std=T._STD)], 8, KEY, 0, tile=(32, 32))
    for step in (0, 1):
        set_step(step)
        rows, images, labels = drawn(s)
        assert rows == replay(KEY, step, 0, 8, SIZES, (32, 32), (32, 32), [(32, 32)], 0.0)
        assert all(r[3:] == [0, 32, 32, 0, 0, 0, 0] for r in rows)
        want_i, want_l = host_batch(arrays, rows, (32, 32), (32, 32), lut=label_lut(1))
        assert torch.equal(images, want_i) and torch.equal(labels, want_l)
        assert (labels == 255).any() and (labels == 6).any() and (labels == 0).any() and int(labels[labels != 255].max()) == 6


def test_sample_kernel_equals_the_tile_kernel_on_contiguous_windows(tree, device):
    """Same decisions, the windows copied out contiguously and run through emrt_augment_tiles: equal bit for bit."""
    root, arrays = tree
    bank = SceneBank(root, device)
    s = SceneSampler(bank, potsdam_chain((32, 32)), 8, KEY, 0)
    for step in covering_steps(SIZES, (32, 32), (32, 32), s.scales, 0.5)[:3]:
        set_step(step)
        rows, images, labels = drawn(s)
        chunks, samples, off = [], [], 0
        for scene, y0, x0, _, h, w, off_y, off_x, flip, _ in rows:
            img, lab = arrays[scene]
            wi, wl = np.ascontiguousarray(img[y0:y0 + 32, x0:x0 + 32]), np.ascontiguousarray(lab[y0:y0 + 32, x0:x0 + 32])
            chunks += [wi.reshape(-1), wl.reshape(-1)]
            samples.append((off, off + wi.size, T.SamplePlan(32, 32, h, w, off_y, off_x, flip)))
            off += wi.size + wl.size
        dp = s.plan
        ti, tl = Fn.augment_tiles(torch.from_numpy(np.concatenate(chunks)).cuda(), samples, (32, 32), dp.mean, dp.stdinv, dp.img_pad, dp.label_pad, None)
        torch.cuda.synchronize()
        assert torch.equal(ti.cpu(), images) and torch.equal(tl.cpu(), labels), step


# ---- engine -------------------------------------------------------------------------------------------------------------------------------------

ENGINE_SIZES = [(96, 80), (96, 80)]


def _engine(root, state, use_graph, start_step=0):
    from emrt_amd.engine import TrainEngine
    from emrt_amd.src.models import get_model
    from emrt_amd.src.models.losses import get_loss_function
    from emrt_amd.src.models.solver import get_optimizer, get_scheduler
    from tests.test_gpu_model import make_config
    cfg = make_config("resnet18", iters=1000)
    model = get_model(cfg)
    if state is not None:
        model.load_state_dict(state)
    model.to_hip("cuda:0", F32)
    model.set_dropout(0.0)
    model.eval()
    model(torch.zeros(2, 3, 64, 64, device="cuda:0"))      # the shape-keyed constants are uploaded outside the capture (tests/test_gpu_captured_step.py)
    model.train()
    opt = get_optimizer(model, get_scheduler(cfg), cfg)
    set_step(start_step)
    bank = SceneBank(root, "cuda:0")
    source = SceneSampler(bank, potsdam_chain((64, 64)), 2, KEY, 0)
    return model, TrainEngine(model, opt, get_loss_function(cfg), 1, use_graph=use_graph, warmup_eager=0, batch_source=source)


def test_engine_draws_a_new_batch_in_every_replay_and_resumes(tmp_path):
    """ResNet-18, batch 2, 64 x 64 tile and crop out of two 96 x 80 scenes, 3 steps eager and captured from the same weights.  After every
    captured step the engine's images / labels are the batch rebuilt on the host from the replay at that step's counter, exactly: the graph was
    captured at counter 0, so steps 1 and 2 prove that a replay reads the counter from the device.  A fresh engine whose counter is set to 2
    cuts the third batch (--resume)."""
    root = str(tmp_path / "s")
    arrays = write_scene_tree(root, ENGINE_SIZES)
    scales = potsdam_scales((64, 64))
    torch.manual_seed(3)
    from oracle.emrt_torch import EMRT as OracleEMRT
    state = {k: v.clone() for k, v in OracleEMRT(6, "resnet18").state_dict().items()}
    losses, third = {}, None
    for mode in ("eager", "graph"):
        model, eng = _engine(root, state, use_graph=(mode == "graph"))
        losses[mode] = []
        for step in range(3):
            assert int(ctx().step_counter.item()) == step
            losses[mode].append(eng.step().item())
            torch.cuda.synchronize()
            rows = replay(KEY, step, 0, 2, ENGINE_SIZES, (64, 64), (64, 64), scales, 0.5)
            assert eng.batch_source.draws.cpu().tolist() == rows, (mode, step)
            want_i, want_l = host_batch(arrays, rows, (64, 64), (64, 64))
            assert torch.equal(eng.images.cpu(), want_i) and torch.equal(eng.labels.cpu(), want_l), (mode, step)
            third = (want_i, want_l)
        if mode == "graph":
            assert eng.graph_a is not None and eng.graph_a.n_graphs == 1 and eng.calls == 3
        with pytest.raises(ValueError, match="takes no tensors"):
            eng.step(eng.images, eng.labels)
        del eng, model
    print("scene-sampled steps, eager %s captured %s" % (["%.6f" % v for v in losses["eager"]], ["%.6f" % v for v in losses["graph"]]))
    assert all(math.isfinite(v) and v > 0 for v in losses["eager"] + losses["graph"])
    assert len({round(v, 4) for v in losses["eager"]}) == 3                  # three different batches
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) / max(1.0, abs(a)) < 1e-3, (losses["eager"], losses["graph"])
    # resume: a fresh engine, the step counter restored to 2 -> the third batch
    model, eng = _engine(root, state, use_graph=True, start_step=2)
    eng.step()
    torch.cuda.synchronize()
    assert torch.equal(eng.images.cpu(), third[0]) and torch.equal(eng.labels.cpu(), third[1])
    assert int(ctx().step_counter.item()) == 3


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------------------

def test_train_cli_with_scenes(tmp_path, capsys):
    """train.main --data scenes --no-eval --iters 4 on a fake scene tree: finite losses on every step and the checkpoint on disk."""
    from emrt_amd import train
    root = str(tmp_path / "s")
    write_scene_tree(root, ENGINE_SIZES)
    cfg = str(tmp_path / "tiny.yaml")
    with open(cfg, "w") as f:
        f.write('BASE: ["%s"]\n' % os.path.relpath(os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam.yaml"), str(tmp_path)))
        f.write('DATA: {CROP_SIZE: "(64, 64)", BATCH_SIZE: 2}\n')
        f.write('MODEL: {ENCODER: {TYPE: "resnet18"}}\n')
        f.write("SAVE_FREQ_CHECKPOINT: 1000\nLOGGING_INFO_FREQ: 1\n")
    out = str(tmp_path / "out")
    train.main(["--config", cfg, "--data", "scenes", "--data_path", root, "--no-eval", "--iters", "4", "--save_dir", out, "--dtype", "fp32"])
    text = capsys.readouterr().out
    assert "[train] data: 2 scenes resident on the GPU" in text
    losses = [float(m) for m in re.findall(r"\[TRAIN\].*?loss: ([^,]+),", text)]
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses), text[-3000:]
    assert os.path.exists(os.path.join(out, "iter_4_state.pt")) and os.path.exists(os.path.join(out, "iter_4_model_state.pdparams"))
    with pytest.raises(SystemExit, match="no val_images/ and val_labels/ for the periodic evaluation; add them or pass --no-eval"):
        train.main(["--config", cfg, "--data", "scenes", "--data_path", root, "--iters", "4", "--save_dir", out, "--dtype", "fp32"])
