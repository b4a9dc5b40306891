"""-m gpu: class-aware tile sampling (csrc/sampler_ext/sampler_ext.hip: emrt_smp_row_counts, emrt_smp_class_redraw) behind
`train.py --data scenes` with DATA.SCENE_SAMPLING.MODE "class".

  index    the device row-count table equals np.bincount per row exactly, twice over
  draws    after draw + redraw the table equals the restatement (tests/class_sampler_reference.py) applied to the table of the draw launch
           alone, bit for bit: columns 3 and up untouched, PROB 0 a no-op, PROB 1 every row, every window around a pixel of its class
  stale    an index of another bank moves windows to wrong places inside their scenes, never outside (judged by the table values)
  tiles    what fill() writes equals the CPU transform functions on the host copy of the drawn windows (the comparison of
           tests/test_gpu_scene_sampler.py)
  engine   a captured TrainEngine step cuts the batch the restatement predicts for its counter, and resumes

One bank: four noise scenes of 40x56, 33x70, 64x64 and 24x1500 (a row of many wave passes), tile 24x40; classes 0 and 1 as noise, 255 ignored,
class 2 on exactly three pixels, class 3 absent -- and the same maps as LoveDA stores them, read through label_lut(1)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd.runtime import F32, ctx                                       # noqa: E402
from emrt_amd.src import transforms as T                                    # noqa: E402
from emrt_amd.src.datasets import SceneBank, SceneSampler, label_lut        # noqa: E402
from tests import class_sampler_reference as R                              # noqa: E402
from tests.test_augment_ext_cpu import aug_chain                            # noqa: E402
from tests.test_gpu_scene_sampler import drawn, host_batch, set_step        # noqa: E402
from tests.test_scene_sampler_cpu import potsdam_chain, potsdam_scales, replay      # noqa: E402

SIZES = [(40, 56), (33, 70), (64, 64), (24, 1500)]
TILE = (24, 40)
NCLS = 4
KEY = 0xFEDCBA9876543210                                                    # both key words in use, top bit set
STEPS = (0, 1, 2, (1 << 32) + 5)


def node(prob=0.5):
    return {"MODE": "class", "PROB": prob, "TEMPERATURE": 0.1, "CLASS_PROBS": None}


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """shift -> (root, [(img, lab)], lut): the bank as Potsdam stores it (shift 0) and as LoveDA does (shift 1); computed once, never changed."""
    out = {}
    for shift in (0, 1):
        root = str(tmp_path_factory.mktemp("rare%d" % shift))
        labels = R.rare_class_labels(SIZES, shift=shift)
        out[shift] = (root, R.write_bank(root, SIZES, labels), label_lut(1) if shift else None)
    plain, shifted = R.mapped([lab for _, lab in out[0][1]]), R.mapped([lab for _, lab in out[1][1]], label_lut(1))
    assert all(np.array_equal(a, b) for a, b in zip(plain, shifted))
    assert plain[0][0, 0] == 2 and plain[3][23, 1499] == 2 and plain[3][12, 1499 - 64] == 2 and sum(int((m == 2).sum()) for m in plain) == 3
    assert not any((m == 3).any() for m in plain)
    return out


@pytest.fixture
def device():
    ctx().init_device("cuda:0", F32)
    return "cuda:0"


def chain(cols):
    return potsdam_chain(TILE) if cols == 10 else aug_chain((TILE[1], TILE[0]), vflip=0.25, rng=0.3, prob=0.6)


def samplers(root, device, shift, cols, B, rank, prob):
    """(class-mode sampler, uniform sampler) over one bank with the same arguments otherwise."""
    bank = SceneBank(root, device, label_shift=shift)
    return (SceneSampler(bank, chain(cols), B, KEY, rank, sampling=node(prob), num_classes=NCLS),
            SceneSampler(bank, chain(cols), B, KEY, rank))


# ---- index --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [0, 1])
def test_row_counts_equal_bincount_exactly_and_twice(trees, device, shift):
    root, arrays, lut = trees[shift]
    want = R.row_counts([lab for _, lab in arrays], NCLS, lut)
    a = SceneBank(root, device, label_shift=shift).class_index(NCLS, lut)
    b = SceneBank(root, device, label_shift=shift).class_index(NCLS, lut)
    assert a.counts.dtype == np.int32 and a.counts.shape == (161, NCLS) and np.array_equal(a.counts, want)
    assert a.counts.tobytes() == b.counts.tobytes() and a.build_ms > 0
    assert a.totals.tolist() == want.sum(0).tolist() and a.totals[2] == 3 and a.totals[3] == 0
    assert torch.equal(a.cum_dev.cpu(), torch.from_numpy(a.cum)) and a.row_start_dev.tolist() == [0, 40, 73, 137, 161]
    # more classes than a wave has lanes: the second trip of the class loop (every class above 2 is empty, 255 is never counted)
    wide = SceneBank(root, device, label_shift=shift).class_index(130, lut)
    assert np.array_equal(wide.counts, R.row_counts([lab for _, lab in arrays], 130, lut)) and not wide.counts[:, 3:].any()


# ---- draws --------------------------------------------------------------------------------------------------------------------------------------

def check_tables(s, u, arrays, lut, step, prob, ncls=NCLS):
    """One fill of each sampler at `step` -> (table, info): the class-mode table is the restatement's redraw of the uniform one."""
    set_step(step)
    base, _, _ = drawn(u)
    got, _, _ = drawn(s)
    labels = [lab for _, lab in arrays]
    want, info = R.redraw(base, KEY, step, s.rank, labels, TILE, ncls, s.thresholds.tolist(), prob, lut)
    assert got == want, (step, s.rank, [(g, w) for g, w in zip(got, want) if g != w][:4])
    assert [r[3:] for r in got] == [r[3:] for r in base]                    # columns 3 and up: the draw launch's, bit for bit
    maps = R.mapped(labels, lut)
    for r, i in zip(got, info):
        if i is not None:                                                   # the window holds a pixel of its class where the anchor says
            cls, sc, y, x, _, _ = i
            H, W = SIZES[sc]
            assert r[0] == sc and 0 <= r[1] <= H - TILE[0] and 0 <= r[2] <= W - TILE[1]
            assert maps[sc][r[1]:r[1] + TILE[0], r[2]:r[2] + TILE[1]][y - r[1], x - r[2]] == cls
    return got, base, info


@pytest.mark.parametrize("cols", [10, 18])
@pytest.mark.parametrize("shift", [0, 1])
def test_draws_equal_the_restatement_exactly(trees, device, shift, cols):
    """Steps 0, 1, 2 and 2^32 + 5, ranks 0 and 3, a 64-bit key, B = 8 and B = 257 (more samples than one block of the draw launch holds)."""
    root, arrays, lut = trees[shift]
    counts = R.row_counts([lab for _, lab in arrays], NCLS, lut)
    seen = set()
    for rank in (0, 3):
        for B in (8, 257):
            s, u = samplers(root, device, shift, cols, B, rank, 0.5)
            assert s.draws.shape == (B, cols) and s.thresholds.tolist() == R.thresholds(R.probabilities(counts.sum(0)))
            for step in STEPS:
                got, base, info = check_tables(s, u, arrays, lut, step, 0.5)
                if cols == 10 and B == 8:                                   # (the base table is what the draw launch is held to elsewhere)
                    assert base == replay(KEY, step, rank, B, SIZES, TILE, TILE, potsdam_scales(TILE), 0.5)
                again, _, _ = drawn(s)
                assert again == got and int(ctx().step_counter.item()) == step
                seen |= {i[:4] for i in info if i is not None}
    # the three pixels of the rare class were all drawn: the bank's first pixel, its last, and one 64 columns from the end of a 1500-byte row
    assert {(2, 0, 0, 0), (2, 3, 23, 1499), (2, 3, 12, 1435)} <= seen and {1, 2} <= {c for c, _, _, _ in seen} <= {0, 1, 2}


def test_prob_zero_changes_nothing_and_prob_one_redraws_every_row(trees, device):
    root, arrays, lut = trees[0]
    s0, u = samplers(root, device, 0, 10, 64, 1, 0.0)
    got, base, info = check_tables(s0, u, arrays, lut, 7, 0.0)
    assert got == base and info == [None] * 64
    s1, u = samplers(root, device, 0, 10, 64, 1, 1.0)
    got, base, info = check_tables(s1, u, arrays, lut, 7, 1.0)
    assert all(i is not None for i in info) and got != base
    # 130 classes, all but three of them absent: the thresholds are compared 64 per round, three rounds
    wide = SceneSampler(u.bank, chain(10), 64, KEY, 1, sampling=node(1.0), num_classes=130)
    assert wide.thresholds.tolist() == s1.thresholds.tolist()[:3] + [1 << 32] * 127
    got130, _, info130 = check_tables(wide, u, arrays, lut, 7, 1.0, ncls=130)
    assert got130 == got and info130 == info


def test_a_stale_index_keeps_every_window_inside_its_scene(trees, device):
    """The prefix table of another bank of the same shape, copied over this bank's on the device: rows move to wrong places or stay; the table
    still equals the restatement given the same stale counts, and every row is a window of its scene."""
    root, arrays, lut = trees[0]
    s, u = samplers(root, device, 0, 10, 257, 0, 1.0)
    stale = R.row_counts(R.rare_class_labels(SIZES, seed=9), NCLS)
    cum = np.zeros_like(s.index.cum)
    cum[:, 1:] = np.cumsum(stale.T, axis=1)
    s.index.cum_dev.copy_(torch.from_numpy(cum))
    set_step(3)
    base, _, _ = drawn(u)
    got, _, _ = drawn(s)
    want, info = R.redraw(base, KEY, 3, 0, [lab for _, lab in arrays], TILE, NCLS, s.thresholds.tolist(), 1.0, counts=stale)
    assert got == want and any(i is None for i in info) and any(i is not None for i in info)
    for r in got:
        H, W = SIZES[r[0]]
        assert 0 <= r[0] < 4 and 0 <= r[1] <= H - TILE[0] and 0 <= r[2] <= W - TILE[1]


# ---- tiles --------------------------------------------------------------------------------------------------------------------------------------

def test_tiles_equal_the_cpu_chain_on_the_redrawn_windows(trees, device):
    root, arrays, _ = trees[0]
    s, _ = samplers(root, device, 0, 10, 8, 0, 1.0)
    for step in (0, 1, 2):
        set_step(step)
        rows, images, labels = drawn(s)
        want_i, want_l = host_batch(arrays, rows, TILE, TILE)
        assert torch.equal(images, want_i) and torch.equal(labels, want_l), step
    # LoveDA's chain: [Normalize] alone on the stored maps, the shift in the lookup table of both the redraw and the sample launch
    root, arrays, lut = trees[1]
    bank = SceneBank(root, device, label_shift=1)
    s = SceneSampler(bank, [T.Normalize(mean=T._MEAN, std=T._STD)], 8, KEY, 0, tile=TILE, sampling=node(1.0), num_classes=NCLS)
    set_step(1)
    rows, images, labels = drawn(s)
    base = replay(KEY, 1, 0, 8, SIZES, TILE, TILE, [TILE], 0.0)
    want, info = R.redraw(base, KEY, 1, 0, [lab for _, lab in arrays], TILE, NCLS, s.thresholds.tolist(), 1.0, lut)
    assert rows == want and all(i is not None for i in info)
    want_i, want_l = host_batch(arrays, rows, TILE, TILE, lut=lut)
    assert torch.equal(images, want_i) and torch.equal(labels, want_l)


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
    model.load_state_dict(state)
    model.to_hip("cuda:0", F32)
    model.set_dropout(0.0)
    model.eval()
    model(torch.zeros(2, 3, 64, 64, device="cuda:0"))      # the shape-keyed constants are uploaded outside the capture
    model.train()
    opt = get_optimizer(model, get_scheduler(cfg), cfg)
    set_step(start_step)
    source = SceneSampler(SceneBank(root, "cuda:0"), potsdam_chain((64, 64)), 2, 1234, 0, sampling=node(0.75), num_classes=6)
    return model, TrainEngine(model, opt, get_loss_function(cfg), 1, use_graph=use_graph, warmup_eager=0, batch_source=source)


def test_engine_cuts_the_predicted_batch_in_every_replay_and_resumes(tmp_path):
    """ResNet-18, batch 2, 64 x 64 tile and crop out of two 96 x 80 scenes, class mode at PROB 0.75, 3 steps eager and captured from the same
    weights.  After every step the engine's batch is the one rebuilt on the host from the restatement at that step's counter: the graph was
    captured at counter 0, so steps 1 and 2 prove that the replayed redraw reads the counter on the device.  A fresh engine whose counter is
    set to 2 cuts the third batch."""
    root = str(tmp_path / "s")
    labels = R.rare_class_labels(ENGINE_SIZES)
    arrays = R.write_bank(root, ENGINE_SIZES, labels)
    scales = potsdam_scales((64, 64))
    thr = R.thresholds(R.probabilities(R.row_counts(labels, 6).sum(0)))
    torch.manual_seed(3)
    from oracle.emrt_torch import EMRT as OracleEMRT
    state = {k: v.clone() for k, v in OracleEMRT(6, "resnet18").state_dict().items()}
    losses, third, moved = {}, None, 0
    for mode in ("eager", "graph"):
        model, eng = _engine(root, state, use_graph=(mode == "graph"))
        assert eng.batch_source.thresholds.tolist() == thr
        losses[mode] = []
        for step in range(3):
            assert int(ctx().step_counter.item()) == step
            losses[mode].append(eng.step().item())
            torch.cuda.synchronize()
            base = replay(1234, step, 0, 2, ENGINE_SIZES, (64, 64), (64, 64), scales, 0.5)
            rows, info = R.redraw(base, 1234, step, 0, labels, (64, 64), 6, thr, 0.75)
            moved += sum(i is not None for i in info)
            assert eng.batch_source.draws.cpu().tolist() == rows, (mode, step)
            want_i, want_l = host_batch(arrays, rows, (64, 64), (64, 64))
            assert torch.equal(eng.images.cpu(), want_i) and torch.equal(eng.labels.cpu(), want_l), (mode, step)
            third = (want_i, want_l)
        if mode == "graph":
            assert eng.graph_a is not None and eng.graph_a.n_graphs == 1 and eng.calls == 3
        del eng, model
    assert moved >= 2                                                        # (seeded: the class decision fired in these steps)
    print("class-sampled steps, eager %s captured %s" % (["%.6f" % v for v in losses["eager"]], ["%.6f" % v for v in losses["graph"]]))
    assert all(math.isfinite(v) and v > 0 for v in losses["eager"] + losses["graph"])
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) / max(1.0, abs(a)) < 1e-3, (losses["eager"], losses["graph"])
    model, eng = _engine(root, state, use_graph=True, start_step=2)
    eng.step()
    torch.cuda.synchronize()
    assert torch.equal(eng.images.cpu(), third[0]) and torch.equal(eng.labels.cpu(), third[1])
    assert int(ctx().step_counter.item()) == 3
