"""-m gpu: boundary-aware scene evaluation on the device (csrc/bnd_ext: emrt_bnd_runs, emrt_bnd_band, emrt_bnd_areas) against the
numpy host model tests/boundary_reference.py.  Every comparison is exact equality of integers.

  kernels   runs and band of blocky class maps for both shapes, both map kinds, r in {1, 3, 32}, the sizes that take another path through the
            tiles (one row, smaller than r, one tile, odd, several tiles both ways) and uint8 maps 1 and 3 bytes off alignment; every output sits
            inside a sentinel-filled allocation whose margins stay untouched
  counts    emrt_bnd_areas for 1, 6 and 256 classes, ignore 255 and 0, predictions outside the classes, n = 1, a second call that accumulates
  scenes    SceneEvaluator(boundary=3) over a resident bank: boundary_per_scene is the host model of ev.predict(i) and the stored label bytes;
            evaluate() and per_scene are those of an evaluator without it; rank 1 of 2; with tta
  val       the command line prints the host model's figures"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                                   # noqa: E402
from emrt_amd.runtime import F32, ctx                                       # noqa: E402
from emrt_amd.src.utils import metrics                                      # noqa: E402
from tests import boundary_reference as BR                                  # noqa: E402
from tests.test_gpu_scene_eval import CROP, MEAN, NCLS, STD, STRIDE, VAL_SUB, _bank, _tiny_yaml, resnet18      # noqa: E402,F401

MARGIN = 4096                      # sentinel bytes on either side of every output
SENTINEL = 0xA5
SIZES = [(1, 9), (5, 7), (64, 64), (97, 131), (300, 517)]
RUN_TILE, BAND_TILE = (8, 256), (32, 128)          # rows x columns of the tiles of bnd_runs_kernel and bnd_band_kernel (csrc/bnd_ext/bnd_ext.hip)
SEEDS = {1: 1, 3: 3, 32: 32}                       # per radius: chosen on the CPU so that the host model's band fraction is inside (0.1, 0.9) (asserted below)


@pytest.fixture
def device():
    ctx().init_device("cuda:0", F32)
    return "cuda:0"


def P(t):
    return ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def class_map(H, W, r):
    """uint8 [H, W] of classes 0..3 in blocks of edge 4r + 1, cut off at odd positions so that class edges cross the tile edges of both kernels and
    their corners both ways; lone differing pixels (255: an ignore byte is a value like any other) in the first and last row and column and on
    either side of multiples of every tile edge (lone_lines)."""
    rng = np.random.RandomState(SEEDS[r] * 1000 + H + W)
    edge = 4 * r + 1
    oy, ox = int(rng.randint(0, edge)) | 1, int(rng.randint(0, edge)) | 1
    cells = rng.randint(0, 4, ((H + oy) // edge + 2, (W + ox) // edge + 2))
    M = np.kron(cells, np.ones((edge, edge), dtype=np.int64))[oy:oy + H, ox:ox + W].astype(np.uint8)
    ys, xs = lone_lines(H, RUN_TILE[0], BAND_TILE[0]), lone_lines(W, BAND_TILE[1], RUN_TILE[1])
    for k, y in enumerate(ys):          # (a handful, paired up: at r = 32 every lone pixel puts up to 65 x 65 pixels into the band)
        M[y, xs[k % len(xs)]] = 255
    for k, x in enumerate(xs):
        M[ys[(k + 1) % len(ys)], x] = 255
    M.setflags(write=False)
    return M


def lone_lines(n, small, large):
    """the first and the last line and, where they exist, the lines on either side of the first multiple of both tile edges and of the last multiple
    of the larger one"""
    last = (n - 1) // large * large
    lines = [0, n - 1] + [t + d for t in (small, large, last) for d in (-1, 1)]
    return [v for k, v in enumerate(lines) if 0 <= v < n and v not in lines[:k]]


@functools.lru_cache(maxsize=None)
def host_band(H, W, r, shape):
    out = BR.band(class_map(H, W, r), r, shape).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_runs(H, W, r):
    out = BR.runs(class_map(H, W, r), r)
    out.setflags(write=False)
    return out


def as_int32(M):
    """the same partition in values no byte holds, negative ones among them: the int32 kind compares all 32 bits"""
    return (M.astype(np.int64) * 16777259 - 2 ** 31).astype(np.int32)


def device_map(M, kind, offset):
    """the map on the device: int32, or uint8 `offset` bytes into a 16-byte aligned allocation whose other bytes are valid class bytes"""
    if kind == 0:
        assert offset == 0
        return torch.from_numpy(as_int32(M)).cuda()
    raw = torch.zeros(M.size + 64, dtype=torch.uint8)
    raw[offset:offset + M.size] = torch.from_numpy(M.reshape(-1).copy())
    raw = raw.cuda()
    assert raw.data_ptr() % 16 == 0
    view = raw[offset:offset + M.size]
    assert view.data_ptr() % 4 == offset % 4
    return view


def guarded(n):
    """(the allocation, its n bytes in the middle): uint8, sentinel-filled"""
    big = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
    return big, big[MARGIN:MARGIN + n]


def margins_untouched(big, n):
    h = big.cpu()
    return bool((h[:MARGIN] == SENTINEL).all()) and bool((h[MARGIN + n:] == SENTINEL).all())


def run_band(M, kind, offset, r, shape):
    """emrt_bnd_runs then emrt_bnd_band -> (runs, band) uint8 [H, W] on the host, after the margins of both outputs were found unchanged"""
    B = _lib.bnd_lib()
    H, W = M.shape
    m = device_map(M, kind, offset)
    big_r, runs = guarded(H * W)
    big_b, band = guarded(H * W)
    B.call("emrt_bnd_runs", P(m), kind, H, W, r, P(runs), ctx().stream)
    B.call("emrt_bnd_band", P(m), kind, P(runs), H, W, r, BR.SHAPES[shape], P(band), ctx().stream)
    torch.cuda.synchronize()
    assert margins_untouched(big_r, H * W) and margins_untouched(big_b, H * W), (H, W, kind, offset, r, shape, "a margin was written")
    return runs.cpu().numpy().reshape(H, W), band.cpu().numpy().reshape(H, W)


# ---- the kernels --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 3, 32])
@pytest.mark.parametrize("shape", ["disk", "square"])
def test_runs_and_band_equal_the_host_model(device, shape, r):
    """Every size, as int32, as uint8 and as uint8 1 and 3 bytes off alignment.  A case with H, W > 4r must have between 10 % and 90 % of its pixels
    in the band ON THE HOST MODEL: all band or no band would say nothing about the interior."""
    for H, W in SIZES:
        M, want_runs, want = class_map(H, W, r), host_runs(H, W, r), host_band(H, W, r, shape)
        if H > 4 * r and W > 4 * r:
            assert 0.1 < want.mean() < 0.9, (H, W, r, shape, want.mean())
            if H >= 64:          # the first row and the last column hold both answers too
                assert want[0].any() and not want[0].all() and want[:, -1].any() and not want[:, -1].all()
        for kind, offset in ((0, 0), (2, 0), (2, 1), (2, 3)):
            runs, band = run_band(M, kind, offset, r, shape)
            bad = np.argwhere(runs != want_runs)
            assert bad.size == 0, (H, W, kind, offset, "runs", len(bad), bad[:5].tolist())
            bad = np.argwhere(band != want)
            assert bad.size == 0, (H, W, kind, offset, "band", len(bad), bad[:5].tolist())
            assert set(np.unique(band).tolist()) <= {0, 1}


def test_a_one_class_map_has_no_band_and_full_runs(device):
    for kind in (0, 2):
        runs, band = run_band(np.full((70, 300), 3, dtype=np.uint8), kind, 0, 32, "square")
        assert not band.any() and (runs == 32).all()


# ---- the counts ---------------------------------------------------------------------------------------------------------------------------------

def _count_inputs(n, ncls, seed):
    rng = np.random.RandomState(seed)
    pred = rng.randint(-1, ncls + 1, n).astype(np.int32)          # -1 and ncls among them
    label = rng.randint(0, min(ncls + 2, 256), n).astype(np.uint8)
    label[rng.rand(n) < 0.1] = 255
    agree = rng.rand(n) < 0.5
    pred[agree] = label[agree]
    if n > 4:
        pred[:4] = [-1, ncls, 0, 0]
        label[:4] = [0, 0, 0, 255]
    return pred, label, (rng.rand(n) < 0.4).astype(np.uint8), (rng.rand(n) < 0.4).astype(np.uint8)


@pytest.mark.parametrize("ignore", [255, 0])
@pytest.mark.parametrize("n,ncls", [(300 * 517, 1), (300 * 517, 6), (300 * 517, 256), (1, 6), (4099, 6)])
def test_areas_equal_the_host_counts_and_accumulate(device, n, ncls, ignore):
    B = _lib.bnd_lib()
    pred, label, bp, bl = _count_inputs(n, ncls, 7 * n + ncls)
    if n == 1:
        pred[0], label[0], bp[0], bl[0] = 2, 2, 1, 1
    want = BR.counts(pred, label, ncls, ignore, None, None, band_pred=bp, band_label=bl)
    assert want.sum() > 0
    if n > 1:
        assert (pred == -1).any() and (pred == ncls).any() and (label == ignore).any() and want[0].sum() > 0 and want[1].sum() > 0
    raw = torch.zeros(n + 8, dtype=torch.uint8)
    raw[1:1 + n] = torch.from_numpy(label)
    lab_d = raw.cuda()[1:1 + n]                                    # one byte off alignment, as a label map in a bank may be
    big = torch.full((2 * 3 * ncls + 16,), -77, dtype=torch.int64, device="cuda")
    out = big[8:8 + 2 * 3 * ncls]
    out.zero_()
    pred_d, bp_d, bl_d = torch.from_numpy(pred).cuda(), torch.from_numpy(bp).cuda(), torch.from_numpy(bl).cuda()          # (kept alive by these names)
    args = (P(pred_d), P(lab_d), P(bp_d), P(bl_d), n, ncls, ignore, P(out), ctx().stream)
    B.call("emrt_bnd_areas", *args)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(2, 3, ncls)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    B.call("emrt_bnd_areas", *args)                                # accumulated into, not overwritten
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(2, 3, ncls), 2 * want)
    h = big.cpu()
    assert bool((h[:8] == -77).all()) and bool((h[8 + 2 * 3 * ncls:] == -77).all())


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------------------

SCENES = [(64, 64), (96, 150), (130, 200)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """(root, [label uint8 HW]): three validation scenes laid out as tests/test_gpu_scene_eval.py lays them out, with labels 0..5 and 255 in blocks of 17, so that the eroded protocol keeps part of every scene"""
    root = str(tmp_path_factory.mktemp("bnd_scenes"))
    rng = np.random.RandomState(5)
    os.makedirs(os.path.join(root, VAL_SUB[0]))
    os.makedirs(os.path.join(root, VAL_SUB[1]))
    labels = []
    for i, (H, W) in enumerate(SCENES):
        cells = rng.randint(0, NCLS + 1, (H // 17 + 2, W // 17 + 2))
        cells[cells == NCLS] = 255
        lab = np.kron(cells, np.ones((17, 17), dtype=np.int64))[5:5 + H, 9:9 + W].astype(np.uint8)
        Image.fromarray(rng.randint(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, VAL_SUB[0], "scene_%d.tif" % i))
        Image.fromarray(lab).save(os.path.join(root, VAL_SUB[1], "scene_%d.png" % i))
        labels.append(lab)
    return root, labels


def _evaluator(model, bank, **kw):
    from emrt_amd.src.api.scene import SceneEvaluator
    return SceneEvaluator(model, bank, NCLS, CROP, STRIDE, MEAN, STD, ignore_index=255, max_batch=32, **kw)


def _host_counts(ev, labels, shape, scenes=None):
    out = np.zeros((len(labels), 2, 3, NCLS), dtype=np.int64)
    for i in (range(len(labels)) if scenes is None else scenes):
        pred = ev.predict(i).cpu().numpy()[0, 0]
        stored = ev.bank.scene(i)[1].cpu().numpy()
        assert np.array_equal(stored, labels[i])
        out[i] = BR.counts(pred, stored, NCLS, 255, 3, shape)
    return out


@pytest.mark.parametrize("shape", ["disk", "square"])
def test_evaluator_counts_equal_the_host_model_and_leave_the_evaluation_as_it_is(resnet18, tree, shape):      # noqa: F811
    root, labels = tree
    bank = _bank(root)
    plain = _evaluator(resnet18, bank)
    want_tot = plain.evaluate().cpu()
    ev = _evaluator(resnet18, bank, boundary=3, boundary_shape=shape)
    tot = ev.evaluate()
    assert tot.is_cuda and torch.equal(tot.cpu(), want_tot) and torch.equal(ev.per_scene.cpu(), plain.per_scene.cpu())
    got = ev.boundary_per_scene.cpu().numpy()
    want = _host_counts(ev, labels, shape)
    assert got.shape == (3, 2, 3, NCLS) and np.array_equal(got, want), (got.tolist(), want.tolist())
    assert np.array_equal(ev.boundary_totals().cpu().numpy(), want.sum(0))
    for i in range(3):          # the eroded protocol keeps something of every scene and drops something
        assert 0 < want[i][0][2].sum() < (labels[i] != 255).sum() and want[i][1][2].sum() > 0
    assert want[:, 1, 1].sum() > 0          # and the predictions have boundaries
    # the second evaluation starts from zero, in the same scratch
    scratch = {k: [t.data_ptr() for t in v] for k, v in ev._bnd_scratch.items()}
    ev.evaluate()
    assert np.array_equal(ev.boundary_per_scene.cpu().numpy(), want) and {k: [t.data_ptr() for t in v] for k, v in ev._bnd_scratch.items()} == scratch
    # rank 1 of 2 fills only its own rows
    tot1 = ev.evaluate(rank=1, nranks=2)
    got1 = ev.boundary_per_scene.cpu().numpy()
    assert not got1[0].any() and not got1[2].any() and np.array_equal(got1[1], want[1]) and torch.equal(tot1.cpu(), plain.per_scene[1].cpu())


def test_evaluator_counts_with_tta(resnet18, tree):      # noqa: F811
    root, labels = tree
    bank = _bank(root)
    plain = _evaluator(resnet18, bank, tta="hflip")
    want_tot = plain.evaluate().cpu()
    ev = _evaluator(resnet18, bank, tta="hflip", boundary=3)
    assert torch.equal(ev.evaluate().cpu(), want_tot) and torch.equal(ev.per_scene.cpu(), plain.per_scene.cpu())
    assert np.array_equal(ev.boundary_per_scene.cpu().numpy(), _host_counts(ev, labels, "disk"))


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------

def test_val_cli_prints_the_host_models_figures(tree, tmp_path, capsys, monkeypatch):
    from emrt_amd import val
    root, labels = tree
    made = []
    real = val.scene_evaluator
    monkeypatch.setattr(val, "scene_evaluator", lambda *a, **k: (made.append(real(*a, **k)), made[-1])[1])
    torch.manual_seed(0)
    val.main(["--config", _tiny_yaml(tmp_path), "--data", "scenes", "--data_path", root, "--boundary", "3", "--boundary_shape", "square"])
    text = capsys.readouterr().out
    ev = made[0]
    assert (ev.boundary, ev.boundary_shape) == (3, 1)
    tot = _host_counts(ev, labels, "square").sum(0)
    miou, acc, _, _, _, cf1, mf1 = val.metric_tuple(torch.from_numpy(tot[0]))
    biou, mbiou = metrics.mean_iou(tot[1][0], tot[1][1], tot[1][2])
    lines = text.splitlines()
    at = lines.index("[EVAL] Eroded (square r=3): mIoU: %.4f  Acc: %.4f  mF1: %.4f" % (miou, acc, mf1))
    assert lines[at + 1] == "[EVAL] Eroded Class F1-score: " + str(np.round(cf1, 4))
    assert lines[at + 2] == "[EVAL] Boundary (square r=3): mBIoU: %.4f" % mbiou
    assert lines[at + 3] == "[EVAL] Boundary Class BIoU: " + str(np.round(biou, 4)) and at + 4 == len(lines)
    assert re.match(r"\[EVAL\] Scene scene_2 \(130x200\)", lines[at - 1]) and text.count("[EVAL] Images: 3  mIoU:") == 1
    assert 0.0 < mbiou < 1.0 and 0.0 < miou < 1.0
