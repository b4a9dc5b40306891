"""-m gpu: flip and rotation test-time augmentation of whole-scene inference -- the two kernels of csrc/tta_ext/tta_ext.hip and
ScenePredictor / SceneEvaluator / predict_tiles under every mode against the numpy float64 restatement tests/tta_reference.py.

The crop kernel is compared bit for bit.  The sums of the accumulation kernel are held to R.bound(K, G, C) = K * G * (C + 8) * 2^-23 absolute, K the
largest number of windows over a pixel: expf and the reciprocal at a few ulp and a C-term denominator per term, and K * G additions of terms <= 1.
Class indices are compared wherever the reference's two largest sums are further apart than twice that bound."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                  # noqa: E402
from emrt_amd.functional import P                          # noqa: E402
from emrt_amd.runtime import F32                           # noqa: E402
from emrt_amd.src.api import infer                         # noqa: E402
from emrt_amd.src.transforms import Normalize              # noqa: E402
from emrt_amd.src.utils import metrics, vis                # noqa: E402
from tests import tta_reference as R                       # noqa: E402
from tests.hip_utils import init                           # noqa: E402
from tests.test_scene_sampler_cpu import write_scene_tree  # noqa: E402

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
STDINV = [float(v) for v in 1.0 / np.asarray(STD, dtype=np.float64)]
VAL_SUB = ("val_images", "val_labels")
TTA = ["hflip", "flips", "d4"]


def _ints(values):
    arr = (ctypes.c_int * len(values))(*values)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _crop(scene, org, codes, ch, cw):
    """one emrt_tta_crop_windows_u8 launch on a uint8 [H, W, 3] numpy scene -> fp32 numpy [n * G, 3, ch, cw] (every element must be written)"""
    c = init(F32)
    sd = torch.from_numpy(scene).cuda()
    batch = torch.full((len(org) * len(codes), 3, ch, cw), float("nan"), device="cuda")
    _o, op = _ints([v for yx in org for v in yx])
    _k, kp = _ints(codes)
    _lib.tta_lib().call("emrt_tta_crop_windows_u8", P(sd), P(batch), op, len(org), kp, len(codes), scene.shape[0], scene.shape[1], ch, cw,
                        *MEAN, *STDINV, c.stream)
    return batch.cpu().numpy()


def _accumulate(logits, final, count, org, codes, ch, cw):
    """the windows in launches of 64 // G, added into the device tensors final [C, H, W] and count [H, W]"""
    c = init(F32)
    G, per = len(codes), 64 // len(codes)
    _k, kp = _ints(codes)
    for i in range(0, len(org), per):
        chunk = org[i:i + per]
        _o, op = _ints([v for yx in chunk for v in yx])
        part = logits[i * G:(i + len(chunk)) * G]
        _lib.tta_lib().call("emrt_tta_window_accumulate", P(part), P(final), P(count), op, len(chunk), kp, G, final.shape[0], final.shape[1], final.shape[2],
                            ch, cw, c.stream)


# ---- 1. the crop kernel ------------------------------------------------------------------------------------------------------------------
CROP_CASES = {
    # (scene H, W), (ch, cw), origins: the second window of the first three touches the right and the bottom edge
    "16-ragged": ((37, 41), (16, 16), [(0, 0), (21, 25), (5, 3)]),
    "20-ragged": ((37, 41), (20, 20), [(0, 0), (17, 21), (5, 3)]),
    "32-aligned": ((64, 96), (32, 32), [(0, 0), (32, 64), (12, 20)]),
    "40-four-ragged-tiles": ((50, 70), (40, 40), [(0, 0), (10, 30), (3, 7)]),
}


@pytest.mark.parametrize("mode", ["none"] + TTA)
@pytest.mark.parametrize("case", list(CROP_CASES))
def test_crop_variants_equal_the_reference_bit_for_bit(case, mode):
    (H, W), (ch, cw), org = CROP_CASES[case]
    rng = np.random.RandomState(5100 + H + ch)
    scene = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    scene[0, 0] = (0, 255, 0)
    codes = R.MODES[mode]
    got = _crop(scene, org, codes, ch, cw)
    want = R.crop_variants(scene, org, codes, ch, cw, MEAN, STD).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)
    assert len({want[g].tobytes() for g in range(len(codes))}) == len(codes)          # the variants differ: a wrong one would show


def test_crop_of_a_rectangle_under_the_flips():
    rng = np.random.RandomState(5200)
    scene = rng.randint(0, 256, (37, 41, 3)).astype(np.uint8)
    org = [(0, 0), (21, 17), (5, 3)]                        # 16 rows x 24 columns; the second touches both edges
    got = _crop(scene, org, R.MODES["flips"], 16, 24)
    assert np.array_equal(got, R.crop_variants(scene, org, R.MODES["flips"], 16, 24, MEAN, STD).astype(np.float32))


# ---- 2. the accumulation kernel -------------------------------------------------------------------------------------------------------------
# crop -> stride (w, h) on the 37 x 41 map: 3 x 3 and 2 x 3 windows, the last of a row or column shifted back inside; 4 windows over a pixel at most
ACC_GRIDS = {16: (13, 11), 20: (14, 17)}


@pytest.mark.parametrize("mode", TTA)
@pytest.mark.parametrize("crop", [16, 20])
@pytest.mark.parametrize("C", [1, 6, 19])
def test_accumulate_equals_the_float64_sums_within_the_derived_bound(C, crop, mode):
    H, W = 37, 41
    codes = R.MODES[mode]
    G = len(codes)
    org = [(a, b) for (a, b, _, _) in infer.window_grid(H, W, (crop, crop), ACC_GRIDS[crop])]
    cover = R.cover(H, W, org, crop, crop)
    K = int(cover.max())
    assert K == 4 and cover.min() >= 1 and (H - crop, W - crop) in org
    assert len(org) == {16: 9, 20: 6}[crop]                 # crop 16 under d4: 72 images, two launches
    g = torch.Generator().manual_seed(5300 + 10 * C + crop)
    logits = torch.randn(len(org) * G, C, crop, crop, generator=g) * 8
    flat = logits.view(-1)
    flat[torch.randint(0, flat.numel(), (24,), generator=g)] = 60.0          # a softmax without the max subtraction overflows here
    flat[torch.randint(0, flat.numel(), (24,), generator=g)] = -60.0
    final0 = torch.rand(C, H, W, generator=g) * 0.75 + 0.25
    count0 = torch.randint(1, 4, (H, W), generator=g).float()
    want, cnt = R.accumulate(logits.numpy(), org, codes, H, W, final=final0.double().numpy().copy(), count=count0.double().numpy().copy())
    runs = []
    for _ in range(2):
        final, count = final0.cuda(), count0.cuda()
        _accumulate(logits.cuda(), final, count, org, codes, crop, crop)
        runs.append((final.cpu(), count.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])          # one fixed order: the same bits
    final, count = runs[0]
    assert np.array_equal(count.numpy(), cnt) and np.array_equal(cnt, count0.numpy() + G * cover)
    err = np.abs(final.double().numpy() - want).max()
    print("tta accumulate C=%d crop=%d %s: K=%d G=%d max |kernel - float64| = %.3g, bound %.3g" % (C, crop, mode, K, G, err, R.bound(K, G, C)))
    assert err <= R.bound(K, G, C)


# ---- 3. the pipeline on stub models -----------------------------------------------------------------------------------------------------------
NCLS, CROP, STRIDE, MAX_BATCH = 6, (32, 32), (24, 24), 16
SIZES = [(72, 88), (64, 50)]


class Stub:
    """A model on the device made of elementwise torch arithmetic: a fixed 1 x 1 channel mix, plus a fixed position ramp unless `equivariant`.
    With the ramp a variant's logits are NOT the variant of the window's logits, so a wrong inverse moves the sums; without it they are, exactly.
    Records the logits of every call."""

    def __init__(self, equivariant, crop=32):
        g = torch.Generator().manual_seed(5400)
        self.mix = (torch.randn(NCLS, 3, generator=g) * 1.5).cuda()
        ys, xs = torch.meshgrid(torch.arange(crop, dtype=torch.float32), torch.arange(crop, dtype=torch.float32), indexing="ij")
        ramp = torch.stack([(k + 1) * 0.05 * ys - (NCLS - k) * 0.03 * xs + 0.002 * k * ys * xs / crop for k in range(NCLS)])
        self.ramp = None if equivariant else ramp.cuda()
        self.logits = []

    def eval(self):
        pass

    def __call__(self, x):
        m = self.mix
        out = m[:, 0].view(1, -1, 1, 1) * x[:, 0:1] + m[:, 1].view(1, -1, 1, 1) * x[:, 1:2] + m[:, 2].view(1, -1, 1, 1) * x[:, 2:3]
        if self.ramp is not None:
            out = out + self.ramp
        out = out.contiguous()
        self.logits.append(out.cpu().numpy())
        return [out]


def _reference(logits, H, W, crop, stride, codes, max_batch):
    """the float64 sums and counts of one scene from the recorded logits of its model calls (consumed from the front of `logits`)"""
    org = [(a, b) for (a, b, _, _) in infer.window_grid(H, W, crop, stride)]
    per = max_batch // len(codes)
    final, count = np.zeros((logits[0].shape[1], H, W)), np.zeros((H, W))
    for i in range(0, len(org), per):
        chunk = org[i:i + per]
        lg = logits.pop(0)
        assert lg.shape[0] == len(chunk) * len(codes)
        R.accumulate(lg, chunk, codes, H, W, final=final, count=count)
    return final, count, int(R.cover(H, W, org, crop[1], crop[0]).max())


def _decided(want, bound):
    """(reference class index, the pixels whose two largest reference sums are more than 2 * bound apart)"""
    top = np.sort(want, axis=0)
    return want.argmax(0), (top[-1] - top[-2]) > 2 * bound


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """(root of the validation tree, [(img uint8 HWC, lab uint8 HW)]) for SIZES: seeded noise, labels 0..5 with some 255"""
    root = str(tmp_path_factory.mktemp("tta_scenes"))
    return root, write_scene_tree(root, SIZES, sub=VAL_SUB, seed=54)


def _predictor(model, **kw):
    from emrt_amd.src.api.scene import ScenePredictor
    kw.setdefault("max_batch", MAX_BATCH)
    return ScenePredictor(model, NCLS, CROP, STRIDE, vis.get_palette("Potsdam"), MEAN, STD, **kw)


def _evaluator(model, root, **kw):
    from emrt_amd.src.api.scene import SceneEvaluator
    from emrt_amd.src.datasets import SceneBank
    bank = SceneBank(root, "cuda:0", 0, sub=VAL_SUB, shift_on_upload=True)
    kw.setdefault("max_batch", MAX_BATCH)
    return SceneEvaluator(model, bank, NCLS, CROP, STRIDE, MEAN, STD, ignore_index=255, **kw)


@pytest.mark.parametrize("mode", TTA)
def test_pipeline_with_a_stub_that_is_not_equivariant(scenes, mode):
    from emrt_amd.src.api import scene as S
    init(F32)
    root, arrays = scenes
    codes = R.MODES[mode]
    G = len(codes)
    img = arrays[0][0]
    H, W = img.shape[:2]
    sd = torch.from_numpy(img).cuda()
    # the predictor's pass, once for its sums and once through the class
    stub = Stub(equivariant=False)
    final = torch.zeros(1, NCLS, H, W, device="cuda")
    count = torch.zeros(1, 1, H, W, device="cuda")
    p = _predictor(stub, tta=mode, overlay=0.5)
    S.accumulate_windows(stub, sd, H, W, p.crop, p.stride, NCLS, MAX_BATCH, p.mean, p.stdinv, final, count, p.codes)
    per = MAX_BATCH // G
    assert [lg.shape[0] for lg in stub.logits] == [min(per, 12 - i) * G for i in range(0, 12, per)]          # 12 windows, max_batch // G per call
    want, cnt, K = _reference(stub.logits, H, W, CROP, STRIDE, codes, MAX_BATCH)
    assert K == 4 and not stub.logits
    bound = R.bound(K, G, NCLS)
    err = np.abs(final[0].double().cpu().numpy() - want).max()
    print("tta pipeline %s: max |device sums - float64| = %.3g, bound %.3g" % (mode, err, bound))
    assert err <= bound and np.array_equal(count[0, 0].cpu().numpy(), cnt)
    ref_index, decided = _decided(want, bound)
    assert decided.mean() >= 0.99, "the reference alone leaves %.2f %% of the pixels undecided" % (100 * (1 - decided.mean()))
    res = p(sd)
    index = res.index.cpu().numpy()
    assert np.array_equal(index[decided], ref_index[decided]) and len(np.unique(index)) > 2
    assert np.array_equal(res.areas.cpu().numpy(), np.bincount(index.reshape(-1), minlength=NCLS)) and int(res.areas.sum()) == H * W
    pal = vis.get_palette("Potsdam")
    assert np.array_equal(res.color.cpu().numpy(), pal[index])
    assert np.array_equal(res.overlay.cpu().double().numpy(), np.floor(0.5 * pal[index].astype(np.float64) + 0.5 * img.astype(np.float64) + 0.5))
    # the evaluator over both scenes
    stub = Stub(equivariant=False)
    ev = _evaluator(stub, root, tta=mode)
    tot = ev.evaluate().cpu()
    for i, (h, w) in enumerate(SIZES):
        want, cnt, K = _reference(stub.logits, h, w, CROP, STRIDE, codes, MAX_BATCH)
        ref_index, decided = _decided(want, R.bound(K, G, NCLS))
        assert decided.mean() >= 0.99
        f, c, _, pred = ev._buffers(h, w)                  # (one scene per shape: what evaluate() left there)
        pred = pred.cpu()
        assert np.abs(f[0].double().cpu().numpy() - want).max() <= R.bound(K, G, NCLS) and np.array_equal(c[0, 0].cpu().numpy(), cnt)
        assert np.array_equal(pred[0, 0].numpy()[decided], ref_index[decided])
        if i == 0:
            assert np.array_equal(pred[0, 0].numpy(), index)                 # the predictor's map of the same scene
        area = torch.stack(metrics.calculate_area(pred, torch.from_numpy(arrays[i][1]), NCLS, 255))
        assert torch.equal(ev.per_scene[i].cpu(), area)
    assert torch.equal(tot, ev.per_scene.cpu().sum(0)) and int(tot[1].sum()) == sum(int((lab != 255).sum()) for _, lab in arrays)


@pytest.mark.parametrize("mode", TTA)
def test_an_equivariant_stub_votes_as_without_tta(scenes, mode):
    init(F32)
    root, arrays = scenes
    img = arrays[0][0]
    H, W = img.shape[:2]
    sd = torch.from_numpy(img).cuda()
    plain = _predictor(Stub(equivariant=True), tta="none")(sd).index.cpu().numpy()
    stub = Stub(equivariant=True)
    got = _predictor(stub, tta=mode)(sd).index.cpu().numpy()
    want, _, K = _reference(stub.logits, H, W, CROP, STRIDE, R.MODES[mode], MAX_BATCH)
    _, decided = _decided(want, R.bound(K, len(R.MODES[mode]), NCLS))
    assert decided.mean() >= 0.99 and np.array_equal(got[decided], plain[decided]) and len(np.unique(plain)) > 2
    ev_plain = _evaluator(Stub(equivariant=True), root, tta="none")
    ev = _evaluator(Stub(equivariant=True), root, tta=mode)
    assert np.array_equal(ev.predict(0)[0, 0].cpu().numpy()[decided], ev_plain.predict(0)[0, 0].cpu().numpy()[decided])


def _normalised_chw(u8_hwc):
    out = Normalize(MEAN, STD)(np.asarray(u8_hwc, dtype=np.float32))[0]
    return torch.from_numpy(np.ascontiguousarray(np.transpose(out, (2, 0, 1))))


def test_tta_none_is_the_existing_path_bit_for_bit(scenes, monkeypatch):
    init(F32)
    root, arrays = scenes
    img = arrays[0][0]
    sd = torch.from_numpy(img).cuda()
    monkeypatch.setattr(_lib, "tta_lib", lambda: (_ for _ in ()).throw(AssertionError("tta='none' loaded the fifth library")))
    stub = Stub(equivariant=False)
    res = _predictor(stub, tta="none", overlay=0.3)(sd)
    old = _predictor(stub, overlay=0.3)(sd)
    for a, b in zip(res, old):
        assert torch.equal(a, b)
    want = infer.ss_inference(stub, [_normalised_chw(img).cuda()], [img.shape[:2]], True, None, STRIDE, CROP, NCLS)[0]
    assert torch.equal(res.index.long().cpu(), want[0, 0].long().cpu()) and len(torch.unique(res.index)) > 2
    assert torch.equal(res.areas.cpu(), torch.bincount(res.index.long().view(-1), minlength=NCLS).cpu())
    ev, ev_old = _evaluator(stub, root, tta="none"), _evaluator(stub, root)
    tot, tot_old = ev.evaluate().cpu(), ev_old.evaluate().cpu()
    assert torch.equal(tot, tot_old) and torch.equal(ev.per_scene, ev_old.per_scene) and torch.equal(ev.predict(0)[0, 0].long().cpu(), want[0, 0].long().cpu())


def test_predict_tiles_under_the_flips_equals_the_per_tile_reference():
    init(F32)
    rng = np.random.RandomState(5500)
    tiles = rng.randint(0, 256, (5, 32, 32, 3)).astype(np.uint8)
    stub = Stub(equivariant=False)
    codes = R.MODES["flips"]
    res = _predictor(stub, tta="flips", max_batch=9).predict_tiles(torch.from_numpy(tiles).cuda())          # 9 // 4 = 2 tiles per model call
    assert [lg.shape[0] for lg in stub.logits] == [8, 8, 4]
    logits = np.concatenate(stub.logits)
    index = res.index.cpu().numpy()
    bound = R.bound(1, 4, NCLS)
    undecided = 0
    for j in range(5):
        want, cnt = R.accumulate(logits[4 * j:4 * j + 4], [(0, 0)], codes, 32, 32)
        ref_index, decided = _decided(want, bound)
        undecided += int((~decided).sum())
        assert np.array_equal(index[j][decided], ref_index[decided]) and np.all(cnt == 4)
    assert undecided <= 0.01 * index.size and len(np.unique(index)) > 2
    assert np.array_equal(res.areas.cpu().numpy(), np.bincount(index.reshape(-1), minlength=NCLS))
    assert np.array_equal(res.color.cpu().numpy(), vis.get_palette("Potsdam")[index])


# ---- 4. a real model ---------------------------------------------------------------------------------------------------------------------------
def test_resnet18_scene_under_d4():
    """ResNet-18 EMRT (conditioned and calibrated as tests/test_gpu_model.py does) at crop 64 on a 96 x 128 scene: six windows, two per model call
    with their eight variants each; the sums against the reference recomputed from the model's own logits on the same batches"""
    from emrt_amd.src.api import scene as S
    from tests.test_gpu_model import build_pair
    g = torch.Generator().manual_seed(5600)
    _, model = build_pair("resnet18", torch.randn(2, 3, 64, 64, generator=g), condition=0.1)
    model.eval()
    seen = []

    def recording(x):
        out = model(x)
        seen.append(out[0].cpu().numpy())
        return out

    H, W, crop, stride, codes = 96, 128, (64, 64), (32, 32), R.MODES["d4"]
    scene = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    final = torch.zeros(1, NCLS, H, W, device="cuda")
    count = torch.zeros(1, 1, H, W, device="cuda")
    mean, stdinv = S.check_normalise(MEAN, STD)
    S.accumulate_windows(recording, scene, H, W, crop, stride, NCLS, 16, mean, stdinv, final, count, tuple(codes))
    assert [lg.shape for lg in seen] == [(16, NCLS, 64, 64)] * 3
    want, cnt, K = _reference(seen, H, W, crop, stride, codes, 16)
    org = [(a, b) for (a, b, _, _) in infer.window_grid(H, W, crop, stride)]
    got = final[0].double().cpu().numpy()
    assert K == 4 and np.isfinite(got).all() and np.array_equal(count[0, 0].cpu().numpy(), 8.0 * R.cover(H, W, org, 64, 64))
    err = np.abs(got - want).max()
    print("tta resnet18 d4: max |device sums - float64| = %.3g, bound %.3g" % (err, R.bound(K, 8, NCLS)))
    assert err <= R.bound(K, 8, NCLS)
    res = S.ScenePredictor(model, NCLS, crop, stride, vis.get_palette("Potsdam"), MEAN, STD, max_batch=16, tta="d4")(scene)
    ref_index, decided = _decided(want, R.bound(K, 8, NCLS))
    assert np.array_equal(res.index.cpu().numpy()[decided], ref_index[decided]) and int(res.areas.sum()) == H * W
