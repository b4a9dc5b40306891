"""-m gpu: multi-scale test-time augmentation of whole-scene inference -- the two kernels of csrc/mstta_ext/mstta_ext.hip and
ScenePredictor / SceneEvaluator with tta_scales against the numpy float64 restatement tests/ms_tta_reference.py.

The crop kernel is held to M.crop_bound per value (8 * 255 * 2^-24 * stdinv_c + 2^-24 * |ref|) and is bit-equal to emrt_tta_crop_windows_u8 at
scale 1.  The sums of the accumulation kernel are held per pixel to the sum over the pixel's terms of M.acc_term_bound = (C + 8) * 2^-23 +
m * 2^-20, m the largest |logit| among the term's four taps.  Class indices are compared wherever the reference's two largest sums are further
apart than twice that bound; the share left out is asserted to be at most 1 % (tests/test_ms_tta_cpu.py judges the same share without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                  # noqa: E402
from emrt_amd.functional import P                          # noqa: E402
from emrt_amd.runtime import F32                           # noqa: E402
from emrt_amd.src.utils import metrics, vis                # noqa: E402
from tests import ms_tta_reference as M                    # noqa: E402
from tests import tta_reference as R                       # noqa: E402
from tests.hip_utils import init                           # noqa: E402
from tests.test_scene_sampler_cpu import write_scene_tree  # noqa: E402

MEAN, STD = M.MEAN, M.STD
STDINV = [float(v) for v in 1.0 / np.asarray(STD, dtype=np.float64)]
VAL_SUB = ("val_images", "val_labels")
ALL_MODES = ["none", "hflip", "flips", "d4"]


def _ints(values):
    arr = (ctypes.c_int * len(values))(*values)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _crop(scene, org, codes, fh, fw, ch, cw):
    """one emrt_mst_crop_windows_u8 launch on a uint8 [H, W, 3] numpy scene -> fp32 numpy [n * G, 3, ch, cw] (every element must be written)"""
    c = init(F32)
    sd = torch.from_numpy(scene).cuda()
    batch = torch.full((len(org) * len(codes), 3, ch, cw), float("nan"), device="cuda")
    _o, op = _ints([v for yx in org for v in yx])
    _k, kp = _ints(codes)
    _lib.mst_lib().call("emrt_mst_crop_windows_u8", P(sd), P(batch), op, len(org), kp, len(codes), scene.shape[0], scene.shape[1], fh, fw, ch, cw,
                        *MEAN, *STDINV, c.stream)
    return batch.cpu().numpy()


def _check_crop(got, want, what):
    bound = M.crop_bound(want)
    err = np.abs(got.astype(np.float64) - want)
    print("ms crop %s: max |kernel - float64| = %.3g, max error / bound = %.3g" % (what, err.max(), (err / bound).max()))
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and np.all(err <= bound)


# ---- 1. the crop kernel ------------------------------------------------------------------------------------------------------------------
def _border_origins(H, W, fh, fw):
    """the four corners (the last is the far one), a footprint flush with each border in between, and one inside"""
    return [(0, 0), (0, W - fw), (H - fh, 0), (3, 0), (0, 5), (H - fh, 4), (2, W - fw), (min(3, H - fh), min(2, W - fw)), (H - fh, W - fw)]


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("s", M.SCALES)
def test_crop_variants_are_within_the_bound_of_the_reference(s, mode):
    H, W, c = 37, 41, 16
    f = int(c / s + 0.5)
    assert f == {0.5: 32, 0.8: 20, 1.0: 16, 1.6: 10, 2.0: 8}[s]
    rng = np.random.RandomState(6100 + f)
    scene = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    scene[0, 0], scene[H - 1, W - 1] = (0, 255, 0), (255, 0, 255)
    codes = R.MODES[mode]
    org = _border_origins(H, W, f, f)[:64 // len(codes)]
    if (H - f, W - f) not in org:
        org[-1] = (H - f, W - f)
    got = _crop(scene, org, codes, f, f, c, c)
    want = M.crop_variants_ms(scene, org, codes, f, f, c, c)
    _check_crop(got, want, "37x41 f=%d %s" % (f, mode))
    assert len({want[g].tobytes() for g in range(len(codes))}) == len(codes)          # the variants differ: a wrong one would show
    if s == 1.0:
        c_ = init(F32)
        sd = torch.from_numpy(scene).cuda()
        ref = torch.full((len(org) * len(codes), 3, c, c), float("nan"), device="cuda")
        _o, op = _ints([v for yx in org for v in yx])
        _k, kp = _ints(codes)
        _lib.tta_lib().call("emrt_tta_crop_windows_u8", P(sd), P(ref), op, len(org), kp, len(codes), H, W, c, c, *MEAN, *STDINV, c_.stream)
        assert np.array_equal(got, ref.cpu().numpy())                                    # at scale 1: the bits of the fifth library's crop


@pytest.mark.parametrize("mode", ["none", "d4"])
def test_crop_of_a_ragged_footprint(mode):
    """64 x 96 scene, crop 32 at 0.75: a footprint of 43, source runs of ragged length; one full tile per window"""
    rng = np.random.RandomState(6143)
    scene = rng.randint(0, 256, (64, 96, 3)).astype(np.uint8)
    org = [(0, 0), (21, 53), (12, 20), (21, 0)]
    got = _crop(scene, org, R.MODES[mode], 43, 43, 32, 32)
    _check_crop(got, M.crop_variants_ms(scene, org, R.MODES[mode], 43, 43, 32, 32), "64x96 f=43 " + mode)


def test_crop_of_more_than_one_tile():
    """crop 40 at 0.8 (footprint 50): four ragged 32 x 32 tiles per window"""
    rng = np.random.RandomState(6150)
    scene = rng.randint(0, 256, (64, 96, 3)).astype(np.uint8)
    org = [(0, 0), (14, 46), (5, 9)]
    got = _crop(scene, org, R.MODES["d4"], 50, 50, 40, 40)
    _check_crop(got, M.crop_variants_ms(scene, org, R.MODES["d4"], 50, 50, 40, 40), "64x96 f=50 c=40 d4")


def test_crop_of_a_rectangle_under_the_flips():
    rng = np.random.RandomState(6200)
    scene = rng.randint(0, 256, (37, 41, 3)).astype(np.uint8)
    fh, fw = int(16 / 0.75 + 0.5), int(24 / 0.75 + 0.5)     # 24 x 16 (w x h) at 0.75: a 21 x 32 (h x w) footprint
    assert (fh, fw) == (21, 32)
    org = [(0, 0), (37 - fh, 41 - fw), (5, 3)]
    got = _crop(scene, org, R.MODES["flips"], fh, fw, 16, 24)
    _check_crop(got, M.crop_variants_ms(scene, org, R.MODES["flips"], fh, fw, 16, 24), "rectangle flips")


# ---- 2. the accumulation kernel -------------------------------------------------------------------------------------------------------------
def _accumulate(lib, name, logits, final, count, org, codes, dims):
    """the footprints in launches of 64 // G, added into the device tensors final [C, H, W] and count [H, W]; dims = (fh, fw, ch, cw) or (ch, cw)"""
    c = init(F32)
    G, per = len(codes), 64 // len(codes)
    _k, kp = _ints(codes)
    for i in range(0, len(org), per):
        chunk = org[i:i + per]
        _o, op = _ints([v for yx in chunk for v in yx])
        part = logits[i * G:(i + len(chunk)) * G]
        lib.call(name, P(part), P(final), P(count), op, len(chunk), kp, G, final.shape[0], final.shape[1], final.shape[2], *dims, c.stream)


@pytest.mark.parametrize("mode", M.ACC_MODES)
@pytest.mark.parametrize("s", M.SCALES)
@pytest.mark.parametrize("C", M.ACC_CLASSES)
def test_accumulate_equals_the_float64_sums_within_the_per_pixel_bound(C, s, mode):
    H, W = M.ACC_MAP
    codes = R.MODES[mode]
    G = len(codes)
    org, fh, fw, logits, final0, count0 = M.acc_case(C, s, mode)
    cover = R.cover(H, W, org, fh, fw)
    assert cover.max() == 4 and cover.min() >= 1 and (H - fh, W - fw) in org
    want, cnt, bound = M.accumulate_ms(logits, org, codes, H, W, fh, fw, final=final0.astype(np.float64), count=count0.astype(np.float64))
    lg = torch.from_numpy(logits).cuda()
    runs = []
    for _ in range(2):
        final, count = torch.from_numpy(final0).cuda(), torch.from_numpy(count0).cuda()
        _accumulate(_lib.mst_lib(), "emrt_mst_window_accumulate", lg, final, count, org, codes, (fh, fw, 16, 16))
        runs.append((final.cpu(), count.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])          # one fixed order: the same bits
    final, count = runs[0]
    assert np.array_equal(count.numpy(), cnt) and np.array_equal(cnt, count0 + G * cover)
    err = np.abs(final.double().numpy() - want).max(0)
    print("ms accumulate C=%d s=%g %s: max |kernel - float64| = %.3g, max error / bound = %.3g"
          % (C, s, mode, err.max(), (err / bound).max()))
    assert np.isfinite(final.numpy()).all() and np.all(err <= bound)
    if s == 1.0:
        f5, c5 = torch.from_numpy(final0).cuda(), torch.from_numpy(count0).cuda()
        _accumulate(_lib.tta_lib(), "emrt_tta_window_accumulate", lg, f5, c5, org, codes, (16, 16))
        diff = (f5.cpu() - final).abs().max().item()
        print("ms accumulate C=%d s=1 %s against emrt_tta_window_accumulate: max |diff| = %.3g, bits equal: %s" % (C, mode, diff, diff == 0.0))
        assert torch.equal(c5.cpu(), count) and diff <= R.bound(4, G, C)


# ---- 3. the pipeline on stub models -----------------------------------------------------------------------------------------------------------
NCLS, CROP, STRIDE, MAX_BATCH, SCALES = M.PIPE_NCLS, M.PIPE_CROP, M.PIPE_STRIDE, M.PIPE_MAX_BATCH, M.PIPE_SCALES


class Stub:
    """A model on the device made of elementwise torch arithmetic, from M.stub_params: a fixed 1 x 1 channel mix plus a fixed position ramp
    (neither equivariant nor scale-invariant), or -- const -- the same logits at every pixel (exactly both).  Records the logits of every call."""

    def __init__(self, const=False):
        mix, ramp = M.stub_params(equivariant=False)
        self.mix, self.ramp = torch.from_numpy(mix).cuda(), torch.from_numpy(ramp).cuda()
        self.const = torch.tensor(M.CONST_LOGITS, device="cuda").view(1, -1, 1, 1) if const else None
        self.logits = []

    def eval(self):
        pass

    def __call__(self, x):
        if self.const is not None:
            out = self.const.expand(x.shape[0], NCLS, x.shape[2], x.shape[3]).contiguous()
        else:
            m = self.mix
            out = m[:, 0].view(1, -1, 1, 1) * x[:, 0:1] + m[:, 1].view(1, -1, 1, 1) * x[:, 1:2] + m[:, 2].view(1, -1, 1, 1) * x[:, 2:3]
            out = (out + self.ramp).contiguous()
        self.logits.append(out.cpu().numpy())
        return [out]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """(root of the validation tree, [(img uint8 HWC, lab uint8 HW)]) for M.PIPE_SIZES: seeded noise, labels 0..5 with some 255"""
    root = str(tmp_path_factory.mktemp("ms_tta_scenes"))
    return root, write_scene_tree(root, M.PIPE_SIZES, sub=VAL_SUB, seed=M.PIPE_SEED)


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


def _decided(want, bound):
    """(reference class index, the pixels whose two largest reference sums are more than 2 * bound apart)"""
    top = np.sort(want, axis=0)
    return want.argmax(0), (top[-1] - top[-2]) > 2 * bound


def _check_recorded_logits(recorded, img, codes):
    """Every model call's logits against the stub, in float64, on the reference's own resampled windows.  Tolerance per value: the crop bound
    of each input through |mix|, plus 8 fp32 roundings (three products, three additions, two spare) at the magnitude sum |mix x| + |ramp|."""
    mix, ramp = M.stub_params(equivariant=False)
    H, W = img.shape[:2]
    G, per = len(codes), MAX_BATCH // len(codes)
    amix = np.abs(mix.astype(np.float64))
    for s in SCALES:
        (fw, fh), _, org = M.footprints(H, W, CROP, STRIDE, s)
        for i in range(0, len(org), per):
            batch = M.crop_variants_ms(img, org[i:i + per], codes, fh, fw, CROP[1], CROP[0])
            tol = np.einsum("kc,nchw->nkhw", amix, M.crop_bound(batch)) + 8 * 2.0 ** -24 * (np.einsum("kc,nchw->nkhw", amix, np.abs(batch)) + np.abs(ramp))
            got = recorded.pop(0)
            assert got.shape[0] == batch.shape[0] == len(org[i:i + per]) * G and np.all(np.abs(got - M.stub_logits(batch, mix, ramp)) <= tol), (s, i)
    assert not recorded


@pytest.mark.parametrize("mode", M.PIPE_MODES)
def test_pipeline_with_a_stub_that_is_neither_equivariant_nor_scale_invariant(scenes, mode):
    from emrt_amd.src.api import scene as S
    init(F32)
    root, arrays = scenes
    codes = R.MODES[mode]
    img = arrays[0][0]
    H, W = img.shape[:2]
    sd = torch.from_numpy(img).cuda()
    # the pass itself, for its sums
    stub = Stub()
    final = torch.zeros(1, NCLS, H, W, device="cuda")
    count = torch.zeros(1, 1, H, W, device="cuda")
    p = _predictor(stub, tta=mode, tta_scales=SCALES, overlay=0.5)
    S.accumulate_windows_ms(stub, sd, H, W, p.crop, p.stride, NCLS, MAX_BATCH, p.mean, p.stdinv, final, count, p.codes, p.tta_scales)
    # (a) against the reference fed with the device's own logits: the accumulation alone
    want, cnt, bound = M.pipeline_reference(img, CROP, STRIDE, SCALES, codes, MAX_BATCH, None, logits=list(stub.logits))
    err = np.abs(final[0].double().cpu().numpy() - want).max(0)
    print("ms pipeline %s: max |device sums - float64| = %.3g, max error / bound = %.3g" % (mode, err.max(), (err / bound).max()))
    assert np.all(err <= bound) and np.array_equal(count[0, 0].cpu().numpy(), cnt) and cnt.min() >= len(SCALES) * len(codes)
    # (b) the logits the model was called for, against the reference's own crops put through the stub in float64: the crop inside the pass
    _check_recorded_logits(list(stub.logits), img, codes)
    # (c) class indices where the reference decides
    ref_index, decided = _decided(want, bound)
    assert 1.0 - decided.mean() <= 0.01, "the reference alone leaves %.2f %% of the pixels undecided" % (100 * (1 - decided.mean()))
    res = p(sd)
    index = res.index.cpu().numpy()
    assert np.array_equal(index[decided], ref_index[decided]) and len(np.unique(index)) > 2
    assert np.array_equal(res.areas.cpu().numpy(), np.bincount(index.reshape(-1), minlength=NCLS)) and int(res.areas.sum()) == H * W
    pal = vis.get_palette("Potsdam")
    assert np.array_equal(res.color.cpu().numpy(), pal[index])
    assert np.array_equal(res.overlay.cpu().double().numpy(), np.floor(0.5 * pal[index].astype(np.float64) + 0.5 * img.astype(np.float64) + 0.5))
    # the evaluator over both scenes
    stub = Stub()
    ev = _evaluator(stub, root, tta=mode, tta_scales=SCALES)
    tot = ev.evaluate().cpu()
    recorded = list(stub.logits)
    for i, (h, w) in enumerate(M.PIPE_SIZES):
        want, cnt, bound = M.pipeline_reference(arrays[i][0], CROP, STRIDE, SCALES, codes, MAX_BATCH, None, logits=recorded)
        ref_index, decided = _decided(want, bound)
        assert 1.0 - decided.mean() <= 0.01
        f, c, _, pred = ev._buffers(h, w)                  # (one scene per shape: what evaluate() left there)
        pred = pred.cpu()
        assert np.all(np.abs(f[0].double().cpu().numpy() - want).max(0) <= bound) and np.array_equal(c[0, 0].cpu().numpy(), cnt)
        assert np.array_equal(pred[0, 0].numpy()[decided], ref_index[decided])
        if i == 0:
            assert np.array_equal(pred[0, 0].numpy(), index)                 # the predictor's map of the same scene
        area = torch.stack(metrics.calculate_area(pred, torch.from_numpy(arrays[i][1]), NCLS, 255))
        assert torch.equal(ev.per_scene[i].cpu(), area)
    assert not recorded and torch.equal(tot, ev.per_scene.cpu().sum(0))


@pytest.mark.parametrize("mode", M.PIPE_MODES)
def test_a_stub_that_is_equivariant_and_scale_invariant_votes_its_own_softmax(scenes, mode):
    """the same logits at every pixel: every blend is the logit itself, so sums / counts is that softmax at every pixel of every scene"""
    init(F32)
    root, arrays = scenes
    codes = R.MODES[mode]
    prob = R.softmax(np.asarray(M.CONST_LOGITS), axis=0)
    ev = _evaluator(Stub(const=True), root, tta=mode, tta_scales=SCALES)
    for i, (h, w) in enumerate(M.PIPE_SIZES):
        pred = ev.predict(i).cpu().numpy()
        f, c, _, _ = ev._buffers(h, w)
        cnt = c[0, 0].double().cpu().numpy()
        err = np.abs(f[0].double().cpu().numpy() - prob[:, None, None] * cnt).max(0)
        assert cnt.min() >= len(SCALES) * len(codes) and np.all(err <= cnt * M.acc_term_bound(NCLS, max(np.abs(M.CONST_LOGITS))))
        assert np.all(pred == int(np.argmax(M.CONST_LOGITS)))
    sd = torch.from_numpy(arrays[0][0]).cuda()
    assert torch.all(_predictor(Stub(const=True), tta=mode, tta_scales=SCALES)(sd).index == int(np.argmax(M.CONST_LOGITS)))


@pytest.mark.parametrize("mode", M.PIPE_MODES)
def test_scale_one_alone_is_the_tta_path_within_both_bounds(scenes, mode):
    from emrt_amd.src.api import scene as S
    init(F32)
    _, arrays = scenes
    img = arrays[0][0]
    H, W = img.shape[:2]
    sd = torch.from_numpy(img).cuda()
    codes = R.MODES[mode]
    sums = []
    for kw in ({"tta_scales": (1.0,)}, {}):
        stub = Stub()
        p = _predictor(stub, tta=mode, **kw)
        final = torch.zeros(1, NCLS, H, W, device="cuda")
        count = torch.zeros(1, 1, H, W, device="cuda")
        if kw:
            S.accumulate_windows_ms(stub, sd, H, W, p.crop, p.stride, NCLS, MAX_BATCH, p.mean, p.stdinv, final, count, p.codes, p.tta_scales)
        elif mode == "none":          # the plain path sums logits, not probabilities: take the fifth library's sums of the one variant
            org = [(a, b) for (a, b, _, _) in S.infer.window_grid(H, W, p.crop, p.stride)]
            S.accumulate_windows_tta(stub, sd, H, W, org, p.crop, NCLS, MAX_BATCH, p.mean, p.stdinv, final, count, p.codes)
        else:
            S.accumulate_windows(stub, sd, H, W, p.crop, p.stride, NCLS, MAX_BATCH, p.mean, p.stdinv, final, count, p.codes)
        sums.append((final[0].double().cpu().numpy(), count[0, 0].cpu().numpy(), list(stub.logits)))
    (f_ms, c_ms, lg_ms), (f_tta, c_tta, lg_tta) = sums
    assert all(np.array_equal(a, b) for a, b in zip(lg_ms, lg_tta)) and len(lg_ms) == len(lg_tta)          # the same batches, bit for bit
    _, _, bound = M.pipeline_reference(img, CROP, STRIDE, (1.0,), codes, MAX_BATCH, None, logits=list(lg_ms))
    K = c_tta.max() / len(codes)
    diff = np.abs(f_ms - f_tta).max(0)
    print("ms pipeline %s at scale 1 against the tta path: max |diff| = %.3g" % (mode, diff.max()))
    assert np.array_equal(c_ms, c_tta) and np.all(diff <= bound + R.bound(K, len(codes), NCLS))


def test_no_scales_is_the_existing_path_bit_for_bit(scenes, monkeypatch):
    init(F32)
    root, arrays = scenes
    sd = torch.from_numpy(arrays[0][0]).cuda()

    def refuse():
        raise AssertionError("tta_scales=None loaded the sixth library")

    monkeypatch.setattr(_lib, "mst_lib", refuse)
    for mode in ("none", "d4"):
        stub = Stub()
        res = _predictor(stub, tta=mode, tta_scales=None, overlay=0.3)(sd)
        old = _predictor(stub, tta=mode, overlay=0.3)(sd)
        for a, b in zip(res, old):
            assert torch.equal(a, b)
        assert len(torch.unique(res.index)) > 2
        ev, ev_old = _evaluator(stub, root, tta=mode, tta_scales=None), _evaluator(stub, root, tta=mode)
        assert torch.equal(ev.evaluate().cpu(), ev_old.evaluate().cpu()) and torch.equal(ev.per_scene, ev_old.per_scene)


# ---- 4. a real model ---------------------------------------------------------------------------------------------------------------------------
def test_resnet18_scene_under_hflip_and_three_scales():
    """ResNet-18 EMRT (conditioned and calibrated as tests/test_gpu_model.py does) at crop 64 on a 96 x 128 scene under hflip with scales
    (0.75, 1.0, 1.25): the sums against the reference recomputed from the model's own logits on the same batches"""
    from emrt_amd.src.api import scene as S
    from tests.test_gpu_model import build_pair
    g = torch.Generator().manual_seed(6600)
    _, model = build_pair("resnet18", torch.randn(2, 3, 64, 64, generator=g), condition=0.1)
    model.eval()
    seen = []

    def recording(x):
        out = model(x)
        seen.append(out[0].cpu().numpy())
        return out

    H, W, crop, stride, codes, scales = 96, 128, (64, 64), (32, 32), R.MODES["hflip"], (0.75, 1.0, 1.25)
    scene = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    final = torch.zeros(1, NCLS, H, W, device="cuda")
    count = torch.zeros(1, 1, H, W, device="cuda")
    mean, stdinv = S.check_normalise(MEAN, STD)
    S.accumulate_windows_ms(recording, scene.cuda(), H, W, crop, stride, NCLS, 16, mean, stdinv, final, count, tuple(codes), scales)
    want, cnt, bound = M.pipeline_reference(scene.numpy(), crop, stride, scales, codes, 16, None, logits=seen)
    got = final[0].double().cpu().numpy()
    assert not seen and np.isfinite(got).all() and np.array_equal(count[0, 0].cpu().numpy(), cnt) and cnt.min() >= 6
    err = np.abs(got - want).max(0)
    print("ms resnet18 hflip x 3 scales: max |device sums - float64| = %.3g, max error / bound = %.3g" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound)
    res = S.ScenePredictor(model, NCLS, crop, stride, vis.get_palette("Potsdam"), MEAN, STD, max_batch=16, tta="hflip", tta_scales=scales)(scene.cuda())
    ref_index, decided = _decided(want, bound)
    assert np.array_equal(res.index.cpu().numpy()[decided], ref_index[decided]) and int(res.areas.sum()) == H * W
