"""CPU: the host side of native-resolution scene evaluation -- the launches one SceneEvaluator.evaluate() issues (on the recording
stand-in tests/fake_abi.py: nothing is computed), its refusals and those of `train.py --eval_scenes`, the validation SceneBank, val.metric_tuple
against val.evaluate, and the label selector check of emrt_segmentation_areas (host code: it returns before anything touches a device)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_scene_sampler_cpu import write_scene_tree

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
VAL_SUB = ("val_images", "val_labels")


class _Model:
    """stands where the network stands: fp32 [n, ncls, h, w] logits for an fp32 [n, 3, h, w] batch, and a record of the calls"""

    def __init__(self, ncls):
        self.ncls, self.batches, self.evals = ncls, [], 0

    def eval(self):
        self.evals += 1

    def __call__(self, x):
        self.batches.append(tuple(x.shape))
        return [torch.zeros(x.shape[0], self.ncls, x.shape[2], x.shape[3])]


@pytest.fixture
def fake():
    from tests import fake_abi
    lib = fake_abi.install()
    yield lib
    fake_abi.uninstall()


def _bank(root, sizes, shift=0, **kw):
    from emrt_amd.src.datasets import SceneBank
    arrays = write_scene_tree(str(root), sizes, sub=VAL_SUB, **kw)
    return SceneBank(str(root), "cpu", shift, sub=VAL_SUB, shift_on_upload=True), arrays


def _evaluator(bank, ncls=6, crop=(64, 64), stride=(48, 48), **kw):
    from emrt_amd.src.api.scene import SceneEvaluator
    model = _Model(ncls)
    return model, SceneEvaluator(model, bank, ncls, crop, stride, MEAN, STD, **kw)


def _origins_of(args, pos, n):
    arr = ctypes.cast(args[pos], ctypes.POINTER(ctypes.c_int))
    return [(arr[2 * j], arr[2 * j + 1]) for j in range(n)]


# ---- the launches of one evaluation ------------------------------------------------------------------------------------------------------
def test_evaluate_issues_crop_model_accumulate_normalise_argmax_areas_per_scene(fake, tmp_path):
    from emrt_amd.src.api import infer
    sizes = [(64, 64), (130, 200)]
    bank, _ = _bank(tmp_path, sizes)
    model, ev = _evaluator(bank, max_batch=5, ignore_index=255)
    assert fake.calls == []                                  # nothing is launched by the constructor
    tot = ev.evaluate()
    assert tot.shape == (3, 6) and tot.dtype == torch.int64 and ev.per_scene.shape == (2, 3, 6) and ev.per_scene.dtype == torch.int64
    assert model.evals == 1
    launches = [(n, a) for n, a in fake.calls if n != "emrt_memset"]
    base = bank.buffer.data_ptr()
    k, batches = 0, []
    for i, (H, W) in enumerate(sizes):
        wins = infer.window_grid(H, W, (64, 64), (48, 48))
        chunks = [wins[j:j + 5] for j in range(0, len(wins), 5)]
        if (H, W) == (130, 200):
            assert [len(c) for c in chunks] == [5, 5, 2]      # 12 windows: a short last chunk
        for chunk in chunks:
            (n1, crop), (n2, acc) = launches[k], launches[k + 1]
            assert (n1, n2) == ("emrt_scene_crop_windows_u8", "emrt_window_accumulate")
            want = [(a, b) for (a, b, _, _) in chunk]
            assert crop[0].value == base + bank.offsets[i][0]                     # the bank's own bytes, no copy
            assert crop[3:8] == (len(chunk), H, W, 64, 64) and _origins_of(crop, 2, len(chunk)) == want
            assert list(crop[8:14]) == MEAN + [1.0 / s for s in STD]
            assert acc[4:10] == (len(chunk), 6, H, W, 64, 64) and _origins_of(acc, 3, len(chunk)) == want
            batches.append((len(chunk), 3, 64, 64))
            k += 2
        (n1, norm), (n2, arg), (n3, area) = launches[k:k + 3]
        assert (n1, n2, n3) == ("emrt_window_normalise", "emrt_argmax_nchw", "emrt_segmentation_areas")
        assert norm[0].value == acc[1].value and norm[1].value == acc[2].value and norm[3:6] == (6, H, W)      # the sums and counts just accumulated
        assert arg[0].value == norm[2].value and arg[2:6] == (1, 6, H, W)
        assert area[0].value == arg[1].value                                      # the int32 prediction
        assert area[1].value == base + bank.offsets[i][1]                         # the label map where it lies: buffer + lab_off
        assert area[2] == 2 and area[3] == H * W and area[4] == 6 and area[5] == 255
        assert area[6].value == ev.per_scene[i].data_ptr()
        k += 3
    assert k == len(launches) and model.batches == batches
    # the sums and counts of every scene are zeroed before its windows are added, and per_scene before the first scene
    zeroed = [a[0].value for n, a in fake.calls if n == "emrt_memset"]
    assert ev.per_scene.data_ptr() in zeroed
    for n, a in launches:
        if n == "emrt_window_normalise":
            assert a[0].value in zeroed and a[1].value in zeroed


def test_scratch_is_allocated_once_per_scene_shape_and_reused(fake, tmp_path):
    bank, _ = _bank(tmp_path, [(64, 80), (70, 64), (64, 80)])
    _, ev = _evaluator(bank)
    ev.evaluate()
    first = [a for n, a in fake.calls if n == "emrt_argmax_nchw"]
    assert first[0][1].value == first[2][1].value != first[1][1].value and first[0][0].value == first[2][0].value
    del fake.calls[:]
    ev.evaluate()
    again = [a for n, a in fake.calls if n == "emrt_argmax_nchw"]
    assert [(a[0].value, a[1].value) for a in again] == [(a[0].value, a[1].value) for a in first]
    assert len(ev._scratch) == 2


def test_rank_shard_touches_only_its_scenes(fake, tmp_path):
    bank, _ = _bank(tmp_path, [(64, 64), (64, 70), (70, 64)])
    _, ev = _evaluator(bank)
    ev.evaluate(rank=1, nranks=2)
    areas = [a for n, a in fake.calls if n == "emrt_segmentation_areas"]
    assert len(areas) == 1 and areas[0][6].value == ev.per_scene[1].data_ptr() and areas[0][3] == 64 * 70


def test_multi_scale_takes_the_whole_scene_as_one_window_and_the_argmax_of_the_softmax_sums(fake, tmp_path):
    bank, _ = _bank(tmp_path, [(96, 150)])
    _, ev = _evaluator(bank, scales=(0.75, 1.0))
    ev.evaluate()
    names = [n for n, _ in fake.calls if n != "emrt_memset"]
    first = [a for n, a in fake.calls if n == "emrt_scene_crop_windows_u8"]
    assert len(first) == 1 and first[0][3:8] == (1, 96, 150, 96, 150)
    assert names.count("emrt_softmax_nchw_acc") == 4 and names[-2:] == ["emrt_argmax_nchw", "emrt_segmentation_areas"]
    assert "emrt_window_normalise" in names                  # slide_inference's own, inside ms_accumulate
    assert fake.calls[-1][1][2] == 2


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_refusals_by_name_before_any_launch(fake, tmp_path):
    bank, _ = _bank(tmp_path, [(64, 64), (64, 63)], names=["big", "narrow"])
    for stride in ((65, 32), (32, 65)):
        with pytest.raises(ValueError, match="uncovered stripes"):
            _evaluator(bank, crop=(63, 63), stride=stride)
    with pytest.raises(ValueError) as e:
        _evaluator(bank)
    assert "narrow" in str(e.value) and "64x63" in str(e.value) and "64x64" in str(e.value), str(e.value)
    for ncls in (0, 257):
        with pytest.raises(ValueError, match="num_classes must be 1..256"):
            _evaluator(bank, ncls=ncls, crop=(63, 63))
    for mb in (0, 65):
        with pytest.raises(ValueError, match="max_batch must be 1..64"):
            _evaluator(bank, crop=(63, 63), max_batch=mb)
    _evaluator(bank, ncls=256, crop=(63, 63), max_batch=64)
    assert fake.calls == []


def test_eval_scenes_native_is_refused_without_scenes_or_with_no_eval():
    from emrt_amd import train
    assert train.parse_args([]).eval_scenes == "resized"
    with pytest.raises(SystemExit, match="--eval_scenes native needs --data scenes"):
        train.main(["--eval_scenes", "native"])
    with pytest.raises(SystemExit, match="--eval_scenes native needs --data scenes"):
        train.main(["--eval_scenes", "native", "--data", "dataset"])
    with pytest.raises(SystemExit, match="--eval_scenes native cannot be combined with --no-eval"):
        train.main(["--eval_scenes", "native", "--data", "scenes", "--no-eval"])
    with pytest.raises(SystemExit):                          # argparse: not one of the two choices
        train.parse_args(["--eval_scenes", "half"])


def test_val_parses_the_scenes_mode():
    from emrt_amd import val
    a = val.parse_args(["--data", "scenes", "--data_path", "/x", "--multi_scales"])
    assert a.data == "scenes" and a.data_path == "/x" and a.multi_scales


# ---- the validation bank -----------------------------------------------------------------------------------------------------------------
def test_validation_bank_packs_val_dirs_and_shifts_labels_with_wrap(tmp_path):
    from emrt_amd.src.datasets import SceneBank
    sizes = [(9, 13), (8, 8)]
    arrays = write_scene_tree(str(tmp_path), sizes, sub=VAL_SUB, label_values=[0, 1, 2, 7])
    with pytest.raises(FileNotFoundError):                   # the defaults still look for images/ + labels/
        SceneBank(str(tmp_path), "cpu")
    for shift in (0, 1):
        bank = SceneBank(str(tmp_path), "cpu", shift, sub=VAL_SUB, shift_on_upload=True)
        assert bank.sizes == sizes and bank.names == ["scene_0", "scene_1"] and bank.nbytes == 4 * (9 * 13 + 8 * 8)
        for i, (img, lab) in enumerate(arrays):
            im, lb = bank.scene(i)
            assert im.dtype == torch.uint8 and lb.dtype == torch.uint8 and im.shape == img.shape and lb.shape == lab.shape
            assert im.data_ptr() == bank.buffer.data_ptr() + bank.offsets[i][0] and lb.data_ptr() == bank.buffer.data_ptr() + bank.offsets[i][1]
            want = lab - np.uint8(1) if shift else lab       # Dataset.__getitem__ in `val` mode: class 0 -> 255, 255 -> 254
            assert np.array_equal(im.numpy(), img) and np.array_equal(lb.numpy(), want)
        if shift:
            assert 255 in bank.scene(0)[1].numpy() and 254 in bank.scene(0)[1].numpy() and 0 in bank.scene(0)[1].numpy()
    # without shift_on_upload the shift is left to the sampler's lookup table: the bytes are the decoded ones
    plain = SceneBank(str(tmp_path), "cpu", 1, sub=VAL_SUB)
    assert np.array_equal(plain.scene(0)[1].numpy(), arrays[0][1])


def test_default_bank_is_byte_identical_to_the_packing_of_images_and_labels(tmp_path):
    from emrt_amd.src.datasets import SceneBank
    sizes = [(9, 13), (8, 8)]
    arrays = write_scene_tree(str(tmp_path), sizes)
    want = np.concatenate([np.concatenate([img.reshape(-1), lab.reshape(-1)]) for img, lab in arrays])
    for kw in ({}, {"sub": ("images", "labels"), "shift_on_upload": False}):
        for shift in (0, 1):
            bank = SceneBank(str(tmp_path), "cpu", shift, **kw)
            assert np.array_equal(bank.buffer.numpy(), want) and bank.label_shift == shift
            assert bank.offsets == [(0, 3 * 9 * 13), (4 * 9 * 13, 4 * 9 * 13 + 3 * 8 * 8)]


# ---- metric_tuple ------------------------------------------------------------------------------------------------------------------------
def test_metric_tuple_is_the_second_half_of_evaluate(fake, monkeypatch):
    from emrt_amd import val
    from emrt_amd.config import get_config
    from emrt_amd.src.api import infer
    from emrt_amd.src.utils import metrics
    g = torch.Generator().manual_seed(5)
    ncls = 6
    labels = [torch.randint(0, ncls, (5, 7), generator=g), torch.randint(0, ncls, (4, 4), generator=g)]
    labels[0][0, :3] = 255
    preds = [torch.randint(0, ncls, (1, 1, 5, 7), generator=g).int(), torch.randint(0, ncls, (1, 1, 4, 4), generator=g).int()]
    preds[0][0, 0, 1] = labels[0][1]                          # some agreement
    images = [torch.zeros(3, 5, 7), torch.ones(3, 4, 4)]
    monkeypatch.setattr(infer, "ss_inference", lambda model, img, *a, **k: [preds[int(img[0][0, 0, 0])]])
    config = get_config()
    config.DATA.NUM_CLASSES = ncls
    got = val.evaluate(_Model(ncls), images, labels, config)
    tot = torch.zeros(3, ncls, dtype=torch.int64)
    for p, l in zip(preds, labels):
        for row, a in zip(tot, metrics.calculate_area(p, l, ncls, 255)):
            row += a
    want = val.metric_tuple(tot)
    assert len(got) == 8 and len(want) == 7 and got[0] >= 0.0
    for a, b in zip(got[1:], want):
        assert type(a) is type(b) and np.array_equal(np.asarray(a), np.asarray(b))
    assert 0.0 < want[0] < 1.0 and 0.0 < want[1] < 1.0


# ---- the library's own argument check ----------------------------------------------------------------------------------------------------
def test_segmentation_areas_refuses_an_unknown_label_selector_before_any_launch():
    from emrt_amd import _lib, build_ext
    build_ext.build(verbose=False)
    _lib._LIB = None
    L = _lib.lib()
    p = ctypes.c_void_p(0x10000)          # "a device pointer": aligned, never read
    for sel in (3, -1):
        assert L.query("emrt_segmentation_areas", p, p, sel, 16, 6, 255, p, None) != 0
        msg = L.last_error()
        assert "0 = int32" in msg and "1 = int64" in msg and "2 = uint8" in msg and "launch failed" not in msg, msg
        with pytest.raises(_lib.EmrtHipError, match="2 = uint8"):
            L.call("emrt_segmentation_areas", p, p, sel, 16, 6, 255, p, None)
    for sel in (0, 1, 2):                                    # the three values pass the check (n = 0: nothing is launched)
        assert L.query("emrt_segmentation_areas", p, p, sel, 0, 6, 255, p, None) == 0
    _lib._LIB = None
