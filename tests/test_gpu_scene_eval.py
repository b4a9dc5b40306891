"""-m gpu: native-resolution scene evaluation -- emrt_segmentation_areas on uint8 labels at any byte offset against the torch
bincount expression, api.scene.SceneEvaluator over a resident validation bank against val.evaluate() fed with the host-normalised full-size
scenes, and the two command lines.  Every comparison is between integers and exact."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd.src.transforms import Normalize                            # noqa: E402
from emrt_amd.src.utils import metrics, vis                              # noqa: E402
from tests.hip_utils import init                                         # noqa: E402
from emrt_amd.runtime import F32                                         # noqa: E402
from tests.test_scene_sampler_cpu import write_scene_tree                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "emrt_amd/configs/EMRT")
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]          # VAL.MEAN / VAL.STD of every shipped config
CROP, STRIDE, NCLS = (64, 64), (48, 48), 6
SIZES = [(64, 64), (96, 150), (130, 200)]
VAL_SUB = ("val_images", "val_labels")


# ---- 1. the kernel on uint8 labels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,offset,ignore", [(3 * 517 * 389, 0, 255), (1, 1, 255), (1, 3, 255), (4099, 1, 255), (4099, 3, 255), (4099, 3, 0)])
def test_segmentation_areas_on_uint8_labels_equals_the_torch_expression(n, offset, ignore):
    """Selector 2 through metrics.calculate_area: the label view starts `offset` bytes into an allocation of 8 n (+ offset) bytes filled with
    valid class bytes, so code that read it as int32 / int64 would stay inside it and count other numbers.  Predictions hold -1 and ncls,
    labels ncls, ncls + 1 and 255; exact equality with the torch expression on CPU copies."""
    init(F32)
    g = torch.Generator().manual_seed(43 + n % 97 + offset)
    ncls = 7
    pred = torch.randint(-1, ncls + 1, (n,), generator=g).to(torch.int32)
    raw = torch.randint(0, ncls, (8 * n + offset,), generator=g).to(torch.uint8)
    lab = torch.randint(0, ncls + 2, (n,), generator=g).to(torch.uint8)
    lab[torch.rand(n, generator=g) < 0.1] = 255
    if n > 1:
        pred[:4] = torch.tensor([-1, ncls, 0, 3], dtype=torch.int32)
        lab[:4] = torch.tensor([ncls, ncls + 1, 0, 255], dtype=torch.uint8)
    raw[offset:offset + n] = lab
    want = metrics.calculate_area(pred, lab, ncls, ignore)                    # CPU tensors: the torch expression
    raw_d = raw.cuda()
    assert raw_d.data_ptr() % 16 == 0
    lab_d = raw_d[offset:offset + n]
    assert lab_d.is_contiguous() and lab_d.dtype == torch.uint8 and lab_d.data_ptr() % 4 == offset % 4
    got = metrics.calculate_area(pred.cuda(), lab_d, ncls, ignore)
    torch.cuda.synchronize()
    for a, b, name in zip(got, want, ("intersect", "pred", "label")):
        assert a.is_cuda and a.dtype == torch.int64 and torch.equal(a.cpu(), b), (name, a.cpu().tolist(), b.tolist())
    if n > 1:
        assert int(want[2].sum()) > 0 and int(want[0].sum()) > 0 and int(want[1].sum()) < n


# ---- 2. the evaluator -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resnet18():
    """ResNet-18 EMRT, 6 classes, fp32, seeded; residual branches conditioned and BatchNorm statistics calibrated as tests/test_gpu_model.py does
    (so that the predictions hold several classes)"""
    from tests.test_gpu_model import build_pair
    g = torch.Generator().manual_seed(4600)
    x = torch.randn(2, 3, 64, 64, generator=g)
    _, model = build_pair("resnet18", x, condition=0.1)
    model.eval()
    return model


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """(root, [(img uint8 HWC, lab uint8 HW)]) of the three validation scenes; labels 0..5 with 5 % of 255"""
    root = str(tmp_path_factory.mktemp("val_scenes"))
    return root, write_scene_tree(root, SIZES, sub=VAL_SUB)


def _bank(root, shift=0):
    from emrt_amd.src.datasets import SceneBank
    return SceneBank(root, "cuda:0", shift, sub=VAL_SUB, shift_on_upload=True)


def _evaluator(model, bank, **kw):
    from emrt_amd.src.api.scene import SceneEvaluator
    kw.setdefault("max_batch", 32)
    return SceneEvaluator(model, bank, NCLS, CROP, STRIDE, MEAN, STD, ignore_index=255, **kw)


def _normalised_chw(u8_hwc):
    """transforms.Normalize on the CPU, as the validation pipeline applies it, and no Resize -> fp32 CHW tensor"""
    out = Normalize(MEAN, STD)(np.asarray(u8_hwc, dtype=np.float32))[0]
    return torch.from_numpy(np.ascontiguousarray(np.transpose(out, (2, 0, 1))))


def _config(scales=None):
    from emrt_amd.config import get_config
    config = get_config()
    config.DATA.NUM_CLASSES = NCLS
    config.VAL.CROP_SIZE, config.VAL.STRIDE_SIZE = list(CROP), list(STRIDE)
    config.VAL.RESCALE_FROM_ORI = False
    config.TRAIN.IGNORE_INDEX = 255
    if scales is not None:
        config.VAL.SCALE_RATIOS = list(scales)
    return config


def _totals_behind_evaluate(monkeypatch, model, arrays, shift=0, scales=None):
    """val.evaluate() over the host-normalised full-size scenes and their label maps (shifted as Dataset.__getitem__ shifts them in `val` mode)
    -> (the int64 [3, ncls] totals it summed, per image [n, 3, ncls], its metric tuple)"""
    from emrt_amd import val
    images = [_normalised_chw(img) for img, _ in arrays]
    labels = [torch.from_numpy((lab - np.uint8(1) if shift else lab).astype(np.int64)) for _, lab in arrays]
    seen = []
    area = metrics.calculate_area

    def recording(*a, **k):
        out = area(*a, **k)
        seen.append(torch.stack([t.clone() for t in out]))
        return out

    monkeypatch.setattr(metrics, "calculate_area", recording)
    got = val.evaluate(model, images, labels, _config(scales), multi_scales=scales is not None)
    monkeypatch.setattr(metrics, "calculate_area", area)
    per = torch.stack(seen).cpu()
    assert per.shape == (len(arrays), 3, NCLS)
    return per.sum(0), per, got[1:]


def _same_tuple(a, b):
    assert len(a) == len(b) == 7
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_evaluator_totals_equal_the_totals_behind_evaluate(resnet18, tree, monkeypatch):
    from emrt_amd import val
    root, arrays = tree
    want, want_per, want_tuple = _totals_behind_evaluate(monkeypatch, resnet18, arrays)
    ev = _evaluator(resnet18, _bank(root))
    tot = ev.evaluate()
    assert tot.is_cuda and tot.dtype == torch.int64 and torch.equal(tot.cpu(), want), (tot.cpu().tolist(), want.tolist())
    assert torch.equal(ev.per_scene.cpu(), want_per)
    _same_tuple(val.metric_tuple(tot), want_tuple)
    n_valid = sum(int((lab != 255).sum()) for _, lab in arrays)
    assert int(want[2].sum()) == n_valid == int(want[1].sum()) and 0 < int(want[0].sum()) < n_valid
    assert int((want[1] > 0).sum()) > 1, "a one-class prediction would compare little"
    assert len(val.scene_lines(ev)) == 3 and "scene_2 (130x200)" in val.scene_lines(ev)[2]


def test_evaluator_with_label_shift_one_counts_class_zero_as_ignored(resnet18, tmp_path, monkeypatch):
    """LoveDA's convention: stored 0 = no data -> 255 (ignored), k -> k - 1; the file's 255 -> 254, outside the classes: counted nowhere."""
    root = str(tmp_path)
    arrays = write_scene_tree(root, [(64, 64), (96, 150)], sub=VAL_SUB, label_values=list(range(0, NCLS + 1)))
    assert all((lab == 0).any() for _, lab in arrays)
    want, want_per, _ = _totals_behind_evaluate(monkeypatch, resnet18, arrays, shift=1)
    ev = _evaluator(resnet18, _bank(root, shift=1))
    tot = ev.evaluate()
    assert torch.equal(tot.cpu(), want) and torch.equal(ev.per_scene.cpu(), want_per)
    assert int(want[2].sum()) == sum(int(((lab != 0) & (lab != 255)).sum()) for _, lab in arrays)


def test_chunks_of_five_equal_the_scene_predictor_and_the_cpu_bincount(resnet18, tree):
    from emrt_amd.src.api import infer
    from emrt_amd.src.api.scene import ScenePredictor
    root, arrays = tree
    wins = infer.window_grid(130, 200, CROP, STRIDE)
    assert len(wins) == 12 and max(w[0] for w in wins) == 66 and max(w[1] for w in wins) == 136          # edge windows shifted back inside
    cover = np.zeros((130, 200), dtype=np.int64)
    for h1, w1, h2, w2 in wins:
        cover[h1:h2, w1:w2] += 1
    assert {2, 4} <= set(np.unique(cover).tolist())
    bank = _bank(root)
    ev = _evaluator(resnet18, bank, max_batch=5)            # chunks of 5, 5 and 2
    pred = ev.predict(2).clone()
    assert pred.dtype == torch.int32 and tuple(pred.shape) == (1, 1, 130, 200)
    res = ScenePredictor(resnet18, NCLS, CROP, STRIDE, vis.get_palette("Potsdam"), MEAN, STD, max_batch=5)(bank.scene(2)[0])
    assert torch.equal(pred[0, 0].long(), res.index.long())
    assert len(torch.unique(pred)) > 1
    ev.evaluate()
    want = torch.stack(metrics.calculate_area(pred.cpu(), torch.from_numpy(arrays[2][1]), NCLS, 255))
    assert torch.equal(ev.per_scene[2].cpu(), want)
    # the chunking does not move a prediction: the default of 32 (one chunk) gives the same map
    assert torch.equal(_evaluator(resnet18, bank).predict(2), pred)


def test_multi_scale_totals_equal_evaluate_multi_scales(resnet18, tmp_path, monkeypatch):
    root = str(tmp_path)
    arrays = write_scene_tree(root, [(96, 150)], sub=VAL_SUB, seed=3)
    scales = (0.75, 1.0, 1.25)
    want, _, _ = _totals_behind_evaluate(monkeypatch, resnet18, arrays, scales=scales)
    ev = _evaluator(resnet18, _bank(root), scales=scales)
    tot = ev.evaluate()
    assert torch.equal(tot.cpu(), want), (tot.cpu().tolist(), want.tolist())
    assert int(want[1].sum()) == int((arrays[0][1] != 255).sum())


def test_second_evaluation_after_a_weight_change_rezeroes_the_reused_scratch(resnet18, tree):
    root, _ = tree
    bank = _bank(root)
    ev = _evaluator(resnet18, bank)
    first = ev.evaluate().cpu()
    scratch = {k: [None if t is None else t.data_ptr() for t in v] for k, v in ev._scratch.items()}
    old = {k: v.detach().clone() for k, v in resnet18.state_dict().items()}
    try:
        new = {k: v.clone() for k, v in old.items()}
        new["uphead.conv_3.bias"][2] += 1000.0              # one weight: the classifier's bias of class 2, beyond any logit
        resnet18.load_state_dict(new)                        # marks the store: the next forward re-packs, as after a checkpoint load
        second = ev.evaluate().cpu()
        assert {k: [None if t is None else t.data_ptr() for t in v] for k, v in ev._scratch.items()} == scratch          # the same buffers
        assert not torch.equal(second, first) and int(second[1][2]) > int(first[1][2])
        assert int(second[1].sum()) == int(first[1].sum())   # still one prediction per counted pixel: nothing left over from the first pass
        fresh = _evaluator(resnet18, bank).evaluate().cpu()
        assert torch.equal(second, fresh)
    finally:
        resnet18.load_state_dict(old)
    assert torch.equal(ev.evaluate().cpu(), first)


def test_rank_one_of_two_touches_only_scene_one(resnet18, tree):
    root, _ = tree
    ev = _evaluator(resnet18, _bank(root))
    whole = ev.evaluate()
    per = ev.per_scene.cpu().clone()
    tot = ev.evaluate(rank=1, nranks=2)
    got = ev.per_scene.cpu()
    assert int(got[0].abs().sum()) == 0 and int(got[2].abs().sum()) == 0 and torch.equal(got[1], per[1]) and int(got[1].sum()) > 0
    assert torch.equal(tot.cpu(), per[1])
    assert torch.equal(ev.evaluate(rank=0, nranks=2).cpu() + per[1], whole.cpu())


# ---- 3. the command lines ---------------------------------------------------------------------------------------------------------------
def _tiny_yaml(tmp_path, extra=""):
    cfg = str(tmp_path / "tiny.yaml")
    with open(cfg, "w") as f:
        f.write('BASE: ["%s"]\n' % os.path.relpath(os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam.yaml"), str(tmp_path)))
        f.write('DATA: {CROP_SIZE: "(64, 64)", BATCH_SIZE: 2}\n')
        f.write('MODEL: {ENCODER: {TYPE: "resnet18"}}\n')
        f.write("VAL: {IMAGE_BASE_SIZE: 64, CROP_SIZE: [64, 64], STRIDE_SIZE: [48, 48]}\n")
        f.write(extra)
    return cfg


SCENE_LINE = r"\[EVAL\] Scene (\S+) \((\d+)x(\d+)\): mIoU: (\d\.\d{4})  Acc: (\d\.\d{4})"


def test_val_cli_evaluates_the_scenes_and_prints_one_line_per_scene(tmp_path, capsys):
    from emrt_amd import val
    root = str(tmp_path / "s")
    write_scene_tree(root, [(64, 64), (96, 150)], sub=VAL_SUB)
    torch.manual_seed(0)
    miou = val.main(["--config", _tiny_yaml(tmp_path), "--data", "scenes", "--data_path", root])
    text = capsys.readouterr().out
    assert "[EVAL] data: 2 validation scenes resident on the GPU" in text
    assert text.count("[EVAL] Images: 2  mIoU:") == 1 and text.count("[EVAL] Class IoU:") == 1 and 0.0 <= miou <= 1.0
    assert [m[:3] for m in re.findall(SCENE_LINE, text)] == [("scene_0", "64", "64"), ("scene_1", "96", "150")], text[-2000:]


def test_train_cli_evaluates_natively_at_every_checkpoint(tmp_path, capsys):
    from emrt_amd import train
    root = str(tmp_path / "s")
    write_scene_tree(root, [(96, 80), (96, 80)])
    write_scene_tree(root, [(64, 64), (96, 150)], sub=VAL_SUB, seed=1)
    cfg = _tiny_yaml(tmp_path, "SAVE_FREQ_CHECKPOINT: 2\nLOGGING_INFO_FREQ: 1\n")
    out = str(tmp_path / "out")
    train.main(["--config", cfg, "--data", "scenes", "--data_path", root, "--eval_scenes", "native", "--iters", "4", "--save_dir", out, "--dtype", "fp32"])
    text = capsys.readouterr().out
    assert "[train] eval: 2 validation scenes resident on the GPU" in text
    assert text.count("In this val: mIoU") == 2 and text.count("Val_time_cost:") == 2, text[-3000:]
    assert [m[0] for m in re.findall(SCENE_LINE, text)] == ["scene_0", "scene_1"] * 2
    assert "[EVAL] Images: 2  mIoU:" in text and os.path.exists(os.path.join(out, "best_model.pdparams"))
    assert len(re.findall(r"\[TRAIN\].*?loss: ", text)) == 4
