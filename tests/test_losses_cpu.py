"""CPU: the loss factory (MixSoftmaxCrossEntropyLoss with optional class weights, OhemCrossEntropyLoss), its config keys and the entry points
each configuration launches, on the recording stand-in for the C-ABI (tests/fake_abi.py).  Nothing is computed here; the kernels are held
to a float64 restatement of the reference in tests/test_gpu_ohem.py."""
import argparse
import os

import pytest
import torch

from tests import fake_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("emrt_ohem_ce_fwd", "emrt_ohem_ce_bwd", "emrt_ohem_ce_pair_fwd", "emrt_ohem_ce_pair_bwd", "emrt_wce_fwd", "emrt_wce_bwd", "emrt_wce_pair_fwd", "emrt_wce_pair_bwd")


@pytest.fixture()
def fake():
    f = fake_abi.install()
    yield f
    fake_abi.uninstall()


def _config(loss="MixSoftmaxCrossEntropyLoss", ncls=6, **train):
    from emrt_amd.config import CfgNode, get_config
    cfg = get_config()
    cfg.DATA.NUM_CLASSES = ncls
    cfg.TRAIN.LOSS = loss
    for k, v in train.items():
        cfg.TRAIN[k] = CfgNode(v) if isinstance(v, dict) else v
    return cfg


def test_new_config_keys_and_the_ohem_yaml():
    from emrt_amd.config import get_config, update_config
    cfg = get_config()
    assert cfg.TRAIN.OHEM.THRESH == 0.7 and cfg.TRAIN.OHEM.MIN_KEPT == 10000 and cfg.TRAIN.CLASS_WEIGHTS == []
    assert cfg.TRAIN.LOSS == "MixSoftmaxCrossEntropyLoss"
    path = os.path.join(ROOT, "emrt_amd", "configs", "EMRT", "EMRT_256x256_160k_potsdam_ohem.yaml")
    cfg = update_config(get_config(), argparse.Namespace(cfg=path))
    assert cfg.TRAIN.LOSS == "OhemCrossEntropyLoss" and cfg.TRAIN.OHEM.THRESH == 0.7
    assert cfg.TRAIN.OHEM.MIN_KEPT == cfg.DATA.BATCH_SIZE * 256 * 256 // 8 == 65536       # the fraction the yaml states
    assert cfg.TRAIN.CLASS_WEIGHTS == [] and cfg.DATA.NUM_CLASSES == 6 and cfg.MODEL.AUX.AUX_WEIGHT == 0.4
    # a key the defaults do not carry is still an error
    with pytest.raises(KeyError):
        get_config()._merge({"TRAIN": {"OHEM": {"KEEP": 1}}}, [])


def test_factory_returns_each_supported_loss_and_refuses_the_rest():
    from emrt_amd.src.models import losses
    mix = losses.get_loss_function(_config())
    assert isinstance(mix, losses.MixSoftmaxCrossEntropyLoss) and mix.class_weights is None
    ohem = losses.get_loss_function(_config("OhemCrossEntropyLoss", OHEM={"THRESH": 0.6, "MIN_KEPT": 123}))
    assert isinstance(ohem, losses.OhemCrossEntropyLoss)
    assert (ohem.thresh, ohem.min_kept, ohem.ignore_index, ohem.aux, ohem.aux_weight) == (0.6, 123, 255, True, 0.4)
    for name in ("MultiCrossEntropyLoss", "CrossEntropyLoss", "DiceLoss"):
        with pytest.raises(NotImplementedError) as e:
            losses.get_loss_function(_config(name))
        assert "MixSoftmaxCrossEntropyLoss" in str(e.value) and "OhemCrossEntropyLoss" in str(e.value)


def test_class_weights_are_checked():
    from emrt_amd.src.models import losses
    w = losses.get_loss_function(_config(CLASS_WEIGHTS=[1.0, 2.0, 0.5, 1.0, 3.0, 1.0]))
    assert w.class_weights == [1.0, 2.0, 0.5, 1.0, 3.0, 1.0]
    with pytest.raises(ValueError, match="The number of weights = 5 must be the same as the number of classes = 6"):
        losses.get_loss_function(_config(CLASS_WEIGHTS=[1.0] * 5))
    with pytest.raises(ValueError, match="OhemCrossEntropyLoss"):
        losses.get_loss_function(_config("OhemCrossEntropyLoss", CLASS_WEIGHTS=[1.0] * 6))
    with pytest.raises(ValueError, match="MIN_KEPT"):
        losses.get_loss_function(_config("OhemCrossEntropyLoss", OHEM={"THRESH": 0.7, "MIN_KEPT": -1}))


def test_class_weight_length_is_checked_against_the_logits_too(fake):
    """the constructor form (no config) learns the class count from the logits"""
    from emrt_amd.src.models.losses import MixSoftmaxCrossEntropyLoss
    preds = [torch.zeros(2, 6, 8, 8), torch.zeros(2, 6, 8, 8)]
    with pytest.raises(ValueError, match="The number of weights = 4 must be the same as the number of classes = 6"):
        MixSoftmaxCrossEntropyLoss(class_weights=[1.0] * 4)(preds, torch.zeros(2, 8, 8, dtype=torch.int64))


def _train_step_calls(fake, loss_fn):
    """entry points of one ResNet-18 2 x 64 x 64 train step (forward, loss, backward), in launch order"""
    from emrt_amd.src.models.emrt import EMRT
    from tests.test_host_logic_cpu import _place
    torch.manual_seed(0)
    m = _place(EMRT(num_classes=6, backbone="resnet18"))
    x, lab = torch.randn(2, 3, 64, 64), torch.randint(0, 6, (2, 64, 64))
    m.train()
    m.clear_gradients()
    fake.calls.clear()
    out = m(x)
    n_fwd = len(fake.calls)
    loss = loss_fn(out, lab)
    n_loss = len(fake.calls)
    loss.backward()
    names = [n for n, _ in fake.calls]
    return names, names[n_fwd:n_loss], fake.calls


def test_default_recipe_launches_what_it_launched(fake):
    from emrt_amd.src.models.losses import get_loss_function
    names, loss_names, _ = _train_step_calls(fake, get_loss_function(_config()))
    assert loss_names == ["emrt_softmax_ce_pair_fwd"]
    assert names.count("emrt_softmax_ce_pair_fwd") == names.count("emrt_softmax_ce_pair_bwd") == 1
    assert not [n for n in names if n in NEW_ENTRY_POINTS]


def test_ohem_step_launches_the_ohem_entry_points_only(fake):
    from emrt_amd.src.models.losses import get_loss_function
    names, loss_names, calls = _train_step_calls(fake, get_loss_function(_config("OhemCrossEntropyLoss", OHEM={"THRESH": 0.7, "MIN_KEPT": 1000})))
    assert loss_names == ["emrt_ohem_ce_pair_fwd"]          # main + aux head at the input size: the launches of one head
    assert names.count("emrt_ohem_ce_pair_bwd") == 1
    assert not [n for n in names if n.startswith("emrt_softmax_ce") or n.startswith("emrt_wce") or n in ("emrt_ohem_ce_fwd", "emrt_ohem_ce_bwd")]
    fwd = [a for n, a in calls if n == "emrt_ohem_ce_pair_fwd"][0]
    bwd = [a for n, a in calls if n == "emrt_ohem_ce_pair_bwd"][0]
    assert fwd[3:10] == (2, 6, 64, 64, 255, 0.7, 1000)
    # the auxiliary head's weight reaches the total and the backward; the backward reads the p arrays and the results of its forward
    assert fwd[10:12] == (1.0, pytest.approx(0.4)) and bwd[9:11] == (1.0, pytest.approx(0.4))
    assert [p.value for p in fwd[12:16]] == [p.value for p in bwd[3:7]]


def test_weighted_mix_step_stays_one_forward_and_one_backward_launch(fake):
    from emrt_amd.src.models.losses import get_loss_function
    names, loss_names, calls = _train_step_calls(fake, get_loss_function(_config(CLASS_WEIGHTS=[1.0, 2.0, 0.5, 1.0, 3.0, 1.0])))
    assert loss_names == ["emrt_wce_pair_fwd"] and names.count("emrt_wce_pair_bwd") == 1
    assert not [n for n in names if n.startswith("emrt_softmax_ce") or n.startswith("emrt_ohem")]
    fwd = [a for n, a in calls if n == "emrt_wce_pair_fwd"][0]
    bwd = [a for n, a in calls if n == "emrt_wce_pair_bwd"][0]
    assert fwd[3].value == bwd[3].value and fwd[3].value        # the same device class-weight vector, not NULL
    assert fwd[9:11] == (1.0, pytest.approx(0.4))


def test_heads_of_different_sizes_and_missing_heads(fake):
    """MODEL.AUX.LOSS off: weight 1; a None head is skipped; heads of different sizes take the single-head entry points"""
    from emrt_amd.src.models.losses import MixSoftmaxCrossEntropyLoss, OhemCrossEntropyLoss
    lab = torch.zeros(2, 8, 8, dtype=torch.int64)
    a, b = torch.zeros(2, 6, 8, 8), torch.zeros(2, 6, 8, 8)
    OhemCrossEntropyLoss(min_kept=5, aux=False)([a, None, b], lab)
    assert [n for n, _ in fake.calls] == ["emrt_ohem_ce_pair_fwd"] and fake.calls[0][1][10:12] == (1.0, 1.0)
    fake.calls.clear()
    OhemCrossEntropyLoss(min_kept=5)([a, torch.zeros(2, 6, 4, 4)], lab)
    assert [n for n, _ in fake.calls] == ["emrt_ohem_ce_fwd", "emrt_ohem_ce_fwd", "emrt_scalar_axpby"]
    assert [x for n, x in fake.calls if n == "emrt_scalar_axpby"][0][4] == pytest.approx(0.4)
    fake.calls.clear()
    OhemCrossEntropyLoss(min_kept=5)([a], lab)
    assert [n for n, _ in fake.calls] == ["emrt_ohem_ce_fwd", "emrt_scalar_axpby"]
    fake.calls.clear()
    MixSoftmaxCrossEntropyLoss(class_weights=[1.0] * 6)([a], lab)
    assert [n for n, _ in fake.calls] == ["emrt_wce_fwd", "emrt_scalar_axpby"]


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    """the argument checks run on the host before anything touches a device (no GPU here; the pointers are never dereferenced)"""
    import ctypes
    from emrt_amd import _lib, build_ext
    build_ext.build(verbose=False)
    _lib._LIB = None
    L = _lib.lib()
    p = ctypes.c_void_p(0x10000)

    def refused(name, *args, match):
        with pytest.raises(_lib.EmrtHipError, match=match):
            L.call(name, *args)

    assert L.query("emrt_abi_version") == 9
    assert L.query("emrt_ohem_workspace_bytes", 0, 1) == 0 and L.query("emrt_ohem_workspace_bytes", 64, 0) == 0 and L.query("emrt_ohem_workspace_bytes", 64, 3) == 0
    # per head: three histograms of 2048 bins + 16 state words, 1024 partial pairs, one CE value per pixel
    one = (3 * 2048 + 16) * 4 + 1024 * 2 * 4 + 8 * 256 * 256 * 4
    assert L.query("emrt_ohem_workspace_bytes", 8 * 256 * 256, 1) == one and L.query("emrt_ohem_workspace_bytes", 8 * 256 * 256, 2) == 2 * one
    refused("emrt_ohem_ce_fwd", p, p, 2, 0, 8, 8, 255, 0.7, 10, p, p, p, None, match="C, H, W >= 1")
    refused("emrt_ohem_ce_fwd", p, p, 2, 6, 8, 8, 255, 0.7, -1, p, p, p, None, match="min_kept >= 0")
    refused("emrt_ohem_ce_fwd", p, p, 2, 6, 8, 8, 255, 0.7, 10, None, p, p, None, match="null pointer")
    refused("emrt_ohem_ce_fwd", p, p, 2, 6, 8, 8, 255, 0.7, 10, p, p, None, None, match="null pointer")
    refused("emrt_ohem_ce_fwd", p, p, 1 << 11, 6, 1 << 10, 1 << 10, 255, 0.7, 10, p, p, p, None, match="2\\^31")
    refused("emrt_ohem_ce_bwd", p, p, None, p, None, 1.0, 2, 6, 8, 8, 255, p, None, match="null pointer")
    refused("emrt_ohem_ce_bwd", p, p, p, p, None, 1.0, 2, 0, 8, 8, 255, p, None, match="C, H, W >= 1")
    refused("emrt_ohem_ce_pair_fwd", p, p, p, 2, 6, 8, 8, 255, 0.7, -5, 1.0, 0.4, p, p, p, p, p, p, None, match="min_kept >= 0")
    refused("emrt_ohem_ce_pair_fwd", p, p, p, 2, 6, 8, 8, 255, 0.7, 5, 1.0, 0.4, p, None, p, p, p, p, None, match="null pointer")
    refused("emrt_ohem_ce_pair_fwd", p, p, p, 2, 6, 0, 8, 255, 0.7, 5, 1.0, 0.4, p, p, p, p, p, p, None, match="C, H, W >= 1")
    refused("emrt_ohem_ce_pair_bwd", p, p, p, p, p, p, None, None, None, 1.0, 0.4, 2, 6, 8, 8, 255, p, p, None, match="null pointer")
    refused("emrt_wce_fwd", p, p, None, 2, 0, 8, 8, 255, p, p, None, match="C, H, W >= 1")
    refused("emrt_wce_fwd", p, None, p, 2, 6, 8, 8, 255, p, p, None, match="null pointer")
    refused("emrt_wce_bwd", p, p, p, p, None, 1.0, 2, 6, 0, 8, 255, p, None, match="C, H, W >= 1")
    refused("emrt_wce_pair_fwd", p, None, p, p, 2, 6, 8, 8, 255, 1.0, 0.4, p, p, p, p, None, match="null pointer")
    refused("emrt_wce_pair_bwd", p, p, p, p, p, None, None, 1.0, 0.4, 2, 0, 8, 8, 255, p, p, None, match="C, H, W >= 1")
    _lib._LIB = None
