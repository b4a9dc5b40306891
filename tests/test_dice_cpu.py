"""CPU: DiceCrossEntropyLoss -- its config keys, the factory, the entry points one step launches (on recording stand-ins for the first and the
fourth library), the fourth library's header, build and host-side refusals, and the float64 restatement (tests/dice_reference.py) against the
closed-form gradient the kernels evaluate.  The kernels themselves are held to that restatement in tests/test_gpu_dice.py."""
import argparse
import ctypes
import math
import os
import subprocess

import pytest
import torch

from tests import dice_reference as R
from tests import fake_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "emrt_amd", "configs", "EMRT", "EMRT_256x256_160k_potsdam_dice.yaml")
LX = ("emrt_lx_dice_ce_fwd", "emrt_lx_dice_ce_bwd", "emrt_lx_dice_ce_pair_fwd", "emrt_lx_dice_ce_pair_bwd")


def _config(loss="DiceCrossEntropyLoss", ncls=6, **train):
    from emrt_amd.config import CfgNode, get_config
    cfg = get_config()
    cfg.DATA.NUM_CLASSES = ncls
    cfg.TRAIN.LOSS = loss
    for k, v in train.items():
        cfg.TRAIN[k] = CfgNode(v) if isinstance(v, dict) else v
    return cfg


# ---- configuration and factory ------------------------------------------------------------------------------------------------------------------

def test_config_carries_the_dice_node_and_the_yaml_loads():
    from emrt_amd.config import get_config, update_config
    cfg = get_config()
    assert dict(cfg.TRAIN.DICE) == {"WEIGHT": 1.0, "CE_WEIGHT": 1.0, "SMOOTH": 1.0} and cfg.TRAIN.LOSS == "MixSoftmaxCrossEntropyLoss"
    cfg = update_config(get_config(), argparse.Namespace(cfg=YAML))
    base = update_config(get_config(), argparse.Namespace(cfg=os.path.join(os.path.dirname(YAML), "EMRT_256x256_160k_potsdam.yaml")))
    assert cfg.TRAIN.LOSS == "DiceCrossEntropyLoss" and dict(cfg.TRAIN.DICE) == {"WEIGHT": 1.0, "CE_WEIGHT": 1.0, "SMOOTH": 1.0}
    assert cfg.DATA == base.DATA and cfg.MODEL == base.MODEL                      # the base recipe with this loss
    assert {k: v for k, v in cfg.TRAIN.items() if k != "LOSS"} == {k: v for k, v in base.TRAIN.items() if k != "LOSS"}
    with pytest.raises(KeyError):
        get_config()._merge({"TRAIN": {"DICE": {"EPS": 1}}}, [])


def test_factory_builds_the_dice_loss():
    from emrt_amd.src.models import losses
    fn = losses.get_loss_function(_config(DICE={"WEIGHT": 0.5, "CE_WEIGHT": 2.0, "SMOOTH": 0.0}, CLASS_WEIGHTS=[1.0, 2.0, 0.5, 1.0, 3.0, 1.0]))
    assert type(fn) is losses.DiceCrossEntropyLoss
    assert (fn.ce_weight, fn.dice_weight, fn.smooth, fn.ignore_index, fn.aux, fn.aux_weight) == (2.0, 0.5, 0.0, 255, True, 0.4)
    assert fn.class_weights == [1.0, 2.0, 0.5, 1.0, 3.0, 1.0]
    plain = losses.get_loss_function(_config())
    assert (plain.ce_weight, plain.dice_weight, plain.smooth, plain.class_weights) == (1.0, 1.0, 1.0, None)
    assert "DiceCrossEntropyLoss" in losses.SUPPORTED_LOSSES
    for name in ("DiceLoss", "MultiCrossEntropyLoss", "CrossEntropyLoss"):
        with pytest.raises(NotImplementedError) as e:
            losses.get_loss_function(_config(name))
        assert "MixSoftmaxCrossEntropyLoss" in str(e.value) and "OhemCrossEntropyLoss" in str(e.value)


@pytest.mark.parametrize("node,match", [
    ({"WEIGHT": -1.0, "CE_WEIGHT": 1.0, "SMOOTH": 1.0}, "TRAIN.DICE.WEIGHT must be >= 0"),
    ({"WEIGHT": 1.0, "CE_WEIGHT": -0.5, "SMOOTH": 1.0}, "TRAIN.DICE.CE_WEIGHT must be >= 0"),
    ({"WEIGHT": 0.0, "CE_WEIGHT": 0.0, "SMOOTH": 1.0}, "both 0"),
    ({"WEIGHT": 1.0, "CE_WEIGHT": 1.0, "SMOOTH": -1e-3}, "TRAIN.DICE.SMOOTH must be >= 0"),
    ({"WEIGHT": math.nan, "CE_WEIGHT": 1.0, "SMOOTH": 1.0}, "TRAIN.DICE.WEIGHT is NaN"),
    ({"WEIGHT": 1.0, "CE_WEIGHT": math.nan, "SMOOTH": 1.0}, "TRAIN.DICE.CE_WEIGHT is NaN"),
    ({"WEIGHT": 1.0, "CE_WEIGHT": 1.0, "SMOOTH": math.nan}, "TRAIN.DICE.SMOOTH is NaN"),
])
def test_bad_dice_values_are_value_errors(node, match):
    from emrt_amd.src.models import losses
    with pytest.raises(ValueError, match=match):
        losses.get_loss_function(_config(DICE=node))
    with pytest.raises(ValueError, match=match):
        losses.DiceCrossEntropyLoss(ce_weight=node["CE_WEIGHT"], dice_weight=node["WEIGHT"], smooth=node["SMOOTH"])


def test_class_weight_count_is_checked():
    from emrt_amd.src.models import losses
    with pytest.raises(ValueError, match="The number of weights = 5 must be the same as the number of classes = 6"):
        losses.get_loss_function(_config(CLASS_WEIGHTS=[1.0] * 5))


# ---- launches through the recording ABIs --------------------------------------------------------------------------------------------------------

class FakeLossLib:
    """Recording stand-in for libemrt_hip_loss.so: checks argument count and kinds against include/emrt_hip_loss.h and logs.  Computes nothing."""

    def __init__(self):
        from emrt_amd import _lib
        self.protos = _lib.parse_header(_lib.LOSS_HEADER)
        self.calls = []

    def _check(self, name, args):
        spec = self.protos[name][1]
        assert len(args) == len(spec), "%s: %d args given, header declares %d" % (name, len(args), len(spec))
        for a, (t, an) in zip(args, spec):
            if t.endswith("*"):
                assert a is None or isinstance(a, (ctypes.c_void_p, int)), "%s.%s: bad pointer %r" % (name, an, a)
            elif t in ("float", "double"):
                assert isinstance(a, float), "%s.%s: expected a float, got %r" % (name, an, a)
            else:
                assert isinstance(a, int) and not isinstance(a, bool), "%s.%s (%s): expected int, got %r" % (name, an, t, a)

    def call(self, name, *args):
        self._check(name, args)
        self.calls.append((name, args))

    def query(self, name, *args):
        self._check(name, args)
        return 1 << 16


@pytest.fixture()
def fakes(monkeypatch):
    from emrt_amd import _lib
    main, lx = fake_abi.install(), FakeLossLib()
    monkeypatch.setattr(_lib, "_LOSS_LIB", lx)
    yield main, lx
    fake_abi.uninstall()


def _train_step(main, lx, loss_fn):
    """one ResNet-18 2 x 64 x 64 train step (forward, loss, backward) -> (entry points of the first library, calls of the fourth)"""
    from emrt_amd.src.models.emrt import EMRT
    from tests.test_host_logic_cpu import _place
    torch.manual_seed(0)
    m = _place(EMRT(num_classes=6, backbone="resnet18"))
    x, lab = torch.randn(2, 3, 64, 64), torch.randint(0, 6, (2, 64, 64))
    m.train()
    m.clear_gradients()
    main.calls.clear()
    lx.calls.clear()
    loss = loss_fn(m(x), lab)
    shapes = [tuple(p.shape) for p in loss.parts] + [tuple(loss.tensor.shape)]
    loss.backward()
    return [n for n, _ in main.calls], list(lx.calls), shapes


def test_dice_step_launches_the_pair_entry_points_once(fakes):
    from emrt_amd.src.models.losses import get_loss_function
    main, lx = fakes
    names, calls, shapes = _train_step(main, lx, get_loss_function(_config(DICE={"WEIGHT": 0.75, "CE_WEIGHT": 1.5, "SMOOTH": 2.0})))
    assert shapes == [(8,), (8,), (1,)]                                      # LossValue: parts are the per-head results
    assert [n for n, _ in calls] == ["emrt_lx_dice_ce_pair_fwd", "emrt_lx_dice_ce_pair_bwd"]
    assert not [n for n in names if n.startswith(("emrt_softmax_ce", "emrt_wce", "emrt_ohem"))]
    assert "emrt_scalar_axpby" not in names                                  # the finalize launch forms the weighted total
    fwd, bwd = calls[0][1], calls[1][1]
    assert fwd[3] is None and bwd[3] is None                                 # no class weights: NULL
    assert fwd[4:9] == (2, 6, 64, 64, 255) and bwd[13:18] == (2, 6, 64, 64, 255)
    assert fwd[9:14] == (1.0, pytest.approx(0.4), 1.5, 0.75, 2.0) and bwd[10:13] == (1.0, pytest.approx(0.4), 1.5)
    assert [p.value for p in fwd[14:18]] == [p.value for p in bwd[4:8]]      # the backward reads the results and coefficients of its forward
    assert bwd[8] is None and bwd[9] is None                                 # no upstream scalar: 1


def test_dice_step_with_class_weights_passes_one_device_vector(fakes):
    from emrt_amd.src.models.losses import get_loss_function
    main, lx = fakes
    fn = get_loss_function(_config(CLASS_WEIGHTS=[1.0, 2.0, 0.5, 1.0, 3.0, 1.0]))
    assert fn._cw is not None                                                # uploaded at construction: the context is placed
    names, calls, _ = _train_step(main, lx, fn)
    assert [n for n, _ in calls] == ["emrt_lx_dice_ce_pair_fwd", "emrt_lx_dice_ce_pair_bwd"]
    assert calls[0][1][3].value == calls[1][1][3].value == fn._cw.data_ptr()


def test_heads_of_different_sizes_and_missing_heads(fakes):
    """heads of different shapes take the single forms and are combined as the other losses combine them; MODEL.AUX.LOSS off: weight 1; a None
    head is skipped"""
    from emrt_amd.src.models.losses import DiceCrossEntropyLoss
    main, lx = fakes
    lab = torch.zeros(2, 8, 8, dtype=torch.int64)
    a, b = torch.zeros(2, 6, 8, 8), torch.zeros(2, 6, 8, 8)
    main.calls.clear()
    DiceCrossEntropyLoss()([a, torch.zeros(2, 6, 4, 4)], lab)
    assert [n for n, _ in lx.calls] == ["emrt_lx_dice_ce_fwd", "emrt_lx_dice_ce_fwd"]
    assert [n for n, _ in main.calls] == ["emrt_scalar_axpby"] and main.calls[0][1][4] == pytest.approx(0.4)
    lx.calls.clear()
    DiceCrossEntropyLoss(aux=False)([a, None, b], lab)
    assert [n for n, _ in lx.calls] == ["emrt_lx_dice_ce_pair_fwd"] and lx.calls[0][1][9:11] == (1.0, 1.0)
    lx.calls.clear()
    main.calls.clear()
    DiceCrossEntropyLoss(class_weights=[1.0] * 6)([a], lab)
    assert [n for n, _ in lx.calls] == ["emrt_lx_dice_ce_fwd"] and lx.calls[0][1][2] is not None
    assert [n for n, _ in main.calls] == ["emrt_scalar_axpby"]


def test_single_form_backward_carries_the_head_weight(fakes):
    from emrt_amd import functional as Fn
    from emrt_amd.runtime import Tape, ctx
    main, lx = fakes
    z, lab = torch.zeros(2, 6, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int64)
    tape = Tape()
    ctx().tape = tape
    try:
        res = Fn.dice_ce(z, lab, 255, 0.4, ce_weight=2.0, dice_weight=3.0, smooth=0.5)
    finally:
        ctx().tape = None
    tape.backward()
    (nf, fwd), (nb, bwd) = lx.calls
    assert (nf, nb) == ("emrt_lx_dice_ce_fwd", "emrt_lx_dice_ce_bwd")
    assert fwd[3:11] == (2, 6, 8, 8, 255, 2.0, 3.0, 0.5) and fwd[11].value == res.data_ptr()
    assert bwd[3].value == res.data_ptr() and bwd[4].value == fwd[12].value and bwd[5] is None
    assert bwd[6:13] == (pytest.approx(0.4), 2.0, 2, 6, 8, 8, 255)


@pytest.mark.parametrize("train", [{}, {"LOSS": "OhemCrossEntropyLoss", "OHEM": {"THRESH": 0.7, "MIN_KEPT": 1000}},
                                   {"CLASS_WEIGHTS": [1.0, 2.0, 0.5, 1.0, 3.0, 1.0]}], ids=["default", "ohem", "weighted"])
def test_the_other_recipes_never_load_the_fourth_library(fakes, monkeypatch, train):
    from emrt_amd import _lib
    from emrt_amd.src.models.losses import get_loss_function
    main, lx = fakes
    monkeypatch.setattr(_lib, "_LOSS_LIB", None)
    monkeypatch.setattr(_lib, "loss_lib", lambda: (_ for _ in ()).throw(AssertionError("a recipe without the Dice loss loaded the fourth library")))
    train = dict(train)
    names, calls, _ = _train_step(main, lx, get_loss_function(_config(train.pop("LOSS", "MixSoftmaxCrossEntropyLoss"), **train)))
    assert calls == [] and [n for n in names if "_ce_pair_fwd" in n or "wce_pair_fwd" in n]


# ---- the fourth library --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    from emrt_amd import build_ext
    build_ext.build(verbose=False)
    return build_ext


def test_fourth_library_exports_exactly_what_its_header_declares(built):
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.LOSS_HEADER)
    assert sorted(protos) == sorted(LX + ("emrt_lx_dice_ce_workspace_bytes", "emrt_lx_last_error", "emrt_lx_version"))
    out = subprocess.run(["nm", "-D", "--defined-only", built.library("loss").lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {n for n in exported if n.startswith("emrt_")} == set(protos)
    others = [_lib.parse_header(), _lib.parse_header(_lib.AUG_HEADER), _lib.parse_header(_lib.SMP_HEADER)]
    assert [len(o) for o in others] == [109, 6, 4]                           # the three pinned headers are untouched
    assert not set(protos) & set().union(*others)                            # nothing is declared twice
    assert [len(protos[n][1]) for n in LX] == [15, 15, 21, 21]
    assert _lib.LOSS_HEADER in built._headers() and os.path.join(built.CSRC, "loss_pixel.hpp") in built._headers()


def test_pixel_arithmetic_is_written_once():
    """pixel_stats / pixel_ce live in csrc/loss_pixel.hpp; both loss sources include it and neither restates it"""
    csrc = os.path.join(ROOT, "emrt_amd", "csrc")
    assert "PixelStats pixel_stats(" in open(os.path.join(csrc, "loss_pixel.hpp")).read()
    for f in ("loss.hip", os.path.join("loss_ext", "loss_ext.hip")):
        text = open(os.path.join(csrc, f)).read()
        assert "loss_pixel.hpp\"" in text and "PixelStats pixel_stats(" not in text and "float pixel_ce(" not in text, f
        assert "atomicAdd(" not in text or f == "loss.hip"                   # (loss.hip: the OHEM histograms' integer atomics)


def test_loader_of_the_fourth_library(built, monkeypatch, tmp_path):
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_LOSS_LIB", None)
    X = _lib.loss_lib()
    assert X.query("emrt_lx_version") == 1 and X is _lib.loss_lib() and sorted(X.protos) == sorted(_lib.parse_header(_lib.LOSS_HEADER))
    monkeypatch.setitem(_lib.SIDE_LIBRARIES, "loss", _lib.SIDE_LIBRARIES["loss"]._replace(path=str(tmp_path / "nope.so")))
    monkeypatch.setattr(_lib, "_LOSS_LIB", None)
    with pytest.raises(_lib.EmrtHipError, match="not found"):
        _lib.loss_lib()


def test_entry_points_refuse_bad_arguments_before_any_launch(built, monkeypatch):
    """Against the real library, no GPU: every bad call returns non-zero with a message before anything touches a device (the pointers are a
    made-up address and never dereferenced; a case that passed its checks would launch on them)."""
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_LOSS_LIB", None)
    X = _lib.loss_lib()
    p, nan = ctypes.c_void_p(0x10000), math.nan

    def fwd(match, logits=p, labels=p, N=2, C=6, H=8, W=8, cw=1.0, dw=1.0, s=1.0, res=p, coef=p, ws=p):
        with pytest.raises(_lib.EmrtHipError, match=match):
            X.call("emrt_lx_dice_ce_fwd", logits, labels, None, N, C, H, W, 255, cw, dw, s, res, coef, ws, None)

    def bwd(match, res=p, coef=p, C=6, H=8, cw=1.0, out=p):
        with pytest.raises(_lib.EmrtHipError, match=match):
            X.call("emrt_lx_dice_ce_bwd", p, p, None, res, coef, None, 1.0, cw, 2, C, H, 8, 255, out, None)

    def pair_fwd(match, lb=p, N=2, C=6, cw=1.0, dw=1.0, s=1.0, coef_b=p, total=p, ws=p):
        with pytest.raises(_lib.EmrtHipError, match=match):
            X.call("emrt_lx_dice_ce_pair_fwd", p, lb, p, None, N, C, 8, 8, 255, 1.0, 0.4, cw, dw, s, p, p, p, coef_b, total, ws, None)

    def pair_bwd(match, res_b=p, C=6, cw=1.0, db=p):
        with pytest.raises(_lib.EmrtHipError, match=match):
            X.call("emrt_lx_dice_ce_pair_bwd", p, p, p, None, p, res_b, p, p, None, None, 1.0, 0.4, cw, 2, C, 8, 8, 255, p, db, None)

    fwd("emrt_lx_dice_ce_fwd: null pointer", logits=None)
    fwd("null pointer", labels=None)
    fwd("null pointer", res=None)
    fwd("null pointer", coef=None)
    fwd("null pointer", ws=None)
    fwd("C must be 1..64", C=0)
    fwd("C must be 1..64 \\(EMRT_LX_MAX_CLASSES\\)", C=65)
    fwd("N \\* H \\* W < 2\\^31", N=1 << 11, H=1 << 10, W=1 << 10)
    fwd("N, C, H, W >= 1", H=0)
    fwd("ce_weight and dice_weight must be >= 0", cw=-1.0)
    fwd("ce_weight and dice_weight must be >= 0", dw=-0.5)
    fwd("ce_weight and dice_weight must be >= 0 and not NaN", cw=nan)
    fwd("ce_weight and dice_weight must be >= 0 and not NaN", dw=nan)
    fwd("both 0", cw=0.0, dw=0.0)
    fwd("smooth must be >= 0", s=-1.0)
    fwd("smooth must be >= 0 and not NaN", s=nan)
    bwd("emrt_lx_dice_ce_bwd: null pointer", res=None)
    bwd("null pointer", coef=None)
    bwd("null pointer", out=None)
    bwd("C must be 1..64", C=65)
    bwd("N, C, H, W >= 1", H=0)
    bwd("ce_weight must be >= 0", cw=-1.0)
    bwd("ce_weight must be >= 0 and not NaN", cw=nan)
    pair_fwd("emrt_lx_dice_ce_pair_fwd: null pointer", lb=None)
    pair_fwd("null pointer", coef_b=None)
    pair_fwd("null pointer", total=None)
    pair_fwd("C must be 1..64", C=0)
    pair_fwd("C must be 1..64", C=100)
    pair_fwd("2\\^31", N=1 << 30)
    pair_fwd("must be >= 0", dw=-1.0)
    pair_fwd("both 0", cw=0.0, dw=0.0)
    pair_fwd("smooth must be >= 0", s=nan)
    pair_bwd("emrt_lx_dice_ce_pair_bwd: null pointer", res_b=None)
    pair_bwd("null pointer", db=None)
    pair_bwd("C must be 1..64", C=65)
    pair_bwd("ce_weight must be >= 0", cw=nan)
    # per head 1024 blocks of {3 CE sums, then I, P, T for every chunk of eight classes} floats; refused arguments: 0
    q = lambda C, heads: X.query("emrt_lx_dice_ce_workspace_bytes", C, heads)
    assert q(6, 1) == q(8, 1) == 1024 * (3 + 24) * 4 and q(9, 1) == 1024 * (3 + 48) * 4 and q(64, 2) == 2 * 1024 * (3 + 8 * 24) * 4
    assert q(0, 1) == q(65, 1) == q(6, 0) == q(6, 3) == 0


# ---- the reference itself --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smooth", [1.0, 0.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_float64_restatement_agrees_with_the_closed_form_gradient(smooth, weighted):
    """1 x 2 x 5 x 3: autograd through the float64 loss against the formula the backward kernel evaluates, in float64 and in float32"""
    logits, labels = R.make_case((1, 2, 5, 3), 7, ignored=0.3, all_present=True)
    assert (labels == R.IGN).any()
    kw = dict(ce_weight=0.7, dice_weight=1.3, smooth=smooth, class_weight=torch.tensor([0.5, 2.0]) if weighted else None)
    terms, grad = R.dice_ce_autograd(logits, labels, **kw)
    assert 0.0 < terms["Dice"].item() < 1.0 and terms["CE"].item() > 0 and terms["T"].sum().item() == terms["num_valid"].item()
    assert terms["L"].item() == pytest.approx(0.7 * terms["CE"].item() + 1.3 * terms["Dice"].item(), rel=1e-14)
    closed = R.dice_ce_closed_form_grad(logits, labels, **kw)
    assert (closed - grad).abs().max().item() < 1e-14
    assert not grad[(labels == R.IGN).unsqueeze(1).expand_as(grad)].any()
    closed32 = R.dice_ce_closed_form_grad(logits, labels, dtype=torch.float32, **kw)
    assert closed32.dtype == torch.float32 and (closed32.double() - grad).abs().max().item() < 1e-6


def test_float64_restatement_edge_cases():
    logits, labels = R.make_case((2, 6, 16, 20), 8, absent=3)
    t, g = R.dice_ce_autograd(logits, labels, smooth=1.0)
    assert t["T"][3].item() == 0 and t["I"][3].item() == 0 and t["P"][3].item() > 0          # an absent class contributes s / (P_c + s)
    assert t["Dice"].item() == pytest.approx(1 - sum(((2 * t["I"][c] + 1) / (t["P"][c] + t["T"][c] + 1)).item() for c in range(6)) / 6, rel=1e-14)
    for s in (1.0, 0.0):                       # every pixel ignored: L = 0 and no gradient
        t, g = R.dice_ce_autograd(logits, torch.full_like(labels, R.IGN), smooth=s)
        assert t["L"].item() == 0.0 and not g.any()
