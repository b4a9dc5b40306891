"""CPU: the resnext50 backbone (ResNeXt-50 64x4d, backbones/resnext.py:153-279) -- the model built from a yaml, its Paddle
structured state-dict names and parameter counts, a backbone-only .pdparams load, the grouped convolution's host wiring on the
recording stand-in for the C-ABI (tests/fake_abi.py), and the early gradient exchange's name-based segments."""
import argparse
import ctypes
import os

import pytest
import torch

from tests import fake_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam.yaml")


def _config(backbone):
    from emrt_amd.config import get_config, update_config
    cfg = update_config(get_config(), argparse.Namespace(cfg=YAML))
    cfg.MODEL.ENCODER.TYPE = backbone
    return cfg


def _expected_shapes():
    """The reference's ResNeXt(layers=50, cardinality=64) parameters, written out from its structure (resnext.py:92-150,153-250)."""
    shapes = {}

    def cbl(name, cin, cout, k, groups=1):
        shapes["backbone.%s._conv.weight" % name] = (cout, cin // groups, k, k)
        for p in ("weight", "bias"):
            shapes["backbone.%s._batch_norm.%s" % (name, p)] = (cout,)

    cbl("conv", 3, 64, 7)
    cin = 64
    for s, (depth, w) in enumerate(zip([3, 4, 6, 3], [256, 512, 1024, 2048])):
        for i in range(depth):
            cbl("bb_%d_%d.conv0" % (s, i), cin, w, 1)
            cbl("bb_%d_%d.conv1" % (s, i), w, w, 3, groups=64)
            cbl("bb_%d_%d.conv2" % (s, i), w, w, 1)
            if i == 0:
                cbl("bb_%d_%d.short" % (s, i), cin, w, 1)
            cin = w
    return shapes


def test_resnext50_from_yaml_has_paddle_names_and_counts():
    from emrt_amd.src.models import get_model
    torch.manual_seed(0)
    model = get_model(_config("resnext50"))
    sd = model.state_dict()
    got = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("backbone.") and not k.endswith(("_mean", "_variance"))}
    want = _expected_shapes()
    want["backbone.out.weight"], want["backbone.out.bias"] = (1000, 2048), (1000,)       # [out, in] here ([in, out] in Paddle: checkpoint.py)
    assert got == want
    assert sd["backbone.bb_0_0.conv1._conv.weight"].shape == (256, 4, 3, 3) and sd["backbone.bb_3_2.conv1._conv.weight"].shape == (2048, 32, 3, 3)
    assert "backbone.bb_1_0.conv1._batch_norm._mean" in sd and "backbone.bb_1_0.conv1._batch_norm._variance" in sd
    n_backbone = sum(v.numel() for k, v in model.named_parameters() if k.startswith("backbone.") and not k.startswith("backbone.out."))
    n_out = sum(v.numel() for k, v in model.named_parameters() if k.startswith("backbone.out."))
    assert (n_backbone, n_out) == (43143488, 2049000)
    assert model.backbone_num_channels == [512, 1024, 2048] and model.auxlayer.convs[0][0].cin == 1024
    # the offline initialisation: Paddle's default conv init (std sqrt(2 / fan_in), fan_in = Cg * 9 for the grouped layers)
    w = sd["backbone.bb_3_0.conv1._conv.weight"]
    assert abs(w.std().item() - (2.0 / (32 * 9)) ** 0.5) < 0.01 * (2.0 / (32 * 9)) ** 0.5 * 10
    # early-exchange segments by this backbone's own names; the module constants stay those of the ResNet
    from emrt_amd.src.models.emrt import LATE_GRAD_PREFIXES
    assert model.late_grad_prefixes != LATE_GRAD_PREFIXES and all(p.startswith("backbone.") for p in model.late_grad_prefixes)
    names = [k for k, _ in model.named_parameters()]
    late = [k for k in names if k.startswith(model.late_grad_prefixes)]
    assert any(k.startswith("backbone.bb_2_") for k in late) and not any(k.startswith("backbone.bb_3_") for k in late)
    assert any(k.startswith("backbone.conv.") for k in late)


@pytest.mark.parametrize("backbone", ["resnest50", "segformer_b4", "resnext101"])
def test_other_backbones_still_refused(backbone):
    from emrt_amd.src.models import get_model
    with pytest.raises(NotImplementedError, match="resnext50"):
        get_model(_config(backbone))


def test_backbone_only_pdparams_loads_under_prefix(tmp_path):
    from emrt_amd.src.models.emrt import EMRT
    from emrt_amd.src.utils.checkpoint import load_pretrained_model, save_pdparams, load_pdparams
    torch.manual_seed(0)
    src = EMRT(num_classes=6, backbone="resnext50")
    bb = {k[len("backbone."):]: v.clone() for k, v in src.state_dict().items() if k.startswith("backbone.")}
    path = str(tmp_path / "resnext50_64x4d.pdparams")
    save_pdparams(bb, path)
    disk = load_pdparams(path)
    assert disk["out.weight"].shape == (2048, 1000)                # Paddle's Linear layout on disk
    assert disk["bb_0_0.conv1._conv.weight"].shape == (256, 4, 3, 3)
    torch.manual_seed(1)
    dst = EMRT(num_classes=6, backbone="resnext50")
    n = load_pretrained_model(dst, path, prefix="backbone.")
    assert n == len(bb)
    for k, v in bb.items():
        assert torch.equal(dst.state_dict()["backbone." + k], v), k


@pytest.fixture()
def fake():
    f = fake_abi.install()
    yield f
    fake_abi.uninstall()


def _place(model):
    from emrt_amd import nn as hnn
    from emrt_amd.runtime import ctx, F32
    from emrt_amd.src.models.emrt import NOGRAD_PARAMS
    model.store = hnn.ParamStore(model, ctx().device, F32, nograd_names=NOGRAD_PARAMS, fused_groups=model.fused_groups(),
                                 lr_mult_names=model.lr_mult_names())
    hnn.bind_all(model, model.store)
    model.store.pack()
    return model


def test_resnext_train_step_launches_grouped_kernels(fake):
    from emrt_amd.src.models.emrt import EMRT
    from emrt_amd.src.models.losses import MixSoftmaxCrossEntropyLoss
    torch.manual_seed(0)
    m = _place(EMRT(num_classes=6, backbone="resnext50"))
    st = m.store
    a, cnt = st.views["backbone.out.weight"]
    assert a >= st.n_train                       # no gradient for the unused classifier
    x, lab = torch.randn(2, 3, 64, 64), torch.randint(0, 6, (2, 64, 64))
    m.train()
    m.clear_gradients()
    out = m(x)
    fwd = [args for name, args in fake.calls if name == "emrt_gconv2d"]
    assert len(fwd) == 16
    # (N, H, W, C, ..., stride, groups) of the first grouped layer and of stage 4's strided one; statistics in the epilogue
    assert fwd[0][4:8] == (2, 16, 16, 256) and fwd[0][15:17] == (1, 64) and fwd[0][18] is not None
    s4 = fwd[13]
    assert s4[4:8] == (2, 4, 4, 2048) and s4[10:13] == (2, 2, 2048) and s4[15] == 2
    loss = MixSoftmaxCrossEntropyLoss()(out, lab)
    fake.calls.clear()
    loss.backward()
    bwd = [args for name, args in fake.calls if name == "emrt_gconv2d_bwd"]
    assert len(bwd) == 16
    g0 = st.offsets["backbone.bb_0_0.conv1._conv.weight"]
    dws = {b[7].value for b in bwd}
    assert st.grad.data_ptr() + 4 * g0 in dws
    assert all(b[3] is not None for b in bwd)          # every grouped layer hands a data gradient back


def test_resnext_backward_split_keeps_early_gradient_ranges_final(fake):
    """test_host_logic_cpu.py::test_backward_split_keeps_early_gradient_ranges_final for resnext50, with the model's own prefixes: no launch
    before the split writes a late range, none after it an early one; the finer segmentation the same."""
    from emrt_amd.runtime import ctx
    from emrt_amd.src.models.emrt import EMRT
    from emrt_amd.src.models.losses import MixSoftmaxCrossEntropyLoss
    torch.manual_seed(0)
    m = _place(EMRT(num_classes=6, backbone="resnext50"))
    st = m.store
    early, late = st.split_ranges(m.late_grad_prefixes)
    cover = sorted(early + late)
    assert cover[0][0] == 0 and cover[-1][1] == st.n_train and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    assert 0.05 < sum(e - a for a, e in late) / st.n_train < 0.5
    base = st.grad.data_ptr()

    def grad_offsets(calls):
        out = []
        for name, args in calls:
            for a in args:
                v = a.value if isinstance(a, ctypes.c_void_p) else None
                if v is not None and base <= v < base + 4 * st.n_total:
                    out.append((name, (v - base) // 4))
        return out

    def inside(off, ranges):
        return any(a <= off < e for a, e in ranges)

    x, lab = torch.randn(2, 3, 64, 64), torch.randint(0, 6, (2, 64, 64))
    m.train()

    def forward():
        m.clear_gradients()
        old, ctx().side_branch = ctx().side_branch, False
        try:
            return MixSoftmaxCrossEntropyLoss()(m(x), lab)
        finally:
            ctx().side_branch = old

    loss = forward()
    fake.calls.clear()
    rest = loss.backward_until_split()
    first = grad_offsets(fake.calls)
    fake.calls.clear()
    rest()
    second = grad_offsets(fake.calls)
    assert len(first) > 50 and len(second) > 20
    assert any(n == "emrt_gconv2d_bwd" for n, _ in first) and any(n == "emrt_gconv2d_bwd" for n, _ in second)
    assert all(inside(off, early) for _, off in first), [x for x in first if not inside(x[1], early)][:5]
    assert all(inside(off, late) for _, off in second), [x for x in second if not inside(x[1], late)][:5]

    seg_ranges = st.segment_ranges(m.grad_segment_prefixes)
    assert seg_ranges[0] == early
    loss = forward()
    fake.calls.clear()
    segs = loss.backward_until_split(segments=True)
    touched = [grad_offsets(fake.calls)]
    for seg in segs:
        fake.calls.clear()
        seg()
        touched.append(grad_offsets(fake.calls))
    assert len(touched) == len(seg_ranges) == 3 and all(len(t) > 5 for t in touched)
    for i, (t, ranges) in enumerate(zip(touched, seg_ranges)):
        assert all(inside(off, ranges) for _, off in t), (i, [x for x in t if not inside(x[1], ranges)][:5])
