"""-m gpu: the resnext50 backbone (backbones/resnext.py, ResNeXt50_64x4d; paddle_EMRT.py:235-236) -- the grouped 3x3 convolution kernels
(emrt_gconv2d / emrt_gconv2d_bwd) against float64 torch, and the whole model against a float64 restatement of ResNeXt-50 64x4d swapped into the
oracle EMRT."""
import ctypes
import math

import pytest
import torch
import torch.nn as tnn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                # noqa: E402
from emrt_amd.runtime import ctx, F32, BF16, F16        # noqa: E402
from tests.hip_utils import init, close_gemm            # noqa: E402

_TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _padded(t_nhwc, ld, dtype, bs=None, fill=0.0):
    """device NHWC map whose pixel stride is ld >= C (a channel slice of a wider buffer) and whose batch stride is bs >= H * W * ld (padding
    behind every image); everything the view does not address holds `fill`"""
    N, H, W, C = t_nhwc.shape
    bs = bs or H * W * ld
    buf = torch.full((N * bs,), fill, dtype=_TD[dtype], device="cuda")
    view = buf.as_strided((N, H, W, C), (bs, W * ld, ld, 1))
    view.copy_(t_nhwc.to(device="cuda", dtype=_TD[dtype]))
    return view


def _whole(view):
    """the flat buffer behind a _padded view"""
    return view.as_strided((view.shape[0] * view.stride(0),), (1,), 0)


def _run_fwd(x, w, groups, stride, dtype, relu=False, bias=None, scale=None, stats=None, ld_in=None, ld_out=None, bs_in=None, bs_out=None, fill=0.0,
             xd=None, wd=None):
    """x, w on the host (or xd, wd as a former call returned them); the output starts as `fill` everywhere"""
    N, H, W, C = x.shape
    OC = w.shape[0]
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if xd is None:
        xd = _padded(x, ld_in or C, dtype, bs_in, fill)
    if wd is None:
        wd = w.permute(0, 2, 3, 1).contiguous().to(device="cuda", dtype=_TD[dtype])       # [OC][3][3][Cg]
    y = _padded(torch.full((N, OH, OW, OC), fill), ld_out or OC, dtype, bs_out, fill)
    L = _lib.lib()
    L.call("emrt_gconv2d", _P(xd), _P(wd), _P(y), _P(bias), N, H, W, C, xd.stride(2), xd.stride(0), OH, OW, OC, y.stride(2), y.stride(0), stride, groups,
           int(relu), _P(stats), _P(scale), dtype, ctx().stream)
    return y, xd, wd


def _run_bwd(xd, wd, dy, groups, stride, dtype, dx=None, accumulate=False, dw=None, dbias=None):
    N, H, W, C = xd.shape
    _, OH, OW, OC = dy.shape
    L = _lib.lib()
    L.call("emrt_gconv2d_bwd", _P(xd), _P(dy), _P(wd), _P(dx), dx.stride(2) if dx is not None else 0, dx.stride(0) if dx is not None else 0, int(accumulate),
           _P(dw), _P(dbias), N, H, W, C, xd.stride(2), xd.stride(0), OH, OW, OC, dy.stride(2), dy.stride(0), stride, groups, dtype, ctx().stream)


def _ref(x, w, groups, stride, dy=None):
    """float64 CPU: y and (with dy) dx, dw through autograd; NHWC in / out"""
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride=stride, padding=1, groups=groups)
    if dy is None:
        return y.detach().permute(0, 2, 3, 1), None, None
    y.backward(dy.permute(0, 3, 1, 2).double())
    return y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad


def _rounded(t, dtype):
    return t.to(_TD[dtype]).float()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cg", [4, 8, 16, 32])
def test_gconv_fwd_dgrad_wgrad_match_float64(cg, stride, dtype):
    """ragged 17 x 13 maps, strided views (ld > C), 8 groups; forward and dx bit-identical over two launches; dw accumulates onto what is there"""
    init(dtype)
    g = torch.Generator().manual_seed(100 + cg + stride)
    groups, N, H, W = 8, 2, 17, 13
    C = OC = groups * cg
    x = _rounded(torch.randn(N, H, W, C, generator=g), dtype)
    w = _rounded(torch.randn(OC, cg, 3, 3, generator=g) / math.sqrt(9 * cg), dtype)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dyh = _rounded(torch.randn(N, OH, OW, OC, generator=g), dtype)
    yr, dxr, dwr = _ref(x, w, groups, stride, dyh)
    y, xd, wd = _run_fwd(x, w, groups, stride, dtype, ld_in=C + 8, ld_out=OC + 8)
    y2, _, _ = _run_fwd(x, w, groups, stride, dtype, ld_in=C + 8, ld_out=OC + 8)
    torch.cuda.synchronize()
    assert torch.equal(y, y2)
    close_gemm("gconv fwd cg%d s%d" % (cg, stride), y, yr, dtype, out_bits=None if dtype == F32 else 8)
    dy = _padded(dyh, OC + 8, dtype)
    dx = _padded(torch.zeros(N, H, W, C), C + 8, dtype)
    base = torch.randn(OC * 9 * cg, generator=g)
    dw = base.cuda().clone()
    _run_bwd(xd, wd, dy, groups, stride, dtype, dx=dx, dw=dw)
    dx2 = _padded(torch.zeros(N, H, W, C), C + 8, dtype)
    _run_bwd(xd, wd, dy, groups, stride, dtype, dx=dx2)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
    close_gemm("gconv dgrad cg%d s%d" % (cg, stride), dx, dxr, dtype, out_bits=None if dtype == F32 else 8)
    got_dw = (dw.cpu() - base).view(OC, 3, 3, cg).permute(0, 3, 1, 2)
    close_gemm("gconv wgrad cg%d s%d" % (cg, stride), got_dw, dwr, dtype)
    # accumulate: dx += dgrad
    _run_bwd(xd, wd, dy, groups, stride, dtype, dx=dx2, accumulate=True)
    torch.cuda.synchronize()
    close_gemm("gconv dgrad accumulate", dx2, 2 * dxr, dtype, out_bits=None if dtype == F32 else 8)


def test_gconv_bn_stats_fold_relu_and_fp16():
    """the fused BatchNorm statistics (fp64 [8][2 OC] replicas) against torch sums of the stored output; the folded eval form with ReLU; fp16 forward"""
    for dtype in (F32, BF16):
        init(dtype)
        g = torch.Generator().manual_seed(7)
        groups, cg, N, H, W = 16, 8, 2, 19, 11
        C = OC = groups * cg
        x = _rounded(torch.randn(N, H, W, C, generator=g), dtype)
        w = _rounded(torch.randn(OC, cg, 3, 3, generator=g) / math.sqrt(9 * cg), dtype)
        stats = torch.zeros(8 * 2 * OC, dtype=torch.float64, device="cuda")
        y, _, _ = _run_fwd(x, w, groups, 2, dtype, stats=stats)
        torch.cuda.synchronize()
        yv = y.double().cpu().reshape(-1, OC)
        s = stats.cpu().view(8, 2, OC).sum(0)
        assert torch.allclose(s[0], yv.sum(0), rtol=1e-5, atol=1e-4) and torch.allclose(s[1], (yv * yv).sum(0), rtol=1e-5, atol=1e-4)
        scale = torch.rand(OC, generator=g) + 0.5
        shift = torch.randn(OC, generator=g)
        y, _, _ = _run_fwd(x, w, groups, 1, dtype, relu=True, scale=scale.cuda(), bias=shift.cuda())
        yr, _, _ = _ref(x, w, groups, 1)
        want = torch.relu(yr * scale.double() + shift.double())
        close_gemm("gconv folded BN + relu", y, want, dtype, out_bits=None if dtype == F32 else 8)
    init(F32)
    g = torch.Generator().manual_seed(8)
    groups, cg = 64, 4
    x = _rounded(torch.randn(2, 9, 14, groups * cg, generator=g), F16)
    w = _rounded(torch.randn(groups * cg, cg, 3, 3, generator=g) / 6.0, F16)
    y, _, _ = _run_fwd(x, w, groups, 1, F16)
    yr, _, _ = _ref(x, w, groups, 1)
    close_gemm("gconv fwd fp16", y, yr, BF16, out_bits=10)
    # refused geometries / dtypes: an error, no launch
    L = _lib.lib()
    from emrt_amd._lib import EmrtHipError
    xd = torch.zeros(2, 8, 8, 96, device="cuda")
    with pytest.raises(EmrtHipError, match="channels per group"):
        L.call("emrt_gconv2d", _P(xd), _P(xd), _P(xd), None, 2, 8, 8, 96, 96, 8 * 8 * 96, 8, 8, 96, 96, 8 * 8 * 96, 1, 4, 0, None, None, F32, ctx().stream)
    with pytest.raises(EmrtHipError, match="inference-only"):
        L.call("emrt_gconv2d_bwd", _P(xd), _P(xd), _P(xd), _P(xd), 96, 8 * 8 * 96, 0, None, None, 2, 8, 8, 96, 96, 8 * 8 * 96, 8, 8, 96, 96, 8 * 8 * 96, 1, 24,
               F16, ctx().stream)


@pytest.mark.parametrize("shape", [(8, 64, 64, 256, 1), (8, 16, 16, 2048, 2)], ids=["stage1", "stage4-first"])
def test_gconv_training_shapes_bf16(shape):
    """the exact stage-1 and (strided) stage-4 shapes of a batch-8 256 x 256 training step, bf16"""
    init(BF16)
    N, H, W, C, stride = shape
    groups, cg = 64, C // 64
    g = torch.Generator().manual_seed(9)
    x = _rounded(torch.randn(N, H, W, C, generator=g), BF16)
    w = _rounded(torch.randn(C, cg, 3, 3, generator=g) / math.sqrt(9 * cg), BF16)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dyh = _rounded(torch.randn(N, OH, OW, C, generator=g), BF16)
    yr, dxr, dwr = _ref(x, w, groups, stride, dyh)
    y, xd, wd = _run_fwd(x, w, groups, stride, BF16)
    close_gemm("stage fwd", y, yr, BF16, out_bits=8)
    dx = torch.zeros(N, H, W, C, dtype=torch.bfloat16, device="cuda")
    dw = torch.zeros(C * 9 * cg, device="cuda")
    _run_bwd(xd, wd, dyh.to(device="cuda", dtype=torch.bfloat16), groups, stride, BF16, dx=dx, dw=dw)
    torch.cuda.synchronize()
    close_gemm("stage dgrad", dx, dxr, BF16, out_bits=8)
    close_gemm("stage wgrad", dw.cpu().view(C, 3, 3, cg).permute(0, 3, 1, 2), dwr, BF16)


# ---------------------------------------------------------------------------------------------------
# whole model: float64 ResNeXt-50 64x4d (written from backbones/resnext.py's structure) inside the oracle EMRT
# ---------------------------------------------------------------------------------------------------
class _OCBL(tnn.Module):
    def __init__(self, cin, cout, k, stride=1, groups=1, act=True):
        super().__init__()
        from oracle.emrt_torch import BatchNorm2D
        self._conv = tnn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False)
        self._batch_norm = BatchNorm2D(cout)
        self.act = act

    def forward(self, x):
        y = self._batch_norm(self._conv(x))
        return torch.relu(y) if self.act else y


class _OBlock(tnn.Module):
    def __init__(self, cin, w, stride, shortcut):
        super().__init__()
        self.conv0 = _OCBL(cin, w, 1)
        self.conv1 = _OCBL(w, w, 3, stride, groups=64)
        self.conv2 = _OCBL(w, w, 1, act=False)
        if not shortcut:
            self.short = _OCBL(cin, w, 1, stride, act=False)
        self.shortcut = shortcut

    def forward(self, x):
        y = self.conv2(self.conv1(self.conv0(x)))
        return torch.relu(y + (x if self.shortcut else self.short(x)))


class OracleResNeXt50(tnn.Module):
    def __init__(self):
        super().__init__()
        self.conv = _OCBL(3, 64, 7, 2)
        self.blocks = []
        cin = 64
        for s, (n, w) in enumerate(zip([3, 4, 6, 3], [256, 512, 1024, 2048])):
            for i in range(n):
                b = _OBlock(cin, w, 2 if (i == 0 and s > 0) else 1, shortcut=i > 0)
                self.add_module("bb_%d_%d" % (s, i), b)
                self.blocks.append(b)
                cin = w
        self.out = tnn.Linear(2048, 1000)

    def forward(self, x):
        y = F.max_pool2d(self.conv(x), 3, 2, 1)
        outs = []
        for b in self.blocks:
            y = b(y)
            outs.append(y)
        return outs[2], outs[6], outs[12], outs[15]


def _oracle_resnext_emrt(x, seed=0, condition=0.2):
    """condition: the residual branches' last BatchNorm gamma scaled down, as tests/test_gpu_model.py::condition_residual_branches does for the
    ResNet (a randomly initialised BatchNorm network is chaotic: at gamma 1 the float32 oracle itself lands 1.5e-3 from its float64 logits here)"""
    from oracle.emrt_torch import EMRT as OracleEMRT, BatchNorm2D as OBN
    from tests.test_gpu_model import oracle_no_dropout, perturb_sampling_offsets
    torch.manual_seed(seed)
    ref = OracleEMRT(6, "resnet50")
    bb = OracleResNeXt50()
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, tnn.Conv2d):
                fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.normal_(0.0, math.sqrt(2.0 / fan))
        for b in bb.blocks:
            b.conv2._batch_norm.weight.mul_(condition)
        for n, m in ref.named_modules():
            if n.startswith("EFP.") and n.endswith(".conv2.1"):
                m.weight.mul_(condition)
    ref.backbone = bb
    oracle_no_dropout(ref)
    # calibrate the running statistics with one train-mode pass (momentum 0), as test_resnet50c_model_matches_oracle does
    for mod in ref.modules():
        if isinstance(mod, OBN):
            mod.momentum = 0.0
    ref.train()
    with torch.no_grad():
        ref(x)
    for mod in ref.modules():
        if isinstance(mod, OBN):
            mod.momentum = 0.9
    perturb_sampling_offsets(ref)
    return ref


def _hip_resnext(state, dtype):
    import argparse
    from emrt_amd.config import get_config, update_config
    from emrt_amd.src.models import get_model
    from tests.test_gpu_model import CFG
    cfg = update_config(get_config(), argparse.Namespace(cfg=CFG))
    cfg.MODEL.ENCODER.TYPE = "resnext50"
    model = get_model(cfg)
    model.load_state_dict(state)
    model.to_hip("cuda:0", dtype)
    model.set_dropout(0.0)
    return model, cfg


def test_resnext50_model_matches_oracle():
    """eval logits within 1e-3 of the float64 oracle, argmax equal up to near-ties; one train-mode forward + backward: loss, whole-gradient cosine
    and every grouped layer's weight gradient"""
    from emrt_amd.src.models.losses import get_loss_function
    from oracle import train_ref
    from tests.test_gpu_model import assert_argmax_match
    g = torch.Generator().manual_seed(73)
    B, S = 2, 64
    x = torch.randn(B, 3, S, S, generator=g)
    labels = torch.randint(0, 6, (B, S, S), generator=g)
    ref = _oracle_resnext_emrt(x)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    model, cfg = _hip_resnext(sd, F32)
    ref.eval()
    model.eval()
    got = model(x.cuda())
    with torch.no_grad():
        ref.double()
        want = [t.float() for t in ref(x.double())]
    for name, a, b in (("main", got[0].cpu(), want[0]), ("aux", got[1].cpu(), want[1])):
        err = (a - b).abs().max().item()
        print("resnext50 %s logits: max |diff| vs float64 oracle %.3g" % (name, err))
        assert err < 1e-3, (name, err)
    assert_argmax_match(got[0].cpu(), want[0])
    ref.load_state_dict(sd)
    ref.train()
    loss_r = train_ref.mix_softmax_ce_loss(ref(x.double()), labels)
    loss_r.backward()
    model.train()
    model.clear_gradients()
    loss = get_loss_function(cfg)(model(x.cuda()), labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    print("resnext50 train loss %.6f vs oracle %.6f" % (loss.item(), loss_r.item()))
    assert abs(loss.item() - loss_r.item()) < 2e-4 * max(1.0, abs(loss_r.item()))
    refp = dict(ref.named_parameters())
    dot = n1 = n2 = 0.0
    worst = 0.0
    for n, p in model.named_parameters():
        gr = refp[n].grad
        if gr is None:
            continue
        gg, gr = p.grad.cpu().double(), gr.double()
        dot += float((gg * gr).sum()); n1 += float((gg * gg).sum()); n2 += float((gr * gr).sum())
        if ".conv1._conv." in n:          # the grouped layers: each gradient on its own
            rel = float((gg - gr).norm() / gr.norm().clamp_min(1e-30))
            worst = max(worst, rel)
            assert rel < 2e-2, (n, rel)
    cos = dot / (n1 ** 0.5 * n2 ** 0.5)
    print("resnext50 gradient cosine %.6f, norm ratio %.5f, worst grouped-layer relative error %.3g" % (cos, (n1 / n2) ** 0.5, worst))
    assert cos > 0.999 and abs((n1 / n2) ** 0.5 - 1.0) < 2e-2


def test_resnext50_captured_bf16_step_equals_eager_and_tracks_fp32():
    """the bf16 step of the engine bench.py times (TrainEngine, captured hipGraph) against the eager bf16 engine over 3 steps, and step 1's
    loss against the fp32 HIP model's (itself held to the float64 oracle above)"""
    from emrt_amd.engine import TrainEngine
    from emrt_amd.src.models.losses import get_loss_function
    from emrt_amd.src.models.solver import get_optimizer, get_scheduler
    g = torch.Generator().manual_seed(31)
    B, S = 2, 128
    x = torch.randn(B, 3, S, S, generator=g)
    labels = torch.randint(0, 6, (B, S, S), generator=g)
    ref = _oracle_resnext_emrt(x[:, :, :64, :64], seed=1, condition=0.1)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    xd, ld = x.cuda(), labels.cuda()
    runs = {}
    for mode, dtype in (("fp32", F32), ("eager", BF16), ("graph", BF16)):
        model, cfg = _hip_resnext(state, dtype)
        model.eval()
        model(xd)
        model.train()
        opt = get_optimizer(model, get_scheduler(cfg), cfg)
        eng = TrainEngine(model, opt, get_loss_function(cfg), 1, use_graph=(mode == "graph"), warmup_eager=0)
        losses = [eng.step(xd, ld).item() for _ in range(3)]
        torch.cuda.synchronize()
        n = model.store.n_train
        runs[mode] = (losses, model.store.master[:n].clone())
        if mode == "graph":
            assert eng.graph_a is not None and eng.calls == 3
    print("resnext50 losses fp32 %s eager bf16 %s captured bf16 %s" % (runs["fp32"][0], runs["eager"][0], runs["graph"][0]))
    for a, b in zip(runs["eager"][0], runs["graph"][0]):
        assert abs(a - b) < 1e-3 * abs(a), (a, b)
    we, wg = runs["eager"][1], runs["graph"][1]
    assert float((we - wg).norm() / we.norm()) < 2e-4
    for a, b in zip(runs["fp32"][0], runs["graph"][0]):
        assert abs(a - b) < 2e-2 * abs(a), (a, b)
    assert all(math.isfinite(v) for v in runs["graph"][0])
