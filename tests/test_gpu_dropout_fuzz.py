"""-m gpu: emrt_dropout_fwd and emrt_mask_bwd (csrc/elementwise.hip), fp32 and bf16, called directly, every mask held bit for bit to the host
model of csrc/drop_hash.hpp (tests/dropout_reference.py; tests/test_dropout_reference_cpu.py holds that model to the header and checks its
statistics on the CPU -- no statistic is taken here).  The case list is fuzz_cases.CASES["dropout"]: element mode at one lane, around a block
and once past the 8192 blocks of the grid (the second trip round the grid-stride loop); channel mode (Dropout2D on NHWC) with N > 1, hw in
{1, 25}, C in {4, 64, 100}, also where C hw is no multiple of a block's 1024 elements; p in {0, 2^-17, 0.1, 0.5, 0.999}; every arm of
emrt_mask_bwd.  Each case has its own 64-bit seed word on the device (0, small, the top bit set, the context's default) and its own salt.

What is asserted, forward and backward alike:
  * the device's mask (output != 0; x and dy are nowhere zero) equals the model's, bit for bit; in channel mode every (image, channel) plane is
    all kept or all dropped;
  * a dropped element is exactly 0;
  * a kept element equals the torch fp32 expression round_T(x * ks), ks = 1.f / (1.f - p), bit for bit -- the kernel's two fp32 operations and
    its one rounding to the compute type have one answer each.  That is the stronger of the two checks the sweep was specified with; the weaker
    one is asserted too: |kept - x / (1 - p)| <= half an ulp of the compute type + 2 fp32 ulps against float64 on the rounded operand (the
    two ulps cover ks and the product, each rounded once in fp32);
  * p = 0 is the identity bit for bit; p = 2^-17 (threshold 0) drops nothing in element mode and still scales by 1 / (1 - 2^-17).
The backward's relu_out has zeros, negatives and positives; its fourth arm (seed == NULL, p > 0) takes the stored output of emrt_conv2d_drop,
built here from the model: (relu_out > 0) is both masks, the kernel only scales.

The 64-bit index branches need more than 2^32 elements and stay unexercised here.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                    # noqa: E402
from emrt_amd.functional import P                            # noqa: E402
from emrt_amd.runtime import F32, BF16                       # noqa: E402
from tests import dropout_reference as dr                    # noqa: E402
from tests import fuzz_cases as fc                           # noqa: E402
from tests.hip_utils import init                             # noqa: E402

NAME = {F32: "f32", BF16: "bf16"}
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
BITS = {F32: 24, BF16: 8}          # significant bits of the compute type
PARAMS = [pytest.param(c, d, id="%s-%s" % (c[0], NAME[d])) for c in fc.CASES["dropout"] for d in (F32, BF16) if c[5] in ("both", NAME[d])]


def _ulp(x64, bits):
    a = x64.abs().clamp_min(2.0 ** -126)
    _, ex = torch.frexp(a)
    return torch.ldexp(torch.ones_like(a), ex - bits)


def _seed_tensor(word):
    return torch.tensor([word - (1 << 64) if word >> 63 else word], dtype=torch.int64).cuda()


def _nonzero(n, g, tdtype):
    """[n] values of both signs, nowhere zero, rounded through the compute type (CPU, as that type)"""
    x = torch.randn(n, generator=g) * 2.0
    x = torch.where(x.abs() < 0.01, torch.full_like(x, 0.75), x)
    return x.to(tdtype)


def _model_mask(case):
    _, mode, dims, p, _, _, salt, _, seed = case
    n = fc.drop_n(case)
    if mode == "element":
        keep = dr.element_mask(seed, salt, p, n)
    else:
        keep = dr.channel_mask(seed, salt, p, n, dims[1], dims[2])
    return torch.from_numpy(np.ascontiguousarray(keep))


def _scaled(x, p):
    """round_T(x * ks) with ks = 1.f / (1.f - p) in fp32: the torch fp32 expression of a kept element"""
    ks = torch.tensor(float(dr.keep_scale(p)), dtype=torch.float32)
    return (x.float() * ks).to(x.dtype)


def _same_bits(a, b):
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _check(name, got, src, on, p, dtype):
    """got: the kernel's output (CPU); src: what it scaled; on: where the model (and, in the backward, relu_out) lets a value through"""
    assert torch.equal(got != 0, on), "%s: the device's mask differs from the model's at %d of %d elements (first %s)" % (
        name, int(((got != 0) != on).sum()), on.numel(), torch.nonzero((got != 0) != on)[:4].flatten().tolist())
    assert bool((got[~on] == 0).all())
    want = torch.where(on, _scaled(src, p) if p > 0.0 else src, torch.zeros_like(src))
    ref = src.double()[on] / (1.0 - float(np.float32(p)))
    err = (got.double()[on] - ref).abs()
    bound = _ulp(ref, BITS[dtype]) / 2 + 2 * _ulp(ref, 24)
    assert bool((err <= bound).all()), "%s: a kept element is off x / (1 - p) by %.3g, bound %.3g" % (name, err.max().item(), bound[err.argmax()].item())
    assert torch.equal(got, want), "%s: %d kept elements differ from round(x * ks) in fp32" % (name, int((got != want).sum()))


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_dropout_masks_are_the_models(case, dtype):
    cid, mode, dims, p, arms, _, salt, _, seed = case
    c = init(dtype)
    L_ = _lib.lib()
    tdt = TORCH[dtype]
    n = fc.drop_n(case)
    m, hw, C = (0, 0, 0) if mode == "element" else (1, dims[1], dims[2])
    g = torch.Generator().manual_seed(seed % (1 << 31) + salt % 1000)
    sd = _seed_tensor(seed)
    keep = _model_mask(case)
    if p in (0.0, 2.0 ** -17) and mode == "element":
        assert bool(keep.all())          # threshold 0
    x = _nonzero(n, g, tdt)
    xd = x.cuda()
    y = torch.full((n + 8,), 3.0, dtype=tdt, device="cuda")          # (two quads of sentinel behind the output)
    L_.call("emrt_dropout_fwd", P(xd), P(y), n, float(p), P(sd), salt, m, hw, C, dtype, c.stream)
    torch.cuda.synchronize()
    assert bool((y[n:] == 3.0).all()), "%s: written past n" % cid
    got = y[:n].cpu()
    if p == 0.0:
        assert _same_bits(got, x), "%s: p = 0 is not the identity" % cid
    _check("%s forward" % cid, got, x, keep, p, dtype)
    if mode == "channel":
        planes = (got != 0).view(dims[0], hw, C)
        assert bool((planes == planes[:, :1]).all()), "%s: an (image, channel) plane is neither all kept nor all dropped" % cid
    # ---- emrt_mask_bwd ----
    dy = _nonzero(n, g, tdt)
    dyd = dy.cuda()
    r = torch.randn(n, generator=g).to(tdt)
    r[torch.rand(n, generator=g) < 0.2] = 0.0          # relu_out: zeros, negatives, positives
    rd = r.cuda()
    for arm in arms:
        dx = torch.full((n + 8,), 3.0, dtype=tdt, device="cuda")
        if arm == "mask":
            L_.call("emrt_mask_bwd", P(dyd), None, P(dx), n, float(p), P(sd), salt, m, hw, C, dtype, c.stream)
            on = keep
        elif arm == "mask+relu":
            L_.call("emrt_mask_bwd", P(dyd), P(rd), P(dx), n, float(p), P(sd), salt, m, hw, C, dtype, c.stream)
            on = keep & (r > 0)
        elif arm == "relu":
            L_.call("emrt_mask_bwd", P(dyd), P(rd), P(dx), n, 0.0, None, 0, 0, 1, 1, dtype, c.stream)
            on = r > 0
        else:          # "stored": what emrt_conv2d_drop would have stored for the pre-activations r under this mask
            stored = torch.where(keep & (r > 0), _scaled(r, p), torch.zeros_like(r))
            sdev = stored.cuda()
            L_.call("emrt_mask_bwd", P(dyd), P(sdev), P(dx), n, float(p), None, 0, 0, 1, 1, dtype, c.stream)
            on = stored > 0
            assert torch.equal(on, keep & (r > 0))
        torch.cuda.synchronize()
        assert bool((dx[n:] == 3.0).all()), "%s %s: written past n" % (cid, arm)
        gx = dx[:n].cpu()
        if arm == "relu":
            assert _same_bits(gx, torch.where(on, dy, torch.zeros_like(dy))), "%s: the ReLU mask alone is not dy or +0 bit for bit" % cid
        _check("%s backward, %s" % (cid, arm), gx, dy, on, p, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_mask_bwd_p0_without_relu_out_is_a_copy(dtype):
    """neither mask: dx = dy bit for bit (NaN payloads and -0 included)"""
    c = init(dtype)
    tdt = TORCH[dtype]
    dy = torch.tensor([1.5, -0.0, 0.0, float("inf"), -2.0, float("nan"), 1e-30, -3.0], dtype=tdt)
    dx = torch.zeros(8, dtype=tdt, device="cuda")
    dyd = dy.cuda()
    _lib.lib().call("emrt_mask_bwd", P(dyd), None, P(dx), 8, 0.0, None, 0, 0, 1, 1, dtype, c.stream)
    torch.cuda.synchronize()
    got = dx.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(dy)) and _same_bits(torch.nan_to_num(got, 7.0), torch.nan_to_num(dy, 7.0))
