"""-m gpu: float16 (EMRT_DTYPE_F16 = 2) parity of every forward entry point that takes it, one kernel at a time.

float16 is the arithmetic of `val.py --dtype fp16`, `model.to_hip(..., F16)` and BASELINE configs[4]; the whole-model bounds that cover it
(relative L2 < 2e-2) cannot see one kernel.  Here every entry point that reaches EMRT_REQUIRE_FWD_DTYPE is compared with a float64 torch
reference on the CPU, on operands already rounded through float16, under the bound of tests/hip_utils.close_f16:

    |got - ref64| <= ulp16(ref64) / 2 + slack

where `slack` bounds the kernel's fp32 arithmetic only and is computed from the reference (hip_utils.gemm_slack / terms_slack, or a derived
term explained where it is used).  Where a kernel's CONTRACT rounds an intermediate to float16 (attention probabilities packed for the PV
product, LayerNorm's q_out = round(out) + pos and its z buffer) the reference applies the same rounding; the bound does not widen.
hip_utils.rounding_is_nearest checks the direction of the final rounding on large cases (a truncating conversion sits at -0.5 ulp).

COVERED / EXEMPT / NO_DTYPE at the end are the ledger tests/test_fp16_ledger_cpu.py checks against the sources: a new float16 entry point
without a test here fails the CPU suite.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                       # noqa: E402
from emrt_amd import functional as Fn          # noqa: E402
from emrt_amd import nn as hnn                  # noqa: E402
from emrt_amd.functional import P              # noqa: E402
from emrt_amd.runtime import ctx, F16          # noqa: E402
from tests.hip_utils import (init, Holder, close_f16, rounding_is_nearest, gemm_slack, terms_slack, round16, ulp16, EPS32,   # noqa: E402
                             F16_INF_FROM)

HALF = torch.float16


def _init():
    c = init(F16)
    c.training = False
    return c


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rh(t):
    """CPU fp32 -> rounded through float16 (one correctly rounded cast), as float64"""
    return t.half().double()


def _d(t64, dtype=HALF):
    """float64 CPU tensor that is exactly representable in `dtype` -> device tensor"""
    return t64.to(dtype).contiguous().cuda()


def _nhwc(t_nchw):
    return t_nchw.permute(0, 2, 3, 1).contiguous()


class _knobs:
    """set tuning knobs for a block, restore after"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        L = _lib.lib()
        self.old = [(k, L.set_tuning(k, v)) for k, v in self.kv.items()]

    def __exit__(self, *exc):
        L = _lib.lib()
        for k, v in self.old:
            L.set_tuning(k, v)


# =====================================================================================================================================
# convolution
# =====================================================================================================================================
def _conv_launch(xv, wd, outv, stride=1, pad=0, dil=1, bias=None, res=None, relu=False, out_f32=False, scale=None):
    """emrt_conv2d through the C ABI on NHWC views: xv [N,H,W,C], wd the forward operand [OC][KH][KW][C], outv [N,OH,OW,OC]"""
    N, H, W, C, ldin, in_bs = Fn._check_map(xv)
    _, OH, OW, OC, ldout, out_bs = Fn._check_map(outv)
    KH, KW = wd.shape[1], wd.shape[2]
    ldres = res_bs = 0
    if res is not None:
        ldres, res_bs = Fn._check_map(res)[4:6]
    _lib.lib().call("emrt_conv2d", P(xv), P(wd), P(outv), P(bias), P(res), N, H, W, C, ldin, in_bs, OH, OW, OC, ldout, out_bs, ldres, res_bs,
                    KH, KW, stride, pad, 0, int(relu), int(out_f32), None, None, 0, 0, dil, P(scale), F16, ctx().stream)


def _conv_ref(x, w, stride=1, pad=0, dil=1, bias=None, res=None, relu=False, scale=None):
    """float64 reference in NHWC and its slack.  x [N,C,H,W], w [OC,C,KH,KW] float64 (float16 values); bias / scale fp32 values as float64 [OC];
    res NHWC float64.  Kernel epilogue (csrc/conv.hip): v = fma(acc, scale, bias) + res, relu -- the contraction's slack scales with |scale|,
    and the epilogue's two fp32 operations get terms_slack of their operands."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    acc = _nhwc(F.conv2d(x, w, None, stride, pad, dil))
    sl = gemm_slack(K, _nhwc(F.conv2d(x * x, w * w, None, stride, pad, dil)))
    y = acc
    terms = []
    if scale is not None:
        y = y * scale
        sl = sl * scale.abs()
    if bias is not None:
        terms += [y, bias.expand_as(y)]
        y = y + bias
    if res is not None:
        terms += [y, res]
        y = y + res
    if terms:
        sl = sl + terms_slack(*terms)
    if relu:
        y = y.clamp_min(0)
    return y, sl


def _conv_case(name, N, H, W, C, OC, k, stride=1, pad=0, dil=1, bias=False, res=False, relu=False, out_f32=False, fold=False, seed=1, wscale=1.0,
               xscale=1.0, check=True):
    g = _gen(seed)
    x = _rh(torch.randn(N, C, H, W, generator=g) * xscale)
    w = _rh(torch.randn(OC, C, k, k, generator=g) * (wscale / math.sqrt(C * k * k)))
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    b = torch.randn(OC, generator=g).double() if (bias or fold) else None
    sc = (torch.rand(OC, generator=g) + 0.5).double() if fold else None
    if fold:
        sc[::3] *= -1          # a negative BatchNorm gamma
    r = _rh(torch.randn(N, OH, OW, OC, generator=g)) if res else None
    want, sl = _conv_ref(x, w, stride, pad, dil, b, r, relu, sc)
    xd, wd = _d(_nhwc(x)), _d(_nhwc(w))
    out = torch.full((N, OH, OW, OC), float("nan"), dtype=torch.float32 if out_f32 else HALF, device="cuda")
    _conv_launch(xd, wd, out, stride, pad, dil, _d(b, torch.float32) if b is not None else None, _d(r) if res else None, relu, out_f32,
                 _d(sc, torch.float32) if fold else None)
    torch.cuda.synchronize()
    if check:
        close_f16(name, out, want, sl, out_f32=out_f32)
    return out, want, sl


@pytest.mark.parametrize("case", [
    dict(name="relu", N=2, H=16, W=16, C=64, OC=64, k=3, pad=1, relu=True),
    dict(name="residual+relu", N=2, H=12, W=20, C=128, OC=256, k=1, res=True, relu=True),
    dict(name="bias+residual", N=1, H=9, W=11, C=72, OC=40, k=3, pad=1, bias=True, res=True),          # channel counts off the 8-element grid
    dict(name="folded-bn+relu", N=2, H=16, W=16, C=64, OC=128, k=3, pad=1, fold=True, relu=True),
    dict(name="folded-bn-1x1", N=2, H=8, W=8, C=512, OC=64, k=1, fold=True),
    dict(name="out_f32", N=2, H=16, W=16, C=256, OC=64, k=1, bias=True, out_f32=True),
    dict(name="out_f32-thin", N=1, H=24, W=24, C=64, OC=6, k=1, bias=True, out_f32=True),
    dict(name="thin-oc6-4096px", N=1, H=64, W=64, C=256, OC=6, k=1, bias=True),
    dict(name="thin-oc7-ragged", N=3, H=17, W=19, C=512, OC=7, k=1, bias=True),
    dict(name="dilation2", N=2, H=15, W=13, C=64, OC=64, k=3, pad=2, dil=2),
    dict(name="dilation4", N=1, H=20, W=20, C=128, OC=96, k=3, pad=4, dil=4, relu=True),
    dict(name="stride2-3x3", N=2, H=17, W=16, C=64, OC=128, k=3, stride=2, pad=1),
    dict(name="stride2-1x1", N=2, H=16, W=16, C=256, OC=512, k=1, stride=2),
    dict(name="stem-7x7", N=1, H=32, W=32, C=3, OC=64, k=7, stride=2, pad=3),
    dict(name="long-k-xk", N=2, H=8, W=8, C=512, OC=512, k=3, pad=1),                                     # cross-block K split by default
], ids=lambda c_: c_["name"])
def test_conv2d_epilogues_and_geometries(case):
    _init()
    case = dict(case)
    _conv_case("conv " + case.pop("name"), **case)


def test_conv2d_token_slab_input_and_concat_slice_output():
    """input: a level slab of a [B, Lv, C] token tensor read as a map (ld = C, batch stride Lv * C); output: a channel slice of a wider concat
    buffer whose other channels must stay untouched; residual: another strided view"""
    _init()
    g = _gen(3)
    B, h, w, C, OC, Lv, s0 = 2, 8, 6, 64, 64, 100, 20
    tok = _rh(torch.randn(B, Lv, C, generator=g))
    wt = _rh(torch.randn(OC, C, 3, 3, generator=g) / math.sqrt(9 * C))
    resw = _rh(torch.randn(B, h, w, 3 * OC, generator=g))
    x = tok[:, s0:s0 + h * w].reshape(B, h, w, C).permute(0, 3, 1, 2)
    res = resw[..., OC:2 * OC]
    want, sl = _conv_ref(x, wt, 1, 1, 1, None, res, True, None)
    tokd = _d(tok)
    xv = Fn.tokens_as_map(tokd[:, s0:s0 + h * w], h, w)
    cat = torch.full((B, h, w, 2 * OC + 8), 7.0, dtype=HALF, device="cuda")
    resd = _d(resw)
    _conv_launch(xv, _d(_nhwc(wt)), cat[..., 8:8 + OC], 1, 1, 1, None, resd[..., OC:2 * OC], True)
    torch.cuda.synchronize()
    close_f16("conv slab -> concat slice", cat[..., 8:8 + OC], want, sl)
    assert float((cat[..., :8].float() - 7.0).abs().max()) == 0.0 and float((cat[..., 8 + OC:].float() - 7.0).abs().max()) == 0.0


def _big_cases():
    from tests.test_gpu_conv_fuzz import BIG
    return BIG


@pytest.mark.parametrize("idx", range(10))
def test_conv2d_big_geometries_through_every_tile(idx):
    """the BIG geometries of test_gpu_conv_fuzz.py, forward only: the dispatcher's own choice (conv_tile 0) and every forced tile
    (1 = 64x64, 2 = 128x64, 3 = 128x128, 4 = 128x32, 5 / 6 = in-block K split, 7 = 256x256 LDS-DMA where its shape conditions hold, 8 = 128x128
    with the K split over two wave groups) and the cross-block K split (xk = 3), one float64 reference for all of them"""
    _init()
    name, N, H, W, Cin, Cout, k, stride, pad, bias, dil = _big_cases()[idx]
    g = _gen(400 + idx)
    x = _rh(torch.randn(N, Cin, H, W, generator=g))
    w = _rh(torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k))
    b = torch.randn(Cout, generator=g).double() if bias else None
    want, sl = _conv_ref(x, w, stride, pad, dil, b, None, False, None)
    xd, wd, bd = _d(_nhwc(x)), _d(_nhwc(w)), (_d(b, torch.float32) if bias else None)
    for knobs in [dict(conv_tile=t) for t in range(0, 9)] + [dict(xk=3)]:
        out = torch.full(tuple(want.shape), float("nan"), dtype=HALF, device="cuda")
        with _knobs(**knobs):
            _conv_launch(xd, wd, out, stride, pad, dil, bd)
            torch.cuda.synchronize()
        close_f16("conv %s %s" % (name, knobs), out, want, sl)


def test_conv2d_outputs_straddle_the_float16_maximum():
    """outputs scaled so that a good part lies beyond +-65504: inf exactly where the float64 result rounds to inf, finite elsewhere"""
    _init()
    out, want, _ = _conv_case("conv overflow", N=2, H=16, W=16, C=64, OC=64, k=3, pad=1, bias=True, wscale=40000.0, seed=9)
    frac = (want.abs() >= F16_INF_FROM).double().mean().item()
    assert 0.05 < frac < 0.6, frac
    assert int(torch.isinf(out).sum()) > 0 and int(torch.isfinite(out).sum()) > 0


def test_conv2d_outputs_mostly_subnormal():
    """outputs around 2^-17: most below the smallest normal float16 (6.1e-5), where the spacing is 2^-24 whatever the value"""
    _init()
    out, want, _ = _conv_case("conv subnormal", N=2, H=16, W=16, C=64, OC=64, k=3, pad=1, wscale=2.0 ** -7, xscale=2.0 ** -10, seed=10)
    frac = (want.abs() < 2.0 ** -14).double().mean().item()
    assert frac > 0.9, frac
    assert float(out.float().abs().max()) > 0.0          # not flushed to zero


def test_conv2d_rounds_to_nearest():
    _init()
    out, want, _ = _conv_case("conv rounding", N=2, H=32, W=32, C=64, OC=128, k=3, pad=1, seed=11)
    rounding_is_nearest("conv2d", out, want)


@pytest.mark.parametrize("n", [2, 6])
def test_conv2d_group_unequal_problems(n):
    """emrt_conv2d_group: n problems of different sizes in one launch (1x1 and 3x3, strided input views, relu, residual, bias)"""
    c = _init()
    g = _gen(20 + n)
    geoms = [(2, 8, 8, 64, 64, 1, 0), (1, 12, 10, 128, 64, 3, 1), (2, 5, 7, 64, 128, 3, 1), (3, 4, 4, 256, 64, 1, 0), (1, 16, 16, 64, 192, 1, 0),
             (2, 6, 6, 128, 128, 3, 1)][:n]
    descs = (Fn._ConvDesc * n)()          # EmrtConvDesc (include/emrt_hip.h)
    keep, checks = [], []
    for i, (d, (N, H, W, C, OC, k, pad)) in enumerate(zip(descs, geoms)):
        x = _rh(torch.randn(N, C, H, W, generator=g))
        w = _rh(torch.randn(OC, C, k, k, generator=g) / math.sqrt(C * k * k))
        b = torch.randn(OC, generator=g).double() if i % 2 == 0 else None
        r = _rh(torch.randn(N, H, W, OC, generator=g)) if i % 3 == 1 else None
        relu = i % 2 == 1
        want, sl = _conv_ref(x, w, 1, pad, 1, b, r, relu, None)
        wide = torch.zeros(N, H, W, C + 8, dtype=HALF, device="cuda")          # input as a channel slice of a wider map
        wide[..., :C] = _d(_nhwc(x))
        xv = wide[..., :C]
        wd, out = _d(_nhwc(w)), torch.full((N, H, W, OC), float("nan"), dtype=HALF, device="cuda")
        bd, rd = (_d(b, torch.float32) if b is not None else None), (_d(r) if r is not None else None)
        keep += [wide, wd, out, bd, rd]
        _, _, _, _, ldin, in_bs = Fn._check_map(xv)
        d.inp, d.w_packed, d.out, d.bias, d.residual, d.bn_stats = xv.data_ptr(), wd.data_ptr(), out.data_ptr(), Fn._dp(bd), Fn._dp(rd), None
        d.N, d.H, d.W, d.C, d.ldin, d.in_bs = N, H, W, C, ldin, in_bs
        d.OH, d.OW, d.OC, d.ldout, d.out_bs = H, W, OC, OC, H * W * OC
        d.ldres, d.res_bs = (OC, H * W * OC) if r is not None else (0, 0)
        d.KH, d.KW, d.stride, d.pad, d.relu, d.out_f32 = k, k, 1, pad, int(relu), 0
        checks.append((out, want, sl))
    _lib.lib().call("emrt_conv2d_group", descs, n, F16, c.stream)
    torch.cuda.synchronize()
    for i, (out, want, sl) in enumerate(checks):
        close_f16("conv group %d/%d" % (i, n), out, want, sl)


def test_gconv2d_grouped_3x3():
    """emrt_gconv2d (ResNeXt): stride 1 and 2, folded BatchNorm + relu, strided views"""
    c = _init()
    g = _gen(30)
    for stride, fold in ((1, False), (2, True)):
        N, H, W, groups, cg = 2, 9, 14, 8, 8
        C = groups * cg
        x = _rh(torch.randn(N, C, H, W, generator=g))
        w = _rh(torch.randn(C, cg, 3, 3, generator=g) / math.sqrt(9 * cg))
        sc = (torch.rand(C, generator=g) + 0.5).double() if fold else None
        sh = torch.randn(C, generator=g).double() if fold else None
        acc = _nhwc(F.conv2d(x, w, None, stride, 1, 1, groups))
        sl = gemm_slack(9 * cg, _nhwc(F.conv2d(x * x, w * w, None, stride, 1, 1, groups)))
        want = acc
        if fold:
            want = (acc * sc + sh).clamp_min(0)
            sl = sl * sc.abs() + terms_slack(acc * sc, sh.expand_as(acc))
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        wide = torch.zeros(N, H, W, C + 16, dtype=HALF, device="cuda")
        wide[..., 16:] = _d(_nhwc(x))
        xv = wide[..., 16:]
        out = torch.full((N, OH, OW, C), float("nan"), dtype=HALF, device="cuda")
        wd, shd, scd = _d(_nhwc(w)), (_d(sh, torch.float32) if fold else None), (_d(sc, torch.float32) if fold else None)
        _lib.lib().call("emrt_gconv2d", P(xv), P(wd), P(out), P(shd), N, H, W, C, xv.stride(2), xv.stride(0), OH, OW, C, C, OH * OW * C, stride, groups,
                        int(fold), None, P(scd), F16, c.stream)
        torch.cuda.synchronize()
        close_f16("gconv stride %d fold %d" % (stride, fold), out, want, sl)


# =====================================================================================================================================
# attention
# =====================================================================================================================================
def _mha_ref(q, k, v, M, rounded_probs):
    """float64 softmax(q k^T * scale) v per head, scale = fp32(1 / sqrt(32)) as the kernels use it; q, k, v [B, L, M * 32] float64.
    rounded_probs (the MFMA kernel's contract, csrc/attn.hip: the probabilities are packed to float16 as the B operand of the PV product):
    p -> round16(p).  Returns (out, slack).

    slack, derived:
      * scores: a K = 32 contraction in fp32 (gemm_slack) times scale, and the scaling's own rounding: ds_j;
      * probabilities: p_j = __expf(s_j - mx) / sum.  __expf is v_exp_f32(x * log2 e): the argument's rounding is |x| 2^-24 relative in the
        result, the instruction itself ~1 ulp; the sum of L terms and the reciprocal a few ulp more.  Relative error of p_j:
        rel_j = 2 ds_j + (2 |s_j - mx| + 8 + 8 sqrt(L) |e|_2 / |e|_1) 2^-24;
      * VALU kernel (fp32 probabilities): sum_j rel_j p_j |v_j| plus the PV contraction's gemm_slack;
      * MFMA kernel: the rounding to float16 absorbs that error unless p_j lies within rel_j p_j of a float16 rounding boundary, where the
        kernel may round the other way: such a j contributes ulp16(p_j) |v_j|, every other j nothing; plus the PV contraction's gemm_slack."""
    B, L, E = q.shape
    scale = float(torch.tensor(1.0 / math.sqrt(32.0), dtype=torch.float32))
    qh, kh, vh = (t.reshape(B, L, M, 32).permute(0, 2, 1, 3) for t in (q, k, v))          # [B, M, L, 32]
    raw = qh @ kh.transpose(-1, -2)
    s = raw * scale
    ds = gemm_slack(32, (qh * qh) @ (kh * kh).transpose(-1, -2)) * scale + 2 * EPS32 * s.abs()
    mx = s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    p = e / e.sum(-1, keepdim=True)
    rel = 2 * ds + (2 * (s - mx).abs() + 8 + 8 * math.sqrt(L) * e.norm(dim=-1, keepdim=True) / e.sum(-1, keepdim=True)) * EPS32
    va = vh.abs()
    if rounded_probs:
        pr = round16(p)
        up, dn = ulp16(pr), ulp16(pr * (1 - 2.0 ** -12))
        dist = torch.minimum((p - (pr + up / 2)).abs(), (p - (pr - dn / 2)).abs())
        flip = (dist <= rel * p).double() * ulp16(p)
        o = pr @ vh
        sl = gemm_slack(L, (pr * pr) @ (vh * vh)) + flip @ va
    else:
        o = p @ vh
        sl = gemm_slack(L, (p * p) @ (vh * vh)) + (rel * p) @ va
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, L, E)
    return back(o), back(sl), p


def _mha_launch(qk_flat, off, v, B, M, L):
    """emrt_mha_fwd through the C ABI; q starts `off` elements into qk_flat (off = 4: a pointer that is only 8-byte aligned)"""
    c = ctx()
    E = M * 32
    out = torch.full((B, L, E), float("nan"), dtype=HALF, device="cuda")
    probs = torch.zeros(B, M, L, L, dtype=torch.float32, device="cuda")
    path = ctypes.c_int(-1)
    q_ptr = qk_flat.data_ptr() + 2 * off
    _lib.lib().call("emrt_mha_fwd", ctypes.c_void_p(q_ptr), 2 * E, ctypes.c_void_p(q_ptr + 2 * E), 2 * E, P(v), E, P(out), E, P(probs), B, M, L, 32,
                    1.0 / math.sqrt(32.0), 0.0, c.seed_ptr, 0, ctypes.pointer(path), F16, c.stream)
    torch.cuda.synchronize()
    return out, path.value


@pytest.mark.parametrize("peaked", [False, True], ids=["ordinary", "peaked"])
@pytest.mark.parametrize("L", [2, 16, 17, 37, 110, 128])
def test_mha_fwd_both_kernels(L, peaked):
    """MFMA kernel (v_mfma_f32_16x16x32_f16, path 1) and VALU kernel (path 0, by the mha_valu knob and by an 8-byte aligned q) against their
    float64 references.  peaked: q, k scaled so that the scores have a standard deviation of ~5 and most probabilities of a long row fall below
    2^-14 -- subnormal or zero once packed to float16."""
    _init()
    B, M = 3, 4
    E = M * 32
    g = _gen(100 + L)
    amp = math.sqrt(5.0) if peaked else 1.0
    qk = _rh(torch.randn(B, L, 2 * E, generator=g) * amp)
    v = _rh(torch.randn(B, L, E, generator=g))
    q, k = qk[..., :E], qk[..., E:]
    flat = torch.zeros(B * L * 2 * E + 8, dtype=HALF, device="cuda")
    flat[:B * L * 2 * E] = _d(qk).reshape(-1)
    vd = _d(v)
    want_m, sl_m, p = _mha_ref(q, k, v, M, True)
    want_v, sl_v, _ = _mha_ref(q, k, v, M, False)
    if peaked and L >= 110:
        assert (p < 2.0 ** -14).double().mean().item() > 0.5
    tag = "mha L%d %s" % (L, "peaked" if peaked else "ordinary")
    out_m, path = _mha_launch(flat, 0, vd, B, M, L)
    assert path == 1, path                                   # attn.hip: 16-bit dtype, knob off, L >= 2, aligned operands
    close_f16(tag + " mfma", out_m, want_m, sl_m)
    with _knobs(mha_valu=1):
        out_v, path = _mha_launch(flat, 0, vd, B, M, L)
    assert path == 0, path
    close_f16(tag + " valu", out_v, want_v, sl_v)
    # the two kernels agree within the sum of their bounds (their references differ by the contract's rounding of the probabilities)
    lim = ulp16(want_m) / 2 + sl_m + ulp16(want_v) / 2 + sl_v + (want_m - want_v).abs()
    assert bool(((out_m.double().cpu() - out_v.double().cpu()).abs() <= lim).all())
    # q (and k, 2 E elements further) 8 bytes off a 16-byte boundary: the dispatcher must take the VALU kernel, same numbers
    flat2 = torch.zeros_like(flat)
    flat2[4:4 + B * L * 2 * E] = flat[:B * L * 2 * E]
    out_u, path = _mha_launch(flat2, 4, vd, B, M, L)
    assert path == 0, path
    assert torch.equal(out_u, out_v)


def test_mha_fwd_rounds_to_nearest():
    _init()
    B, M, L = 8, 8, 128
    E = M * 32
    g = _gen(140)
    qk = _rh(torch.randn(B, L, 2 * E, generator=g) * 1.5)
    v = _rh(torch.randn(B, L, E, generator=g))
    flat, vd = _d(qk).reshape(-1), _d(v)
    want_m, sl_m, _ = _mha_ref(qk[..., :E], qk[..., E:], v, M, True)
    out, path = _mha_launch(flat, 0, vd, B, M, L)
    assert path == 1
    close_f16("mha rounding mfma", out, want_m, sl_m)
    rounding_is_nearest("mha mfma", out, want_m)
    want_v, sl_v, _ = _mha_ref(qk[..., :E], qk[..., E:], v, M, False)
    with _knobs(mha_valu=1):
        out, path = _mha_launch(flat, 0, vd, B, M, L)
    assert path == 0
    close_f16("mha rounding valu", out, want_v, sl_v)
    rounding_is_nearest("mha valu", out, want_v)


from tests.msda_reference import forward_with_slack as _msda_ref64          # noqa: E402  (this project's float64 forward, kept beside the backward)


def test_msda_fwd_small():
    """emrt_msda_fwd, both kernels (LDS-staged and global: bit-identical), against the explicit float64 reference above -- itself checked
    against the oracle's core function (grid_sample) with unrounded weights"""
    from tests.test_gpu_kernels import _msda_ref
    _init()
    g = _gen(150)
    M, shapes, Pn, B = 8, [(8, 8), (4, 4), (2, 2)], 4, 2
    L = len(shapes)
    Lv = sum(h * w for h, w in shapes)
    tp = M * L * Pn
    value = _rh(torch.randn(B, Lv, M * 32, generator=g))
    offw = torch.cat([torch.randn(B, Lv, 2 * tp, generator=g) * 1.5, torch.randn(B, Lv, tp, generator=g)], -1)
    ref = torch.rand(1, Lv, 1, 2, generator=g)
    oracle = _msda_ref(value, offw.double(), ref.double(), shapes, M, L, Pn).double().reshape(B, Lv, M * 32)
    plain, _ = _msda_ref64(value, offw.double(), ref.double(), shapes, M, Pn, False)
    assert (plain - oracle).abs().max().item() < 1e-9
    want, sl = _msda_ref64(value, offw.double(), ref.double(), shapes, M, Pn, True)
    vd, od, rd = _d(value), _d(offw, torch.float32), _d(ref, torch.float32)
    y = Fn.msda(vd, od, rd, shapes, M, Pn)
    torch.cuda.synchronize()
    with _knobs(msda_fwd_global=1):
        y2 = Fn.msda(vd, od, rd, shapes, M, Pn)
        torch.cuda.synchronize()
    assert torch.equal(y, y2)
    close_f16("msda fwd", y, want, sl)


# =====================================================================================================================================
# normalisation
# =====================================================================================================================================
def _norm_ref(z, gamma, beta, eps, dim):
    """float64 (z - mean) * rstd * gamma + beta over `dim` (biased variance, eps as the fp32 value the kernel adds) and the slack of an fp32
    implementation, derived:
      * mean: a sum of n terms, error 8 sqrt(n) 2^-24 sqrt(sum z^2) / n = 8 * 2^-24 * rms(z)            (gemm_slack of the averaging operator)
      * variance: the same on d^2 = (z - mean)^2, relative to the variance: 8 * 2^-24 * rms(d^2) / mean(d^2); rstd moves by half of that
        relative, plus rsqrtf (2 ulp) and the division by n (1 ulp)
      * out = (d * rstd) * gamma + beta: three more roundings on |xhat gamma|, one on |out|
    -> |xhat gamma| (4 kurt + 8) 2^-24 + 8 * 2^-24 rms(z) rstd |gamma| + 2 * 2^-24 (|out| + |beta|).  With mean >> std the second term
    dominates (the fp32 mean is only known to ~rms(z) 2^-21): that is the arithmetic, not a tolerance."""
    n = 1
    for d_ in (dim if isinstance(dim, tuple) else (dim,)):
        n *= z.shape[d_]
    mu = z.mean(dim, keepdim=True)
    d = z - mu
    var = (d * d).mean(dim, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    xg = d * rstd * gamma
    out = xg + beta
    rms = (z * z).mean(dim, keepdim=True).sqrt()
    kurt = torch.where(var > 0, (d ** 4).mean(dim, keepdim=True).sqrt() / var.clamp_min(1e-300), torch.zeros_like(var))
    sl = xg.abs() * (4 * kurt + 8) * EPS32 + 8 * EPS32 * rms * rstd * gamma.abs() + 2 * EPS32 * (out.abs() + beta.abs())
    return out, sl, rstd


def _ln_launch(a, b, post, with_z, gamma, beta, qpos):
    c = ctx()
    rows, C = a.numel() // a.shape[-1], a.shape[-1]
    out = torch.full(tuple(a.shape), float("nan"), dtype=HALF, device="cuda")
    z = torch.full(tuple(a.shape), float("nan"), dtype=HALF, device="cuda") if with_z else None
    q = torch.full(tuple(a.shape), float("nan"), dtype=HALF, device="cuda") if qpos is not None else None
    _lib.lib().call("emrt_layernorm_fwd", P(a), P(b), P(post), P(z), P(out), P(gamma), P(beta), None, None, rows, C, 1e-5, 0.0, None, 0,
                    P(qpos), (qpos.numel() // C) if qpos is not None else 0, P(q), F16, c.stream)
    torch.cuda.synchronize()
    return out, z, q


@pytest.mark.parametrize("with_z", [False, True], ids=["no-z", "z-buffer"])
@pytest.mark.parametrize("case", [
    dict(name="a-only", rows=(1, 5), C=256, b=False, post=False, qpos=0),                   # 5 rows: not a multiple of the block's 4
    dict(name="a+b", rows=(3, 113), C=256, b=True, post=False, qpos=0),
    dict(name="a+b+post", rows=(2, 37), C=256, b=True, post=True, qpos=0),
    dict(name="a+b+qpos", rows=(3, 110), C=256, b=True, post=False, qpos=110),              # qpos_rows < rows: broadcast over the batch
    dict(name="a+b+post+qpos", rows=(2, 7), C=64, b=True, post=True, qpos=7),
    dict(name="C1024", rows=(1, 6), C=1024, b=True, post=False, qpos=0),
    dict(name="mean>>std", rows=(2, 9), C=256, b=True, post=False, qpos=0, mean=200.0, std=0.5),
    dict(name="constant-rows", rows=(1, 6), C=256, b=True, post=True, qpos=6, const=True),
], ids=lambda c_: c_["name"])
def test_layernorm_fwd(case, with_z):
    """emrt_layernorm_fwd through the C ABI.  With a z buffer the kernel rounds z = a + b to float16 before the statistics (the stored z is
    the backward's input) and the reference does the same; without one (inference) z stays in fp32 and the reference keeps the exact sum --
    the two differ by one rounding of a + b.  q_out = round16(out) + pos (norm.hip: `to_f32(from_f32<T>(o[e]))`): checked against the OUT the
    kernel stored, so a q built from the unrounded out is off by up to an ulp and fails."""
    _init()
    g = _gen(200)
    B, Lr = case["rows"]
    C = case["C"]
    if case.get("const"):
        a = _rh(torch.randn(B, Lr, 1, generator=g).expand(B, Lr, C).contiguous() * 3)
        b = _rh(torch.randn(B, Lr, 1, generator=g).expand(B, Lr, C).contiguous())
    else:
        a = _rh(torch.randn(B, Lr, C, generator=g) * case.get("std", 1.0) + case.get("mean", 0.0))
        b = _rh(torch.randn(B, Lr, C, generator=g) * case.get("std", 1.0)) if case["b"] else None
    post = _rh(torch.randn(B, Lr, C, generator=g)) if case["post"] else None
    qpos = _rh(torch.randn(case["qpos"], C, generator=g)) if case["qpos"] else None
    gamma, beta = (torch.rand(C, generator=g) + 0.5).double(), (torch.randn(C, generator=g) * 0.3).double()
    z = a + b if b is not None else a
    zsl = torch.zeros_like(z)
    if with_z and b is not None:
        z = round16(z)
    elif b is not None:
        zsl = EPS32 * z.abs()                     # a + b in fp32: not always exact (exponents up to 2^39 apart)
    ln, sl, rstd = _norm_ref(z, gamma, beta, 1e-5, -1)
    sl = sl + zsl * rstd * gamma.abs()
    want = ln
    if post is not None:
        want = ln + post
        sl = sl + terms_slack(ln, post)
    out, zd, qd = _ln_launch(_d(a), _d(b) if b is not None else None, _d(post) if post is not None else None, with_z,
                             _d(gamma, torch.float32), _d(beta, torch.float32), _d(qpos) if qpos is not None else None)
    tag = "ln %s %s" % (case["name"], "z" if with_z else "no-z")
    close_f16(tag, out, want, sl)
    if with_z and b is not None:
        assert torch.equal(zd.cpu(), z.half())               # the stored z IS the rounded sum, bit for bit
    if qpos is not None:
        stored = out.double().cpu()
        qref = stored + qpos.repeat(B, 1).reshape(B, Lr, C)
        close_f16(tag + " q_out", qd, qref, EPS32 * qref.abs())          # one fp32 add of two float16 values


def test_layernorm_fwd_rounds_to_nearest():
    _init()
    g = _gen(201)
    B, Lr, C = 6, 110, 256
    a, b = _rh(torch.randn(B, Lr, C, generator=g)), _rh(torch.randn(B, Lr, C, generator=g))
    qpos = _rh(torch.randn(Lr, C, generator=g))
    gamma, beta = (torch.rand(C, generator=g) + 0.5).double(), (torch.randn(C, generator=g) * 0.3).double()
    ln, sl, rstd = _norm_ref(a + b, gamma, beta, 1e-5, -1)
    sl = sl + EPS32 * (a + b).abs() * rstd * gamma.abs()
    out, _, qd = _ln_launch(_d(a), _d(b), None, False, _d(gamma, torch.float32), _d(beta, torch.float32), _d(qpos))
    close_f16("ln rounding", out, ln, sl)
    rounding_is_nearest("layernorm out", out, ln)
    qref = out.double().cpu() + qpos
    close_f16("ln rounding q_out", qd, qref, EPS32 * qref.abs())
    rounding_is_nearest("layernorm q_out", qd, qref)


def _gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def _gn_ref(x, G, gamma, beta, gelu, res):
    """x [N, HW, C] float64 -> GroupNorm over (HW, C / G) per (n, group), [gelu], [+ res]; checked against F.group_norm in float64.
    gelu(u) = u/2 (1 + erff(u / sqrt 2)): erff is good to a few ulp of ITS value, i.e. an absolute 4 * 2^-24 on (1 + erf) where that sum
    cancels (u << 0), so the slack gets |u| / 2 * 8 * 2^-24 next to |gelu'| <= 1.13 times u's slack and two roundings of the product."""
    N, HW, C = x.shape
    xg = x.reshape(N, HW, G, C // G)
    u, sl, _ = _norm_ref(xg, gamma.reshape(1, 1, G, C // G), beta.reshape(1, 1, G, C // G), 1e-5, (1, 3))
    u, sl = u.reshape(N, HW, C), sl.reshape(N, HW, C)
    chk = F.group_norm(x.transpose(1, 2), G, gamma, beta, float(torch.tensor(1e-5, dtype=torch.float32))).transpose(1, 2)
    assert (chk - u).abs().max().item() < 1e-9
    if gelu:
        y = _gelu64(u)
        sl = 1.13 * sl + 4 * EPS32 * u.abs() + 2 * EPS32 * y.abs()
        u = y
    if res is not None:
        sl = sl + terms_slack(u, res)
        u = u + res
    return u, sl


@pytest.mark.parametrize("case", [
    dict(name="fused", N=2, H=16, W=16, C=256, G=32, gelu=True, res=True),                  # gn_use_fused: HW <= 4096, C / G a multiple of 4
    dict(name="fused-plain", N=3, H=5, W=7, C=128, G=8, gelu=False, res=False),
    dict(name="two-pass-big-map", N=1, H=72, W=72, C=64, G=8, gelu=True, res=True),         # HW = 5184 > 4096: fp64 statistics + apply
    dict(name="two-pass-wide-groups", N=2, H=6, W=5, C=1024, G=2, gelu=False, res=True),    # (C / G) / 4 = 128 > 64 lanes: not fused either
], ids=lambda c_: c_["name"])
def test_groupnorm_fwd_single_level(case):
    """emrt_groupnorm_fwd on both sides of gn_use_fused(HW, C, G), input / residual / output as channel slices of wider buffers, and one group
    whose values are all equal (variance 0: the output is beta there)"""
    c = _init()
    g = _gen(210)
    N, H, W, C, G = case["N"], case["H"], case["W"], case["C"], case["G"]
    x = torch.randn(N, H * W, C, generator=g) * 1.5 + 0.3
    x[0, :, :C // G] = 1.25                                    # group 0 of image 0: constant
    x = _rh(x)
    res = _rh(torch.randn(N, H * W, C, generator=g)) if case["res"] else None
    gamma, beta = (torch.rand(C, generator=g) + 0.5).double(), (torch.randn(C, generator=g) * 0.3).double()
    want, sl = _gn_ref(x, G, gamma, beta, case["gelu"], res)
    wide = torch.zeros(N, H, W, C + 8, dtype=HALF, device="cuda")
    wide[..., 8:] = _d(x).reshape(N, H, W, C)
    rwide = None
    if res is not None:
        rwide = torch.zeros(N, H, W, 2 * C, dtype=HALF, device="cuda")
        rwide[..., :C] = _d(res).reshape(N, H, W, C)
    owide = torch.full((N, H, W, C + 16), 3.0, dtype=HALF, device="cuda")
    Fn.group_norm(wide[..., 8:], _d(gamma, torch.float32), _d(beta, torch.float32), None, None, G, 1e-5, case["gelu"],
                  rwide[..., :C] if res is not None else None, owide[..., 16:])
    torch.cuda.synchronize()
    close_f16("gn " + case["name"], owide[..., 16:].reshape(N, H * W, C), want, sl)
    assert float((owide[..., :16].float() - 3.0).abs().max()) == 0.0


@pytest.mark.parametrize("group_blocks", [0, 1])
@pytest.mark.parametrize("gelu,with_res", [(True, True), (False, False)])
def test_groupnorm_levels_fwd(group_blocks, gelu, with_res):
    """emrt_groupnorm_levels_fwd (row-major statistics + apply pair, and the one-block-per-(image, group) kernel behind gn_group_blocks) on a
    ragged level set, as strided views of wider token buffers, against float64 GroupNorm per level"""
    c = _init()
    g = _gen(220)
    B, hws, C, G, pad = 2, (240, 60, 15, 1), 256, 32, 8
    L, Lv = len(hws), sum(hws)
    x = torch.randn(B, Lv, C, generator=g) * 1.5 + 0.3
    x[1, 240:300, 8:16] = -0.75                                # one whole (image, level, group) constant
    x = _rh(x)
    res = _rh(torch.randn(B, Lv, C, generator=g)) if with_res else None
    gam = [(torch.rand(C, generator=g) + 0.5).double() for _ in range(L)]
    bet = [(torch.randn(C, generator=g) * 0.2).double() for _ in range(L)]
    wants, sls, s0 = [], [], 0
    for l, n in enumerate(hws):
        w_, s_ = _gn_ref(x[:, s0:s0 + n], G, gam[l], bet[l], gelu, res[:, s0:s0 + n] if with_res else None)
        wants.append(w_)
        sls.append(s_)
        s0 += n
    want, sl = torch.cat(wants, 1), torch.cat(sls, 1)
    ld = C + pad
    xw = torch.zeros(B, Lv, ld, dtype=HALF, device="cuda")
    xw[..., :C] = _d(x)
    rw = None
    if with_res:
        rw = torch.zeros(B, Lv, ld, dtype=HALF, device="cuda")
        rw[..., :C] = _d(res)
    ow = torch.full((B, Lv, ld), 3.0, dtype=HALF, device="cuda")
    gd, bd = [_d(t, torch.float32) for t in gam], [_d(t, torch.float32) for t in bet]
    arr = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
    starts = (ctypes.c_int * L)(*[sum(hws[:l]) for l in range(L)])
    hw = (ctypes.c_int * L)(*hws)
    mean, rstd = torch.empty(L * B * G, device="cuda"), torch.empty(L * B * G, device="cuda")
    ws = torch.zeros(L * B * G * 2, dtype=torch.float64, device="cuda")
    with _knobs(gn_group_blocks=group_blocks):
        _lib.lib().call("emrt_groupnorm_levels_fwd", P(xw), ld, Lv * ld, P(rw), ld if with_res else 0, Lv * ld if with_res else 0, P(ow), ld, Lv * ld,
                        arr(gd), arr(bd), P(mean), P(rstd), starts, hw, L, B, C, G, 1e-5, int(gelu), P(ws), F16, c.stream)
        torch.cuda.synchronize()
    close_f16("gn levels blocks=%d gelu=%d" % (group_blocks, gelu), ow[..., :C], want, sl)
    assert float((ow[..., C:].float() - 3.0).abs().max()) == 0.0


def test_bn_apply_eval():
    """emrt_bn_apply with sums == null (running statistics): relu, residual, sliced output, running variances down to 1e-6.
    Kernel: scale = rsqrtf(var + eps) * gamma, shift = fma(-mean, scale, beta), y = fma(x, scale, shift) (+ res): each of x * scale,
    mean * scale carries the few ulp of `scale` (terms_slack's margin of 8 covers add, rsqrtf, multiply), beta and res one rounding."""
    c = _init()
    g = _gen(230)
    N, H, W, C = 2, 9, 8, 256
    M = N * H * W
    x = _rh(torch.randn(M, C, generator=g) * 2 + 0.5)
    rm = (torch.randn(C, generator=g) * 0.3).double()
    rv = (torch.rand(C, generator=g) + 0.5).double()
    rv[::5] = torch.tensor(10.0, dtype=torch.float64) ** (-6 * torch.rand(C, generator=g).double()[::5])       # 1 .. 1e-6
    rv[3] = float(torch.tensor(1e-6, dtype=torch.float32))
    rv = rv.float().double()
    gam, bet = (torch.rand(C, generator=g) + 0.5).double(), torch.randn(C, generator=g).double()
    res = _rh(torch.randn(M, C, generator=g))
    scale = gam / torch.sqrt(rv + float(torch.tensor(1e-5, dtype=torch.float32)))
    xd, resd, rmd, rvd, gamd, betd = _d(x), _d(res), _d(rm, torch.float32), _d(rv, torch.float32), _d(gam, torch.float32), _d(bet, torch.float32)
    for relu, with_res in ((True, True), (True, False), (False, True)):
        want = x * scale + (bet - rm * scale)
        sl = terms_slack(x * scale, rm * scale, bet.expand_as(x), want)
        if with_res:
            sl = sl + terms_slack(want, res)
            want = want + res
        if relu:
            want = want.clamp_min(0)
        cat = torch.full((M, 3 * C), 5.0, dtype=HALF, device="cuda")
        _lib.lib().call("emrt_bn_apply", P(xd), C, P(resd) if with_res else None, C if with_res else 0, P(cat[:, C:2 * C]), 3 * C, None, 1.0, 1e-5, 0.9,
                        None, None, P(rmd), P(rvd), P(gamd), P(betd), M, C, int(relu), F16, c.stream)
        torch.cuda.synchronize()
        close_f16("bn eval relu=%d res=%d" % (relu, with_res), cat[:, C:2 * C], want, sl)
        assert float((cat[:, :C].float() - 5.0).abs().max()) == 0.0 and float((cat[:, 2 * C:].float() - 5.0).abs().max()) == 0.0


# =====================================================================================================================================
# spatial
# =====================================================================================================================================
def _axis64(n_in, n_out, align):
    """float64 (i0, i1, l1) per destination index, the formulas of csrc/spatial.hip (make_axis / axis_src)"""
    d = torch.arange(n_out, dtype=torch.float64)
    if align:
        src = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        src = ((d + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, src - i0


def _resize_ref(x, OH, OW, align):
    """x [N, IH, IW, C] float64 -> bilinear [N, OH, OW, C] and its slack; checked against F.interpolate in float64.
    The kernel computes source coordinates in fp32 (scale = in / out rounded once, one multiply, one add): a coordinate up to `in` carries
    up to 4 * 2^-24 * in of error, which moves the output by that times the slope between the taps -- the derived term dl * (|do/dly| +
    |do/dlx|) -- next to terms_slack over the four weighted taps (two roundings each, covered by its margin)."""
    N, IH, IW, C = x.shape
    y0, y1, ly = _axis64(IH, OH, align)
    x0, x1, lx = _axis64(IW, OW, align)
    ly, lx = ly.reshape(1, OH, 1, 1), lx.reshape(1, 1, OW, 1)
    v00, v01, v10, v11 = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    top, bot = (1 - lx) * v00 + lx * v01, (1 - lx) * v10 + lx * v11
    out = (1 - ly) * top + ly * bot
    chk = F.interpolate(x.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
    assert (chk - out).abs().max().item() < 1e-9
    # the slope the coordinate error multiplies: a sample at (or within that error of) a source pixel may fall into either of the two
    # segments that meet there -- floor() of the fp32 coordinate need not be floor() of the float64 one -- so take the steeper of the two
    rowx = lambda yi: (1 - lx) * x[:, yi][:, :, x0] + lx * x[:, yi][:, :, x1]
    coly = lambda xi: (1 - ly) * x[:, y0][:, :, xi] + ly * x[:, y1][:, :, xi]
    ym, yp, xm, xp = (y0 - 1).clamp_min(0), (y0 + 1).clamp_max(IH - 1), (x0 - 1).clamp_min(0), (x0 + 1).clamp_max(IW - 1)
    dly = torch.maximum((rowx(yp) - rowx(y0)).abs(), (rowx(y0) - rowx(ym)).abs())
    dlx = torch.maximum((coly(xp) - coly(x0)).abs(), (coly(x0) - coly(xm)).abs())
    sl = terms_slack((1 - ly) * (1 - lx) * v00, (1 - ly) * lx * v01, ly * (1 - lx) * v10, ly * lx * v11) + 4 * EPS32 * (IH * dly + IW * dlx)
    return out, sl


@pytest.mark.parametrize("case", [
    dict(name="up-align", N=2, IH=8, IW=8, C=64, OH=16, OW=16, align=True),
    dict(name="up-noalign", N=2, IH=8, IW=8, C=64, OH=16, OW=16, align=False),
    dict(name="up-ragged-c6", N=1, IH=7, IW=9, C=6, OH=20, OW=31, align=False),            # scalar path
    dict(name="down-align", N=2, IH=32, IW=32, C=32, OH=12, OW=20, align=True),
    dict(name="down-noalign", N=2, IH=33, IW=17, C=16, OH=8, OW=8, align=False),
    dict(name="1x1-source", N=2, IH=1, IW=1, C=64, OH=8, OW=8, align=True),
    dict(name="add", N=2, IH=8, IW=8, C=256, OH=16, OW=16, align=False, add=True),
    dict(name="add-align-view", N=2, IH=4, IW=4, C=64, OH=8, OW=8, align=True, add=True, view=True),
    dict(name="view", N=2, IH=3, IW=3, C=256, OH=32, OW=32, align=True, view=True),
], ids=lambda c_: c_["name"])
def test_resize_bilinear_fwd(case):
    c = _init()
    g = _gen(300)
    N, IH, IW, C, OH, OW, align = (case[k] for k in ("N", "IH", "IW", "C", "OH", "OW", "align"))
    x = _rh(torch.randn(N, IH, IW, C, generator=g) * 2)
    add = _rh(torch.randn(N, OH, OW, C, generator=g)) if case.get("add") else None
    want, sl = _resize_ref(x, OH, OW, align)
    if add is not None:
        sl = sl + terms_slack(want, add)
        want = want + add
    view = case.get("view")
    xw = torch.zeros(N, IH, IW, C + (8 if view else 0), dtype=HALF, device="cuda")
    xw[..., :C] = _d(x)
    ow = torch.full((N, OH, OW, C + (24 if view else 0)), 3.0, dtype=HALF, device="cuda")
    aw = None
    if add is not None:
        aw = torch.zeros(N, OH, OW, C + (16 if view else 0), dtype=HALF, device="cuda")
        aw[..., -C:] = _d(add)
    ov = ow[..., 8:8 + C] if view else ow
    Fn.resize_bilinear(xw[..., :C], OH, OW, align, add_t=aw[..., -C:] if add is not None else None, out=ov)
    torch.cuda.synchronize()
    close_f16("resize " + case["name"], ov, want, sl)
    if view:
        assert float((ow[..., :8].float() - 3.0).abs().max()) == 0.0 and float((ow[..., 8 + C:].float() - 3.0).abs().max()) == 0.0


def test_resize_bilinear_to_nchw_f32_and_rounding():
    """out_nchw_f32 (the logits path): fp32 [N, C, OH, OW], no float16 rounding at all (bound: ulp32 / 2 + slack); and the direction of the
    float16 rounding on a large map"""
    _init()
    g = _gen(301)
    x = _rh(torch.randn(2, 16, 16, 6, generator=g) * 3)
    for align in (False, True):
        want, sl = _resize_ref(x, 64, 64, align)
        y = Fn.resize_bilinear(_d(x), 64, 64, align, out_nchw_f32=True)
        torch.cuda.synchronize()
        assert y.dtype == torch.float32 and tuple(y.shape) == (2, 6, 64, 64)
        close_f16("resize nchw f32 align=%d" % align, y.permute(0, 2, 3, 1), want, sl, out_f32=True)
    x = _rh(torch.randn(2, 24, 24, 32, generator=g) * 2)
    want, sl = _resize_ref(x, 64, 64, False)
    y = Fn.resize_bilinear(_d(x), 64, 64, False)
    torch.cuda.synchronize()
    close_f16("resize rounding", y, want, sl)
    rounding_is_nearest("resize_bilinear", y, want)


@pytest.mark.parametrize("grouped", [1, 0])
def test_pyramid_tokens_to_maps(grouped):
    """emrt_pyramid_resize_fwd (all scales in one launch) and the per-scale emrt_resize_bilinear_fwd launches on token-slab views: each k x k
    token map resized (align_corners) into a channel slice of the concat buffer"""
    c = _init()
    g = _gen(310)
    B, C, OH, OW, scales = 2, 64, 24, 40, (1, 3, 6, 8)
    ntok = sum(k * k for k in scales)
    tok = _rh(torch.randn(B, ntok, C, generator=g) * 2)
    cat = torch.full((B, OH, OW, (len(scales) + 1) * C), 3.0, dtype=HALF, device="cuda")
    outs = [cat[..., (i + 1) * C:(i + 2) * C] for i in range(len(scales))]
    old = c.pyramid_group
    c.pyramid_group = bool(grouped)
    try:
        L_ = _lib.lib()
        L_.start_record()
        Fn.pyramid_tokens_to_maps(_d(tok), scales, OH, OW, outs)
        names = [n for n, _ in L_.stop_record()]
    finally:
        c.pyramid_group = old
    torch.cuda.synchronize()
    assert names == (["emrt_pyramid_resize_fwd"] if grouped else ["emrt_resize_bilinear_fwd"] * len(scales)), names
    s0 = 0
    for k, o in zip(scales, outs):
        want, sl = _resize_ref(tok[:, s0:s0 + k * k].reshape(B, k, k, C), OH, OW, True)
        close_f16("pyramid k=%d grouped=%d" % (k, grouped), o, want, sl)
        s0 += k * k
    assert float((cat[..., :C].float() - 3.0).abs().max()) == 0.0


def test_adaptive_avgpool_tokens_uneven_bins():
    """21 x 30 map, scales 1 / 2 / 3 / 6: bins of unequal size (floor / ceil edges) against float64 adaptive_avg_pool2d.  A bin of n pixels
    is a sum of n terms times 1 / n: gemm_slack(n, sum of squares) / n, and one rounding of the division."""
    _init()
    g = _gen(320)
    N, H, W, C, scales = 2, 21, 30, 64, (1, 2, 3, 6)
    x = _rh(torch.randn(N, H, W, C, generator=g) + 0.5)
    wide = torch.zeros(N, H, W, C + 8, dtype=HALF, device="cuda")
    wide[..., 8:] = _d(x)
    y = Fn.adaptive_avgpool_tokens(wide[..., 8:], scales)
    torch.cuda.synchronize()
    xc = x.permute(0, 3, 1, 2)
    tok = lambda m, k: m.permute(0, 2, 3, 1).reshape(N, k * k, C)
    wants = [tok(F.adaptive_avg_pool2d(xc, k), k) for k in scales]
    # gemm_slack(n, sum sq) / n = 8 sqrt(n) 2^-24 sqrt(n * mean sq) / n = 8 * 2^-24 * sqrt(mean sq): independent of the bin's size
    sls = [8 * EPS32 * tok(F.adaptive_avg_pool2d(xc * xc, k), k).sqrt() + 2 * EPS32 * w_.abs() for k, w_ in zip(scales, wants)]
    close_f16("adaptive avgpool", y, torch.cat(wants, 1), torch.cat(sls, 1))


def test_maxpool_fwd_ties_and_negative_windows():
    """3x3 / stride 2 / pad 1: the result is one of the inputs, so the comparison is exact (slack 0, and 0 <= ulp / 2 + 0 means equal up to
    nothing: asserted with torch.equal).  Ties (quantised values) and all-negative maps: the zero padding must not win."""
    _init()
    g = _gen(330)
    for C in (64, 20):                                         # vec8 kernel / element kernel
        for name, x in (("ties", torch.randint(-3, 4, (2, 13, 17, C), generator=g).float() * 0.5),
                        ("negative", -torch.rand(2, 12, 12, C, generator=g) - 0.25),
                        ("random", torch.randn(2, 9, 16, C, generator=g))):
            x = _rh(x)
            want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
            y = Fn.maxpool(_d(x))
            torch.cuda.synchronize()
            close_f16("maxpool %s C%d" % (name, C), y, want, 0.0)
            assert torch.equal(y.double().cpu(), want), name
            if name == "negative":
                assert float(y.float().max()) < 0.0


def test_nchw_to_nhwc_ingest():
    """fp32 NCHW image -> float16 NHWC, channels padded to c_out (8: the stem's vector path; 4; 5: element kernel): one rounding, exact bits"""
    _init()
    g = _gen(340)
    img = torch.randn(2, 3, 16, 24, generator=g) * 3
    img[0, 0, 0, :6] = torch.tensor([65504.0, 65519.9, 65520.0, -1e6, 3e-8, 2.0 ** -25])       # largest finite, just below / at overflow, subnormal, tie to zero
    want = img.permute(0, 2, 3, 1).half()
    for co in (None, 8, 4, 5):
        y = Fn.nchw_to_nhwc(img.cuda(), c_out=co)
        torch.cuda.synchronize()
        assert y.dtype == HALF and tuple(y.shape) == (2, 16, 24, co or 3)
        assert torch.equal(y[..., :3].cpu().view(torch.int16), want.view(torch.int16)), co
        if co:
            assert float(y[..., 3:].float().abs().max()) == 0.0
    close_f16("nchw_to_nhwc", Fn.nchw_to_nhwc(img.cuda(), c_out=8)[..., :3], img.permute(0, 2, 3, 1).double(), 0.0)


# =====================================================================================================================================
# elementwise
# =====================================================================================================================================
def test_add_and_add3d_and_acc3d():
    """one fp32 add of two float16 values then one rounding: slack = 2^-24 |a + b| (the fp32 sum of two float16 values is not always exact)"""
    c = _init()
    g = _gen(400)
    a, b = _rh(torch.randn(2, 21, 64, generator=g) * 4), _rh(torch.randn(21, 64, generator=g))
    a[0, 0, :4] = torch.tensor([65504.0, -65504.0, 40000.0, 6e-5]).half().double()
    b[0, :4] = torch.tensor([32.0, -16.0, 30000.0, -5.9e-5]).half().double()
    want = a + b
    close_f16("add period", Fn.add(_d(a), _d(b), period=21 * 64), want, EPS32 * want.abs())
    b2 = _rh(torch.randn(2, 21, 64, generator=g))
    close_f16("add same shape", Fn.add(_d(a), _d(b2)), a + b2, EPS32 * (a + b2).abs())
    # add3d: a level slab of a token tensor + a channel slice, dense result
    tok = _rh(torch.randn(2, 50, 64, generator=g))
    wide = _rh(torch.randn(2, 4, 5, 192, generator=g))
    tokd, wided = _d(tok), _d(wide)
    y = Fn.add_maps(Fn.tokens_as_map(tokd[:, 7:27], 4, 5), wided[..., 64:128])
    want = tok[:, 7:27].reshape(2, 4, 5, 64) + wide[..., 64:128]
    close_f16("add3d views", y, want, EPS32 * want.abs())
    # acc3d: dst += src into a slab and into a channel slice
    base = _rh(torch.randn(2, 21, 64, generator=g))
    src = _rh(torch.randn(2, 16, 64, generator=g))
    based = _d(base)
    Fn.add_into(based.narrow(1, 5, 16), _d(src))
    want = base.clone()
    want[:, 5:] += src
    close_f16("acc3d slab", based, want, EPS32 * want.abs())
    cat = _rh(torch.randn(2, 4, 4, 192, generator=g))
    part = _rh(torch.randn(2, 4, 4, 64, generator=g))
    catd = _d(cat)
    Fn.add_into(catd.narrow(3, 64, 64), _d(part))
    want = cat.clone()
    want[..., 64:128] += part
    torch.cuda.synchronize()
    close_f16("acc3d slice", catd, want, EPS32 * want.abs())


def test_add_f32row_and_levels():
    """a (float16) + an fp32 row broadcast over the rows (positional / level embeddings): the fp32 row is NOT rounded first"""
    c = _init()
    g = _gen(410)
    spans, C, Lv = [(0, 35), (35, 12), (47, 5), (52, 1)], 64, 53
    a = _rh(torch.randn(Lv, C, generator=g))
    rows = torch.randn(len(spans), C, generator=g) * 1.001
    ad, rd = _d(a), rows.cuda()
    one, per = torch.empty_like(ad), torch.empty_like(ad)
    L_ = _lib.lib()
    starts = (ctypes.c_int * len(spans))(*[s0 for s0, _ in spans])
    L_.call("emrt_add_f32row_levels", P(ad), P(rd), P(one), starts, len(spans), Lv, C, F16, c.stream)
    for l, (s0, n) in enumerate(spans):
        L_.call("emrt_add_f32row", P(ad[s0:s0 + n]), P(rd[l]), P(per[s0:s0 + n]), n * C, C, F16, c.stream)
    torch.cuda.synchronize()
    want = a + rows.double().repeat_interleave(torch.tensor([n for _, n in spans]), 0)
    close_f16("add_f32row_levels", one, want, EPS32 * want.abs())
    close_f16("add_f32row", per, want, EPS32 * want.abs())
    assert torch.equal(one, per)


def test_concat_tokens_and_split():
    c = _init()
    g = _gen(420)
    B, C = 3, 64
    parts = [_rh(torch.randn(B, n, C, generator=g)) for n in (1, 9, 36, 64)]
    pd = [_d(p_) for p_ in parts]
    y = Fn.concat_tokens(pd)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.cat(parts, 1).half())
    close_f16("concat_tokens", y, torch.cat(parts, 1), 0.0)
    # the split (the backward's direction, split = 1) is a forward-dtype entry point too
    ns = [p_.shape[1] for p_ in parts]
    back = [torch.full(tuple(p_.shape), float("nan"), dtype=HALF, device="cuda") for p_ in parts]
    _lib.lib().call("emrt_concat_tokens", (ctypes.c_void_p * 4)(*[t.data_ptr() for t in back]), (ctypes.c_int * 4)(*ns), 4, P(y), B, C, 1, F16, c.stream)
    torch.cuda.synchronize()
    for got, p_ in zip(back, pd):
        assert torch.equal(got, p_)


def test_cast_both_ways_bit_exact():
    """emrt_cast fp32 -> float16 (direction 0) against Tensor.half() and back (direction 1) against .float(), bit for bit: subnormals,
    +-65504, overflow, -0.0, ties, and 2^18 random values for the direction of the rounding"""
    c = _init()
    g = _gen(430)
    special = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 65519.99, 65520.0, -65520.0, 1e6, -1e6, 6.1e-5, 6.0e-5, 5.96e-8, 2.0 ** -25, 2.0 ** -25 * 1.0001,
                            -2.0 ** -25, 3e-8, 2.9e-8, 1e-10, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -11, 2049.0, 2051.0,
                            float("inf"), -float("inf")])
    x = torch.cat([special, torch.randn(1 << 18, generator=g) * 3, torch.randn(4096, generator=g) * 1e-5, torch.randn(4096, generator=g) * 3e4])
    xd = x.cuda()
    h = Fn.cast_from_f32(xd)
    torch.cuda.synchronize()
    assert h.dtype == HALF
    assert torch.equal(h.cpu().view(torch.int16), x.half().view(torch.int16))
    back = Fn.cast_to_f32(h)
    torch.cuda.synchronize()
    assert back.dtype == torch.float32 and torch.equal(back.cpu().view(torch.int32), x.half().float().view(torch.int32))
    fin = torch.isfinite(x)
    close_f16("cast f32 -> f16", h[fin.cuda()], x[fin].double(), 0.0)
    rounding_is_nearest("cast", h[len(special):len(special) + (1 << 18)], x[len(special):len(special) + (1 << 18)].double())


def test_pack_weights_decodes_to_half():
    """emrt_pack_weights with dtype 2: the forward operand [OC][KH][KW][C] and the transposed copy [C][KH][KW][OC] equal weight.half() bit for
    bit (weights NOT pre-rounded: the pack does the rounding), in the layouts test_pack_weights_layouts checks"""
    c = _init()
    g = _gen(440)
    conv = hnn.Conv2D(40, 72, 3, 1, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(72, 40, 3, 3, generator=g))
        conv.weight[0, 0, 0, :3] = torch.tensor([70000.0, 3e-8, -2.0 ** -25])
    w = conv.weight.detach().clone()
    h = Holder(conv=conv).place()
    torch.cuda.synchronize()
    base = h.store.packed.data_ptr()
    assert h.store.packed.dtype == HALF
    off = (conv.gw.fwd_ptr - base) // 2
    fwd = h.store.packed[off:off + w.numel()].cpu().view(72, 3, 3, 40)
    assert torch.equal(fwd.view(torch.int16), w.permute(0, 2, 3, 1).contiguous().half().view(torch.int16))
    assert conv.gw.bwd_ptr is not None
    off = (conv.gw.bwd_ptr - base) // 2
    bwd = h.store.packed[off:off + w.numel()].cpu().view(40, 3, 3, 72)
    assert torch.equal(bwd.view(torch.int16), w.permute(1, 2, 3, 0).contiguous().half().view(torch.int16))


# =====================================================================================================================================
# the ledger: which float16 entry point is tested where (tests/test_fp16_ledger_cpu.py checks it against csrc/*.hip and the header)
# =====================================================================================================================================
COVERED = {
    "emrt_conv2d": "test_conv2d_epilogues_and_geometries",
    "emrt_conv2d_group": "test_conv2d_group_unequal_problems",
    "emrt_gconv2d": "test_gconv2d_grouped_3x3",
    "emrt_mha_fwd": "test_mha_fwd_both_kernels",
    "emrt_msda_fwd": "test_msda_fwd_small",
    "emrt_layernorm_fwd": "test_layernorm_fwd",
    "emrt_groupnorm_fwd": "test_groupnorm_fwd_single_level",
    "emrt_groupnorm_levels_fwd": "test_groupnorm_levels_fwd",
    "emrt_bn_apply": "test_bn_apply_eval",
    "emrt_resize_bilinear_fwd": "test_resize_bilinear_fwd",
    "emrt_pyramid_resize_fwd": "test_pyramid_tokens_to_maps",
    "emrt_adaptive_avgpool_fwd": "test_adaptive_avgpool_tokens_uneven_bins",
    "emrt_maxpool_fwd": "test_maxpool_fwd_ties_and_negative_windows",
    "emrt_nchw_to_nhwc": "test_nchw_to_nhwc_ingest",
    "emrt_add": "test_add_and_add3d_and_acc3d",
    "emrt_add3d": "test_add_and_add3d_and_acc3d",
    "emrt_acc3d": "test_add_and_add3d_and_acc3d",
    "emrt_add_f32row": "test_add_f32row_and_levels",
    "emrt_add_f32row_levels": "test_add_f32row_and_levels",
    "emrt_concat_tokens": "test_concat_tokens_and_split",
    "emrt_cast": "test_cast_both_ways_bit_exact",
    "emrt_pack_weights": "test_pack_weights_decodes_to_half",
}
EXEMPT = {
    "emrt_conv2d_drop": "dropout epilogue of the FFN's first linear: training only (EMRT_REQUIRE_TRAIN_DTYPE refuses dtype 2 before the shared helper)",
}
# entry points an eval forward records whose prototype has no `dtype` argument (fp32 / integer / byte plumbing)
NO_DTYPE = {
    "emrt_bn_fold", "emrt_memcpy", "emrt_memset", "emrt_crop_windows", "emrt_window_accumulate", "emrt_window_normalise", "emrt_argmax_nchw",
    "emrt_sigmoid_fwd", "emrt_set_scratch", "emrt_flip_w", "emrt_softmax_nchw_acc",
}


def test_recorded_fp16_forward_only_uses_ledgered_entry_points():
    """Record a float16 eval forward of resnet18 at 64^2, of resnet50 at 128^2 and one slide_inference call: every entry point launched is in
    COVERED, EXEMPT or NO_DTYPE -- a float16 path the source scan of the CPU ledger test cannot see would show up here."""
    from emrt_amd.src.api import infer
    from emrt_amd.src.models.emrt import EMRT
    L_ = _lib.lib()
    g = _gen(500)
    seen = set()
    for backbone, size in (("resnet18", 64), ("resnet50", 128)):
        torch.manual_seed(0)
        model = EMRT(num_classes=6, backbone=backbone)
        model.to_hip("cuda:0", F16)
        model.eval()
        x = torch.randn(2, 3, size, size, generator=g)
        L_.start_record()
        try:
            y = model(x.cuda())[0]
            torch.cuda.synchronize()
        finally:
            rec = L_.stop_record()
        assert tuple(y.shape) == (2, 6, size, size)
        seen |= {n for n, _ in rec}
        if backbone == "resnet18":
            img = torch.randn(3, 96, 96, generator=g)
            L_.start_record()
            try:
                out = infer.slide_inference(model, [img.cuda()], (64, 64), (32, 32), 6)[0]
                torch.cuda.synchronize()
            finally:
                rec = L_.stop_record()
            assert tuple(out.shape) == (1, 6, 96, 96)
            seen |= {n for n, _ in rec}
    assert "emrt_conv2d" in seen and "emrt_mha_fwd" in seen and "emrt_layernorm_fwd" in seen, sorted(seen)
    unknown = sorted(n for n in seen if n not in COVERED and n not in EXEMPT and n not in NO_DTYPE)
    assert not unknown, "float16 forward launches entry points without a float16 kernel test: %s" % unknown
