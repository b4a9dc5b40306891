"""-m gpu: the fused epilogues of the dense convolution (csrc/conv.hip, csrc/igemm8p.hpp) swept through every tile and backward path -- the op
"conv" of tests/fuzz_cases.py, a written-out list whose regimes, (kernel kind) x (epilogue copy) x (epilogue features), are computed from the
host-side decisions of conv.hip restated in Python (conv_plan and its ladder, igemm_s2_ok, igemm_xk_copies, igemm8p_ok, the epilogue's vec_ok,
thin_bwd_ok, the pair condition of conv_bwd_dispatch).  tests/test_gpu_conv_fuzz.py sweeps geometries through the same kernels with a plain
epilogue; here the geometry is small and fixed per kernel and the epilogue is what varies.

Every case calls the C ABI directly on torch tensors -- emrt_conv2d (mode 0) forward, emrt_conv2d_bwd backward, and a handful send two unequal
problems of the list through emrt_conv2d_dgrad_multi / emrt_conv2d_group in one launch -- with the weight operands the library's own packing
made (emrt_pack_weights through ParamStore: the forward operand and the transposed data-gradient copy), on operands already rounded to the
case's dtype.  The reference is float64 torch on the CPU (F.conv2d under autograd) with the epilogue applied in the kernel's documented order:
acc x scale + bias, + residual (forward) or + addend / + what dx held (backward), ReLU, then zero where mask_y <= 0 and x mask_scale elsewhere.
mask_y is an input of the call -- relu(randn) with a sprinkling of negative values and of -0.0, so `> 0` and `!= 0` differ -- and needs no
margin.  Forward ReLU cases keep the gconv sweep's rule: no pre-activation within the forward bound of zero on the CPU reference, else the
case is redrawn with the next seed.  With 10^4 to 10^5 outputs per case a randn draw never passes that rule, so these cases draw positive
inputs and one weight sign per output channel: whole channels are clamped, the others pass, and every pre-activation is far from zero.

Bounds, element by element: tests.hip_utils.close_gemm at the project's settings (a bf16 y / dx at out_bits = 8, an fp32 output of bf16 operands
and dw / dbias at out_bits = None, F32 at its own bound), taken at the reference of the FULL expression; float16 through close_f16 with the
slack of tests/test_gpu_fp16_kernels._conv_ref.  No tolerance of this file's own.

The statistics (8 replicas summed) against float64 sums of the output the device STORED, per channel: sum v, and sum v * v or sum v * mask_y
or sum v * stat_x, under n 2^-23 sum |term| -- the recursive-summation bound (n - 1) 2^-24 with a factor 2 of margin, as in the gconv sweep --
where n is the number of fp32 additions in front of one fp64 atomic (fuzz_cases.conv_stat_n):
  * igemm_body, row-vectorised epilogue: a thread adds its BM / RP rows, then one thread adds the RP partials of a column: BM additions;
  * igemm_body, scalar epilogue: a lane adds its 16 TM rows and the other half-wave's sum: 32 TM <= BM;
  * igemm8p_kernel: 16 rows per lane, three shuffle steps over the 8 row lanes, the two wave rows: 256 = BM;
  * thin_bwd_kernel: a thread's share of the block's pixels, then the block's pixel slots: the block's pixel count.
  BM is 64 (64x64 tiles, their K splits, the parity-class, pair and grouped kernels), 128 (128x64, 128x128) or 256 (256x32, 256x256).
A guard of zeros behind the replicas must stay zero, and a column >= OC would land in another statistic's columns and break its sum.

What a case checks beyond the values: every buffer starts as a finite sentinel, everything outside the addressed slice comes back bit-unchanged,
nothing inside keeps the sentinel, no input operand (the packed weights included) is written; masked-out elements are exactly 0.0, also
under addend and accumulate; dw and dbias start from random fp32 contents and come back as contents + gradient, and stay bit-unchanged when
the call was not given them; `corner` / `lastpixel` inputs: every output whose float64 reference is exactly 0 is exactly 0; forward y and dx
are bit-identical over two launches.  The parity-class cases run once more under no_s2_dgrad = 1 (with conv_tile = 1: the generic 64x64 tile
without a K split, the only generic kernel with the same k order per accumulator) and dx must be bit-identical, the statistics within their
bound; the thin cases run once more under no_thin_bwd = 1 on the generic kernels, held to the same reference.

-s prints error / bound per output and case and, at the end, one line per case with the regimes it hit.  A run on an MI355X: DESIGN.md 2.3."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                 # noqa: E402
from emrt_amd import functional as Fn                     # noqa: E402
from emrt_amd import nn as hnn                            # noqa: E402
from emrt_amd._lib import EmrtHipError                    # noqa: E402
from emrt_amd.runtime import ctx, F32, BF16, F16          # noqa: E402
from tests import dropout_reference as dr                 # noqa: E402
from tests import fuzz_cases as fc                        # noqa: E402
from tests.hip_utils import init, close_gemm, close_f16, ulp16, Holder      # noqa: E402
from tests.test_gpu_resnext import _P, _TD, _padded, _whole, _rounded       # noqa: E402
from tests.test_gpu_gconv_fuzz import _bound, _ratio, _clear_of_zero, _sparse, _exact_zeros, _sent, SENTINEL, REDRAWS      # noqa: E402
from tests.test_gpu_fp16_kernels import _conv_ref         # noqa: E402

SWEEP = fc.CASES["conv"]
DTYPE = {"f32": F32, "bf16": BF16, "f16": F16}
MASK_SCALE = 1.0 / (1.0 - 0.25)
GUARD = 512                  # zeros behind the statistics' replicas
LINES = []                   # one summary line per case of this process


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if LINES:
        print("\n[conv epilogue sweep] worst error / bound per output, the kernel each launch took and the regimes each case hit")
        for line in LINES:
            print(line)


class _knobs:
    """set tuning knobs for a block, restore after"""

    def __init__(self, kv):
        self.kv = tuple(kv)

    def __enter__(self):
        L = _lib.lib()
        self.old = [(k, L.set_tuning(k, v)) for k, v in self.kv]

    def __exit__(self, *exc):
        L = _lib.lib()
        for k, v in reversed(self.old):
            L.set_tuning(k, v)


class _Bag(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _mask_like(shape, g, dtype):
    """relu(randn) with a tenth of the elements negative and a twentieth -0.0"""
    m = torch.relu(torch.randn(shape, generator=g))
    r = torch.rand(shape, generator=g)
    m = torch.where(r < 0.1, -torch.randn(shape, generator=g).abs() - 0.01, m)
    m = torch.where((r >= 0.1) & (r < 0.15), torch.full(shape, -0.0), m)
    return _rounded(m, dtype)


def _draw(case, seed):
    """host operands, rounded to the case's dtype, and the float64 reference"""
    f = fc.conv_case_fields(case)
    feats, dtype = fc.conv_feats(case), DTYPE[f.dtype]
    OH, OW = fc.conv_out_size(f.H, f.k, f.stride, f.pad, f.dil), fc.conv_out_size(f.W, f.k, f.stride, f.pad, f.dil)
    g = torch.Generator().manual_seed(seed)
    x = _mask_like((f.N, f.H, f.W, f.C), g, dtype) if "mask_is_x" in feats else _rounded(torch.randn(f.N, f.H, f.W, f.C, generator=g), dtype)
    w = _rounded(torch.randn(f.OC, f.C, f.k, f.k, generator=g) / math.sqrt(f.C * f.k * f.k), dtype)
    d = _Bag(f=f, feats=feats, dtype=dtype, OH=OH, OW=OW, w=w, clear=True, slack=None)
    if f.side == "fwd":
        d.bias, d.scale = torch.randn(f.OC, generator=g), torch.rand(f.OC, generator=g) + 0.5
        d.scale[::3] *= -1          # a negative BatchNorm gamma
        d.res = _rounded(torch.randn(f.N, OH, OW, f.OC, generator=g), dtype)
        if f.inputs != "ordinary":
            x = _sparse(x, f.inputs)
        if "relu" in feats:          # positive inputs, one weight sign per output channel: pre-activations far from zero on both sides of it
            x = x.abs()
            d.w = w = w.abs() * (1.0 - 2.0 * (torch.rand(f.OC, generator=g) < 0.5).float()).view(-1, 1, 1, 1)
        d.x = x
        x64, w64 = x.permute(0, 3, 1, 2).double(), w.double()
        b64 = d.bias.double() if "bias" in feats else None
        s64 = d.scale.double() if "scale" in feats else None
        r64 = d.res.double() if "residual" in feats else None
        if dtype == F16:
            pre, d.slack = _conv_ref(x64, w64, f.stride, f.pad, f.dil, b64, r64, False, s64)
        else:
            pre = F.conv2d(x64, w64, None, f.stride, f.pad, f.dil).permute(0, 2, 3, 1)
            pre = pre * s64 if s64 is not None else pre
            pre = pre + b64 if b64 is not None else pre
            pre = pre + r64 if r64 is not None else pre
        d.want = torch.relu(pre) if "relu" in feats else pre
        if "relu" in feats:          # no pre-activation within the forward bound of zero
            if dtype == F16:
                d.clear = bool((pre.abs() > 0.5 * ulp16(pre) + d.slack).all())
            else:
                d.clear = _clear_of_zero(pre, d.want, *_settings(d))
        return d
    dy = _rounded(torch.randn(f.N, OH, OW, f.OC, generator=g), dtype)
    d.mask = x if "mask_is_x" in feats else _mask_like((f.N, f.H, f.W, f.C), g, dtype)
    d.statx, d.addend, d.prefill = [_rounded(torch.randn(f.N, f.H, f.W, f.C, generator=g), dtype) for _ in range(3)]
    d.dw0, d.db0 = torch.randn(f.OC * f.k * f.k * f.C, generator=g), torch.randn(f.OC, generator=g)
    if f.inputs == "corner":
        x, dy = _sparse(x, "corner"), _sparse(dy, "corner")
        if "mask_is_x" in feats:
            d.mask = x
    elif f.inputs == "lastpixel":
        dy = _sparse(dy, "lastpixel")
    d.x, d.dy = x, dy
    xr, wr = x.permute(0, 3, 1, 2).double().requires_grad_(True), w.double().requires_grad_(True)
    br = torch.zeros(f.OC, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, br, f.stride, f.pad, f.dil).backward(dy.permute(0, 3, 1, 2).double())
    d.dgrad, d.dwr, d.dbr = xr.grad.permute(0, 2, 3, 1), wr.grad, br.grad
    want = d.dgrad
    if "addend" in feats:
        want = want + d.addend.double()
    if "accumulate" in feats:
        want = want + d.prefill.double()
    if "mask" in feats:
        ms = float(torch.tensor(MASK_SCALE, dtype=torch.float32)) if "mask_scale" in feats else 1.0
        want = torch.where(d.mask > 0, want * ms, torch.zeros_like(want))
    d.want = want
    return d


def _settings(d):
    """(dtype, out_bits) close_gemm takes for y / dx: a bf16 stored output at 8 bits, an fp32 output of bf16 operands at None, F32 at its own bound"""
    if d.dtype == F32:
        return F32, None
    return BF16, (None if "out_f32" in d.feats else 8)


def _view(t, v, tdtype, fill=SENTINEL):
    """device NHWC view of the layout fuzz_cases.conv_view describes: channels [off, off + C) of rows ld wide, images bs apart"""
    if v.off == 0 and tdtype != torch.float32:
        return _padded(t, v.ld, {torch.bfloat16: BF16, torch.float16: F16}[tdtype], v.bs, fill)
    N, H, W, C = t.shape
    buf = torch.full((N * v.bs,), fill, dtype=tdtype, device="cuda")
    view = buf.as_strided((N, H, W, C), (v.bs, W * v.ld, v.ld, 1), v.off)
    view.copy_(t.to(device="cuda", dtype=tdtype))
    return view


def _prepare(case):
    """draw (redrawing a forward ReLU case until it is clear of zero), pack the weights with the library, put every input on the device"""
    for k in range(REDRAWS):
        d = _draw(case, case[-1] + 1000 * k)
        if d.clear:
            break
    else:
        raise AssertionError("%s: no draw in %d keeps every pre-activation outside the forward bound of zero" % (case[0], REDRAWS))
    d.redraws = k
    f, td = d.f, _TD[d.dtype]
    conv = hnn.Conv2D(f.C, f.OC, f.k, f.stride, f.pad, bias=False, dilation=f.dil)
    with torch.no_grad():
        conv.weight.copy_(d.w)
    d.holder = Holder(conv=conv).place()
    d.gw = conv.gw
    d.t = t = fc.conv_tensors(case)
    d.dev = {}
    if f.side == "fwd":
        d.dev["in"] = _view(d.x, t["in"], td)
        d.bias_d = d.bias.cuda() if "bias" in d.feats else None
        d.scale_d = d.scale.cuda() if "scale" in d.feats else None
        if "res" in t:
            d.dev["res"] = _view(d.res, t["res"], td)
    else:
        d.dev["x"] = _view(d.x, t["x"], td)
        d.dev["dy"] = _view(d.dy, t["dy"], td)
        if "mask" in d.feats:
            d.dev["mask"] = d.dev["x"] if "mask_is_x" in d.feats else _view(d.mask, t["mask"], td)
        if "statx" in t:
            d.dev["statx"] = _view(d.statx, t["statx"], td)
        if "addend" in t:
            d.dev["addend"] = _view(d.addend, t["addend"], td)
    torch.cuda.synchronize()
    d.before = dict((k, _whole(v).clone()) for k, v in d.dev.items())
    d.before["packed"], d.before["master"] = d.holder.store.packed.clone(), d.holder.store.master.clone()
    return d


def _outputs(d):
    """fresh outputs of one launch: the output view (sentinel, or what dx held under accumulate), zeroed statistics with their guard, dw / dbias"""
    f = d.f
    if f.side == "fwd":
        o = _Bag(out=_view(torch.full((f.N, d.OH, d.OW, f.OC), SENTINEL), d.t["out"], torch.float32 if "out_f32" in d.feats else _TD[d.dtype]))
        Cn = f.OC
    else:
        start = d.prefill if "accumulate" in d.feats else torch.full((f.N, f.H, f.W, f.C), SENTINEL)
        o = _Bag(out=_view(start, d.t["dx"], _TD[d.dtype]), dw=d.dw0.cuda(), db=d.db0.cuda())
        Cn = f.C
    o.stats = torch.zeros(8 * 2 * Cn + GUARD, dtype=torch.float64, device="cuda") if "stats" in d.feats else None
    return o


def _launch(d, o, single=True):
    """one call of the entry point (single), or the descriptor of this problem for a grouped launch"""
    f, t, L, st = d.f, d.t, _lib.lib(), ctx().stream
    if f.side == "fwd":
        res = d.dev.get("res")
        ldres, res_bs = (t["res"].ld, t["res"].bs) if res is not None else (0, 0)
        if single:
            L.call("emrt_conv2d", _P(d.dev["in"]), ctypes.c_void_p(d.gw.fwd_ptr), _P(o.out), _P(d.bias_d), _P(res), f.N, f.H, f.W, f.C, t["in"].ld, t["in"].bs,
                   d.OH, d.OW, f.OC, t["out"].ld, t["out"].bs, ldres, res_bs, f.k, f.k, f.stride, f.pad, 0, int("relu" in d.feats), int("out_f32" in d.feats),
                   _P(o.stats), None, 0, 0, f.dil, _P(d.scale_d), d.dtype, st)
            return None
        e = Fn._ConvDesc()
        e.inp, e.w_packed, e.out, e.bias, e.residual, e.bn_stats = d.dev["in"].data_ptr(), d.gw.fwd_ptr, o.out.data_ptr(), Fn._dp(d.bias_d), Fn._dp(res), Fn._dp(o.stats)
        e.N, e.H, e.W, e.C, e.ldin, e.in_bs = f.N, f.H, f.W, f.C, t["in"].ld, t["in"].bs
        e.OH, e.OW, e.OC, e.ldout, e.out_bs, e.ldres, e.res_bs = d.OH, d.OW, f.OC, t["out"].ld, t["out"].bs, ldres, res_bs
        e.KH, e.KW, e.stride, e.pad, e.relu, e.out_f32 = f.k, f.k, f.stride, f.pad, int("relu" in d.feats), int("out_f32" in d.feats)
        return e
    mask, statx, addend = d.dev.get("mask"), d.dev.get("statx"), d.dev.get("addend")
    ldy, y_bs = (t["mask"].ld, t["mask"].bs) if mask is not None else (0, 0)
    ldsx, sx_bs = (t["statx"].ld, t["statx"].bs) if statx is not None else (0, 0)
    ldadd, add_bs = (t["addend"].ld, t["addend"].bs) if addend is not None else (0, 0)
    ms = MASK_SCALE if "mask_scale" in d.feats else 1.0
    acc = int("accumulate" in d.feats)
    if single:
        L.call("emrt_conv2d_bwd", _P(d.dev["x"]), _P(d.dev["dy"]), ctypes.c_void_p(d.gw.bwd_ptr), _P(o.out), t["dx"].ld, t["dx"].bs, acc,
               _P(o.dw) if "dw" in f.arm else None, _P(o.db) if "dbias" in f.arm else None, f.N, f.H, f.W, f.C, t["x"].ld, t["x"].bs, d.OH, d.OW, f.OC,
               t["dy"].ld, t["dy"].bs, f.k, f.k, f.stride, f.pad, _P(o.stats), _P(mask), ldy, y_bs, ms, _P(statx), ldsx, sx_bs, _P(addend), ldadd, add_bs,
               f.dil, d.dtype, st)
        return None
    e = Fn._DgradDesc()
    e.dy, e.w_bwd_packed, e.dx, e.lddx, e.dx_bs, e.accumulate = d.dev["dy"].data_ptr(), d.gw.bwd_ptr, o.out.data_ptr(), t["dx"].ld, t["dx"].bs, acc
    e.N, e.H, e.W, e.C, e.OH, e.OW, e.OC, e.lddy, e.dy_bs = f.N, f.H, f.W, f.C, d.OH, d.OW, f.OC, t["dy"].ld, t["dy"].bs
    e.KH, e.KW, e.stride, e.pad, e.dilation = f.k, f.k, f.stride, f.pad, f.dil
    e.bn_stats, e.mask_y, e.ldy, e.y_bs, e.mask_scale = Fn._dp(o.stats), Fn._dp(mask), ldy, y_bs, ms
    e.stat_x, e.ldsx, e.sx_bs, e.addend, e.ldadd, e.add_bs = Fn._dp(statx), ldsx, sx_bs, Fn._dp(addend), ldadd, add_bs
    return e


def _slice_checks(name, view, must_be_written):
    whole = _whole(view)
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside.as_strided(tuple(view.shape), view.stride(), view.storage_offset()).fill_(False)
    assert bool((whole[outside] == _sent(view)).all()), "%s: written outside the addressed slice (channels beside it or rows behind an image)" % name
    if must_be_written:
        assert not bool((view == _sent(view)).any()), "%s: an element inside the slice was never written" % name


def _hold(name, got, ref, dtype, out_bits, ratios, key):
    got, ref = got.float().cpu(), ref.float().cpu()
    ratios[key] = max(ratios.get(key, 0.0), _ratio((got - ref).abs(), _bound(ref, dtype, out_bits)))
    print("    %-40s error / bound %.3f" % (name, ratios[key]))
    close_gemm(name, got, ref, dtype, out_bits=out_bits)


def _check(d, o, n, ratios, tag, grads=True):
    """one launch's outputs against the reference; n: fp32 additions in front of one statistics atomic (fuzz_cases.conv_stat_n)"""
    f = d.f
    name = "%s %s" % (tag, "y" if f.side == "fwd" else "dx")
    sparse = f.inputs != "ordinary"
    _slice_checks(name, o.out, "accumulate" not in d.feats)
    if d.dtype == F16:
        use = close_f16(name, o.out, d.want, d.slack, out_f32="out_f32" in d.feats)
        ratios["y (err - ulp/2) / slack"] = max(ratios.get("y (err - ulp/2) / slack", -1.0), use)
    else:
        _hold(name, o.out, d.want, *_settings(d), ratios=ratios, key="y" if f.side == "fwd" else "dx")
    if sparse:
        _exact_zeros(name, o.out, d.want)
    if "mask" in d.feats:
        off = (d.mask <= 0)
        assert bool((o.out.float().cpu()[off] == 0).all()), "%s: a masked-out element is not exactly 0" % name
    if o.stats is not None:
        Cn = o.out.shape[-1]
        tail = o.stats[8 * 2 * Cn:].cpu()
        assert bool((tail == 0).all()), "%s: the statistics were written behind their 8 replicas" % name
        got = o.stats[:8 * 2 * Cn].cpu().view(8, 2, Cn).sum(0)
        assert bool(torch.isfinite(got).all())
        v = o.out.double().cpu().reshape(-1, Cn)
        second = (d.statx if "stat_x" in d.feats else d.mask).double().reshape(-1, Cn) if "mask" in d.feats else v
        for which, term in enumerate((v, v * second)):
            key = ("sum", "second sum")[which]
            r = _ratio((got[which] - term.sum(0)).abs(), n * 2.0 ** -23 * term.abs().sum(0))
            ratios[key] = max(ratios.get(key, 0.0), r)
        print("    %-40s error / bound %.3f (sums), %.3f (second statistic); n = %d" % (name + " statistics", ratios["sum"], ratios["second sum"], n))
        assert ratios["sum"] <= 1.0 and ratios["second sum"] <= 1.0, "%s: statistics beyond n 2^-23 sum |term| (n = %d): %s" % (name, n, ratios)
    if f.side == "bwd" and grads:
        if "dw" in f.arm:
            got = (o.dw.cpu() - d.dw0).view(f.OC, f.k, f.k, f.C).permute(0, 3, 1, 2)
            _hold(tag + " dw", got, d.dwr, d.dtype, None, ratios, "dw")
            if sparse:
                _exact_zeros(tag + " dw", got, d.dwr)
        else:
            assert torch.equal(o.dw.cpu(), d.dw0), "%s: dw was written by a call that was not given it" % tag
        if "dbias" in f.arm:
            got = o.db.cpu() - d.db0
            _hold(tag + " dbias", got, d.dbr, d.dtype, None, ratios, "dbias")
            if sparse:
                _exact_zeros(tag + " dbias", got, d.dbr)
        else:
            assert torch.equal(o.db.cpu(), d.db0), "%s: dbias was written by a call that was not given it" % tag


def _inputs_unwritten(d, tag):
    for k, v in d.dev.items():
        assert torch.equal(_whole(v), d.before[k]), "%s: the input operand %s was written" % (tag, k)
    assert torch.equal(d.holder.store.packed, d.before["packed"]) and torch.equal(d.holder.store.master, d.before["master"]), "%s: the weights were written" % tag


def _describe(d):
    f = d.f
    return "%s %dx%dx%dx%d -> %d, k %d stride %d pad %d, %s %s, %s, arm %s, views [%s], knobs %s, %s%s" % (
        f.id, f.N, f.H, f.W, f.C, f.OC, f.k, f.stride, f.pad, f.dtype, f.side, f.epilogue, f.arm, f.views, dict(f.knobs), f.inputs,
        ", redrawn %d x" % d.redraws if d.redraws else "")


def _grouped(case):
    """two problems of the list in one launch of emrt_conv2d_dgrad_multi / emrt_conv2d_group, twice, each held to its single case's reference"""
    side, dtype = case[11], DTYPE[case[10]]
    init(dtype)
    ds = [_prepare(m) for m in fc.conv_group_members(case)]
    entry, desc = ("emrt_conv2d_dgrad_multi", Fn._DgradDesc) if side == "multi" else ("emrt_conv2d_group", Fn._ConvDesc)
    ratios, runs = {}, []
    print("\n  %s %s of %s" % (case[0], entry, ", ".join(d.f.id for d in ds)))
    for _ in range(2):
        outs = [_outputs(d) for d in ds]
        arr = (desc * 2)()
        for i, (d, o) in enumerate(zip(ds, outs)):
            arr[i] = _launch(d, o, single=False)
        _lib.lib().call(entry, arr, 2, dtype, ctx().stream)
        torch.cuda.synchronize()
        runs.append(outs)
    for i, d in enumerate(ds):
        _check(d, runs[0][i], 64, ratios, "%s[%s]" % (case[0], d.f.id), grads=False)
        assert torch.equal(runs[0][i].out, runs[1][i].out), "%s: problem %d differs between two launches" % (case[0], i)
        assert torch.equal(runs[0][i].dw.cpu(), d.dw0) if side == "multi" else True
        _inputs_unwritten(d, case[0])
    hit = [name for name, pred in fc.CONV_REGIMES if pred(case)]
    LINES.append("  %-13s %s | grouped 64x64 | %s" % (case[0], "  ".join("%s %.3f" % kv for kv in ratios.items()), "; ".join(hit)))


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_conv_epilogue_sweep(case):
    if case[11] in ("multi", "group"):
        return _grouped(case)
    init(DTYPE[case[10]])
    d = _prepare(case)
    f, ratios = d.f, {}
    route = fc.conv_route(case)
    print("\n  %s -> %s, %s epilogue" % (_describe(d), fc.conv_kind_name(route), route[2]))
    first = None
    for k in range(2):          # the same launch twice: forward y and dx are bit-identical (dw, dbias and the statistics are atomics: held to their bounds both times)
        o = _outputs(d)
        with _knobs(f.knobs):
            _launch(d, o)
            torch.cuda.synchronize()
        _check(d, o, fc.conv_stat_n(case), ratios, f.id if k == 0 else f.id + " (again)")
        if first is None:
            first = o
        else:
            assert torch.equal(first.out, o.out), "%s: the output differs between two launches" % f.id
    twin = ""
    if f.twin:
        o = _outputs(d)
        with _knobs(f.twin):
            _launch(d, o)
            torch.cuda.synchronize()
        troute = fc.conv_route(case, True)
        twin = " (twin: %s, %s epilogue)" % (fc.conv_kind_name(troute), troute[2])
        _check(d, o, fc.conv_stat_n(case, True), ratios, f.id + " twin")
        if route[0] == "s2":
            assert torch.equal(first.out, o.out), "%s: the parity-class kernel's dx differs from the generic 64x64 tile's" % f.id
    _inputs_unwritten(d, f.id)
    hit = [name for name, pred in fc.CONV_REGIMES if pred(case)]
    LINES.append("  %-13s %s | %s, %s epilogue%s | %s" % (f.id, "  ".join("%s %.3f" % kv for kv in ratios.items()), fc.conv_kind_name(route), route[2], twin, "; ".join(hit)))


def test_conv_epilogue_refusals_launch_nothing():
    """argument combinations outside the domain of fuzz_cases.conv_in_domain: an error from the entry point's checks, in front of any launch"""
    init(F32)
    L = _lib.lib()
    st = ctx().stream
    N, H, W, C, OC = 2, 8, 8, 16, 16
    buf = torch.zeros(N * H * W * 32, device="cuda")
    stats = torch.zeros(8 * 2 * 32, dtype=torch.float64, device="cuda")
    before, sb = buf.clone(), stats.clone()
    p = _P(buf)

    def bwd(lddx=C, acc=0, dw=p, db=None, mask=None, statx=None, addend=None, OH=H):
        L.call("emrt_conv2d_bwd", p, p, p, p, lddx, H * W * lddx, acc, dw, db, N, H, W, C, C, H * W * C, OH, W, OC, OC, H * W * OC, 3, 3, 1, 1, _P(stats), mask, C,
               H * W * C, 1.0, statx, C, H * W * C, addend, C, H * W * C, 1, F32, st)

    with pytest.raises(EmrtHipError, match="accumulate adds into dx itself"):
        bwd(acc=1, addend=p)
    with pytest.raises(EmrtHipError, match="stat_x replaces the mask tensor"):
        bwd(statx=p)
    with pytest.raises(EmrtHipError, match="dw == NULL asks for the data gradient only"):
        bwd(dw=None, db=p)
    with pytest.raises(EmrtHipError, match="bad dx strides"):
        bwd(lddx=C - 4)
    with pytest.raises(EmrtHipError, match="output size mismatch"):
        bwd(OH=H - 1)
    with pytest.raises(EmrtHipError, match="the ReLU mask needs an output in the compute dtype"):
        L.call("emrt_conv2d", p, p, p, None, None, N, H, W, C, C, H * W * C, H, W, OC, OC, H * W * OC, 0, 0, 3, 3, 1, 1, 0, 0, 1, None, p, OC, H * W * OC, 1, None, F32, st)
    arr = (Fn._DgradDesc * 2)()
    for e in arr:
        e.dy, e.w_bwd_packed, e.dx, e.lddx, e.dx_bs = buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), C, H * W * C
        e.N, e.H, e.W, e.C, e.OH, e.OW, e.OC, e.lddy, e.dy_bs = N, H, W, C, H, W, OC, OC, H * W * OC
        e.KH, e.KW, e.stride, e.pad, e.dilation, e.mask_scale = 3, 3, 1, 1, 1, 1.0
    with pytest.raises(EmrtHipError, match="must not write the same dx"):
        L.call("emrt_conv2d_dgrad_multi", arr, 2, F32, st)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and torch.equal(stats, sb)


# ---- emrt_conv2d_drop: dropout(relu(x w^T + bias)) with the mask drawn in the 64x64 tile's epilogue ---------------------------------------------
DROP_SWEEP = fc.CASES["conv_drop"]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", DROP_SWEEP, ids=[c[0] for c in DROP_SWEEP])
def test_conv2d_drop_mask_is_the_models(dtype, case):
    """emrt_conv2d_drop called directly over fuzz_cases.CASES["conv_drop"]: M on both sides of the 64-row tile, one to sixteen N tiles, K of one
    chunk to several k-tiles, the output dense and as a slice of wider rows (ldout > OC), the input once with ldin > C; pre-activations of both
    signs.  The mask is the host model's (tests/dropout_reference.py: drop_words8 at (m * OC + n0) >> 3 -- OC, not ldout), bit for bit: an
    element the model drops is exactly 0; an element it keeps equals relu(x w^T + bias) / (1 - p) in float64 on the rounded operands within
    close_gemm's bound on relu(linear) times ks, so wherever the kept value stands clear of zero the device's mask is read off the output and
    must be the model's.  The columns beside the slice and the rows behind it keep their sentinel bits; the inputs are not written."""
    cid, M, C, ldin, OC, ldout, p, salt, _, seed = case
    c = init(dtype, seed=seed)
    td = _TD[dtype]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g).to(td)
    w = (torch.randn(OC, C, generator=g) / math.sqrt(C)).to(td)
    b = torch.randn(OC, generator=g) * 0.3
    lin = hnn.Linear(C, OC)
    with torch.no_grad():
        lin.weight.copy_(w.float())
        lin.bias.copy_(b)
    holder = Holder(lin=lin).place()
    xbuf = torch.full((M + 2, ldin), 1.0e4, dtype=td)          # (what lies beside and behind the input would show in every output)
    xbuf[:M, :C] = x
    xd = xbuf.cuda()
    out = torch.full((M + 2, ldout), SENTINEL, dtype=td, device="cuda")
    before = (holder.store.packed.clone(), holder.store.master.clone())
    _lib.lib().call("emrt_conv2d_drop", _P(xd), ctypes.c_void_p(lin.gw.fwd_ptr), _P(out), _P(lin.gw.bias), M, C, ldin, OC, ldout, float(p), c.seed_ptr,
                    salt, dtype, c.stream)
    torch.cuda.synchronize()
    keep = torch.from_numpy(dr.conv_drop_mask(dr.context_seed(seed), salt, p, M, OC))
    got = out[:M, :OC].cpu()
    fresh = torch.full((M + 2, ldout), SENTINEL, dtype=td)
    it = torch.int32 if td == torch.float32 else torch.int16
    assert torch.equal(out.cpu().view(it)[:, OC:], fresh.view(it)[:, OC:]) and torch.equal(out.cpu().view(it)[M:], fresh.view(it)[M:]), \
        "%s: written beside the slice (columns >= %d of rows of %d) or behind it" % (cid, OC, ldout)
    assert bool(torch.isfinite(got.float()).all()), "%s: an element of the slice was not written" % cid
    assert torch.equal(xd.cpu().view(it), xbuf.view(it)) and torch.equal(holder.store.packed, before[0]) and torch.equal(holder.store.master, before[1])
    assert bool((got[~keep] == 0).all()), "%s: %d elements the model drops are not 0" % (cid, int((got[~keep] != 0).sum()))
    r = (x.double() @ w.double().t() + b.double()).clamp_min(0)
    assert bool((r > 0).any()) and bool((r == 0).any())          # pre-activations of both signs
    ks = 1.0 / (1.0 - float(torch.tensor(p, dtype=torch.float32)))
    rms = r.pow(2).mean().sqrt().item()
    bound = (2e-4 * r + 2e-4 * max(rms, 1e-30)) if dtype == F32 else (2.0 ** -8 * r + 2.0 ** -10 * rms)          # close_gemm's bound on relu(linear)
    want = torch.where(keep, r * ks, torch.zeros_like(r))
    err = (got.double() - want).abs()
    bad = err > bound * ks
    assert not bool(bad.any()), "%s: %d of %d elements beyond the bound; worst error / bound %.3f; first at %s: got %.6g, want %.6g (model keeps: %s)" % (
        cid, int(bad.sum()), bad.numel(), (err / (bound * ks)).max().item(), torch.nonzero(bad)[0].tolist(), got[bad][0].item(), want[bad][0].item(),
        bool(keep[bad][0]))
    clear = r * ks > 2 * bound * ks          # here a kept value cannot be mistaken for a dropped one: the device's mask, read back
    assert torch.equal((got != 0)[clear], keep[clear]) and int(clear.sum()) >= max(1, M * OC // 5)          # (about half the pre-activations are positive)
