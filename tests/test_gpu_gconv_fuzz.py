"""-m gpu: the grouped 3x3 convolution kernels of csrc/gconv.hip (forward, data gradient, weight gradient, bias gradient) swept by group shape,
launch plan and view -- the op "gconv" of tests/fuzz_cases.py, 41 written-out cases whose regimes are computed from pick_block / launch_fwd /
launch_dgrad / launch_wgrad restated in Python.  Every case calls the C ABI directly (emrt_gconv2d, emrt_gconv2d_bwd) and is held, element by
element, to float64 torch (F.conv2d(..., padding=1, groups=g) under autograd on the CPU) on operands already rounded to the case's dtype, under
tests.hip_utils.close_gemm at the settings of tests/test_gpu_resnext.py (out_bits = 8 for a bf16 y / dx, fp32 dw / dbias at out_bits = None,
fp16 y at out_bits = 10).

What a case checks beyond the values:
  * output channels per group different from the input's (Og < Cg, Og > Cg, Og = 4, 12, 20), block shapes that leave threads idle or end on a
    ragged channel slice, maps of one or two rows / columns, fewer pixels than a tile, pixel quads that cross a row or an image end;
  * a second trip round each grid-stride loop (4129 tiles on 4096 blocks forward and in the data gradient; 265 tiles on 256 x 8 blocks with
    the statistics' per-thread fp32 sums over two tiles);
  * every tensor as a channel slice of a wider buffer (ld), with padding behind each image (bs) and both: all buffers start as a finite sentinel,
    everything outside the addressed slice must come back bit-unchanged, nothing inside may keep the sentinel, and no operand is written;
  * dw and dbias start from random fp32 contents and must come back as contents + gradient; an output the call was not given stays bit-unchanged;
    dx with accumulate starts from random contents; the backward arms are all three outputs, dx alone, dw alone, dbias alone, dx-accumulate + dw;
  * forward and dx are bit-identical over two launches (the kernel header's promise);
  * the BatchNorm statistics (8 replicas summed) against float64 sums of the STORED output per channel, under n 2^-23 sum |v| and n 2^-23 sum v^2
    with n = 4 ceil(ntiles / gx) + PS: the number of fp32 additions in front of one fp64 atomic (per-thread over its tiles' 4 pixels, then PS
    slots in the column sum) -- the recursive-summation bound (n - 1) 2^-24 with a factor 2 of margin;
  * the ReLU cases: the gradient reference is masked by the reference's own sign (the kernel-level backward takes dy as it is: the mask is
    functional.gconv2d's emrt_mask_bwd, which the two wrapper tests below run).  No pre-activation lies within the forward bound of zero -- the
    margin is close_gemm's bound taken at |pre|, checked on the CPU reference; a draw that misses it is redrawn with the next seed;
  * `corner` (x and dy zero but for the four corner pixels of the first image and the last pixel of the last one) and `lastpixel` (dy at the last
    output pixel alone): every output whose float64 reference is exactly 0 is exactly 0 on the device.

-s prints error / bound per output and case, and one line per case with the regimes it hit at the end.  Refusals are one test without a launch.
A run on an MI355X: DESIGN.md 2.2."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                 # noqa: E402
from emrt_amd import nn as hnn                            # noqa: E402
from emrt_amd._lib import EmrtHipError                    # noqa: E402
from emrt_amd.runtime import ctx, F32, BF16, F16, Tape     # noqa: E402
from tests import fuzz_cases as fc                        # noqa: E402
from tests.hip_utils import init, close_gemm, Holder      # noqa: E402
from tests.test_gpu_resnext import _P, _TD, _padded, _whole, _run_fwd, _run_bwd, _rounded      # noqa: E402

SWEEP = fc.CASES["gconv"]
DTYPE = {"f32": F32, "bf16": BF16, "f16": F16}
SENTINEL = -12345.0          # finite in every dtype (bf16 stores -12352); no reference value comes near it
REDRAWS = 400
LINES = []                   # one summary line per case of this process


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if LINES:
        print("\n[gconv sweep] worst error / bound per output, and the regimes each case hit")
        for line in LINES:
            print(line)


def _bound(ref, dtype, out_bits):
    """close_gemm's bound (tests/hip_utils.py), for the printed error / bound and the ReLU margin only: the assertion is close_gemm itself"""
    ref = ref.float()
    rms = ref.pow(2).mean().sqrt().item()
    if dtype == F32:
        return 2e-4 * ref.abs() + 2e-4 * max(rms, 1e-30)
    if out_bits is None:
        return 2.0 ** -12 * (ref.abs() + rms)
    return 2.0 ** -out_bits * ref.abs() + 2.0 ** -(out_bits + 2) * rms


def _clear_of_zero(pre, yr, dtype, out_bits):
    """the ReLU margin: every |pre| lies beyond close_gemm's forward bound taken at |pre| (the RMS term from the stored reference yr)"""
    at = pre.abs().float()
    rms = yr.float().pow(2).mean().sqrt().item()
    margin = (2e-4 * at + 2e-4 * max(rms, 1e-30)) if dtype == F32 else (2.0 ** -out_bits * at + 2.0 ** -(out_bits + 2) * rms)
    return bool((at > margin).all())


def _ratio(err, bound):
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


def _hold(name, got, ref, dtype, out_bits, ratios, key):
    got, ref = got.float().cpu(), ref.float().cpu()
    ratios[key] = max(ratios.get(key, 0.0), _ratio((got - ref).abs(), _bound(ref, dtype, out_bits)))
    print("    %-34s error / bound %.3f" % (name, ratios[key]))
    close_gemm(name, got, ref, dtype, out_bits=out_bits)


def _y_settings(dname):
    """(dtype, out_bits) close_gemm takes for y and dx: as tests/test_gpu_resnext.py (fp16 as test_gconv_bn_stats_fold_relu_and_fp16)"""
    return {"f32": (F32, None), "bf16": (BF16, 8), "f16": (BF16, 10)}[dname]


def _sparse(t, kind):
    """corner: zero but for the four corner pixels of the first image and the last pixel of the last image; lastpixel: that last pixel alone"""
    keep = torch.zeros(t.shape[:3], dtype=torch.bool)
    keep[-1, -1, -1] = True
    if kind == "corner":
        keep[0, 0, 0] = keep[0, 0, -1] = keep[0, -1, 0] = keep[0, -1, -1] = True
    return t * keep[..., None]


def _draw(case, seed):
    """host operands, rounded to the case's dtype, and the float64 reference -> dict"""
    cid, N, H, W, groups, Cg, Og, stride, dname, epilogue, _, arm, inputs, _, _ = case
    dtype = DTYPE[dname]
    C, OC, OH, OW, _, _ = fc.gconv_dims(case)
    g = torch.Generator().manual_seed(seed)
    x = _rounded(torch.randn(N, H, W, C, generator=g), dtype)
    w = _rounded(torch.randn(OC, Cg, 3, 3, generator=g) / math.sqrt(9 * Cg), dtype)
    dy = _rounded(torch.randn(N, OH, OW, OC, generator=g), dtype)
    bias, scale, shift = torch.randn(OC, generator=g), torch.rand(OC, generator=g) + 0.5, torch.randn(OC, generator=g)
    prefill = _rounded(torch.randn(N, H, W, C, generator=g), dtype)
    dw0, db0 = torch.randn(OC * 9 * Cg, generator=g), torch.randn(OC, generator=g)
    if inputs == "corner":
        x, dy = _sparse(x, "corner"), _sparse(dy, "corner")
    elif inputs == "lastpixel":
        dy = _sparse(dy, "lastpixel")
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = torch.zeros(OC, dtype=torch.float64, requires_grad=True)
    z = F.conv2d(xr, wr, br, stride=stride, padding=1, groups=groups)
    pre = z.detach().permute(0, 2, 3, 1)
    if "bias" in epilogue:
        pre = pre + bias.double()
    if epilogue.startswith("fold"):
        pre = pre * scale.double() + shift.double()
    relu = epilogue.endswith("relu")
    yr = torch.relu(pre) if relu else pre
    d = dict(x=x, w=w, bias=bias, scale=scale, shift=shift, prefill=prefill, dw0=dw0, db0=db0, yr=yr, relu=relu, clear=True)
    if relu:          # the margin: no pre-activation within the forward bound of zero
        d["clear"] = _clear_of_zero(pre, yr, *_y_settings(dname))
        dy = dy * (pre > 0).float()          # the mask of the reference's own sign: the kernel-level backward takes dy as it is
    d["dy"] = dy
    if arm != "none":
        z.backward(dy.permute(0, 3, 1, 2).double())
        d["dxr"], d["dwr"], d["dbr"] = xr.grad.permute(0, 2, 3, 1), wr.grad, br.grad
    return d


def _inputs(case):
    for k in range(REDRAWS):
        d = _draw(case, case[-1] + 1000 * k)
        if d["clear"]:
            return d, k
    raise AssertionError("%s: no draw in %d keeps every pre-activation outside the forward bound of zero" % (case[0], REDRAWS))


def _sent(view):
    return torch.full((), SENTINEL, dtype=view.dtype, device=view.device)


def _outside_untouched(name, view):
    """every element of the buffer that the view does not address still holds the sentinel"""
    whole = _whole(view)
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside.as_strided(tuple(view.shape), view.stride()).fill_(False)
    assert bool((whole[outside] == _sent(view)).all()), "%s: written outside the addressed slice (channels beyond C or rows behind an image)" % name


def _none_kept(name, view):
    assert not bool((view == _sent(view)).any()), "%s: an element inside the slice was never written" % name


def _exact_zeros(name, got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    zero = ref == 0
    assert bool((got[zero] == 0).all()), "%s: %d of the %d outputs whose reference is exactly 0 are not" % (name, int((got[zero] != 0).sum()), int(zero.sum()))


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_gconv_sweep(case):
    cid, N, H, W, groups, Cg, Og, stride, dname, epilogue, views, arm, inputs, _, _ = case
    dtype = DTYPE[dname]
    init(dtype if dtype != F16 else F32)
    C, OC, OH, OW, M, Mi = fc.gconv_dims(case)
    (ldin, in_bs), (ldout, out_bs) = fc.gconv_view(views[0], C, H * W), fc.gconv_view(views[1], OC, OH * OW)
    (lddy, dy_bs), (lddx, dx_bs) = fc.gconv_view(views[2], OC, OH * OW), fc.gconv_view(views[3], C, H * W)
    d, redraws = _inputs(case)
    ratios = {}
    ydt, ybits = _y_settings(dname)
    sparse = inputs != "ordinary"
    print("\n  %s %dx%dx%d, %d groups of %d -> %d, stride %d, %s, %s, views %s, arm %s, %s%s" % (
        cid, N, H, W, groups, Cg, Og, stride, dname, epilogue, "/".join(views), arm, inputs, ", redrawn %d x" % redraws if redraws else ""))

    # ---- forward, twice ----
    stats = epilogue.startswith("stats")
    dev_bias = d["shift"].cuda() if epilogue.startswith("fold") else (d["bias"].cuda() if "bias" in epilogue else None)
    dev_scale = d["scale"].cuda() if epilogue.startswith("fold") else None
    sums = [torch.zeros(8 * 2 * OC, dtype=torch.float64, device="cuda") if stats else None for _ in range(2)]
    kw = dict(relu=d["relu"], bias=dev_bias, scale=dev_scale, ld_in=ldin, ld_out=ldout, bs_in=in_bs, bs_out=out_bs, fill=SENTINEL)
    y, xd, wd = _run_fwd(d["x"], d["w"], groups, stride, dtype, stats=sums[0], **kw)
    x_before, w_before = _whole(xd).clone(), wd.clone()
    y2, _, _ = _run_fwd(d["x"], d["w"], groups, stride, dtype, stats=sums[1], xd=xd, wd=wd, **kw)
    torch.cuda.synchronize()
    assert torch.equal(y, y2), "%s: the forward differs between two launches" % cid
    _outside_untouched(cid + " y", y)
    _none_kept(cid + " y", y)
    _hold(cid + " y", y, d["yr"], ydt, ybits, ratios, "y")
    if sparse:
        _exact_zeros(cid + " y", y, d["yr"])
    if stats:
        ntiles, gx, _, _ = fc.gconv_grid(M, OC, True)
        n = 4 * fc._ceil_div(ntiles, gx) + fc.gconv_block(OC // 4)[1]
        yv = y.double().cpu().reshape(-1, OC)
        for s in sums:
            got = s.cpu().view(8, 2, OC).sum(0)
            for which, (want, mag) in enumerate(((yv.sum(0), yv.abs().sum(0)), ((yv * yv).sum(0), (yv * yv).sum(0)))):
                key = ("sum", "sumsq")[which]
                ratios[key] = max(ratios.get(key, 0.0), _ratio((got[which] - want).abs(), n * 2.0 ** -23 * mag))
            assert bool(torch.isfinite(got).all())
        print("    %-34s error / bound %.3f (sums), %.3f (sums of squares); n = %d" % (cid + " statistics", ratios["sum"], ratios["sumsq"], n))
        assert ratios["sum"] <= 1.0 and ratios["sumsq"] <= 1.0, "%s: BatchNorm statistics beyond n 2^-23 sum |v| (n = %d): %s" % (cid, n, ratios)

    # ---- backward ----
    if arm != "none":
        with_dx, acc = arm in ("all", "dx", "dx-acc+dw"), arm == "dx-acc+dw"
        with_dw, with_db = arm in ("all", "dw", "dx-acc+dw"), arm in ("all", "dbias")
        dyd = _padded(d["dy"], lddy, dtype, dy_bs, SENTINEL)
        dy_before = _whole(dyd).clone()
        start = d["prefill"] if acc else torch.full((N, H, W, C), SENTINEL)
        dx, dx2 = [_padded(start, lddx, dtype, dx_bs, SENTINEL) if with_dx else None for _ in range(2)]
        dw0, db0 = d["dw0"].cuda(), d["db0"].cuda()
        dw, db = dw0.clone(), db0.clone()
        _run_bwd(xd, wd, dyd, groups, stride, dtype, dx=dx, accumulate=acc, dw=dw if with_dw else None, dbias=db if with_db else None)
        if with_dx:
            _run_bwd(xd, wd, dyd, groups, stride, dtype, dx=dx2, accumulate=acc)
        torch.cuda.synchronize()
        if with_dx:
            assert torch.equal(dx, dx2), "%s: dx differs between two launches" % cid
            _outside_untouched(cid + " dx", dx)
            want = d["dxr"] + d["prefill"].double() if acc else d["dxr"]
            if not acc:
                _none_kept(cid + " dx", dx)
            _hold(cid + " dx", dx, want, ydt, ybits, ratios, "dx")
            if sparse and not acc:
                _exact_zeros(cid + " dx", dx, d["dxr"])
        if with_dw:
            got = (dw.cpu() - d["dw0"]).view(OC, 3, 3, Cg).permute(0, 3, 1, 2)
            _hold(cid + " dw", got, d["dwr"], dtype, None, ratios, "dw")
            if sparse:
                _exact_zeros(cid + " dw", got, d["dwr"])
        else:
            assert torch.equal(dw, dw0), "%s: dw was written by a call that was not given it" % cid
        if with_db:
            got = db.cpu() - d["db0"]
            _hold(cid + " dbias", got, d["dbr"], dtype, None, ratios, "dbias")
            if sparse:
                _exact_zeros(cid + " dbias", got, d["dbr"])
        else:
            assert torch.equal(db, db0), "%s: dbias was written by a call that was not given it" % cid
        assert torch.equal(_whole(dyd), dy_before), "%s: dy was written" % cid
    assert torch.equal(_whole(xd), x_before) and torch.equal(wd, w_before), "%s: an operand was written" % cid
    hit = [name for name, pred in fc.GCONV_REGIMES if pred(case)]
    LINES.append("  %-13s %s | %s" % (cid, "  ".join("%s %.3f" % kv for kv in ratios.items()), "; ".join(hit)))


def test_gconv_refusals_launch_nothing():
    """outside the domain of gconv_in_domain: an error from the entry point's checks, in front of any launch"""
    init(F32)
    L = _lib.lib()
    st = ctx().stream
    N, H, W, C, OC, g = 2, 8, 8, 16, 16, 4
    buf = torch.zeros(N * H * W * 32, device="cuda")
    stats = torch.zeros(8 * 2 * 32, dtype=torch.float64, device="cuda")
    before, sb = buf.clone(), stats.clone()
    p = _P(buf)

    def fwd(C=C, ldin=C, in_bs=H * W * C, OC=OC, ldout=OC, out_bs=H * W * OC, OH=H, OW=W, stride=1, groups=g, bn=None, dtype=F32):
        L.call("emrt_gconv2d", p, p, p, None, N, H, W, C, ldin, in_bs, OH, OW, OC, ldout, out_bs, stride, groups, 0, bn, None, dtype, st)

    with pytest.raises(EmrtHipError, match="output channels per group"):
        fwd(OC=24, ldout=24, out_bs=H * W * 24)          # Og = 6
    with pytest.raises(EmrtHipError, match="multiples of 8"):
        fwd(ldin=20, in_bs=H * W * 20)
    with pytest.raises(EmrtHipError, match="stride must be 1 or 2"):
        fwd(stride=3, OH=3, OW=3, out_bs=3 * 3 * OC)
    with pytest.raises(EmrtHipError, match="strides smaller than the map"):
        fwd(in_bs=H * W * C - 8)
    with pytest.raises(EmrtHipError, match="strides smaller than the map"):
        fwd(out_bs=H * W * OC - 4)
    with pytest.raises(EmrtHipError, match="inference-only"):
        fwd(bn=_P(stats), dtype=F16)
    with pytest.raises(EmrtHipError, match="inference-only"):
        L.call("emrt_gconv2d_bwd", p, p, p, p, C, H * W * C, 0, p, p, N, H, W, C, C, H * W * C, H, W, OC, OC, H * W * OC, 1, g, F16, st)
    with pytest.raises(EmrtHipError, match="at least the map"):
        L.call("emrt_gconv2d_bwd", p, p, p, p, C, H * W * C, 0, None, None, N, H, W, C, C, H * W * C, H, W, OC, OC, H * W * OC - 4, 1, g, F32, st)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and torch.equal(stats, sb)


# ---------------------------------------------------------------------------------------------------------------------------------
# the wrapper: hnn.Conv2D(groups=g, bias=True) -> functional.gconv2d under a Tape
# ---------------------------------------------------------------------------------------------------------------------------------
def _layer(cin, cout, groups, stride, g, dtype):
    conv = hnn.Conv2D(cin, cout, 3, stride, 1, bias=True, groups=groups)
    with torch.no_grad():
        conv.weight.copy_(_rounded(torch.randn(cout, cin // groups, 3, 3, generator=g) / math.sqrt(9 * cin // groups), dtype))
        conv.bias.copy_(torch.randn(cout, generator=g))
    return conv, conv.weight.detach().clone().double(), conv.bias.detach().clone().double()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_gconv_wrapper_biased_relu_layer_on_a_channel_slice(dtype):
    """3 groups of 4 channels read from a slice of a 16-channel buffer, bias, relu=True: y, dx, weight.grad and bias.grad against float64.  The
    backward masks dy by the DEVICE's y (emrt_mask_bwd), so no pre-activation may lie within the forward bound of zero: redrawn until none does."""
    c = init(dtype)
    N, H, W, groups, Cg, Og = 2, 9, 7, 3, 4, 8
    C, OC = groups * Cg, groups * Og
    out_bits = None if dtype == F32 else 8
    for k in range(REDRAWS):
        g = torch.Generator().manual_seed(4100 + k)
        conv, w64, b64 = _layer(C, OC, groups, 1, g, dtype)
        x = _rounded(torch.randn(N, H, W, C, generator=g), dtype)
        dyh = _rounded(torch.randn(N, H, W, OC, generator=g), dtype)
        xr, wr, br = x.permute(0, 3, 1, 2).double().requires_grad_(True), w64.requires_grad_(True), b64.requires_grad_(True)
        pre = F.conv2d(xr, wr, br, padding=1, groups=groups)
        yr = torch.relu(pre)
        if _clear_of_zero(pre.detach(), yr.detach(), dtype, out_bits):
            break
    else:
        raise AssertionError("no draw keeps every pre-activation outside the forward bound of zero")
    yr.backward(dyh.permute(0, 3, 1, 2).double())
    Holder(conv=conv).place()
    wide = _padded(x, 16, dtype)          # channels 12..15 of every pixel belong to somebody else
    assert wide.stride(2) == 16
    tape = Tape()
    c.tape = tape
    y = conv(wide, relu=True)
    c.tape = None
    tape.watch(wide)
    tape.add_grad(y, dyh.to(device="cuda", dtype=_TD[dtype]))
    tape.backward()
    dx = tape.result(wide)
    torch.cuda.synchronize()
    close_gemm("wrapper y", y, yr.detach().permute(0, 2, 3, 1), dtype, out_bits=out_bits)
    close_gemm("wrapper dx", dx, xr.grad.permute(0, 2, 3, 1), dtype, out_bits=out_bits)
    close_gemm("wrapper weight.grad", conv.weight.grad.float().cpu(), wr.grad, dtype)
    close_gemm("wrapper bias.grad", conv.bias.grad.float().cpu(), br.grad, dtype)
    assert float(_whole(wide).view(N, H, W, 16)[..., C:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_gconv_wrapper_two_layers_share_an_input(dtype):
    """one input, two grouped layers (8 groups of 4 -> 4, 4 groups of 8 -> 12): the backward that runs second finds the tape's gradient slot and
    accumulates into it (accumulate = 1); the summed dx against float64.  The layer recorded last runs its backward first and STORES its dx in the
    compute dtype; the other layer's kernel then reads it back, adds and rounds again.  Two stored roundings, so the bound is close_gemm's taken
    at the contribution stored first plus close_gemm's at the sum (with one rounding, as in the sweep's dx-accumulate cases whose starting
    contents are exact, the second term alone would do; in bf16 a sum that cancels carries the first term's half ulp of the larger addend)."""
    c = init(dtype)
    N, H, W, C = 2, 9, 7, 32
    g = torch.Generator().manual_seed(4200)
    a, wa, ba = _layer(C, 32, 8, 1, g, dtype)
    b, wb, bb = _layer(C, 48, 4, 1, g, dtype)
    x = _rounded(torch.randn(N, H, W, C, generator=g), dtype)
    dya, dyb = _rounded(torch.randn(N, H, W, 32, generator=g), dtype), _rounded(torch.randn(N, H, W, 48, generator=g), dtype)
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wa, wb, ba, bb = [t.requires_grad_(True) for t in (wa, wb, ba, bb)]
    ya, yb = F.conv2d(xr, wa, ba, padding=1, groups=8), F.conv2d(xr, wb, bb, padding=1, groups=4)
    dxb_r, = torch.autograd.grad((yb * dyb.permute(0, 3, 1, 2).double()).sum(), xr, retain_graph=True)          # the second layer's share of dx alone
    (ya * dya.permute(0, 3, 1, 2).double()).sum().add((yb * dyb.permute(0, 3, 1, 2).double()).sum()).backward()
    Holder(a=a, b=b).place()
    xd = x.to(device="cuda", dtype=_TD[dtype])
    tape = Tape()
    c.tape = tape
    outa, outb = a(xd), b(xd)
    c.tape = None
    tape.watch(xd)
    tape.add_grad(outa, dya.to(device="cuda", dtype=_TD[dtype]))
    tape.add_grad(outb, dyb.to(device="cuda", dtype=_TD[dtype]))
    tape.backward()
    dx = tape.result(xd)
    torch.cuda.synchronize()
    out_bits = None if dtype == F32 else 8
    close_gemm("shared input: y of the first layer", outa, ya.detach().permute(0, 2, 3, 1), dtype, out_bits=out_bits)
    close_gemm("shared input: y of the second layer", outb, yb.detach().permute(0, 2, 3, 1), dtype, out_bits=out_bits)
    want = xr.grad.permute(0, 2, 3, 1).float()
    bound = _bound(dxb_r.permute(0, 2, 3, 1), dtype, out_bits) + _bound(want, dtype, out_bits)
    err = (dx.float().cpu() - want).abs()
    print("    shared input: summed dx error / bound %.3f" % _ratio(err, bound))
    assert bool(torch.isfinite(dx.float()).all()) and bool((err <= bound).all()), "summed dx: %d of %d elements beyond the two-rounding bound, worst error / bound %.3f" % (
        int((err > bound).sum()), err.numel(), _ratio(err, bound))
    for name, layer, wref, bref in (("first", a, wa, ba), ("second", b, wb, bb)):
        close_gemm("shared input: weight.grad of the %s layer" % name, layer.weight.grad.float().cpu(), wref.grad, dtype)
        close_gemm("shared input: bias.grad of the %s layer" % name, layer.bias.grad.float().cpu(), bref.grad, dtype)
