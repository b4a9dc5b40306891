"""-m gpu: the small streaming kernels of csrc/elementwise.hip, called directly through the C ABI, over fuzz_cases.CASES["elementwise"]:
emrt_add, emrt_add_f32row, emrt_add_f32row_levels, emrt_add3d, emrt_acc3d, emrt_concat_tokens (both directions), emrt_cast (both directions),
emrt_sigmoid_fwd / _bwd and the memcpy_kernel = 1 arm of emrt_memcpy, in fp32, bf16 and float16 where the entry point takes them.

Sizes: one lane, 255 / 256 / 257 lanes (a block is 256), and for every kernel one case one lane past ew_grid's 8192 blocks (2048 for the copy
kernel), which sends the grid-stride loop round a second time.  Periods that equal n, are 4, divide n and do not divide n; 1 to 4 levels with
a level of one row in every position; token slabs and channel slices on each side of emrt_add3d / emrt_acc3d in turn and on all at once, with
B = 1 and with rows = 1; 1, 4 and 8 parts with a part of one token first, last and in the middle.

Expected values.  An add kernel loads its operands to fp32, adds once and rounds once to the type: the torch fp32 expression on the same
(already rounded) operands, rounded once with Tensor.to, has the same one answer, so every comparison is BIT FOR BIT (NaN compared with
isnan); the moves (concat, split, cast to fp32, copy) are exact by definition and the cast from fp32 is Tensor.to.  Every output lies in a
buffer pre-filled with a sentinel, and the whole buffer is compared: nothing outside the destination view changes.

The sigmoid is the one kernel with a bound, derived from its fp32 operations (sigmoid_fwd_kernel: y = 1.f / (1.f + __expf(-x))):
  * __expf(-x) is exp2(fl(c * -x)) with c = fl(log2 e) = 0x1.715476p+0: c is off log2 e by 0.24 x 2^-24 relative (a known constant), the
    product is rounded once (2^-24), and both errors sit in the exponent: relative error |x| ln 2 log2 e (0.24 + 1) 2^-24 = |x| ARG_ERR in
    e, plus the hardware exp2's own error of EXP_ULPS ulps = EXP_ULPS 2^-23 relative;
  * d = fl(1 + e) and y = fl(1 / d) (IEEE division: the library is built without fast-math) add 2^-24 each; an error of e reaches y
    multiplied by e / (1 + e) = 1 - y;
  so |y_dev - y| <= y ((1 - y) (EXP_ULPS 2^-23 + |x| ARG_ERR) + 2^-23) (1 + 2^-20) + 2^-126; the last term is for x < -87, where e
  overflows or y is below the smallest normal number.
EXP_ULPS cannot be derived and no document shipped with the toolchain states it.  Measured on an MI355X as the exp2 error that the device's
error against the float64 reference would need beyond the derived terms, over every swept input with e >= 1 (x <= 0, where the term is not
divided by a vanishing 1 - y): at most -0.044 ulps (at x = -0.0178; -s prints it), i.e. the two roundings and the argument error already
explain every error seen.  A maximum over finitely many points has no headroom of its own, and an exp2 is not exact, so the bound does not
rest on it: EXP_ULPS is the 1 ulp that the CDNA instruction-set reference gives for V_EXP_F32 (more than twice anything measured).  With
it every term of the bound is a worst case of the operation it stands for: the bound is sound, it holds for any inputs and any schedule of
the expression, not only at the swept points.  A kernel with the wrong sign or without the `1 +` is off by orders of magnitude.
Backward: dx = dy * y * (1 - y) in fp32 is three roundings: 3 fp32 ulps of the float64 value (plus 2^-126 where the product is subnormal).

The 64-bit index branches (n4 | period4 > 2^32 in the add kernels, unravel3's in add3d / acc3d / concat) need more than 2^32 elements and
stay unexercised here.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                    # noqa: E402
from emrt_amd.functional import P                            # noqa: E402
from emrt_amd.runtime import F32, BF16, F16                  # noqa: E402
from tests import fuzz_cases as fc                           # noqa: E402
from tests.hip_utils import init, ulp32                      # noqa: E402

CODE = {"f32": F32, "bf16": BF16, "f16": F16}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = 7.0
GUARD = 8
LOG2E_F32 = float(torch.tensor(math.log2(math.e), dtype=torch.float32))          # 0x1.715476p+0, the constant of __expf
ARG_ERR = abs(LOG2E_F32 - math.log2(math.e)) / math.log2(math.e) + 2.0 ** -24          # relative error of fl(c * x) against x log2 e: 1.24 x 2^-24
EXP_ULPS_MEASURED = -0.044          # the largest exp2 error, in ulps, needed to explain the device's error beyond the derived terms (MI355X)
EXP_ULPS = 1.0                      # V_EXP_F32's documented accuracy; >= 2 max(EXP_ULPS_MEASURED, 0)
SEEN = {}          # the measurement behind EXP_ULPS_MEASURED, printed at the end of a run (-s)


def _cases(*kernels):
    cs = [c for c in fc.CASES["elementwise"] if c[1] in kernels]
    return pytest.mark.parametrize("case", cs, ids=[c[0] for c in cs])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if SEEN:
        print("\n[elementwise sweep] sigmoid forward: largest exp2 error that explains the device's, in ulps: %.3f (at x = %.4f)" % (SEEN["k"], SEEN["x"]))


def _ctx(d):
    c = init(CODE[d])
    c.training = False
    return c


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(name, got, want):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape
    nan = torch.isnan(want) if want.is_floating_point() else torch.zeros(want.shape, dtype=torch.bool)
    if nan.any():
        assert torch.equal(torch.isnan(got), nan), "%s: NaNs in other places" % name
        got, want = torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want)
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), "%s: %d of %d elements differ bit for bit; first at %s: got %r, want %r" % (
        name, int(bad.sum()), bad.numel(), torch.nonzero(bad)[0].tolist(), got[bad][0].item(), want[bad][0].item())


def _rand(shape, g, T, scale=2.0):
    return (torch.randn(shape, generator=g) * scale).to(T)


def _guarded(n, T):
    """device [n + GUARD] filled with the sentinel; the kernel gets the first n"""
    return torch.full((n + GUARD,), SENTINEL, dtype=T, device="cuda")


def _gen(case):
    return torch.Generator().manual_seed(case[-1])


# ---- emrt_add / emrt_add_f32row ------------------------------------------------------------------------------------------------
@_cases("add", "add_f32row")
def test_add_periods(case):
    cid, k, d, (n, period), _, _ = case
    c, T, g = _ctx(d), TORCH[d], _gen(case)
    a = _rand(n, g, T)
    b = _rand(period, g, T) if k == "add" else torch.randn(period, generator=g)
    idx = torch.arange(n) % period
    want = (a.float() + b.float()[idx]).to(T)
    ad, bd, out = a.cuda(), b.cuda(), _guarded(n, T)
    _lib.lib().call("emrt_add" if k == "add" else "emrt_add_f32row", P(ad), P(bd), P(out), n, period, CODE[d], c.stream)
    torch.cuda.synchronize()
    _same(cid, out, torch.cat([want, torch.full((GUARD,), SENTINEL, dtype=T)]))


# ---- emrt_add_f32row_levels ----------------------------------------------------------------------------------------------------
@_cases("levels")
def test_add_f32row_levels(case):
    cid, _, d, (sizes, C), _, _ = case
    c, T, g = _ctx(d), TORCH[d], _gen(case)
    Lv, L = sum(sizes), len(sizes)
    a, rows = _rand((Lv, C), g, T), torch.randn(L, C, generator=g)
    starts = [sum(sizes[:l]) for l in range(L)]
    want = torch.empty_like(a)
    for l, (s0, n) in enumerate(zip(starts, sizes)):          # the per-level expression
        want[s0:s0 + n] = (a[s0:s0 + n].float() + rows[l]).to(T)
    ad, rd, out = a.cuda(), rows.cuda(), _guarded(Lv * C, T)
    arr = (ctypes.c_int * L)(*starts)
    _lib.lib().call("emrt_add_f32row_levels", P(ad), P(rd), P(out), arr, L, Lv, C, CODE[d], c.stream)
    torch.cuda.synchronize()
    _same(cid, out, torch.cat([want.reshape(-1), torch.full((GUARD,), SENTINEL, dtype=T)]))


# ---- emrt_add3d / emrt_acc3d ---------------------------------------------------------------------------------------------------
def _view(kind, B, rows, cols, T, g):
    """(flat CPU buffer of random values with GUARD trailing elements, offset, batch stride, row stride) of a [B, rows, cols] view"""
    if kind == "dense":
        off, bs, rs = 0, rows * cols, cols
    elif kind == "slab":          # tokens [:, 3:3 + rows] of [B, rows + 5, cols]
        off, bs, rs = 3 * cols, (rows + 5) * cols, cols
    else:                         # channels [4:4 + cols] of a [B, rows, cols + 8] map
        off, bs, rs = 4, rows * (cols + 8), cols + 8
    return _rand(B * bs + GUARD, g, T), off, bs, rs


def _strided(flat, off, bs, rs, B, rows, cols):
    return torch.as_strided(flat, (B, rows, cols), (bs, rs, 1), off)


@_cases("add3d", "acc3d")
def test_add3d_acc3d_views(case):
    cid, k, d, shape, _, _ = case
    c, T, g = _ctx(d), TORCH[d], _gen(case)
    B, rows, cols = shape[:3]
    ops = [_view(kind, B, rows, cols, T, g) for kind in shape[3:]]
    host = [_strided(flat, off, bs, rs, B, rows, cols) for flat, off, bs, rs in ops]
    dev_flat = [flat.cuda() for flat, _, _, _ in ops]
    dev = [_strided(df, off, bs, rs, B, rows, cols) for df, (_, off, bs, rs) in zip(dev_flat, ops)]
    want_flat = ops[-1][0].clone() if k == "add3d" else ops[0][0].clone()          # the destination's buffer: its view changes, nothing else
    if k == "add3d":          # out = a + b; the destination's old (random, non-zero) contents are overwritten
        res = (host[0].float() + host[1].float()).to(T)
        _strided(want_flat, *ops[2][1:], B, rows, cols).copy_(res)
        _lib.lib().call("emrt_add3d", P(dev[0]), ops[0][2], ops[0][3], P(dev[1]), ops[1][2], ops[1][3], P(dev[2]), ops[2][2], ops[2][3], B, rows, cols,
                        CODE[d], c.stream)
        got = dev_flat[2]
    else:                     # dst += src into a non-zero destination
        res = (host[0].float() + host[1].float()).to(T)
        _strided(want_flat, *ops[0][1:], B, rows, cols).copy_(res)
        _lib.lib().call("emrt_acc3d", P(dev[0]), ops[0][2], ops[0][3], P(dev[1]), ops[1][2], ops[1][3], B, rows, cols, CODE[d], c.stream)
        got = dev_flat[0]
    torch.cuda.synchronize()
    _same(cid, got, want_flat)
    for i, (df, (flat, _, _, _)) in enumerate(zip(dev_flat, ops)):          # the sources are read only
        if df is not got:
            _same("%s operand %d" % (cid, i), df, flat)


# ---- emrt_concat_tokens --------------------------------------------------------------------------------------------------------
@_cases("concat", "split")
def test_concat_tokens_and_split(case):
    cid, k, d, (B, C, ns), _, _ = case
    c, T, g = _ctx(d), TORCH[d], _gen(case)
    total, np_ = sum(ns), len(ns)
    sent = torch.full((GUARD,), SENTINEL, dtype=T)
    if k == "concat":
        parts = [_rand((B, n, C), g, T) for n in ns]
        pd = [p_.cuda() for p_ in parts]
        whole = _guarded(B * total * C, T)
        _lib.lib().call("emrt_concat_tokens", (ctypes.c_void_p * np_)(*[t.data_ptr() for t in pd]), (ctypes.c_int * np_)(*ns), np_, P(whole), B, C, 0,
                        CODE[d], c.stream)
        torch.cuda.synchronize()
        _same(cid, whole, torch.cat([torch.cat(parts, 1).reshape(-1), sent]))
        for got, p_ in zip(pd, parts):
            _same(cid + " part", got, p_)
    else:
        whole = _rand((B, total, C), g, T)
        wd = whole.cuda()
        back = [_guarded(B * n * C, T) for n in ns]
        _lib.lib().call("emrt_concat_tokens", (ctypes.c_void_p * np_)(*[t.data_ptr() for t in back]), (ctypes.c_int * np_)(*ns), np_, P(wd), B, C, 1,
                        CODE[d], c.stream)
        torch.cuda.synchronize()
        s0 = 0
        for got, n in zip(back, ns):
            _same("%s part at token %d" % (cid, s0), got, torch.cat([whole[:, s0:s0 + n].reshape(-1), sent]))
            s0 += n
        _same(cid + " whole", wd, whole)


# ---- emrt_cast -----------------------------------------------------------------------------------------------------------------
CAST_SPECIALS = [
    0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1.0, -1.5, 3.14159274, 1e-3, -123456.789,
    1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2049.0, 2051.0,      # ties (and just past them)
    65504.0, 65519.99, 65520.0, -65520.0, 1e6, 3.3895313892515355e38, 3.3961775292304601e38, 3.4e38, -3.4e38,                                  # the largest values, overflow
    6.1e-5, 6.0e-5, 5.96e-8, 2.0 ** -25, 2.0 ** -25 * 1.0001, -2.0 ** -25, 2.0 ** -24, 3e-8, 1e-10,                                            # float16 subnormals
    1e-38, 1.1754942e-38, 9.1835e-41, 2.0 ** -133, 2.0 ** -134, 2.0 ** -134 * 1.0001, 2.0 ** -149,                                             # bfloat16 subnormals
]


def _cast_inputs(n, g):
    sp = torch.tensor(CAST_SPECIALS, dtype=torch.float32)
    if n <= len(CAST_SPECIALS):          # n = 1, 3: specials picked by the case's seed
        return sp[torch.randperm(len(CAST_SPECIALS), generator=g)[:n]]
    scale = torch.tensor([1.0, 1e-3, 1e3, 1e-6])[torch.randint(0, 4, (n - len(CAST_SPECIALS),), generator=g)]
    return torch.cat([sp, torch.randn(n - len(CAST_SPECIALS), generator=g) * scale])[torch.randperm(n, generator=g)]


@_cases("cast_to", "cast_from")
def test_cast_both_ways(case):
    cid, k, d, (n,), _, _ = case
    c, T, g = _ctx(d), TORCH[d], _gen(case)
    x = _cast_inputs(n, g)
    if k == "cast_to":
        src, want, To = x, x.to(T), T
    else:          # every special value as the narrow type holds it (its subnormals, infinities and NaN among them), widened exactly
        src, want, To = x.to(T), x.to(T).float(), torch.float32
    sd, out = src.cuda(), _guarded(n, To)
    _lib.lib().call("emrt_cast", P(sd), P(out), n, 0 if k == "cast_to" else 1, CODE[d], c.stream)
    torch.cuda.synchronize()
    _same(cid, out, torch.cat([want, torch.full((GUARD,), SENTINEL, dtype=To)]))


# ---- emrt_sigmoid_fwd / _bwd -----------------------------------------------------------------------------------------------------
def _sigmoid_x(n, g):
    if n == 2443:
        return torch.cat([torch.linspace(-30.0, 30.0, 2441), torch.tensor([100.0, -100.0])])
    if n == 1:
        return torch.tensor([0.3])
    if n <= 2441:
        return torch.linspace(-30.0, 30.0, n)
    return torch.rand(n, generator=g) * 60.0 - 30.0


@_cases("sigmoid_fwd")
def test_sigmoid_forward(case):
    cid, _, _, (n,), _, _ = case
    c, g = _ctx("f32"), _gen(case)
    x = _sigmoid_x(n, g)
    xd, out = x.cuda(), _guarded(n, torch.float32)
    _lib.lib().call("emrt_sigmoid_fwd", P(xd), P(out), n, c.stream)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[n:] == SENTINEL).all())
    x64 = x.double()
    y = 1.0 / (1.0 + torch.exp(-x64))
    err = (got[:n].double() - y).abs()
    # the exp2 error, in ulps, that would explain each element's error (only where e >= 1: see the module docstring)
    neg = x64 <= 0
    if bool(neg.any()):
        need = (((err / y / (1.0 + 2.0 ** -20) - 2.0 ** -23) / (1.0 - y) - x64.abs() * ARG_ERR) / 2.0 ** -23)[neg & (y > 2.0 ** -120)]
        if need.numel() and need.max().item() > SEEN.get("k", -1e9):
            SEEN["k"], SEEN["x"] = need.max().item(), x64[neg & (y > 2.0 ** -120)][need.argmax()].item()
        print("[elementwise sweep] %s: exp2 error needed %.3f ulps" % (cid, need.max().item() if need.numel() else float("nan")))
    bound = y * ((1.0 - y) * (EXP_ULPS * 2.0 ** -23 + x64.abs() * ARG_ERR) + 2.0 ** -23) * (1.0 + 2.0 ** -20) + 2.0 ** -126
    bad = err > bound
    assert not bool(bad.any()), "%s: %d elements beyond the derived bound; worst error / bound %.3f at x = %.5f" % (
        cid, int(bad.sum()), (err / bound).max().item(), x[(err / bound).argmax()].item())
    assert bool(((got[:n] >= 0) & (got[:n] <= 1)).all())


@_cases("sigmoid_bwd")
def test_sigmoid_backward(case):
    cid, _, _, (n,), _, _ = case
    c, g = _ctx("f32"), _gen(case)
    y = torch.sigmoid(_sigmoid_x(n, g))          # fp32 values in [0, 1], 1.0 and subnormals among them
    dy = torch.randn(n, generator=g) * 3.0
    yd, dyd, out = y.cuda(), dy.cuda(), _guarded(n, torch.float32)
    _lib.lib().call("emrt_sigmoid_bwd", P(yd), P(dyd), P(out), n, c.stream)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[n:] == SENTINEL).all())
    want = dy.double() * y.double() * (1.0 - y.double())
    err = (got[:n].double() - want).abs()
    bound = 3.0 * ulp32(want) + 2.0 ** -126
    assert bool((err <= bound).all()), "%s: worst error %.3g fp32 ulps at y = %.6g" % (cid, (err / ulp32(want)).max().item(), y[(err / bound).argmax()].item())


# ---- emrt_memcpy, memcpy_kernel = 1 ----------------------------------------------------------------------------------------------
@_cases("memcpy")
def test_memcpy_kernel_arm(case):
    cid, _, _, (nbytes, off), _, _ = case
    c, g = _ctx("f32"), _gen(case)
    src = torch.randint(0, 256, (nbytes + 64,), generator=g, dtype=torch.uint8)
    sd = src.cuda()
    dst = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    lo = 32 + off
    assert (sd.data_ptr() + lo) % 16 == off and (dst.data_ptr() + lo) % 16 == off
    L_ = _lib.lib()
    old = L_.set_tuning("memcpy_kernel", 1)
    try:
        L_.call("emrt_memcpy", ctypes.c_void_p(dst.data_ptr() + lo), ctypes.c_void_p(sd.data_ptr() + lo), nbytes, c.stream)
        torch.cuda.synchronize()
    finally:
        L_.set_tuning("memcpy_kernel", old)
    want = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8)
    want[lo:lo + nbytes] = src[lo:lo + nbytes]
    _same(cid, dst, want)
    _same(cid + " source", sd, src)


def test_the_sweep_has_every_kernel_of_the_file():
    assert {c[1] for c in fc.CASES["elementwise"]} == set(fc.EW_KERNELS) and EXP_ULPS >= 2.0 * max(EXP_ULPS_MEASURED, 0.0)
