"""Helpers for the -m gpu parity tests: host<->device layout conversion and a tiny parameter store for single layers."""
import contextlib
import fcntl
import math
import os
import tempfile

import pytest
import torch
import torch.nn as tnn

from emrt_amd import nn as hnn
from emrt_amd.runtime import ctx, F32, BF16, Tape

TOL = {F32: dict(atol=2e-4, rtol=2e-4), BF16: dict(atol=6e-2, rtol=6e-2)}


def init(dtype, seed=0):
    c = ctx()
    c.init_device("cuda:0", dtype, seed)
    c.ensure_scratch()          # (a training context: the model's train-mode forward does this; bf16 only)
    c.training = True
    c.tape = None
    c.world_size = 1
    return c


def dev_map(t_nchw, dtype=None):
    """CPU [N,C,H,W] float -> device [N,H,W,C] in the compute dtype."""
    c = ctx()
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(device=c.device, dtype=dtype or c.tdtype)


def host_map(t_nhwc):
    return t_nhwc.float().cpu().permute(0, 3, 1, 2).contiguous()


def dev(t, dtype=None):
    c = ctx()
    return t.contiguous().to(device=c.device, dtype=dtype or c.tdtype)


def host(t):
    return t.float().cpu()


def rnd(x):
    """Round a CPU fp32 tensor through the compute dtype so CPU reference and GPU kernel see identical inputs."""
    return x.to(ctx().tdtype).float()


class Holder(tnn.Module):
    """Wraps HIP layers so ParamStore / bind_all can place their parameters on the device."""

    def __init__(self, **layers):
        super().__init__()
        for k, v in layers.items():
            self.add_module(k, v)

    def place(self):
        c = ctx()
        self.store = hnn.ParamStore(self, c.device, c.dtype)
        hnn.bind_all(self, self.store)
        self.store.pack()
        return self


def close(name, got, ref, dtype, scale=1.0, atol=None, rtol=None):
    tol = dict(TOL[dtype])
    if atol is not None:
        tol["atol"] = atol
    if rtol is not None:
        tol["rtol"] = rtol
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bound = tol["atol"] * scale + tol["rtol"] * ref.abs()
    bad = err > bound
    if bad.any():
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s: %d/%d elements off; max |diff| %.4g (ref max %.4g); first at %s got %.6g ref %.6g" % (
            name, int(bad.sum()), bad.numel(), err.max().item(), ref.abs().max().item(), idx,
            got[tuple(idx)].item(), ref[tuple(idx)].item()))
    assert torch.isfinite(got).all(), "%s: non-finite values" % name


def close_gemm(name, got, ref, dtype, out_bits=None):
    """Tolerance of a GEMM-shaped kernel (convolution / linear forward, data gradient, weight gradient) from what can actually differ, instead of
    the flat 6e-2 of TOL[BF16].  The reference is fp32 torch on the SAME rounded operands, the kernel multiplies them exactly (bf16 x bf16 fits
    fp32) and accumulates in fp32, so the only differences are
      * the rounding of the stored result: 2^-9 relative for a bf16 output (out_bits = 8 significant bits), none for an fp32 output;
      * the fp32 summation order over the contraction: ~2^-23 sqrt(K) of the terms' magnitude, i.e. parts in 10^5..10^6 of the output's RMS.
    bound = 2^-out_bits |ref| + 2^-(out_bits + 2) rms(ref) for a rounded output (twice the rounding; the RMS floor covers outputs that cancel to
    ~0), 2^-12 (|ref| + rms(ref)) for an fp32 output (fp32 atomics / split reductions in any order).  A mis-weighted tap of a 3x3 kernel moves an
    output by ~rms(ref) / 3: 40 to 100 times these bounds (the flat tolerance let it pass at kernel level)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "%s: non-finite values" % name
    rms = ref.pow(2).mean().sqrt().item()
    if dtype == F32:
        bound = 2e-4 * ref.abs() + 2e-4 * max(rms, 1e-30)
    elif out_bits is None:          # fp32 output of bf16 operands
        bound = 2.0 ** -12 * (ref.abs() + rms)
    else:
        bound = 2.0 ** -out_bits * ref.abs() + 2.0 ** -(out_bits + 2) * rms
    err = (got - ref).abs()
    bad = err > bound
    if bad.any():
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s: %d/%d elements beyond the contraction-derived bound; max |diff| %.4g at rms(ref) %.4g; first at %s got %.6g ref %.6g" % (
            name, int(bad.sum()), bad.numel(), err.max().item(), rms, idx, got[tuple(idx)].item(), ref[tuple(idx)].item()))


# ---------------------------------------------------------------------------------------------------------------------------------
# float16 kernel parity (tests/test_gpu_fp16_kernels.py).  References are float64 torch on the CPU, computed from operands that were
# already rounded through float16, so kernel and reference see identical inputs; what may differ is (a) the ONE rounding of the stored
# result, at most half a float16 ulp of the exact value, and (b) the kernel's fp32 arithmetic in front of it, bounded by `slack`.
# ---------------------------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24          # unit round-off of fp32
F16_MAX = 65504.0
F16_INF_FROM = 65520.0      # |x| >= this rounds to inf in float16 (round to nearest even: half way between 65504 and 2^16)
SLACK_USE = []              # (name, worst (err - ulp/2) / slack) of every close_f16 call of this process, in call order


def ulp16(x):
    """Spacing of float16 at |x| (float64 tensor): 2^(e - 10) in the binade [2^e, 2^(e + 1)), 2^-24 below 2^-14 (subnormals), 32 from 2^15 up."""
    a = x.abs().double().clamp(2.0 ** -14, 2.0 ** 15)
    _, ex = torch.frexp(a)                                   # a = m * 2^ex with m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), ex - 11)


def ulp32(x):
    a = x.abs().double().clamp_min(2.0 ** -126)
    _, ex = torch.frexp(a)
    return torch.ldexp(torch.ones_like(a), ex - 24)


def round16(x):
    """float64 -> nearest float16 value (ties to even, overflow to inf from 65520), as float64.  Done on the float16 grid directly:
    a float64 -> float32 -> float16 cast chain would round twice."""
    x = x.double()
    u = ulp16(x)
    r = torch.round(x / u) * u                               # torch.round: half to even
    return torch.where(r.abs() >= 65536.0, torch.sign(x) * float("inf"), r)


def gemm_slack(K, sq):
    """fp32 accumulation error of a contraction of length K.  sq = the same operator applied to the SQUARED operands (float64), i.e. the sum
    of the squared terms of each output.  K roundings of relative size <= 2^-24 on partial sums of random-sign terms walk sqrt(K) * 2^-24 *
    sqrt(sum of squared terms); 8 is the margin.  (The worst-case bound K * 2^-24 * sum |terms| is 1 to 126 float16 ulps at K = 64..13 824 and
    would hide a wrong rounding of the result: not used.)"""
    return 8.0 * math.sqrt(K) * EPS32 * sq.double().clamp_min(0).sqrt()


def terms_slack(*terms):
    """The same bound for a kernel whose output is a short fp32 expression of K = len(terms) terms (interpolation, pooling, elementwise,
    an epilogue): 8 sqrt(K) 2^-24 sqrt(sum of the squared terms).  Terms are float64 tensors broadcastable to the output."""
    sq = None
    for t in terms:
        sq = t.double() ** 2 if sq is None else sq + t.double() ** 2
    return 8.0 * math.sqrt(len(terms)) * EPS32 * sq.sqrt()


def close_f16(name, got, ref64, slack, out_f32=False):
    """Elementwise |got - ref64| <= ulp16(ref64) / 2 + slack (ulp32 for an fp32 output of a float16 kernel).  `slack` bounds the kernel's fp32
    arithmetic only and comes from the reference (gemm_slack / terms_slack / a derived term the caller documents), never from a measured error.
    Overflow: got is inf (of ref64's sign) exactly where ref64 rounds to inf in float16, finite elsewhere; only within `slack` of the
    threshold 65520 either is accepted.  Prints and records the worst (err - ulp / 2) / slack; returns it."""
    got = got.detach().double().cpu()
    ref64 = ref64.detach().double().cpu()
    slack = torch.as_tensor(slack, dtype=torch.float64).expand_as(ref64) if not torch.is_tensor(slack) else slack.double().expand_as(ref64)
    assert got.shape == ref64.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(ref64.shape))
    assert not torch.isnan(got).any(), "%s: NaN in the output" % name
    half = 0.5 * (ulp32(ref64) if out_f32 else ulp16(ref64))
    if out_f32:
        finite = torch.ones_like(ref64, dtype=torch.bool)
        assert torch.isfinite(got).all(), "%s: non-finite fp32 output" % name
    else:
        over = ref64.abs() >= F16_INF_FROM
        band = (ref64.abs() - F16_INF_FROM).abs() <= slack
        ginf = torch.isinf(got)
        wrong = (ginf != over) & ~band
        if wrong.any():
            idx = tuple(torch.nonzero(wrong)[0].tolist())
            raise AssertionError("%s: %d outputs overflow on one side only; first at %s got %r ref %r" % (
                name, int(wrong.sum()), idx, got[idx].item(), ref64[idx].item()))
        both = ginf & over
        assert (torch.sign(got[both]) == torch.sign(ref64[both])).all(), "%s: inf of the wrong sign" % name
        finite = ~ginf & ~over
    err = (got - ref64).abs()
    excess = torch.where(finite, err - half, torch.zeros_like(err))
    use = torch.where(slack > 0, excess / slack.clamp_min(1e-300), torch.where(excess > 0, torch.full_like(excess, float("inf")), torch.zeros_like(excess)))
    worst = use.max().item() if use.numel() else 0.0
    SLACK_USE.append((name, worst))
    print("[close_f16] %-44s n=%-9d worst (err - ulp/2) / slack = %+.3f" % (name, ref64.numel(), worst))
    bad = finite & (excess > slack)
    if bad.any():
        idx = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError("%s: %d/%d outputs beyond ulp16/2 + slack; worst excess / slack %.3g; first at %s got %.9g ref %.9g (ulp/2 %.3g, slack %.3g)" % (
            name, int(bad.sum()), bad.numel(), worst, idx, got[idx].item(), ref64[idx].item(), half[idx].item(), slack[idx].item()))
    return worst


def rounding_is_nearest(name, got, ref64):
    """A result rounded to nearest errs uniformly in +-ulp/2: over the outputs with |ref64| >= rms(ref64) / 4 the mean of (|got| - |ref64|) /
    ulp16 is within 6 standard errors (0.289 / sqrt(n)) of zero.  Truncation (round toward zero) sits at -0.5.  Needs n >= 1e5 outputs after
    the filter (enlarge the case, not the bound).  Returns the mean."""
    got = got.detach().double().cpu().reshape(-1)
    ref64 = ref64.detach().double().cpu().reshape(-1)
    rms = ref64.pow(2).mean().sqrt()
    sel = (ref64.abs() >= rms / 4) & (ref64.abs() < F16_MAX) & torch.isfinite(got)
    n = int(sel.sum())
    assert n >= 100000, "%s: %d outputs after the filter, need 1e5" % (name, n)
    bias = ((got[sel].abs() - ref64[sel].abs()) / ulp16(ref64[sel])).mean().item()
    bound = 6 * 0.289 / math.sqrt(n)
    print("[rounding_is_nearest] %-34s n=%d mean signed error %+.5f ulp16 (bound %.5f)" % (name, n, bias, bound))
    assert abs(bias) <= bound, "%s: mean of (|got| - |ref|) / ulp16 = %+.5f over %d outputs, bound %.5f (truncation gives -0.5)" % (name, bias, n, bound)
    return bias


# Processes that may hold the GPU at one time while the suite runs: the test workers (each one opens the device) and the rank processes of a
# multi-rank test together (every rank of these tests runs on GPU 0).  The GPU test hosts stop a run in which more than 6 processes hold a
# GPU at once, hence the default cap; EMRT_TEST_MAX_GPU_PROCS sets another where the host allows more.  Rank processes of different tests
# never overlap (a lock file shared by the workers of this user), and a test whose ranks do not fit beside the workers under the cap skips
# before it starts any of them.
MAX_GPU_PROCS = int(os.environ.get("EMRT_TEST_MAX_GPU_PROCS", "6"))


@contextlib.contextmanager
def rank_processes(world):
    """Wraps the start and the whole lifetime of one test's `world` rank processes."""
    workers = max(1, int(os.environ.get("PYTEST_XDIST_WORKER_COUNT", "1")))
    if workers + world > MAX_GPU_PROCS:
        pytest.skip("%d rank processes on GPU 0 beside %d test worker(s) would hold the GPU in %d processes at once, above the cap of %d "
                    "(EMRT_TEST_MAX_GPU_PROCS)" % (world, workers, workers + world, MAX_GPU_PROCS))
    path = os.path.join(tempfile.gettempdir(), "emrt_test_rank_processes.%d.lock" % os.getuid())
    with open(path, "a") as f:
        fcntl.flock(f, fcntl.LOCK_EX)
        try:
            yield
        finally:
            fcntl.flock(f, fcntl.LOCK_UN)
