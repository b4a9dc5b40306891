"""The attention kernels' operation (csrc/attn.hip: emrt_mha_fwd / emrt_mha_bwd) restated in float64, the error measure of the sweep in
tests/test_gpu_mha_fuzz.py, and the reference-side calibration of its bounds (tests/test_mha_reference_cpu.py).  No GPU and no library
import: everything here is plain torch on the CPU.

All tensors are [B, M, L, 32] (batch, head, row, head dim); scale = fp32(1 / sqrt(32)), as the kernels receive it.

  P = softmax(q k^T scale)            Pd = P mask / (1 - p)          o  = Pd v
  dP = (dy v^T) mask / (1 - p)        rowdot_i = sum_j dP_ij P_ij    dS = P (dP - rowdot) scale
  dq = dS k                           dk = dS^T q                    dv = Pd^T dy

Error measure: PER ROW, relative to the row of `magnitude` -- the same expressions with absolute values on both operands of every product
and P (|dP| + |rowdot|) in place of dS, which is what rounding errors scale with and which cannot cancel:
    err(b, m, i) = || got[b, m, i, :] - exact[b, m, i, :] ||_2 / || magnitude[b, m, i, :] ||_2 ,  maximised over rows.
Not relative to the result's own norm: with peaked scores dq and dk cancel to almost nothing (at L = 1 they are exactly 0).

Bounds (MHA_BOUND): constants, calibrated on the CPU only.  The floor of a dtype is the worst per-row error, over every case of the sweep
(tests/fuzz_cases.py, op "mha"), of the best a correct kernel can do:
  bf16: contract_bf16 -- the exact values with the MFMA kernels' stated roundings (Pd and dS rounded to bf16 as matrix operands, every
        output rounded to bf16; attn.hip, the comment above the MFMA kernels).  bound = 3 x floor: the model has every stated rounding, the
        factor covers fp32 accumulation order and __expf.
  fp32: evaluate_f32 -- the same chain in fp32 torch.  bound = 16 x floor: __expf rounds its argument (a relative |s - max| 2^-23 on the
        entries that carry mass, which torch's exp does not have) and the VALU kernels sum in another order than torch.
tests/test_mha_reference_cpu.py recomputes the floors and asserts floor <= bound / 3 (bf16), bound / 16 (fp32): an edit of a seed or a
regime that raises a floor fails there instead of silently loosening the GPU test.  It also asserts that the mutants below -- wrong on
purpose, each with one named cause -- exceed 2 x bound in the regime built for them.
"""
import math

import torch

F64 = torch.float64
D = 32
SCALE = float(torch.tensor(1.0 / math.sqrt(32.0), dtype=torch.float32))          # what functional.mha passes, as the C float the kernels see
TENSORS = ("o", "dq", "dk", "dv")
DTYPES = ("f32", "bf16")
REGIMES = ("ordinary", "peaked", "negative", "lastkey")

# Per-row error bounds of the GPU sweep.  floors measured by tests/test_mha_reference_cpu.py::test_floors_and_bounds over the sweep's cases
# (it prints them):            o        dq       dk       dv
#   bf16 contract floor     3.872e-3 6.941e-4 1.354e-3 4.133e-3       bound = 3 x floor, rounded up in the third digit
#   fp32 torch floor        2.550e-6 2.226e-7 6.452e-7 5.402e-6       bound = 16 x floor, rounded up in the second digit (the floor is a
#                                                                     maximum over fp32 sums whose order belongs to the BLAS underneath)
# (the fp32 floors of o and dv come from the negative regime: raw dot products of ~ -113 carry an fp32 error of ~1e-5 into the exponent)
MHA_BOUND = {
    "bf16": {"o": 1.17e-2, "dq": 2.09e-3, "dk": 4.07e-3, "dv": 1.25e-2},
    "f32": {"o": 4.2e-5, "dq": 3.7e-6, "dk": 1.1e-5, "dv": 8.9e-5},
}
FLOOR_MARGIN = {"bf16": 3.0, "f32": 16.0}


def round_to(x, dtype):
    """float64 values of x rounded through the compute dtype ('f32' | 'bf16'), as tests/hip_utils.rnd does"""
    t = x.to(torch.float32)
    if dtype == "bf16":
        t = t.to(torch.bfloat16)
    return t.to(F64)


def _bf(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def _ident(x):
    return x


def make_inputs(regime, B, M, L, seed, dtype):
    """q, k, v, dy in float64, every one rounded through `dtype`.
      ordinary: N(0, 1)
      peaked:   q, k x sqrt(5): score s.d. ~ 5 (the float16 test's regime)
      negative: q += a u, k -= a u, one random unit vector u per (batch, head), a^2 scale = 20: the scores lie around -20, so a padding
                column that enters with score 0 takes most of the row
      lastkey:  q += a u, k[L - 1] = a u, a^2 scale = min(6, L): the last key carries most of every row (and row L - 1 most of dk, dv), so
                losing the ragged tail is an O(1) error.  (Below L = 6 the shift is L, not 6: dq is proportional to P_i0 P_i1 at L = 2, and with
                a shift of 6 the last key takes 0.997 of the row -- a kernel that lost it, whose dq is exactly 0, would then be wrong by a
                sixth of the bf16 bound only.  With a shift of 2 the last key still takes 0.88 and the lost dq is 8 bounds.)"""
    g = torch.Generator().manual_seed(seed)
    q, k, v, dy = (torch.randn(B, M, L, D, generator=g, dtype=F64) for _ in range(4))
    u = torch.randn(B, M, 1, D, generator=g, dtype=F64)
    u = u / u.norm(dim=-1, keepdim=True)
    if regime == "peaked":
        q, k = q * math.sqrt(5.0), k * math.sqrt(5.0)
    elif regime == "negative":
        a = math.sqrt(20.0 / SCALE)
        q, k = q + a * u, k - a * u
    elif regime == "lastkey":
        a = math.sqrt(min(6.0, float(L)) / SCALE)
        q = q + a * u
        k = k.clone()
        k[:, :, L - 1:, :] = a * u
    else:
        assert regime == "ordinary", regime
    return tuple(round_to(t, dtype) for t in (q, k, v, dy))


def scores(q, k):
    return (q @ k.transpose(-1, -2)) * SCALE


def _keep(mask, p, like):
    if mask is None:
        assert p == 0.0
        return torch.ones((), dtype=like.dtype)
    return mask.to(like.dtype) / (1.0 - p)


def _chain(P, q, k, v, dy, keep_f, keep_b, r=_ident, ro=_ident):
    """o, dq, dk, dv from the probabilities P.  keep_f / keep_b: mask / (1 - p) as the forward / the backward sees it (the same tensor, except
    in the mask mutants); r: rounding of a matrix operand (Pd, dS), ro: rounding of an output."""
    o = ro(r(P * keep_f) @ v)
    dP = (dy @ v.transpose(-1, -2)) * keep_b
    rowdot = (dP * P).sum(-1, keepdim=True)
    dS = r(P * (dP - rowdot) * SCALE)
    return o, ro(dS @ k), ro(dS.transpose(-1, -2) @ q), ro(r(P * keep_b).transpose(-1, -2) @ dy)


def exact(q, k, v, dy, mask=None, p=0.0):
    """o, dq, dk, dv in float64.  mask: [B, M, L, L] of 0 / 1 (1 = kept), p: the dropout probability it was drawn with."""
    q, k, v, dy = (t.to(F64) for t in (q, k, v, dy))
    P = torch.softmax(scores(q, k), -1)
    kp = _keep(mask, p, P)
    return _chain(P, q, k, v, dy, kp, kp)


def magnitude(q, k, v, dy, mask=None, p=0.0):
    """what the rounding errors of o, dq, dk, dv scale with: |.| on both operands of every product, P (|dP| + |rowdot|) in place of dS"""
    q, k, v, dy = (t.to(F64) for t in (q, k, v, dy))
    P = torch.softmax(scores(q, k), -1)
    kp = _keep(mask, p, P)
    Pd = P * kp
    dP = (dy.abs() @ v.abs().transpose(-1, -2)) * kp
    rowdot = (dP * P).sum(-1, keepdim=True)
    dS = P * (dP + rowdot) * SCALE
    return Pd @ v.abs(), dS @ k.abs(), dS.transpose(-1, -2) @ q.abs(), Pd.transpose(-1, -2) @ dy.abs()


def contract_bf16(q, k, v, dy, mask=None, p=0.0):
    """the exact values with the MFMA kernels' stated roundings: the best a correct bf16 kernel can do"""
    q, k, v, dy = (t.to(F64) for t in (q, k, v, dy))
    P = torch.softmax(scores(q, k), -1)
    kp = _keep(mask, p, P)
    return _chain(P, q, k, v, dy, kp, kp, _bf, _bf)


def evaluate_f32(q, k, v, dy, mask=None, p=0.0):
    """the same chain in fp32 torch; returned as float64"""
    q, k, v, dy = (t.to(torch.float32) for t in (q, k, v, dy))
    P = torch.softmax((q @ k.transpose(-1, -2)) * SCALE, -1)
    kp = _keep(mask, p, P)
    return tuple(t.to(F64) for t in _chain(P, q, k, v, dy, kp, kp))


# ---- mutants: wrong on purpose, on the reference side only ----------------------------------------------------------------------
def drop_last_key(q, k, v, dy):
    """the softmax runs over keys 0 .. L - 2: a kernel that loses the ragged tail"""
    s = scores(q, k)
    assert s.shape[-1] >= 2
    P = torch.zeros_like(s)
    P[..., :-1] = torch.softmax(s[..., :-1], -1)
    one = torch.ones((), dtype=F64)
    return _chain(P, q, k, v, dy, one, one)


def pad_in_denominator(q, k, v, dy):
    """one extra key of score 0 and value 0 in the row maximum and the row sum: a padding column that is not masked out"""
    s = scores(q, k)
    mx = torch.clamp_min(s.max(-1, keepdim=True).values, 0.0)
    e = torch.exp(s - mx)
    P = e / (e.sum(-1, keepdim=True) + torch.exp(-mx))
    one = torch.ones((), dtype=F64)
    return _chain(P, q, k, v, dy, one, one)


def mask_transposed(q, k, v, dy, mask, p):
    """the backward uses mask[j][i] where the forward used mask[i][j]"""
    P = torch.softmax(scores(q, k), -1)
    return _chain(P, q, k, v, dy, _keep(mask, p, P), _keep(mask.transpose(-1, -2), p, P))


def mask_other_head(q, k, v, dy, mask, p):
    """the backward takes the mask of (b, m) from (b, (m + 1) mod M)"""
    P = torch.softmax(scores(q, k), -1)
    return _chain(P, q, k, v, dy, _keep(mask, p, P), _keep(torch.roll(mask, -1, 1), p, P))


def random_mask(B, M, L, p, seed):
    """a stand-in for the device's mask in the CPU calibration: i.i.d. keep with probability 1 - p"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, M, L, L, generator=g, dtype=F64) >= p).to(F64)


# ---- the measure ----------------------------------------------------------------------------------------------------------------
def row_errors(got, want, mag):
    """[B, M, L]: || got_row - want_row || / || magnitude_row ||; a row whose magnitude is 0 (every key dropped) must be reproduced exactly"""
    num = (got.to(F64) - want).norm(dim=-1)
    den = mag.norm(dim=-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


def worst_errors(got4, want4, mag4):
    """{tensor: worst per-row error}"""
    return {n: row_errors(g, w, m).max().item() for n, g, w, m in zip(TENSORS, got4, want4, mag4)}
