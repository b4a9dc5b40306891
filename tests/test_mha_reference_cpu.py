"""tests/mha_reference.py checked without a GPU: the float64 closed form equals autograd, the bounds of the GPU sweep
(tests/test_gpu_mha_fuzz.py) are at least the stated multiples of the floors of the sweep's own cases, and every mutant -- a reference that is
wrong on purpose in one named way -- lies beyond twice the bound in the regime built for it.  So the bounds separate right from wrong
before any GPU is involved, and an edit of a seed or a regime that moves a floor fails here."""
import functools

import pytest
import torch

from tests import fuzz_cases as fc
from tests import mha_reference as mr

F64 = torch.float64
CASES = fc.CASES["mha"]


def _mask_of(case):
    """the stand-in mask of a dropout case (None, 0.0 without dropout)"""
    _, B, M, L, _, p, _, seed = case
    return (mr.random_mask(B, M, L, p, seed + 7), p) if p > 0.0 else (None, 0.0)


@functools.lru_cache(maxsize=None)
def _case_data(idx, dtype):
    _, B, M, L, regime, _, _, seed = CASES[idx]
    ins = mr.make_inputs(regime, B, M, L, seed, dtype)
    mask, p = _mask_of(CASES[idx])
    return ins, mask, p, mr.exact(*ins, mask=mask, p=p), mr.magnitude(*ins, mask=mask, p=p)


def _autograd(q, k, v, dy, mask, p):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    w = torch.softmax((q @ k.transpose(-1, -2)) * mr.SCALE, -1)
    if mask is not None:
        w = w * mask / (1.0 - p)
    o = w @ v
    o.backward(dy)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("regime", mr.REGIMES)
@pytest.mark.parametrize("B,M,L,p", [(2, 3, 1, 0.0), (1, 2, 5, 0.0), (2, 1, 33, 0.0), (2, 2, 17, 0.5), (1, 3, 48, 0.1)])
def test_exact_equals_float64_autograd(regime, B, M, L, p):
    ins = mr.make_inputs(regime, B, M, L, 4000 + L, "bf16")
    mask = mr.random_mask(B, M, L, p, 5) if p > 0 else None
    got, want = mr.exact(*ins, mask=mask, p=p), _autograd(*ins, mask, p)
    mag = mr.magnitude(*ins, mask=mask, p=p)
    for n, g, w, m in zip(mr.TENSORS, got, want, mag):
        assert g.dtype == F64 and g.shape == (B, M, L, 32)
        # float64 on both sides: 2^-53 times a few hundred operations; 1e-12 of the magnitude is three orders above that and nine below any bound
        assert mr.row_errors(g, w, m).max().item() < 1e-12, n
        assert (m >= g.abs() * (1 - 1e-12)).all(), "%s: the magnitude bounds the value elementwise" % n


def test_input_regimes_are_what_they_say():
    for dtype in mr.DTYPES:
        q, k, v, dy = mr.make_inputs("negative", 2, 2, 97, 11, dtype)
        assert mr.scores(q, k).median().item() < -15          # around -20: a padding column of score 0 takes the row
        q, k, v, dy = mr.make_inputs("lastkey", 2, 2, 97, 12, dtype)
        P = torch.softmax(mr.scores(q, k), -1)
        assert P[..., -1].median().item() > 0.5               # the last key carries most of every row
        q, k, v, dy = mr.make_inputs("peaked", 2, 2, 97, 13, dtype)
        assert 4.0 < mr.scores(q, k).std().item() < 6.0
        for t in (q, k, v, dy):
            assert torch.equal(mr.round_to(t, dtype), t)     # rounded through the compute dtype


def test_floors_and_bounds():
    """the worst per-row error of the best a correct kernel can do, over every case of the sweep, against MHA_BOUND / margin"""
    floors = {d: dict.fromkeys(mr.TENSORS, 0.0) for d in mr.DTYPES}
    model = {"bf16": mr.contract_bf16, "f32": mr.evaluate_f32}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # the fp32 floor is a maximum over fp32 sums: one thread, one summation order
    try:
        for idx in range(len(CASES)):
            for d in mr.DTYPES:
                ins, mask, p, ex, mag = _case_data(idx, d)
                for n, e in mr.worst_errors(model[d](*ins, mask=mask, p=p), ex, mag).items():
                    floors[d][n] = max(floors[d][n], e)
    finally:
        torch.set_num_threads(threads)
    for d in mr.DTYPES:
        print("[mha floors] %-4s " % d + "  ".join("%s %.3e (bound %.3e)" % (n, floors[d][n], mr.MHA_BOUND[d][n]) for n in mr.TENSORS))
    for d in mr.DTYPES:
        for n in mr.TENSORS:
            assert floors[d][n] > 0.0
            assert floors[d][n] <= mr.MHA_BOUND[d][n] / mr.FLOOR_MARGIN[d], "%s %s: floor %.4g, bound %.4g" % (d, n, floors[d][n], mr.MHA_BOUND[d][n])
            # and the bound is that multiple of the floor, not something wider: rounded up by at most a quarter
            assert mr.MHA_BOUND[d][n] <= 1.25 * mr.FLOOR_MARGIN[d] * floors[d][n], "%s %s: bound %.4g is wider than %g x floor %.4g" % (
                d, n, mr.MHA_BOUND[d][n], mr.FLOOR_MARGIN[d], floors[d][n])


def _separates(name, got4, ex, mag, dtype, tensors, half_of_o):
    for n, g, w, m in zip(mr.TENSORS, got4, ex, mag):
        if n not in tensors:
            continue
        err = mr.row_errors(g, w, m)
        bound = mr.MHA_BOUND[dtype][n]
        assert err.max().item() > 2 * bound, "%s %s %s: worst row %.3g does not clear 2 x %.3g" % (name, dtype, n, err.max().item(), bound)
        if n == "o" and half_of_o:
            assert (err > bound).double().mean().item() >= 0.5, "%s %s: only %.2f of the rows of o beyond the bound" % (
                name, dtype, (err > bound).double().mean().item())


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_padding_mutants_are_caught(dtype):
    """drop_last_key in the lastkey regime at every length >= 2, pad_in_denominator in the negative regime at every length that is not a whole
    number of tiles: at the sweep's own cases of those regimes and at every length of the list with B = M = 2"""
    todo = [(c[1], c[2], c[3], c[4], c[7]) for c in CASES if c[5] == 0.0 and c[4] in ("lastkey", "negative")]
    todo += [(2, 2, L, r, 6000 + L) for L in fc.MHA_LS for r in ("lastkey", "negative")]
    ran = {"lastkey": 0, "negative": 0}
    for B, M, L, regime, seed in todo:
        if L < 2 or (regime == "negative" and L % 16 == 0):
            continue
        ins = mr.make_inputs(regime, B, M, L, seed, dtype)
        ex, mag = mr.exact(*ins), mr.magnitude(*ins)
        mutant = mr.drop_last_key if regime == "lastkey" else mr.pad_in_denominator
        _separates("%s L=%d" % (mutant.__name__, L), mutant(*ins), ex, mag, dtype, mr.TENSORS, True)
        ran[regime] += 1
    assert ran["lastkey"] >= len(fc.MHA_LS) - 1 and ran["negative"] >= sum(L % 16 != 0 for L in fc.MHA_LS) - 1


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_mask_mutants_are_caught(dtype):
    """a backward that uses another mask than the forward (transposed; another head's) in every dropout case: beyond twice the bound on the three
    gradients (o is the forward's and does not move).  Another head needs M >= 2."""
    n_heads = 0
    for idx, c in enumerate(CASES):
        if c[5] == 0.0:
            continue
        ins, mask, p, ex, mag = _case_data(idx, dtype)
        _separates("mask_transposed %s" % c[0], mr.mask_transposed(*ins, mask, p), ex, mag, dtype, ("dq", "dk", "dv"), False)
        if c[2] >= 2:
            _separates("mask_other_head %s" % c[0], mr.mask_other_head(*ins, mask, p), ex, mag, dtype, ("dq", "dk", "dv"), False)
            n_heads += 1
    assert n_heads >= 8, n_heads
