"""-m gpu: seeded random shapes through the BatchNorm, GroupNorm and LayerNorm kernels of csrc/norm.hip, forward and backward, against
float64 torch on the CPU (F.batch_norm / F.group_norm / F.layer_norm + autograd) on operands already rounded through the compute dtype.
The fixed-shape tests of tests/test_gpu_kernels.py and tests/test_gpu_gn_levels.py are the shapes thought of in advance; this sweep is for
the rest: every channel count bn_rowgeom accepts on both sides of its thresholds (also thread counts that are not whole waves), both sides
of gn_use_fused for the backward too, ragged LayerNorm passes, short rows, one-row inputs.  The bodies are the fixed tests' own helpers and
the bounds are the fixed tests' (tests/hip_utils.close with the same scale factors); tests/fuzz_cases.py holds the case lists and the
regime -> case table, tests/test_fuzz_cases_cpu.py keeps every regime populated.

The inputs differ from the fixed tests' in one respect: every channel (and group, and row) has its own scale in [0.5, 2] and shift in
[-2, 2].  With one scale and shift for the whole tensor every population has the same statistics up to sampling noise, and a kernel that
normalises channel c with channel c' s mean and variance passes, in bf16 entirely.  Each test first asserts that the smallest population
standard deviation of the rounded input is above 0.1 (test_gpu_kernels.population_floor).

Degenerate populations are tested on their own: one all-zero channel / group / row (a dead post-ReLU channel, variance exactly 0) must give
beta forward and a finite backward, both equal to the float64 reference under the same bounds (x - mean is exactly 0 on both sides, so
1 / sqrt(eps) multiplies only dy terms).

The 64-bit index branches of csrc/common.hpp need more than 2^32 elements and stay unexercised here.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                                                    # noqa: E402
from tests import fuzz_cases as fc                                                           # noqa: E402
from tests.test_gpu_kernels import DTYPES, bn_train_case, group_norm_case, layer_norm_case   # noqa: E402
from tests.test_gpu_gn_levels import _run as gn_levels_run, _check as gn_levels_check        # noqa: E402

F64 = torch.float64


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["batchnorm"], ids=_ids(fc.CASES["batchnorm"]))
def test_batch_norm_random_shapes(dtype, case):
    _, N, H, W, C, relu, with_res, seed = case
    bn_train_case(dtype, N, H, W, C, relu, with_res, seed=seed, per_channel=True, ref=F64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,M", [(64, 40), (1028, 24)], ids=["256-threads", "257-threads"])
def test_batch_norm_dead_channel(dtype, C, M):
    """one all-zero channel, in the middle of a quad: forward = beta there, backward finite, both equal to the float64 reference"""
    bn_train_case(dtype, 2, M // 2, 1, C, False, False, seed=2101, per_channel=True, dead_channel=C // 2 + 1, ref=F64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["groupnorm"], ids=_ids(fc.CASES["groupnorm"]))
def test_group_norm_random_shapes(dtype, case):
    _, N, H, W, C, G, gelu, with_res, seed = case
    group_norm_case(dtype, N, H, W, C, G, gelu, with_res, seed=seed, per_group=True, ref=F64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W,C,G", [(2, 5, 7, 64, 8), (2, 4, 5, 1024, 2)], ids=["fused", "two-pass"])
def test_group_norm_dead_group(dtype, N, H, W, C, G):
    """one all-zero group of image 0 (the last group), on both sides of gn_use_fused"""
    assert fc.gn_use_fused(H * W, C, G) == (C // G <= 256)
    group_norm_case(dtype, N, H, W, C, G, False, False, seed=2202, per_group=True, dead_group=G - 1, ref=F64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["groupnorm_levels"], ids=_ids(fc.CASES["groupnorm_levels"]))
def test_group_norm_levels_random_shapes(dtype, case):
    """emrt_groupnorm_levels_fwd / _bwd through the reference builder and the bounds of tests/test_gpu_gn_levels.py (float64 reference)"""
    _, B, hws, C, G, gelu, with_res, seed = case
    r = gn_levels_run(dtype, B, hws, gelu, with_res, False, seed=seed, C=C, G=G, per_group=True)
    assert r["min_std"] > 0.1, r["min_std"]
    gn_levels_check(r, dtype, len(hws))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["layernorm"], ids=_ids(fc.CASES["layernorm"]))
def test_layer_norm_random_shapes(dtype, case):
    _, B, L, C, form, max_blocks, rows_knob, seed = case
    Lb = _lib.lib()
    old = [(k, Lb.set_tuning(k, v)) for k, v in (("ln_bwd_max_blocks", max_blocks), ("ln_bwd_rows", rows_knob))]
    try:
        layer_norm_case(dtype, B, L, C, form, seed=seed, spread=True, ref=F64)
    finally:
        for k, v in old:
            Lb.set_tuning(k, v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,L,C,form,row", [(2, 9, 256, "a", 17), (1, 7, 1000, "a+b", 3)], ids=["last-row-C256", "ragged-pass"])
def test_layer_norm_dead_row(dtype, B, L, C, form, row):
    """one all-zero row (with rows % 4 != 0, once the very last row)"""
    layer_norm_case(dtype, B, L, C, form, seed=2303, spread=True, dead_row=row, ref=F64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["layernorm_drop"], ids=_ids(fc.CASES["layernorm_drop"]))
def test_layer_norm_branch_dropout_random_shapes(dtype, case):
    """LN(a + dropout(b)) with the dropout drawn inside emrt_layernorm_fwd / _bwd, the mask held to the host model of csrc/drop_hash.hpp
    (tests/dropout_reference.py) instead of being read back: every channel count on both sides of a 256-lane pass, rows % 4 != 0 and one
    row, the post, q_pos and addend arms, p in {0.1, 0.5}, the backward under its default block shape and under ln_bwd_rows /
    ln_bwd_max_blocks settings that change which rows a block walks (a block that re-derived another quad's word would mask dz_b wrongly)."""
    _, B, L, C, form, p, salt, max_blocks, rows_knob, _, seed = case
    Lb = _lib.lib()
    old = [(k, Lb.set_tuning(k, v)) for k, v in (("ln_bwd_max_blocks", max_blocks), ("ln_bwd_rows", rows_knob))]
    try:
        layer_norm_case(dtype, B, L, C, form, seed=seed, spread=True, ref=F64, drop=(p, salt))
    finally:
        for k, v in old:
            Lb.set_tuning(k, v)
