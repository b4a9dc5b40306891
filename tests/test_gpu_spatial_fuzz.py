"""-m gpu: seeded random geometries through the resampling and pooling kernels of csrc/spatial.hip, forward and backward, against float64
torch on the CPU (F.interpolate / F.max_pool2d / F.adaptive_avg_pool2d + autograd) on operands already rounded through the compute dtype:
bilinear resize up, down, mixed and identity under both align_corners conventions, every vector width, the fused addend and the fp32 NCHW
output with its two-kernel backward; max pooling at stride below, at and above the window size with tie-ridden inputs; the adaptive
pooling pyramid on maps smaller than a scale, non-square maps, the several-blocks-per-bin forward and the scalar kernels; the pyramid
token maps as one launch per direction and as one per scale.  The bodies are the fixed tests' own helpers (tests/test_gpu_kernels.py) and
the bounds are theirs; tests/fuzz_cases.py holds the case lists and the regime -> case table.

Max pooling draws its input from three levels {0, 0.5, 1}, zero the most likely: nearly every window then has ties and all-zero windows
are common, as after a ReLU.  The forward must be bit-exact and dx must take torch's route, the first maximum in scan order.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import fuzz_cases as fc                                                           # noqa: E402
from tests.hip_utils import init, rnd                                                        # noqa: E402
from tests.test_gpu_kernels import (DTYPES, resize_case, maxpool_case, adaptive_pool_case,   # noqa: E402
                                    pyramid_run, pyramid_vs_torch)

F64 = torch.float64


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["resize"], ids=_ids(fc.CASES["resize"]))
def test_resize_random_geometry(dtype, case):
    _, N, IH, IW, C, OH, OW, ac, add, nchw, seed = case
    resize_case(dtype, N, IH, IW, C, OH, OW, ac, add=add, nchw=nchw, seed=seed, ref=F64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["maxpool"], ids=_ids(fc.CASES["maxpool"]))
def test_maxpool_random_geometry_with_ties(dtype, case):
    _, N, H, W, C, k, stride, pad, seed = case
    init(dtype)
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(N, C, H, W, generator=g)
    x = rnd(torch.where(u < 0.6, torch.zeros_like(u), torch.where(u < 0.8, torch.full_like(u, 0.5), torch.ones_like(u))))
    maxpool_case(dtype, x, k, stride, pad, g, ref=F64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["adaptive_pool"], ids=_ids(fc.CASES["adaptive_pool"]))
def test_adaptive_pool_random_geometry(dtype, case):
    _, N, H, W, C, Ctot, scales, seed = case
    adaptive_pool_case(dtype, N, H, W, C, Ctot, scales, seed=seed, ref=F64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", fc.CASES["pyramid"], ids=_ids(fc.CASES["pyramid"]))
def test_pyramid_maps_random_geometry(dtype, case):
    _, B, C, scales, OH, OW, knob, seed = case
    c = init(dtype)
    # which launches the wrapper must choose: its own predicate, restated in tests/fuzz_cases.py (bf16 slices of 4 or 12 channels start on
    # an 8-byte boundary, off the vector path, and go one launch per scale whatever the knob says)
    grouped = fc.pyramid_grouped(C, scales, OH, OW, torch.empty((), dtype=c.tdtype).element_size(), knob)
    g = torch.Generator().manual_seed(seed)
    tok = rnd(torch.randn(B, sum(k * k for k in scales), C, generator=g))
    dcat = rnd(torch.randn(B, OH, OW, C * (len(scales) + 1), generator=g))
    names, cat, dtok = pyramid_run(dtype, tok, dcat, scales, OH, OW, knob)
    assert names.count("emrt_pyramid_resize_fwd") == (1 if grouped else 0) and names.count("emrt_pyramid_resize_bwd") == (1 if grouped else 0)
    assert names.count("emrt_resize_bilinear_fwd") == (0 if grouped else len(scales)) and names.count("emrt_resize_bilinear_bwd") == (0 if grouped else len(scales))
    pyramid_vs_torch(dtype, tok, dcat, scales, OH, OW, cat, dtok, ref=F64)
