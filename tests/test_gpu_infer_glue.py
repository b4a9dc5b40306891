"""-m gpu, kernel level: the sliding-window and multi-scale inference glue of csrc/spatial.hip -- emrt_crop_windows, emrt_window_accumulate
(scalar and vec4 kernels), emrt_window_normalise, emrt_argmax_nchw, emrt_flip_w, emrt_softmax_nchw_acc -- called through the C-ABI the way
emrt_amd/src/api/infer.py calls them.  Every reported mask and mIoU goes through these six; before this file they ran only inside the
whole-model inference tests.  fp32 NCHW throughout, as the reference's inference code.  (The 64-bit index branch of unravel3 / unravel4
needs more than 2^32 elements and stays unexercised.)
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                          # noqa: E402
from emrt_amd.functional import P                  # noqa: E402
from emrt_amd.runtime import F32                   # noqa: E402
from tests import fuzz_cases as fc                 # noqa: E402
from tests.hip_utils import init, close            # noqa: E402


def _origins(org):
    arr = (ctypes.c_int * max(2, 2 * len(org)))(*[v for yx in org for v in yx])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _refused(name, message, *args):
    with pytest.raises(_lib.EmrtHipError) as e:
        _lib.lib().call(name, *args)
    assert message in str(e.value), str(e.value)


def test_crop_windows_equal_the_slices_and_bad_windows_are_refused():
    c = init(F32)
    L = _lib.lib()
    g = torch.Generator().manual_seed(3001)
    C, H, W, ch, cw = 3, 37, 50, 16, 12                    # non-square image, non-square windows
    img = torch.randn(C, H, W, generator=g)
    org = [(int(torch.randint(0, H - ch + 1, (1,), generator=g)), int(torch.randint(0, W - cw + 1, (1,), generator=g))) for _ in range(9)]
    org += [(0, 0), (H - ch, W - cw), (0, W - cw), (H - ch, 0)]          # the four corners: flush with every edge
    imd = img.cuda()
    batch = torch.full((len(org), C, ch, cw), -7.0, device="cuda")
    arr, ptr = _origins(org)
    L.call("emrt_crop_windows", P(imd), P(batch), ptr, len(org), C, H, W, ch, cw, c.stream)
    want = torch.stack([img[:, y:y + ch, x:x + cw] for y, x in org])
    assert torch.equal(batch.cpu(), want)
    # refusals: no window, more than 64, one that sticks out by a pixel (right edge, bottom edge) -- by name, and nothing is launched
    batch.fill_(-7.0)
    msg = "1..64 windows inside the image"
    _refused("emrt_crop_windows", msg, P(imd), P(batch), ptr, 0, C, H, W, ch, cw, c.stream)
    many = torch.full((65, C, ch, cw), -7.0, device="cuda")
    arr65, ptr65 = _origins([(0, 0)] * 65)
    _refused("emrt_crop_windows", msg, P(imd), P(many), ptr65, 65, C, H, W, ch, cw, c.stream)
    for bad in ((0, W - cw + 1), (H - ch + 1, 0), (-1, 0)):
        arr1, ptr1 = _origins([(3, 4), bad])
        _refused("emrt_crop_windows", msg, P(imd), P(batch), ptr1, 2, C, H, W, ch, cw, c.stream)
    torch.cuda.synchronize()
    assert float((batch + 7.0).abs().max()) == 0.0 and float((many + 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("which", ["grid", "odd"])
def test_window_accumulate_and_normalise(which):
    """Two accumulate calls into one final / count (slide_inference's max_batch chunks) over windows that cover pixels 1, 2, 3 and 4 times
    and leave a strip uncovered, against a float64 loop over the windows: counts exact, the mean within close(F32), NaN exactly on the
    uncovered strip (0 / 0, the reference's behaviour: csrc/spatial.hip window_normalise_kernel).  "grid": every origin's x, cw and W are
    multiples of 4 (window_accumulate_vec4_kernel); "odd": one origin per call moved by a pixel (window_accumulate_kernel)."""
    c = init(F32)
    L = _lib.lib()
    im = fc.WINDOW_IMAGE
    C, H, W, ch, cw = im["C"], im["H"], im["W"], im["ch"], im["cw"]
    org = fc.WINDOW_ORIGINS[which]
    chunks = (org[:fc.WINDOW_SPLIT], org[fc.WINDOW_SPLIT:])
    for part in chunks:
        assert fc.window_vec4(W, cw, part) == (which == "grid")
    g = torch.Generator().manual_seed(3002)
    logits = torch.randn(len(org), C, ch, cw, generator=g) * 4
    final = torch.zeros(1, C, H, W, device="cuda")
    count = torch.zeros(1, 1, H, W, device="cuda")
    j0 = 0
    for part in chunks:
        arr, ptr = _origins(part)
        ld = logits[j0:j0 + len(part)].contiguous().cuda()
        L.call("emrt_window_accumulate", P(ld), P(final), P(count), ptr, len(part), C, H, W, ch, cw, c.stream)
        j0 += len(part)
    out = torch.empty(1, C, H, W, device="cuda")
    L.call("emrt_window_normalise", P(final), P(count), P(out), C, H, W, c.stream)
    want = torch.zeros(C, H, W, dtype=torch.float64)
    for j, (y, x) in enumerate(org):
        want[:, y:y + ch, x:x + cw] += logits[j].double()
    cov = torch.tensor(fc.window_cover(org, H, W, ch, cw), dtype=torch.float32)
    assert {0.0, 1.0, 2.0, 3.0, 4.0} <= set(cov.flatten().tolist())
    assert torch.equal(count.cpu()[0, 0], cov), "hit counts must be exact integers"
    close("window sums", final.cpu()[0], want, F32)
    got = out.cpu()[0]
    covered = (cov > 0).expand(C, H, W)
    assert torch.equal(torch.isnan(got), ~covered), "NaN exactly where no window covers the pixel"
    assert bool((~covered)[:, :, 20:].all()) and not bool((~covered)[:, :, :20].all())
    mean = want / cov.double().clamp_min(1.0)
    close("window mean", got[covered], mean[covered], F32)


@pytest.mark.parametrize("C", [1, 7])
def test_argmax_over_classes_first_maximum_and_first_nan_win(C):
    c = init(F32)
    g = torch.Generator().manual_seed(3003)
    N, H, W = 2, 9, 31                                      # N * H * W = 558: two full blocks and a ragged third
    x = torch.randn(N, C, H, W, generator=g)
    if C > 1:
        x[0, :, 0, :] = x[0, 3:4, 0, :]                     # all classes tie: class 0
        x[1, 2, 1, :] = x[1, 5, 1, :] = 9.0                 # two classes tie for the maximum: class 2
        x[0, 3, 2, :] = float("nan")                        # a NaN in a middle class counts as the maximum ...
        x[0, 5, 2, ::2] = float("nan")                      # ... and the first NaN wins
        x[0, 6, 2, :] = 50.0
        x[1, 0, 3, :] = float("nan")                        # class 0 NaN
    pred = torch.full((N, 1, H, W), -1, dtype=torch.int32, device="cuda")
    xd = x.cuda()
    _lib.lib().call("emrt_argmax_nchw", P(xd), P(pred), N, C, H, W, c.stream)
    want = torch.argmax(x, dim=1, keepdim=True)
    assert torch.equal(pred.cpu().long(), want)
    if C > 1:
        assert bool((want[0, 0, 0] == 0).all() and (want[1, 0, 1] == 2).all() and (want[0, 0, 2] == 3).all() and (want[1, 0, 3] == 0).all())


@pytest.mark.parametrize("W", [1, 2, 7, 64, 101])
def test_flip_w_equals_torch_flip(W):
    c = init(F32)
    g = torch.Generator().manual_seed(3004)
    x = torch.randn(2, 3, 5, W, generator=g)
    xd = x.cuda()
    out = torch.empty_like(xd)
    _lib.lib().call("emrt_flip_w", P(xd), P(out), x.numel() // W, W, c.stream)
    assert torch.equal(out.cpu(), torch.flip(x, dims=[-1]))
    before = xd.clone()
    _refused("emrt_flip_w", "null or aliased pointers", P(xd), P(xd), x.numel() // W, W, c.stream)
    torch.cuda.synchronize()
    assert torch.equal(xd, before)


def _softmax_inputs():
    g = torch.Generator().manual_seed(3101)
    N, C, H, W = 2, 7, 11, 13                              # N * H * W = 286: one full block and a ragged second
    xs = []
    for _ in range(2):
        x = torch.randn(N, C, H, W, generator=g) * 3
        x[:, :, 0, :] = -80.0 + torch.randn(N, C, W, generator=g)          # a row of pixels with every logit near -80 ...
        x[:, 2, 0, ::2] = 80.0                                               # ... every other one with one class near +80 (the others underflow)
        x[:, :, 1, :] = 80.0 + torch.randn(N, C, W, generator=g) * 0.5       # a row of pixels with every logit near +80
        xs.append(x)
    return xs


SOFTMAX_F32_ERR = 2.55e-7          # max |float32 - float64| of torch's CPU softmax, summed over the two calls, on _softmax_inputs() (values up to 2.0)
SOFTMAX_BOUND = 4 * SOFTMAX_F32_ERR


def test_softmax_accumulated_over_two_calls():
    """final += softmax(logits, dim=1) twice into one accumulator (ms_inference: one call per scale / flip) against float64 softmax summed.
    Bound: torch's own float32 CPU softmax differs from float64 by at most 2.55e-7 on these inputs (sums up to 2.0, so half an fp32 ulp is
    already 1.2e-7); the kernel is allowed four times that, 1.02e-6 absolute.  The reference pair is re-measured here and must hold its own
    figure, so the bound never comes from the kernel's output."""
    c = init(F32)
    xs = _softmax_inputs()
    N, C, H, W = xs[0].shape
    want = sum(torch.softmax(x.double(), 1) for x in xs)
    pair = ((torch.softmax(xs[0], 1) + torch.softmax(xs[1], 1)).double() - want).abs().max().item()
    print("softmax: torch float32 vs float64 %.3e (recorded %.3e), bound %.3e" % (pair, SOFTMAX_F32_ERR, SOFTMAX_BOUND))
    assert pair <= SOFTMAX_F32_ERR * 1.01
    acc = torch.zeros(N, C, H, W, device="cuda")
    for x in xs:
        xd = x.cuda()
        _lib.lib().call("emrt_softmax_nchw_acc", P(xd), P(acc), N, C, H, W, c.stream)
    got = acc.cpu()
    assert torch.isfinite(got).all()
    err = (got.double() - want).abs().max().item()
    print("softmax: kernel vs float64 %.3e" % err)
    assert err <= SOFTMAX_BOUND, "max |acc - float64| = %.3e > %.3e" % (err, SOFTMAX_BOUND)
