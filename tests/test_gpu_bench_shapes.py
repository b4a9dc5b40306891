"""-m gpu parity tests AT THE BENCHMARK'S OWN SHAPES AND DTYPE (bf16, BASELINE configs[1] and configs[2]).

The kernel-level cases of test_gpu_kernels.py are small, so the dispatchers route them to the small-problem kernels; the
kernels bench.py actually times are selected by size:
  * msda_fwd_lds_kernel      -- bf16, B*M*Lq >= 8192 and the (batch, head) slab fits in LDS (msda.hip: emrt_msda_fwd)
  * igemm_kernel 128x128 bf16 -- OC > 64, >= 16 k-tiles, >= 256 blocks (conv.hip: conv_pick_tile)
  * wgrad_kernel<bf16> with the pixel reduction split over blockIdx.z (wgrad_plan), bwd_pair_kernel on the 16x16 / 32x32 maps
Each is compared here with the oracle's torch-CPU expression of the same reference operator on bf16-rounded inputs
(reference arithmetic: EMRT_utils/utils.py:64-97, paddle_EMRT.py:134-138,201-209), the two MSDA forward kernels with each
other bit for bit, and the whole bf16 model at batch 8 / 256x256 / ResNet-50 with the fp32 oracle under stated bounds.
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
from emrt_amd.runtime import ctx, F32, BF16, Tape   # noqa: E402
from tests.hip_utils import close_gemm, init, dev_map, host_map, dev, host, rnd, Holder, close   # noqa: E402
from tests.test_gpu_kernels import _msda_ref, run_bwd   # noqa: E402


# -----------------------------------------------------------------------------------------------------------------
# MSDA at the encoder-call shapes of cfg2 (B=8, 256^2 -> Lv=1344) and cfg3 (B=4, 512^2 -> Lv=5376)
# -----------------------------------------------------------------------------------------------------------------
MSDA_BENCH = [
    dict(name="cfg2-encoder", B=8, shapes=[(32, 32), (16, 16), (8, 8)], Lq=None, lds=True),
    dict(name="cfg2-decoder", B=8, shapes=[(32, 32), (16, 16), (8, 8)], Lq=110, lds=True),     # B*M*Lq = 7040 >= 2048: LDS kernel too (forward)
    dict(name="tiny-decoder", B=1, shapes=[(32, 32), (16, 16), (8, 8)], Lq=110, lds=False),    # B*M*Lq = 880: global kernel
    # slab 344 KB > LDS: the ROW-BAND kernel (msda_fwd_band_kernel: 8 bands x (22 of 64 + 18 of 32 + 16 of 16 rows) staged per block)
    dict(name="cfg3-encoder", B=4, shapes=[(64, 64), (32, 32), (16, 16)], Lq=None, lds=False, band=True),
    # the same with offsets far beyond the staged halo (sigma 12 px): most level-0 / level-1 samples miss the band -> global fallback
    dict(name="cfg3-encoder-wild", B=4, shapes=[(64, 64), (32, 32), (16, 16)], Lq=None, lds=False, band=True, sigma=12.0),
    # non-square pyramid (16 bands; widths that are not multiples of the 16-pixel DMA piece)
    dict(name="band-nonsquare", B=2, shapes=[(64, 80), (32, 40), (16, 20)], Lq=None, lds=False, band=True),
]


def _msda_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    M, L, Pn = 8, 3, 6
    shapes = cfg["shapes"]
    Lv = sum(h * w for h, w in shapes)
    B = cfg["B"]
    Lq = cfg["Lq"] or Lv
    tp = M * L * Pn
    value = rnd(torch.randn(B, Lv, M * 32, generator=g))
    # offsets of a few pixels (the trained regime: |off| <~ 6 px in the level's own units) and O(1) logits
    offw = torch.cat([torch.randn(B, Lq, 2 * tp, generator=g) * cfg.get("sigma", 2.5), torch.randn(B, Lq, tp, generator=g)], -1)
    if cfg["Lq"] is None:      # encoder: pixel-centre reference points, shared by the batch, one per level (identical)
        from emrt_amd.src.models.emrt import encoder_reference_points
        ref = encoder_reference_points(shapes)
    else:
        ref = torch.rand(1, Lq, 1, 2, generator=g)
    return value, offw, ref, shapes, (B, Lq, Lv, M, L, Pn)


@pytest.mark.parametrize("cfg", MSDA_BENCH, ids=[c["name"] for c in MSDA_BENCH])
def test_msda_bench_shape_bf16_vs_oracle(cfg):
    c = init(BF16)
    L_ = _lib.lib()
    value, offw, ref, shapes, (B, Lq, Lv, M, L, Pn) = _msda_inputs(cfg, 31)
    vr, orq = value.clone().requires_grad_(True), offw.clone().requires_grad_(True)
    out_r = _msda_ref(vr, orq, ref, shapes, M, L, Pn)
    dy = rnd(torch.randn(out_r.shape, generator=torch.Generator().manual_seed(32)))
    out_r.backward(dy)
    vd, od, rd = dev(value), dev(offw, torch.float32), dev(ref, torch.float32)
    tape = Tape()
    c.tape = tape
    y = Fn.msda(vd, od, rd, shapes, M, Pn)
    c.tape = None
    tape.watch(vd)
    tape.watch(od)
    # which kernel ran: the library's own answer (emrt_msda_plan: the planner emrt_msda_fwd launches from; kinds EMRT_MSDA_K_FWD_*)
    arr = (ctypes.c_int * (2 * L))(*[int(v) for hw in shapes for v in hw])
    plan = (ctypes.c_int * 6)()
    assert L_.query("emrt_msda_plan", 0, B, Lq, M, L, Pn, ctypes.cast(arr, ctypes.c_void_p), 0, BF16, ctypes.cast(plan, ctypes.c_void_p), 6) == 6, L_.last_error()
    assert plan[0] == (1 if cfg["lds"] else 2 if cfg.get("band") else 0), "the test case no longer selects the kernel it was written for"
    # bf16 output of an fp32 accumulation over bf16 values: one rounding of the result (2^-9 relative) + accumulation noise
    close("msda fwd (bench shape)", host(y), out_r.detach(), BF16, atol=2e-2, rtol=1e-2)
    rel = ((host(y) - out_r.detach()).norm() / out_r.detach().norm()).item()
    assert rel < 4e-3, "relative L2 error %.4g" % rel
    # the same call on the other forward kernel must be BIT-identical (msda.hip states the two share arithmetic and order)
    old = L_.set_tuning("msda_fwd_global", 1)
    try:
        y_glob = Fn.msda(vd, od, rd, shapes, M, Pn)
    finally:
        L_.set_tuning("msda_fwd_global", old)
    if cfg.get("band"):
        # the band kernel adds the samples that missed its staged rows LAST (from global memory): same terms, other order for those
        # pairs only -- a last-bit fp32 difference can flip the bf16 rounding of an output (1 ulp = 2^-8 relative)
        diff = (y_glob.float() - y.float()).abs()
        frac = (diff > 0).float().mean().item()
        print("msda %s: band vs global kernel: %.4f %% of the outputs differ, max |diff| %.3g" % (cfg["name"], 100 * frac, diff.max().item()))
        assert frac < (0.2 if cfg.get("sigma") else 0.01) and diff.max().item() <= 2.0 ** -6 * max(1.0, y.float().abs().max().item())
    else:
        assert torch.equal(y_glob, y), "LDS-staged and global MSDA forward differ: max |diff| %.3g" % (y_glob.float() - y.float()).abs().max().item()
    dv, do = run_bwd(tape, [(y, dev(dy))], [vd, od])
    gv, go = vr.grad, orq.grad
    rel_v = ((host(dv) - gv).norm() / gv.norm()).item()
    rel_o = ((host(do) - go).norm() / go.norm()).item()
    print("msda %s: fwd rel %.2e, dvalue rel %.2e, doffw rel %.2e" % (cfg["name"], rel, rel_v, rel_o))
    # dvalue: fixed-point LDS scatter then ONE bf16 rounding; doffw: fp32 arithmetic on bf16 operands, stored in bf16 (what the
    # projection's backward GEMM reads: the old fp32 tensor was cast to exactly these values by a separate launch)
    assert rel_v < 6e-3 and rel_o < 6e-3, (rel_v, rel_o)
    close("msda dvalue (bench shape)", host(dv), gv, BF16, atol=6e-2 * float(gv.abs().max()) / 8, rtol=2e-2)
    # the LDS-staged gradient kernel (encoder calls) against the global-gather one: same math, other summation order
    old = L_.set_tuning("msda_bwd_global", 1)
    try:
        tape = Tape()
        c.tape = tape
        y2 = Fn.msda(vd, od, rd, shapes, M, Pn)
        c.tape = None
        tape.watch(vd)
        tape.watch(od)
        dv2, do2 = run_bwd(tape, [(y2, dev(dy))], [vd, od])
    finally:
        L_.set_tuning("msda_bwd_global", old)
    rel_k = ((host(do) - host(do2)).norm() / host(do2).norm()).item()
    assert rel_k < 5e-4, rel_k          # bf16 outputs: a last-bit fp32 difference flips a rounding (1 ulp = 4e-3) in a few elements
    assert (host(dv) - host(dv2)).abs().max().item() <= 2e-2 * float(gv.abs().max())       # one bf16 ulp where the probabilities differ in the last bit


def test_msda_lds_scatter_is_bit_reproducible():
    """The value gradient is an integer (fixed-point) LDS scatter: two launches on the same inputs must agree bit for bit
    (DESIGN.md 4); the fp32 offset / logit gradients have no atomics at all."""
    c = init(BF16)
    value, offw, ref, shapes, (B, Lq, Lv, M, L, Pn) = _msda_inputs(MSDA_BENCH[0], 33)
    vd, od, rd = dev(value), dev(offw, torch.float32), dev(ref, torch.float32)
    dy = dev(rnd(torch.randn(B, Lq, M * 32, generator=torch.Generator().manual_seed(34))))
    res = []
    for _ in range(2):
        tape = Tape()
        c.tape = tape
        y = Fn.msda(vd, od, rd, shapes, M, Pn)
        c.tape = None
        tape.watch(vd)
        tape.watch(od)
        res.append(run_bwd(tape, [(y, dy)], [vd, od]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("offsets", ["compass", "spread"])
def test_msda_scatter_merging_consecutive_points_gives_the_same_value_gradient(offsets):
    """Knob msda_scatter_merge (csrc/msda.hip: msda_bwd_value_lds_kernel): consecutive points of a query with the same 2 x 2 footprint are
    added in registers before the LDS atomics.  Same value gradient as the unmerged scatter up to the fixed-point rounding of a merged pair
    (|sum of two roundings - rounding of the sum| <= 1 unit of 2^-30 / (Lq max|g|)), on the untrained compass offsets of _reset_parameters
    (t_e_d.py:46-63: many merges in the coarser levels) and on offsets spread by 2.5 px (hardly any); bit-reproducible either way."""
    import math
    c = init(BF16)
    L_ = _lib.lib()
    cfg = MSDA_BENCH[0]
    value, offw, ref, shapes, (B, Lq, Lv, M, L, Pn) = _msda_inputs(cfg, 35)
    if offsets == "compass":      # offsets = head m's compass direction x point index k = 1..P, the same for every query and level; zero logits
        th = torch.arange(M, dtype=torch.float32) * (2.0 * math.pi / M)
        grid = torch.stack([th.cos(), th.sin()], -1)
        grid = grid / grid.abs().max(-1, keepdim=True)[0]
        grid = grid.reshape(M, 1, 1, 2).repeat(1, L, Pn, 1) * torch.arange(1, Pn + 1, dtype=torch.float32).reshape(1, 1, -1, 1)
        offw = torch.cat([grid.flatten().expand(B, Lq, -1), torch.zeros(B, Lq, M * L * Pn)], -1).contiguous()
    vd, od, rd = dev(value), dev(offw, torch.float32), dev(ref, torch.float32)
    dy = dev(rnd(torch.randn(B, Lq, M * 32, generator=torch.Generator().manual_seed(36))))
    res = {}
    old_mf = L_.set_tuning("msda_scatter_mfma", 0)          # the knob under test belongs to the LDS atomic scatter (bf16 at this shape defaults to the matrix-product kernel)
    for knob in (0, 1, 1):
        old = L_.set_tuning("msda_scatter_merge", knob)
        try:
            tape = Tape()
            c.tape = tape
            y = Fn.msda(vd, od, rd, shapes, M, Pn)
            c.tape = None
            tape.watch(vd)
            dv, = run_bwd(tape, [(y, dy)], [vd])
            res.setdefault(knob, []).append(host(dv))
        finally:
            L_.set_tuning("msda_scatter_merge", old)
    L_.set_tuning("msda_scatter_mfma", old_mf)
    assert torch.equal(res[1][0], res[1][1]), "the merged scatter is not bit-reproducible"
    a, b = res[0][0], res[1][0]
    rel = ((a - b).norm() / a.norm()).item()
    differ = (a != b).float().mean().item()
    print("msda scatter merge (%s offsets): value gradient rel L2 %.2e vs unmerged, %.4f %% of the elements differ" % (offsets, rel, 100 * differ))
    assert rel < 2e-4 and differ < 0.01, (rel, differ)          # a bf16 element flips only where the fixed-point sums differ by a unit right at a rounding boundary


@pytest.mark.parametrize("cfg", MSDA_BENCH[:2], ids=[c["name"] for c in MSDA_BENCH[:2]])
def test_msda_value_gradient_as_a_matrix_product_vs_the_atomic_scatter(cfg):
    """msda_bwd_value_mfma_kernel (knob msda_scatter_mfma) against msda_bwd_value_lds_kernel on the same inputs at the bench shapes: both are
    within the oracle bound of test_msda_bench_shapes_vs_oracle by that test and the fuzz; HERE they are compared with each other -- the atomic
    scatter is exact to 2^-30 of Lq max|g| per addend, the matrix product rounds each summed (pixel, query) weight once to bf16 (2^-9 relative,
    independent errors over the ~100 queries that reach a pixel) -- and the matrix product must be bit-reproducible (integer LDS adds, MFMA)."""
    c = init(BF16)
    L_ = _lib.lib()
    value, offw, ref, shapes, (B, Lq, Lv, M, L, Pn) = _msda_inputs(cfg, 41)
    vd, od, rd = dev(value), dev(offw, torch.float32), dev(ref, torch.float32)
    dy = dev(rnd(torch.randn(B, Lq, M * 32, generator=torch.Generator().manual_seed(42))))
    res = {}
    for knob in (0, 2, 2):
        old = L_.set_tuning("msda_scatter_mfma", knob)
        try:
            tape = Tape()
            c.tape = tape
            y = Fn.msda(vd, od, rd, shapes, M, Pn)
            c.tape = None
            tape.watch(vd)
            dv, = run_bwd(tape, [(y, dy)], [vd])
            res.setdefault(knob, []).append(host(dv))
        finally:
            L_.set_tuning("msda_scatter_mfma", old)
    assert torch.equal(res[2][0], res[2][1]), "the matrix-product scatter is not bit-reproducible"
    a, b = res[0][0], res[2][0]
    rel = ((a - b).norm() / a.norm()).item()
    worst = ((a - b).abs().max() / a.abs().max()).item()
    print("msda value gradient %s: matrix product vs atomic scatter rel L2 %.2e, worst element %.2e of max|dvalue|" % (cfg["name"], rel, worst))
    assert rel > 0.0, "both knob settings ran the same kernel"
    assert rel < 3e-3 and worst < 1e-2, (rel, worst)


# -----------------------------------------------------------------------------------------------------------------
# convolutions at the shapes that carry the step's FLOPs
# -----------------------------------------------------------------------------------------------------------------
CONV_BENCH = [
    # name, N, H, W, Cin, Cout, k, stride, pad, bias, expected forward path
    ("uphead-128", 8, 128, 128, 256, 256, 3, 1, 1, True, "128x128"),      # paddle_EMRT.py:136 (conv_2), 77 GFLOP forward
    ("uphead-64", 8, 64, 64, 256, 256, 3, 1, 1, True, "128x128"),         # :135 (conv_1)
    ("cls_psp-0", 8, 32, 32, 1536, 512, 3, 1, 1, False, "128x128"),       # :201-203, K = 13 824
    ("layer4-1x1", 8, 8, 8, 2048, 512, 1, 1, 0, False, "ksplit"),         # paddle_vision_resnet.py:108 at 8x8
    ("layer3-3x3", 8, 16, 16, 256, 256, 3, 1, 1, False, "pair"),          # :111-119 at 16x16: dgrad+wgrad pair launch
    ("efp-3x3", 8, 32, 32, 256, 256, 3, 1, 1, False, "pair"),             # paddle_EMRT.py:16-23 at 32x32
    ("ffn-linear1", 8, 1, 1344, 256, 1024, 1, 1, 0, True, "pair"),        # transformer_encoder_decoder.py:118 over [8,1344,256]
]


def _expected_paths(N, H, W, Cin, Cout, k, stride, pad):
    """What conv.hip's dispatchers pick for a bf16 problem (mirrors conv_pick_tile / conv_bwd_dispatch)."""
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    M = N * OH * OW
    nkt = (k * k * Cin + 63) // 64
    blocks128 = ((M + 127) // 128) * ((Cout + 127) // 128)
    fwd_big = Cout > 64 and nkt >= 16 and blocks128 >= 256
    Md = N * H * W
    nd = ((Md + 63) // 64) * ((Cin + 63) // 64)
    nkt_d = (k * k * Cout + 63) // 64
    dgrad_big = Cin > 64 and nkt_d >= 16 and ((Md + 127) // 128) * ((Cin + 127) // 128) >= 256
    pair = Cin > 32 and not dgrad_big and nd <= 768
    return fwd_big, dgrad_big, pair


@pytest.mark.parametrize("case", CONV_BENCH, ids=[c[0] for c in CONV_BENCH])
def test_conv_bench_shape_bf16_vs_torch(case):
    name, N, H, W, Cin, Cout, k, stride, pad, bias, path = case
    fwd_big, dgrad_big, pair = _expected_paths(N, H, W, Cin, Cout, k, stride, pad)
    assert {"128x128": fwd_big and dgrad_big and not pair, "pair": pair, "ksplit": not fwd_big}[path], \
        "the case no longer reaches the kernel it was written for: %s" % ((fwd_big, dgrad_big, pair),)
    _conv_case_vs_torch(case)          # default: the data gradient alone, the weight gradient through emrt_conv2d_wgrad_group
    if pair:                           # the layer-by-layer backward (Context.wgrad_batch = 0): dgrad + wgrad tiles in one launch
        from emrt_amd.runtime import ctx
        ctx().wgrad_batch = 0
        try:
            _conv_case_vs_torch(case)
        finally:
            ctx().wgrad_batch = 24


# the 256 x 256 LDS-DMA kernel (csrc/igemm8p.hpp), forced through the dispatcher knob so that every edge it has is exercised
# whatever the size heuristics pick: ragged M (rows past the last pixel), ragged OC (weight rows past OC, tile columns past OC),
# stride 2 forward and its data gradient (stride holes), a 1x1 kernel (one tap), dilation, an odd number of k-tiles (the loop
# multiplies one all-zero tile), two N tiles, and the three layers it is built for at the benchmark's size
CONV_8P = [
    ("8p-uphead-128", 8, 128, 128, 256, 256, 3, 1, 1, True, None),
    ("8p-uphead-64", 8, 64, 64, 256, 256, 3, 1, 1, True, None),
    ("8p-cls_psp-0", 8, 32, 32, 1536, 512, 3, 1, 1, False, None),
    ("8p-ragged-m-oc", 3, 40, 24, 128, 320, 3, 1, 1, True, None),
    ("8p-stride2", 2, 48, 48, 64, 192, 3, 2, 1, False, None),
    ("8p-1x1-odd-ktiles", 2, 30, 34, 192, 256, 1, 1, 0, True, None),
    ("8p-dilated", 2, 32, 32, 64, 64, 3, 1, 2, False, 2),
]


@pytest.mark.parametrize("cmajor", [0, 1])        # tap-major (default) and channel-block-major k order
@pytest.mark.parametrize("case", CONV_8P, ids=[c[0] for c in CONV_8P])
def test_conv_8phase_kernel_bf16_vs_torch(case, cmajor):
    from emrt_amd import _lib
    L_ = _lib.lib()
    old = L_.set_tuning("conv_tile", 7)
    oldp = L_.set_tuning("pair_max", 0)          # the data gradient goes out as its own launch: through the forced tile
    oldc = L_.set_tuning("igemm8p_cmajor", cmajor)
    try:
        _conv_case_vs_torch(case, dilation=case[10] or 1)
    finally:
        L_.set_tuning("conv_tile", old)
        L_.set_tuning("pair_max", oldp)
        L_.set_tuning("igemm8p_cmajor", oldc)


# the 256 x 256 weight-gradient kernel (csrc/wgrad8p.hpp), forced through its knob: one-step blocks (an odd step count multiplies an all-zero
# step), stride 2 (stride holes of the x operand), one tap, dilation, OW = 128 / 8 (both carries of the pixel cursor), two oc tiles with two
# channel blocks, x as a channel slice of a wider buffer is covered by the model tests; partial tiles through the scratch slabs AND fp32
# atomics, forced slice counts with a ragged last slice, and the three layers it is built for at the benchmark's size
WGRAD_8P = [
    ("w8p-uphead-128", 8, 128, 128, 256, 256, 3, 1, 1, True, None),
    ("w8p-uphead-64", 8, 64, 64, 256, 256, 3, 1, 1, True, None),
    ("w8p-cls_psp-0", 8, 32, 32, 1536, 512, 3, 1, 1, False, None),
    ("w8p-one-step", 2, 16, 16, 256, 256, 3, 1, 1, True, None),
    ("w8p-stride2", 2, 32, 32, 256, 512, 3, 2, 1, True, None),
    ("w8p-1x1", 5, 8, 8, 512, 256, 1, 1, 0, True, None),
    ("w8p-dilated", 2, 16, 16, 256, 256, 3, 1, 2, False, 2),
    ("w8p-wide-rows", 1, 8, 128, 256, 256, 3, 1, 1, True, None),
]


@pytest.mark.parametrize("slab,split", [(1, 0), (0, 0), (1, 3), (1, 1)], ids=["slab", "atomics", "slab-3-slices", "one-slice"])
@pytest.mark.parametrize("case", WGRAD_8P, ids=[c[0] for c in WGRAD_8P])
def test_wgrad_8phase_kernel_bf16_vs_torch(case, slab, split):
    from emrt_amd import _lib
    L_ = _lib.lib()
    old = [(k, L_.set_tuning(k, v)) for k, v in (("wgrad8p_force", 1), ("pair_max", 0), ("wgrad8p_slab", slab), ("wgrad_split", split))]
    try:
        _conv_case_vs_torch(case, dilation=case[10] or 1)
    finally:
        for k, v in old:
            L_.set_tuning(k, v)


def test_wgrad_8phase_slab_path_is_bit_reproducible_and_matches_the_128_tile():
    """Partial tiles through the scratch slabs are summed in a fixed order: two launches give identical bits (the fp32-atomic paths do
    not); and the 256 x 256 kernel agrees with the 128 x 128 register-staged one to fp32 summation-order noise."""
    from emrt_amd import _lib
    L_ = _lib.lib()
    c = init(BF16)
    g = torch.Generator().manual_seed(47)
    N, H, W, Cin, Cout = 8, 64, 64, 256, 256
    conv = hnn.Conv2D(Cin, Cout, 3, 1, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(rnd(torch.randn(Cout, Cin, 3, 3, generator=g) / 48))
    Holder(conv=conv).place()
    xd = dev_map(rnd(torch.randn(N, Cin, H, W, generator=g)))
    dyd = dev_map(rnd(torch.randn(N, Cout, H, W, generator=g)))

    def grad():
        conv.weight.grad.zero_()
        tape = Tape()
        c.tape = tape
        y = conv(xd)
        c.tape = None
        tape.add_grad(y, dyd)
        tape.backward()
        torch.cuda.synchronize()
        return conv.weight.grad.clone()

    a, b = grad(), grad()
    assert torch.equal(a, b)
    old = L_.set_tuning("wgrad8p_min_steps", 0)      # 0 = never: the 128 x 128 kernel
    try:
        ref = grad()
    finally:
        L_.set_tuning("wgrad8p_min_steps", old)
    rel = ((a - ref).norm() / ref.norm()).item()
    print("wgrad 256x256 vs 128x128: rel %.2e" % rel)
    assert 0 < rel < 2e-6, rel


def _conv_case_vs_torch(case, dilation=1):
    name, N, H, W, Cin, Cout, k, stride, pad, bias = case[:10]
    c = init(BF16)
    g = torch.Generator().manual_seed(41)
    x = rnd(torch.randn(N, Cin, H, W, generator=g))
    conv = hnn.Conv2D(Cin, Cout, k, stride, pad, bias=bias, dilation=dilation)
    with torch.no_grad():
        conv.weight.copy_(rnd(torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)))
        if bias:
            conv.bias.copy_(torch.randn(Cout, generator=g))
    w_ref, b_ref = conv.weight.detach().clone(), (conv.bias.detach().clone() if bias else None)
    Holder(conv=conv).place()
    xr = x.clone().requires_grad_(True)
    wr = w_ref.clone().requires_grad_(True)
    br = b_ref.clone().requires_grad_(True) if bias else None
    yr = F.conv2d(xr, wr, br, stride=stride, padding=pad, dilation=dilation)
    dy = rnd(torch.randn(yr.shape, generator=g))
    yr.backward(dy)
    xd = dev_map(x)
    tape = Tape()
    c.tape = tape
    y = conv(xd)
    c.tape = None
    tape.watch(xd)
    yh = host_map(y)
    rel = ((yh - yr.detach()).norm() / yr.detach().norm()).item()
    # outputs are O(1); a bf16 store is 2^-9 relative, the fp32 accumulation over K <= 13 824 terms adds ~1e-3 absolute
    close_gemm("conv fwd " + name, yh, yr.detach(), BF16, out_bits=8)          # elementwise: the bf16 store's rounding + summation order (hip_utils.close_gemm)
    assert rel < 4e-3, rel
    dx, = run_bwd(tape, [(y, dev_map(dy))], [xd])
    dxh = host_map(dx)
    rel_dx = ((dxh - xr.grad).norm() / xr.grad.norm()).item()
    rel_dw = ((host(conv.weight.grad) - wr.grad).norm() / wr.grad.norm()).item()
    print("conv %s: fwd rel %.2e, dgrad rel %.2e, wgrad rel %.2e" % (name, rel, rel_dx, rel_dw))
    assert rel_dx < 4e-3, rel_dx          # one bf16 rounding of the stored dx
    assert rel_dw < 1e-3, rel_dw          # fp32 atomics over bf16 operands: only summation-order noise
    close_gemm("conv dgrad " + name, dxh, xr.grad, BF16, out_bits=8)
    close_gemm("conv wgrad " + name, host(conv.weight.grad), wr.grad, BF16)
    if bias:
        rel_db = ((host(conv.bias.grad) - br.grad).norm() / br.grad.norm()).item()
        assert rel_db < 1e-3, rel_db


def test_wgrad_fp32_atomics_run_to_run_spread_is_bounded():
    """The weight gradient is summed with fp32 atomics over blockIdx.z slices (atomics-based backward): the
    order of the adds differs between launches, so results are NOT bit-reproducible; the spread must stay at fp32
    rounding level (relative 1e-6 of the gradient norm), three orders below the bf16 noise of the operands."""
    c = init(BF16)
    g = torch.Generator().manual_seed(43)
    N, H, W, Cin, Cout = 8, 64, 64, 256, 256
    conv = hnn.Conv2D(Cin, Cout, 3, 1, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(rnd(torch.randn(Cout, Cin, 3, 3, generator=g) / 48))
    Holder(conv=conv).place()
    xd = dev_map(rnd(torch.randn(N, Cin, H, W, generator=g)))
    dyd = dev_map(rnd(torch.randn(N, Cout, H, W, generator=g)))
    grads = []
    for _ in range(2):
        conv.weight.grad.zero_()
        conv.bias.grad.zero_()
        tape = Tape()
        c.tape = tape
        y = conv(xd)
        c.tape = None
        tape.add_grad(y, dyd)
        tape.backward()
        torch.cuda.synchronize()
        grads.append((conv.weight.grad.clone(), conv.bias.grad.clone()))
    dw = (grads[0][0] - grads[1][0]).norm().item() / grads[0][0].norm().item()
    db = (grads[0][1] - grads[1][1]).norm().item() / grads[0][1].norm().item()
    print("wgrad run-to-run relative spread: dW %.2e, dbias %.2e" % (dw, db))
    assert dw < 2e-6 and db < 2e-6, (dw, db)


# -----------------------------------------------------------------------------------------------------------------
# the whole model in bf16 -- the benchmark's dtype -- at the benchmark's size, against the fp32 oracle
# -----------------------------------------------------------------------------------------------------------------
# A randomly initialised BatchNorm network is chaotic in depth (tests/test_gpu_model.py: condition_residual_branches), so the
# comparison is made (1) on weights whose residual branches are down-weighted as in a trained / zero-init-residual network,
# with absolute bounds, and (2) always next to the yardstick "torch's own CPU bf16 autocast of the same fp32 oracle": the HIP
# path stores activations in bf16 exactly where autocast does, so it must not be further from fp32 than autocast is.
# Bounds (measured values are printed; see DESIGN.md "Parity results"):
BF16_LOGIT_REL_L2 = 0.06        # ||logits_bf16 - logits_ref|| / ||logits_ref||, main and aux head (conditioned weights)
BF16_ARGMAX_AGREE = 0.95        # fraction of pixels with the same argmax class (all pixels, near-ties included)
BF16_DECISIVE_AGREE = 0.999     # ... among pixels whose fp32 top-2 margin exceeds 10 % of the logit range
BF16_VS_AUTOCAST = 1.25         # HIP error <= 1.25 x (torch CPU bf16 autocast error) + 0.005, both vs the fp32 oracle
BF16_LOSS_REL = 2e-3
BF16_GRAD_COSINE = 0.985        # cosine between the whole bf16 gradient vector and the fp32 oracle's
BF16_GRAD_NORM_RATIO = 0.02     # | ||g_bf16|| / ||g_ref|| - 1 |


@pytest.mark.parametrize("B,S,ncls", [(8, 256, 6)], ids=["cfg2-8x256"])      # (cfg3-4x512: tests/test_gpu_bench_shapes_cfg3.py, a file of its own for pytest-xdist)
def test_full_size_bf16_model_vs_fp32_oracle(B, S, ncls):
    full_size_bf16_model_case(B, S, ncls)


def full_size_bf16_model_case(B, S, ncls):
    """BASELINE configs[1] (ResNet-50, batch 8, 256x256, 6 classes) and configs[2] (LoveDA geometry: batch 4, 512x512, 7 classes,
    Lv = 5376 -- the row-band MSDA kernels, the query-split scatter) in THEIR OWN dtype and batch: bf16 storage / fp32 accumulation
    against the fp32 CPU oracle (the reference is fp32 throughout, train.py:141-159): eval-mode logits and argmax masks, then one
    train-mode forward + loss + backward (dropout off: the oracle cannot share the device's mask stream)."""
    from tests.test_gpu_model import build_pair, make_config
    from emrt_amd.src.models.losses import get_loss_function
    from oracle import train_ref
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, 3, S, S, generator=g)
    labels = torch.randint(0, ncls, (B, S, S), generator=g)
    labels[torch.rand(B, S, S, generator=g) < 0.02] = 255
    ref, model = build_pair("resnet50", x, dtype=BF16, perturb=True, condition=0.1, ncls=ncls)
    # ---- eval-mode logits (running statistics calibrated on this batch) ---------------------------------------------
    ref.eval()
    model.eval()
    with torch.no_grad():
        want = ref(x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            yard = [t.float() for t in ref(x)]
    got = model(x.cuda())
    for name, a, b, y in (("main", got[0].cpu(), want[0], yard[0]), ("aux", got[1].cpu(), want[1], yard[1])):
        rel = ((a - b).norm() / b.norm()).item()
        rel_y = ((y - b).norm() / b.norm()).item()
        agree = (a.argmax(1) == b.argmax(1)).float().mean().item()
        agree_y = (y.argmax(1) == b.argmax(1)).float().mean().item()
        top2 = b.topk(2, dim=1).values
        margin = top2[:, 0] - top2[:, 1]
        decisive = margin > 0.1 * (b.max() - b.min())
        agree_dec = (a.argmax(1) == b.argmax(1))[decisive].float().mean().item()
        print("bf16 eval %dx%dx%d %s logits: rel L2 %.4f (torch CPU autocast: %.4f), max |diff| %.4f (|ref| max %.3f), argmax agreement %.5f (autocast %.5f) "
              "= %d of %d pixels differ, among %d decisive pixels %.6f" % (B, S, S, name, rel, rel_y, (a - b).abs().max().item(), b.abs().max().item(), agree, agree_y,
                                                   int((a.argmax(1) != b.argmax(1)).sum()), a.argmax(1).numel(), int(decisive.sum()), agree_dec))
        assert rel < BF16_LOGIT_REL_L2, (name, rel)
        assert rel <= BF16_VS_AUTOCAST * rel_y + 0.005, (name, rel, rel_y)
        assert agree >= BF16_ARGMAX_AGREE and agree >= agree_y - 0.01, (name, agree, agree_y)
        assert agree_dec >= BF16_DECISIVE_AGREE, (name, agree_dec)
    # ---- one training step's forward / loss / backward ------------------------------------------------------------------
    ref.train()
    out_r = ref(x)
    loss_r = train_ref.mix_softmax_ce_loss(out_r, labels)
    loss_r.backward()
    model.train()
    model.clear_gradients()
    out = model(x.cuda())
    loss = get_loss_function(make_config("resnet50", ncls=ncls))(out, labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    rel_main = ((out[0].cpu() - out_r[0].detach()).norm() / out_r[0].detach().norm()).item()
    rel_loss = abs(loss.item() - loss_r.item()) / abs(loss_r.item())
    refp = dict(ref.named_parameters())
    dot = n_hip = n_ref = 0.0
    per = []
    for n, p in model.named_parameters():
        gr = refp[n].grad
        if gr is None:
            continue
        gg, gr = p.grad.cpu().double(), gr.double()
        dot += float((gg * gr).sum())
        n_hip += float((gg * gg).sum())
        n_ref += float((gr * gr).sum())
        if gr.norm() > 0:
            per.append((float((gg * gr).sum() / (gg.norm() * gr.norm() + 1e-300)), n))
    cos = dot / (n_hip ** 0.5 * n_ref ** 0.5)
    ratio = (n_hip / n_ref) ** 0.5
    per.sort()
    print("bf16 train step: logits rel L2 %.4f, loss %.5f vs %.5f (rel %.2e), gradient cosine %.5f, norm ratio %.4f, worst per-parameter cosines %s" % (
        rel_main, loss.item(), loss_r.item(), rel_loss, cos, ratio, per[:4]))
    assert rel_main < BF16_LOGIT_REL_L2 and rel_loss < BF16_LOSS_REL
    assert cos > BF16_GRAD_COSINE and abs(ratio - 1.0) < BF16_GRAD_NORM_RATIO, (cos, ratio)
