"""The deformable-attention kernels' operation (csrc/msda.hip: emrt_msda_fwd / emrt_msda_bwd) restated in float64, the error measure of
the sweep in tests/test_gpu_msda_fuzz.py, and the reference-side calibration of its bounds (tests/test_msda_reference_cpu.py).  No GPU and
no library import: everything here is plain torch on the CPU.

value [B, Lv, M * 32], offw [B, Lq, 3 M L P] (M L P (x, y) offsets in pixels of the sample's level, then M L P logits), ref [B or 1, Lq,
ref_L, 2] (ref_L = 1: one point for every level), dout [B, Lq, M * 32]; level l is H_l x W_l, its pixels start at sum_{t < l} H_t W_t.
Per (batch b, query q, head m), sample (l, p), corner c in {00, 01, 10, 11}, written from the expressions of msda.hip (MsdaPrep::run,
msda_bwd_kernel):

  a  = softmax over the L P logits            x = (ref_x + off_x / W_l) W_l - 0.5      y likewise with H_l
  x0 = floor(x), lx = x - x0 (y0, ly)         bw_c = (ly | 1 - ly) (lx | 1 - lx)       ok_c = corner inside the map (zero padding)
  out      = sum a bw_c ok_c value[pixel_c]                                           d_c = ok_c <dout, value[pixel_c]>
  dvalue[pixel_c] += a bw_c ok_c dout
  dA = sum_c bw_c d_c                          dlogit = a (dA - sum a dA)
  doff_x = a ((1 - ly) (d01 - d00) + ly (d11 - d10))          doff_y = a ((1 - lx) (d10 - d00) + lx (d11 - d01))
  dref_x(l) = W_l sum_{m, p} doff_x            (ref_L = 1: summed over l as well; reference points shared by the batch: summed over b)

Levels and corners are walked in a loop: one gather is [B, Lq, M, P, 32], never [.., L P, 4, 32].

Error measure: PER ROW, relative to the row of `magnitude` -- the same expressions with absolute values on both operands of every product
and sums in place of the differences, which is what rounding errors scale with and which cannot cancel:
    out:     rows (b, q, m) over the 32 channels            doffw: rows (b, q, m), the 2 L P offset gradients and the L P logit gradients apart
    dvalue:  rows (b, pixel, m) over the 32 channels        dref:  rows (b, q[, l]) over (x, y)
    err(row) = || got - exact ||_2 / || magnitude ||_2, maximised over rows; a row of magnitude 0 must be reproduced exactly.
dvalue only: both scatter kernels accumulate in FIXED point, so each of the n addends of a row carries an error that does not shrink
with the addend.  msda.hip states the resolutions: the integer LDS scatter quantises every addend to R = Lq max|dout over (b, m)| 2^-30
(msda_bwd_value_lds_kernel), the matrix-product scatter every weight to 2^-24, i.e. R = max|dout over (b, m)| 2^-24 per addend
(msda_bwd_value_mfma_kernel).  A pixel reached only by a corner of weight 1e-6 would have an unbounded RELATIVE error under a correct
kernel, so the dvalue row is measured against
    || magnitude ||_2 + sqrt(32) n R / (2 u)           n = corners of non-zero weight that land on the pixel, u = 2^-9 (bf16) | 2^-24 (fp32)
-- the worst case n R / 2 per channel, expressed in units of the stored type's rounding so that one constant bounds both parts.  Pixels
with n = 0 are not measured but must come back as exact zeros (the GPU test asserts it).

Bounds (MSDA_BOUND): constants, calibrated on the CPU only.  The floor of a (dtype, tensor) is the worst per-row error, over every case of
the sweep (tests/fuzz_cases.py, op "msda"), of the best a correct kernel can do:
  16-bit: the exact values with the kernels' stated roundings.  contract_16 (forward, bf16 and fp16): corner weights rounded to the value
          type (pack16), fp32 products and sums, the output rounded once.  contract_bwd: doffw and dvalue rounded to bf16 on store, the
          integer scatter's addends rounded to R, the matrix-product scatter's (pixel, query) weight summed in 2^-24 fixed point and rounded
          once to bf16.  bound = 3 x floor: the model has every stated rounding, the factor covers fp32 arithmetic and __expf.
  fp32 and dref (an fp32 sum of unrounded terms in every dtype): evaluate_f32 -- the same chain in fp32 torch, dvalue through the integer
          scatter's model.  bound = 16 x floor: __expf, fp32 atomics in any order, another summation order than torch's.
tests/test_msda_reference_cpu.py recomputes the floors and asserts floor <= bound / 3 (16-bit), bound / 16 (fp32, dref); it also asserts
that the mutants below -- wrong on purpose, each with one named cause -- exceed 2 x bound in the regime built for them.
"""
import math

import torch

from tests.fuzz_cases import msda_band_geometry

F64 = torch.float64
D = 32
UNIT = {"f32": 2.0 ** -24, "bf16": 2.0 ** -9, "f16": 2.0 ** -11}
CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))
NEAR_LINE, NUDGE, NEAR_RANGE = 2.0 ** -10, 2.0 ** -9, 4096.0

# Per-row error bounds of the GPU sweep.  Floors measured by tests/test_msda_reference_cpu.py::test_floors_and_bounds over the sweep's cases
# (it prints them):
#                                   out       doff      dlogit    dvalue: lds   mf        spike-lds  spike-mf    dref
#   bf16 contract floor           4.793e-3  2.647e-3  1.879e-3    2.561e-3   4.974e-3   3.281e-3   5.585e-3   (fp32 torch) 4.045e-7
#   fp16 contract floor (forward) 4.651e-4
#   fp32 torch floor              3.770e-4  4.165e-6  7.280e-5    4.178e-8      --      1.713e-8      --       2.261e-7
# bound = 3 x floor (16-bit), rounded up in the third digit; 16 x floor (fp32, and dref in every dtype), rounded up in the second.
# The 16-bit floors are roundings of the stored type: 2^-9 = 1.95e-3 (bf16), 2^-11 = 4.88e-4 (fp16), once for doffw and the integer
# scatter's dvalue, twice and a bit for out (weights, then the sum) and the matrix-product dvalue (the (pixel, query) weight, then the sum).
# The fp32 floors of out, doff and dlogit come from the far regime (sigma = 40 pixels): coordinates of ~100 carry an fp32 error of ~1e-5
# pixel, which is 1e-2 of a bilinear weight of 1e-3 -- and where every other sample of the row lies outside, that corner IS the row.
MSDA_BOUND = {
    "bf16": {"out": 1.44e-2, "doff": 7.95e-3, "dlogit": 5.64e-3,
             "dvalue": {"lds": 7.69e-3, "mf": 1.50e-2, "spike-lds": 9.85e-3, "spike-mf": 1.68e-2}, "dref": 6.5e-6},
    "f16": {"out": 1.40e-3},
    "f32": {"out": 6.1e-3, "doff": 6.7e-5, "dlogit": 1.2e-3, "dvalue": {"lds": 6.7e-7, "spike-lds": 2.8e-7}, "dref": 3.7e-6},
}
FLOOR_MARGIN = {"bf16": 3.0, "f16": 3.0, "f32": 16.0}
DREF_MARGIN = 16.0


def round_to(x, dtype):
    """float64 values of x rounded through the compute dtype ('f32' | 'bf16' | 'f16')"""
    t = x.to(torch.float32)
    if dtype == "bf16":
        t = t.to(torch.bfloat16)
    elif dtype == "f16":
        t = t.to(torch.float16)
    return t.to(F64)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _coords(offw, ref, shapes, M, P):
    """float64 pixel coordinates (x, y) of every sample: [B, Lq, M, L, P] each"""
    B, Lq = offw.shape[:2]
    L = len(shapes)
    off = offw[..., :2 * M * L * P].reshape(B, Lq, M, L, P, 2).to(F64)
    xs, ys = [], []
    for l, (h, w) in enumerate(shapes):
        r = ref[:, :, l if ref.shape[2] == L else 0].to(F64)
        xs.append((r[..., 0].reshape(-1, Lq, 1, 1) + off[:, :, :, l, :, 0] / w) * w - 0.5)
        ys.append((r[..., 1].reshape(-1, Lq, 1, 1) + off[:, :, :, l, :, 1] / h) * h - 0.5)
    return torch.stack(xs, 3), torch.stack(ys, 3)


def line_distance(offw, ref, shapes, M, P):
    """the smallest distance of a float64 coordinate with |coordinate| < 4096 from an integer line"""
    x, y = _coords(offw, ref, shapes, M, P)
    c = torch.cat([x.reshape(-1), y.reshape(-1)])
    c = c[c.abs() < NEAR_RANGE]
    return ((c - c.round()).abs().min().item()) if c.numel() else float("inf")


def _nudge(offw, ref, shapes, M, P):
    """move every offset whose coordinate lies within 2^-10 pixel of an integer line (|coordinate| < 4096) away from it by 2^-9 pixel"""
    B, Lq = offw.shape[:2]
    L = len(shapes)
    n = 2 * M * L * P
    for _ in range(4):
        x, y = _coords(offw, ref, shapes, M, P)
        xy = torch.stack([x, y], -1)                                          # [B, Lq, M, L, P, 2]
        d = xy - xy.round()
        near = (d.abs() < NEAR_LINE) & (xy.abs() < NEAR_RANGE)
        if not near.any():
            return offw
        step = torch.where(d >= 0, torch.full_like(d, NUDGE), torch.full_like(d, -NUDGE)) * near
        off = offw[..., :n].reshape(B, Lq, M, L, P, 2) + step
        offw = torch.cat([off.reshape(B, Lq, n).to(torch.float32).to(F64), offw[..., n:]], -1)
    raise AssertionError("offsets still within 2^-10 of an integer line after four passes")


def _centres(shapes):
    """the encoder's reference points: pixel centres of every level, level by level, row-major -> [Lv, 2] (x, y)"""
    pts = []
    for h, w in shapes:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=F64) + 0.5, torch.arange(w, dtype=F64) + 0.5, indexing="ij")
        pts.append(torch.stack([xx.reshape(-1) / w, yy.reshape(-1) / h], -1))
    return torch.cat(pts, 0)


def make_inputs(case, dtype):
    """dict(value, offw, ref, dout) in float64: value and dout rounded through `dtype`, offw and ref through fp32.  case: a tuple of
    tests/fuzz_cases.py, op "msda".  Regimes, each built so that one fault is an O(1) error in some row:
      ordinary:  offsets N(0, sigma) pixels, sigma = 0.3 (even seed) | 2.5 (odd)
      far:       sigma = 8 (even seed) | 40 (odd): many samples wholly outside and beyond a band's halo; query 64 k + 5 of head k mod M has
                 offsets of +-1e9 (the clamp of the integer conversion)
      border:    every sample has x0 = -1, x0 = W - 1, y0 = -1 or y0 = H - 1 (by p mod 4): one or two valid corners, the slab's guard bands
      bandedge:  band plans: sample p of level t aims at row c0 - halo - 1, c0 - halo, c1 + halo - 1 or c1 + halo (by p mod 4) of the query's
                 own band -- just outside, just inside, half outside, outside the staged rows; every sample is such a one
      centres:   power-of-two levels, reference points at pixel centres, integer offsets: every coordinate is a dyadic rational, exact in
                 fp32 and float64 alike, lx = ly = 0 at the query's own level
      spike:     dout = 0.01 with one 1000.0 per (batch, head), on query 64 k + 63 (the last row of a 64-row part, row lane >= 8 of the
                 max |dout| scan)
      lastquery: dout of query Lq - 1 is 100 x the others; its samples fall into the last two rows of every level, where every other
                 query's samples get a logit of -30
    Reference points: the levels' pixel centres when Lq = Lv (self-attention over the pyramid), uniform otherwise; ref_L = L moves the point of
    level l by up to 0.75 of that level's pixels (reading another level's point is then an O(1) error), per-batch points differ by +-0.01."""
    cid, B, M, shapes, Lq, P, regime, layout, refmode, knobs, expect, seed = case
    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    Lv = sum(h * w for h, w in shapes)
    self_attn = Lq is None
    Lq = Lq or Lv
    tp = M * L * P
    sizes = torch.tensor([[w, h] for h, w in shapes], dtype=F64)            # [L, 2] (W, H)
    shared, per_level = refmode.startswith("shared"), refmode.partition("+")[0].endswith("L")
    Br, refL = (1 if shared else B), (L if per_level else 1)
    base = _centres(shapes) if self_attn else torch.rand(Lq, 2, generator=g, dtype=F64)
    ref = base.reshape(1, Lq, 1, 2).expand(Br, Lq, refL, 2).clone()
    if regime != "centres":
        if per_level:
            ref = ref + (torch.rand(Br, Lq, refL, 2, generator=g, dtype=F64) - 0.5) * 1.5 / sizes.reshape(1, 1, L, 2)
        elif not shared:
            ref = ref + (torch.rand(Br, Lq, 1, 2, generator=g, dtype=F64) - 0.5) * 0.02
    ref = ref.to(torch.float32).to(F64)
    value = round_to(torch.randn(B, Lv, M * D, generator=g, dtype=F64), dtype)
    dout = torch.randn(B, Lq, M * D, generator=g, dtype=F64)
    logit = torch.randn(B, Lq, M, L, P, generator=g, dtype=F64)
    sigma = {"ordinary": (0.3, 2.5), "far": (8.0, 40.0)}.get(regime, (1.5, 1.5))[seed % 2]
    off = torch.randn(B, Lq, M, L, P, 2, generator=g, dtype=F64) * sigma
    refl = ref.expand(B, Lq, refL, 2)
    refl = (refl if per_level else refl.expand(B, Lq, L, 2)).reshape(B, Lq, 1, L, 1, 2)       # the point level l's samples start from
    pos = refl * sizes.reshape(1, 1, 1, L, 1, 2)                                                # ... in pixels of that level (x + 0.5)
    frac = 0.15 + 0.7 * torch.rand(B, Lq, M, L, P, 2, generator=g, dtype=F64)

    def aim(cell):
        """offsets that put floor(coordinate) at `cell` (integer-valued tensor) with a fraction in (0.15, 0.85)"""
        return cell + frac + 0.5 - pos

    pk = (torch.arange(P) % 4).reshape(1, 1, 1, 1, P)
    if regime == "far":
        for k in range((Lq + 58) // 64):
            q = 64 * k + 5
            if q < Lq:
                off[:, q, k % M] = torch.where(torch.rand(L, P, 2, generator=g) < 0.5, -1.0e9, 1.0e9).to(F64)
    elif regime == "border":
        hw = sizes.reshape(1, 1, 1, L, 1, 2)
        inside = torch.floor(torch.rand(B, Lq, M, L, P, 2, generator=g, dtype=F64) * hw)
        edge = torch.where(pk.unsqueeze(-1) % 2 == 0, torch.full((1,), -1.0, dtype=F64), hw - 1)          # p even: cell -1, p odd: the last cell
        axis = torch.arange(2).reshape(1, 1, 1, 1, 1, 2) == (pk >= 2).unsqueeze(-1).long()                 # p mod 4 in (0, 1): x on the border, else y
        off = aim(torch.where(axis, edge, inside))
    elif regime == "bandedge":
        NB, halo = msda_band_geometry(shapes, B, M, knobs.get("msda_band_halo", 0))[:2]
        assert self_attn and NB, "bandedge needs a band plan"
        qrow = torch.cat([torch.arange(h).repeat_interleave(w) for h, w in shapes])             # the query's row in its own level
        qlev = torch.cat([torch.full((h * w,), l) for l, (h, w) in enumerate(shapes)])
        hs = torch.tensor([h for h, _ in shapes])
        band = qrow // (hs[qlev] // NB)                                                         # [Lq]
        c0 = band.reshape(Lq, 1) * (hs.reshape(1, L) // NB)                                     # [Lq, L] first own row of the band, per level
        c1 = c0 + hs.reshape(1, L) // NB
        rows = torch.stack([c0 - halo - 1, c0 - halo, c1 + halo - 1, c1 + halo], -1).to(F64)    # [Lq, L, 4]
        tgt = rows[:, :, torch.arange(P) % 4].reshape(1, Lq, 1, L, P).expand(B, Lq, M, L, P)
        colx = torch.floor(torch.rand(B, Lq, M, L, P, generator=g, dtype=F64) * sizes[:, 0].reshape(1, 1, 1, L, 1))
        off = aim(torch.stack([colx, tgt], -1))
    elif regime == "centres":
        assert all(h & (h - 1) == 0 and w & (w - 1) == 0 for h, w in shapes), "centres needs power-of-two levels"
        if not self_attn:
            h0, w0 = shapes[0]
            ref = torch.stack([(torch.randint(0, w0, (Lq,), generator=g).to(F64) + 0.5) / w0,
                               (torch.randint(0, h0, (Lq,), generator=g).to(F64) + 0.5) / h0], -1).reshape(1, Lq, 1, 2).expand(Br, Lq, refL, 2).clone()
        off = torch.randint(-3, 4, (B, Lq, M, L, P, 2), generator=g).to(F64)
    elif regime == "spike":
        dout = torch.full_like(dout, 0.01)
        for b in range(B):
            for m in range(M):
                q = min(Lq - 1, 64 * int(torch.randint(0, max(1, Lq // 64), (1,), generator=g)) + 63)
                dout[b, q, m * D + int(torch.randint(0, D, (1,), generator=g))] = 1000.0
    elif regime == "lastquery":
        hw = sizes.reshape(1, 1, 1, L, 1, 2)
        cell = torch.stack([torch.floor(torch.rand(B, 1, M, L, P, generator=g, dtype=F64) * (sizes[:, 0].reshape(1, 1, 1, L, 1) - 1)),
                            (sizes[:, 1].reshape(1, 1, 1, L, 1) - 2).clamp_min(0).expand(B, 1, M, L, P)], -1)
        off[:, Lq - 1:] = (aim(cell.expand(B, Lq, M, L, P, 2)))[:, Lq - 1:]
        y = pos[..., 1] + off[..., 1] - 0.5                                                     # other queries: keep out of the last two rows
        hit = (torch.floor(y) + 1 >= (hw[..., 1] - 2).clamp_min(0)) & (torch.floor(y) < hw[..., 1])
        hit[:, Lq - 1] = False
        logit = torch.where(hit, torch.full_like(logit, -30.0), logit)
        dout[:, Lq - 1] *= 100.0
    else:
        assert regime == "ordinary", regime
    dout = round_to(dout, dtype)
    offw = torch.cat([off.reshape(B, Lq, 2 * tp), logit.reshape(B, Lq, tp)], -1).to(torch.float32).to(F64)
    if regime != "centres":
        offw = _nudge(offw, ref, shapes, M, P)
    return dict(value=value, offw=offw, ref=ref.contiguous(), dout=dout)


# ---- the operation --------------------------------------------------------------------------------------------------------------
def _chain(inp, shapes, M, P, dt=F64, absolute=False, wround=None, drop=None, ref_level0=False):
    """dict(out [B, Lq, M, 32], dvalue [B, Lv, M, 32], count [B, Lv, M], doff [B, Lq, M, L P 2], dlogit [B, Lq, M, L P], dref [B, Lq, ref_L, 2],
    corners) in dtype dt.
    absolute: the magnitudes instead (see the module docstring); wround: rounding of a corner weight in the forward sum (pack16);
    drop(l, x0, y0, (vx0, vx1, vy0, vy1)) -> bool [B, Lq, M, P]: samples whose corners all count as outside (the mutants); ref_level0:
    every level reads level 0's point.  corners: per level and corner (token rows [B, Lq, M, P] of the [B Lv M, 32] view, weight) for the
    scatter models."""
    value, offw, ref, dout = (inp[k].to(dt) for k in ("value", "offw", "ref", "dout"))
    B, Lv, _ = value.shape
    Lq = offw.shape[1]
    L = len(shapes)
    tp = M * L * P
    off = offw[..., :2 * tp].reshape(B, Lq, M, L, P, 2)
    a = torch.softmax(offw[..., 2 * tp:3 * tp].reshape(B, Lq, M, L * P), -1).reshape(B, Lq, M, L, P)
    val = value.reshape(B * Lv * M, D)
    g = dout.reshape(B, Lq, M, 1, D)
    if absolute:
        val, g = val.abs(), g.abs()
    sgn = 1.0 if absolute else -1.0
    bi = torch.arange(B).reshape(B, 1, 1, 1)
    mi = torch.arange(M).reshape(1, 1, M, 1)
    out = torch.zeros(B, Lq, M, D, dtype=dt)
    dval = torch.zeros(B * Lv * M, D, dtype=dt)
    count = torch.zeros(B * Lv * M, dtype=dt)
    dA, gx, gy, corners = [], [], [], []
    refL = ref.shape[2]
    start = 0
    for l, (h, w) in enumerate(shapes):
        r = ref[:, :, l if (refL == L and not ref_level0) else 0]
        rx, ry = r[..., 0].reshape(-1, Lq, 1, 1), r[..., 1].reshape(-1, Lq, 1, 1)
        ox, oy = off[:, :, :, l, :, 0], off[:, :, :, l, :, 1]
        if dt == F64:
            x, y = (rx + ox / w) * w - 0.5, (ry + oy / h) * h - 0.5
        else:       # as the kernels write it: the division is a multiplication by the fp32 reciprocal
            iw, ih = torch.tensor(1.0, dtype=dt) / torch.tensor(float(w), dtype=dt), torch.tensor(1.0, dtype=dt) / torch.tensor(float(h), dtype=dt)
            x, y = (rx + ox * iw) * float(w) - 0.5, (ry + oy * ih) * float(h) - 0.5
        xf, yf = x.floor(), y.floor()
        lx, ly = x - xf, y - yf
        x0, y0 = xf.clamp(-2.0, 16777216.0).long(), yf.clamp(-2.0, 16777216.0).long()
        vx = ((x0 >= 0) & (x0 < w), (x0 + 1 >= 0) & (x0 + 1 < w))
        vy = ((y0 >= 0) & (y0 < h), (y0 + 1 >= 0) & (y0 + 1 < h))
        dropped = drop(l, x0, y0, (vx[0], vx[1], vy[0], vy[1])) if drop is not None else None
        al = a[:, :, :, l]
        d = {}
        for cy, cx in CORNERS:
            bw = (ly if cy else 1.0 - ly) * (lx if cx else 1.0 - lx)
            ok = vy[cy] & vx[cx]
            if dropped is not None:
                ok = ok & ~dropped
            wgt = al * bw * ok.to(dt)
            pix = start + (y0 + cy).clamp(0, h - 1) * w + (x0 + cx).clamp(0, w - 1)
            rows = (bi * Lv + pix) * M + mi
            v = val[rows]                                                                     # [B, Lq, M, P, 32]
            wf = wgt if wround is None else wround(wgt)
            out += (wf.unsqueeze(-1) * v).sum(3)
            d[(cy, cx)] = (g * v).sum(-1) * ok.to(dt)
            dval.index_add_(0, rows.reshape(-1), (wgt.unsqueeze(-1) * g).reshape(-1, D))
            count.index_add_(0, rows.reshape(-1), (wgt > 0).to(dt).reshape(-1))
            corners.append((l, rows, wgt))
        dA.append((1.0 - ly) * ((1.0 - lx) * d[0, 0] + lx * d[0, 1]) + ly * ((1.0 - lx) * d[1, 0] + lx * d[1, 1]))
        gx.append(al * ((1.0 - ly) * (d[0, 1] + sgn * d[0, 0]) + ly * (d[1, 1] + sgn * d[1, 0])))
        gy.append(al * ((1.0 - lx) * (d[1, 0] + sgn * d[0, 0]) + lx * (d[1, 1] + sgn * d[0, 1])))
        start += h * w
    dA, gx, gy = torch.stack(dA, 3), torch.stack(gx, 3), torch.stack(gy, 3)                # [B, Lq, M, L, P]
    dot = (a * dA).sum((3, 4), keepdim=True)
    dlogit = a * (dA + sgn * dot)
    sizes = torch.tensor([[w, h] for h, w in shapes], dtype=dt)
    per_level = torch.stack([gx.sum((2, 4)), gy.sum((2, 4))], -1) * sizes.reshape(1, 1, L, 2)      # [B, Lq, L, 2]
    dref = per_level if refL == L else per_level.sum(2, keepdim=True)
    return dict(out=out, dvalue=dval.reshape(B, Lv, M, D), count=count.reshape(B, Lv, M), doff=torch.stack([gx, gy], -1).reshape(B, Lq, M, L * P * 2),
                dlogit=dlogit.reshape(B, Lq, M, L * P), dref=dref, corners=corners)


def exact(inp, shapes, M, P, **kw):
    return _chain(inp, shapes, M, P, **kw)


def magnitude(inp, shapes, M, P):
    return _chain(inp, shapes, M, P, absolute=True)


def evaluate_f32(inp, shapes, M, P):
    """the same chain in fp32 torch"""
    return _chain(inp, shapes, M, P, dt=torch.float32)


def contract_16(inp, shapes, M, P, dtype):
    """the 16-bit forward with its stated roundings (MsdaPrep::pack16, msda_dot_row): corner weights in the value type, fp32 products and
    sums (exact here), the output rounded once"""
    return round_to(_chain(inp, shapes, M, P, wround=lambda t: round_to(t, dtype))["out"], dtype)


def absmax_bm(dout, M):
    """max |dout| per (batch, head): [B, M]"""
    B, Lq, _ = dout.shape
    return dout.reshape(B, Lq, M, D).abs().amax((1, 3))


def resolution(dout, M, kind):
    """R of the module docstring, [B, M]: the absolute size of one fixed-point step of the scatter, in dvalue's units"""
    gm = absmax_bm(dout.to(F64), M)
    return gm * dout.shape[1] * 2.0 ** -30 if kind == "lds" else gm * 2.0 ** -24


def scatter_lds(ch, inp, M, dtype, gmax=None, wrap=False):
    """dvalue as msda_bwd_value_lds_kernel makes it: scale = 2^30 / (Lq max|dout over (b, m)|) in fp32, every addend rint(dout scale w),
    integer sums, one multiplication by 1 / scale, one rounding to the stored type.  ch: a _chain result (its corner weights are used).
    gmax / wrap: the spike mutant (another maximum; the int32 accumulator wraps)."""
    dout = inp["dout"].to(F64)
    B, Lq, _ = dout.shape
    Lv = ch["dvalue"].shape[1]
    gm = (absmax_bm(dout, M) if gmax is None else gmax).to(torch.float32)
    lqm = torch.tensor(float(Lq), dtype=torch.float32) * gm
    scale = torch.where(gm > 0, torch.tensor(1073741824.0, dtype=torch.float32) / lqm, torch.zeros_like(gm)).to(F64)      # [B, M]
    inv_scale = torch.where(gm > 0, lqm * torch.tensor(1.0 / 1073741824.0, dtype=torch.float32), torch.zeros_like(gm)).to(F64)
    gs = (dout.reshape(B, Lq, M, 1, D) * scale.reshape(B, 1, M, 1, 1)).to(torch.float32).to(F64)
    acc = torch.zeros(B * Lv * M, D, dtype=F64)
    for _, rows, wgt in ch["corners"]:
        acc.index_add_(0, rows.reshape(-1), torch.round(gs * wgt.to(torch.float32).to(F64).unsqueeze(-1)).reshape(-1, D))
    if wrap:
        acc = torch.remainder(acc + 2.0 ** 31, 2.0 ** 32) - 2.0 ** 31
    return round_to(acc.reshape(B, Lv, M, D) * inv_scale.reshape(B, 1, M, 1), dtype)


def scatter_mf(ch, inp, M):
    """dvalue as msda_bwd_value_mfma_kernel makes it: the weights of a (pixel, query) pair summed as rint(w 2^24) integers, the sum rounded
    once to bf16, fp32 products with dout and fp32 sums (exact here), one rounding to bf16"""
    dout = inp["dout"].to(F64)
    B, Lq, _ = dout.shape
    Lv = ch["dvalue"].shape[1]
    qi = torch.arange(Lq).reshape(1, Lq, 1, 1)
    keys, vals = [], []
    for _, rows, wgt in ch["corners"]:
        keys.append((rows * Lq + qi).reshape(-1))
        vals.append(torch.round(wgt.to(torch.float32).to(F64) * 16777216.0).reshape(-1))
    keys, vals = torch.cat(keys), torch.cat(vals)
    uniq, inv = torch.unique(keys, return_inverse=True)
    tile = torch.zeros(uniq.numel(), dtype=F64).index_add_(0, inv, vals)
    wq = round_to(tile / 16777216.0, "bf16")
    rows, q = uniq // Lq, uniq % Lq                                  # rows = (b Lv + pixel) M + m
    b, m = rows // (Lv * M), rows % M
    gsel = dout.reshape(B, Lq, M, D)[b, q, m]
    acc = torch.zeros(B * Lv * M, D, dtype=F64).index_add_(0, rows, wq.unsqueeze(-1) * gsel)
    return round_to(acc.reshape(B, Lv, M, D), "bf16")


def contract_bwd(inp, shapes, M, P, dtype, kind):
    """the backward with its stated roundings.  bf16: doffw rounded to bf16 on store (store_doffw), dvalue by the model of scatter `kind`
    ('lds' | 'mf'); dref is an fp32 sum of unrounded terms.  f32: the fp32 chain, dvalue through the integer scatter's model."""
    ch = _chain(inp, shapes, M, P, dt=torch.float32 if dtype == "f32" else F64)
    res = {k: ch[k].to(F64) for k in ("doff", "dlogit", "dref")}
    if dtype == "bf16":
        res["doff"], res["dlogit"] = round_to(res["doff"], "bf16"), round_to(res["dlogit"], "bf16")
    res["dvalue"] = scatter_mf(ch, inp, M) if kind == "mf" else scatter_lds(ch, inp, M, dtype)
    return res


# ---- mutants: wrong on purpose, on the reference side only ----------------------------------------------------------------------
def band_rows(shapes, NB, halo):
    """(band of every query [Lv], lo [NB, L], hi [NB, L]): the rows band k stages of level l, as msda_fwd_band_kernel computes them"""
    hs = torch.tensor([h for h, _ in shapes])
    qrow = torch.cat([torch.arange(h).repeat_interleave(w) for h, w in shapes])
    qlev = torch.cat([torch.full((h * w,), l) for l, (h, w) in enumerate(shapes)])
    band = qrow // (hs[qlev] // NB)
    k = torch.arange(NB).reshape(NB, 1)
    c0, c1 = k * hs.reshape(1, -1) // NB, (k + 1) * hs.reshape(1, -1) // NB
    return band, (c0 - halo).clamp_min(0), torch.minimum(c1 + halo, hs.reshape(1, -1))


def drop_outside_band(inp, shapes, M, P, NB, halo):
    """a band block that loses the samples it has not staged: a sample with a valid corner outside the staged rows contributes nothing"""
    band, lo, hi = band_rows(shapes, NB, halo)

    def drop(l, x0, y0, v):
        blo, bhi = lo[band, l].reshape(1, -1, 1, 1), hi[band, l].reshape(1, -1, 1, 1)
        vx0, vx1, vy0, vy1 = v
        in_band = (~vy0 | ((y0 >= blo) & (y0 < bhi))) & (~vy1 | ((y0 + 1 >= blo) & (y0 + 1 < bhi)))
        return (vy0 | vy1) & (vx0 | vx1) & ~in_band
    return _chain(inp, shapes, M, P, drop=drop)


def drop_partly_outside(inp, shapes, M, P):
    """a sample with any corner outside the map is dropped whole (zero padding applied to the sample, not to the corner)"""
    return _chain(inp, shapes, M, P, drop=lambda l, x0, y0, v: ~(v[0] & v[1] & v[2] & v[3]))


def last_query_twice(inp, shapes, M, P):
    """tail lanes that shadow the last query also ADD: its contribution to dvalue and dref counted twice"""
    ch = _chain(inp, shapes, M, P)
    only = dict(inp)
    only["dout"] = inp["dout"].clone()
    only["dout"][:, :-1] = 0.0
    ch2 = _chain(only, shapes, M, P)
    ch["dvalue"] = ch["dvalue"] + ch2["dvalue"]
    ch["dref"] = ch["dref"] + ch2["dref"]
    return ch


def ref_level0(inp, shapes, M, P):
    """ref_L = L read as level 0's point for every level"""
    return _chain(inp, shapes, M, P, ref_level0=True)


def scale_without_spikes(inp, shapes, M, P, dtype):
    """the integer scatter's scale taken from max |dout| without the spike rows (a max |dout| scan that loses rows); the int32 cells wrap"""
    dout = inp["dout"]
    B, Lq, _ = dout.shape
    g = dout.reshape(B, Lq, M, D).abs()
    rowmax = g.amax(3)
    gm = torch.where(rowmax >= 0.5 * rowmax.amax(1, keepdim=True), torch.zeros_like(rowmax), rowmax).amax(1)
    ch = _chain(inp, shapes, M, P)
    return scatter_lds(ch, inp, M, dtype, gmax=gm, wrap=True)


# ---- the measure ----------------------------------------------------------------------------------------------------------------
def _ratio(num, den):
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


def row_errors(got, want, mag):
    """|| got_row - want_row || / || magnitude_row || over the last dimension"""
    return _ratio((got.to(F64) - want.to(F64)).norm(dim=-1), mag.to(F64).norm(dim=-1))


def dvalue_errors(got, want, mag, count, res, unit):
    """rows [B, Lv, M]; res: resolution(...) [B, M]; unit: UNIT[dtype].  Rows no corner reaches (count = 0) are left to the exact-zero check."""
    den = mag.to(F64).norm(dim=-1) + math.sqrt(D) * count.to(F64) * res.reshape(res.shape[0], 1, -1) / (2.0 * unit)
    e = _ratio((got.to(F64) - want.to(F64)).norm(dim=-1), den)
    return torch.where(count > 0, e, torch.zeros_like(e))


def reduce_dref(dref, shared):
    """reference points shared by the batch receive the sum over the batch"""
    return dref.sum(0, keepdim=True) if shared else dref


def worst_errors(got, want, mag, inp, M, dtype, kind, shared_ref=False):
    """{tensor: worst per-row error} for the tensors `got` has (dicts as _chain returns them; dvalue needs the scatter kind 'lds' | 'mf')"""
    res = {}
    for k in ("out", "doff", "dlogit"):
        if k in got and got[k] is not None:
            res[k] = row_errors(got[k], want[k], mag[k]).max().item()
    if got.get("dvalue") is not None:
        res["dvalue"] = dvalue_errors(got["dvalue"], want["dvalue"], mag["dvalue"], want["count"], resolution(inp["dout"], M, kind),
                                      UNIT["f32" if dtype == "f32" else "bf16"]).max().item()
    if got.get("dref") is not None:
        res["dref"] = row_errors(reduce_dref(got["dref"], shared_ref and got["dref"].shape[0] != 1), reduce_dref(want["dref"], shared_ref),
                                 reduce_dref(mag["dref"], shared_ref)).max().item()
    return res


def dvalue_key(regime, kind):
    return ("spike-" if regime == "spike" else "") + kind


def bound_of(dtype, tensor, regime="ordinary", kind="lds"):
    b = MSDA_BOUND[dtype][tensor]
    return b[dvalue_key(regime, kind)] if tensor == "dvalue" else b


# ---- the float16 forward test's reference (tests/test_gpu_fp16_kernels.py::test_msda_fwd_small) ------------------------------------
def forward_with_slack(value, offw, ref, shapes, M, Pn, round_weights):
    """Multi-scale deformable attention in float64 with explicit corners (grid_sample, align_corners = False, zero padding):
    out[b, q, m] = sum over (level, point, corner) of w * value[b, pixel, m], w = softmax weight * bilinear corner weight.
    round_weights: the kernels' contract for 16-bit value types (csrc/msda.hip: the four corner weights are packed to the value type so that
    one v_dot2_f32_f16 does two multiply-adds; products and sums stay fp32) -- w -> round16(w).  Returns (out, slack).
    slack, derived: the kernel computes pixel coordinates (ref + off / size) * size - 0.5 and the softmax in fp32, so a weight carries
    dw = aw * 2 * 4 * 2^-24 * (extent + |offset| + 1) (coordinate error times the unit slope of a bilinear weight, x and y) + 16 * 2^-24 w
    (__expf, sum, divide, two products).  Unrounded weights: sum dw |v|.  Rounded weights: the rounding absorbs dw unless w lies within dw of
    a float16 rounding boundary, where the kernel may round the other way: such a corner contributes ulp16(w) |v|.  Plus the fp32
    accumulation of the 4 L P products (gemm_slack)."""
    from tests.hip_utils import EPS32, gemm_slack, round16, ulp16          # (imports the library: kept out of this module's own import)
    B, Lv, CC = value.shape
    L = len(shapes)
    Lq = offw.shape[1]
    tp = M * L * Pn
    off = offw[..., :2 * tp].reshape(B, Lq, M, L, Pn, 2)
    aw = torch.softmax(offw[..., 2 * tp:3 * tp].reshape(B, Lq, M, L * Pn), -1).reshape(B, Lq, M, L, Pn)
    val = value.reshape(B, Lv, M, 32).permute(0, 2, 1, 3)                     # [B, M, Lv, 32]
    out = torch.zeros(B, M, Lq, 32, dtype=torch.float64)
    sq = torch.zeros_like(out)
    extra = torch.zeros_like(out)
    start = 0
    for l, (h, w) in enumerate(shapes):
        rl = ref[:, :, l if ref.shape[2] == L else 0].reshape(ref.shape[0], Lq, 1, 1, 2)
        loc = rl + off[:, :, :, l] / torch.tensor([w, h], dtype=torch.float64)              # normalised (x, y)
        px, py = loc[..., 0] * w - 0.5, loc[..., 1] * h - 0.5                            # [B, Lq, M, P]
        x0, y0 = px.floor(), py.floor()
        lx, ly = px - x0, py - y0
        dcoord = 4 * EPS32 * (max(h, w) + off[:, :, :, l].abs().amax(-1) + 1)
        for dy_, dx_, cw in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
            xi, yi = x0 + dx_, y0 + dy_
            ok = ((xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)).double()
            wgt = aw[:, :, :, l] * cw * ok                                                # [B, Lq, M, P]
            dw = (aw[:, :, :, l] * 2 * dcoord + 16 * EPS32 * wgt) * ok
            idx = (start + yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
            idx = idx.permute(0, 2, 1, 3).reshape(B, M, Lq * Pn, 1).expand(B, M, Lq * Pn, 32)
            v = torch.gather(val, 2, idx).reshape(B, M, Lq, Pn, 32)
            wq = wgt.permute(0, 2, 1, 3).unsqueeze(-1)                                    # [B, M, Lq, P, 1]
            dwq = dw.permute(0, 2, 1, 3).unsqueeze(-1)
            if round_weights:
                wr = round16(wq)
                up, dn = ulp16(wr), ulp16(wr * (1 - 2.0 ** -12))
                dist = torch.minimum((wq - (wr + up / 2)).abs(), (wq - (wr - dn / 2)).abs())
                extra += (((dist <= dwq) & (dwq > 0)).double() * ulp16(wq) * v.abs()).sum(3)
                wq = wr
            else:
                extra += (dwq * v.abs()).sum(3)
            out += (wq * v).sum(3)
            sq += (wq * wq * v * v).sum(3)
        start += h * w
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, Lq, CC)
    return back(out), back(gemm_slack(4 * L * Pn, sq) + extra)
