"""Inputs, float64 references and rounding-count bounds of the sweeps "loss", "step" and "areas" of tests/fuzz_cases.py: what
tests/test_gpu_loss_fuzz.py and tests/test_gpu_step_fuzz.py hold the kernels to, and what tests/test_fuzz_cases_cpu.py checks the input
conditions on.  Everything here runs on the CPU from a case tuple alone; nothing reads a kernel's output.

Bounds count fp32 roundings, U = 2^-24 relative each, from the float64 run's own terms (first order).
  exponential   e_c = __expf(a_c), a_c = z_c - max: the subtraction, the fp32 constant log2(e) and the rounded product a * log2(e) move the
                argument by |a| U each, the hardware exponential is good to one ulp = 2 U           -> rel_e(a) = (3 |a| + 2) U
  denominator   C - 1 additions of positive terms                                                   -> rel_den = (C - 1) U + sum_c p_c rel_e(a_c)
  pixel CE      logf(den) + (mx - picked): logf to one ulp, the subtraction of the two logits and the addition, at magnitude
                M = |mx - picked| + |log den| (csrc/loss_pixel.hpp subtracts the two logits first, so a common offset of the logits
                cancels exactly; the magnitude max(|mx|, |picked|) does not enter)            -> ce_err = rel_den + 2 U |log den| + 2 U M
  stored p      __expf(picked - mx) / den                                                           -> p (rel_e(a_y) + rel_den + U) + TINY
  softmax_c     __expf(a_c) * (1 / den)                                                             -> p_c (rel_e(a_c) + rel_den + 2 U) + TINY
                TINY = 2^-126: below the smallest normal fp32 number a probability is stored as 0 (or a denormal)
  a mean        a thread adds `depth` terms (fuzz_cases.loss_depth of the restated grid), wave_sum adds six times, the block three, then
                float64; one product w * ce and one rounding of the result                           -> (depth + 10) U of sum |terms|
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import fuzz_cases as fc

U = 2.0 ** -24
UPSTREAM = 0.37
TINY = 2.0 ** -126
ENVELOPE_C, ENVELOPE_GAP = 9, 16.0          # today's fixed tests: C <= 9, |z - max| <= 16


# ---------------------------------------------------------------------------------------------------------------------------------
# loss: inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _draw_labels(g, N, C, H, W, ign, pattern):
    npix = N * H * W
    labels = torch.randint(0, C, (N, H, W), generator=g)
    pick = int(torch.randint(0, C, (1,), generator=g))
    drop = torch.rand(N, H, W, generator=g) < 0.1
    inside = 0 <= ign < C
    if inside and pick == ign:
        pick = (pick + 1) % C
    if pattern == "oneclass":
        labels.fill_(pick)
    if pattern in ("tenth", "oneclass"):
        if npix > 1 and not drop.any():
            drop.view(-1)[-1] = True
        if npix > 1:
            drop.view(-1)[0] = False
        labels[drop] = ign
        if inside and labels.view(-1)[0] == ign:
            labels.view(-1)[0] = pick
    elif pattern == "all":
        labels.fill_(ign)
    elif pattern == "allbut1":
        labels.fill_(ign)
        labels.view(-1)[npix // 2] = pick
    return labels


def _draw_logits(g, pattern, shape, own, scale):
    """own: the class whose logit the patterns "confident" and "wide" steer, [N, H, W] in [0, C)"""
    N, C, H, W = shape
    z = scale * torch.randn(N, C, H, W, generator=g)
    if pattern == "confident":
        z = z / scale + 4 * F.one_hot(own, C).permute(0, 3, 1, 2).float()
    elif pattern == "shift+":
        z = z + 1000.0
    elif pattern == "shift-":
        z = z - 1000.0
    elif pattern == "wide" and C > 1:
        z = z / scale
        oh = F.one_hot(own, C).permute(0, 3, 1, 2).bool()
        top = z.masked_fill(oh, -1e30).max(1).values
        r = torch.rand(N, H, W, generator=g)
        gap = torch.where(r < 1 / 3, torch.full_like(r, 60.0), torch.where(r < 2 / 3, torch.full_like(r, 120.0), torch.zeros_like(r)))
        z = torch.where(oh & (gap > 0).unsqueeze(1), (top - gap).unsqueeze(1).expand_as(z), z)
    elif pattern == "constant":
        z = torch.full_like(z, 0.25)
    elif pattern == "grid":
        z = torch.round(z) / 2
    return z.contiguous()


def loss_inputs(case):
    """-> dict(la, lb fp32 NCHW, labels int64, cw fp32 [C] or None), from the case's seed alone"""
    _, fam, form, N, C, H, W, ign, lpat, zpat, cwk, hw, up, thresh, min_kept, dice, _, seed = case
    g = torch.Generator().manual_seed(seed)
    labels = _draw_labels(g, N, C, H, W, ign, lpat)
    own = torch.where(labels == ign, torch.zeros_like(labels), labels)
    la = _draw_logits(g, zpat, (N, C, H, W), own, 2.0)
    lb = _draw_logits(g, zpat, (N, C, H, W), own, 3.0)
    cw = None
    if cwk != "none":
        cw = 0.5 + 1.5 * torch.rand(C, generator=g)
        present = torch.unique(labels[labels != ign])
        if cwk == "onezero" and present.numel():
            cw[int(present[0]) if present.numel() >= 2 else (int(present[0]) + 1) % C] = 0.0
        if cwk == "zeropresent":
            cw[present] = 0.0
    return dict(la=la, lb=lb, labels=labels, cw=cw)


# ---------------------------------------------------------------------------------------------------------------------------------
# loss: the float64 terms of every pixel and what they bound
# ---------------------------------------------------------------------------------------------------------------------------------
def pixel_terms(z, labels, ign):
    """float64, per pixel ([N, H, W]) or per logit ([N, C, H, W]): valid, a, p, ce, p_own and the rounding bounds of the module docstring"""
    z = z.double()
    N, C, H, W = z.shape
    valid = labels != ign
    y = torch.where(valid, labels, torch.zeros_like(labels)).unsqueeze(1)
    mx = z.max(1, keepdim=True).values
    a = z - mx
    e = a.exp()
    den = e.sum(1, keepdim=True)
    p = e / den
    picked = z.gather(1, y)
    rel_e = (3 * a.abs() + 2) * U
    rel_den = (C - 1) * U + (p * rel_e).sum(1, keepdim=True)
    ce = den.log() - a.gather(1, y)
    M = (mx - picked).abs() + den.log().abs()
    ce_err = rel_den + 2 * U * den.log().abs() + 2 * U * M
    p_own = p.gather(1, y)
    p_own_err = p_own * (rel_e.gather(1, y) + rel_den + U) + TINY
    p_err = p * (rel_e + rel_den + 2 * U) + TINY
    gap = (a.abs().amax(1) * valid).max().item() if valid.any() else 0.0
    sq = lambda t: t.squeeze(1)
    return dict(valid=valid, y=sq(y), a=a, p=p, ce=sq(ce), ce_err=sq(ce_err), p_own=sq(p_own), p_own_err=sq(p_own_err), p_err=p_err, rel_e=rel_e,
                rel_den=sq(rel_den), gap=gap, envelope=C <= ENVELOPE_C and gap <= ENVELOPE_GAP)


def class_weights_of(labels, cw, ign, C):
    """float64 w[y] per pixel, 0 at the ignored ones"""
    valid = labels != ign
    y = torch.where(valid, labels, torch.zeros_like(labels))
    w = torch.ones(C, dtype=torch.float64) if cw is None else cw.double()
    return w[y] * valid.double()


def ce_reference(z, labels, cw, ign):
    """float64 F.cross_entropy(weight=, ignore_index=) with autograd -> (loss, dloss/dz, sum of weights); total weight zero: loss 0, gradient 0
    (the kernels' contract, where torch gives nan)"""
    C = z.shape[1]
    wy = class_weights_of(labels, cw, ign, C)
    sum_w = wy.sum().item()
    if sum_w <= 0.0:
        return 0.0, torch.zeros_like(z, dtype=torch.float64), sum_w
    x = z.double().clone().requires_grad_(True)
    loss = F.cross_entropy(x, labels, weight=None if cw is None else cw.double(), ignore_index=ign)
    loss.backward()
    return loss.item(), x.grad, sum_w


def ohem_reference(case, z, labels):
    """tests/test_gpu_ohem.py's ohem_ref (float64) of one head with its gradient; the case's ignore index is mapped onto that module's 255
    (no case has 255 classes).  tied: the tie and constant cases, whose margin excludes the pixels EQUAL to the threshold"""
    from tests.test_gpu_ohem import ohem_ref, IGN
    lab = torch.where(labels == case[7], torch.full_like(labels, IGN), labels)
    x = z.double().clone().requires_grad_(True)
    r = ohem_ref(x, lab, case[13], case[14])
    r["loss"].backward()
    r["grad"], r["loss"], r["tied"] = x.grad, r["loss"].item(), case[9] in ("constant", "grid")
    return r


def mean_bound(t, wy, depth):
    """|fp32 mean - float64 mean| of sum w ce / sum w over the non-ignored pixels"""
    sw = wy.sum().item()
    if sw <= 0.0:
        return 0.0
    num = (wy * t["ce_err"]).sum().item() + (depth + 10) * U * (wy * t["ce"].abs()).sum().item()
    loss = (wy * t["ce"]).sum().item() / sw
    return num / sw + abs(loss) * ((depth + 9) * U + 2 * U)


def ce_grad_bound(t, wy, depth, scale):
    """|dlogits - float64| per logit for dlogits = scale * w[y] / sum w * (softmax - onehot); scale = head weight * upstream (* ce_weight)"""
    sw = wy.sum().item()
    G = (abs(scale) * wy / (sw if sw > 0 else 1.0)).unsqueeze(1)
    oh = F.one_hot(t["y"], t["p"].shape[1]).permute(0, 3, 1, 2).double()
    return G * (t["p_err"] + (t["p"] - oh).abs() * (2 * U + (depth + 14) * U))


def ohem_loss_bound(t, kept, npix, depth):
    den = kept.sum().item() + 1e-5 * npix
    k = kept.double()
    num = (k * t["ce_err"]).sum().item() + (depth + 10) * U * (k * t["ce"].abs()).sum().item()
    return num / den + 2 * U * (k * t["ce"]).sum().item() / den


def ohem_grad_bound(t, kept, npix, scale):
    den = kept.sum().item() + 1e-5 * npix
    G = (abs(scale) * kept.double() / den).unsqueeze(1)
    oh = F.one_hot(t["y"], t["p"].shape[1]).permute(0, 3, 1, 2).double()
    return G * (t["p_err"] + (t["p"] - oh).abs() * 6 * U)


def dice_bounds(t, terms, wy, dice, depth_f, scale):
    """-> (bound on L, bound on Dice, bound on dlogits) of one head of the Dice + CE loss, scale = head weight * upstream.  I_c and P_c are
    fp32 sums of softmax values (depth + 10 additions, as a mean), U_c adds the exact integer T_c; the coefficients a_c, b_c come out of
    float64 arithmetic on those sums and are rounded once: rel_coef = 2 (depth + 10) U + 2 U; sum_c p_c g_c is C products and additions."""
    cew, dw, smooth = dice
    C = t["p"].shape[1]
    v = t["valid"].double().unsqueeze(1)
    oh = F.one_hot(t["y"], C).permute(0, 3, 1, 2).double() * v
    Uc, I = terms["U"], terms["I"]
    live = Uc > 0
    Us = torch.where(live, Uc, torch.ones_like(Uc))
    rel_sum = (depth_f + 10) * U
    I_err = (t["p_err"] * oh).sum(dim=(0, 2, 3)) + rel_sum * I
    P_err = (t["p_err"] * v).sum(dim=(0, 2, 3)) + rel_sum * terms["P"]
    dice_err = (torch.where(live, 2 * I_err / Us + (2 * I + smooth) * P_err / (Us * Us), torch.zeros_like(Us)).sum() / C).item() + 2 * U
    ce_b = mean_bound(t, wy, depth_f)
    L_err = cew * (ce_b + U * abs(terms["CE"].item())) + dw * (dice_err + U * abs(terms["Dice"].item())) + U * abs(terms["L"].item())
    a_c = torch.where(live, -2 * dw / (C * Us), torch.zeros_like(Us)).view(1, C, 1, 1)
    b_c = torch.where(live, dw * (2 * I + smooth) / (C * Us * Us), torch.zeros_like(Us)).view(1, C, 1, 1)
    gk = (b_c + a_c * oh).abs()
    pg = (t["p"] * gk).sum(1, keepdim=True)
    relp = (t["p_err"] / t["p"].clamp_min(1e-300)).amax(1, keepdim=True)
    rel_coef = 2 * rel_sum + 2 * U
    g_dice = abs(scale) * v * t["p"] * (gk + pg) * (2 * relp + (C + 4) * U + 3 * rel_coef)
    g_ce = ce_grad_bound(t, wy, depth_f + 2, scale * cew)
    return L_err, dice_err, g_ce + g_dice + U * (g_ce + g_dice)


# ---------------------------------------------------------------------------------------------------------------------------------
# step: inputs and float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
SGD = dict(base_lr=0.01, end_lr=1e-4, power=0.9, decay_steps=100, momentum=0.9, weight_decay=1e-4)
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
ADAM_SCHED = dict(kind=1, base_lr=1e-2, end_lr=0.0, power=0.9, warmup_lr_init=1e-3, total_steps=160000, warmup_steps=1500)
STEP_INDEX, SCALE, MULT = 37, 0.37, 0.1
CLIP = 1.0


def f32(x):
    return float(np.float32(x))


def step_inputs(case):
    """p, g, s0 (velocity / first moment), s1 (second moment), fp32 numpy.  Signs are shared per element and magnitudes kept away from zero, so
    that every element moves by far more than its own spacing (the range-membership condition, checked by step_condition)."""
    _, entry, n, layout, mirror, nt, clip, nulls, _, seed = case
    r = np.random.default_rng(seed)
    s = np.where(r.random(n) < 0.5, -1.0, 1.0)
    g = (s * (0.5 + np.abs(r.standard_normal(n)))).astype(np.float32)
    if entry == "clip":
        if clip == "zerograd":
            g[:] = 0.0
        if clip == "below":
            g *= np.float32(0.5 / max(np.sqrt((g.astype(np.float64) ** 2).sum()), 1e-30))          # norm 0.5 < CLIP
        return dict(g=g)
    p = (s * (0.25 + np.abs(r.standard_normal(n)))).astype(np.float32)
    s0 = (0.1 * s * r.random(n)).astype(np.float32)
    s1 = ((0.1 * r.standard_normal(n)) ** 2).astype(np.float32)
    return dict(p=p, g=g, s0=s0, s1=s1)


def step_lr_host(entry, step):
    """the schedule in float64 (the kernels' fp32 value is within 1e-6 relative: tests/test_gpu_adamw.py), for the input condition alone"""
    if entry in ("sgd", "sgd_sched"):
        t = min(step, SGD["decay_steps"])
        return (SGD["base_lr"] - SGD["end_lr"]) * (1 - t / SGD["decay_steps"]) ** SGD["power"] + SGD["end_lr"]
    W, T = ADAM_SCHED["warmup_steps"], ADAM_SCHED["total_steps"]
    b, i = ADAM_SCHED["base_lr"], ADAM_SCHED["warmup_lr_init"]
    return i + (b - i) * step / W if step < W else max(i + (b - i) * (1 - (step - W) / (T - W)) ** ADAM_SCHED["power"], ADAM_SCHED["end_lr"])


def step_mask(case):
    m = np.zeros(case[2], dtype=bool)
    m[fc.step_selected(case[3], case[2])] = True
    return m


def sgd_reference(x, scale, lr, mult, mask):
    """g' = g * scale + wd * p, v = momentum * v + g', p -= lr_e * v in float64 from the fp32 inputs; lr_e = the fp32 product lr * mult inside
    the ranges.  Each of the kernel's three fused steps and the product g * scale is one rounding of its own result:
    |v - v_ref| <= U (|g scale| + |g'| + |v_ref|), |p - p_ref| <= lr_e * that + U |p_ref|."""
    p, g, v = (x[k].astype(np.float64) for k in ("p", "g", "s0"))
    wd, mom, scale = (np.float64(np.float32(t)) for t in (SGD["weight_decay"], SGD["momentum"], scale))
    lre = np.where(mask, np.float64(np.float32(lr) * np.float32(mult)), np.float64(np.float32(lr)))
    gs = g * scale
    gg = gs + wd * p
    v_ref = mom * v + gg
    p_ref = p - lre * v_ref
    v_b = U * (np.abs(gs) + np.abs(gg) + np.abs(v_ref))
    return p_ref, v_ref, lre * v_b + U * np.abs(p_ref), v_b, lre * v_ref


def adam_reference(x, scale, step, lr, mult, mask, decoupled=1):
    """tests/test_gpu_adamw.py's adam_reference at any n and any range mask: the formulas of include/emrt_hip.h in float64 from the fp32 inputs
    -> p_ref, m_ref, v_ref, u_ref, m_mag, v_mag; the bounds are that test's: 3 U m_mag, 3 U v_mag, U (3 |p_ref| + 8 |u_ref|)"""
    p, g, m, v = (x[k].astype(np.float64) for k in ("p", "g", "s0", "s1"))
    b1, b2, eps, wd, mult, scale = (np.float64(np.float32(t)) for t in (ADAM["beta1"], ADAM["beta2"], ADAM["eps"], ADAM["weight_decay"], mult, scale))
    lre = np.full(p.shape, np.float64(lr))
    lre[mask] *= mult
    t = step + 1
    g = g * scale
    if decoupled:
        p1 = p * (1.0 - lre * wd)
    else:
        g = g + wd * p
        p1 = p
    gm, gv = (1.0 - b1) * g, (1.0 - b2) * g * g
    m_ref, v_ref = b1 * m + gm, b2 * v + gv
    bc1, bc2s = 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)
    u_ref = lre * bc2s / bc1 * m_ref / (np.sqrt(v_ref) + eps * bc2s)
    return p1 - u_ref, m_ref, v_ref, u_ref, np.abs(b1 * m) + np.abs(gm), np.abs(b2 * v) + np.abs(gv)


def step_condition(case):
    """the input condition of the range-membership check, from float64 alone: with range_mult = 0, the smallest |change of p| / (4 ulp of |p|)
    over the elements OUTSIDE the ranges (must exceed 1), and the number of such elements"""
    _, entry, n, layout, mirror, nt, clip, nulls, _, seed = case
    x = step_inputs(case)
    mask = step_mask(case)
    step = 0 if "step" in nulls else STEP_INDEX
    scale = 1.0 if "clip_state" in nulls else SCALE
    lr = step_lr_host(entry, step)
    if entry == "adamw":
        p_ref = adam_reference(x, scale, step, lr, 0.0, mask)[0]
    else:
        p_ref = sgd_reference(x, scale, lr, 0.0, mask)[0]
    p = x["p"].astype(np.float64)
    ulp = np.spacing(np.abs(x["p"])).astype(np.float64)
    out = ~mask
    if not out.any():
        return float("inf"), 0
    return float((np.abs(p_ref - p)[out] / (4 * ulp[out])).min()), int(out.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# areas
# ---------------------------------------------------------------------------------------------------------------------------------
AREAS_NP = {0: np.int32, 1: np.int64, 2: np.uint8}


def areas_inputs(case):
    """pred int32 in [-2, ncls + 2), labels of the case's type in [-2, ncls + 3) (uint8: [0, min(ncls + 3, 256))), the ignore index among them"""
    _, ncls, ltype, offset, n, ignore, _, seed = case
    r = np.random.default_rng(seed)
    pred = r.integers(-2, ncls + 2, n).astype(np.int32)
    lo, hi = (0, min(ncls + 3, 256)) if ltype == 2 else (-2, ncls + 3)
    label = r.integers(lo, hi, n)
    agree = r.random(n) < 0.5
    ok = (pred >= lo) & (pred < hi)
    label = np.where(agree & ok, pred, label)
    if ltype != 2 or 0 <= ignore <= 255:
        label = np.where(r.random(n) < 0.1, ignore, label)
    return pred, label.astype(AREAS_NP[ltype])


def areas_reference(pred, label, ncls, ignore):
    """intersect / prediction / label pixel counts [3, ncls], int64: csrc/optim.hip's seg_areas_kernel restated with numpy"""
    l = label.astype(np.int64)
    p = pred.astype(np.int64)
    keep = l != ignore
    pv, lv = keep & (p >= 0) & (p < ncls), keep & (l >= 0) & (l < ncls)
    out = np.zeros((3, ncls), dtype=np.int64)
    out[1] = np.bincount(p[pv], minlength=ncls)
    out[2] = np.bincount(l[lv], minlength=ncls)
    out[0] = np.bincount(p[pv & (p == l)], minlength=ncls)
    return out
