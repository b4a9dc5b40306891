"""float64 restatement of the Dice + cross-entropy contract of include/emrt_hip_loss.h, in plain torch: the loss through autograd, and the
closed-form gradient the backward kernel evaluates, written out separately.  tests/test_dice_cpu.py holds the two against each other;
tests/test_gpu_dice.py holds the kernels to the autograd form."""
import torch
import torch.nn.functional as F

IGN = 255


def dice_ce_terms(logits, labels, ce_weight=1.0, dice_weight=1.0, smooth=1.0, class_weight=None, ignore_index=IGN):
    """-> dict(L, CE, Dice, I, P, T, U, sum_w, num_valid) as float64 tensors; differentiable in `logits` (any float dtype, NCHW)."""
    z = logits.double()
    N, C, H, W = z.shape
    valid = labels != ignore_index
    v = valid.double().unsqueeze(1)
    p = torch.softmax(z, dim=1)
    y = torch.where(valid, labels, torch.zeros_like(labels))
    onehot = F.one_hot(y, C).permute(0, 3, 1, 2).double() * v
    I = (p * onehot).sum(dim=(0, 2, 3))
    P = (p * v).sum(dim=(0, 2, 3))
    T = onehot.sum(dim=(0, 2, 3))
    U = P + T + smooth
    live = U > 0                      # U = 0 (only with smooth = 0): the class's dice is 1 and carries no gradient
    dice_c = torch.where(live, (2 * I + smooth) / torch.where(live, U, torch.ones_like(U)), torch.ones_like(U))
    dice = 1 - dice_c.sum() / C
    w = torch.ones(C, dtype=torch.float64) if class_weight is None else class_weight.double()
    wy = w[y] * valid.double()
    ce_i = -(torch.log_softmax(z, dim=1) * onehot).sum(dim=1)
    sum_w = wy.sum()
    ce = (wy * ce_i).sum() / (sum_w if sum_w > 0 else 1.0)      # every pixel ignored: 0, not 0 / 0
    return dict(L=ce_weight * ce + dice_weight * dice, CE=ce, Dice=dice, I=I, P=P, T=T, U=U, sum_w=sum_w, num_valid=valid.sum())


def dice_ce_autograd(logits, labels, **kw):
    """-> (terms with detached values, dL/dlogits as float64)"""
    z = logits.double().clone().requires_grad_(True)
    t = dice_ce_terms(z, labels, **kw)
    t["L"].backward()
    return {k: v.detach() for k, v in t.items()}, z.grad


def dice_ce_closed_form_grad(logits, labels, ce_weight=1.0, dice_weight=1.0, smooth=1.0, class_weight=None, ignore_index=IGN, dtype=torch.float64):
    """The gradient as the header states it: a_c = -2 dw / (C U_c), b_c = dw (2 I_c + s) / (C U_c^2), g_ic = a_c [y_i = c] + b_c,
    dz_ik = v_i (cw w[y_i] / sum w (p_ik - [y_i = k]) + p_ik (g_ik - sum_c p_ic g_ic)).  The batch sums are taken in float64; the per-pixel
    arithmetic runs in `dtype` (float32: how far an fp32 evaluation is from float64)."""
    with torch.no_grad():
        t = dice_ce_terms(logits, labels, ce_weight, dice_weight, smooth, class_weight, ignore_index)
        z = logits.to(dtype)
        N, C, H, W = z.shape
        live = t["U"] > 0
        U = torch.where(live, t["U"], torch.ones_like(t["U"]))
        a = torch.where(live, -2 * dice_weight / (C * U), torch.zeros_like(U)).to(dtype)
        b = torch.where(live, dice_weight * (2 * t["I"] + smooth) / (C * U * U), torch.zeros_like(U)).to(dtype)
        valid = labels != ignore_index
        v = valid.to(dtype).unsqueeze(1)
        y = torch.where(valid, labels, torch.zeros_like(labels))
        onehot = F.one_hot(y, C).permute(0, 3, 1, 2).to(dtype)
        p = torch.softmax(z, dim=1)
        g = a.view(1, C, 1, 1) * onehot + b.view(1, C, 1, 1)
        w = torch.ones(C, dtype=dtype) if class_weight is None else class_weight.to(dtype)
        sum_w = t["sum_w"].item() if t["sum_w"].item() > 0 else 1.0
        ce_scale = (ce_weight * w[y] / sum_w).to(dtype).unsqueeze(1)
        return v * (ce_scale * (p - onehot) + p * (g - (p * g).sum(dim=1, keepdim=True)))


def make_case(shape, seed, ignored=0.1, absent=None, all_present=False):
    """(logits fp32 NCHW, labels int64) from a seeded generator; `absent`: a class that no label carries; all_present: class c is planted at
    flat pixel c before the ignore mask is drawn and those pixels stay labelled.  With ignored > 0 at least one pixel is ignored (the last one, when
    the draw ignored none: the smallest cases have fifteen pixels)."""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    logits = 2 * torch.randn(N, C, H, W, generator=g)
    labels = torch.randint(0, C, (N, H, W), generator=g)
    if absent is not None:
        labels[labels == absent] = (absent + 1) % C
    drop = torch.rand(N, H, W, generator=g) < ignored
    if all_present:
        flat, fdrop = labels.view(-1), drop.view(-1)
        assert flat.numel() >= C
        flat[:C] = torch.arange(C)
        fdrop[:C] = False
    if ignored > 0 and not drop.any():
        drop.view(-1)[-1] = True
    labels[drop] = IGN
    return logits, labels
