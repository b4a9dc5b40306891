"""-m gpu: the loss kernels -- emrt_softmax_ce_*, emrt_wce_*, emrt_ohem_ce_* (csrc/loss.hip) and emrt_lx_dice_ce_* (csrc/loss_ext/loss_ext.hip),
all on the pixel core of csrc/loss_pixel.hpp -- swept by shape, class count, labels, logit range, class and head weights: the op "loss" of
tests/fuzz_cases.py, every case forward and backward through the C ABI, single form and (where the case says so) pair form.

References (float64, CPU): ce / wce: F.cross_entropy(weight=, ignore_index=) under autograd; ohem: tests/test_gpu_ohem.py's ohem_ref; dice:
tests/dice_reference.py.  Inputs and bounds: tests/loss_step_reference.py.

Exact checks of every case: each output (result, prob, coef, dlogits, total) is a slice of a sentinel-filled allocation, nothing outside the
slice may change and every entry of dlogits must be written; ignored pixels hold exact zeros in the gradient and the NaN pattern in prob; the
pair form gives each head the single form's bits; a second launch gives equal bits; all ignored or total weight zero: loss 0, gradient 0.
ce: emrt_wce_* with a NULL weight and with an all-ones weight give emrt_softmax_ce_*'s bits.  dice: dice_weight 0, ce_weight 1 gives the CE
bits of emrt_wce_* (the gradient within 2 ulp, as tests/test_gpu_dice.py holds it).  ohem: the kept mask, the kept and the non-ignored count
are exact -- under the input condition tests/test_fuzz_cases_cpu.py checks in float64 (no other pixel within 1e-5 of the threshold; the tie
and constant cases: none but the exact ties) -- and the threshold is the one the three branches give on the device's OWN stored p.

Bounds.  A case inside the envelope of the fixed tests (C <= 9, |z - max| <= 16 over its non-ignored pixels) keeps their numbers: atol 1e-5
on the loss scalars, tests/test_gpu_ohem.py's grad_atol (weighted: its max(w) K / sum w form) or tests/test_gpu_dice.py's grad_bound on the
gradients, times |head weight * upstream|, and 25 * 2^-24 on the stored p at C <= 7.  Outside it the bound is DERIVED from the float64 run's
own terms by counting fp32 roundings (tests/loss_step_reference.py's module docstring has the count per quantity: the exponential's argument
and its one-ulp hardware evaluation, C - 1 additions, the divide or logf, the CE's subtraction and addition at the magnitude of
|mx - picked| + |log den| -- pixel_ce subtracts the two logits first, so max(|mx|, |picked|) does not enter and logits shifted by 1000 are
held to the bound of unshifted ones --, the underflow floor 2^-126 of a stored probability, and for a mean the per-thread depth of the
restated grid plus the wave's and the block's additions).  No bound comes from a kernel's output.  -s
prints, per case, the worst error over the asserted bound and over the derived bound (DESIGN.md 2.4 has a run on an MI355X)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                                 # noqa: E402
from emrt_amd.runtime import ctx, F32                                     # noqa: E402
from tests import dice_reference as DR                                    # noqa: E402
from tests import fuzz_cases as fc                                        # noqa: E402
from tests import loss_step_reference as R                                # noqa: E402
from tests.hip_utils import init, ulp32                                   # noqa: E402
from tests.test_gpu_ohem import IGN, P_BOUND, ce_test_count, expected_device_threshold, grad_atol      # noqa: E402
from tests.test_gpu_dice import grad_bound as dice_grad_bound            # noqa: E402

PAD = 64
SENTINEL = -12345.0
SWEEP = fc.CASES["loss"]
LINES = []


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if LINES:
        print("\n[loss sweep] worst error / bound per case: asserted (loss, gradient, stored p), then against the derived bound")
        for line in LINES:
            print(line)


class Guarded:
    """`size` floats inside a sentinel-filled allocation"""

    def __init__(self, size):
        self.full = torch.full((size + 2 * PAD,), SENTINEL, device="cuda")
        self.view = self.full[PAD:PAD + size]
        self.size = size

    def check(self, name, written=False):
        assert bool((self.full[:PAD] == SENTINEL).all()) and bool((self.full[PAD + self.size:] == SENTINEL).all()), "%s: written outside its buffer" % name
        if written:
            assert not bool((self.view == SENTINEL).any()), "%s: %d entries never written" % (name, int((self.view == SENTINEL).sum()))
        return self.view.cpu()


def run_family(fam, dev, case, cw, pair, dice=None):
    """one forward + backward of both heads through the C ABI -> dict(res=[a, b], grad=[a, b], prob=[a, b] or None, coef, total or None).
    fam: softmax_ce | wce | ohem | dice; cw: device class weights or None (NULL); the single form is two calls, one per head"""
    _, _, _, N, C, H, W, ign, _, _, _, hw, up, thresh, min_kept, _, _, _ = case
    L, X, st = _lib.lib(), (_lib.loss_lib() if fam == "dice" else None), ctx().stream
    npix, heads = N * H * W, 2
    z, lab = [dev["la"], dev["lb"]], dev["labels"]
    upt = torch.tensor([R.UPSTREAM], device="cuda") if up else None
    nres = 2 if fam in ("softmax_ce", "wce") else 8
    res, grad, total = [Guarded(nres) for _ in range(heads)], [Guarded(N * C * H * W) for _ in range(heads)], Guarded(1)
    prob = [Guarded(npix) for _ in range(heads)] if fam == "ohem" else None
    coef = [Guarded(2 * C) for _ in range(heads)] if fam == "dice" else None
    if fam == "ohem":
        nbytes = L.query("emrt_ohem_workspace_bytes", npix, 2)
    elif fam == "dice":
        nbytes = X.query("emrt_lx_dice_ce_workspace_bytes", C, 2)
    else:
        nbytes = L.query("emrt_ce_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    shape = (N, C, H, W, ign)
    cwa = () if fam in ("softmax_ce", "ohem") else (P(cw),)
    v = lambda g: P(g.view)
    if fam in ("softmax_ce", "wce"):
        if pair:
            L.call("emrt_%s_pair_fwd" % fam, P(z[0]), P(z[1]), P(lab), *cwa, *shape, hw[0], hw[1], v(res[0]), v(res[1]), v(total), P(ws), st)
            L.call("emrt_%s_pair_bwd" % fam, P(z[0]), P(z[1]), P(lab), *cwa, v(res[0]), P(upt), P(upt), hw[0], hw[1], *shape, v(grad[0]), v(grad[1]), st)
        else:
            for h in range(2):
                L.call("emrt_%s_fwd" % fam, P(z[h]), P(lab), *cwa, *shape, v(res[h]), P(ws), st)
                L.call("emrt_%s_bwd" % fam, P(z[h]), P(lab), *cwa, v(res[h]), P(upt), hw[h], *shape, v(grad[h]), st)
    elif fam == "ohem":
        if pair:
            L.call("emrt_ohem_ce_pair_fwd", P(z[0]), P(z[1]), P(lab), *shape, thresh, min_kept, hw[0], hw[1], v(prob[0]), v(prob[1]), v(res[0]), v(res[1]), v(total),
                   P(ws), st)
            L.call("emrt_ohem_ce_pair_bwd", P(z[0]), P(z[1]), P(lab), v(prob[0]), v(prob[1]), v(res[0]), v(res[1]), P(upt), P(upt), hw[0], hw[1], *shape,
                   v(grad[0]), v(grad[1]), st)
        else:
            for h in range(2):
                L.call("emrt_ohem_ce_fwd", P(z[h]), P(lab), *shape, thresh, min_kept, v(prob[h]), v(res[h]), P(ws), st)
                L.call("emrt_ohem_ce_bwd", P(z[h]), P(lab), v(prob[h]), v(res[h]), P(upt), hw[h], *shape, v(grad[h]), st)
    else:
        cew, dw, smooth = dice
        if pair:
            X.call("emrt_lx_dice_ce_pair_fwd", P(z[0]), P(z[1]), P(lab), *cwa, *shape, hw[0], hw[1], cew, dw, smooth, v(res[0]), v(res[1]), v(coef[0]), v(coef[1]),
                   v(total), P(ws), st)
            X.call("emrt_lx_dice_ce_pair_bwd", P(z[0]), P(z[1]), P(lab), *cwa, v(res[0]), v(res[1]), v(coef[0]), v(coef[1]), P(upt), P(upt), hw[0], hw[1], cew, *shape,
                   v(grad[0]), v(grad[1]), st)
        else:
            for h in range(2):
                X.call("emrt_lx_dice_ce_fwd", P(z[h]), P(lab), *cwa, *shape, cew, dw, smooth, v(res[h]), v(coef[h]), P(ws), st)
                X.call("emrt_lx_dice_ce_bwd", P(z[h]), P(lab), *cwa, v(res[h]), v(coef[h]), P(upt), hw[h], cew, *shape, v(grad[h]), st)
    torch.cuda.synchronize()
    out = dict(res=[], grad=[], prob=None, coef=None, total=None)
    for h in range(2):
        r = res[h].check("result %d" % h)
        used = {"softmax_ce": 2, "wce": 2, "ohem": 5, "dice": 8}[fam]
        assert not bool((r[:used] == SENTINEL).any()) and bool((r[used:] == SENTINEL).all()), (fam, h, r)
        out["res"].append(r)
        out["grad"].append(grad[h].check("dlogits %d" % h, written=True).view(N, C, H, W))
    if prob:
        out["prob"] = [prob[h].check("prob %d" % h).view(N, H, W) for h in range(2)]
        assert all(not bool((p == SENTINEL).any()) for p in out["prob"])
    if coef:
        out["coef"] = [coef[h].check("coef %d" % h, written=True) for h in range(2)]
    t = total.check("total")
    assert (t.item() != SENTINEL) == pair
    out["total"] = t if pair else None
    for a, b in ((dev["la"], dev["la0"]), (dev["lb"], dev["lb0"])):
        assert torch.equal(a, b), "the logits were written"
    return out


def same_bits(a, b, what):
    for k in ("res", "grad", "prob", "coef"):
        if a[k] is not None:
            for h in range(2):
                x, y = a[k][h], b[k][h]
                eq = (x.view(torch.int32) == y.view(torch.int32)) | (torch.isnan(x) & torch.isnan(y))
                assert bool(eq.all()), "%s: %s of head %d differs at %d places" % (what, k, h, int((~eq).sum()))


def dice_env_bound(terms, kw, C):
    """tests/test_gpu_dice.py's grad_bound; with a total class weight of zero its CE term (a division by sum w) is absent, as the CE gradient is"""
    if terms["sum_w"].item() > 0:
        return dice_grad_bound(terms, kw, C)
    return 1e-7 * ce_test_count() * 3 * kw["dice_weight"] / (C * terms["U"].min().item())


def ratio(err, bound):
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_loss_sweep(case):
    cid, family, form, N, C, H, W, ign, lpat, zpat, cwk, hw, up, thresh, min_kept, dice, why, _ = case
    init(F32)
    x = R.loss_inputs(case)
    labels, npix = x["labels"], N * H * W
    valid = labels != ign
    nv = int(valid.sum())
    ignored = (~valid).unsqueeze(1).expand(N, C, H, W)
    dev = dict(la=x["la"].cuda(), lb=x["lb"].cuda(), labels=labels.cuda())
    dev["la0"], dev["lb0"] = dev["la"].clone(), dev["lb"].clone()
    cwd = None if x["cw"] is None else x["cw"].cuda()
    fam = {"ce": "softmax_ce", "wce": "wce", "ohem": "ohem", "dice": "dice"}[family]
    fwd_grid, _, _ = fc.loss_grids(case)
    depth = fc.loss_depth(npix, fwd_grid)
    pair = form == "pair"
    single = run_family(fam, dev, case, cwd, False, dice)
    got = single
    if pair:
        got = run_family(fam, dev, case, cwd, True, dice)
        same_bits(got, single, "%s: pair against the two single calls" % cid)
    same_bits(run_family(fam, dev, case, cwd, pair, dice), got, "%s: a second launch" % cid)
    upv = R.UPSTREAM if up else 1.0
    wy = R.class_weights_of(labels, x["cw"], ign, C)
    worst = dict(loss=0.0, grad=0.0, p=0.0, dloss=0.0, dgrad=0.0)
    losses64 = []
    for h, z in enumerate((x["la"], x["lb"])):
        t = R.pixel_terms(z, labels, ign)
        scale = R.f32(hw[h]) * R.f32(upv)
        res, grad = got["res"][h], got["grad"][h].double()
        assert not bool(grad[ignored].any()), "%s: a non-zero gradient at an ignored pixel" % cid
        assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(res[:2]).all())
        if family in ("ce", "wce"):
            loss64, grad64, sum_w = R.ce_reference(z, labels, x["cw"], ign)
            grad64 = grad64 * scale
            l_der, g_der = R.mean_bound(t, wy, depth), R.ce_grad_bound(t, wy, depth, scale)
            if family == "ce":
                assert res[1].item() == nv
                g_env = grad_atol(float(nv))
            else:
                assert abs(res[1].item() - sum_w) <= (depth + 10) * R.U * sum_w
                g_env = 1e-7 * max(1.0, x["cw"].max().item() * ce_test_count() / max(sum_w, 1e-30))
            if sum_w <= 0.0:
                assert res[0].item() == 0.0 and not bool(grad.any())
            lerr, gerr = abs(res[0].item() - loss64), (grad - grad64).abs()
        elif family == "ohem":
            r = R.ohem_reference(case, z, labels)
            lab255 = torch.where(valid, labels, torch.full_like(labels, IGN))
            prob = got["prob"][h]
            assert bool(torch.isnan(prob[~valid]).all()) and not bool(torch.isnan(prob[valid]).any())
            p_bound = torch.full_like(t["p_own"], P_BOUND) if (t["envelope"] and C <= 7) else t["p_own_err"]
            worst["p"] = max(worst["p"], ratio((prob.double() - r["p"]).abs()[valid], p_bound[valid]))
            thr = res[2].item()
            assert thr == expected_device_threshold(dict(prob=prob), lab255, thresh, min_kept), (cid, thr)
            kept_dev = valid & (prob < thr)
            assert torch.equal(kept_dev, r["kept"]), "%s head %d: the kept mask differs at %d pixels" % (cid, h, int((kept_dev != r["kept"]).sum()))
            kept = int(r["kept"].sum())
            assert res[1].item() == kept and res[3].item() == nv
            assert not bool(grad[(~r["kept"]).unsqueeze(1).expand(N, C, H, W)].any())
            loss64, grad64 = r["loss"], r["grad"] * scale
            l_der, g_der = R.ohem_loss_bound(t, r["kept"], npix, depth), R.ohem_grad_bound(t, r["kept"], npix, scale)
            g_env = grad_atol(float(kept))
            if kept == 0:
                assert res[0].item() == 0.0 and not bool(grad.any())
            lerr, gerr = abs(res[0].item() - loss64), (grad - grad64).abs()
        else:
            kw = dict(ce_weight=dice[0], dice_weight=dice[1], smooth=dice[2], class_weight=x["cw"])
            terms, grad64 = DR.dice_ce_autograd(z, labels, ignore_index=ign, **kw)
            grad64 = grad64 * scale
            loss64 = terms["L"].item()
            l_der, d_der, g_der = R.dice_bounds(t, terms, wy, dice, depth, scale)
            g_env = dice_env_bound(terms, kw, C)
            want = torch.stack([terms["L"], terms["CE"], terms["Dice"]])
            lerr = (res[:3].double() - want).abs().max().item()
            assert abs(res[3].item() - terms["sum_w"].item()) <= (depth + 10) * R.U * terms["sum_w"].item() and res[4].item() == nv and not bool(res[5:].any())
            if nv == 0:
                assert res[0].item() == 0.0 and not bool(grad.any())
            gerr = (grad - grad64).abs()
        losses64.append(loss64)
        worst["dloss"], worst["dgrad"] = max(worst["dloss"], ratio(lerr, l_der)), max(worst["dgrad"], ratio(gerr, g_der))
        if t["envelope"]:
            worst["loss"], worst["grad"] = max(worst["loss"], ratio(lerr, 1e-5)), max(worst["grad"], ratio(gerr, torch.full_like(gerr, g_env * abs(scale))))
        else:
            worst["loss"], worst["grad"] = max(worst["loss"], ratio(lerr, l_der)), max(worst["grad"], ratio(gerr, g_der))
    if pair:
        a, b = torch.tensor(hw[0]) * got["res"][0][:1], torch.tensor(hw[1]) * got["res"][1][:1]
        want = (a + b).double()
        assert abs(got["total"].double().item() - want.item()) <= 2 * ulp32(torch.maximum(a.abs(), b.abs()).double()).item(), (got["total"], want)
    line = "  %-8s %-4s %-6s %dx%dx%dx%d %-9s %-8s env %d depth %d: loss %.3f grad %.3f p %.3f | derived: loss %.3f grad %.3f" % (
        cid, family, form, N, C, H, W, zpat, lpat, t["envelope"], depth, worst["loss"], worst["grad"], worst["p"], worst["dloss"], worst["dgrad"])
    LINES.append(line)
    print(line)
    assert worst["loss"] <= 1.0 and worst["grad"] <= 1.0 and worst["p"] <= 1.0, line
    # the identities between the entry points
    if family == "ce":
        for cw_arg, what in ((None, "NULL weight"), (torch.ones(C, device="cuda"), "all-ones weight")):
            same_bits(run_family("wce", dev, case, cw_arg, pair), got, "%s: emrt_wce_* with %s against emrt_softmax_ce_*" % (cid, what))
    if family == "dice":
        mix = run_family("wce", dev, case, cwd, pair)
        d0 = run_family("dice", dev, case, cwd, pair, (1.0, 0.0, 1.0))
        for h in range(2):
            assert d0["res"][h][1].item() == mix["res"][h][0].item() == d0["res"][h][0].item() and d0["res"][h][3].item() == mix["res"][h][1].item(), (cid, h)
            gm = mix["grad"][h].double()
            assert bool(((d0["grad"][h].double() - gm).abs() <= 2 * ulp32(gm)).all()), (cid, h)
