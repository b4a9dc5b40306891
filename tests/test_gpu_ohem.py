"""-m gpu: OhemCrossEntropyLoss with the threshold selected on the device, and class-weighted cross entropy (csrc/loss.hip), kernel and
model level.  The OHEM reference is a float64 restatement of the reference's formulae (losses/ohem_cross_entropy_loss.py:41-79), written
below; the yardstick of the weighted cross entropy is float64 torch.nn.functional.cross_entropy(weight=...).

Masks are compared EXACTLY.  That is sound because every case first asserts, on the CPU in float64, that no non-ignored pixel other than
the k-th itself has |p - threshold| < 1e-5 (a condition on the inputs, not a tolerance), while the fp32 p the kernel stores is within
25 * 2^-24 ~ 1.5e-6 of the exact value (<= 7 classes, x - max >= -16: the rounded a * log2(e) product |a| * 2^-24, one ulp of the hardware
exponential, 7 adds, one divide); that bound is asserted on the stored array and the measured maximum printed."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from emrt_amd import functional as Fn                                   # noqa: E402
from emrt_amd.runtime import ctx, F32, BF16, Tape                        # noqa: E402
from tests.hip_utils import init, dev, close, ulp32                      # noqa: E402

IGN = 255
MARGIN = 1e-5                 # input condition: distance of every other non-ignored p from the threshold
P_BOUND = 25 * 2.0 ** -24     # fp32 error of the stored p (module docstring)
INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 restatement of the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def own_class_prob(logits64, labels):
    """p of every pixel's own class and its CE in float64 (ignored pixels: class 0, masked by the caller)"""
    valid = labels != IGN
    lab = (labels * valid).unsqueeze(1)
    z = logits64 - logits64.max(1, keepdim=True).values
    e = z.exp()
    den = e.sum(1, keepdim=True)
    p = (e.gather(1, lab) / den).squeeze(1)
    ce = (den.log() - z.gather(1, lab)).squeeze(1)
    return p, ce, valid


def ohem_threshold(p, valid, thresh, min_kept):
    """-> (threshold, flat index of the k-th pixel among the valid ones or None): the three branches of the reference"""
    num_valid = int(valid.sum())
    if min_kept >= num_valid or num_valid == 0:
        return INF, None
    if min_kept <= 0:
        return thresh, None
    pv = p[valid]
    order = torch.argsort(pv, stable=True)
    kth = pv[order[min_kept - 1]].item()
    return (kth, int(order[min_kept - 1])) if kth > thresh else (thresh, None)


def ohem_ref(logits, labels, thresh, min_kept, mask=None):
    """float64 OHEM of one head.  mask: use this kept mask instead of the reference's own (the device's, at model level).
    -> dict(loss (differentiable in `logits`), p, ce, valid, threshold, kth_index, kept)"""
    p, ce, valid = own_class_prob(logits, labels)
    thr, kidx = ohem_threshold(p.detach(), valid, thresh, min_kept)
    kept = (valid & (p.detach() < thr)) if mask is None else mask
    npix = labels.numel()
    loss = (ce * kept).sum() / (kept.sum() + 1e-5 * npix)       # mean(loss * mask) / (mean(mask) + 1e-5), both times npix
    return dict(loss=loss, p=p.detach(), ce=ce.detach(), valid=valid, threshold=thr, kth_index=kidx, kept=kept)


def assert_input_margin(r, tied_with_kth=False):
    """no non-ignored pixel other than the k-th (with tied_with_kth: other than the pixels EQUAL to it) within MARGIN of the threshold"""
    if r["threshold"] == INF:
        return INF
    pv = r["p"][r["valid"]]
    d = (pv - r["threshold"]).abs()
    if tied_with_kth:
        d = d[pv != r["threshold"]]
    elif r["kth_index"] is not None:
        d[r["kth_index"]] = INF
    nearest = d.min().item() if d.numel() else INF
    assert nearest >= MARGIN, "input condition: a pixel lies %.3g from the threshold %.6f" % (nearest, r["threshold"])
    return nearest


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and the device run
# ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(recipe, seed, N=2, C=6, H=33, W=31, ignored=0.1):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (N, H, W), generator=g)
    if recipe == "hard":        # threshold stays thresh = 0.7: most pixels are below it
        logits = 2 * torch.randn(N, C, H, W, generator=g)
    else:                       # "easy": most pixels confident, the k-th smallest p is above 0.7 and becomes the threshold
        logits = torch.randn(N, C, H, W, generator=g) + 4 * F.one_hot(labels, C).permute(0, 3, 1, 2).float()
    labels[torch.rand(N, H, W, generator=g) < ignored] = IGN
    return logits, labels


def run_device(logits, labels, thresh, min_kept, weight=1.0, backward=True):
    c = init(F32)
    ld, lab = dev(logits, torch.float32), labels.cuda()
    tape = Tape()
    c.tape = tape if backward else None
    res, prob = Fn.ohem_ce(ld, lab, IGN, thresh, min_kept, weight)
    c.tape = None
    grad = None
    if backward:
        tape.watch(ld)
        tape.backward()
        grad = tape.result(ld).cpu()
    torch.cuda.synchronize()
    r = res.cpu()
    return dict(loss=r[0].item(), loss_t=r[:1].clone(), kept=r[1].item(), threshold=r[2].item(), threshold_t=r[2:3].clone(), num_valid=r[3].item(),
                prob=prob.cpu(), grad=grad)


def device_mask(d):
    """kept pixels as the GRADIENT shows them: a kept pixel's row is non-zero, a dropped one's is all zeros"""
    return (d["grad"] != 0).any(1)


def f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


def kth_of_stored(d, labels, min_kept):
    pv = d["prob"][labels != IGN]
    return torch.sort(pv).values[min_kept - 1]


def expected_device_threshold(d, labels, thresh, min_kept):
    """the three branches applied to the device's OWN stored p array, sorted on the host"""
    nv = int((labels != IGN).sum())
    if min_kept >= nv or nv == 0:
        return INF
    if min_kept <= 0:
        return f32(thresh)
    kth = kth_of_stored(d, labels, min_kept).item()
    return kth if kth > f32(thresh) else f32(thresh)


def assert_stored_p(d, r):
    valid = r["valid"]
    err = (d["prob"].double() - r["p"])[valid].abs().max().item() if valid.any() else 0.0
    print("stored p: max |fp32 - float64| = %.3g (bound %.3g)" % (err, P_BOUND))
    assert err <= P_BOUND
    assert torch.isnan(d["prob"][~valid]).all()          # ignored pixels: the pattern that compares false


@functools.lru_cache(maxsize=None)
def ce_test_count():
    """non-ignored pixels of tests/test_gpu_kernels.py::test_softmax_ce_and_optimizer (same generator calls): its gradient tolerance 1e-7 is stated at that count"""
    g = torch.Generator().manual_seed(14)
    torch.randn(3, 6, 16, 20, generator=g)
    labels = torch.randint(0, 6, (3, 16, 20), generator=g)
    labels[torch.rand(3, 16, 20, generator=g) < 0.1] = IGN
    return int((labels != IGN).sum())


def grad_atol(kept):
    """1e-7 at the existing CE test's pixel count; gradients scale with 1 / kept, so a smaller kept count scales the bound up -- never down"""
    return 1e-7 * max(1.0, ce_test_count() / max(kept, 1.0))


@functools.lru_cache(maxsize=None)
def case1(recipe, seed, C):
    logits, labels = make_inputs(recipe, seed, C=C)
    lr = logits.double().requires_grad_(True)
    r = ohem_ref(lr, labels, 0.7, 500)
    r["loss"].backward()
    r["grad"] = lr.grad.float()
    r["loss"] = r["loss"].detach()
    return logits, labels, r


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,seed,C", [("hard", 100, 6), ("easy", 101, 6), ("easy", 102, 7), ("hard", 103, 7)])
def test_ohem_matches_float64_reference(recipe, seed, C):
    """2 x C x 33 x 31 (ragged: no multiple of a block or a vector), 10 % ignored, min_kept 500, thresh 0.7: both threshold branches"""
    logits, labels, r = case1(recipe, seed, C)
    nearest = assert_input_margin(r)
    assert (r["threshold"] == 0.7) == (recipe == "hard")          # each recipe reaches its branch
    d = run_device(logits, labels, 0.7, 500)
    assert_stored_p(d, r)
    kept_ref = int(r["kept"].sum())
    print("%s C=%d: threshold %.6f (device %.6f), kept %d of %d valid, nearest other p %.3g away" % (
        recipe, C, r["threshold"], d["threshold"], kept_ref, int(r["valid"].sum()), nearest))
    assert torch.equal(device_mask(d), r["kept"])
    assert d["kept"] == kept_ref and d["num_valid"] == int(r["valid"].sum())
    if recipe == "easy":
        assert kept_ref <= 499                                    # strict <: the k-th pixel itself is dropped
        assert torch.equal(d["threshold_t"], kth_of_stored(d, labels, 500).reshape(1))      # bit for bit
    assert d["threshold"] == expected_device_threshold(d, labels, 0.7, 500)
    close("ohem loss", d["loss_t"], r["loss"].float().reshape(1), F32, atol=1e-5)
    close("ohem dlogits", d["grad"], r["grad"], F32, atol=grad_atol(kept_ref))


def test_ohem_keeps_every_valid_pixel_when_min_kept_reaches_their_number():
    """min_kept >= num_valid: threshold +inf; the gradient is the plain CE gradient times count / (count + 1e-5 N), within 2 ulp"""
    logits, labels, _ = case1("hard", 100, 6)
    count, npix = int((labels != IGN).sum()), labels.numel()
    c = init(F32)
    ld = dev(logits, torch.float32)
    tape = Tape()
    c.tape = tape
    Fn.softmax_ce(ld, labels.cuda(), IGN, 1.0)
    c.tape = None
    tape.watch(ld)
    tape.backward()
    want = tape.result(ld).cpu().double() * (count / (count + 1e-5 * npix))
    lr = logits.double()
    for min_kept in (count, count + 1, 10 ** 9):
        d = run_device(logits, labels, 0.7, min_kept)
        assert d["threshold"] == INF and d["kept"] == count == d["num_valid"]
        assert torch.equal(device_mask(d), labels != IGN)
        assert ((d["grad"].double() - want).abs() <= 2 * ulp32(want)).all()
        r = ohem_ref(lr, labels, 0.7, min_kept)
        close("ohem keep-all loss", d["loss_t"], r["loss"].float().reshape(1), F32, atol=1e-5)
    # one below: the selection runs (rank count - 1 of count)
    d = run_device(logits, labels, 0.7, count - 1)
    assert d["threshold"] == expected_device_threshold(d, labels, 0.7, count - 1) and d["threshold"] != INF


def test_ohem_min_kept_zero_uses_thresh():
    for recipe, seed in (("hard", 100), ("easy", 101)):
        logits, labels, _ = case1(recipe, seed, 6)
        r = ohem_ref(logits.double(), labels, 0.7, 0)
        assert r["threshold"] == 0.7
        assert_input_margin(r)
        d = run_device(logits, labels, 0.7, 0)
        assert d["threshold"] == f32(0.7)
        assert torch.equal(device_mask(d), r["kept"]) and d["kept"] == int(r["kept"].sum())
        close("ohem loss", d["loss_t"], r["loss"].float().reshape(1), F32, atol=1e-5)


def test_ohem_heavy_ties():
    """C = 2, logits on a grid of 0.5: a few dozen distinct p, min_kept inside a tie group, thresh 0.1 -> the whole group is dropped"""
    g = torch.Generator().manual_seed(7)
    N, C, H, W = 2, 2, 33, 31
    logits = torch.round(2 * torch.randn(N, C, H, W, generator=g)) / 2
    labels = torch.randint(0, C, (N, H, W), generator=g)
    labels[torch.rand(N, H, W, generator=g) < 0.1] = IGN
    nv = int((labels != IGN).sum())
    min_kept = nv // 2
    lr = logits.double().requires_grad_(True)
    r = ohem_ref(lr, labels, 0.1, min_kept)
    r["loss"].backward()
    pv = torch.sort(r["p"][r["valid"]]).values
    assert pv.unique().numel() <= 48
    assert pv[min_kept - 2] == pv[min_kept - 1] == pv[min_kept] and r["threshold"] == pv[min_kept - 1].item() > 0.1      # inside a tie group
    assert_input_margin(r, tied_with_kth=True)
    d = run_device(logits, labels, 0.1, min_kept)
    assert_stored_p(d, r)
    # ties are exact in both precisions: every float64 tie group is ONE bit pattern in the stored array, and the groups stay distinct
    valid = r["valid"]
    u, inv = torch.unique(r["p"][valid], return_inverse=True)
    sp = d["prob"][valid]
    lo = torch.full((u.numel(),), INF).scatter_reduce(0, inv, sp, "amin")
    hi = torch.full((u.numel(),), -INF).scatter_reduce(0, inv, sp, "amax")
    assert torch.equal(lo, hi) and lo.unique().numel() == u.numel()
    group = int((r["p"][valid] == r["threshold"]).sum())
    kept_ref = int(r["kept"].sum())
    print("ties: %d distinct p, tie group of %d around rank %d, kept %d" % (u.numel(), group, min_kept, kept_ref))
    assert group >= 3 and kept_ref <= min_kept - 2
    assert torch.equal(device_mask(d), r["kept"]) and d["kept"] == kept_ref
    assert torch.equal(d["threshold_t"], kth_of_stored(d, labels, min_kept).reshape(1))
    close("ohem ties loss", d["loss_t"], r["loss"].detach().float().reshape(1), F32, atol=1e-5)
    close("ohem ties dlogits", d["grad"], lr.grad.float(), F32, atol=grad_atol(kept_ref))
    # all pixels identical with p = 0.5 > thresh: the threshold is their own p and nothing is below it
    z = torch.zeros(N, C, H, W)
    d = run_device(z, labels, 0.1, 10)
    assert d["threshold"] == 0.5 and d["kept"] == 0.0 and d["loss"] == 0.0 and d["num_valid"] == nv
    assert not d["grad"].any() and torch.isfinite(d["grad"]).all()


def test_ohem_all_labels_ignored():
    logits, labels, _ = case1("hard", 100, 6)
    d = run_device(logits, torch.full_like(labels, IGN), 0.7, 500)
    assert d["loss"] == 0.0 and d["kept"] == 0.0 and d["num_valid"] == 0.0 and d["threshold"] == INF
    assert not d["grad"].any() and torch.isfinite(d["grad"]).all() and math.isfinite(d["loss"])


def test_ohem_training_size_selection():
    """8 x 6 x 256 x 256, recipe "easy", min_kept 100 000: bins far above 65 535, the full grid; threshold and count against the host sort
    of the stored p"""
    logits, labels = make_inputs("easy", 104, N=8, C=6, H=256, W=256)
    d = run_device(logits, labels, 0.7, 100000, backward=False)
    valid = labels != IGN
    want = expected_device_threshold(d, labels, 0.7, 100000)
    kth = kth_of_stored(d, labels, 100000)
    print("training size: threshold %.7f, k-th stored p %.7f, kept %d of %d valid" % (d["threshold"], kth.item(), int(d["kept"]), int(valid.sum())))
    assert d["threshold"] == want
    if kth.item() > f32(0.7):
        assert torch.equal(d["threshold_t"], kth.reshape(1))
    assert d["num_valid"] == int(valid.sum())
    assert d["kept"] == int((d["prob"][valid] < d["threshold"]).sum())
    p, ce, _ = own_class_prob(logits.double(), labels)
    kept = valid & (d["prob"] < d["threshold"])
    loss = (ce * kept).sum() / (kept.sum() + 1e-5 * labels.numel())
    close("ohem training-size loss", d["loss_t"], loss.float().reshape(1), F32, atol=1e-5)


def test_ohem_is_bit_reproducible():
    logits, labels, _ = case1("easy", 101, 6)
    a, b = run_device(logits, labels, 0.7, 500), run_device(logits, labels, 0.7, 500)
    assert torch.equal(a["loss_t"], b["loss_t"]) and torch.equal(a["threshold_t"], b["threshold_t"]) and torch.equal(a["grad"], b["grad"])
    assert torch.equal(a["prob"][labels != IGN], b["prob"][labels != IGN]) and a["kept"] == b["kept"]


def test_ohem_pair_equals_the_two_single_head_calls():
    """both heads through the launches of one (emrt_ohem_ce_pair_*): results, stored p and gradients bit-identical to two single-head calls,
    the two heads on DIFFERENT threshold branches; total = wa * loss_a + wb * loss_b"""
    la, labels, _ = case1("easy", 101, 6)          # threshold = its k-th smallest p
    lb = make_inputs("hard", 101, C=6)[0]           # threshold stays 0.7 (same labels: the head of another network state)
    single = [run_device(la, labels, 0.7, 500, weight=1.0), run_device(lb, labels, 0.7, 500, weight=0.4)]
    assert single[0]["threshold"] > f32(0.7) and single[1]["threshold"] == f32(0.7)
    c = init(F32)
    ad, bd, lab = dev(la, torch.float32), dev(lb, torch.float32), labels.cuda()
    tape = Tape()
    c.tape = tape
    ra, rb, total, pa, pb = Fn.ohem_ce_pair(ad, bd, lab, IGN, 0.7, 500, 1.0, 0.4)
    c.tape = None
    tape.watch(ad)
    tape.watch(bd)
    tape.backward()
    valid = labels != IGN
    for res, prob, x, s in ((ra, pa, ad, single[0]), (rb, pb, bd, single[1])):
        r = res.cpu()
        assert torch.equal(r[:1], s["loss_t"]) and r[1].item() == s["kept"] and torch.equal(r[2:3], s["threshold_t"]) and r[3].item() == s["num_valid"]
        assert torch.equal(prob.cpu()[valid], s["prob"][valid]) and torch.equal(tape.result(x).cpu(), s["grad"])
    want = torch.tensor(1.0, dtype=torch.float32) * single[0]["loss_t"] + torch.tensor(0.4, dtype=torch.float32) * single[1]["loss_t"]
    assert abs(total.item() - want.item()) <= 2 * ulp32(want.double()).item()


def _ce_inputs(shape, seed, ignored):
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    la, lb = torch.randn(N, C, H, W, generator=g) * 2, torch.randn(N, C, H, W, generator=g) * 3
    labels = torch.randint(0, C, (N, H, W), generator=g)
    labels[torch.rand(N, H, W, generator=g) < ignored] = IGN
    w = 0.5 + 1.5 * torch.rand(C, generator=g)          # class weights in [0.5, 2]
    return la, lb, labels, w


def _run_ce(la, lb, labels, cw, pair):
    """-> [loss a, loss b, dlogits a, dlogits b(, total)] of softmax_ce (1.0 / 0.4) or softmax_ce_pair on the device"""
    c = init(F32)
    ad, bd, lab = dev(la, torch.float32), dev(lb, torch.float32), labels.cuda()
    cwd = None if cw is None else dev(cw, torch.float32)
    tape = Tape()
    c.tape = tape
    if pair:
        ra, rb, total = Fn.softmax_ce_pair(ad, bd, lab, IGN, 1.0, 0.4, class_weight=cwd) if cwd is not None else Fn.softmax_ce_pair(ad, bd, lab, IGN, 1.0, 0.4)
    else:
        kw = {} if cwd is None else {"class_weight": cwd}
        ra, rb, total = Fn.softmax_ce(ad, lab, IGN, 1.0, **kw), Fn.softmax_ce(bd, lab, IGN, 0.4, **kw), None
    c.tape = None
    tape.watch(ad)
    tape.watch(bd)
    tape.backward()
    out = [ra.cpu(), rb.cpu(), tape.result(ad).cpu(), tape.result(bd).cpu()]
    return out + ([total.cpu()] if total is not None else [])


@pytest.mark.parametrize("shape,seed,ignored", [((3, 6, 16, 20), 34, 0.1), ((4, 7, 24, 40), 35, 0.15)])
def test_weighted_cross_entropy(shape, seed, ignored):
    """single and pair form against float64 F.cross_entropy(weight=w, ignore_index=255); with unit weights within 2 ulp of the unweighted
    entry points"""
    la, lb, labels, w = _ce_inputs(shape, seed, ignored)
    ra_, rb_ = la.double().requires_grad_(True), lb.double().requires_grad_(True)
    ref_a = F.cross_entropy(ra_, labels, weight=w.double(), ignore_index=IGN)
    ref_b = F.cross_entropy(rb_, labels, weight=w.double(), ignore_index=IGN)
    (ref_a + 0.4 * ref_b).backward()
    valid = labels != IGN
    wsum = w[labels[valid]].double().sum().item()
    # gradients are w[y] / sum w (softmax - onehot): against the unweighted 1 / count of the existing test they are at most max(w) count' / sum w
    # times larger, and the absolute bound scales with them (never below 1e-7)
    atol = 1e-7 * max(1.0, w.max().item() * ce_test_count() / wsum)
    for pair in (False, True):
        got = _run_ce(la, lb, labels, w, pair)
        what = "pair" if pair else "single"
        close("wce %s loss a" % what, got[0][:1], ref_a.detach().float().reshape(1), F32, atol=1e-5)
        close("wce %s loss b" % what, got[1][:1], ref_b.detach().float().reshape(1), F32, atol=1e-5)
        assert abs(got[0][1].item() - wsum) <= 1e-6 * wsum and got[1][1].item() == got[0][1].item()
        close("wce %s dlogits a" % what, got[2], ra_.grad.float(), F32, atol=atol)
        close("wce %s dlogits b" % what, got[3], rb_.grad.float(), F32, atol=atol)
        if pair:
            close("wce pair total", got[4], (ref_a + 0.4 * ref_b).detach().float().reshape(1), F32, atol=1e-5)
        ones = _run_ce(la, lb, labels, torch.ones(shape[1]), pair)
        plain = _run_ce(la, lb, labels, None, pair)
        for u, v, name in zip(ones, plain, ("loss a", "loss b", "dlogits a", "dlogits b", "total")):
            assert ((u.double() - v.double()).abs() <= 2 * ulp32(v.double())).all(), "%s %s: unit weights differ from the unweighted entry point" % (what, name)
    # every pixel ignored: 0, not 0 / 0
    got = _run_ce(la, lb, torch.full_like(labels, IGN), w, True)
    assert got[0][0].item() == got[1][0].item() == got[4].item() == 0.0 and not got[2].any() and not got[3].any()


def _abi_ce(family, la, lb, lab, pair, up):
    """The C-ABI itself, family "softmax_ce" or "wce" with class_weight = NULL (functional never passes a null weight to emrt_wce_*):
    -> [result a, result b, dlogits a, dlogits b(, total)], head weights 1.0 / 0.4, upstream `up` (device scalar or None)."""
    import ctypes
    from emrt_amd import _lib
    L, c = _lib.lib(), ctx()
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    cw = (None,) if family == "wce" else ()                      # the extra argument of emrt_wce_*: behind labels
    N, C, H, W = la.shape
    ws = torch.empty(L.query("emrt_ce_workspace_bytes"), dtype=torch.uint8, device="cuda")
    ra, rb, total = (torch.full((2,), -1.0, device="cuda") for _ in range(3))
    da, db = torch.full_like(la, 7.0), torch.full_like(lb, 7.0)
    if pair:
        L.call("emrt_%s_pair_fwd" % family, P(la), P(lb), P(lab), *cw, N, C, H, W, IGN, 1.0, 0.4, P(ra), P(rb), P(total), P(ws), c.stream)
        L.call("emrt_%s_pair_bwd" % family, P(la), P(lb), P(lab), *cw, P(ra), P(up), P(up), 1.0, 0.4, N, C, H, W, IGN, P(da), P(db), c.stream)
    else:
        for lg, r, d, wgt in ((la, ra, da, 1.0), (lb, rb, db, 0.4)):
            L.call("emrt_%s_fwd" % family, P(lg), P(lab), *cw, N, C, H, W, IGN, P(r), P(ws), c.stream)
            L.call("emrt_%s_bwd" % family, P(lg), P(lab), *cw, P(r), P(up), wgt, N, C, H, W, IGN, P(d), c.stream)
    torch.cuda.synchronize()
    return [ra.cpu(), rb.cpu(), da.cpu(), db.cpu()] + ([total.cpu()] if pair else [])


@pytest.mark.parametrize("shape,seed,ignored", [((3, 6, 16, 20), 34, 0.1), ((4, 7, 24, 40), 35, 0.15), ((3, 6, 16, 20), 36, 1.0)],
                         ids=["3x6x16x20", "4x7x24x40", "all_ignored"])
def test_null_class_weight_takes_the_plain_kernels(shape, seed, ignored):
    """emrt_wce_* with class_weight = NULL against emrt_softmax_ce_*, single and pair form: results, total and both gradients are the same
    bits (they are the same kernels)."""
    init(F32)
    la, lb, labels, _ = _ce_inputs(shape, seed, ignored)
    assert bool((labels == IGN).all()) == (ignored == 1.0)
    la, lb, lab = la.cuda(), lb.cuda(), labels.cuda()
    up = torch.tensor([0.37], device="cuda")
    for pair in (False, True):
        for u in (None, up):
            plain, null_w = _abi_ce("softmax_ce", la, lb, lab, pair, u), _abi_ce("wce", la, lb, lab, pair, u)
            for a, b, name in zip(null_w, plain, ("result a", "result b", "dlogits a", "dlogits b", "total")):
                assert torch.equal(a, b), (pair, u is not None, name, int((a != b).sum()))
            assert not bool((plain[2] == 7.0).any()) and bool(plain[2].any()) != (ignored == 1.0)      # the gradient was written, and is zero only when all is ignored


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: ResNet-18, 2 x 64 x 64, 6 classes
# ---------------------------------------------------------------------------------------------------------------------------------
def _model_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, 64, 64, generator=g)
    labels = torch.randint(0, 6, (2, 64, 64), generator=g)
    labels[torch.rand(2, 64, 64, generator=g) < 0.05] = IGN
    return x, labels


def _cosine(model, ref):
    refp = dict(ref.named_parameters())
    dot = n1 = n2 = 0.0
    for n, p in model.named_parameters():
        gr = refp[n].grad
        if gr is None:
            continue
        gg, gr = p.grad.cpu().double(), gr.double()
        dot += float((gg * gr).sum()); n1 += float((gg * gg).sum()); n2 += float((gr * gr).sum())
    return dot / (n1 ** 0.5 * n2 ** 0.5)


def test_model_ohem_train_step_fp32():
    """one train step under OHEM (min_kept 1000 of 8192): the float64 OHEM evaluated on the HIP model's own logits gives the same masks up to
    pixels within 1e-5 of the threshold (<= 8 per head) and, with the device masks, the same loss; the whole gradient follows autograd through
    the oracle EMRT"""
    from emrt_amd.src.models.losses import get_loss_function
    from tests.test_gpu_model import build_pair, make_config
    thresh, min_kept = 0.7, 1000
    x, labels = _model_inputs(41)
    ref, model = build_pair("resnet18", x, perturb=True, condition=0.1)
    cfg = make_config("resnet18")
    cfg.TRAIN.LOSS = "OhemCrossEntropyLoss"
    cfg.TRAIN.OHEM.THRESH, cfg.TRAIN.OHEM.MIN_KEPT = thresh, min_kept
    loss_fn = get_loss_function(cfg)
    ref.double().train()
    out_r = ref(x.double())
    loss_r = sum(w * ohem_ref(o, labels, thresh, min_kept)["loss"] for o, w in zip(out_r, (1.0, 0.4)))
    loss_r.backward()
    model.train()
    model.clear_gradients()
    out = model(x.cuda())
    logits = [out[0].cpu().double(), out[1].cpu().double()]
    loss = loss_fn(out, labels.cuda())
    parts = [p.cpu() for p in loss.parts]
    probs = [p.cpu() for p in loss_fn.last_prob]
    loss.backward()
    torch.cuda.synchronize()
    total = 0.0
    for h, w in enumerate((1.0, 0.4)):
        r = ohem_ref(logits[h], labels, thresh, min_kept)
        dmask = r["valid"] & (probs[h] < parts[h][2])
        diff = dmask != r["kept"]
        near = (r["p"] - r["threshold"]).abs() < MARGIN
        print("head %d: threshold %.6f (device %.6f), kept %d (device %d), masks differ at %d pixels" % (
            h, r["threshold"], parts[h][2].item(), int(r["kept"].sum()), int(parts[h][1].item()), int(diff.sum())))
        assert not (diff & ~near).any() and int(diff.sum()) <= 8
        assert parts[h][1].item() == int(dmask.sum())
        total += w * ohem_ref(logits[h], labels, thresh, min_kept, mask=dmask)["loss"].item()
    print("OHEM train loss %.6f, float64 on the same logits and masks %.6f, oracle EMRT %.6f" % (loss.item(), total, loss_r.item()))
    assert abs(loss.item() - total) < 2e-4 * max(1.0, abs(total))
    cos = _cosine(model, ref)
    print("OHEM whole-gradient cosine vs the oracle EMRT %.6f" % cos)
    assert cos > 0.999


def test_model_weighted_mix_train_step_fp32():
    from emrt_amd.src.models.losses import get_loss_function
    from tests.test_gpu_model import build_pair, make_config
    x, labels = _model_inputs(42)
    w = [1.0, 2.0, 0.5, 1.5, 3.0, 0.75]
    ref, model = build_pair("resnet18", x, perturb=True, condition=0.1)
    cfg = make_config("resnet18")
    cfg.TRAIN.CLASS_WEIGHTS = w
    ref.double().train()
    out_r = ref(x.double())
    wt = torch.tensor(w, dtype=torch.float64)
    loss_r = F.cross_entropy(out_r[0], labels, weight=wt, ignore_index=IGN) + 0.4 * F.cross_entropy(out_r[1], labels, weight=wt, ignore_index=IGN)
    loss_r.backward()
    model.train()
    model.clear_gradients()
    loss = get_loss_function(cfg)(model(x.cuda()), labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    cos = _cosine(model, ref)
    print("weighted Mix train loss %.6f vs oracle %.6f, whole-gradient cosine %.6f" % (loss.item(), loss_r.item(), cos))
    assert abs(loss.item() - loss_r.item()) < 2e-4 * max(1.0, abs(loss_r.item()))
    assert cos > 0.999


# (last in the file: a loss that synchronised or allocated under capture would fail here; it is not retried)
def test_model_ohem_captured_bf16_step_equals_eager():
    """bf16, OHEM: three steps of TrainEngine captured from its first call (use_graph=True, warmup_eager=0) against the eager engine"""
    from emrt_amd.engine import TrainEngine
    from emrt_amd.src.models import get_model
    from emrt_amd.src.models.losses import get_loss_function
    from emrt_amd.src.models.solver import get_optimizer, get_scheduler
    from tests.test_gpu_model import calibrated_oracle, make_config
    x, labels = _model_inputs(43)
    ref = calibrated_oracle("resnet18", x, seed=1, condition=0.1)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    xd, ld = x.cuda(), labels.cuda()
    runs = {}
    for mode in ("eager", "graph"):
        cfg = make_config("resnet18")
        cfg.TRAIN.LOSS = "OhemCrossEntropyLoss"
        cfg.TRAIN.OHEM.MIN_KEPT = 1000
        model = get_model(cfg)
        model.load_state_dict(state)
        model.to_hip("cuda:0", BF16)
        model.set_dropout(0.0)
        model.eval()
        model(xd)
        model.train()
        opt = get_optimizer(model, get_scheduler(cfg), cfg)
        loss_fn = get_loss_function(cfg)
        eng = TrainEngine(model, opt, loss_fn, 1, use_graph=(mode == "graph"), warmup_eager=0)
        losses = [eng.step(xd, ld).item() for _ in range(3)]
        torch.cuda.synchronize()
        n = model.store.n_train
        runs[mode] = (losses, model.store.master[:n].clone())
        if mode == "graph":
            assert eng.graph_a is not None and eng.calls == 3
    print("OHEM bf16 losses eager %s captured %s" % (runs["eager"][0], runs["graph"][0]))
    for a, b in zip(runs["eager"][0], runs["graph"][0]):
        assert math.isfinite(b) and abs(a - b) < 1e-3 * abs(a), (a, b)
    we, wg = runs["eager"][1], runs["graph"][1]
    assert float((we - wg).norm() / we.norm()) < 2e-4
