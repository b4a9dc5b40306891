"""-m gpu: DiceCrossEntropyLoss (csrc/loss_ext/loss_ext.hip, include/emrt_hip_loss.h), kernel and model level.  The yardstick is the float64
restatement of the contract in tests/dice_reference.py (torch autograd); tests/test_dice_cpu.py pins that restatement itself.

Tolerances.  Loss scalars: atol 1e-5, the bound tests/test_gpu_ohem.py holds fp32 loss scalars to.  Gradients: atol = 1e-7 * K * G, the existing
grad_atol rule (1e-7 at gradient scale 1 / K, K = ce_test_count()) applied to this loss's largest possible entry
G = CE_WEIGHT max(w) / sum w[y] + 3 DICE_WEIGHT / (C min_c U_c), taken from the float64 run: |g_c| <= 2 DICE_WEIGHT / (C U_c),
0 <= b_c <= DICE_WEIGHT / (C U_c), p <= 1.  A head of weight 0.4 is held to 0.4 of the bound.  No relative term in either."""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import functional as Fn                                   # noqa: E402
from emrt_amd.runtime import ctx, F32, BF16, Tape                        # noqa: E402
from tests import dice_reference as R                                    # noqa: E402
from tests.hip_utils import init, dev, close, ulp32                      # noqa: E402
from tests.test_gpu_ohem import ce_test_count, _cosine, _model_inputs    # noqa: E402

IGN = R.IGN
HEAD_W = (1.0, 0.4)

# name -> (shape, seed, smooth, class weights?, absent class, every class present, CE_WEIGHT, DICE_WEIGHT)
CASES = {
    "2x7x33x31_s1": ((2, 7, 33, 31), 50, 1.0, False, None, False, 1.0, 1.0),          # odd extent, C < 8
    "2x7x33x31_s0": ((2, 7, 33, 31), 50, 0.0, False, None, True, 1.0, 1.0),
    "1x9x5x3_s1": ((1, 9, 5, 3), 51, 1.0, False, None, False, 1.0, 1.0),             # two class chunks, fewer pixels than one block
    "1x9x5x3_s0": ((1, 9, 5, 3), 51, 0.0, False, None, True, 0.5, 2.0),
    "3x6x16x20_weighted": ((3, 6, 16, 20), 52, 1.0, True, None, False, 1.5, 0.75),
    "2x6x16x20_absent": ((2, 6, 16, 20), 53, 1.0, False, 4, False, 1.0, 1.0),
    "5x6x256x256": ((5, 6, 256, 256), 54, 1.0, False, None, False, 1.0, 1.0),         # 327 680 pixels: the 1024-block forward grid strides
}


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and the float64 reference of both heads, computed once and shared (never modified)"""
    shape, seed, smooth, weighted, absent, present, cew, dw = CASES[name]
    la, labels = R.make_case(shape, seed, ignored=0.1, absent=absent, all_present=present)
    lb = 3 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1000))
    C = shape[1]
    cw = 0.5 + 1.5 * torch.rand(C, generator=torch.Generator().manual_seed(seed + 2000)) if weighted else None
    kw = dict(ce_weight=cew, dice_weight=dw, smooth=smooth, class_weight=cw)
    refs = [R.dice_ce_autograd(z, labels, **kw) for z in (la, lb)]
    if absent is not None:
        assert refs[0][0]["T"][absent].item() == 0
    if present:
        assert (refs[0][0]["T"] > 0).all()
    assert (labels == IGN).any() and shape[0] * shape[2] * shape[3] > 0
    return dict(la=la, lb=lb, labels=labels, kw=kw, refs=refs, C=C)


def grad_bound(terms, kw, C):
    """1e-7 * K * G (module docstring), from the float64 run"""
    wmax = 1.0 if kw["class_weight"] is None else kw["class_weight"].max().item()
    G = kw["ce_weight"] * wmax / terms["sum_w"].item() + 3 * kw["dice_weight"] / (C * terms["U"].min().item())
    return 1e-7 * ce_test_count() * G


def run_device(la, lb, labels, kw, pair, tape_on=True):
    """-> [result a, result b, dlogits a, dlogits b(, total)] of dice_ce (head weights 1.0 / 0.4) or dice_ce_pair on the device"""
    c = init(F32)
    ad, bd, lab = dev(la, torch.float32), dev(lb, torch.float32), labels.cuda()
    kw = dict(kw, class_weight=None if kw["class_weight"] is None else dev(kw["class_weight"], torch.float32))
    tape = Tape()
    c.tape = tape
    try:
        if pair:
            ra, rb, total = Fn.dice_ce_pair(ad, bd, lab, IGN, HEAD_W[0], HEAD_W[1], **kw)
        else:
            ra, rb, total = Fn.dice_ce(ad, lab, IGN, HEAD_W[0], **kw), Fn.dice_ce(bd, lab, IGN, HEAD_W[1], **kw), None
    finally:
        c.tape = None
    tape.watch(ad)
    tape.watch(bd)
    tape.backward()
    torch.cuda.synchronize()
    out = [ra.cpu(), rb.cpu(), tape.result(ad).cpu(), tape.result(bd).cpu()]
    return out + ([total.cpu()] if total is not None else [])


@pytest.mark.parametrize("name", list(CASES))
def test_dice_ce_matches_float64_reference(name):
    """single and pair form: L, CE, Dice, sum w, the non-ignored count and both gradients against float64 autograd; exact zeros at the ignored
    pixels; the pair form gives each head the single form's bits"""
    k = case(name)
    labels, kw, C = k["labels"], k["kw"], k["C"]
    ign = (labels == IGN).unsqueeze(1)
    got = {pair: run_device(k["la"], k["lb"], labels, kw, pair) for pair in (False, True)}
    for pair, what in ((False, "single"), (True, "pair")):
        for h, hw in enumerate(HEAD_W):
            terms, grad = k["refs"][h]
            res, dl = got[pair][h], got[pair][2 + h]
            want = torch.stack([terms["L"], terms["CE"], terms["Dice"]]).float()
            print("%s %s head %d: L %.7f (ref %.7f) CE %.7f (%.7f) Dice %.7f (%.7f); max |dlogits - ref| %.3g (bound %.3g), min U %.4g" % (
                name, what, h, res[0].item(), want[0].item(), res[1].item(), want[1].item(), res[2].item(), want[2].item(),
                (dl.double() - hw * grad).abs().max().item(), hw * grad_bound(terms, kw, C), terms["U"].min().item()))
            close("dice %s %s L/CE/Dice head %d" % (name, what, h), res[:3], want, F32, atol=1e-5, rtol=0.0)
            assert abs(res[3].item() - terms["sum_w"].item()) <= 1e-6 * terms["sum_w"].item() and res[4].item() == terms["num_valid"].item()
            assert not res[5:].any()
            close("dice %s %s dlogits head %d" % (name, what, h), dl, (hw * grad).float(), F32, atol=hw * grad_bound(terms, kw, C), rtol=0.0)
            assert not dl[ign.expand_as(dl)].any() and dl[~ign.expand_as(dl)].any()
        if pair:
            want_total = sum(hw * k["refs"][h][0]["L"] for h, hw in enumerate(HEAD_W)).float().reshape(1)
            close("dice %s pair total" % name, got[True][4], want_total, F32, atol=1e-5, rtol=0.0)
    for a, b, part in zip(got[True], got[False], ("result a", "result b", "dlogits a", "dlogits b")):
        assert torch.equal(a, b), "%s: the pair form's %s differs from the single call at %d places" % (name, part, int((a != b).sum()))


@pytest.mark.parametrize("smooth", [1.0, 0.0])
def test_all_pixels_ignored_gives_zero_loss_and_zero_gradient(smooth):
    k = case("3x6x16x20_weighted")
    for pair in (False, True):
        got = run_device(k["la"], k["lb"], torch.full_like(k["labels"], IGN), dict(k["kw"], smooth=smooth), pair)
        assert got[0][0].item() == got[1][0].item() == 0.0 and got[0][4].item() == 0.0
        assert not got[2].any() and not got[3].any()
        assert not pair or got[4].item() == 0.0


def test_two_runs_give_equal_bits():
    k = case("5x6x256x256")
    one, two = (run_device(k["la"], k["lb"], k["labels"], k["kw"], True) for _ in range(2))
    for a, b in zip(one, two):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["2x7x33x31_s1", "3x6x16x20_weighted", "5x6x256x256"])
def test_dice_weight_zero_is_the_mix_loss(name):
    """DICE_WEIGHT = 0, CE_WEIGHT = 1: CE and L carry the bits of functional.softmax_ce (plain, and weighted where the case has class weights);
    the gradient is within 2 ulp of it"""
    k = case(name)
    c = init(F32)
    cw = None if k["kw"]["class_weight"] is None else dev(k["kw"]["class_weight"], torch.float32)
    lab = k["labels"].cuda()
    for z, hw in ((k["la"], HEAD_W[0]), (k["lb"], HEAD_W[1])):
        zd = dev(z, torch.float32)
        outs = []
        for fn in (lambda: Fn.softmax_ce(zd, lab, IGN, hw, class_weight=cw),
                   lambda: Fn.dice_ce(zd, lab, IGN, hw, class_weight=cw, ce_weight=1.0, dice_weight=0.0, smooth=1.0)):
            tape = Tape()
            c.tape = tape
            try:
                res = fn()
            finally:
                c.tape = None
            tape.watch(zd)
            tape.backward()
            torch.cuda.synchronize()
            outs.append((res.cpu(), tape.result(zd).cpu()))
        (mix, gmix), (dice, gdice) = outs
        assert dice[1].item() == mix[0].item() and dice[0].item() == mix[0].item(), (dice[:3].tolist(), mix.tolist())
        assert dice[3].item() == mix[1].item()
        assert ((gdice.double() - gmix.double()).abs() <= 2 * ulp32(gmix.double())).all()


def test_upstream_scalar_halves_the_gradient_exactly():
    from emrt_amd import _lib
    k = case("2x7x33x31_s1")
    c = init(F32)
    X = _lib.loss_lib()
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    la, lb, lab = k["la"].cuda(), k["lb"].cuda(), k["labels"].cuda()
    N, C, H, W = la.shape
    ws = torch.empty(X.query("emrt_lx_dice_ce_workspace_bytes", C, 2), dtype=torch.uint8, device="cuda")
    ra, rb, total = (torch.full((8,), -1.0, device="cuda") for _ in range(3))
    ca, cb = torch.empty(2 * C, device="cuda"), torch.empty(2 * C, device="cuda")
    X.call("emrt_lx_dice_ce_pair_fwd", P(la), P(lb), P(lab), None, N, C, H, W, IGN, 1.0, 0.4, 1.0, 1.0, 1.0, P(ra), P(rb), P(ca), P(cb), P(total), P(ws), c.stream)
    grads = {}
    for name, up in (("none", None), ("one", torch.tensor([1.0], device="cuda")), ("half", torch.tensor([0.5], device="cuda"))):
        da, db = torch.full_like(la, 7.0), torch.full_like(lb, 7.0)
        X.call("emrt_lx_dice_ce_pair_bwd", P(la), P(lb), P(lab), None, P(ra), P(rb), P(ca), P(cb), P(up), P(up), 1.0, 0.4, 1.0, N, C, H, W, IGN, P(da), P(db),
               c.stream)
        torch.cuda.synchronize()
        grads[name] = (da.cpu(), db.cpu())
    for h in range(2):
        assert not (grads["none"][h] == 7.0).any() and grads["none"][h].any()              # every entry was written
        assert torch.equal(grads["one"][h], grads["none"][h])
        assert torch.equal(grads["half"][h], 0.5 * grads["none"][h])


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: ResNet-18, 2 x 64 x 64, 6 classes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_model_dice_train_step_fp32():
    """one train step under CE + Dice against the oracle EMRT in float64 with the float64 Dice on top: the loss, and the whole gradient"""
    from emrt_amd.src.models.losses import get_loss_function
    from tests.test_gpu_model import build_pair, make_config
    x, labels = _model_inputs(44)
    ref, model = build_pair("resnet18", x, perturb=True, condition=0.1)
    cfg = make_config("resnet18")
    cfg.TRAIN.LOSS = "DiceCrossEntropyLoss"
    ref.double().train()
    out_r = ref(x.double())
    loss_r = sum(w * R.dice_ce_terms(o, labels)["L"] for o, w in zip(out_r, HEAD_W))
    loss_r.backward()
    model.train()
    model.clear_gradients()
    loss = get_loss_function(cfg)(model(x.cuda()), labels.cuda())
    parts = [p.cpu() for p in loss.parts]
    loss.backward()
    torch.cuda.synchronize()
    cos = _cosine(model, ref)
    print("CE + Dice train loss %.6f vs oracle %.6f (main head: CE %.6f Dice %.6f), whole-gradient cosine %.6f" % (
        loss.item(), loss_r.item(), parts[0][1].item(), parts[0][2].item(), cos))
    assert abs(loss.item() - loss_r.item()) < 2e-4 * max(1.0, abs(loss_r.item()))
    assert cos > 0.999


# (last in the file: a loss that synchronised or allocated under capture would fail here; it is not retried)
def test_model_dice_captured_bf16_step_equals_eager():
    """bf16, CE + Dice: three steps of TrainEngine captured from its first call (use_graph=True, warmup_eager=0) against the eager engine"""
    from emrt_amd.engine import TrainEngine
    from emrt_amd.src.models import get_model
    from emrt_amd.src.models.losses import get_loss_function
    from emrt_amd.src.models.solver import get_optimizer, get_scheduler
    from tests.test_gpu_model import calibrated_oracle, make_config
    x, labels = _model_inputs(45)
    ref = calibrated_oracle("resnet18", x, seed=1, condition=0.1)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    xd, ld = x.cuda(), labels.cuda()
    runs = {}
    for mode in ("eager", "graph"):
        cfg = make_config("resnet18")
        cfg.TRAIN.LOSS = "DiceCrossEntropyLoss"
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
        runs[mode] = [eng.step(xd, ld).item() for _ in range(3)]
        torch.cuda.synchronize()
        if mode == "graph":
            assert eng.graph_a is not None and eng.calls == 3
    print("CE + Dice bf16 losses eager %s captured %s" % (runs["eager"], runs["graph"]))
    for a, b in zip(runs["eager"], runs["graph"]):
        assert math.isfinite(b) and abs(a - b) < 1e-3 * abs(a), (a, b)
