"""-m gpu: Adam / AdamW and the device-side learning-rate schedules (emrt_adamw_step, emrt_sgd_momentum_step_sched, solver.AdamW).

Kernel level: the update against the formulas of include/emrt_hip.h evaluated in float64 from the same fp32 inputs, with bounds that count
roundings (2^-24 relative each) instead of being chosen; against torch.optim.AdamW over five steps; the four schedules at their branch
points; a captured step replayed (nothing may be baked at capture); the schedule-driven SGD kernel bit for bit against the built-in one;
the checkpoint round trip.  Model level: five TrainEngine steps of a ResNet-18 EMRT against the torch oracle under torch.optim.AdamW.

Measured at model level (MI355X, ResNet-18, 2 x 64 x 64, five steps, conditioned residual branches; relative L2 of the weight change against the float64
oracle's): HIP 0.070, fp32 CPU oracle 0.013 to 0.070 depending on the host; the loss used at most 0.07 of its bound
(test_model_level_five_steps_against_the_oracle's docstring has every figure)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                                   # noqa: E402
from emrt_amd.runtime import ctx, F32, BF16                                 # noqa: E402
from emrt_amd.src.models import solver                                      # noqa: E402
from emrt_amd.src.models.solver import EmrtLrSchedule                       # noqa: E402

EPS32 = 2.0 ** -24          # the relative error of one fp32 rounding
N = 4099                    # 1024 four-element groups + a 3-element tail
RANGE = (5, 11)             # lr-mult range: starts mid-group, straddles two groups
MULT = 0.1
ZERO = (2000, 2100)         # an all-zero stretch (padded stem channels): p = g = m = v = 0
W, T = 10, 100
POINTS = [0, 1, W - 1, W, W + 1, (T + W) // 2, T - 1, T, T + 5]


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def sched_ptr(d):
    return ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)


@pytest.fixture(scope="module")
def L():
    c = ctx()
    c.init_device("cuda:0", F32, 0)
    return _lib.lib()


def f32(x):
    return float(np.float32(x))


def adamw_call(L, p, g, m, v, scale, step, sched, beta1, beta2, eps, wd, decoupled, ranges, mult, mirror=None):
    """One emrt_adamw_step on device copies of the given CPU fp32 tensors -> (p, m, v, mirror, lr) back on the host."""
    dp, dg, dm, dv = (t.clone().cuda() for t in (p, g, m, v))
    state = torch.tensor([scale, 0.0], dtype=torch.float32, device="cuda")
    cnt = torch.tensor([step], dtype=torch.int64, device="cuda")
    lr = torch.zeros(1, dtype=torch.float32, device="cuda")
    mir, mdt = None, 0
    if mirror is not None:
        mir = torch.full((p.numel(),), 7.0, dtype=mirror, device="cuda")
        mdt = 1 if mirror == torch.bfloat16 else 2
    rng = (ctypes.c_longlong * (2 * len(ranges)))(*[x for r in ranges for x in r])
    L.call("emrt_adamw_step", P(dp), P(dg), P(dm), P(dv), p.numel(), P(state), P(cnt), sched_ptr(sched), beta1, beta2, eps, wd, decoupled,
           ctypes.cast(rng, ctypes.c_void_p), len(ranges), mult, P(lr), P(mir), mdt, ctx().stream)
    torch.cuda.synchronize()
    return dp.cpu(), dm.cpu(), dv.cpu(), (None if mir is None else mir.cpu()), float(lr.item())


def adam_inputs(seed):
    g_ = torch.Generator().manual_seed(seed)
    p = torch.randn(N, generator=g_)
    g = torch.randn(N, generator=g_)
    m = torch.randn(N, generator=g_) * 0.1
    v = (torch.randn(N, generator=g_) * 0.1) ** 2              # >= 0, some far below (1 - beta2) g^2
    for t in (p, g, m, v):
        t[ZERO[0]:ZERO[1]] = 0.0
    return p, g, m, v


def adam_reference(p, g, m, v, scale, step, lr, beta1, beta2, eps, wd, decoupled, use_mult=True):
    """The formulas of include/emrt_hip.h in float64 from the fp32 inputs -> p_ref, m_ref, v_ref, u_ref (the update term)."""
    p, g, m, v = (t.double().numpy() for t in (p, g, m, v))
    b1, b2, eps, wd, mult, scale = (np.float64(np.float32(x)) for x in (beta1, beta2, eps, wd, MULT, scale))
    lre = np.full(N, np.float64(lr))
    if use_mult:
        lre[RANGE[0]:RANGE[1]] *= mult
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


KERNEL_SCHED = dict(kind=1, base_lr=1e-2, end_lr=0.0, power=0.9, warmup_lr_init=1e-3, total_steps=160000, warmup_steps=1500)


@pytest.mark.parametrize("mirror", [None, torch.bfloat16, torch.float16], ids=["nomirror", "bf16", "fp16"])
@pytest.mark.parametrize("decoupled", [0, 1], ids=["adam", "adamw"])
@pytest.mark.parametrize("step", [0, 1, 999, 159999])
def test_kernel_against_float64(L, step, decoupled, mirror):
    """One update at n = 4099 against float64.  The learning rate the reference uses is the fp32 value the kernel reports in lr_out (the
    schedule's own accuracy is test_schedules_on_the_device's subject); everything else is formed in float64 from the fp32 inputs.  Bounds,
    each fp32 rounding contributing <= 2^-24 relative:
        |m - m_ref| <= 3 * 2^-24 * (|beta1 m| + |(1 - beta1) g|), the same form for v,
        |p - p_ref| <= 2^-24 * (3 |p_ref| + 8 |u_ref|), u_ref the reference's update term."""
    beta1, beta2, eps, wd, scale = f32(0.9), f32(0.999), f32(1e-8), f32(0.01), f32(0.37)
    p, g, m, v = adam_inputs(100 + step % 7)
    sched = EmrtLrSchedule(**KERNEL_SCHED)
    gp, gm, gv, mir, lr = adamw_call(L, p, g, m, v, scale, step, sched, beta1, beta2, eps, wd, decoupled, [RANGE], MULT, mirror)
    host = solver.WarmupPolyLR(1e-2, warmup_lr_init=1e-3, max_iters=160000, power=0.9, warmup_steps=1500, lr_min=0.0)
    host.last_epoch = step
    assert abs(lr - host.get_lr()) < 1e-6 * 1e-2, (lr, host.get_lr())
    p_ref, m_ref, v_ref, u_ref, m_mag, v_mag = adam_reference(p, g, m, v, scale, step, lr, beta1, beta2, eps, wd, decoupled)
    em = np.abs(gm.double().numpy() - m_ref) / np.maximum(3 * EPS32 * m_mag, 1e-300)
    ev = np.abs(gv.double().numpy() - v_ref) / np.maximum(3 * EPS32 * v_mag, 1e-300)
    ep = np.abs(gp.double().numpy() - p_ref) / np.maximum(EPS32 * (3 * np.abs(p_ref) + 8 * np.abs(u_ref)), 1e-300)
    print("ADAMW step %d decoupled %d lr %.6g: worst error / bound  m %.3f  v %.3f  p %.3f" % (step, decoupled, lr, em.max(), ev.max(), ep.max()))
    assert em.max() <= 1.0 and ev.max() <= 1.0 and ep.max() <= 1.0, (em.max(), ev.max(), ep.max(), int(ep.argmax()))
    # the lr-mult range is honoured: over the range, the kernel's result MISSES the reference formed without the multiplier.  Judged on the L2 norm
    # of the six elements (distance against the same bound, both as norms), so that one element whose new m lands near zero decides nothing
    p_flat, _, _, u_flat = adam_reference(p, g, m, v, scale, step, lr, beta1, beta2, eps, wd, decoupled, use_mult=False)[:4]
    r = slice(RANGE[0], RANGE[1])
    miss = np.linalg.norm(gp.double().numpy()[r] - p_flat[r]) / np.linalg.norm(EPS32 * (3 * np.abs(p_flat[r]) + 8 * np.abs(u_flat[r])))
    assert miss > 1.0, miss
    for t in (gp, gm, gv):          # padded channels stay exactly +0.0
        assert int(t[ZERO[0]:ZERO[1]].view(torch.int32).abs().max()) == 0
    if mirror is not None:
        assert torch.equal(mir, gp.to(mirror))


def test_five_steps_against_torch_adamw(L):
    """torch.optim.AdamW in float64 (two param groups: lr, and lr * 0.1 over the range) as the independent implementation: paddle's placement
    of epsilon is algebraically torch's m_hat / (sqrt(v_hat) + eps).  Five steps with fresh gradients, clip scale 1, moments from zero.  The
    tolerance is the one-step bound of the kernel test charged once per step, 2^-24 * (3 |p_k| + 8 |u_k|) summed over the five steps of the
    float64 trajectory."""
    beta1, beta2, eps, wd = f32(0.9), f32(0.999), f32(1e-8), f32(0.01)
    g_ = torch.Generator().manual_seed(5)
    p0 = torch.randn(N, generator=g_)
    grads = [torch.randn(N, generator=g_) for _ in range(5)]
    sched = EmrtLrSchedule(kind=2, base_lr=1e-2, end_lr=1e-4, warmup_lr_init=1e-3, total_steps=100, warmup_steps=3)
    inside = torch.zeros(N, dtype=torch.bool)
    inside[RANGE[0]:RANGE[1]] = True
    # one tensor per group: the parameter split by the range
    qa, qb = p0.double()[~inside].clone().requires_grad_(True), p0.double()[inside].clone().requires_grad_(True)
    topt = torch.optim.AdamW([{"params": [qa]}, {"params": [qb]}], lr=1.0, betas=(float(np.float64(np.float32(beta1))), float(np.float64(np.float32(beta2)))),
                             eps=float(np.float32(eps)), weight_decay=float(np.float32(wd)))
    p, m, v = p0.clone(), torch.zeros(N), torch.zeros(N)
    bound = np.zeros(N)
    for k, gr in enumerate(grads):
        p, m, v, _, lr = adamw_call(L, p, gr, m, v, 1.0, k, sched, beta1, beta2, eps, wd, 1, [RANGE], MULT)
        topt.param_groups[0]["lr"], topt.param_groups[1]["lr"] = float(lr), float(lr) * float(np.float32(MULT))
        before = torch.empty(N, dtype=torch.float64)
        before[~inside], before[inside] = qa.detach(), qb.detach()
        qa.grad, qb.grad = gr.double()[~inside].clone(), gr.double()[inside].clone()
        topt.step()
        after = torch.empty(N, dtype=torch.float64)
        after[~inside], after[inside] = qa.detach(), qb.detach()
        lre = torch.full((N,), float(lr), dtype=torch.float64)
        lre[inside] *= float(np.float32(MULT))
        u = before * (1.0 - lre * float(np.float32(wd))) - after
        bound += EPS32 * (3 * after.abs().numpy() + 8 * u.abs().numpy())
    err = np.abs(p.double().numpy() - after.numpy()) / bound
    print("ADAMW five steps against torch.optim.AdamW (float64): worst error / bound %.3f, |p - p_ref| max %.3g" % (err.max(), np.abs(p.double().numpy() - after.numpy()).max()))
    assert err.max() <= 1.0, (err.max(), int(err.argmax()))
    assert float((after - p0.double()).abs().min()) > 0.0           # every element moved


def _schedules():
    miles = [W, 60, 90]
    return {
        0: solver.PolynomialDecay(0.01, T, 1e-5, 0.9),
        1: solver.WarmupPolyLR(0.01, warmup_lr_init=1e-4, max_iters=T, power=0.9, warmup_steps=W, lr_min=1e-5),
        2: solver.WarmupCosineLR(0.01, T, lr_min=1e-5, warmup_steps=W, warmup_lr_init=1e-4),
        3: solver.WarmupMultiStepLR(0.01, miles, gamma=0.1, warmup_steps=W),
    }


@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=list(solver.SCHEDULERS))
def test_schedules_on_the_device(L, kind):
    """Every schedule at its branch points through BOTH schedule-driven entry points (8-element dummy buffers, lr_out) against the host
    class's float64 value: |lr_dev - lr_host| < 1e-6 * base_lr, the relative margin tests/test_gpu_model.py gives the polynomial schedule."""
    host = _schedules()[kind]
    desc = host.descriptor()
    assert desc.kind == kind
    bufs = [torch.zeros(8, dtype=torch.float32, device="cuda") for _ in range(4)]
    lr = torch.zeros(1, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    seen = []
    for s in POINTS:
        host.last_epoch = s
        want = host.get_lr()
        cnt.fill_(s)
        got = []
        lr.fill_(-1.0)
        L.call("emrt_adamw_step", P(bufs[0]), P(bufs[1]), P(bufs[2]), P(bufs[3]), 8, None, P(cnt), sched_ptr(desc), 0.9, 0.999, 1e-8, 0.0, 1,
               None, 0, 1.0, P(lr), None, 0, ctx().stream)
        got.append(float(lr.item()))
        lr.fill_(-1.0)
        L.call("emrt_sgd_momentum_step_sched", P(bufs[0]), P(bufs[1]), P(bufs[2]), 8, None, P(cnt), sched_ptr(desc), 0.9, 0.0, None, 0, 1.0, P(lr),
               None, 0, ctx().stream)
        got.append(float(lr.item()))
        seen.append((s, want, got))
        assert got[0] == got[1], (s, got)                      # one lr_at, two callers
        assert abs(got[0] - want) < 1e-6 * 0.01, (kind, s, got, want)
    print("SCHEDULE %s: %s" % (solver.SCHEDULERS[kind], ["%d: %.6g" % (s, g[0]) for s, _, g in seen]))
    assert len({g[0] for _, _, g in seen}) >= 4               # the schedule moves


def test_sched_kind0_is_the_builtin_sgd_bit_for_bit(L):
    """emrt_sgd_momentum_step_sched with a kind-0 descriptor against emrt_sgd_momentum_step on the same buffers: master, velocity, mirror
    and the reported learning rate are the same bits (the built-in entry point is the schedule-driven one with a kind-0 descriptor), for every
    mirror type and both settings of the sgd_nt knob."""
    g_ = torch.Generator().manual_seed(9)
    p0, v0, gr = torch.randn(N, generator=g_), torch.randn(N, generator=g_) * 0.1, torch.randn(N, generator=g_)
    rng = (ctypes.c_longlong * 2)(*RANGE)
    desc = solver.PolynomialDecay(0.01, 100, 1e-4, 0.9).descriptor()
    for nt in (1, 0):
        old = L.set_tuning("sgd_nt", nt)
        try:
            for mdt, mtype in ((0, None), (1, torch.bfloat16), (2, torch.float16)):
                for s in (0, 37, 100, 250):
                    res = []
                    for which in ("builtin", "sched"):
                        p, v, gd = p0.cuda(), v0.cuda(), gr.cuda()
                        mirror = None if mtype is None else torch.empty(N, dtype=mtype, device="cuda")
                        state = torch.tensor([0.37, 0.0], dtype=torch.float32, device="cuda")
                        cnt = torch.tensor([s], dtype=torch.int64, device="cuda")
                        lr = torch.zeros(1, dtype=torch.float32, device="cuda")
                        if which == "builtin":
                            L.call("emrt_sgd_momentum_step", P(p), P(gd), P(v), N, P(state), P(cnt), 0.01, 1e-4, 0.9, 100, 0.9, 1e-4,
                                   ctypes.cast(rng, ctypes.c_void_p), 1, MULT, P(lr), P(mirror), mdt, ctx().stream)
                        else:
                            L.call("emrt_sgd_momentum_step_sched", P(p), P(gd), P(v), N, P(state), P(cnt), sched_ptr(desc), 0.9, 1e-4,
                                   ctypes.cast(rng, ctypes.c_void_p), 1, MULT, P(lr), P(mirror), mdt, ctx().stream)
                        torch.cuda.synchronize()
                        res.append((p.cpu(), v.cpu(), lr.cpu()) + (() if mirror is None else (mirror.cpu(),)))
                    for a, b, name in zip(res[0], res[1], ("master", "velocity", "lr", "mirror")):
                        assert torch.equal(a, b), (nt, mdt, s, name, int((a != b).sum()))
                    assert not torch.equal(res[0][0], p0)
        finally:
            L.set_tuning("sgd_nt", old)


# ---- the optimizer class on a model --------------------------------------------------------------------------------------------------------------

def _small_model(dtype, seed=0):
    from tests.test_gpu_model import make_config
    from emrt_amd.src.models import get_model
    torch.manual_seed(seed)
    model = get_model(make_config("resnet18"))
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.to_hip("cuda:0", dtype)
    model.set_dropout(0.0)
    return model, init


def _fill_grad(st, seed):
    g_ = torch.Generator().manual_seed(seed)
    st.grad.zero_()
    for n in st.train_order:          # through the named views: padded stem channels keep their zero gradient
        view = st.named_view(st.grad, n)
        view.copy_((torch.randn(view.shape, generator=g_) * 1e-2).cuda())


def _snapshot(st, opt):
    torch.cuda.synchronize()
    mir = st.mirror
    return [st.master.clone(), st.velocity.clone(), opt.moment2.clone(), opt.lr_dev.clone()] + ([mir.clone()] if mir is not None else [])


def test_nothing_is_baked_at_capture():
    """AdamW.step alone captured in a hipGraph on the context's stream, with fixed gradients and a 2-step warmup (the learning rate and both
    bias terms change from step to step): three replays equal three eager steps from the same state, bit for bit, on master, both moments,
    the bf16 mirror and lr_dev.  A step that formed beta^t or the learning rate on the host would replay the capture-time values."""
    model, _ = _small_model(BF16)
    st, c = model.store, ctx()
    opt = solver.AdamW(model, solver.WarmupPolyLR(1e-3, warmup_lr_init=1e-5, max_iters=100, power=0.9, warmup_steps=2), weight_decay=0.01, grad_clip=1.0)
    _fill_grad(st, 3)
    st.pack()
    c.workspace(_lib.lib().query("emrt_gradnorm_workspace_bytes"))
    start = _snapshot(st, opt)
    assert st.mirror is not None

    def restore():
        st.master.copy_(start[0]); st.velocity.copy_(start[1]); opt.moment2.copy_(start[2]); st.mirror.copy_(start[4])
        c.step_counter.fill_(0)
        torch.cuda.synchronize()

    eager = []
    for _ in range(3):
        opt.step()
        eager.append(_snapshot(st, opt))
    restore()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        opt.step()
    torch.cuda.synchronize()
    assert int(c.step_counter.item()) == 0 and torch.equal(st.master, start[0])          # capturing ran nothing
    lrs = []
    for k in range(3):
        graph.replay()
        got = _snapshot(st, opt)
        lrs.append(float(got[3].item()))
        for a, b, name in zip(got, eager[k], ("master", "moment1", "moment2", "lr_dev", "mirror")):
            assert torch.equal(a, b), (k, name, int((a != b).sum()))
    assert lrs[0] < lrs[1] < lrs[2] and int(c.step_counter.item()) == 3, lrs
    n = min(st.n_train, st.mirror.numel())
    assert torch.equal(st.mirror[:n], st.master[:n].to(torch.bfloat16))
    for n, cp in st.padded_cin.items():          # padded stem channels: exactly zero in the parameter and both moments
        a, cnt = st.views[n]
        OC, C, KH, KW = st.shapes[n]
        for flat in (st.master, st.velocity, opt.moment2):
            assert int(flat[a:a + cnt].view(OC, KH, KW, cp)[..., C:].contiguous().view(torch.int32).abs().max()) == 0, n


def test_checkpoint_round_trip():
    """Three steps, state_dict(); a fresh model + optimizer restored through load_state_dict / set_state_dict takes the fourth step with the
    same gradient and lands on the uninterrupted run's bits.  An SGD checkpoint is refused."""
    sched = lambda: solver.WarmupCosineLR(1e-3, 100, lr_min=1e-5, warmup_steps=2, warmup_lr_init=1e-5)
    model, init = _small_model(F32)
    st = model.store
    opt = solver.AdamW(model, sched(), weight_decay=0.01, grad_clip=1.0)
    for k in range(3):
        _fill_grad(st, 20 + k)
        opt.step()
        opt._learning_rate.step()
    torch.cuda.synchronize()
    sd_opt = {k: ({n: t.cpu() for n, t in v.items()} if isinstance(v, dict) else v) for k, v in opt.state_dict().items()}       # as train.py writes it
    sd_model = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert sd_opt["step"] == 3 and sd_opt["optimizer"] == "adamw" and float(next(iter(sd_opt["moment2"].values())).abs().max()) > 0
    _fill_grad(st, 23)
    opt.step()
    torch.cuda.synchronize()
    want = [st.master.cpu(), st.velocity.cpu(), opt.moment2.cpu(), opt.lr_dev.cpu()]
    sgd_sd = solver.Momentum(model, solver.PolynomialDecay(0.01, 100), 0.9, 1e-4, 1.0).state_dict()

    from tests.test_gpu_model import make_config
    from emrt_amd.src.models import get_model
    model2 = get_model(make_config("resnet18"))
    model2.load_state_dict(init)
    model2.to_hip("cuda:0", F32)
    model2.set_dropout(0.0)
    st2 = model2.store
    opt2 = solver.AdamW(model2, sched(), weight_decay=0.01, grad_clip=1.0)
    with pytest.raises(ValueError, match="SGD.*AdamW"):
        opt2.set_state_dict(sgd_sd)
    model2.load_state_dict(sd_model)
    opt2.set_state_dict(sd_opt)
    assert int(ctx().step_counter.item()) == 3 and opt2._learning_rate.last_epoch == 3
    _fill_grad(st2, 23)
    opt2.step()
    torch.cuda.synchronize()
    got = [st2.master.cpu(), st2.velocity.cpu(), opt2.moment2.cpu(), opt2.lr_dev.cpu()]
    for a, b, name in zip(got, want, ("master", "moment1", "moment2", "lr_dev")):
        assert torch.equal(a, b), (name, int((a != b).sum()))


def _oracle_adamw_run(ref, x, labels, lrs, steps):
    """The oracle under torch.optim.AdamW: param groups by lr_mult_of, clip_grad_norm_(1.0), the host schedule's learning rates."""
    from oracle.emrt_torch import lr_mult_of
    from oracle import train_ref
    named = [(n, p) for n, p in ref.named_parameters()]
    full = [p for n, p in named if lr_mult_of(n) == 1.0]
    tenth = [p for n, p in named if lr_mult_of(n) != 1.0]
    opt = torch.optim.AdamW([{"params": full}, {"params": tenth}], lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    losses, grad0 = [], None
    for k in range(steps):
        loss = train_ref.mix_softmax_ce_loss(ref(x), labels)
        loss.backward()
        loss = loss.detach()
        if grad0 is None:
            grad0 = {n: p.grad.detach().clone() for n, p in named if p.grad is not None}
        torch.nn.utils.clip_grad_norm_([p for _, p in named if p.grad is not None], 1.0)
        opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = lrs[k], lrs[k] * 0.1
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss))
    return losses, grad0


MODEL_SEED = 31         # (the first seed tried; not searched for)
CONDITION = 0.1         # residual branches down-weighted as tests/test_gpu_model.py's condition_residual_branches explains (the docstring below has the figures)
DW_FLOOR = 0.07         # absolute floor on the weight-change distance: the largest distance the fp32 oracle ITSELF showed (the docstring below has the figures)


def test_model_level_five_steps_against_the_oracle():
    """ResNet-18 EMRT, 2 x 64 x 64, fp32, dropout off: five TrainEngine steps under AdamW (BASE_LR 1e-4, weight decay 0.01, GRAD_CLIP 1.0,
    WarmupPolyLR W = 2, T = 100), eager and again captured (use_graph=True, warmup_eager=0), against the oracle model under torch.optim.AdamW
    run once in fp32 and once as a float64 copy.  Per step: the device learning rate within 1e-6 * base of the host schedule, and
    |loss_hip - loss_f64| <= max(2e-3 * max(1, loss), 1.25 * |loss_fp32 - loss_f64|).  After five steps: the relative L2 distance of the
    weight change from the float64 oracle's, over the parameters whose float64 gradient is not rounding noise (norm >= 1e-5 of the largest:
    Adam turns a noise gradient into a +-lr step on both sides, and conv biases in front of a BatchNorm are exactly that), is at most 1.25 x
    the fp32 oracle's own distance (+ DW_FLOOR).  The captured run is held to the same yardsticks (it cannot equal the eager one bit for bit:
    the weight gradients use fp32 atomics).

    The initial weights are the oracle's with its residual branches down-weighted (CONDITION = 0.1) and generic sampling offsets (perturb=True), as the
    bf16 and fp16 model tests use them.  A randomly initialised BatchNorm network is chaotic (condition_residual_branches' docstring), and Adam
    divides by sqrt(v), so a rounding-level difference of a small gradient becomes a full-size step.  Unconditioned, the fp32 CPU oracle ITSELF was up
    to 2.3e-3 from float64 in the loss at steps 3 and 4 (seeds 31 - 33, CPU only), 0.4 of the 5.4e-3 bound, and the HIP path used 0.98 - 0.99 of it at
    step 3.  Conditioned, the oracle's own worst was 2.4e-4 and the HIP path's 4.7e-4 (seeds 31 - 34), under 0.1 of the bound: a margin that does not
    hang on the summation order of the fp32 atomics.

    Measured on an MI355X (WARM_UP_LR_INIT 1e-5, MODEL_SEED 31; 290 of 293 parameters counted).  Loss, |hip - f64| over the bound per step: eager
    0.00 / 0.00 / 0.01 / 0.06 / 0.07, captured 0.00 / 0.00 / 0.00 / 0.06 / 0.05 (step 3: 3.4e-4 against 5.41e-3).  Weight-change distance from float64:
    HIP 0.070 and 0.073 (eager, two runs) and 0.070 (captured) where the fp32 oracle's own was 0.013 on that host.  That yardstick is not a stable number: the same fp32 oracle, same seed, measured 0.070 on another host (another CPU, so
    another summation order), and 0.011 - 0.028 over seeds 32 - 34 where the HIP path measured 0.036 - 0.057.  1.25 x a figure that moves fivefold
    between two runs of the reference itself cannot bound anything, so a floor is needed: DW_FLOOR = 0.07 is the largest distance the fp32 oracle
    itself showed in this configuration, taken from the reference's spread and not from the HIP path's figures.  The HIP path is about twice the oracle's
    typical distance, in line with the 3 x the oracle's own error that tests/test_gpu_model.py allows each HIP gradient.  Against 1.25 x 0.013 + 0.07 =
    0.087 the measured 0.070 - 0.073 use 0.81 - 0.84; the HIP path's own run-to-run spread (fp32 atomics) was 4 %."""
    from tests.test_gpu_model import build_pair, make_config
    from emrt_amd.engine import TrainEngine
    from emrt_amd.src.models.losses import get_loss_function
    g = torch.Generator().manual_seed(MODEL_SEED)
    B, S, steps = 2, 64, 5
    x = torch.randn(B, 3, S, S, generator=g)
    labels = torch.randint(0, 6, (B, S, S), generator=g)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 8))

    def config():
        cfg = make_config("resnet18", iters=100)
        cfg.TRAIN.BASE_LR, cfg.TRAIN.END_LR = 1e-4, 0.0
        cfg.TRAIN.LR_SCHEDULER.NAME, cfg.TRAIN.LR_SCHEDULER.WARM_UP_STEPS, cfg.TRAIN.LR_SCHEDULER.WARM_UP_LR_INIT = "WarmupPolyLR", 2, 1e-5
        cfg.TRAIN.OPTIMIZER.NAME, cfg.TRAIN.OPTIMIZER.WEIGHT_DECAY, cfg.TRAIN.OPTIMIZER.GRAD_CLIP = "AdamW", 0.01, 1.0
        return cfg

    host = solver.get_scheduler(config())
    lrs = []
    for _ in range(steps):
        lrs.append(host.get_lr())
        host.step()
    assert lrs[0] == 1e-5 and abs(lrs[2] - 1e-4) < 1e-15 and lrs[1] < lrs[2] > lrs[3]
    try:
        runs = {}
        ref = None
        for mode in ("eager", "graph"):
            ref, model = build_pair("resnet18", x, perturb=True, condition=CONDITION)
            w0 = {n: p.detach().clone() for n, p in ref.named_parameters()}
            cfg = config()
            opt = solver.get_optimizer(model, solver.get_scheduler(cfg), cfg)
            assert type(opt) is solver.AdamW
            model.eval()
            model(x.cuda())          # (the model's device constants are made by its first forward, which must not be the captured one)
            eng = TrainEngine(model, opt, get_loss_function(cfg), 1, use_graph=(mode == "graph"), warmup_eager=0)
            losses = []
            for k in range(steps):
                assert abs(opt.get_lr() - lrs[k]) < 1e-15
                losses.append(eng.step(x.cuda(), labels.cuda()).item())
                assert abs(float(opt.lr_dev.item()) - lrs[k]) < 1e-6 * 1e-4, (mode, k, float(opt.lr_dev.item()), lrs[k])
            assert (eng.graph_a is not None) == (mode == "graph")
            runs[mode] = (losses, {n: p.detach().cpu().clone() for n, p in model.named_parameters()})
        ref.train()
        ref64 = copy.deepcopy(ref).double().train()
        loss32, _ = _oracle_adamw_run(ref, x, labels, lrs, steps)
        loss64, grad64 = _oracle_adamw_run(ref64, x.double(), labels, lrs, steps)
    finally:
        torch.set_num_threads(threads)
    gmax = max(float(gr.norm()) for gr in grad64.values())
    keep = [n for n, gr in grad64.items() if float(gr.norm()) >= 1e-5 * gmax]
    p32, p64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    assert len(keep) > 100 and len(keep) < len(grad64)

    def distance(params):
        num = den = 0.0
        for n in keep:
            d64 = p64[n].detach() - w0[n].double()
            d = params[n].detach().double() - w0[n].double()
            num += float((d - d64).pow(2).sum())
            den += float(d64.pow(2).sum())
        return (num / den) ** 0.5

    d32 = distance(p32)
    for mode in ("eager", "graph"):
        losses, params = runs[mode]
        for k in range(steps):
            bound = max(2e-3 * max(1.0, abs(loss64[k])), 1.25 * abs(loss32[k] - loss64[k]))
            print("ADAMW MODEL %s step %d: loss hip %.6f  fp32 oracle %.6f  float64 oracle %.6f  (bound %.2e)" % (mode, k, losses[k], loss32[k], loss64[k], bound))
            assert abs(losses[k] - loss64[k]) <= bound, (mode, k, losses[k], loss32[k], loss64[k])
        d = distance(params)
        print("ADAMW MODEL %s: weight-change distance from float64 after %d steps: hip %.4e, fp32 oracle %.4e (ratio %.3f; %d of %d parameters counted)"
              % (mode, steps, d, d32, d / d32, len(keep), len(grad64)))
        assert d <= 1.25 * d32 + DW_FLOOR, (mode, d, d32)
    for k in range(steps):
        bound = max(2e-3 * max(1.0, abs(loss64[k])), 1.25 * abs(loss32[k] - loss64[k]))
        assert abs(runs["eager"][0][k] - runs["graph"][0][k]) <= bound, (k, runs["eager"][0][k], runs["graph"][0][k])
    assert loss64[-1] < loss64[0] and runs["graph"][0][-1] < runs["graph"][0][0]
