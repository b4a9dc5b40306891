"""CPU: the solver's host layer -- the four learning-rate schedules against independent values, the optimizer / schedule factories from the
shipped AdamW yaml, the launch sequences of one optimizer step on the recording stand-in (tests/fake_abi.py), and the argument refusals of
emrt_adamw_step / emrt_sgd_momentum_step_sched / emrt_sgd_momentum_step (and the null-pointer refusals of the loss entry points), which run on the host before anything is launched (no GPU here)."""
import argparse
import ctypes
import os

import pytest
import torch

from tests import fake_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam_adamw.yaml")

W, T = 10, 100
POINTS = [0, 1, W - 1, W, W + 1, (T + W) // 2, T - 1, T, T + 5]
BASE, END, INIT = 0.01, 1e-5, 1e-4
TOL = 1e-15             # absolute, as tests/test_golden_cpu.py holds PolynomialDecay


def _at(sched, s):
    sched.last_epoch = s
    return sched.get_lr()


def _torch_closed_form(make, s):
    """Closed-form value of a torch.optim.lr_scheduler at epoch s (base lr BASE)."""
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=BASE)
    sch = make(opt)
    sch.last_epoch = s
    return sch._get_closed_form_lr()[0]


def test_warmup_poly_known_answers():
    from emrt_amd.src.models.solver import WarmupPolyLR
    # power 1: every value can be written down.  ramp INIT + (BASE - INIT) * s / W; decay INIT + (BASE - INIT) * (1 - (s - W) / (T - W))
    lin = WarmupPolyLR(BASE, warmup_lr_init=INIT, max_iters=T, power=1.0, warmup_steps=W, lr_min=END)
    expect = {0: 1e-4, 1: 1e-4 + 0.0099 * 0.1, W - 1: 1e-4 + 0.0099 * 0.9, W: 0.01, W + 1: 1e-4 + 0.0099 * (1 - 1 / 90),
              (T + W) // 2: 1e-4 + 0.0099 * 0.5, T - 1: 1e-4 + 0.0099 * (1 - 89 / 90),
              T: 1e-4,             # quirk: the decay's floor is warmup_lr_init, not lr_min
              T + 5: 1e-5}         # past the end (the reference's pow() is complex there): lr_min
    assert sorted(expect) == sorted(POINTS)
    for s, e in expect.items():
        assert abs(_at(lin, s) - e) <= TOL, (s, _at(lin, s), e)
    # power 0.9 after the warmup: the formula written out once more here, not imported
    pw = WarmupPolyLR(BASE, warmup_lr_init=INIT, max_iters=T, power=0.9, warmup_steps=W, lr_min=END)
    for s in POINTS:
        if s < W:
            e = INIT + (BASE - INIT) * (s / W)
        elif s > T:
            e = END
        else:
            e = INIT + (BASE - INIT) * pow(1 - (s - W) / (T - W), 0.9)
        assert abs(_at(pw, s) - e) <= TOL, (s, _at(pw, s), e)
    # a value at or below lr_min becomes lr_min, in both branches
    low = WarmupPolyLR(BASE, warmup_lr_init=0.0, max_iters=T, power=1.0, warmup_steps=W, lr_min=2e-3)
    assert _at(low, 1) == 2e-3 and abs(_at(low, 3) - 0.003) <= TOL and _at(low, W) == 0.01 and _at(low, T - 1) == 2e-3
    assert _at(lin, W - 1) < _at(lin, W) > _at(lin, W + 1)


def test_warmup_cosine_against_torch_closed_form():
    from emrt_amd.src.models.solver import WarmupCosineLR
    sch = WarmupCosineLR(BASE, T, lr_min=END, warmup_steps=W, warmup_lr_init=INIT)
    for s in POINTS:
        if s < W:
            e = INIT + s * (BASE - INIT) / W              # 1e-4, 1.09e-3, ..., 9.01e-3
        else:                                             # the reference restarts the cosine every T steps; torch's closed form at s mod T
            e = _torch_closed_form(lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=T, eta_min=END), s % T)
        assert abs(_at(sch, s) - e) <= TOL, (s, _at(sch, s), e)
    assert abs(_at(sch, 1) - 1.09e-3) <= TOL and abs(_at(sch, W - 1) - 9.01e-3) <= TOL
    assert abs(_at(sch, T) - BASE) <= TOL                  # restart
    assert abs(_at(sch, T // 2) - (END + 0.5 * (BASE - END))) <= TOL


def test_warmup_multistep_against_torch():
    from emrt_amd.src.models.solver import WarmupMultiStepLR
    miles = [W, 60, 90]                                    # milestones[0] == W: the quirk below is visible
    sch = WarmupMultiStepLR(BASE, miles, gamma=0.1, warmup_steps=W)
    for s in POINTS:
        if s <= W:
            e = BASE * s / W
        else:
            e = _torch_closed_form(lambda o: torch.optim.lr_scheduler.MultiStepLR(o, milestones=miles, gamma=0.1), s)
        assert abs(_at(sch, s) - e) <= TOL, (s, _at(sch, s), e)
    # quirk: the ramp holds for s <= W, so at s == W == milestones[0] the rate is base, not base * gamma
    assert _at(sch, W) == BASE and abs(_at(sch, W + 1) - BASE * 0.1) <= TOL and abs(_at(sch, T + 5) - BASE * 1e-3) <= TOL


def test_polynomial_decay_descriptor_and_step():
    from emrt_amd.src.models.solver import EmrtLrSchedule, PolynomialDecay, WarmupMultiStepLR
    d = PolynomialDecay(0.01, 100, 1e-4, 0.9).descriptor()
    assert isinstance(d, EmrtLrSchedule) and (d.kind, d.total_steps, d.warmup_steps, d.nmilestones) == (0, 100, 0, 0)
    assert d.base_lr == pytest.approx(0.01) and d.end_lr == pytest.approx(1e-4) and d.power == pytest.approx(0.9)
    d = WarmupMultiStepLR(0.01, [30, 60, 90], 0.5, 7).descriptor()
    assert (d.kind, d.warmup_steps, d.nmilestones, list(d.milestones)[:4]) == (3, 7, 3, [30, 60, 90, 0]) and d.gamma == 0.5
    # the struct's layout is the C one (include/emrt_hip.h): 6 x 4 bytes, 2 x int64, int + padding, 16 x int64
    assert ctypes.sizeof(EmrtLrSchedule) == 24 + 16 + 8 + 128 and EmrtLrSchedule.milestones.offset == 48
    s = WarmupMultiStepLR(0.01, [30], 0.5, 7)
    s.step()
    s.step()
    assert s.last_epoch == 2


def _cfg():
    from emrt_amd.config import get_config, update_config
    return update_config(get_config(), argparse.Namespace(cfg=YAML))


def test_shipped_yaml_and_scheduler_factory():
    from emrt_amd.src.models import solver
    cfg = _cfg()
    assert cfg.TRAIN.OPTIMIZER.NAME == "AdamW" and cfg.TRAIN.LR_SCHEDULER.NAME == "WarmupPolyLR" and cfg.TRAIN.BASE_LR == 6e-5
    assert cfg.MODEL.ENCODER.TYPE == "resnet50" and cfg.TRAIN.OPTIMIZER.GRAD_CLIP == 1.0 and cfg.TRAIN.OPTIMIZER.WEIGHT_DECAY == 0.01
    sch = solver.get_scheduler(cfg)
    assert isinstance(sch, solver.WarmupPolyLR) and (sch.max_iters, sch.warmup_steps, sch.power) == (160000, 1500, 1.0)
    assert sch.get_lr() == 1e-6
    cfg.TRAIN.LR_SCHEDULER.MILESTONES = [40000, 80000]
    for name, cls in (("PolynomialDecay", solver.PolynomialDecay), ("WarmupPolyLR", solver.WarmupPolyLR), ("WarmupCosineLR", solver.WarmupCosineLR),
                      ("WarmupMultiStepLR", solver.WarmupMultiStepLR)):
        cfg.TRAIN.LR_SCHEDULER.NAME = name
        s = solver.get_scheduler(cfg)
        assert type(s) is cls and s.descriptor().kind == solver.SCHEDULERS.index(name)
    cfg.TRAIN.LR_SCHEDULER.NAME = "CosineAnnealing"
    with pytest.raises(NotImplementedError, match="WarmupCosineLR"):
        solver.get_scheduler(cfg)


def test_train_shortens_only_the_warmup_that_would_refuse(capsys):
    """train.py --iters N: WarmupPolyLR refuses max_iters <= warmup_steps, so its warmup shrinks to N // 4 with a log line; every other
    schedule (WarmupCosineLR accepts W >= T, as the reference does) and every run longer than the warmup is left as the yaml says."""
    from emrt_amd.src.models import solver
    from emrt_amd.train import shorten_warmup
    cfg = _cfg()
    cfg.TRAIN.ITERS = 20
    assert shorten_warmup(cfg, 20) and cfg.TRAIN.LR_SCHEDULER.WARM_UP_STEPS == 5
    assert "warming up over 5 steps" in capsys.readouterr().out
    sch = solver.get_scheduler(cfg)
    assert (sch.max_iters, sch.warmup_steps) == (20, 5)
    cfg = _cfg()
    assert not shorten_warmup(cfg, 1501) and cfg.TRAIN.LR_SCHEDULER.WARM_UP_STEPS == 1500
    assert shorten_warmup(cfg, 1500, verbose=False) and cfg.TRAIN.LR_SCHEDULER.WARM_UP_STEPS == 375
    assert shorten_warmup(_cfg(), 1, verbose=False)
    for name in ("WarmupCosineLR", "WarmupMultiStepLR", "PolynomialDecay"):
        cfg = _cfg()
        cfg.TRAIN.LR_SCHEDULER.NAME = name
        assert not shorten_warmup(cfg, 20) and cfg.TRAIN.LR_SCHEDULER.WARM_UP_STEPS == 1500
    assert "warming up" not in capsys.readouterr().out


def test_scheduler_constructor_refusals():
    from emrt_amd.src.models.solver import WarmupCosineLR, WarmupMultiStepLR, WarmupPolyLR
    with pytest.raises(ValueError, match="lr_min"):                      # the reference asserts base_lr > end_lr
        WarmupPolyLR(1e-4, max_iters=100, warmup_steps=5, lr_min=1e-4)
    with pytest.raises(ValueError, match="warmup_steps"):                # N = T - W = 0 divides by zero
        WarmupPolyLR(1e-4, max_iters=100, warmup_steps=100)
    with pytest.raises(ValueError, match="at least 1"):                  # the reference divides by zero in get_lr
        WarmupMultiStepLR(0.01, [30, 60], warmup_steps=0)
    with pytest.raises(ValueError, match="milestones\\[0\\]"):
        WarmupMultiStepLR(0.01, [30, 60], warmup_steps=31)
    with pytest.raises(ValueError, match="increasing"):
        WarmupMultiStepLR(0.01, [60, 30], warmup_steps=5)
    with pytest.raises(ValueError, match="1..16"):
        WarmupMultiStepLR(0.01, list(range(10, 27)), warmup_steps=5)
    with pytest.raises(ValueError):
        WarmupCosineLR(0.01, 0)


@pytest.fixture(scope="module")
def placed():
    """A ResNet-18 EMRT laid out in CPU buffers behind the recording C-ABI."""
    from emrt_amd import nn as hnn
    from emrt_amd.runtime import ctx, F32
    from emrt_amd.src.models.emrt import EMRT, NOGRAD_PARAMS
    f = fake_abi.install()
    torch.manual_seed(0)
    m = EMRT(num_classes=6, backbone="resnet18")
    m.store = hnn.ParamStore(m, ctx().device, F32, nograd_names=NOGRAD_PARAMS, fused_groups=m.fused_groups(), lr_mult_names=m.lr_mult_names())
    hnn.bind_all(m, m.store)
    m.store.pack()
    yield f, m
    fake_abi.uninstall()


def _step_names(f, opt):
    f.calls.clear()
    opt.step()
    return [n for n, _ in f.calls]


def test_optimizer_factory_from_the_shipped_yaml(placed, capsys):
    from emrt_amd.src.models import solver
    f, m = placed
    cfg = _cfg()
    opt = solver.get_optimizer(m, solver.get_scheduler(cfg), cfg)
    assert type(opt) is solver.AdamW and opt.decoupled and (opt.beta1, opt.beta2, opt.epsilon, opt.weight_decay, opt.grad_clip) == (0.9, 0.999, 1e-8, 0.01, 1.0)
    assert opt.moment2.shape == m.store.velocity.shape and opt.moment2.dtype == torch.float32
    assert _step_names(f, opt) == ["emrt_grad_clip_scale", "emrt_adamw_step", "emrt_counter_add"]
    args = dict(zip([a for _, a in f.protos["emrt_adamw_step"][1]], f.calls[1][1]))
    assert args["n"] == m.store.n_train and args["decoupled"] == 1 and args["nranges"] == len(m.store.lr_ranges) == 14
    assert args["range_mult"] == 0.1 and args["clip_state"] is not None and args["mirror"] is None      # fp32 store: no mirror
    # adam: paddle's default betas whatever BETAS says, and no clip call (the reference does not hand its clip object to optim.Adam)
    cfg.TRAIN.OPTIMIZER.NAME = "adam"
    cfg.TRAIN.OPTIMIZER.BETAS = [0.8, 0.9]
    capsys.readouterr()
    opt = solver.get_optimizer(m, solver.get_scheduler(cfg), cfg)
    out = capsys.readouterr().out
    assert "GRAD_CLIP" in out and "BETAS (0.8, 0.9) are not used" in out
    cfg.TRAIN.OPTIMIZER.GRAD_CLIP = None          # the BETAS note does not depend on the clip
    solver.get_optimizer(m, solver.get_scheduler(cfg), cfg)
    out = capsys.readouterr().out
    assert "GRAD_CLIP" not in out and "BETAS (0.8, 0.9) are not used" in out
    cfg.TRAIN.OPTIMIZER.BETAS = [0.9, 0.999]
    solver.get_optimizer(m, solver.get_scheduler(cfg), cfg)
    assert capsys.readouterr().out == ""
    cfg.TRAIN.OPTIMIZER.GRAD_CLIP = 1.0
    assert type(opt) is solver.AdamW and not opt.decoupled and (opt.beta1, opt.beta2, opt.grad_clip) == (0.9, 0.999, None)
    assert _step_names(f, opt) == ["emrt_adamw_step", "emrt_counter_add"]
    args = dict(zip([a for _, a in f.protos["emrt_adamw_step"][1]], f.calls[0][1]))
    assert args["decoupled"] == 0 and args["clip_state"] is None
    # every optimizer name with every schedule name
    for oname in ("SGD", "sgd", "Adam", "AdamW"):
        for sname in solver.SCHEDULERS:
            cfg.TRAIN.OPTIMIZER.NAME, cfg.TRAIN.LR_SCHEDULER.NAME = oname, sname
            cfg.TRAIN.LR_SCHEDULER.MILESTONES = [40000, 80000]
            o = solver.get_optimizer(m, solver.get_scheduler(cfg), cfg)
            assert type(o) is (solver.Momentum if oname.lower() == "sgd" else solver.AdamW)
            assert "emrt_counter_add" == _step_names(f, o)[-1]
    for oname in ("adadelta", "rmsprop", "RMSProp", "lamb"):
        cfg.TRAIN.OPTIMIZER.NAME = oname
        with pytest.raises(NotImplementedError, match="sgd, adam, adamw"):
            solver.get_optimizer(m, solver.get_scheduler(cfg), cfg)
    cfg.TRAIN.OPTIMIZER.NAME, cfg.TRAIN.OPTIMIZER.NESTEROV = "sgd", True
    with pytest.raises(NotImplementedError, match="adamw"):
        solver.get_optimizer(m, solver.get_scheduler(cfg), cfg)
    with pytest.raises(ValueError, match="betas"):
        solver.AdamW(m, solver.PolynomialDecay(0.01, 100), beta2=1.0)
    with pytest.raises(ValueError, match="epsilon"):
        solver.AdamW(m, solver.PolynomialDecay(0.01, 100), epsilon=0.0)


def test_sgd_launch_sequences(placed):
    from emrt_amd.src.models.solver import Momentum, PolynomialDecay, WarmupCosineLR
    f, m = placed
    # the shipped recipe: exactly the three calls it has always made
    assert _step_names(f, Momentum(m, PolynomialDecay(0.01, 100), 0.9, 1e-4, 1.0)) == ["emrt_grad_clip_scale", "emrt_sgd_momentum_step", "emrt_counter_add"]
    opt = Momentum(m, WarmupCosineLR(0.01, 100, warmup_steps=10), 0.9, 1e-4, 1.0)
    assert _step_names(f, opt) == ["emrt_grad_clip_scale", "emrt_sgd_momentum_step_sched", "emrt_counter_add"]
    args = dict(zip([a for _, a in f.protos["emrt_sgd_momentum_step_sched"][1]], f.calls[1][1]))
    assert args["sched"].value == ctypes.addressof(opt.sched_desc) and opt.sched_desc.kind == 2 and args["momentum"] == 0.9


def test_adamw_state_dict_on_the_host(placed):
    from emrt_amd.runtime import ctx
    from emrt_amd.src.models.solver import AdamW, Momentum, PolynomialDecay, WarmupPolyLR
    f, m = placed
    st = m.store
    opt = AdamW(m, WarmupPolyLR(1e-4, max_iters=100, warmup_steps=2), weight_decay=0.01, grad_clip=1.0)
    st.velocity.copy_(torch.randn(st.velocity.shape))
    opt.moment2.copy_(torch.rand(opt.moment2.shape))
    ctx().step_counter.fill_(7)
    sd = opt.state_dict()
    assert sd["optimizer"] == "adamw" and sd["format"] == "per-parameter" and sd["step"] == 7
    assert set(sd["moment1"]) == set(sd["moment2"]) == set(st.train_order)
    n0 = st.train_order[0]
    assert tuple(sd["moment2"][n0].shape) == tuple(st.shapes[n0])          # logical shape, not the padded flat layout
    m1, m2 = st.velocity.clone(), opt.moment2.clone()
    for n in st.padded_cin:               # what lies in the padded channels is not part of the file format
        assert sd["moment1"][n].shape[1] < st.padded_cin[n]
    st.velocity.zero_()
    opt.moment2.zero_()
    ctx().step_counter.fill_(0)
    opt.set_state_dict(sd)
    for n in st.train_order:
        assert torch.equal(st.named_view(st.velocity, n), st.named_view(m1, n)) and torch.equal(st.named_view(opt.moment2, n), st.named_view(m2, n))
    assert int(ctx().step_counter.item()) == 7 and opt._learning_rate.last_epoch == 7
    sgd = Momentum(m, PolynomialDecay(0.01, 100), 0.9, 1e-4, 1.0)
    with pytest.raises(ValueError, match="SGD.*AdamW"):
        opt.set_state_dict(sgd.state_dict())
    with pytest.raises(ValueError, match="AdamW.*SGD"):
        sgd.set_state_dict(sd)
    bad = {k: (dict(v) if isinstance(v, dict) else v) for k, v in sd.items()}
    del bad["moment2"][n0]
    with pytest.raises(KeyError, match="moment2"):
        opt.set_state_dict(bad)
    bad["moment2"][n0] = torch.zeros(3)
    with pytest.raises(ValueError, match="shape"):
        opt.set_state_dict(bad)
    st.velocity.zero_()
    ctx().step_counter.fill_(0)


# ---- argument refusals of the two entry points, on the real library (host checks only: the pointers are never dereferenced) ----------------------

@pytest.fixture(scope="module")
def real_lib():
    from emrt_amd import _lib, build_ext
    build_ext.build(verbose=False)
    saved = _lib._LIB
    _lib._LIB = None
    L = _lib.lib()
    yield L
    _lib._LIB = saved


def _sched(**kw):
    from emrt_amd.src.models.solver import EmrtLrSchedule
    f = dict(kind=1, base_lr=1e-4, end_lr=0.0, power=1.0, warmup_lr_init=0.0, gamma=0.1, total_steps=100, warmup_steps=10, nmilestones=0)
    f.update(kw)
    miles = f.pop("milestones", ())
    d = EmrtLrSchedule(**f)
    for i, v in enumerate(miles):
        d.milestones[i] = v
    return d


P_OK, P_ODD = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)       # "device pointers": aligned / misaligned, never read


def _adamw_args(**kw):
    a = dict(params=P_OK, grads=P_OK, moment1=P_OK, moment2=P_OK, n=64, clip_state=P_OK, step=P_OK, sched=_sched(), beta1=0.9, beta2=0.999,
             eps=1e-8, weight_decay=0.01, decoupled=1, ranges=None, nranges=0, range_mult=0.1, lr_out=None, mirror=None, mirror_dtype=0, stream=None)
    a.update(kw)
    return a


def _sgd_args(**kw):
    a = dict(params=P_OK, grads=P_OK, velocity=P_OK, n=64, clip_state=P_OK, step=P_OK, sched=_sched(), momentum=0.9, weight_decay=1e-4,
             ranges=None, nranges=0, range_mult=0.1, lr_out=None, mirror=None, mirror_dtype=0, stream=None)
    a.update(kw)
    return a


SCHED_REFUSALS = [
    (dict(kind=4), "unknown schedule kind"),
    (dict(kind=-1), "unknown schedule kind"),
    (dict(kind=3, nmilestones=17), "0..16 milestones"),
    (dict(kind=3, nmilestones=3, milestones=(30, 60, 60)), "increasing"),
    (dict(kind=1, total_steps=10, warmup_steps=10), "total_steps > warmup_steps"),
    (dict(kind=3, warmup_steps=0, nmilestones=1, milestones=(30,)), "warmup_steps >= 1"),
    (dict(kind=0, total_steps=0), "total_steps must be positive"),
]
ADAMW_REFUSALS = [
    (dict(params=None), "null pointer"),
    (dict(moment2=None), "null pointer"),
    (dict(sched=None), "null schedule"),
    (dict(grads=P_ODD), "16-byte aligned"),
    (dict(moment2=P_ODD), "16-byte aligned"),
    (dict(mirror=P_ODD, mirror_dtype=1), "16-byte aligned"),
    (dict(mirror=P_OK, mirror_dtype=0), "mirror is bf16 or fp16"),
    (dict(beta1=1.0), "0 <= beta < 1"),
    (dict(beta1=-0.1), "0 <= beta < 1"),
    (dict(beta2=1.0), "0 <= beta < 1"),
    (dict(beta2=float("nan")), "0 <= beta < 1"),
    (dict(eps=0.0), "eps must be positive"),
    (dict(eps=-1e-8), "eps must be positive"),
    (dict(eps=1e-40), "eps is too small"),          # a denormal: eps * sqrt(1 - beta2^t) would flush the zero channels' 0 / (0 + eps') to 0 / 0
    (dict(eps=2e-38), "eps is too small"),          # normal itself, but times sqrt(1 - 0.999) it is not
    (dict(decoupled=2), "decoupled is 0"),
    (dict(nranges=33, ranges=P_OK), "lr-mult ranges"),
    (dict(nranges=1, ranges=None), "lr-mult ranges"),
]
SGD_REFUSALS = [
    (dict(velocity=None), "null pointer"),
    (dict(sched=None), "null schedule"),
    (dict(params=P_ODD), "16-byte aligned"),
    (dict(mirror=P_OK, mirror_dtype=3), "mirror is bf16 or fp16"),
    (dict(nranges=-1), "lr-mult ranges"),
]


def _call(L, name, args):
    sched = args["sched"]           # kept alive across the call
    vals = [ctypes.cast(ctypes.pointer(v), ctypes.c_void_p) if k == "sched" and v is not None else v for k, v in args.items()]
    assert [k for k in args] == [a for _, a in L.protos[name][1]]
    L.call(name, *vals)
    return sched


@pytest.mark.parametrize("change,match", ADAMW_REFUSALS + [(dict(sched=_sched(**c)), m) for c, m in SCHED_REFUSALS],
                         ids=lambda v: None if isinstance(v, dict) else v.replace(" ", "_"))
def test_adamw_step_refuses_bad_arguments_before_any_launch(real_lib, change, match):
    from emrt_amd import _lib
    with pytest.raises(_lib.EmrtHipError, match="emrt_adamw_step.*" + match):
        _call(real_lib, "emrt_adamw_step", _adamw_args(**change))


@pytest.mark.parametrize("change,match", SGD_REFUSALS + [(dict(sched=_sched(**c)), m) for c, m in SCHED_REFUSALS],
                         ids=lambda v: None if isinstance(v, dict) else v.replace(" ", "_"))
def test_sgd_step_sched_refuses_bad_arguments_before_any_launch(real_lib, change, match):
    from emrt_amd import _lib
    with pytest.raises(_lib.EmrtHipError, match="emrt_sgd_momentum_step_sched.*" + match):
        _call(real_lib, "emrt_sgd_momentum_step_sched", _sgd_args(**change))


def _builtin_sgd_args(**kw):
    a = dict(params=P_OK, grads=P_OK, velocity=P_OK, n=64, clip_state=P_OK, step=P_OK, base_lr=0.01, end_lr=0.0, power=0.9, decay_steps=100, momentum=0.9,
             weight_decay=1e-4, ranges=None, nranges=0, range_mult=0.1, lr_out=None, mirror=None, mirror_dtype=0, stream=None)
    a.update(kw)
    return a


# (the entry point with the built-in polynomial shares its checks with the other two: the messages must still carry ITS name)
@pytest.mark.parametrize("change,match", [
    (dict(velocity=None), "null pointer"),
    (dict(params=P_ODD), "16-byte aligned"),
    (dict(mirror=P_OK, mirror_dtype=3), "mirror is bf16 or fp16"),
    (dict(nranges=-1), "lr-mult ranges"),
    (dict(decay_steps=0), "decay_steps must be positive"),
], ids=lambda v: None if isinstance(v, dict) else v.replace(" ", "_"))
def test_sgd_step_refuses_bad_arguments_before_any_launch(real_lib, change, match):
    from emrt_amd import _lib
    args = _builtin_sgd_args(**change)
    assert [k for k in args] == [a for _, a in real_lib.protos["emrt_sgd_momentum_step"][1]]
    with pytest.raises(_lib.EmrtHipError, match="emrt_sgd_momentum_step: .*" + match):
        real_lib.call("emrt_sgd_momentum_step", *args.values())


# one null required pointer per loss entry point that tests/test_losses_cpu.py does not refuse with one (shapes 2 x 6 x 8 x 8, ignore_index 255)
LOSS_NULL_REFUSALS = [
    ("emrt_softmax_ce_fwd", (P_OK, P_OK, 2, 6, 8, 8, 255, None, P_OK, None)),                                       # result
    ("emrt_softmax_ce_bwd", (P_OK, None, P_OK, None, 1.0, 2, 6, 8, 8, 255, P_OK, None)),                            # labels
    ("emrt_softmax_ce_pair_fwd", (P_OK, P_OK, P_OK, 2, 6, 8, 8, 255, 1.0, 0.4, P_OK, P_OK, None, P_OK, None)),               # total
    ("emrt_softmax_ce_pair_bwd", (P_OK, P_OK, P_OK, P_OK, None, None, 1.0, 0.4, 2, 6, 8, 8, 255, P_OK, None, None)),      # dlogits_b
    ("emrt_wce_bwd", (P_OK, P_OK, None, P_OK, None, 1.0, 2, 6, 8, 8, 255, None, None)),                             # dlogits (class_weight may be null)
    ("emrt_wce_pair_bwd", (P_OK, P_OK, P_OK, None, None, None, None, 1.0, 0.4, 2, 6, 8, 8, 255, P_OK, P_OK, None)),       # res_a
]


@pytest.mark.parametrize("name,args", LOSS_NULL_REFUSALS, ids=[n for n, _ in LOSS_NULL_REFUSALS])
def test_loss_entry_points_refuse_a_null_pointer_under_their_own_name(real_lib, name, args):
    from emrt_amd import _lib
    assert len(args) == len(real_lib.protos[name][1])
    with pytest.raises(_lib.EmrtHipError, match=name + ": null pointer"):
        real_lib.call(name, *args)


def test_abi_is_still_version_9_with_the_new_entry_points(real_lib):
    assert real_lib.query("emrt_abi_version") == 9
    assert "emrt_adamw_step" in real_lib.protos and "emrt_sgd_momentum_step_sched" in real_lib.protos
