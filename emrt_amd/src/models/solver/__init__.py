"""Optimizers / LR schedules of the EMRT recipe (reference: src/models/solver/optimizer.py:29-55, lr_scheduler.py:30-267).

Momentum = ClipGradByGlobalNorm -> L2 decay (g += wd * p) -> v = mu * v + g -> p -= lr * lr_mult * v, run by two HIP
kernels over the model's flat parameter buffer; AdamW / Adam = the same clip -> emrt_adamw_step (include/emrt_hip.h states
the arithmetic).  Every schedule is evaluated on the device from the step counter (the host classes mirror it in float64
for logging), so one optimizer step is capturable in a hipGraph."""
import bisect
import ctypes
import math

import torch

from .... import _lib
from .... import functional as Fn
from ....runtime import ctx


class PolynomialDecay:
    def __init__(self, learning_rate, decay_steps, end_lr=0.0, power=0.9):
        self.base_lr, self.decay_steps, self.end_lr, self.power = learning_rate, decay_steps, end_lr, power
        self.last_epoch = 0

    def get_lr(self):
        t = min(self.last_epoch, self.decay_steps)
        return (self.base_lr - self.end_lr) * (1.0 - t / self.decay_steps) ** self.power + self.end_lr

    def step(self):
        self.last_epoch += 1

    def descriptor(self):
        return EmrtLrSchedule(kind=0, base_lr=self.base_lr, end_lr=self.end_lr, power=self.power, total_steps=int(self.decay_steps))


EmrtLrSchedule = _lib.struct("EmrtLrSchedule")      # generated from include/emrt_hip.h
EmrtLrSchedule.__doc__ = "include/emrt_hip.h: EmrtLrSchedule, the host descriptor the schedule-driven optimizer kernels evaluate on the device."
EmrtLrSchedule.KINDS = ("PolynomialDecay", "WarmupPolyLR", "WarmupCosineLR", "WarmupMultiStepLR")


class _Schedule:
    """What the optimizers and TrainEngine use of a schedule: get_lr() in float64 from last_epoch (= the device step counter),
    step(), descriptor()."""
    last_epoch = 0

    def step(self):
        self.last_epoch += 1


class WarmupPolyLR(_Schedule):
    """lr_scheduler.py:120-184, quirks included: the decay's floor is warmup_lr_init (not lr_min), a value <= lr_min becomes
    lr_min, and past max_iters (where the reference's pow() turns complex) the answer is lr_min."""

    def __init__(self, learning_rate, warmup_lr_init=0.0, max_iters=0, power=0.9, warmup_steps=5, lr_min=0.0):
        if not learning_rate > lr_min:
            raise ValueError("WarmupPolyLR: learning_rate (%g) must be greater than lr_min (%g)" % (learning_rate, lr_min))
        if warmup_steps < 0 or max_iters <= warmup_steps:
            raise ValueError("WarmupPolyLR: max_iters (%d) must be greater than warmup_steps (%d)" % (max_iters, warmup_steps))
        self.base_lr, self.warmup_lr_init, self.max_iters = float(learning_rate), float(warmup_lr_init), int(max_iters)
        self.power, self.warmup_steps, self.lr_min = float(power), int(warmup_steps), float(lr_min)

    def get_lr(self):
        s, W = self.last_epoch, self.warmup_steps
        if s < W:
            lr = self.warmup_lr_init + (self.base_lr - self.warmup_lr_init) * (float(s) / W)
        else:
            f = 1 - (s - W) / (self.max_iters - W)
            if f < 0:
                return self.lr_min
            lr = self.warmup_lr_init + (self.base_lr - self.warmup_lr_init) * f ** self.power
        return self.lr_min if lr <= self.lr_min else lr

    def descriptor(self):
        return EmrtLrSchedule(kind=1, base_lr=self.base_lr, end_lr=self.lr_min, power=self.power, warmup_lr_init=self.warmup_lr_init,
                              total_steps=self.max_iters, warmup_steps=self.warmup_steps)


class WarmupCosineLR(_Schedule):
    """lr_scheduler.py:30-117 as get_scheduler builds it (t_mul = decay_rate = 1, no warmup prefix, no cycle limit): the
    cosine restarts every max_iters steps."""

    def __init__(self, learning_rate, max_iters, lr_min=0.0, warmup_steps=0, warmup_lr_init=0.0):
        if max_iters < 1 or lr_min < 0 or warmup_steps < 0:
            raise ValueError("WarmupCosineLR: max_iters >= 1, lr_min >= 0 and warmup_steps >= 0 (got %r, %r, %r)" % (max_iters, lr_min, warmup_steps))
        self.base_lr, self.max_iters, self.lr_min = float(learning_rate), int(max_iters), float(lr_min)
        self.warmup_steps, self.warmup_lr_init = int(warmup_steps), float(warmup_lr_init)

    def get_lr(self):
        s = self.last_epoch
        if s < self.warmup_steps:
            return self.warmup_lr_init + s * ((self.base_lr - self.warmup_lr_init) / self.warmup_steps)
        tc = s % self.max_iters
        return self.lr_min + 0.5 * (self.base_lr - self.lr_min) * (1 + math.cos(math.pi * tc / self.max_iters))

    def descriptor(self):
        return EmrtLrSchedule(kind=2, base_lr=self.base_lr, end_lr=self.lr_min, warmup_lr_init=self.warmup_lr_init,
                              total_steps=self.max_iters, warmup_steps=self.warmup_steps)


class WarmupMultiStepLR(_Schedule):
    """lr_scheduler.py:187-240: the ramp holds for s <= warmup_steps (not <), then base * gamma^(milestones passed).  The
    reference divides by zero for warmup_steps = 0; that is a ValueError here."""

    def __init__(self, learning_rate, milestones, gamma=0.1, warmup_steps=1000):
        milestones = [int(m) for m in milestones]
        if any(b <= a for a, b in zip(milestones, milestones[1:])):
            raise ValueError("WarmupMultiStepLR: milestones must be increasing integers, got %s" % (milestones,))
        if not 1 <= len(milestones) <= 16:
            raise ValueError("WarmupMultiStepLR: 1..16 milestones, got %d" % len(milestones))
        if warmup_steps < 1:
            raise ValueError("WarmupMultiStepLR: warmup_steps must be at least 1 (the ramp divides by it)")
        if warmup_steps > milestones[0]:
            raise ValueError("WarmupMultiStepLR: warmup_steps (%d) must not exceed milestones[0] (%d)" % (warmup_steps, milestones[0]))
        self.base_lr, self.milestones, self.gamma, self.warmup_steps = float(learning_rate), milestones, float(gamma), int(warmup_steps)

    def get_lr(self):
        s = self.last_epoch
        if s <= self.warmup_steps:
            return self.base_lr * (float(s) / self.warmup_steps)
        return self.base_lr * self.gamma ** bisect.bisect_right(self.milestones, s)

    def descriptor(self):
        d = EmrtLrSchedule(kind=3, base_lr=self.base_lr, gamma=self.gamma, total_steps=max(self.milestones[-1], 1), warmup_steps=self.warmup_steps,
                           nmilestones=len(self.milestones))
        for i, m in enumerate(self.milestones):
            d.milestones[i] = m
        return d


class Momentum:
    def __init__(self, model, lr_scheduler, momentum=0.9, weight_decay=0.0, grad_clip=None, use_nesterov=False):
        if use_nesterov:
            raise NotImplementedError("Nesterov momentum is not used by any EMRT config; supported: sgd (plain momentum), adam, adamw")
        self.model, self._learning_rate = model, lr_scheduler
        self.momentum, self.weight_decay, self.grad_clip = momentum, float(weight_decay), grad_clip
        st = model.store
        c = ctx()
        self.clip_state = c.zeros((2,), torch.float32)
        self.lr_dev = c.zeros((1,), torch.float32)
        self.ranges = (ctypes.c_longlong * (2 * len(st.lr_ranges)))(*[v for r in st.lr_ranges for v in r])
        # any schedule but the built-in polynomial goes to the kernel as a descriptor (kept alive here: the call reads it on the host)
        self.sched_desc = None if isinstance(lr_scheduler, PolynomialDecay) else lr_scheduler.descriptor()

    def get_lr(self):
        return self._learning_rate.get_lr()

    def grad_norm(self):
        return float(self.clip_state[1].item())

    def step(self):
        """Enqueues clip + update (master and compute-dtype mirror) on the current stream; advances the device step counter."""
        c, st, L = ctx(), self.model.store, _lib.lib()
        sch = self._learning_rate
        ws = c.workspace(L.query("emrt_gradnorm_workspace_bytes"))
        L.call("emrt_grad_clip_scale", Fn.P(st.grad), st.n_train, float(self.grad_clip or 0.0), Fn.P(self.clip_state), Fn.P(ws), c.stream)
        if self.sched_desc is None:
            L.call("emrt_sgd_momentum_step", Fn.P(st.master), Fn.P(st.grad), Fn.P(st.velocity), st.n_train, Fn.P(self.clip_state),
                   Fn.P(c.step_counter), sch.base_lr, sch.end_lr, sch.power, sch.decay_steps, self.momentum, self.weight_decay,
                   ctypes.cast(self.ranges, ctypes.c_void_p), len(st.lr_ranges), st.lr_mult, Fn.P(self.lr_dev), Fn.P(st.mirror), st.dtype, c.stream)
        else:
            L.call("emrt_sgd_momentum_step_sched", Fn.P(st.master), Fn.P(st.grad), Fn.P(st.velocity), st.n_train, Fn.P(self.clip_state),
                   Fn.P(c.step_counter), ctypes.cast(ctypes.pointer(self.sched_desc), ctypes.c_void_p), self.momentum, self.weight_decay,
                   ctypes.cast(self.ranges, ctypes.c_void_p), len(st.lr_ranges), st.lr_mult, Fn.P(self.lr_dev), Fn.P(st.mirror), st.dtype, c.stream)
        L.call("emrt_counter_add", Fn.P(c.step_counter), 1, c.stream)
        # the forward operands (fp32 master / its compute-dtype mirror) are current; the transposed dgrad copies are refreshed
        # where they are next needed, at the start of the next backward (EMRT.__call__ records it): the step then ends with
        # the mirror as the last thing written, which is what the next forward reads first
        if st.dirty:
            st.pack()

    def state_dict(self):
        """Momentum per parameter NAME in the parameter's logical shape (as the reference's .pdopt is keyed, train.py:204-206): the flat
        buffer's layout (alignment, padded stem channels) is an internal detail that has changed before and must not be the file format."""
        st = self.model.store
        return {"velocity": {n: st.named_view(st.velocity, n).detach().clone() for n in st.train_order},
                "step": int(ctx().step_counter.item()), "format": "per-parameter"}

    def set_state_dict(self, sd):
        st = self.model.store
        if "velocity" not in sd and "moment2" in sd:
            raise ValueError("optimizer checkpoint was written by AdamW / Adam (it holds moment1 / moment2) but this run uses SGD-momentum: "
                             "the states do not convert; resume with TRAIN.OPTIMIZER.NAME as it was, or from the model weights alone")
        vel = sd["velocity"]
        if torch.is_tensor(vel):        # a checkpoint of an earlier version: the raw flat buffer, only valid for the identical layout
            if vel.numel() != st.velocity.numel():
                raise ValueError("optimizer checkpoint holds a flat velocity buffer of %d elements but this build lays the parameters out in %d: "
                                 "the flat format is layout-dependent and cannot be converted; resume from the model weights instead"
                                 % (vel.numel(), st.velocity.numel()))
            st.velocity.copy_(vel)
        else:
            missing = [n for n in st.train_order if n not in vel]
            if missing:
                raise KeyError("optimizer checkpoint lacks momentum for %d parameters, e.g. %s" % (len(missing), missing[:3]))
            st.velocity.zero_()
            for n in st.train_order:
                view = st.named_view(st.velocity, n)
                if tuple(vel[n].shape) != tuple(view.shape):
                    raise ValueError("optimizer checkpoint: momentum of %s has shape %s, the parameter %s" % (n, tuple(vel[n].shape), tuple(view.shape)))
                view.copy_(vel[n].to(view.device))
        ctx().step_counter.fill_(int(sd["step"]))
        self._learning_rate.last_epoch = int(sd["step"])


class AdamW:
    """paddle.optimizer.AdamW (decoupled=True; optimizer.py:48-55) or paddle.optimizer.Adam (decoupled=False; optimizer.py:43-47) over the
    model's flat parameter buffer, with Momentum's surface.  One step = ClipGradByGlobalNorm (emrt_grad_clip_scale) -> emrt_adamw_step ->
    emrt_counter_add, all on the context's stream and with the learning rate and both bias terms formed on the device from the step counter,
    so the step is capturable.  The first moment lives in the store's velocity buffer; the second is allocated here (an SGD run does not
    pay for it).  Both decays scale with the parameter's learning-rate multiplier, and every parameter decays (apply_decay_param_fun=None).

    decoupled=False follows the reference in NOT clipping: it builds the clip object but does not hand it to optim.Adam, so grad_clip is
    ignored there (get_optimizer says so in a log line); no norm is computed either, so grad_norm() returns 0.0 on that path."""

    def __init__(self, model, lr_scheduler, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.0, grad_clip=None, decoupled=True):
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError("AdamW: betas must lie in [0, 1), got (%r, %r)" % (beta1, beta2))
        if not epsilon > 0.0:
            raise ValueError("AdamW: epsilon must be positive, got %r" % (epsilon,))
        self.model, self._learning_rate = model, lr_scheduler
        self.beta1, self.beta2, self.epsilon, self.weight_decay = float(beta1), float(beta2), float(epsilon), float(weight_decay)
        self.decoupled = bool(decoupled)
        self.grad_clip = grad_clip if self.decoupled else None
        st = model.store
        c = ctx()
        self.clip_state = c.zeros((2,), torch.float32)
        self.lr_dev = c.zeros((1,), torch.float32)
        self.moment2 = torch.zeros_like(st.velocity)
        self.ranges = (ctypes.c_longlong * (2 * len(st.lr_ranges)))(*[v for r in st.lr_ranges for v in r])
        self.sched_desc = lr_scheduler.descriptor()

    def get_lr(self):
        return self._learning_rate.get_lr()

    def grad_norm(self):
        return float(self.clip_state[1].item())

    def step(self):
        """Enqueues clip + update (master, both moments and the compute-dtype mirror) on the current stream; advances the device step counter."""
        c, st, L = ctx(), self.model.store, _lib.lib()
        if self.decoupled:
            ws = c.workspace(L.query("emrt_gradnorm_workspace_bytes"))
            L.call("emrt_grad_clip_scale", Fn.P(st.grad), st.n_train, float(self.grad_clip or 0.0), Fn.P(self.clip_state), Fn.P(ws), c.stream)
        L.call("emrt_adamw_step", Fn.P(st.master), Fn.P(st.grad), Fn.P(st.velocity), Fn.P(self.moment2), st.n_train,
               Fn.P(self.clip_state) if self.decoupled else None, Fn.P(c.step_counter), ctypes.cast(ctypes.pointer(self.sched_desc), ctypes.c_void_p),
               self.beta1, self.beta2, self.epsilon, self.weight_decay, int(self.decoupled), ctypes.cast(self.ranges, ctypes.c_void_p),
               len(st.lr_ranges), st.lr_mult, Fn.P(self.lr_dev), Fn.P(st.mirror), st.dtype, c.stream)
        L.call("emrt_counter_add", Fn.P(c.step_counter), 1, c.stream)
        if st.dirty:        # as Momentum.step: the mirror is current, the transposed copies are refreshed by the next backward
            st.pack()

    def state_dict(self):
        """Both moments per parameter NAME in the parameter's logical shape, as Momentum.state_dict keys its velocity."""
        st = self.model.store
        return {"moment1": {n: st.named_view(st.velocity, n).detach().clone() for n in st.train_order},
                "moment2": {n: st.named_view(self.moment2, n).detach().clone() for n in st.train_order},
                "step": int(ctx().step_counter.item()), "format": "per-parameter", "optimizer": "adamw" if self.decoupled else "adam"}

    def set_state_dict(self, sd):
        st = self.model.store
        if "moment2" not in sd:
            if "velocity" in sd:
                raise ValueError("optimizer checkpoint was written by SGD-momentum (it holds a velocity and no moment2) but this run uses AdamW / Adam: "
                                 "the states do not convert; resume with TRAIN.OPTIMIZER.NAME as it was, or from the model weights alone")
            raise KeyError("optimizer checkpoint holds neither moment2 nor velocity")
        for key, flat in (("moment1", st.velocity), ("moment2", self.moment2)):
            src = sd[key]
            missing = [n for n in st.train_order if n not in src]
            if missing:
                raise KeyError("optimizer checkpoint lacks %s for %d parameters, e.g. %s" % (key, len(missing), missing[:3]))
            for n in st.train_order:
                view = st.named_view(flat, n)
                if tuple(src[n].shape) != tuple(view.shape):
                    raise ValueError("optimizer checkpoint: %s of %s has shape %s, the parameter %s" % (key, n, tuple(src[n].shape), tuple(view.shape)))
        for key, flat in (("moment1", st.velocity), ("moment2", self.moment2)):
            flat.zero_()
            for n in st.train_order:
                view = st.named_view(flat, n)
                view.copy_(sd[key][n].to(view.device))
        ctx().step_counter.fill_(int(sd["step"]))
        self._learning_rate.last_epoch = int(sd["step"])


SCHEDULERS = ("PolynomialDecay", "WarmupPolyLR", "WarmupCosineLR", "WarmupMultiStepLR")
OPTIMIZERS = ("sgd", "adam", "adamw")


def get_scheduler(config):
    T, S = config.TRAIN, config.TRAIN.LR_SCHEDULER
    if S.NAME == "PolynomialDecay":
        return PolynomialDecay(T.BASE_LR, T.ITERS, T.END_LR, T.POWER)
    if S.NAME == "WarmupPolyLR":
        return WarmupPolyLR(T.BASE_LR, warmup_lr_init=S.WARM_UP_LR_INIT, max_iters=T.ITERS, power=S.POWER, warmup_steps=S.WARM_UP_STEPS, lr_min=T.END_LR)
    if S.NAME == "WarmupCosineLR":
        return WarmupCosineLR(T.BASE_LR, T.ITERS, lr_min=T.END_LR, warmup_steps=S.WARM_UP_STEPS, warmup_lr_init=S.WARM_UP_LR_INIT)
    if S.NAME == "WarmupMultiStepLR":
        return WarmupMultiStepLR(T.BASE_LR, S.MILESTONES, gamma=S.GAMMA, warmup_steps=S.WARM_UP_STEPS)
    raise NotImplementedError("LR_SCHEDULER.NAME %r is not on the EMRT path; supported: %s" % (S.NAME, ", ".join(SCHEDULERS)))


def get_optimizer(model, lr_scheduler, config):
    O = config.TRAIN.OPTIMIZER
    name = O.NAME.lower()
    if name == "sgd":
        return Momentum(model, lr_scheduler, momentum=O.MOMENTUM, weight_decay=float(O.WEIGHT_DECAY), grad_clip=O.GRAD_CLIP, use_nesterov=O.NESTEROV)
    if name == "adamw":
        return AdamW(model, lr_scheduler, beta1=O.BETAS[0], beta2=O.BETAS[1], epsilon=O.EPS, weight_decay=float(O.WEIGHT_DECAY), grad_clip=O.GRAD_CLIP)
    if name == "adam":
        # the reference passes neither BETAS nor its clip object to optim.Adam (optimizer.py:43-47): paddle's defaults, no clipping
        if O.GRAD_CLIP:
            print("[solver] OPTIMIZER.NAME adam: GRAD_CLIP %s is not applied (the reference does not pass it to optim.Adam)" % (O.GRAD_CLIP,), flush=True)
        if tuple(O.BETAS) != (0.9, 0.999):
            print("[solver] OPTIMIZER.NAME adam: BETAS %s are not used (the reference does not pass them to optim.Adam); betas are (0.9, 0.999)"
                  % (tuple(O.BETAS),), flush=True)
        return AdamW(model, lr_scheduler, beta1=0.9, beta2=0.999, epsilon=O.EPS, weight_decay=float(O.WEIGHT_DECAY), grad_clip=None, decoupled=False)
    raise NotImplementedError("OPTIMIZER.NAME %r is not on the EMRT path (no kernel for it); supported: %s" % (O.NAME, ", ".join(OPTIMIZERS)))
