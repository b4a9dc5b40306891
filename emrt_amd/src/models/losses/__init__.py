"""Loss factory (reference: src/models/losses/__init__.py:6-12, mix_softmax_cross_entropy_loss.py:20-51)."""
from .... import functional as Fn
from ....runtime import ctx
from .... import _lib


class LossValue:
    """Device-resident scalar loss with the reference's call surface: .backward(), .numpy(), float()."""

    def __init__(self, total, parts, tape):
        self.tensor, self.parts, self.tape = total, parts, tape

    def backward(self):
        if self.tape is None:
            raise RuntimeError("loss was computed in eval mode; nothing to differentiate")
        self.tape.backward()
        self.tape = None

    def backward_until_split(self, segments=False):
        """First part of backward(): every op recorded after the model's last exchange mark.  Returns a callable that
        runs the rest -- or, with segments=True, one callable per remaining segment (between the marks, newest first)."""
        if self.tape is None:
            raise RuntimeError("loss was computed in eval mode; nothing to differentiate")
        tape, self.tape = self.tape, None
        marks = list(tape.splits)
        if not marks:
            tape.backward()
            return [] if segments else (lambda: None)
        tape.backward(stop_at=marks[-1])
        if not segments:
            return tape.backward
        stops = list(reversed(marks[:-1])) + [0]
        return [(lambda s_=s_: tape.backward(s_)) for s_ in stops]

    def item(self):
        return float(self.tensor[0].item())

    __float__ = item

    def numpy(self):
        import numpy as np
        return np.array([self.item()], dtype=np.float32)   # shape [1], as Paddle 2.1-2.4 (train.py:160)

    def __iter__(self):     # `sum(loss_list)` in the reference iterates the shape-[1] loss tensor (train.py:151-152)
        yield self

    def __radd__(self, other):
        return self if other == 0 else NotImplemented


def _combine_heads(parts, weights, tape):
    """total = parts[0] + weights[1] * parts[1] (one head: the head itself), formed on the device outside the tape: each head's weight is
    already part of its backward."""
    c = ctx()
    total = c.empty((1,), parts[0].dtype)
    L = _lib.lib()
    L.call("emrt_scalar_axpby", Fn.P(total), Fn.P(parts[0]), 1.0, Fn.P(parts[1]) if len(parts) > 1 else None,
           weights[1] if len(parts) > 1 else 0.0, c.stream)
    return LossValue(total, parts, tape)


def _class_weights(config_or_list, num_classes=None):
    """TRAIN.CLASS_WEIGHTS -> list of floats or None (empty = off); the length check is worded as losses/cross_entropy_loss.py:47-49."""
    w = config_or_list
    if w is None or len(w) == 0:
        return None
    w = [float(v) for v in w]
    if num_classes is not None and len(w) != num_classes:
        raise ValueError("The number of weights = {} must be the same as the number of classes = {}.".format(len(w), num_classes))
    return w


class MixSoftmaxCrossEntropyLoss:
    """CE(main) + AUX_WEIGHT * CE(aux), each the mean over pixels with label != IGNORE_INDEX.
    class_weights (TRAIN.CLASS_WEIGHTS, one float per class; empty = off): each head becomes nn.CrossEntropyLoss(weight=w, ignore_index),
    sum w[y] CE / sum w[y] (reference: the weight option of losses/cross_entropy_loss.py:30-35)."""

    def __init__(self, config=None, ignore_index=255, aux=True, aux_weight=0.4, class_weights=None):
        num_classes = None
        if config is not None:
            ignore_index, aux, aux_weight = config.TRAIN.IGNORE_INDEX, config.MODEL.AUX.LOSS, config.MODEL.AUX.AUX_WEIGHT
            class_weights, num_classes = config.TRAIN.CLASS_WEIGHTS, config.DATA.NUM_CLASSES
        self.ignore_index, self.aux, self.aux_weight = ignore_index, aux, aux_weight
        self.class_weights = _class_weights(class_weights, num_classes)
        # the weights on the device: uploaded here when the model is already placed (train.py's order), so that a step captured from its very
        # first call holds no host-to-device copy; else at the first call
        self._cw = None
        if self.class_weights is not None and ctx().device is not None:
            self._upload(ctx().device)

    def _upload(self, device):
        import torch
        self._cw = torch.tensor(self.class_weights, dtype=torch.float32, device=device)

    def _device_class_weights(self, logits):
        if self.class_weights is None:
            return None
        C = logits.shape[1]
        if len(self.class_weights) != C:
            raise ValueError("The number of weights = {} must be the same as the number of classes = {}.".format(len(self.class_weights), C))
        if self._cw is None or self._cw.device != logits.device:
            self._upload(logits.device)
        return self._cw

    def __call__(self, preds, target):
        c = ctx()
        tape = getattr(preds, "tape", None)
        c.tape = tape
        try:
            target = target.contiguous()
            weights = [1.0] + [self.aux_weight if self.aux else 1.0] * (len(preds) - 1)
            live = [(p, w) for p, w in zip(preds, weights) if p is not None]
            cw = self._device_class_weights(live[0][0])
            if len(live) == 2 and tuple(live[0][0].shape) == tuple(live[1][0].shape):
                # the recipe's case (main + aux head at the input size): both heads in one pass, the weighted total formed by the finalize launch
                ra, rb, total = Fn.softmax_ce_pair(live[0][0], live[1][0], target, self.ignore_index, live[0][1], live[1][1], class_weight=cw)
                return LossValue(total, [ra, rb], tape)
            parts = [Fn.softmax_ce(p, target, self.ignore_index, w, class_weight=cw) for p, w in live]
        finally:
            c.tape = None
        return _combine_heads(parts, weights, tape)


class OhemCrossEntropyLoss:
    """Online hard example mining (reference: losses/ohem_cross_entropy_loss.py:41-79), per head: keep the non-ignored pixels whose probability
    of their own class is below max(thresh, the min_kept-th smallest such probability) -- strictly below, so the k-th pixel and its ties are
    dropped, as in the reference -- and average their CE over kept + 1e-5 * B * H * W.  Every non-ignored pixel is kept when min_kept >= their
    number.  The threshold is selected on the device (functional.ohem_ce), so the loss is part of a captured step.

    The reference class takes ONE tensor and is not wired into its factory.  This build's wiring: the loss is applied to every head the model
    returns and the heads are combined as MixSoftmaxCrossEntropyLoss combines them, main + AUX_WEIGHT * aux (MODEL.AUX.LOSS off: weight 1;
    a None head is skipped)."""

    def __init__(self, config=None, thresh=0.7, min_kept=10000, ignore_index=255, aux=True, aux_weight=0.4):
        if config is not None:
            ignore_index, aux, aux_weight = config.TRAIN.IGNORE_INDEX, config.MODEL.AUX.LOSS, config.MODEL.AUX.AUX_WEIGHT
            thresh, min_kept = config.TRAIN.OHEM.THRESH, config.TRAIN.OHEM.MIN_KEPT
            if _class_weights(config.TRAIN.CLASS_WEIGHTS) is not None:
                raise ValueError("TRAIN.CLASS_WEIGHTS cannot be combined with OhemCrossEntropyLoss (the reference has no class-weighted OHEM)")
        if int(min_kept) < 0:
            raise ValueError("TRAIN.OHEM.MIN_KEPT must be >= 0, got %r" % (min_kept,))
        self.thresh, self.min_kept = float(thresh), int(min_kept)
        self.last_prob = []     # per head of the last call: the stored probabilities its mask was decided from (diagnostics; parts[i][2] is the threshold)
        self.ignore_index, self.aux, self.aux_weight = ignore_index, aux, aux_weight

    def __call__(self, preds, target):
        c = ctx()
        tape = getattr(preds, "tape", None)
        c.tape = tape
        try:
            target = target.contiguous()
            weights = [1.0] + [self.aux_weight if self.aux else 1.0] * (len(preds) - 1)
            live = [(p, w) for p, w in zip(preds, weights) if p is not None]
            if len(live) == 2 and tuple(live[0][0].shape) == tuple(live[1][0].shape):
                # main + aux head at the input size: both heads through the launches of one, the weighted total formed by the finalize launch
                ra, rb, total, pa, pb = Fn.ohem_ce_pair(live[0][0], live[1][0], target, self.ignore_index, self.thresh, self.min_kept, live[0][1], live[1][1])
                self.last_prob = [pa, pb]
                return LossValue(total, [ra, rb], tape)
            heads = [Fn.ohem_ce(p, target, self.ignore_index, self.thresh, self.min_kept, w) for p, w in live]
            parts = [res for res, _ in heads]
            self.last_prob = [prob for _, prob in heads]
        finally:
            c.tape = None
        return _combine_heads(parts, weights, tape)


class DiceCrossEntropyLoss:
    """CE_WEIGHT * CE + DICE_WEIGHT * Dice per head, in one pass over the logits on the device (functional.dice_ce; include/emrt_hip_loss.h).
    CE is MixSoftmaxCrossEntropyLoss's term (class_weights likewise); Dice = 1 - the mean over ALL classes of (2 I_c + s) / (P_c + T_c + s),
    I_c / P_c / T_c = intersection, probability mass and pixel count of class c over the non-ignored pixels of the whole batch, s = smooth:
    PaddleSeg's DiceLoss(ignore_index, smooth) in its softmax form.  The per-class sums are formed on the device between forward and backward, so
    the loss is part of a captured step.  Under data parallelism each rank forms Dice over its own shard and the gradients are averaged: that is
    not the Dice of the global batch.

    The heads are combined as MixSoftmaxCrossEntropyLoss combines them, main + AUX_WEIGHT * aux (MODEL.AUX.LOSS off: weight 1; a None head is
    skipped).  parts[i] is head i's device float[8] = {L, CE, Dice, sum w[y], non-ignored count, ...}."""

    def __init__(self, config=None, ce_weight=1.0, dice_weight=1.0, smooth=1.0, ignore_index=255, aux=True, aux_weight=0.4, class_weights=None):
        num_classes = None
        if config is not None:
            ignore_index, aux, aux_weight = config.TRAIN.IGNORE_INDEX, config.MODEL.AUX.LOSS, config.MODEL.AUX.AUX_WEIGHT
            class_weights, num_classes = config.TRAIN.CLASS_WEIGHTS, config.DATA.NUM_CLASSES
            ce_weight, dice_weight, smooth = config.TRAIN.DICE.CE_WEIGHT, config.TRAIN.DICE.WEIGHT, config.TRAIN.DICE.SMOOTH
        ce_weight, dice_weight, smooth = float(ce_weight), float(dice_weight), float(smooth)
        for key, v in (("CE_WEIGHT", ce_weight), ("WEIGHT", dice_weight), ("SMOOTH", smooth)):
            if v != v:
                raise ValueError("TRAIN.DICE.%s is NaN" % key)
            if v < 0:
                raise ValueError("TRAIN.DICE.%s must be >= 0, got %r" % (key, v))
        if ce_weight == 0 and dice_weight == 0:
            raise ValueError("TRAIN.DICE.WEIGHT and TRAIN.DICE.CE_WEIGHT are both 0: nothing to minimise")
        self.ce_weight, self.dice_weight, self.smooth = ce_weight, dice_weight, smooth
        self.ignore_index, self.aux, self.aux_weight = ignore_index, aux, aux_weight
        self.class_weights = _class_weights(class_weights, num_classes)
        self._cw = None      # uploaded here when the model is already placed, as MixSoftmaxCrossEntropyLoss does: no copy inside a captured step
        if self.class_weights is not None and ctx().device is not None:
            self._upload(ctx().device)

    _upload = MixSoftmaxCrossEntropyLoss._upload
    _device_class_weights = MixSoftmaxCrossEntropyLoss._device_class_weights

    def __call__(self, preds, target):
        c = ctx()
        tape = getattr(preds, "tape", None)
        c.tape = tape
        try:
            target = target.contiguous()
            weights = [1.0] + [self.aux_weight if self.aux else 1.0] * (len(preds) - 1)
            live = [(p, w) for p, w in zip(preds, weights) if p is not None]
            kw = dict(class_weight=self._device_class_weights(live[0][0]), ce_weight=self.ce_weight, dice_weight=self.dice_weight, smooth=self.smooth)
            if len(live) == 2 and tuple(live[0][0].shape) == tuple(live[1][0].shape):
                # main + aux head at the input size: both heads through the launches of one, the weighted total formed by the finalize launch
                ra, rb, total = Fn.dice_ce_pair(live[0][0], live[1][0], target, self.ignore_index, live[0][1], live[1][1], **kw)
                return LossValue(total, [ra, rb], tape)
            parts = [Fn.dice_ce(p, target, self.ignore_index, w, **kw) for p, w in live]
        finally:
            c.tape = None
        return _combine_heads(parts, weights, tape)


SUPPORTED_LOSSES = ("MixSoftmaxCrossEntropyLoss", "OhemCrossEntropyLoss", "DiceCrossEntropyLoss")


def get_loss_function(config):
    if config.TRAIN.LOSS == "MixSoftmaxCrossEntropyLoss":
        return MixSoftmaxCrossEntropyLoss(config)
    if config.TRAIN.LOSS == "OhemCrossEntropyLoss":
        return OhemCrossEntropyLoss(config)
    if config.TRAIN.LOSS == "DiceCrossEntropyLoss":
        return DiceCrossEntropyLoss(config)
    raise NotImplementedError("TRAIN.LOSS %r is not on the EMRT path: supported are %s" % (config.TRAIN.LOSS, ", ".join(SUPPORTED_LOSSES)))
