"""The two learning-rate schedules of the reference's training loop (codes/models/lr_scheduler.py: MultiStepLR_Restart :8-32,
CosineAnnealingLR_Restart :35-64), with its constructor arguments, defaults and attribute names -- so ``state_dict()`` carries the keys
a reference ``.state`` file carries and either side loads the other's -- but written in CLOSED FORM instead of as the reference's
step-to-step recursion on ``param_group['lr']``:

  cosine      lr(t) = eta_min + (initial_lr * w_s - eta_min) * (1 + cos(pi (t - s) / T)) / 2,   lr(0) = base_lr
              s = the last restart epoch reached (0 before the first), w_s its weight (1 before the first), T that segment's period.
              Running past T without a restart, the cosine's own periodicity gives the reference's rising branch (:56-60).
  multi-step  lr(t) = initial_lr * w_s * gamma ** #{milestones m (with multiplicity): s < m <= t}
              a milestone on the restart epoch itself is not applied (:22-26 returns before :27 looks), milestones before it are forgotten.

A rate is therefore a function of (last_epoch, last_restart, T_max | milestones) alone: ``load_state_dict`` needs nothing beyond torch's
own, a warm-up that overwrites ``param_group['lr']`` (update_learning_rate) does not leak into the schedule, and no rounding accumulates
over 600 000 steps.  Against the reference's recursion the deviation is about 1e-14 of the base rate (tests/test_lr_scheduler_host.py).

The arithmetic is host scalars; FlatAdam.step passes ``param_group['lr']`` to its kernel as an argument, so a schedule adds no launch and
no synchronisation to a training step.
"""
import math
from collections import Counter, defaultdict

from torch.optim.lr_scheduler import _LRScheduler


def _shifted(restarts):
    """The reference counts a restart one epoch late (:15, :41): the scheduler's epoch 0 is the constructor's own step."""
    return [v + 1 for v in (restarts if restarts else [0])]


def _cosine(initial_lr, weight, eta_min, t, s, T):
    return eta_min + (initial_lr * weight - eta_min) * (1 + math.cos(math.pi * (t - s) / T)) / 2


def _segment(t, shifted_restarts):
    """Index of the last (shifted) restart epoch <= t in the order the stepped class meets them, or -1."""
    hit = -1
    for i, r in enumerate(shifted_restarts):
        if r <= t and (hit < 0 or r >= shifted_restarts[hit]):
            hit = i
    return hit


def cosine_restart_lr(t, base_lr, T_period, restarts=None, weights=None, eta_min=0):
    """CosineAnnealingLR_Restart's rate at epoch t as a pure function (arguments as the constructor's, restarts unshifted)."""
    shifted = _shifted(restarts)
    weights = weights if weights else [1]
    if t == 0:
        return base_lr
    i = _segment(t, shifted)
    if i < 0:
        return _cosine(base_lr, 1, eta_min, t, 0, T_period[0])
    if t == shifted[i]:
        return base_lr * weights[i]
    return _cosine(base_lr, weights[i], eta_min, t, shifted[i], T_period[min(i + 1, len(T_period) - 1)])


def multistep_restart_lr(t, base_lr, milestones, restarts=None, weights=None, gamma=0.1):
    """MultiStepLR_Restart's rate at epoch t as a pure function (arguments as the constructor's, restarts unshifted)."""
    shifted = _shifted(restarts)
    weights = weights if weights else [1]
    i = _segment(t, shifted)
    s, w = (shifted[i], weights[i]) if i >= 0 else (-1, 1)
    return base_lr * w * gamma ** sum(n for m, n in Counter(milestones).items() if s < m <= t)


class MultiStepLR_Restart(_LRScheduler):
    def __init__(self, optimizer, milestones, restarts=None, weights=None, gamma=0.1, clear_state=False, last_epoch=-1):
        self.milestones = Counter(milestones)
        self.gamma = gamma
        self.clear_state = clear_state
        self.restarts = _shifted(restarts)
        self.restart_weights = weights if weights else [1]
        assert len(self.restarts) == len(self.restart_weights), 'restarts and their weights do not match.'
        super(MultiStepLR_Restart, self).__init__(optimizer, last_epoch)

    def get_lr(self):
        t = self.last_epoch
        if t in self.restarts and self.clear_state:
            # FlatAdam.step turns an empty state into reset_state(): the moments and step counts start over (optim.py)
            self.optimizer.state = defaultdict(dict)
        i = _segment(t, self.restarts)
        s, w = (self.restarts[i], self.restart_weights[i]) if i >= 0 else (-1, 1)
        decay = self.gamma ** sum(n for m, n in self.milestones.items() if s < m <= t)
        return [group['initial_lr'] * w * decay for group in self.optimizer.param_groups]


class CosineAnnealingLR_Restart(_LRScheduler):
    def __init__(self, optimizer, T_period, restarts=None, weights=None, eta_min=0, last_epoch=-1):
        self.T_period = T_period
        self.T_max = self.T_period[0]  # the current segment's period
        self.eta_min = eta_min
        self.restarts = _shifted(restarts)
        self.restart_weights = weights if weights else [1]
        self.last_restart = 0
        assert len(self.restarts) == len(self.restart_weights), 'restarts and their weights do not match.'
        super(CosineAnnealingLR_Restart, self).__init__(optimizer, last_epoch)

    def get_lr(self):
        t = self.last_epoch
        if t == 0:
            return list(self.base_lrs)
        groups = self.optimizer.param_groups
        if t in self.restarts:
            i = self.restarts.index(t)
            self.last_restart = t
            # (the reference indexes T_period[i + 1] and fails where the list is one short; the last period is kept instead)
            self.T_max = self.T_period[min(i + 1, len(self.T_period) - 1)]
            return [group['initial_lr'] * self.restart_weights[i] for group in groups]
        # last_restart and T_max are state (state_dict carries them): a loaded scheduler continues from them
        s = self.last_restart
        w = self.restart_weights[self.restarts.index(s)] if s in self.restarts else 1
        return [_cosine(group['initial_lr'], w, self.eta_min, t, s, self.T_max) for group in groups]
