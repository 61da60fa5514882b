"""realvsr_amd.lr_scheduler against per-step rates recorded from the reference's classes (tests/golden/make_golden_lr.py).

The bound is 1e-12 * base_lr: the closed form and the reference's step-to-step recursion differ by rounding only -- measured 1.45e-14 *
base_lr over the shipped 600 000-step schedule -- and the recursion itself rounds at that level, so == is not the claim."""
import json
import types
import warnings
from collections import Counter

import numpy as np
import pytest
import torch

from conftest import load_golden
from realvsr_amd import lr_scheduler as S
from realvsr_amd.VideoSR_model import _TrainingState

G = load_golden('lr_schedules')
THREE = dict(T_period=[50, 30, 40], restarts=[50, 80], weights=[1, 0.5], eta_min=1e-7)


def _adam(lrs):
    return torch.optim.Adam([{'params': [torch.zeros(2, requires_grad=True)], 'lr': lr} for lr in lrs])


def _run(sched, steps):
    opt = sched.optimizer
    rows = [[g['lr'] for g in opt.param_groups]]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')     # (stepped without optimizer steps)
        for _ in range(steps):
            sched.step()
            rows.append([g['lr'] for g in opt.param_groups])
    return np.array(rows, dtype=np.float64)


def _close(got, want, base):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want).max() / base
    print('largest deviation %.3g * base_lr' % err)
    assert err <= 1e-12


def test_shipped_schedule_as_a_function_of_t():
    t = G['shipped_t']
    assert len(t) > 600 and {150001, 300001, 450001, 149998, 450004} <= set(t.tolist())
    got = [S.cosine_restart_lr(int(v), 1e-4, [150000] * 4, [150000, 300000, 450000], [1, 1, 1], 1e-7) for v in t]
    _close(got, G['shipped_lr'], 1e-4)
    assert got[0] == 1e-4 and S.cosine_restart_lr(150001, 1e-4, [150000] * 4, [150000, 300000, 450000], [1, 1, 1], 1e-7) == 1e-4


def test_stepped_cosine_three_segments():
    got = _run(S.CosineAnnealingLR_Restart(_adam([2e-4]), **THREE), 120)[:, 0]
    _close(got, G['three_lr'], 2e-4)
    assert got[51] == 2e-4 and got[81] == 1e-4     # the restarts, one epoch late, at initial_lr * weight
    pure = [S.cosine_restart_lr(t, 2e-4, THREE['T_period'], THREE['restarts'], THREE['weights'], 1e-7) for t in range(121)]
    assert np.array_equal(np.array(pure), got)


def test_stepped_cosine_past_its_period_rises_again():
    got = _run(S.CosineAnnealingLR_Restart(_adam([1e-4]), [20, 20], restarts=[70], weights=[1], eta_min=1e-7), 100)[:, 0]
    _close(got, G['rising_lr'], 1e-4)
    assert got[30] > got[20] and got[40] > got[30]


def test_two_parameter_groups():
    got = _run(S.CosineAnnealingLR_Restart(_adam([1e-4, 3e-4]), **THREE), 120)
    _close(got, G['groups_lr'], 1e-4)
    assert (got[:, 1] >= got[:, 0]).all() and got[0].tolist() == [1e-4, 3e-4] and got[81].tolist() == [0.5e-4, 1.5e-4]


def test_multistep_restart_rates_and_cleared_state():
    opt = _adam([1e-3])
    sched = S.MultiStepLR_Restart(opt, [3, 6, 6, 9], restarts=[5], weights=[0.5], gamma=0.5, clear_state=True)
    p = opt.param_groups[0]['params'][0]
    rates, empty = [opt.param_groups[0]['lr']], []
    for t in range(1, 13):
        p.grad = torch.ones_like(p)
        opt.step()
        sched.step()
        rates.append(opt.param_groups[0]['lr'])
        empty.append(len(opt.state) == 0)
    _close(rates, G['multistep_lr'], 1e-3)
    # 1e-3 until the milestone 3, the restart one epoch after 5 at half the initial rate -- the double milestone on that epoch is
    # not applied -- then the milestone 9
    assert rates == [1e-3] * 3 + [5e-4] * 6 + [2.5e-4] * 4
    assert empty == [t == 6 for t in range(1, 13)]
    pure = [S.multistep_restart_lr(t, 1e-3, [3, 6, 6, 9], [5], [0.5], 0.5) for t in range(13)]
    assert pure == rates


def test_multistep_keeps_state_without_clear_state():
    opt = _adam([1e-3])
    sched = S.MultiStepLR_Restart(opt, [3], restarts=[5], weights=[0.5], gamma=0.5)
    p = opt.param_groups[0]['params'][0]
    for _ in range(8):
        p.grad = torch.ones_like(p)
        opt.step()
        sched.step()
        assert len(opt.state) == 1
    assert sched.restarts == [6] and sched.milestones == Counter([3])      # restarts shifted, milestones not


def test_state_dict_carries_the_reference_attribute_names():
    cos = S.CosineAnnealingLR_Restart(_adam([1e-4]), **THREE).state_dict()
    assert {'T_period', 'T_max', 'eta_min', 'restarts', 'restart_weights', 'last_restart', 'base_lrs', 'last_epoch', '_step_count'} <= set(cos)
    assert cos['restarts'] == [51, 81] and cos['T_max'] == 50 and cos['last_restart'] == 0 and 'optimizer' not in cos
    ms = S.MultiStepLR_Restart(_adam([1e-4]), [3, 6, 6], restarts=[5], weights=[1], gamma=0.5, clear_state=True).state_dict()
    assert {'milestones', 'gamma', 'clear_state', 'restarts', 'restart_weights', 'base_lrs', 'last_epoch', '_step_count'} <= set(ms)
    assert isinstance(ms['milestones'], Counter) and ms['milestones'][6] == 2 and ms['restarts'] == [6]
    assert issubclass(S.CosineAnnealingLR_Restart, torch.optim.lr_scheduler._LRScheduler)
    assert issubclass(S.MultiStepLR_Restart, torch.optim.lr_scheduler._LRScheduler)


def test_recorded_reference_state_continues_on_the_recorded_curve():
    state = json.loads(str(G['resume_state']))
    assert state['last_epoch'] == 60 and state['last_restart'] == 51 and state['T_max'] == 30
    opt = _adam([2e-4])
    sched = S.CosineAnnealingLR_Restart(opt, **THREE)
    opt.param_groups[0]['lr'] = float(G['resume_group_lr'])     # (what the optimizer's own state_dict restores)
    sched.load_state_dict(state)
    assert sched.last_epoch == 60 and sched.last_restart == 51 and sched.T_max == 30
    got = _run(sched, 60)[:, 0]
    _close(got, G['three_lr'][60:], 2e-4)
    # and one of ours, saved mid-schedule and loaded into a fresh object
    a = S.CosineAnnealingLR_Restart(_adam([2e-4]), **THREE)
    _run(a, 95)
    b = S.CosineAnnealingLR_Restart(_adam([2e-4]), **THREE)
    b.load_state_dict(a.state_dict())
    assert np.array_equal(_run(b, 25)[1:, 0], _run(a, 25)[1:, 0])
    _close([b.optimizer.param_groups[0]['lr']], G['three_lr'][120:], 2e-4)


def _stub_model(lrs_per_optimizer, scheme=None):
    m = types.SimpleNamespace(optimizers=[_adam(lrs) for lrs in lrs_per_optimizer], schedulers=[])
    for name in ('_set_lr', '_get_init_lr', 'update_learning_rate', '_build_schedulers'):
        setattr(m, name, types.MethodType(getattr(_TrainingState, name), m))
    if scheme:
        m._build_schedulers(scheme, 'MultiStepLR_Restart')
    return m


def test_warm_up_overrides_the_first_iterations_only():
    train_opt = dict(lr_scheme='CosineAnnealingLR_Restart', restarts=THREE['restarts'], restart_weights=THREE['weights'],
                     T_period=THREE['T_period'], eta_min=1e-7)
    m = _stub_model([[2e-4, 4e-4], [1e-4]], train_opt)
    assert len(m.schedulers) == 2 and m._get_init_lr() == [[2e-4, 4e-4], [1e-4]]
    with warnings.catch_warnings():
        warnings.simplefilter('error')      # the loop's order (schedule, then optimizer) must not trip torch's warning
        for i in range(1, 6):
            m.update_learning_rate(i, warmup_iter=3)
            got = [[g['lr'] for g in o.param_groups] for o in m.optimizers]
            if i < 3:
                assert got == [[2e-4 / 3 * i, 4e-4 / 3 * i], [1e-4 / 3 * i]]
            else:       # the closed form is back on the schedule at once: the warm-up value does not leak into it
                _close([got[0][0]], [G['three_lr'][i]], 2e-4)
                assert got == [[S.cosine_restart_lr(i, b, THREE['T_period'], THREE['restarts'], THREE['weights'], 1e-7) for b in bs]
                               for bs in ([2e-4, 4e-4], [1e-4])]


def test_scheme_names():
    m = _stub_model([[1e-4]], dict(lr_scheme='MultiStepLR_Restart', lr_steps=[2], restarts=None, restart_weights=None, lr_gamma=0.5,
                                   clear_state=False))
    assert isinstance(m.schedulers[0], S.MultiStepLR_Restart)
    assert _stub_model([[1e-4]], {}).schedulers == []          # no lr_scheme: no scheduler, no error
    with pytest.raises(NotImplementedError):
        _stub_model([[1e-4]], dict(lr_scheme='StepLR'))
