#!/usr/bin/env python
"""Generate tests/golden/lr_schedules.npz and tests/golden/sampler.npz by IMPORTING the reference's models/lr_scheduler.py and
data/data_sampler.py (build container only; both import nothing but torch, so they are loaded by file, without the packages around them).

Run from the repo root:   python tests/golden/make_golden_lr.py

lr_schedules.npz -- a rate is param_groups[g]['lr'] with the scheduler's last_epoch = t (t = 0 is the constructor's own step):
  shipped_t, shipped_lr      the schedule of every shipped option file (lr 1e-4, T_period [150000] * 4, restarts [150000, 300000, 450000],
                             weights [1, 1, 1], eta_min 1e-7) stepped 600 000 times; kept at every 1000th t and from 3 before to 4 after
                             each restart epoch
  three_lr [121]             T_period [50, 30, 40], restarts [50, 80], weights [1, 0.5], eta_min 1e-7, lr 2e-4
  rising_lr [101]            T_period [20, 20], restarts [70], weights [1], eta_min 1e-7, lr 1e-4: runs past T, the rising branch
  groups_lr [121, 2]         the 'three' schedule on two parameter groups, lr 1e-4 and 3e-4
  multistep_lr [13]          MultiStepLR_Restart: milestones [3, 6, 6, 9], restarts [5], weights [0.5], gamma 0.5, clear_state, lr 1e-3
  resume_state               json of the 'three' scheduler's state_dict() at last_epoch 60, and resume_group_lr: its group's 'lr' then
                             (what a .state file's 'schedulers' and 'optimizers' entries hold); three_lr[61:] is how it continues
sampler.npz
  indices [4, 8]             DistIterSampler(range(10), num_replicas 4, rank r, ratio 3) after set_epoch(2), r = 0 .. 3
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_golden import OUT, REF  # noqa: E402


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def adam(lrs):
    return torch.optim.Adam([{'params': [torch.zeros(2, requires_grad=True)], 'lr': lr} for lr in lrs])


def run(sched, steps):
    opt = sched.optimizer
    rows = [[g['lr'] for g in opt.param_groups]]
    for _ in range(steps):
        sched.step()
        rows.append([g['lr'] for g in opt.param_groups])
    return np.array(rows, dtype=np.float64)


def main():
    import warnings
    warnings.filterwarnings('ignore')   # (scheduler stepped without optimizer steps: on purpose)
    ref = load('models/lr_scheduler.py', 'ref_lr_scheduler')
    out = {}
    three = dict(T_period=[50, 30, 40], restarts=[50, 80], weights=[1, 0.5], eta_min=1e-7)

    lr = run(ref.CosineAnnealingLR_Restart(adam([1e-4]), [150000] * 4, restarts=[150000, 300000, 450000], weights=[1, 1, 1],
                                           eta_min=1e-7), 600000)[:, 0]
    keep = sorted(set(range(0, 600001, 1000)) | {r + d for r in (150000, 300000, 450000) for d in range(-3, 5)})
    out['shipped_t'] = np.array(keep, dtype=np.int64)
    out['shipped_lr'] = lr[keep]
    out['three_lr'] = run(ref.CosineAnnealingLR_Restart(adam([2e-4]), **three), 120)[:, 0]
    out['rising_lr'] = run(ref.CosineAnnealingLR_Restart(adam([1e-4]), [20, 20], restarts=[70], weights=[1], eta_min=1e-7), 100)[:, 0]
    out['groups_lr'] = run(ref.CosineAnnealingLR_Restart(adam([1e-4, 3e-4]), **three), 120)
    out['multistep_lr'] = run(ref.MultiStepLR_Restart(adam([1e-3]), [3, 6, 6, 9], restarts=[5], weights=[0.5], gamma=0.5,
                                                      clear_state=True), 12)[:, 0]

    sched = ref.CosineAnnealingLR_Restart(adam([2e-4]), **three)
    head = run(sched, 60)[:, 0]
    assert np.array_equal(head, out['three_lr'][:61])
    state = sched.state_dict()
    assert state['last_epoch'] == 60 and state['last_restart'] == 51 and state['T_max'] == 30
    out['resume_state'] = np.array(json.dumps(state))
    out['resume_group_lr'] = np.array(sched.optimizer.param_groups[0]['lr'], dtype=np.float64)
    assert np.array_equal(run(sched, 60)[1:, 0], out['three_lr'][61:])
    np.savez(os.path.join(OUT, 'lr_schedules.npz'), **out)

    sampler = load('data/data_sampler.py', 'ref_data_sampler')
    rows = []
    for r in range(4):
        s = sampler.DistIterSampler(list(range(10)), num_replicas=4, rank=r, ratio=3)
        s.set_epoch(2)
        rows.append(list(s))
    np.savez(os.path.join(OUT, 'sampler.npz'), indices=np.array(rows, dtype=np.int64))
    print('wrote lr_schedules.npz (%d arrays), sampler.npz %s' % (len(out), np.array(rows).shape))


if __name__ == '__main__':
    main()
