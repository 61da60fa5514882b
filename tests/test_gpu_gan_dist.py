"""The GAN stage data-parallel: VideoSRGANModel under opt['dist'] with one bucketed all-reduce for G and one, armed for two backward
passes, for D.  -m gpu

  * two ranks sharing ONE MI355X over gloo (three cases) against non-distributed models stepped on each rank's shard
  * RCCL itself in a one-rank group with both reducers forced on, in a fresh process
  * realvsr_amd.train under torch.distributed.run, two gloo ranks: trains, validates on rank 0, checkpoints, resumes
  * tools/gan_step.py --gpus 2 starts its own ranks and reports both reducers

Shapes: those of tests/golden/gan_step.npz (G = EDVR_NoUp nf 64, 3 frames, one residual block each side; D = MultiscaleDiscriminator_v4
nf 16, num_D 2; 48 x 64 frames; weights from fill_state_dict seeds 505 / 606), batch 4 = 2 per rank, bucket_mb 0.05."""
import glob
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, REPO
from rank_procs import free_port, run_ranks

pytestmark = pytest.mark.gpu

CASES = ['ragan', 'gan', 'ratio']
G_STEPS = {'ragan': (1, 2, 3), 'gan': (1, 2, 3), 'ratio': (2,)}       # the steps with a G update
NBT = {'ragan': 15, 'gan': 9, 'ratio': 11}    # D forwards over 3 steps: 5 per RaGAN step, 3 per vanilla step, 2 fewer without a G update


def _reset_bn_buffers(net):
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.reset_running_stats()


def _opt(case, dist, force=False):
    train = {'lr_G': 1e-3, 'weight_decay_G': 0, 'beta1_G': 0.9, 'beta2_G': 0.99, 'lr_D': 1e-3, 'weight_decay_D': 0, 'beta1_D': 0.9,
             'beta2_D': 0.99, 'pixel_criterion_s': 'ssim', 'pixel_weight_s': 1.0, 'pixel_criterion_d': 'cb', 'pixel_weight_d': 1.0,
             'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0, 'feature_criterion': 'cb', 'feature_weight': 0.0,
             'gan_type': 'gan' if case == 'gan' else 'ragan', 'gan_weight': 0.1, 'bucket_mb': 0.05, 'force_allreduce': force}
    if case == 'ratio':
        train.update(D_update_ratio=2, D_init_iters=1)
    return {'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'dist': dist, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
            'network_G': {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1, 'back_RBs': 1,
                          'predeblur': False, 'HR_in': False, 'w_TSA': False, 'center': None},
            'network_D': {'which_model_D': 'MultiscaleDiscriminator_v4', 'in_nc': 1, 'nf': 16, 'num_D': 2, 'gan_type': 'patch'},
            'path': {'pretrain_model_G': None, 'pretrain_model_D': None, 'strict_load': True}, 'train': train}


def _fill(model):
    from weights import fill_state_dict
    fill_state_dict(model.netG, 505, offset_std=0.02)
    fill_state_dict(model.netD, 606)
    _reset_bn_buffers(model.netD)


def _batch():
    """Batch 4: the two shards come from different seeds (and different brightness), so one shard's gradient is far from the mean."""
    parts = []
    for seed, gain in ((11, 1.0), (12, 0.6)):
        g = torch.Generator().manual_seed(seed)
        parts.append((torch.rand(2, 3, 3, 48, 64, generator=g) * gain, torch.rand(2, 3, 3, 48, 64, generator=g) * gain))
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _flat(o):
    return o.buffers.param.detach().cpu().clone()


# ---------------------------------------------------------------------------------------------------------------- two gloo ranks, one GPU
def _worker(rank, world, port, q, case):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from realvsr_amd.dist import broadcast_parameters, shard_range
    from realvsr_amd.VideoSR_model import create_model
    torch.manual_seed(100 + rank)                       # different initial weights per rank ...
    model = create_model(_opt(case, True))
    assert model.rank == rank and model.reducer_G.active and model.reducer_D.active
    if rank == 0:
        _fill(model)
    broadcast_parameters(model.netG)                    # ... until rank 0's are broadcast (parameters and buffers)
    broadcast_parameters(model.netD)
    out = {'buckets_G': len(model.reducer_G.buckets), 'buckets_D': len(model.reducer_D.buckets), 'G_after': [], 'D_after': []}
    x, gt = _batch()
    s, e = shard_range(4, rank, world)
    for step in (1, 2, 3):
        model.feed_data({'LQs': x[s:e], 'GT': gt[s:e]})
        model.optimize_parameters(step)
        if step == 1:
            out['gG'] = model.optimizer_G.buffers.grad.detach().cpu().numpy().copy()
            out['gD'] = model.optimizer_D.buffers.grad.detach().cpu().numpy().copy()
        out['G_after'].append(_flat(model.optimizer_G).numpy())
        out['D_after'].append(_flat(model.optimizer_D).numpy())
    out['nbt'] = sorted({int(v) for k, v in model.netD.state_dict().items() if 'num_batches_tracked' in k})
    out['log'] = dict(model.get_current_log())
    # numpy payloads: torch tensors travel through an fd-sharing side channel that dies with this process
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _reference(case):
    """Non-distributed models in this process, from the same weights: A and B stepped once on one shard each; C stepped once with its flat
    gradient buffers overwritten by (g_A + g_B) / 2 right before each optimizer's step."""
    from realvsr_amd.VideoSR_model import create_model
    torch.cuda.set_device(0)
    x, gt = _batch()
    grads, p0 = [], None
    for lo in (0, 2):
        m = create_model(_opt(case, False))
        _fill(m)
        p0 = p0 or (_flat(m.optimizer_G), _flat(m.optimizer_D))
        m.feed_data({'LQs': x[lo:lo + 2], 'GT': gt[lo:lo + 2]})
        m.optimize_parameters(1)
        grads.append((m.optimizer_G.buffers.grad.detach().clone(), m.optimizer_D.buffers.grad.detach().clone()))
    want = [(grads[0][i] + grads[1][i]) / 2 for i in (0, 1)]
    c = create_model(_opt(case, False))
    _fill(c)
    for o, w in ((c.optimizer_G, want[0]), (c.optimizer_D, want[1])):
        def step(o=o, w=w, inner=o.step):
            o.buffers.rebind()          # (first: a gradient that autograd adopted outside the flat buffer is copied home by the next rebind)
            o.buffers.grad.copy_(w)
            return inner()
        o.step = step
    c.feed_data({'LQs': x[0:2], 'GT': gt[0:2]})
    c.optimize_parameters(1)
    torch.cuda.synchronize()
    return {'gG': want[0].cpu(), 'gD': want[1].cpu(), 'G1': _flat(c.optimizer_G), 'D1': _flat(c.optimizer_D), 'G0': p0[0], 'D0': p0[1],
            'gG_A': grads[0][0].cpu(), 'gD_A': grads[0][1].cpu()}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize('case', CASES)
def test_two_ranks_one_gpu_match_the_mean_of_the_shards(case):
    got = run_ranks(_worker, 2, args=(case,), limit=600)
    got = {r: {k: ([torch.from_numpy(a) for a in v] if k.endswith('_after') else torch.from_numpy(v) if isinstance(v, np.ndarray) else v)
               for k, v in d.items()} for r, d in got.items()}
    ref = _reference(case)
    a, b = got[0], got[1]
    assert a['buckets_G'] > 3 and a['buckets_D'] > 3
    g_updated = 1 in G_STEPS[case]
    # step 1: the ranks' gradients, bit for bit, and against the mean of the two shards' gradients
    for k in ('gG', 'gD'):
        assert torch.equal(a[k], b[k]), k
        if k == 'gG' and not g_updated:
            # (D_init_iters: no G backward at step 1, so there is no G gradient to compare -- the buffer is the memset's zeros on both ranks,
            # and the G collectives of step 2 are covered by the parameter checks below)
            assert float(a[k].abs().max()) == 0.0 and float(ref[k].abs().max()) == 0.0
            continue
        err, one_shard = _rel(a[k], ref[k]), _rel(ref[k + '_A'], ref[k])
        print('%s %s: reduced gradient vs (g_A + g_B) / 2: rel l2 %.3e  (one shard alone: %.3e)' % (case, k, err, one_shard))
        assert one_shard > 100 * 2e-4, 'the shards are too alike for this comparison to mean anything'
        assert err <= 2e-4, (k, err)
    # step 1: parameters against the model that stepped on the expected gradients
    for k, k0, after in (('G1', 'G0', 'G_after'), ('D1', 'D0', 'D_after')):
        perr = _rel(a[after][0], ref[k])
        print('%s %s: parameters after step 1 vs a step on the expected gradients: rel l2 %.3e' % (case, k, perr))
        assert perr <= 1e-4, (k, perr)
        assert torch.equal(a[after][0], ref[k0]) == (k == 'G1' and not g_updated)       # (it did move, where it should)
    # every step: ranks bit-identical; G bit-unchanged exactly on the steps without a G update
    for i, step in enumerate((1, 2, 3)):
        assert torch.equal(a['G_after'][i], b['G_after'][i]) and torch.equal(a['D_after'][i], b['D_after'][i]), step
        before = ref['G0'] if i == 0 else a['G_after'][i - 1]
        for r in (a, b):
            assert torch.equal(r['G_after'][i], before) == (step not in G_STEPS[case]), step
        assert not torch.equal(a['D_after'][i], ref['D0'] if i == 0 else a['D_after'][i - 1])
    assert a['nbt'] == [NBT[case]], a['nbt']
    assert all(np.isfinite(v) for v in a['log'].values()) and 'l_d_real' in a['log'] and 'l_d_fake' in b['log']


# ---------------------------------------------------------------------------------------------------------------- RCCL, one rank
_RCCL_WORLD1 = r"""
import json, os, sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, os.path.join(%(repo)r, 'tests')); sys.path.insert(0, os.path.join(%(repo)r, 'tests', 'golden'))
import torch, torch.distributed as dist
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=%(port)r)
torch.cuda.set_device(0)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))   # nccl IS RCCL on ROCm
import test_gpu_gan_dist as T
from realvsr_amd.VideoSR_model import create_model
x, gt = T._batch()
grads, info, seen = {}, {}, []
inner = torch.Tensor.backward
for tag, on in (('plain', False), ('plain2', False), ('rccl', True)):
    torch.manual_seed(3)
    m = create_model(T._opt('ragan', on, force=on))
    T._fill(m)
    m.feed_data({'LQs': x, 'GT': gt})
    if on:
        def backward(self, *a, **k):          # what D's reducer had issued when each of the step's three backward passes began
            seen.append(m.reducer_D.issued)
            return inner(self, *a, **k)
        torch.Tensor.backward = backward
    m.optimize_parameters(1)
    torch.Tensor.backward = inner
    torch.cuda.synchronize()
    grads[tag] = (m.optimizer_G.buffers.grad.detach().cpu().clone(), m.optimizer_D.buffers.grad.detach().cpu().clone())
    if on:
        for k, r in (('G', m.reducer_G), ('D', m.reducer_D)):
            info[k] = {'active': r.active, 'world': r.world, 'buckets': len(r.buckets), 'issued_during_backward': r.stats_issued_in_backward,
                       'exposed_ms': r.exposed_ms()}
        info['backend'] = dist.get_backend()
    else:
        assert m.reducer_G is None and m.reducer_D is None
info['D_issued_at_backward_entry'] = seen
for i, k in enumerate(('G', 'D')):
    n = float(grads['plain'][i].double().norm())
    info['grad_rel_rccl_' + k] = float((grads['plain'][i].double() - grads['rccl'][i].double()).norm()) / n
    info['grad_rel_repeat_' + k] = float((grads['plain'][i].double() - grads['plain2'][i].double()).norm()) / n
info['rccl_loaded'] = any('librccl' in l for l in open('/proc/self/maps'))
print('RESULT ' + json.dumps(info), flush=True)
dist.destroy_process_group()
"""


def test_rccl_one_rank_forced_gan_step_matches_plain_step():
    """A one-rank `nccl` group on cuda:0, one RaGAN step with both reducers forced on (hooks, one asynchronous all_reduce per bucket on RCCL's
    stream, finish()) against the same step without reducers.  A one-rank sum times 1/1 is the identity, so the forced step may sit no
    further from a plain step than 4 x the distance of a second plain step (the DCN input gradient's f32 atomics make two plain runs differ
    in the last bits), with a floor of one f32 ulp of the gradient norm."""
    code = _RCCL_WORLD1 % {'repo': REPO, 'port': str(free_port())}
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'RVSR_DIST_CHECK'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    info = json.loads([l for l in out.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    print(info)
    assert info['backend'] == 'nccl' and info['rccl_loaded']
    for k in ('G', 'D'):
        assert info[k]['active'] and info[k]['world'] == 1 and info[k]['buckets'] > 3
        assert np.isfinite(info[k]['exposed_ms']) and info[k]['exposed_ms'] >= 0.0
        assert info['grad_rel_rccl_' + k] <= max(4 * info['grad_rel_repeat_' + k], 2.0 ** -23), (k, info)
    assert info['G']['issued_during_backward'] == info['G']['buckets']
    # D: nothing had left when the G backward, the first D pass and the second D pass began; buckets left during the second pass
    assert info['D_issued_at_backward_entry'] == [0, 0, 0]
    assert 0 < info['D']['issued_during_backward'] <= info['D']['buckets']


# ---------------------------------------------------------------------------------------------------------------- the driver
def _write_gan_option_file(root, resume_state=None):
    """The shipped GAN option file with the sizes shrunk, on the synthetic clip folders of test_gpu_train_driver.py (its _write_clips): 2
    training sequences x 10 frames of 56 x 72 (48 x 48 crops: the low band still holds the SSIM window), 2 validation clips, batch 4."""
    from test_gpu_train_driver import _write_clips
    with open(os.path.join(GOLDEN, 'options', 'train_EDVR-GAN_woTSA_RealVSR_YCbCr_Split.yml')) as f:
        opt = yaml.safe_load(f)
    data_root = os.path.join(str(root), 'data')
    if not os.path.isdir(data_root):
        _write_clips(data_root, ('000', '001'), 10, (56, 72), 1, seed=4)
        with open(os.path.join(data_root, 'keys.pkl'), 'wb') as f:
            pickle.dump({'keys': ['%s_%05d' % (s, i) for s in ('000', '001') for i in range(1, 9)]}, f)
        _write_clips(os.path.join(data_root, 'val'), ('003', '017'), 5, (16, 24), 1)
    opt['name'] = 'gan2'
    opt['use_tb_logger'] = False
    opt['gpu_ids'] = [0]
    opt['datasets']['train'].update(dataroot_GT=os.path.join(data_root, 'GT'), dataroot_LQ=os.path.join(data_root, 'LQ'),
                                    cache_keys=os.path.join(data_root, 'keys.pkl'), remove_list=None, n_workers=0, batch_size=4,
                                    GT_size=48, LQ_size=48, frame_chw=[3, 56, 72])
    opt['datasets']['val'].update(dataroot_GT=os.path.join(data_root, 'val', 'GT'), dataroot_LQ=os.path.join(data_root, 'val', 'LQ'))
    opt['network_G'].update(front_RBs=1, back_RBs=1)
    opt['network_D'].update(nf=16)
    opt['path']['pretrain_model_G'] = None
    opt['path']['resume_state'] = resume_state
    opt['train'].update(lr_G=2e-4, lr_D=2e-4, niter=4 if resume_state is None else 6, val_freq=2, bucket_mb=0.05,
                        T_period=[50, 30, 40], restarts=[50, 80], restart_weights=[1, 0.5])
    opt['logger'].update(print_freq=1, save_checkpoint_freq=2)
    opt['augment'] = None
    path = os.path.join(str(root), 'gan2.yml')
    with open(path, 'w') as f:
        yaml.safe_dump(opt, f)
    return path


def _run_driver(root, option_file):
    env = dict(os.environ, RVSR_DIST_CHECK='1', PYTHONPATH=os.pathsep.join([REPO] + [p for p in [os.environ.get('PYTHONPATH')] if p]))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc_per_node=2', '--master-addr', '127.0.0.1', '--master-port',
           str(free_port()), '-m', 'realvsr_amd.train', '-opt', option_file, '--launcher', 'pytorch', '--dist-backend', 'gloo', '--root', str(root)]
    out = subprocess.run(cmd, env=env, cwd=str(root), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-4000:])
    return out.stdout + out.stderr


CHECKSUM = re.compile(r'rank (\d): iter (\d+), parameter checksums (-?\d+) (-?\d+)')
ITER_LINE = re.compile(r'<epoch:\s*(\d+), iter:\s*([\d,]+), lr:')


def test_driver_two_gloo_ranks_trains_validates_checkpoints_and_resumes(tmp_path):
    exp = os.path.join(str(tmp_path), 'experiments', 'gan2')
    text = _run_driver(tmp_path, _write_gan_option_file(tmp_path))
    assert sorted(os.listdir(os.path.join(exp, 'models'))) == ['2_D.pth', '2_G.pth', '4_D.pth', '4_G.pth', 'latest_D.pth', 'latest_G.pth']
    assert sorted(os.listdir(os.path.join(exp, 'training_state'))) == ['2.state', '4.state']
    logs = glob.glob(os.path.join(exp, 'train_gan2_*.log'))
    assert len(logs) == 1                                            # rank 0 alone writes a log file
    with open(logs[0]) as f:
        log = f.read()
    assert [int(v[1]) for v in ITER_LINE.findall(log)] == [1, 2, 3, 4] and 'l_d_fake:' in log and 'l_g_gan:' in log
    assert len(re.findall(r'# Validation # PSNR: \d+\.\d\d dB,  003: \d+\.\d\d dB,  017: \d+\.\d\d dB', log)) == 2     # rank 0 validated
    assert len(re.findall(r'# Validation # PSNR', text)) == 2 and len(re.findall(r'Saving models and training states', text)) == 2
    sums = {int(r): (int(it), g, d) for r, it, g, d in CHECKSUM.findall(text)}
    assert sorted(sums) == [0, 1] and sums[0] == sums[1] and sums[0][0] == 4, sums
    four = dict(sums)

    resume = os.path.join(exp, 'training_state', '4.state')
    text = _run_driver(tmp_path, _write_gan_option_file(tmp_path, resume_state=resume))
    assert 'Resuming training from epoch: 0, iter: 4.' in text and '4_G.pth' in text and '4_D.pth' in text
    newest = sorted(glob.glob(os.path.join(exp, 'train_gan2_*.log')), key=os.path.getmtime)[-1]
    with open(newest) as f:
        assert [int(v[1]) for v in ITER_LINE.findall(f.read())] == [5, 6]
    sums = {int(r): (int(it), g, d) for r, it, g, d in CHECKSUM.findall(text)}
    assert sorted(sums) == [0, 1] and sums[0] == sums[1] and sums[0][0] == 6, sums
    assert sums[0][1:] != four[0][1:]                                # both networks moved on from iteration 4
    state = torch.load(os.path.join(exp, 'training_state', '6.state'), map_location='cpu', weights_only=False)
    assert state['iter'] == 6 and len(state['optimizers']) == 2
    assert [float(o['state'][0]['step']) for o in state['optimizers']] == [6.0, 6.0]       # 4 resumed + 2 taken, G and D


# ---------------------------------------------------------------------------------------------------------------- the tool
TOOL_KEYS = {'metric', 'batch', 'frames', 'size', 'ms_step', 'g_ms', 'd_ms', 'd_share', 'loss_terms', 'conv5', 'steps', 'warmup'}


def _tool(extra, env_extra):
    env = dict(os.environ, **env_extra)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT') + (() if env_extra else ('RVSR_BENCH_BACKEND',)):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'gan_step.py'), '--steps', '2', '--warmup', '1', '--batch', '2',
                          '--size', '48'] + extra, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_gan_step_tool_starts_two_ranks():
    rec = _tool(['--gpus', '2'], {'RVSR_BENCH_BACKEND': 'gloo'})
    assert TOOL_KEYS <= set(rec) and rec['n_gpus'] == 2 and rec['batch'] == 2 and rec['batch_per_gpu'] == 1
    ar = rec['allreduce']
    assert ar['backend'] == 'gloo' and ar['params_identical_after_last_step'] is True
    for k in ('G', 'D'):
        assert ar[k]['world'] == 2 and ar[k]['buckets'] >= 1 and len(ar[k]['bucket_bytes']) == ar[k]['buckets']
        assert 0 <= ar[k]['issued_during_backward'] <= ar[k]['buckets'] and ar[k]['exposed_ms'] >= 0.0


def test_gan_step_tool_plain_line_keeps_its_keys():
    rec = _tool([], {})
    assert TOOL_KEYS <= set(rec) and rec['n_gpus'] == 1 and 'allreduce' not in rec
    assert rec['ms_step'] > 0 and set(rec['loss_terms']) >= {'l_g_total', 'l_d_real', 'l_d_fake'}
