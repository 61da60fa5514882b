"""The N > 1 path on real kernels: two ranks sharing ONE MI355X over gloo (the driver has no multi-GPU box for tests), and RCCL
itself in a one-rank group with the reducer's hook path forced on (`BucketedGradAllReduce(force=True)`).  -m gpu

  * the real EDVR training step through VideoSRModel(dist) -> FlatAdam buffers -> BucketedGradAllReduce hooks on the
    custom autograd Functions: averaged gradients == full-batch gradients, ranks end with identical parameters
  * `python bench.py --gpus 2` with WORLD_SIZE unset spawns its own ranks and reports n_gpus = 2
  * a plain `bench.py` run prints the headline only and `--dump-outputs` writes what its last timed step computed
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO
from gpu_util import dev

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _opt(dist):
    net = dict(which_model_G='EDVR', nf=16, nc=3, nframes=3, groups=4, front_RBs=1, back_RBs=1, center=None, predeblur=False,
               HR_in=False, w_TSA=True)
    return {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': dist, 'gpu_ids': [0], 'is_train': True, 'scale': 4, 'augment': None,
            'network_G': net, 'path': {'pretrain_model_G': None, 'strict_load': True},
            'train': {'pixel_criterion_y': 'lappyr', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 0.5,
                      'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-3, 'beta1': 0.9, 'beta2': 0.99, 'bucket_mb': 0.05}}


def _data():
    g = torch.Generator().manual_seed(11)
    return torch.rand(4, 3, 3, 24, 32, generator=g), torch.rand(4, 3, 96, 128, generator=g)


def _build(dist, seed):
    sys.path.insert(0, os.path.join(REPO, 'tests', 'golden'))
    from weights import fill_state_dict
    from realvsr_amd.VideoSR_model import create_model
    torch.manual_seed(seed)
    model = create_model(_opt(dist))
    return model, fill_state_dict


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from realvsr_amd.dist import shard_range, broadcast_parameters
    model, fill = _build(True, seed=100 + rank)          # different initial weights per rank ...
    if rank == 0:
        fill(model.netG, 808, offset_std=0.02)
    broadcast_parameters(model.netG)                     # ... until rank 0's are broadcast
    assert len(model.reducer.buckets) > 3
    x, gt = _data()
    s, e = shard_range(4, rank, world)
    model.feed_data({'LQs': x[s:e], 'GT': gt[s:e]})
    for step in (1, 2):
        model.optimize_parameters(step)
        if step == 1:
            grads = model.optimizer_G.buffers.grad.detach().cpu().clone()
    # numpy payloads: torch tensors travel through an fd-sharing side channel that dies with this process
    q.put((rank, grads.numpy(), model.optimizer_G.buffers.param.detach().cpu().numpy(), model.get_current_log()['l_pix']))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_match_full_batch():
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, grads, params, l = q.get(timeout=600)
        got[r] = (torch.from_numpy(grads), torch.from_numpy(params), l)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    # single process, full batch of 4
    torch.cuda.set_device(0)
    model, fill = _build(False, seed=7)
    fill(model.netG, 808, offset_std=0.02)
    x, gt = _data()
    model.feed_data({'LQs': x, 'GT': gt})
    model.optimize_parameters(1)
    ref_g = model.optimizer_G.buffers.grad.detach().cpu().clone()
    model.optimize_parameters(2)
    ref_p = model.optimizer_G.buffers.param.detach().cpu()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])      # ranks agree bit for bit
    err = ((got[0][0].double() - ref_g.double()).norm() / ref_g.double().norm()).item()
    print('averaged gradient vs full-batch gradient: rel l2 err %.3e' % err)
    assert err <= 2e-4, err
    # two Adam steps from the same start: updates agree
    perr = ((got[0][1].double() - ref_p.double()).norm() / ref_p.double().norm()).item()
    print('parameters after 2 steps, 2 ranks vs 1: rel l2 err %.3e' % perr)
    assert perr <= 1e-4, perr


_RCCL_WORLD1 = r"""
import json, os, sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, os.path.join(%(repo)r, 'tests')); sys.path.insert(0, os.path.join(%(repo)r, 'tests', 'golden'))
import torch, torch.distributed as dist
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=%(port)r)
torch.cuda.set_device(0)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))   # nccl IS RCCL on ROCm
from weights import fill_state_dict
from realvsr_amd.VideoSR_model import create_model
net = dict(which_model_G='EDVR', nf=64, nc=3, nframes=5, groups=8, front_RBs=2, back_RBs=3, center=None, predeblur=False, HR_in=False, w_TSA=True)
def opt(dist_on):
    return {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': dist_on, 'gpu_ids': [0], 'is_train': True, 'scale': 4, 'augment': None,
            'network_G': net, 'path': {'pretrain_model_G': None, 'strict_load': True},
            'train': {'pixel_criterion_y': 'lappyr', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 0.5, 'weight_decay_G': 0,
                      'ft_tsa_only': 0, 'lr_G': 1e-3, 'beta1': 0.9, 'beta2': 0.99, 'bucket_mb': 0.5, 'force_allreduce': dist_on}}
g = torch.Generator().manual_seed(11)
x, gt = torch.rand(2, 5, 3, 48, 64, generator=g), torch.rand(2, 3, 192, 256, generator=g)
res, grads = {}, {}
for tag, on in (('plain', False), ('plain2', False), ('rccl', True)):
    torch.manual_seed(3)
    m = create_model(opt(on))
    fill_state_dict(m.netG, 808, offset_std=0.02)
    m.feed_data({'LQs': x, 'GT': gt})
    for step in (1, 2):
        m.optimize_parameters(step)
        if step == 1:
            grads[tag] = m.optimizer_G.buffers.grad.detach().cpu().clone()     # (after the all-reduce, before the next zero_grad)
    torch.cuda.synchronize()
    res[tag] = m.optimizer_G.buffers.param.detach().cpu().clone()
    if on:
        r = m.reducer
        info = {'active': r.active, 'world': r.world, 'buckets': len(r.buckets), 'issued_during_backward': r.stats_issued_in_backward,
                'exposed_ms': r.exposed_ms(), 'backend': dist.get_backend()}
    else:
        assert m.reducer is None
info['identical'] = bool(torch.equal(res['plain'], res['rccl']))
# (the DCN input gradient is flushed with f32 global atomics where the halos of up to four workgroups overlap: two plain runs need not agree
# in the last bit, so the all-reduce is held to "no further than a plain repeat")
info['repeat_identical'] = bool(torch.equal(res['plain'], res['plain2']))
info['diff_rccl'] = float((res['plain'].double() - res['rccl'].double()).abs().max())
info['diff_repeat'] = float((res['plain'].double() - res['plain2'].double()).abs().max())
gn = float(grads['plain'].double().norm())
info['grad_rel_rccl'] = float((grads['plain'].double() - grads['rccl'].double()).norm()) / gn
info['grad_rel_repeat'] = float((grads['plain'].double() - grads['plain2'].double()).norm()) / gn
# the collective itself, bit for bit: a one-rank sum must return its input (async, on RCCL's stream, like the reducer's buckets)
t = torch.randn(1 << 20, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
t0 = t.clone()
dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True).wait()
torch.cuda.synchronize()
info['allreduce_identity_exact'] = bool(torch.equal(t, t0))
info['rccl_loaded'] = any('librccl' in l for l in open('/proc/self/maps'))
print('RESULT ' + json.dumps(info), flush=True)
dist.destroy_process_group()
"""


def test_rccl_one_rank_forced_allreduce_matches_plain_step():
    """RCCL on hardware before a multi-GPU node exists (reference: codes/train.py:19-26 init_dist(backend='nccl')): a
    one-rank `nccl` process group on cuda:0, a real EDVR (nf64, 5 frames, TSA) `optimize_parameters` with the reducer forced on -- gradient
    hooks, one asynchronous all_reduce per bucket on RCCL's stream, finish() -- against the same two steps without a reducer: parameters
    bit-identical (a one-rank sum times 1/1), at least one bucket issued from a hook while backward was still running, a finite exposed time,
    and librccl mapped into the process."""
    import math
    code = _RCCL_WORLD1 % {'repo': REPO, 'port': str(_free_port())}
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    info = json.loads([l for l in out.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    print(info)
    assert info['backend'] == 'nccl' and info['active'] and info['world'] == 1 and info['rccl_loaded']
    assert info['buckets'] > 3 and 1 <= info['issued_during_backward'] <= info['buckets']
    assert math.isfinite(info['exposed_ms']) and info['exposed_ms'] >= 0.0
    assert info['allreduce_identity_exact']
    if info['repeat_identical']:
        assert info['identical'], 'the forced one-rank all-reduce changed the parameters'
    else:
        # The plain step is not bit-reproducible: the DCN input gradient is flushed with f32 global atomics where the windows of up to four
        # workgroups overlap (measured: two plain runs differ by ~1e-7 of the gradient norm, which Adam's g / sqrt(v) turns into up to 2 lr on
        # elements whose gradient is ~0).  The forced all-reduce may not add to that: its run must sit no further from a plain run than a
        # second plain run does.
        assert info['grad_rel_repeat'] <= 1e-5, info
        assert info['grad_rel_rccl'] <= 4 * info['grad_rel_repeat'] + 1e-12, info
        # (the parameter difference is the MAXIMUM over 3.3 M elements of a heavy-tailed quantity -- an element whose gradient is ~0 moves by up to
        # 2 lr on a 1e-7 perturbation -- so two samples of it differ by more than the gradients do: 1.1e-3 against 2.7e-4 was seen once in round 6
        # with both gradient errors at 1e-10; the gradients carry the 4 x bound, the parameters an absolute one of a few Adam steps)
        assert info['diff_rccl'] <= max(10 * info['diff_repeat'], 5e-3) + 1e-12, info


def test_bench_force_allreduce_line():
    """`bench.py --gpus 1 --force-allreduce`: the driver's N = 1 line with the all-reduce inside every timed step, over RCCL."""
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'RVSR_BENCH_BACKEND'):
        env.pop(k, None)
    env['MASTER_PORT'] = str(_free_port())
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--force-allreduce', '--steps', '2', '--warmup', '1',
                          '--batch', '1', '--height', '32', '--width', '48', '--no-cpu-baseline', '--no-extra', '--no-sweep'],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    ar = rec['allreduce']
    assert rec['n_gpus'] == 1 and ar['world'] == 1 and ar['backend'].startswith('nccl')
    assert ar['buckets'] >= 1 and ar['bytes'] == sum(ar['bucket_bytes']) and ar['params_identical_after_last_step'] is True
    assert 1 <= ar['issued_during_backward'] <= ar['buckets'] and ar['exposed_ms'] >= 0.0


def test_bench_self_launches_n_ranks():
    env = dict(os.environ, RVSR_BENCH_BACKEND='gloo')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '1',
                          '--height', '32', '--width', '48', '--full', '--no-cpu-baseline', '--no-extra'], env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('{')][-1]
    rec = json.loads(line)
    assert rec['n_gpus'] == 2 and rec['config']['global_batch'] == 2 and rec['config']['parallelism'] == 'sequence-dp2'
    assert rec['value'] > 0 and rec['roofline']['launches'] == 2 * 4
    # evidence for the day the scaling run happens: what was all-reduced, how much of it during backward, what stayed exposed
    ar = rec['allreduce']
    assert ar['buckets'] >= 1 and ar['bytes'] == sum(ar['bucket_bytes']) and ar['params_identical_after_last_step'] is True
    assert 0 <= ar['issued_during_backward'] <= ar['buckets'] and ar['exposed_ms'] >= 0.0


def test_bench_line_carries_offset_sweep_and_f32_step():
    """The driver-timed line (N = 1) runs at 1 px mean offsets and reports the raw-init and large-motion steps, the exact-f32 step, the
    LDS roofline object and the config-3 / config-5 side lines next to the headline."""
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '2', '--warmup', '1', '--batch', '1',
                          '--height', '32', '--width', '48', '--full', '--no-cpu-baseline'], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert abs(rec['config']['offset_abs_mean_px'] - 1.0) < 0.2 and rec['config']['offset_px_requested'] == 1.0
    assert set(rec['offset_sweep']) == {'raw_init', '3px'}
    for k, v in rec['offset_sweep'].items():
        assert v['ms_per_step'] > 0 and v['dcn_bwd_ms'] > 0 and 0 < v['dcn_fwd_frac'] < 1
        if k == 'raw_init':
            assert v['offset_abs_mean_px'] < 0.1
        else:
            assert abs(v['offset_abs_mean_px'] - float(k[:-2])) < 0.2 * float(k[:-2])
    assert 0 < rec['roofline_lds']['frac'] < 1 and rec['roofline_lds']['bound'] == 'lds'
    assert rec['extra']['config3']['ms_per_step'] > 0 and rec['extra']['config5']['ms_per_frame'] > 0 and rec['extra']['config5']['graph_bit_identical']
    assert rec['f32_mode_ms_per_step'] > 0 and rec['roofline']['dcn_bwd_ms_per_step'] > 0
    assert 'allreduce' not in rec


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """A plain `bench.py --steps K --warmup W` run: the headline line of exactly K timed steps, none of the --full objects; `--dump-outputs DIR`
    writes the last timed step's output, loss terms and parameter gradients -- and a second run with the same arguments writes the same
    arrays (every step starts from the same state: same inputs, so the same results up to the rounding of the DCN input gradient's atomics)."""
    import numpy as np
    from realvsr_amd.archs.EDVR_arch import EDVR
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    runs = []
    for tag in ('a', 'b'):
        d = tmp_path / tag
        out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '1',
                              '--height', '32', '--width', '48', '--dump-outputs', str(d)], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
        assert sorted(os.listdir(d)) == ['grads.npy', 'l_pix.npy', 'l_pix_c.npy', 'l_pix_y.npy', 'output.npy']
        runs.append((rec, {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}))
    rec, arrs = runs[0]
    assert rec['steps'] == 3 and rec['warmup'] == 1 and rec['n_gpus'] == 1 and rec['higher_is_better'] is True
    assert rec['unit'] == 'HR frames/s' and rec['dtype'].startswith('f32') and rec['metric'].startswith('HR frames/sec')
    assert rec['ms_per_step'] > 0 and abs(rec['value'] * rec['ms_per_step'] / 1e3 - 1.0) < 1e-2   # value = B / (ms_per_step / 1e3), B = 1
    assert not {'roofline', 'roofline_lds', 'roofline_conv', 'offset_sweep', 'f32_mode_ms_per_step', 'speed_modes', 'cpu_baseline', 'parity',
                'extra', 'allreduce'} & set(rec)
    assert sum(a.nbytes for a in arrs.values()) < 64 * 2 ** 20
    nparam = sum(p.numel() for p in EDVR(nf=64, nc=3, nframes=5, groups=8, front_RBs=5, back_RBs=10, w_TSA=True).parameters())
    assert arrs['output'].dtype == np.float32 and arrs['output'].shape == (1 * 3 * 128 * 192,)
    assert arrs['grads'].dtype == np.float32 and arrs['grads'].shape == (nparam,)
    assert all(np.isfinite(a).all() for a in arrs.values()) and np.abs(arrs['grads']).max() > 0
    for k in ('l_pix', 'l_pix_y', 'l_pix_c'):
        assert arrs[k].dtype == np.float64 and arrs[k].shape == (1,)
    assert abs(arrs['l_pix'][0] - (arrs['l_pix_y'][0] + arrs['l_pix_c'][0])) <= 1e-6 * abs(arrs['l_pix'][0])
    assert abs(arrs['l_pix'][0] - rec['config']['loss_last_step']) <= 1e-6
    # run to run: the forward is deterministic, the gradients carry the rounding of the atomic scatter only
    other = runs[1][1]
    for k in ('output', 'l_pix', 'l_pix_y', 'l_pix_c'):
        assert np.array_equal(arrs[k], other[k]), k
    g, h = arrs['grads'].astype(np.float64), other['grads'].astype(np.float64)
    assert np.abs(g - h).max() <= 1e-5 * np.abs(h).max() and np.linalg.norm(g - h) <= 1e-5 * np.linalg.norm(h)
