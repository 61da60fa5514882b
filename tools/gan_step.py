#!/usr/bin/env python
"""One JSON line for the GAN stage at the shape of train_EDVR-GAN_woTSA_RealVSR_YCbCr_Split.yml: batch 32, 3 x 192^2 frames, scale 1,
G = EDVR_NoUp nf 64 (front 5 / back 10, no TSA), D = MultiscaleDiscriminator_v4 nf 64, num_D 2, RaGAN, SSIM + Charbonnier + GWLoss.

  ms_step          wall time per VideoSRGANModel.optimize_parameters(step, log=False) (device-bound: events around K steps)
  g_ms / d_ms      device time of the G half (G forward, pyramids, pixel terms, 2 D forwards, backward, Adam) and of the D half
                   (3 D forwards, 2 backwards, Adam), from events recorded where the model switches D's requires_grad
  conv5_*_tflops   achieved rate of the 5x5 forward / weight-gradient kernels on two D layers at this shape

  n_gpus           ranks (one process per GPU); every rank runs batch B // N, ms_step is the slowest rank's
  allreduce        (N > 1 or --force-allreduce) per reducer, G and D: buckets, bucket_bytes, issued_during_backward (buckets enqueued from a
                   gradient hook in the last step; for D that is the second of its two backward passes), exposed_ms (stream time inside
                   finish(), mean over the timed steps, rank 0), world; plus the backend and params_identical_after_last_step, a bitwise
                   comparison of both flat parameter buffers over the ranks

usage: python tools/gan_step.py [--steps K] [--warmup W] [--batch B] [--size S] [--gpus N] [--force-allreduce]

--gpus N > 1 without a launcher (WORLD_SIZE unset): the tool starts its N ranks as child processes through python -m torch.distributed.run.
RVSR_BENCH_BACKEND=gloo puts all ranks on GPU 0 (a rehearsal of the N > 1 code path on a one-GPU box, not a scaling number); the default
backend is nccl (RCCL), one GPU per rank.  --force-allreduce runs both reducers over RCCL in a one-rank group.
"""
import argparse
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from step_timing import clip_batch  # noqa: E402


def conv5_rates(B, reps=5):
    """(forward, weight gradient) TFLOP/s of two discriminator layers: 64 -> 64 at S/2 and 256 -> 256 at S/4."""
    from realvsr_amd import functional as RF
    d = torch.device('cuda', 0)
    out = {}
    for C, Co, H in ((64, 64, 96), (256, 256, 48)):
        conv = torch.nn.Conv2d(C, Co, 5, 1, 2, bias=False).to(d)
        x = torch.randn(B, C, H, H, device=d)
        flop = 2.0 * B * Co * C * 25 * H * H
        y = RF.conv2d(x, conv)
        gout = torch.randn_like(y)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            y = RF.conv2d(x, conv)
        ev[1].record()
        for _ in range(reps):
            conv.weight.grad = None
            y.backward(gout, retain_graph=True)     # x needs no gradient: the weight gradient alone
        ev[2].record()
        torch.cuda.synchronize()
        fwd_ms, wg_ms = ev[0].elapsed_time(ev[1]) / reps, ev[1].elapsed_time(ev[2]) / reps
        key = '%d-%d@%d' % (C, Co, H)
        out[key] = {'fwd_ms': round(fwd_ms, 3), 'fwd_tflops': round(flop / fwd_ms / 1e9, 1),
                    'wgrad_ms': round(wg_ms, 3), 'wgrad_tflops': round(flop / wg_ms / 1e9, 1)}
    return out


def relaunch(gpus):
    """`--gpus N` without a launcher: the N ranks are children of this process (which never touches the GPU itself)."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    raise SystemExit(subprocess.call(cmd, env=env))


def params_identical(model):
    """Do all ranks hold the same bits in both flat parameter buffers?  One all-reduce: MAX over [v, -v] gives max(v) and -min(v)."""
    v = torch.cat([o.buffers.param.view(torch.int32) for o in model.optimizers]).to(torch.int64)
    t = torch.cat([v, -v])
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    n = v.numel()
    return bool(torch.equal(t[:n], -t[n:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1, help='ranks, one process per GPU; each runs batch B // N')
    ap.add_argument('--force-allreduce', action='store_true',
                    help='N = 1: a one-rank RCCL process group, both bucketed all-reduces inside every step (arithmetically the identity)')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=192)
    a = ap.parse_args()
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        relaunch(a.gpus)
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (('WORLD_SIZE', '1'), ('RANK', '0'), ('LOCAL_RANK', '0')))
    if a.gpus != world:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d' % (a.gpus, world))
    if a.batch % world:
        raise SystemExit('--batch %d does not divide over %d ranks' % (a.batch, world))
    ndev = torch.cuda.device_count()
    backend = os.environ.get('RVSR_BENCH_BACKEND', 'nccl')
    if backend == 'nccl' and world > ndev:
        raise SystemExit('gan_step.py --gpus %d: %d ranks over RCCL need one GPU each, but %d are visible.  Set RVSR_BENCH_BACKEND=gloo to '
                         'rehearse the N > 1 path with all ranks sharing GPU 0 (not a scaling number).' % (a.gpus, world, ndev))
    local = local % max(ndev, 1)
    torch.cuda.set_device(local)
    use_pg = world > 1 or a.force_allreduce
    if use_pg:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29512')
        if backend == 'nccl':
            torch.distributed.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', local))
        else:
            torch.distributed.init_process_group(backend, rank=rank, world_size=world)
    from realvsr_amd.VideoSR_model import create_model
    train = {'lr_G': 5e-5, 'weight_decay_G': 0, 'beta1_G': 0.9, 'beta2_G': 0.99, 'lr_D': 5e-5, 'weight_decay_D': 0, 'beta1_D': 0.9,
             'beta2_D': 0.99, 'pixel_criterion_s': 'ssim', 'pixel_weight_s': 1.0, 'pixel_criterion_d': 'cb', 'pixel_weight_d': 1.0,
             'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0, 'feature_criterion': 'cb', 'feature_weight': 0.0, 'gan_type': 'ragan',
             'gan_weight': 1e-4, 'force_allreduce': a.force_allreduce}
    opt = {'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'dist': use_pg, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
           'network_G': {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 5, 'back_RBs': 10,
                         'predeblur': False, 'HR_in': False, 'w_TSA': False},
           'network_D': {'which_model_D': 'MultiscaleDiscriminator_v4', 'in_nc': 1, 'nf': 64, 'num_D': 2, 'gan_type': 'patch'},
           'path': {}, 'train': train}
    torch.manual_seed(0 if rank == 0 else 12345 + rank)   # ranks > 0 start from different weights: the model broadcasts rank 0's
    model = create_model(opt)
    B, S = a.batch // world, a.size
    data = clip_batch(B, S, 1 + rank)

    # events where the model switches D's requires_grad: False = start of the G half, True = start of the D half
    marks = []
    switch = model._set_requires_grad_D

    def marked(flag):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((flag, e))
        switch(flag)
    model._set_requires_grad_D = marked

    for step in range(1, a.warmup + 1):
        model.feed_data(data)
        model.optimize_parameters(step, log=False)
    torch.cuda.synchronize()
    marks.clear()
    for r in (model.reducer_G, model.reducer_D):
        if r is not None:
            r.reset_stats()
    if world > 1:
        torch.distributed.barrier()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ends = []
    t0.record()
    for step in range(a.warmup + 1, a.warmup + a.steps + 1):
        model.feed_data(data)
        model.optimize_parameters(step, log=False)
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        ends.append(e)
    t1.record()
    torch.cuda.synchronize()
    g_ms = d_ms = 0.0
    for i in range(a.steps):
        (_, eg), (_, ed) = marks[2 * i], marks[2 * i + 1]
        g_ms += eg.elapsed_time(ed)
        d_ms += ed.elapsed_time(ends[i])
    ms = t0.elapsed_time(t1) / a.steps
    allreduce = None
    if use_pg:
        allreduce = {'backend': backend + (' (RCCL)' if backend == 'nccl' else ''), 'params_identical_after_last_step': params_identical(model)}
        for k, r in (('G', model.reducer_G), ('D', model.reducer_D)):
            allreduce[k] = {'buckets': len(r.buckets), 'bucket_bytes': [4 * (e - s) for s, e in r.buckets],
                            'issued_during_backward': r.stats_issued_in_backward, 'exposed_ms': round(r.exposed_ms(), 3), 'world': r.world}
        if world > 1:
            t = torch.tensor([ms], device='cuda', dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            ms = t.item()
    if rank == 0:
        report(a, model, world, B, S, ms, g_ms, d_ms, allreduce)
    if use_pg:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def report(a, model, world, B, S, ms, g_ms, d_ms, allreduce):
    res = {'metric': 'gan_step', 'batch': B * world, 'frames': 3, 'size': S, 'ms_step': round(ms, 2), 'g_ms': round(g_ms / a.steps, 2),
           'd_ms': round(d_ms / a.steps, 2), 'd_share': round(d_ms / (g_ms + d_ms), 3),
           'loss_terms': {k: round(float(v), 5) for k, v in model.loss_terms.items()},
           'conv5': conv5_rates(B), 'steps': a.steps, 'warmup': a.warmup, 'n_gpus': world, 'batch_per_gpu': B}
    if allreduce is not None:
        res['allreduce'] = allreduce
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
