#!/usr/bin/env python
"""One JSON line for the device-side validation metrics (realvsr_amd.metrics) on a synthetic 2160 x 3840 Y plane.

  psnr_ms            rvsr_psnr_sse on the plane pair (both launches: partial sums + finish)
  ssim_ms            rvsr_ssim_sum on the plane pair (both launches: tiles + finish)
  ssim_tbps          two f32 planes read once, over ssim_ms: the share of the ~6.3 TB/s a stream reaches says how far the f64 arithmetic
                     keeps the kernel from its HBM floor (~10 us)
  frame_metrics_ms   host wall time of metrics.frame_metrics (both metrics, the copy of the scalars and its synchronisation included)
  d2h_f32_ms         host wall time of the copy the reference's path starts with: a [3, 2160, 3840] f32 output to pageable host memory
                     (get_current_visuals / single_forward's .cpu()); the numpy filters that follow it there are not timed
  loss_ssim_fwd_ms   the f32, 121-tap, untiled rvsr_ssim_forward of the training loss on the same plane pair, for comparison
Kernel times: device events around `--inner` back-to-back calls, divided; the median of `--reps` such samples after warm-up.
Each value is measured in a child process of its own under its own time limit; a child that fails ends the run (nothing further is
started on the GPU) and the line reports which one.

usage: python tools/eval_clip.py [--height H] [--width W] [--reps R] [--inner K] [--timeout S]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEASUREMENTS = ('psnr', 'ssim', 'frame_metrics', 'd2h_f32', 'loss_ssim_fwd')


def _event_ms(fn, reps, inner, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    samples = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        torch.cuda.synchronize()
        samples.append(t0.elapsed_time(t1) / inner)
    return sorted(samples)


def _wall_ms(fn, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    samples = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t) * 1e3)
    return sorted(samples)


def measure(name, H, W, reps, inner):
    import torch
    from realvsr_amd import _lib, metrics
    from realvsr_amd._lib import _p, _stream
    torch.cuda.set_device(0)
    d = torch.device('cuda', 0)
    g = torch.Generator(device='cuda').manual_seed(4)
    fake = torch.rand(1, 3, H, W, device=d, generator=g)
    real = (fake + 0.02 * torch.randn(1, 3, H, W, device=d, generator=g)).clamp_(0, 1)
    L = _lib.lib()
    a, b = fake[:, 0], real[:, 0]
    ws = torch.empty(max(L.rvsr_metric_workspace_bytes(1, H, W, 0), L.rvsr_reduce_workspace_bytes()), dtype=torch.uint8, device=d)
    out = torch.zeros(2, dtype=torch.int64, device=d)
    res = {}
    if name == 'psnr':
        s = _event_ms(lambda: _lib.check(L.rvsr_psnr_sse(_p(a), 3 * H * W, _p(b), 3 * H * W, 1, H, W, 0, _p(out[0:1]), _p(ws), ws.numel(),
                                                         _stream()), 'psnr_sse'), reps, inner)
    elif name == 'ssim':
        s = _event_ms(lambda: _lib.check(L.rvsr_ssim_sum(_p(a), 3 * H * W, _p(b), 3 * H * W, 1, H, W, 0, _p(out[1:2]), _p(ws), ws.numel(),
                                                         _stream()), 'ssim_sum'), reps, inner)
        res['ssim_tbps'] = round(2 * H * W * 4 / (s[len(s) // 2] * 1e-3) / 1e12, 3)
    elif name == 'frame_metrics':
        s = _wall_ms(lambda: metrics.frame_metrics(fake, real), reps)
        res['values'] = metrics.frame_metrics(fake, real)
    elif name == 'd2h_f32':
        s = _wall_ms(lambda: fake[0].cpu(), max(3, reps // 4))
    elif name == 'loss_ssim_fwd':
        x, y, o = a.contiguous(), b.contiguous(), torch.zeros(1, device=d)
        scale = 1.0 / ((H - 10) * (W - 10))
        s = _event_ms(lambda: _lib.check(L.rvsr_ssim_forward(_p(x), _p(y), 1, H, W, scale, _p(o), None, None, None, _p(ws), _stream()),
                                         'ssim_forward'), reps, max(1, inner // 4))
    else:
        raise ValueError(name)
    res[name + '_ms'] = round(s[len(s) // 2], 4)
    res[name + '_ms_min_max'] = [round(s[0], 4), round(s[-1], 4)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=2160)
    ap.add_argument('--width', type=int, default=3840)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--timeout', type=float, default=120.0, help='seconds for each measurement')
    ap.add_argument('--only', choices=MEASUREMENTS, help='(internal) run one measurement in this process')
    a = ap.parse_args()
    if a.only:
        print(json.dumps(measure(a.only, a.height, a.width, a.reps, a.inner)))
        return 0
    res = {'metric': 'eval_clip', 'height': a.height, 'width': a.width, 'reps': a.reps, 'inner': a.inner,
           'floor_us_at_6p3_tbps': round(2 * a.height * a.width * 4 / 6.3e12 * 1e6, 2)}
    rc = 0
    for name in MEASUREMENTS:
        cmd = [sys.executable, os.path.abspath(__file__), '--only', name, '--height', str(a.height), '--width', str(a.width),
               '--reps', str(a.reps), '--inner', str(a.inner)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.timeout, universal_newlines=True)
        except subprocess.TimeoutExpired:
            res['failed'], rc = '%s: no result within %g s' % (name, a.timeout), 1
            break
        if p.returncode != 0:
            res['failed'], rc = '%s: exit %d: %s' % (name, p.returncode, p.stderr.strip().splitlines()[-1:] or ''), 1
            break
        res.update(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(res))
    return rc


if __name__ == '__main__':
    sys.exit(main())
