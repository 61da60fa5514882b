#!/usr/bin/env python
"""One JSON line for TOF at the shape of train_TOF_RealVSR_YCbCr_Split.yml: batch 32, 3 x 192^2 frames, scale 1, nc 3, nf 64, nb 10, K 3,
LapPyr(ssim, cb) on Y + GWLoss on CbCr through VideoSRModel.

  ms_step                wall time per VideoSRModel.optimize_parameters(step, log=False) (device-bound: events around K steps)
  spynet_ms / sr_ms      forward + backward of the two halves alone: SpyNet on both neighbours (gradient of sum of the warped frames and
                         flows into the parameters), MSRResNet on a 9-channel clip
  conv7                  per SpyNet layer shape (6 / 8 -> 32 -> 64 -> 32 -> 16 -> 2) on batch x size^2: forward, data gradient and weight
                         gradient of the 7x7 convolution alone, ms and TFLOP/s (2 * 49 * C * Co FLOP per pixel each) -- the exact-f32
                         kernels, whatever the GEMM mode: the baseline a bf16-split 7x7 has to beat
  resample               the flow warp (forward; backward with the flow gradient only, as in TOF), the 2 x 2 average pool and the x2
                         align_corners upsample at full resolution, and `resample_ms_step`: all their calls of one step (both
                         neighbours, every pyramid level, forward + backward) timed one by one and summed
Every figure outside ms_step is the median of `--reps` timed calls after warm-up, device events.

usage: python tools/tof_step.py [--steps K] [--warmup W] [--batch B] [--size S] [--reps R]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from step_timing import clip_batch, lap_ms, median, split_opt, train_ms_step  # noqa: E402

SPYNET_LAYERS = [(6, 32), (8, 32), (32, 64), (64, 32), (32, 16), (16, 2)]



def conv7_times(B, S, reps):
    from realvsr_amd import functional as RF
    d = torch.device('cuda', 0)
    g = torch.Generator(device='cuda').manual_seed(2)
    out = {}
    for C, Co in SPYNET_LAYERS:
        x = torch.randn(B, C, S, S, device=d, generator=g)
        gout = torch.randn(B, Co, S, S, device=d, generator=g)
        w = torch.randn(Co, C, 7, 7, device=d, generator=g) / (7.0 * C ** 0.5)
        b = torch.zeros(Co, device=d)
        y, gx, gw, gb = torch.empty_like(gout), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
        tflop = 2.0 * 49 * C * Co * B * S * S / 1e12
        row = {}
        for name, fn in (('fwd', lambda: RF._conv(x, w, y, bias=b, what='conv7 fwd')),
                         ('dgrad', lambda: RF._conv(gout, w, gx, transposed=True, what='conv7 dgrad')),
                         ('wgrad', lambda: RF._conv_wgrad(x, gout, gw, gb, what='conv7 wgrad'))):
            ms = median(lap_ms(fn, reps, 2))
            row[name + '_ms'], row[name + '_tflops'] = round(ms, 3), round(tflop / ms * 1e3, 1)
        out['%dto%d' % (C, Co)] = row
        del x, gout, y, gx
    return out


def resample_times(B, S, K, reps):
    from realvsr_amd import functional as RF
    d = torch.device('cuda', 0)
    g = torch.Generator(device='cuda').manual_seed(3)

    def ops(s):
        """{name: (forward ms, backward ms)} of the three operators on a level of s x s (pool and warp) / s/2 x s/2 (upsample)."""
        img = torch.rand(B, 3, s, s, device=d, generator=g)
        flow = (2.0 * torch.randn(B, s, s, 2, device=d, generator=g)).requires_grad_(True)
        small = torch.randn(B, 2, s // 2, s // 2, device=d, generator=g).requires_grad_(True)
        imgr = img.clone().requires_grad_(True)
        res = {}
        for name, make in (('warp', lambda: RF.flow_warp(img, flow)), ('pool', lambda: RF.avg_pool2(imgr)),
                           ('upsample', lambda: RF.upsample2_ac(small, 2.0))):
            y = make()
            gy = torch.randn_like(y)
            fwd = median(lap_ms(make, reps, 2))
            bwd = median(lap_ms(lambda: y.backward(gy, retain_graph=True), reps, 2))
            res[name] = (fwd, bwd)
        return res

    full = ops(S)
    out = {'%s_%s_ms' % (k, p): round(v[i], 4) for k, v in full.items() for i, p in enumerate(('fwd', 'bwd'))}
    total = full['warp'][0] + full['warp'][1]   # the final warp at full resolution
    for lvl in range(K):   # level inputs at S, S/2, ...: a warp, the pool that made the next level (forward only: images are data), an upsample
        o = full if lvl == 0 else ops(S >> lvl)
        total += sum(o['warp']) + 2 * o['pool'][0] + sum(o['upsample'])
    out['resample_ms_step'] = round(2 * total, 3)   # two neighbours
    return out


def halves(model, B, S, reps):
    net = model.netG
    g = torch.Generator(device='cuda').manual_seed(4)
    ref, nbr = (torch.rand(B, 3, S, S, device='cuda', generator=g) for _ in range(2))
    clip = torch.rand(B, 9, S, S, device='cuda', generator=g)

    def spynet():
        net.zero_grad(set_to_none=True)
        for _ in range(2):
            warped, flow = net.align_arch(ref, nbr)
            (warped.sum() + flow.sum()).backward()

    def sr():
        net.zero_grad(set_to_none=True)
        net.sr_arch(clip).sum().backward()

    return {'spynet_ms': round(median(lap_ms(spynet, reps, 1)), 2), 'sr_ms': round(median(lap_ms(sr, reps, 1)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=192)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from realvsr_amd import _lib
    from realvsr_amd.VideoSR_model import create_model
    torch.cuda.set_device(0)
    K = 3
    opt = split_opt({'which_model_G': 'TOF', 'nframes': 3, 'K': K, 'nc': 3, 'nf': 64, 'nb': 10})
    torch.manual_seed(0)
    model = create_model(opt)
    B, S = a.batch, a.size
    data = clip_batch(B, S, 1)
    ms_step = train_ms_step(model, data, a.warmup, a.steps)
    res = {'metric': 'tof_step', 'gemm_mode': _lib.get_gemm_mode(), 'batch': B, 'frames': 3, 'size': S, 'K': K,
           'ms_step': round(ms_step, 2),
           'loss_terms': {k: round(float(v), 5) for k, v in model.loss_terms.items()},
           'peak_mem_gb': round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    del data
    res.update(halves(model, B, S, max(a.reps // 2, 2)))
    del model
    torch.cuda.empty_cache()
    res['conv7'] = conv7_times(B, S, a.reps)
    res['resample'] = resample_times(B, S, K, a.reps)
    res['resample_share_of_step'] = round(res['resample']['resample_ms_step'] / res['ms_step'], 4)
    res.update(steps=a.steps, warmup=a.warmup, reps=a.reps)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
