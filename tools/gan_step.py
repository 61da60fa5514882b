#!/usr/bin/env python
"""One JSON line for the GAN stage at the shape of train_EDVR-GAN_woTSA_RealVSR_YCbCr_Split.yml: batch 32, 3 x 192^2 frames, scale 1,
G = EDVR_NoUp nf 64 (front 5 / back 10, no TSA), D = MultiscaleDiscriminator_v4 nf 64, num_D 2, RaGAN, SSIM + Charbonnier + GWLoss.

  ms_step          wall time per VideoSRGANModel.optimize_parameters(step, log=False) (device-bound: events around K steps)
  g_ms / d_ms      device time of the G half (G forward, pyramids, pixel terms, 2 D forwards, backward, Adam) and of the D half
                   (3 D forwards, 2 backwards, Adam), from events recorded where the model switches D's requires_grad
  conv5_*_tflops   achieved rate of the 5x5 forward / weight-gradient kernels on two D layers at this shape

usage: python tools/gan_step.py [--steps K] [--warmup W] [--batch B] [--size S]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=192)
    a = ap.parse_args()
    from realvsr_amd.VideoSR_model import create_model
    torch.cuda.set_device(0)
    train = {'lr_G': 5e-5, 'weight_decay_G': 0, 'beta1_G': 0.9, 'beta2_G': 0.99, 'lr_D': 5e-5, 'weight_decay_D': 0, 'beta1_D': 0.9,
             'beta2_D': 0.99, 'pixel_criterion_s': 'ssim', 'pixel_weight_s': 1.0, 'pixel_criterion_d': 'cb', 'pixel_weight_d': 1.0,
             'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0, 'feature_criterion': 'cb', 'feature_weight': 0.0, 'gan_type': 'ragan',
             'gan_weight': 1e-4}
    opt = {'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
           'network_G': {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 5, 'back_RBs': 10,
                         'predeblur': False, 'HR_in': False, 'w_TSA': False},
           'network_D': {'which_model_D': 'MultiscaleDiscriminator_v4', 'in_nc': 1, 'nf': 64, 'num_D': 2, 'gan_type': 'patch'},
           'path': {}, 'train': train}
    torch.manual_seed(0)
    model = create_model(opt)
    g = torch.Generator(device='cuda').manual_seed(1)
    B, S = a.batch, a.size
    data = {'LQs': torch.rand(B, 3, 3, S, S, device='cuda', generator=g), 'GT': torch.rand(B, 3, 3, S, S, device='cuda', generator=g)}

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
    res = {'metric': 'gan_step', 'batch': B, 'frames': 3, 'size': S, 'ms_step': round(ms, 2), 'g_ms': round(g_ms / a.steps, 2),
           'd_ms': round(d_ms / a.steps, 2), 'd_share': round(d_ms / (g_ms + d_ms), 3),
           'loss_terms': {k: round(float(v), 5) for k, v in model.loss_terms.items()},
           'conv5': conv5_rates(B), 'steps': a.steps, 'warmup': a.warmup}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
