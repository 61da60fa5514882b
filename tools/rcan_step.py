#!/usr/bin/env python
"""One JSON line for RCAN at the shape of train_RCAN_RealVSR_YCbCr_Split.yml: batch 32, 3 x 192^2 frames, scale 1, num_feat 64,
num_group 5, num_block 2, squeeze_factor 16, res_scale 1, LapPyr(ssim, cb) on Y + GWLoss on CbCr.

  ms_step              wall time per VideoSRModel.optimize_parameters(step, log=False) (device-bound: events around K steps)
  ca_fwd_ms / ca_bwd_ms  the fused channel-attention operator alone on a batch x 64 x size^2 tensor with its residual (out = x + u * gate),
                       median of `--reps` timed calls after warm-up; *_gbs: the GB/s they imply at 4 passes over the tensor each
  composed_*_ms        the same operator composed from torch ops under autograd, built here only: mean, F.conv2d 1x1, relu, F.conv2d
                       1x1, sigmoid, mul, add

usage: python tools/rcan_step.py [--steps K] [--warmup W] [--batch B] [--size S] [--reps R]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from step_timing import clip_batch, lap_ms, median, split_opt, train_ms_step  # noqa: E402


def ca_times(B, S, reps):
    """Forward and backward of the channel-attention tail of an RCAB, fused and composed, on B x 64 x S x S."""
    from realvsr_amd import functional as RF
    d = torch.device('cuda', 0)
    C, Cr = 64, 4
    g = torch.Generator(device='cuda').manual_seed(2)
    u = (torch.randn(B, C, S, S, device=d, generator=g) + torch.randn(1, C, 1, 1, device=d, generator=g)).requires_grad_(True)
    x = torch.randn(B, C, S, S, device=d, generator=g).requires_grad_(True)
    gout = torch.randn(B, C, S, S, device=d, generator=g)
    down, up = torch.nn.Conv2d(C, Cr, 1).to(d), torch.nn.Conv2d(Cr, C, 1).to(d)

    def fused():
        return RF.channel_attention(u, down, up, x=x, res_scale=1.0)

    def composed():
        a = torch.sigmoid(F.conv2d(torch.relu(F.conv2d(u.mean((2, 3), keepdim=True), down.weight, down.bias)), up.weight, up.bias))
        return u * a + x

    out = {}
    passes = 4 * B * C * S * S * 4 / 1e9   # GB moved at 4 passes over one f32 tensor
    for name, fn in (('ca', fused), ('composed', composed)):
        with torch.no_grad():
            fwd = median(lap_ms(fn, reps, 3))
        y = fn()

        def bwd():
            for t in (u, x, down.weight, down.bias, up.weight, up.bias):
                t.grad = None
            y.backward(gout, retain_graph=True)
        out[name + '_fwd_ms'], out[name + '_bwd_ms'] = round(fwd, 4), round(median(lap_ms(bwd, reps, 3)), 4)
        del y
    out['ca_fwd_gbs'], out['ca_bwd_gbs'] = round(passes / out['ca_fwd_ms'] * 1e3, 1), round(passes / out['ca_bwd_ms'] * 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=192)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    from realvsr_amd.VideoSR_model import create_model
    torch.cuda.set_device(0)
    opt = split_opt({'which_model_G': 'RCAN', 'num_in_ch': 3, 'num_out_ch': 3, 'num_frames': 3, 'num_feat': 64, 'num_group': 5,
                     'num_block': 2, 'squeeze_factor': 16, 'res_scale': 1})
    torch.manual_seed(0)
    model = create_model(opt)
    B, S = a.batch, a.size
    data = clip_batch(B, S, 1)
    ms_step = train_ms_step(model, data, a.warmup, a.steps)
    res = {'metric': 'rcan_step', 'batch': B, 'frames': 3, 'size': S, 'ms_step': round(ms_step, 2),
           'loss_terms': {k: round(float(v), 5) for k, v in model.loss_terms.items()}}
    del model, data
    torch.cuda.empty_cache()
    res.update(ca_times(B, S, a.reps))
    res.update(steps=a.steps, warmup=a.warmup, reps=a.reps)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
