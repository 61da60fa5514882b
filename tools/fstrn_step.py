#!/usr/bin/env python
"""One JSON line for FSTRN at the shape of train_FSTRN_RealVSR_YCbCr_Split.yml: batch 32, 3 x 192^2 frames, scale 1, k 3, nf 64,
LapPyr(ssim, cb) on Y + GWLoss on CbCr through VideoSRModel.

  ms_step                wall time per VideoSRModel.optimize_parameters(step, log=False) (device-bound: events around K steps)
  tconv3_fwd_ms          the fused temporal convolution of an FRB alone on frames * batch x 64 x size^2: bias, the block's residual and the
                         next block's PReLU as second output (4 passes over the tensor: s, residual, out, pout -- and none for the taps)
  tconv3_dgrad_ms        the same kernel as the data gradient (transposed weight, no residual: 2 passes)
  tconv3_wgrad_ms        the weight gradient: the 1x1 weight-gradient kernel once per tap (the same with the switch off; 2 passes at best)
  composed_*_ms          the same three with functional._FUSE_TCONV3 off: three accumulated 1x1 convolutions over frame ranges on the
                         kernels the project had, and a PReLU pass for the second output
  *_gbs                  GB/s the fused times imply at the passes named above
Fused and composed alternate in one process; every figure is the median of `--reps` timed calls after warm-up, device events.

usage: python tools/fstrn_step.py [--steps K] [--warmup W] [--batch B] [--size S] [--reps R]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from step_timing import clip_batch, lap_ms, median, split_opt, train_ms_step  # noqa: E402


def tconv3_times(T, B, S, reps, rounds=2):
    """Forward, data gradient and weight gradient of the temporal convolution, fused and composed alternating, on T * B x 64 x S x S."""
    from realvsr_amd import functional as RF
    d = torch.device('cuda', 0)
    C = 64
    g = torch.Generator(device='cuda').manual_seed(2)
    s = torch.randn(T, B, C, S, S, device=d, generator=g)
    res = torch.randn(T, B, C, S, S, device=d, generator=g)
    gout = torch.randn(T, B, C, S, S, device=d, generator=g)
    conv = torch.nn.Conv3d(C, C, (3, 1, 1), padding=(1, 0, 0)).to(d)
    act = torch.nn.PReLU().to(d)
    w, b, sl = conv.weight.detach(), conv.bias.detach(), act.weight.detach()
    calls = {'fwd': lambda: RF._tconv3_run(s, w, b, res, sl), 'dgrad': lambda: RF._tconv3_run(gout, w, transposed=True),
             'wgrad': lambda: RF._tconv3_wgrad(s, gout, w, b)}
    samples = {}
    was = RF._FUSE_TCONV3
    try:
        with torch.no_grad():
            for _ in range(rounds):   # fused, composed, fused, composed: drift of the clocks shows up as a difference between the rounds
                for fuse in (True, False):
                    RF._FUSE_TCONV3 = fuse
                    for name, fn in calls.items():
                        samples.setdefault((('tconv3' if fuse else 'composed'), name), []).extend(lap_ms(fn, reps, 3))
    finally:
        RF._FUSE_TCONV3 = was
    out = {}
    for (kind, name), v in samples.items():
        out['%s_%s_ms' % (kind, name)] = round(median(v), 4)
        out['%s_%s_ms_min_max' % (kind, name)] = [round(min(v), 4), round(max(v), 4)]
    tensor_gb = T * B * C * S * S * 4 / 1e9
    for name, passes in (('fwd', 4), ('dgrad', 2), ('wgrad', 2)):
        out['tconv3_%s_gbs' % name] = round(passes * tensor_gb / out['tconv3_%s_ms' % name] * 1e3, 1)
    out['tconv3_passes'] = {'fwd': 4, 'dgrad': 2, 'wgrad': 2}
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
    opt = split_opt({'which_model_G': 'FSTRN', 'k': 3, 'nf': 64, 'nframes': 3})
    torch.manual_seed(0)
    model = create_model(opt)
    B, S = a.batch, a.size
    data = clip_batch(B, S, 1)
    ms_step = train_ms_step(model, data, a.warmup, a.steps)
    res = {'metric': 'fstrn_step', 'batch': B, 'frames': 3, 'size': S, 'ms_step': round(ms_step, 2),
           'loss_terms': {k: round(float(v), 5) for k, v in model.loss_terms.items()},
           'peak_mem_gb': round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    del model, data
    torch.cuda.empty_cache()
    res.update(tconv3_times(3, B, S, a.reps))
    res.update(steps=a.steps, warmup=a.warmup, reps=a.reps)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
