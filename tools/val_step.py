#!/usr/bin/env python
"""One JSON line for what the training driver (realvsr_amd.train) adds around the step, on synthetic validation clips.

  val_clipwise_ms_per_frame    train.validate: a clip uploaded once as uint8, per-frame features once (SlidingWindowRunner), PSNR on the
                               device, every fifth frame written as PNG
  val_clipwise_no_png_ms_per_frame   the same pass with save_images=False: what the PNG encoder on the host costs is the difference
                               (synthetic noise frames are the worst case for it: they do not compress)
  val_framewise_ms_per_frame   the same frames one sample at a time: feed_data(collated sample) / test() / get_current_metrics() -- the
                               loop of the reference's train.py with the two-line change of INTEGRATION.md; no PNG is written here
  sched_us_per_step            update_learning_rate alone (host arithmetic; the shipped cosine schedule)
Host wall time around each pass with a device synchronisation at both ends; the first pass of each kind warms up and is not counted.
The two validation passes must return the same PSNR values (==); the line says so in `equal`.

usage: python tools/val_step.py [--folders F] [--frames T] [--height H] [--width W] [--small] [--passes P]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _write_clips(root, folders, T, H, W):
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(2)
    for which in ('GT', 'LQ'):
        for f in range(folders):
            d = os.path.join(root, which, '%03d' % f)
            os.makedirs(d)
            base = rng.randint(0, 256, size=(H, W, 3))
            for i in range(T):
                frame = np.clip(base + rng.randint(-30, 31, size=base.shape), 0, 255).astype(np.uint8)
                Image.fromarray(frame, 'RGB').save(os.path.join(d, '%05d.png' % i))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--folders', type=int, default=2)
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--small', action='store_true', help='one residual block each (default: the shipped EDVR_NoUp woTSA, nf 64, 5 + 10 blocks)')
    ap.add_argument('--passes', type=int, default=2)
    a = ap.parse_args()

    import torch
    from torch.utils.data import default_collate
    from realvsr_amd import data, train
    from realvsr_amd.VideoSR_model import create_model
    torch.cuda.set_device(0)
    net = dict(which_model_G='EDVR_NoUp', nf=64, nc=3, nframes=3, groups=8, front_RBs=5, back_RBs=10, predeblur=False, HR_in=False,
               w_TSA=False, center=None)
    if a.small:
        net.update(front_RBs=1, back_RBs=1)
    with tempfile.TemporaryDirectory() as root:
        _write_clips(root, a.folders, a.frames, a.height, a.width)
        opt = {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
               'network_G': net, 'path': {'pretrain_model_G': None, 'strict_load': True, 'val_images': os.path.join(root, 'val_images')},
               'train': {'pixel_criterion_y': 'cb', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'cb', 'pixel_weight_c': 1.0,
                         'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-4, 'beta1': 0.9, 'beta2': 0.99,
                         'lr_scheme': 'CosineAnnealingLR_Restart', 'T_period': [150000] * 4, 'restarts': [150000, 300000, 450000],
                         'restart_weights': [1, 1, 1], 'eta_min': 1e-7}}
        model = create_model(opt)
        val_set = data.VideoTestDataset({'name': 'RealVSR_Test', 'mode': 'VideoTest', 'dataroot_GT': os.path.join(root, 'GT'),
                                         'dataroot_LQ': os.path.join(root, 'LQ'), 'cache_data': True, 'N_frames': 3, 'padding': 'new_info',
                                         'color': 'ycbcr', 'phase': 'val', 'scale': 1, 'data_type': 'img'})
        n = len(val_set)

        def clipwise(save_images=True):
            return [v for vs in train.validate(model, val_set, 1, save_images=save_images)['psnr'].values() for v in vs]

        def clipwise_no_png():
            return clipwise(False)

        def framewise():
            out = []
            for i in range(n):
                model.feed_data(default_collate([val_set[i]]))
                model.test()
                out.append(model.get_current_metrics()['psnr'][0])
            return out

        res = {'metric': 'val_step', 'folders': a.folders, 'frames': a.frames, 'height': a.height, 'width': a.width,
               'network': 'EDVR_NoUp nf%d %d+%d' % (net['nf'], net['front_RBs'], net['back_RBs'])}
        values = {}
        for name, fn in (('val_clipwise', clipwise), ('val_clipwise_no_png', clipwise_no_png), ('val_framewise', framewise)):
            values[name] = fn()      # warm-up
            samples = []
            for _ in range(a.passes):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                samples.append((time.perf_counter() - t) * 1e3 / n)
            res[name + '_ms_per_frame'] = round(min(samples), 3)
            res[name + '_ms_per_frame_all'] = [round(v, 3) for v in samples]
        res['equal'] = values['val_clipwise'] == values['val_framewise'] == values['val_clipwise_no_png']
        res['psnr_mean'] = round(sum(values['val_clipwise']) / n, 4)

        steps = 20000
        model.update_learning_rate(1)
        t = time.perf_counter()
        for k in range(2, steps + 2):
            model.update_learning_rate(k, warmup_iter=-1)
        res['sched_us_per_step'] = round((time.perf_counter() - t) * 1e6 / steps, 3)
    print(json.dumps(res))
    return 0 if res['equal'] else 1


if __name__ == '__main__':
    sys.exit(main())
