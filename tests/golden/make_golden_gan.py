#!/usr/bin/env python
"""Generate tests/golden/gan_step.npz from the reference's OWN VideoSRGANModel (build container only).

Run from the repo root:   python tests/golden/make_golden_gan.py
Same recipe as make_golden.py (import_reference / save / weights.fill_state_dict): the reference's
codes/models/VideoSRGAN_AllPair_model_YCbCr_Split.py is built through models.create_model(opt) on CPU (gpu_ids None) and
stepped 3 times on one seeded batch.
  G: EDVR_NoUp nf 64 (its HRconv is wired for 64), N 3, groups 8, front/back RBs 1, no TSA;
  D: MultiscaleDiscriminator_v4, in_nc 1, nf 16, num_D 2;  batch 2 of 48x64 frames, scale 1 (the low pyramid band holds the
  11x11 SSIM window);  Adam lr 1e-3 (G and D), betas (0.9, 0.99);  gan_weight 0.1.
Weights: G and D filled from seeds, then D's BatchNorm buffers reset to their defaults; the tests re-create both.
Tags:
  ragan_cb   : cri_pix_s replaced by the reference's CharbonnierLoss -- every op in-tree => PINNED
  ragan_ssim : the option file's criteria (SSIM on the low band: the restated SSIM of oracle/ssim_oracle.py => UNPINNED term)
  gan_cb     : vanilla GAN, Charbonnier low band
  ratio      : ragan_cb with D_update_ratio 2, D_init_iters 1 (steps 1 and 3 skip the G update)
Stored per tag: 3 steps of log_dict values, G / D gradient norms of step 1 (where computed), G / D state after step 3 (subsets,
to bound the file size: G_KEEP, and D_KEEP -- every BatchNorm2d with its running statistics and num_batches_tracked).  Plus D's state_dict key / shape list.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save  # noqa: E402
from weights import fill_state_dict  # noqa: E402

LOG_KEYS = ['l_g_pix_s', 'l_g_pix_d', 'l_g_pix_c', 'l_g_gan', 'l_g_total', 'l_d_real', 'l_d_fake']
G_KEEP = ('conv_first.', 'pcd_align.cas_dcnpack.conv_offset_mask.bias', 'recon_trunk.0.conv1.bias', 'HRconv.bias', 'conv_last.')
D_KEEP = (0, 2, 3, 6, 9, 12, 15, 18, 20)   # Sequential indices: first conv, one stride-2 conv, every BatchNorm2d, last conv
G_SEED, D_SEED = 505, 606


class Opt(dict):
    """The reference reads optional keys with [] (train_opt['D_update_ratio'], path['pretrain_model_D']): None when absent."""

    def __missing__(self, key):
        return None


def gan_opt(tag):
    train = Opt(lr_G=1e-3, weight_decay_G=0, beta1_G=0.9, beta2_G=0.99, lr_D=1e-3, weight_decay_D=0, beta1_D=0.9, beta2_D=0.99,
                lr_scheme='MultiStepLR', lr_steps=[1000], restarts=None, restart_weights=None, lr_gamma=0.5, clear_state=None,
                pixel_criterion_s='ssim', pixel_weight_s=1.0, pixel_criterion_d='cb', pixel_weight_d=1.0,
                pixel_criterion_c='gw', pixel_weight_c=1.0, feature_criterion='cb', feature_weight=0.0,
                gan_type='gan' if tag == 'gan_cb' else 'ragan', gan_weight=0.1)
    if tag == 'ratio':
        train.update(D_update_ratio=2, D_init_iters=1)
    return Opt(model='VideoSRGAN_AllPair_YCbCr_Split', dist=False, gpu_ids=None, is_train=True, scale=1, augment=None,
               network_G=Opt(which_model_G='EDVR_NoUp', nf=64, nc=3, nframes=3, groups=8, front_RBs=1, back_RBs=1, predeblur=False,
                             HR_in=False, w_TSA=False, center=None),
               network_D=Opt(which_model_D='MultiscaleDiscriminator_v4', in_nc=1, nf=16, num_D=2, gan_type='patch'),
               path=Opt(pretrain_model_G=None, pretrain_model_D=None, strict_load=True), train=train)


def gan_data():
    gen = torch.Generator().manual_seed(71)
    return {'LQs': torch.rand(2, 3, 3, 48, 64, generator=gen), 'GT': torch.rand(2, 3, 3, 48, 64, generator=gen)}


def fill_weights(netG, netD):
    fill_state_dict(netG, G_SEED, offset_std=0.02)
    fill_state_dict(netD, D_SEED)
    for m in netD.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.reset_running_stats()


def main():
    torch.set_num_threads(8)
    _, loss_mod, _, _ = import_reference()
    import models
    data = gan_data()
    arrs = {'LQs': data['LQs'].numpy(), 'GT': data['GT'].numpy()}
    for tag in ('ragan_cb', 'ragan_ssim', 'gan_cb', 'ratio'):
        torch.manual_seed(5)
        model = models.create_model(gan_opt(tag))
        netG = model.netG.module if hasattr(model.netG, 'module') else model.netG
        netD = model.netD.module if hasattr(model.netD, 'module') else model.netD
        fill_weights(netG, netD)
        if 'D.keys' not in arrs:
            sd = netD.state_dict()
            arrs['D.keys'] = np.array(list(sd.keys()))
            arrs['D.shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
        if tag != 'ragan_ssim':
            model.cri_pix_s = loss_mod.CharbonnierLoss()
        logs = []
        for step in range(1, 4):
            model.feed_data(data)
            model.optimize_parameters(step)
            log = model.get_current_log()   # (G terms of a skipped step: the log keeps the previous values -> NaN here)
            g_step = step % model.D_update_ratio == 0 and step > model.D_init_iters
            logs.append([log[k] if (k.startswith('l_d') or g_step) else np.nan for k in LOG_KEYS])
            if step == 1:
                gG = [p.grad for p in netG.parameters() if p.grad is not None]
                arrs[tag + '.gnormG1'] = np.float64(torch.sqrt(sum((g.double() ** 2).sum() for g in gG)).item()) if gG else np.float64(np.nan)
                arrs[tag + '.gnormD1'] = np.float64(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in netD.parameters())).item())
        arrs[tag + '.logs'] = np.array(logs, dtype=np.float64)
        for k, v in netG.state_dict().items():
            if k.startswith(G_KEEP):
                arrs[tag + '.G.' + k] = v.detach().numpy().copy()
        for k, v in netD.state_dict().items():
            if int(k.split('.')[1]) in D_KEEP:
                arrs[tag + '.D.' + k] = v.detach().numpy().copy()
    save('gan_step', **arrs)


if __name__ == '__main__':
    main()
