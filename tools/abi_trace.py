#!/usr/bin/env python
"""Record of the C-ABI calls a fixed set of small workloads makes, as call counts per entry and SHA-256 digests: two commits whose host
glue differs but whose digests agree drive the library identically.  Uses only realvsr_amd._lib and public entry points, so the same
file runs on any commit.

Every rvsr_* call is recorded in order: the entry's name, each non-pointer argument verbatim (floats by repr), each device pointer as
None or the index of the first pointer argument of the same call with the same address (aliasing such as "the residual is the output
buffer" is part of the record, allocator addresses are not), a host pointer as None / 'host'.  `digest` covers everything; `launches`
leaves out the argument-only host queries (*_workspace_bytes, rvsr_get_gemm_mode, the *_plan exports and the three DCN rule exports), which launch nothing.

usage: python tools/abi_trace.py [--dump FILE]
"""
import ctypes
import hashlib
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from realvsr_amd import _lib  # noqa: E402

RECORD = []


class Proxy:
    def __init__(self, handle):
        self._handle = handle

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.startswith('rvsr_') or name == 'rvsr_last_error':
            return fn
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            rec, seen = [name], {}
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if t is ctypes.c_void_p:
                    addr = a.value if isinstance(a, ctypes.c_void_p) else a
                    rec.append(None if not addr else seen.setdefault(addr, i))
                elif t in (ctypes.c_float, ctypes.c_double):
                    rec.append(repr(float(a)))
                elif t in (ctypes.c_int, ctypes.c_size_t):
                    rec.append(int(a))
                else:
                    rec.append(None if a is None else 'host')
            RECORD.append(tuple(rec))
            return fn(*args)
        return call


def section(name, fn):
    RECORD.append(('SECTION', name))
    n = len(RECORD)
    try:
        fn()
    except Exception as e:   # (kept in the record: both commits must then fail alike)
        RECORD.append(('ERROR', type(e).__name__))
        print('  %-28s FAILED: %s: %s' % (name, type(e).__name__, e))
    torch.cuda.synchronize()
    print('  %-28s %5d calls' % (name, len(RECORD) - n))


def train_opt(**net_kw):
    net = dict(which_model_G='EDVR', nf=16, nc=3, nframes=3, groups=4, front_RBs=1, back_RBs=1, center=None, predeblur=False,
               HR_in=False, w_TSA=True)
    net.update(net_kw)
    return {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 4, 'augment': None,
            'network_G': net, 'path': {'pretrain_model_G': None, 'strict_load': True},
            'train': {'pixel_criterion_y': 'lappyr', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 0.5,
                      'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-3, 'beta1': 0.9, 'beta2': 0.99}}


def randomize(net, seed):
    """Seeded weights with non-zero DCN offsets (the default initialisation of conv_offset_mask is zero)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(net.named_parameters()):
            std = 0.01 if name.endswith('bias') else (0.02 if 'conv_offset_mask' in name else 0.5 / max(p[0].numel(), 1) ** 0.5)
            p.copy_((torch.randn(p.shape, generator=gen) * std).to(p.device))


def edvr_steps(enabled=True, lq=(24, 32), gt=(96, 128), **net_kw):
    from realvsr_amd import functional as RF
    from realvsr_amd.VideoSR_model import create_model
    gen = torch.Generator().manual_seed(3)
    data = {'LQs': torch.rand(2, 3, 3, *lq, generator=gen), 'GT': torch.rand(2, 3, 3, *gt, generator=gen)}
    RF.packed_weights.invalidate()
    RF.packed_weights.enabled = enabled
    try:
        torch.manual_seed(1)
        model = create_model(train_opt(**net_kw))
        randomize(model.netG, 808)
        for step in (1, 2, 3):
            model.feed_data(data)
            model.optimize_parameters(step)
            if step == 2:   # edits behind the optimizer's back, through torch (version bump)
                with torch.no_grad():
                    model.netG.conv_first.weight.mul_(1.01)
                    model.netG.pcd_align.L1_dcnpack.weight.mul_(0.99)
    finally:
        RF.packed_weights.enabled = True
        RF.packed_weights.invalidate()


def tdan():
    from realvsr_amd.archs.TDAN_arch import TDAN
    torch.manual_seed(2)
    net = TDAN(channel=3, nframes=3, scale=2, nf=64, nb_f=1, nb_b=1, groups=8)
    randomize(net, 5)
    net = net.cuda()
    x = torch.rand(1, 3, 3, 16, 24, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    out = net(x)
    (out[0] if isinstance(out, (tuple, list)) else out).sum().backward()


def gan_step():
    from realvsr_amd.VideoSR_model import create_model
    train = {'lr_G': 5e-5, 'weight_decay_G': 0, 'beta1_G': 0.9, 'beta2_G': 0.99, 'lr_D': 5e-5, 'weight_decay_D': 0, 'beta1_D': 0.9,
             'beta2_D': 0.99, 'pixel_criterion_s': 'ssim', 'pixel_weight_s': 1.0, 'pixel_criterion_d': 'cb', 'pixel_weight_d': 1.0,
             'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0, 'feature_criterion': 'cb', 'feature_weight': 0.0, 'gan_type': 'ragan',
             'gan_weight': 1e-4}
    opt = {'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
           'network_G': {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1, 'back_RBs': 1,
                         'predeblur': False, 'HR_in': False, 'w_TSA': False},
           'network_D': {'which_model_D': 'MultiscaleDiscriminator_v4', 'in_nc': 1, 'nf': 64, 'num_D': 2, 'gan_type': 'patch'},
           'path': {}, 'train': train}
    torch.manual_seed(0)
    model = create_model(opt)
    gen = torch.Generator().manual_seed(1)
    data = {'LQs': torch.rand(2, 3, 3, 64, 64, generator=gen).cuda(), 'GT': torch.rand(2, 3, 3, 64, 64, generator=gen).cuda()}
    model.feed_data(data)
    model.optimize_parameters(1, log=False)


def sliding_window():
    from realvsr_amd.archs.EDVR_arch import EDVR_NoUp
    from realvsr_amd.infer import SlidingWindowRunner
    torch.manual_seed(6)
    net = EDVR_NoUp(nf=64, nc=3, nframes=3, groups=8, front_RBs=1, back_RBs=1, w_TSA=True)
    randomize(net, 123)
    clip = torch.rand(5, 3, 24, 40, generator=torch.Generator().manual_seed(7)).cuda()
    SlidingWindowRunner(net.cuda().eval(), 3, padding='reflection', chunk=4)(clip)


def convs():
    from realvsr_amd import functional as RF
    gen = torch.Generator().manual_seed(9)
    torch.manual_seed(9)
    x = torch.randn(2, 16, 12, 20, generator=gen).cuda().requires_grad_(True)
    down = torch.nn.Conv2d(16, 32, 3, 2, 1).cuda()
    RF.conv2d(x, down, RF.ACT_LRELU, 0.1).sum().backward()
    up = torch.nn.Conv2d(16, 64, 3, 1, 1).cuda()
    RF.conv2d(x, up, RF.ACT_LRELU, 0.1, pixel_shuffle=True).sum().backward()
    # conv_cat_bcast whose reference is block 1 of x, with one sink for x: an owner conv, then the depositing concat conv
    N, B = 3, 2
    x = torch.randn(N * B, 16, 12, 20, generator=gen).cuda().requires_grad_(True)
    first, cat = torch.nn.Conv2d(16, 16, 3, 1, 1).cuda(), torch.nn.Conv2d(32, 16, 3, 1, 1).cuda()
    sink = RF.GradSink(x.shape)
    y0 = RF.conv2d(x, first, RF.ACT_LRELU, 0.1, sink=sink)
    y1 = RF.conv_cat_bcast(x, x[B:2 * B], cat, N, RF.ACT_LRELU, 0.1, x_sink=sink, ref_sink=sink, ref_block=1)
    (y0.sum() + y1.sum()).backward()


def main():
    torch.cuda.set_device(0)
    _lib._lib = Proxy(_lib.lib())
    section('edvr cache on', edvr_steps)
    section('edvr cache off', lambda: edvr_steps(enabled=False))
    section('edvr predeblur HR_in', lambda: edvr_steps(lq=(64, 64), gt=(64, 64), predeblur=True, HR_in=True))
    section('tdan', tdan)
    section('gan step', gan_step)
    section('sliding window', sliding_window)
    section('conv2d / conv_cat_bcast', convs)
    for mode in ('f16fp8', 'f32'):
        _lib.set_gemm_mode(mode)
        section('edvr ' + mode, edvr_steps)
    _lib.set_gemm_mode('bf16x3')
    counts = Counter(r[0] for r in RECORD if r[0] not in ('SECTION', 'ERROR'))
    for name in sorted(counts):
        print('%6d  %s' % (counts[name], name))
    query = lambda r: r[0].endswith(('_workspace_bytes', '_plan')) or r[0] in ('rvsr_get_gemm_mode', 'rvsr_dcn_fused_takes', 'rvsr_dcn_probe_samples',   # noqa: E731
                                                                              'rvsr_dcn_forward_halo')
    print('calls %d  digest %s' % (sum(counts.values()), hashlib.sha256(repr(RECORD).encode()).hexdigest()))
    print('launches %d  digest %s' % (sum(v for k, v in counts.items() if not query((k,))),
                                      hashlib.sha256(repr([r for r in RECORD if not query(r)]).encode()).hexdigest()))
    if '--dump' in sys.argv:
        with open(sys.argv[sys.argv.index('--dump') + 1], 'w') as f:
            f.writelines(repr(r) + '\n' for r in RECORD)


if __name__ == '__main__':
    main()
