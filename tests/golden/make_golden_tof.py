#!/usr/bin/env python
"""Generate tests/golden/tof.npz and tof_s4.npz from the reference's OWN TOF (build container only).

Run from the repo root:   python tests/golden/make_golden_tof.py
Same recipe as make_golden_fstrn.py (import_reference / save / weights.fill_state_dict): models.archs.TOF_arch is imported from the
read-only reference tree and run on CPU; only the .npz files written here are committed: tof.npz holds k3 and k2, tof_s4.npz holds k1s4
(one file with all three is 1.2 MiB, above the limit for a committed file; what is stored per case is the same).  After the seeded fill every BatchNorm2d gets
reset_running_stats() (the fill draws negative variances).  x = rand (seed 7), gout = randn (seed 8).
  k3   : nframes 3, K 3, nf 32, nb 2, upscale 1, x (2, 3, 3, 16, 24)   coarsest level 2 x 3: a 7x7 conv on a frame smaller than its kernel
  k2   : nframes 3, K 2, nf 16, nb 1, upscale 1, x (1, 3, 3, 20, 36)   a 5 x 9 level: odd sizes, W % 4 != 0
  k1s4 : nframes 5, K 1, nf 16, nb 1, upscale 4, x (1, 5, 3, 10, 14)   four neighbours, the x4 tail
Each case runs a training-mode forward + backward, then an eval forward on the running statistics that step left.  Stored per case: x,
gout; train.out, train.gx, eval.out; train.flow.<j>, the final flow of neighbour j; the running mean / var and num_batches_tracked of
align_arch.block0.block.1 and align_arch.blocks.0.block.10 after the step; names and shapes of every state_dict entry; the gradients of
every bias and every BatchNorm weight, and the first 4 output channels of every conv weight gradient; for every conv bias in front of a
BatchNorm the per-channel sum |g| of its output gradient (gradmag.*); the ReLU input closest to zero and its layer (min_preact*).
main() asserts what makes the fixture worth having, so a change of the seeded values fails here instead of writing a weak fixture (the
flow gradient is discontinuous where a sampling coordinate crosses an integer, so no coordinate of any warp may come near one): see
CHECKS and MIN_PREACT.  About one weight seed in ten clears the first of them at these sizes; k2 uses seed 90, k3 seed 378, k1s4 -- whose flows at K 1 are
small, so that training and eval outputs rarely differ by 0.01 -- seed 3208, the one of 1 .. 7000 that clears all five.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save  # noqa: E402
from weights import fill_state_dict  # noqa: E402

CASES = {'k3': (dict(nframes=3, K=3, in_nc=3, out_nc=3, nf=32, nb=2, upscale=1), (2, 3, 3, 16, 24), 378),
         'k2': (dict(nframes=3, K=2, in_nc=3, out_nc=3, nf=16, nb=1, upscale=1), (1, 3, 3, 20, 36), 90),
         'k1s4': (dict(nframes=5, K=1, in_nc=3, out_nc=3, nf=16, nb=1, upscale=4), (1, 5, 3, 10, 14), 3208)}
FILES = {'tof': ('k3', 'k2'), 'tof_s4': ('k1s4',)}
BN_STORED = ('align_arch.block0.block.1', 'align_arch.blocks.0.block.10')
# min distance of a sampling coordinate to an integer; mean and max |flow| at full resolution (px); share of full-resolution sampling
# positions outside the frame; max |training output - eval output|
CHECKS = dict(min_dist=1e-4, mean_flow=0.3, max_flow=1.0, outside=(0.05, 0.30), train_eval=0.01)
# ... and the distance of every ReLU input (BatchNorm output) of the training forward from zero, where the ReLU's derivative jumps.  The HIP
# forward sits within ~1e-6 of the reference's, and a sign that flips changes every gradient upstream of it by percents: weight seed 90
# put one k3 activation (align_arch.blocks.0.block.7) 1.0e-7 from zero, it flipped on the device, and 32 gradients were off by 3e-3 .. 2e-1.
# With ~6e5 activations per case the closest one is typically at 1e-6; about one seed in a hundred clears 3e-6, none of 1200 clears 1e-5.
# k3 is bounded (seed 378: 3.05e-6).  k2 (seed 90: 2.1e-7) and k1s4 (the only seed of 7000 that clears the five checks above: 8.7e-7) are
# recorded, not bounded: no seed of the 360 scanned clears 3e-6 and the other checks for k2; what holds them is that the device kernels
# are deterministic and tests/test_gpu_tof.py passes on them as generated.  The closest activation and its layer are stored
# (min_preact, min_preact_layer); tests/test_gpu_tof.py describes what a flipped sign looks like and names them when a gradient misses.
MIN_PREACT = {'k3': 3e-6, 'k2': None, 'k1s4': None}


def _coords(flow, h, w):
    """The sampling coordinates of arch_util.flow_warp in its own float arithmetic, then grid_sample's align_corners=True un-normalisation."""
    gy, gx = torch.meshgrid(torch.arange(0, h), torch.arange(0, w), indexing='ij')
    vx, vy = gx.float() + flow[..., 0], gy.float() + flow[..., 1]
    cx = ((2.0 * vx / max(w - 1, 1) - 1.0) + 1) / 2 * (w - 1)
    cy = ((2.0 * vy / max(h - 1, 1) - 1.0) + 1) / 2 * (h - 1)
    return cx, cy


def run_case(TOF_arch, tag, seed=None):
    """-> (arrays of the case, statistics that CHECKS bounds)."""
    kw, xshape, case_seed = CASES[tag]
    seed = case_seed if seed is None else seed
    net = TOF_arch.TOF(**kw)
    fill_state_dict(net, seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.reset_running_stats()
    H, W = xshape[-2:]
    warps, flows = [], []
    ref_warp = TOF_arch.arch_util.flow_warp

    def recording_warp(x, flow, *a, **k):
        warps.append((flow.detach().clone(), x.shape[-2], x.shape[-1]))
        return ref_warp(x, flow, *a, **k)

    handle = net.align_arch.register_forward_hook(lambda mod, i, o: flows.append(o[1].detach().clone()))
    preact, gradmag = [], {}
    for name, m in net.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):      # its output is the ReLU's input
            m.register_forward_hook(lambda mod, i, o, n=name: preact.append((o.detach().abs().min().item(), n)))
        elif isinstance(m, torch.nn.Conv2d) and name.startswith('align_arch') and not name.endswith('block.12'):
            # a bias in front of a training-mode BatchNorm: its gradient, the sum of the conv's output gradient, is zero in exact
            # arithmetic; what float32 leaves of a channel's sum lives on the scale of that channel's sum |g| (all SpyNet passes), stored
            # next to it, one value per output channel
            m.register_full_backward_hook(lambda mod, gi, go, n=name: gradmag.__setitem__(n, gradmag.get(n, 0.0) + go[0].double().abs().sum((0, 2, 3))))
    TOF_arch.arch_util.flow_warp = recording_warp
    try:
        x = torch.rand(*xshape, generator=torch.Generator().manual_seed(7))
        net.train()
        xi = x.clone().requires_grad_(True)
        out = net(xi)
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(8))
        out.backward(gout)
        train_warps, train_flows, train_preact = list(warps), list(flows), min(preact)
        stats_after = {k: v.detach().clone() for k, v in net.state_dict().items()}
        net.eval()
        with torch.no_grad():
            out_eval = net(x)
    finally:
        TOF_arch.arch_util.flow_warp = ref_warp
        handle.remove()
    assert len(train_flows) == kw['nframes'] - 1 and len(warps) == 2 * (kw['nframes'] - 1) * (kw['K'] + 1)

    dist, outside = [], []
    for flow, h, w in train_warps:   # (the forward whose gradients are stored; the eval output is continuous in the coordinates)
        cx, cy = _coords(flow, h, w)
        for c, n in ((cx, w), (cy, h)):
            if n > 1:
                dist.append((c - c.round()).abs().min().item())
        if (h, w) == (H, W):
            outside.append(((cx < 0) | (cx > w - 1) | (cy < 0) | (cy > h - 1)).float().mean().item())
    fl = torch.stack(train_flows)
    stats = dict(min_dist=min(dist), mean_flow=fl.abs().mean().item(), max_flow=fl.abs().max().item(), outside=(min(outside), max(outside)),
                 train_eval=(out.detach() - out_eval).abs().max().item(), min_preact=train_preact[0])

    a = {tag + '.x': x.numpy(), tag + '.gout': gout.numpy(), tag + '.train.out': out.detach().numpy(), tag + '.train.gx': xi.grad.numpy().copy(),
         tag + '.eval.out': out_eval.numpy()}
    for j, f in enumerate(train_flows):
        a['%s.train.flow.%d' % (tag, j)] = f.numpy()
    for name in BN_STORED:
        for s in ('running_mean', 'running_var', 'num_batches_tracked'):
            a['%s.bn.%s.%s' % (tag, name, s)] = stats_after['%s.%s' % (name, s)].numpy().copy()
    sd = net.state_dict()
    a[tag + '.keys'] = np.array(list(sd.keys()))
    a[tag + '.shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    for k, p in net.named_parameters():
        if p.dim() == 4:
            a[tag + '.grad.' + k] = p.grad.numpy()[:4].copy()
        else:   # biases and BatchNorm weights
            a[tag + '.grad.' + k] = p.grad.numpy().copy()
    for n, v in gradmag.items():
        a['%s.gradmag.%s.bias' % (tag, n)] = v.numpy()
    # the ReLU input closest to zero and the BatchNorm it leaves: where a flipped sign would show (tests/test_gpu_tof.py names the signature)
    a[tag + '.min_preact'], a[tag + '.min_preact_layer'] = np.array([train_preact[0]]), np.array(train_preact[1])
    return a, stats


def holds(stats, tag=None):
    lo, hi = CHECKS['outside']
    if tag is not None and MIN_PREACT[tag] is not None and stats['min_preact'] < MIN_PREACT[tag]:
        return False
    return (stats['min_dist'] >= CHECKS['min_dist'] and stats['mean_flow'] >= CHECKS['mean_flow'] and stats['max_flow'] >= CHECKS['max_flow']
            and lo <= stats['outside'][0] and stats['outside'][1] <= hi and stats['train_eval'] > CHECKS['train_eval'])


def main():
    torch.set_num_threads(8)
    import_reference()
    import models.archs.TOF_arch as TOF_arch
    arrs = {}
    for tag in CASES:
        a, stats = run_case(TOF_arch, tag)
        print(tag, 'seed %d |' % CASES[tag][2], 'min dist %.2e | mean |flow| %.2f max %.2f | outside %.3f .. %.3f | train - eval %.3f | '
              'min |ReLU input| %.2e' % (stats['min_dist'], stats['mean_flow'], stats['max_flow'], stats['outside'][0], stats['outside'][1],
                                         stats['train_eval'], stats['min_preact']))
        assert holds(stats, tag), (tag, stats)
        arrs.update(a)
    for name, tags in FILES.items():
        save(name, **{k: v for k, v in arrs.items() if k.split('.')[0] in tags})
        assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), name + '.npz')) < (1 << 20)


if __name__ == '__main__':
    main()
