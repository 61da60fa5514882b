#!/usr/bin/env python
"""Generate tests/golden/fstrn.npz from the reference's OWN FSTRN (build container only).

Run from the repo root:   python tests/golden/make_golden_fstrn.py
Same recipe as make_golden_rcan.py (import_reference / save / weights.fill_state_dict): models.archs.FSTRN_arch is imported from the
read-only reference tree and run on CPU; only the .npz written here is committed.
Two cases, both scale 1, weights.fill_state_dict(net, 61), x = rand (seed 7), gout = randn (seed 8):
  t3 : nf 64, nframes 3, x (2, 3, 3, 20, 36)
  t5 : nf 32, nframes 5, x (1, 5, 3, 13, 22)      (H * W % 4 != 0, conv3d_1 / upsample at three of five frames, 32-row tiles)
Each case runs in eval mode (Dropout is the identity) and in training mode (torch.manual_seed(5) before the forward).  The keep mask of
the training run is taken with a forward hook on net.dropout as (o != 0) | (i == 0) -- an element the PReLU left at exactly zero counts
as kept, either way it contributes nothing -- and stored with np.packbits in the reference's [B, C, T, H, W] order.
Stored per case: x, gout; eval.out / eval.gx and train.out / train.gx; train.keep (+ its shape); names and shapes of every state_dict
entry; from the TRAINING run the gradients of every bias, every PReLU slope, conv3d_fe, upsample and conv3d_2, and the first 16 output
channels of the weight gradients of frb_1, frb_5 and conv3d_1 (the file stays below 1 MiB).  A slope gradient is sum g * x * [x <= 0] over
the PReLU's input x and output gradient g, terms of both signs: next to each, gradmag.<name> = sum |g * x * [x <= 0]| of the same run
(float64), the scale on which the rounding of that sum lives.
main() asserts what makes the fixture worth having, so a change of the seeded values fails here instead of writing a weak fixture: every
PReLU sees 25-75 % positive inputs, the mask keeps 65-75 %, training and eval outputs differ, and t5 has a negative slope.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save  # noqa: E402
from weights import fill_state_dict  # noqa: E402

SEED = 61
CASES = {'t3': (dict(k=3, nf=64, scale=1, nframes=3), (2, 3, 3, 20, 36)),
         't5': (dict(k=3, nf=32, scale=1, nframes=5), (1, 5, 3, 13, 22))}
FIRST16 = ('frb_1.conv3d_1.weight', 'frb_1.conv3d_2.weight', 'frb_5.conv3d_1.weight', 'frb_5.conv3d_2.weight', 'conv3d_1.weight')
WHOLE = ('conv3d_fe.weight', 'upsample.weight', 'conv3d_2.weight')


def main():
    torch.set_num_threads(8)
    import_reference()
    import models.archs.FSTRN_arch as FSTRN_arch
    arrs = {}
    for tag, (kw, xshape) in CASES.items():
        net = FSTRN_arch.FSTRN(**kw)
        fill_state_dict(net, SEED)
        x = torch.rand(*xshape, generator=torch.Generator().manual_seed(7))
        positive, masks, seen = [], [], {}
        for name, m in net.named_modules():
            if isinstance(m, torch.nn.PReLU):
                m.register_forward_pre_hook(lambda mod, i, n=name: positive.append((n, (i[0] > 0).float().mean().item())))
                m.register_forward_hook(lambda mod, i, o, n=name: seen.__setitem__(n + '.x', i[0].detach()))
                m.register_full_backward_hook(lambda mod, gi, go, n=name: seen.__setitem__(n + '.g', go[0].detach()))
        net.dropout.register_forward_hook(lambda mod, i, o: masks.append(((o != 0) | (i[0] == 0)).numpy()))
        outs = {}
        for mode in ('eval', 'train'):
            net.train(mode == 'train')
            net.zero_grad()
            xi = x.clone().requires_grad_(True)
            torch.manual_seed(5)
            out = net(xi)
            gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(8))
            out.backward(gout)
            outs[mode] = out.detach()
            arrs['%s.%s.out' % (tag, mode)], arrs['%s.%s.gx' % (tag, mode)] = out.detach().numpy(), xi.grad.numpy().copy()
        arrs[tag + '.x'], arrs[tag + '.gout'] = x.numpy(), gout.numpy()
        keep = masks[1]
        assert masks[0].all() and keep.shape == (xshape[0], kw['nf'], xshape[1], xshape[3], xshape[4])
        arrs[tag + '.train.keep'], arrs[tag + '.train.keep_shape'] = np.packbits(keep), np.array(keep.shape, dtype=np.int64)
        slopes = {n: p.item() for n, p in net.named_parameters() if n.endswith('prelu.weight')}
        print(tag, 'kept %.4f' % keep.mean(), '| train - eval %.3f' % (outs['train'] - outs['eval']).abs().max().item(),
              '| max |out| %.3f' % outs['eval'].abs().max().item(), '| slopes', ' '.join('%.2f' % v for v in slopes.values()))
        assert 0.65 <= keep.mean() <= 0.75, keep.mean()
        assert (outs['train'] - outs['eval']).abs().max().item() > 0.01
        assert len(positive) == 12 and len(slopes) == 6
        for name, v in positive:
            assert 0.25 <= v <= 0.75, (tag, name, v)
        if tag == 't5':
            assert min(slopes.values()) < 0, slopes
        sd = net.state_dict()
        assert len(sd) == 34
        arrs[tag + '.keys'] = np.array(list(sd.keys()))
        arrs[tag + '.shapes'] = np.array([list(v.shape) + [0] * (5 - v.dim()) for v in sd.values()], dtype=np.int64)
        for k, p in net.named_parameters():   # (the gradients of the training run, the last one)
            if k.endswith('.bias') or k.endswith('prelu.weight') or k in WHOLE:
                arrs[tag + '.grad.' + k] = p.grad.numpy().copy()
            if k.endswith('prelu.weight'):
                xx, gg = seen[k[:-7] + '.x'].double(), seen[k[:-7] + '.g'].double()
                terms = gg * xx * (xx <= 0)
                assert abs(terms.sum().item() - p.grad.item()) <= 1e-5 * terms.abs().sum().item(), (k, terms.sum().item(), p.grad.item())
                arrs[tag + '.gradmag.' + k] = np.array([terms.abs().sum().item()])
                print(tag, k, 'grad %.5f of magnitude %.3f' % (p.grad.item(), terms.abs().sum().item()))
            elif k in FIRST16:
                arrs[tag + '.grad.' + k] = p.grad.numpy()[:16].copy()
    save('fstrn', **arrs)


if __name__ == '__main__':
    main()
