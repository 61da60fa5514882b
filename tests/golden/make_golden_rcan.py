#!/usr/bin/env python
"""Generate tests/golden/rcan.npz from the reference's OWN RCAN (build container only).

Run from the repo root:   python tests/golden/make_golden_rcan.py
Same recipe as make_golden.py (import_reference / save / weights.fill_state_dict): models.archs.RCAN_arch is imported from the
read-only reference tree and run on CPU; only the .npz written here is committed.
Two cases on one input, x = rand(2, 3, 3, 20, 36) (seed 7), gout = randn (seed 8):
  s1 : num_feat 64, squeeze 16, num_group 2, num_block 2, upscale 1, res_scale 1
  s2 : num_feat 32, squeeze 8, num_group 2, num_block 2, upscale 2, res_scale 0.5   (32-row conv tiles, PixelShuffle, res_scale != 1)
Weights: weights.fill_state_dict(net, 51), then every parameter whose name contains '.attention.' times ATT_GAIN.  The plain fill
leaves the gates inert (0.493 .. 0.505): an error in the attention path would hide below tolerance.  With the gain every attention
module of both cases spans gates from <= 0.21 to >= 0.85 with 25-75 % of its hidden units positive; main() asserts that, so a change
of the seeded values fails here instead of writing a weak fixture.  The two gate figures are compared at the two decimals they are
quoted with: the narrowest module (s1, body.1.residual_group.0) spans 0.2121 .. 0.8471.
Stored per case: x, gout, out, names and shapes of every state_dict entry, and the gradients of every attention parameter, conv_first,
the first and last RCAB convs, body.1.conv, conv_after_body, upsample.0 (s2) and conv_last.  Weight gradients of more than 20000
elements keep their first 16 output channels (as edvr_c3.npz does), which holds the file below 1 MiB.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save  # noqa: E402
from weights import fill_state_dict  # noqa: E402

SEED, ATT_GAIN = 51, 30.0
CASES = {'s1': dict(num_feat=64, squeeze_factor=16, num_group=2, num_block=2, upscale=1, res_scale=1),
         's2': dict(num_feat=32, squeeze_factor=8, num_group=2, num_block=2, upscale=2, res_scale=0.5)}
KEEP = ('conv_first.', 'body.0.residual_group.0.rcab.0.', 'body.0.residual_group.0.rcab.2.', 'body.1.residual_group.1.rcab.0.',
        'body.1.residual_group.1.rcab.2.', 'body.1.conv.', 'conv_after_body.', 'upsample.0.', 'conv_last.')


def fill_rcan(net):
    """The fixture's weights: shared with the tests, which re-create them on the project's own RCAN."""
    fill_state_dict(net, SEED)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if '.attention.' in name:
                p.mul_(ATT_GAIN)
    return net


def main():
    torch.set_num_threads(8)
    import_reference()
    import models.archs.RCAN_arch as RCAN_arch
    arrs = {}
    x = torch.rand(2, 3, 3, 20, 36, generator=torch.Generator().manual_seed(7))
    for tag, kw in CASES.items():
        torch.manual_seed(5)
        net = fill_rcan(RCAN_arch.RCAN(num_in_ch=3, num_out_ch=3, num_frames=3, **kw))
        # watch every attention module: gate span and share of positive hidden units
        stats = []
        for name, m in net.named_modules():
            if isinstance(m, RCAN_arch.ChannelAttention):
                m.attention[2].register_forward_hook(lambda mod, i, o, n=name: stats.append((n, 'hidden', (o > 0).float().mean().item())))
                m.attention[4].register_forward_hook(lambda mod, i, o, n=name: stats.append((n, 'gate', (o.min().item(), o.max().item()))))
        out = net(x)
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(8))
        out.backward(gout)
        assert len(stats) == 2 * kw['num_group'] * kw['num_block']
        for name, kind, v in stats:
            print(tag, name, kind, v)
            if kind == 'hidden':
                assert 0.25 <= v <= 0.75, (tag, name, v)
            else:
                assert round(v[0], 2) <= 0.21 and round(v[1], 2) >= 0.85, (tag, name, v)
        arrs[tag + '.x'], arrs[tag + '.gout'], arrs[tag + '.out'] = x.numpy(), gout.numpy(), out.detach().numpy()
        sd = net.state_dict()
        arrs[tag + '.keys'] = np.array(list(sd.keys()))
        arrs[tag + '.shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
        for k, p in net.named_parameters():
            if '.attention.' in k or k.startswith(KEEP):
                g = p.grad.numpy()
                arrs[tag + '.grad.' + k] = (g[:16] if g.ndim == 4 and g.size > 20000 else g).copy()
                if '.attention.' in k:
                    print(tag, 'max |grad|', k, p.grad.abs().max().item())
    save('rcan', **arrs)


if __name__ == '__main__':
    main()
