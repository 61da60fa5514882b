"""The patch discriminators of the GAN stage (codes/models/archs/discriminator_arch.py:46-92 PatchDiscriminator, :279-305
MultiscaleDiscriminator_v4) with the reference's constructor arguments and state_dict schema.

``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.LeakyReLU`` modules are kept in the reference's ``nn.Sequential`` (indices 0-20 for
n_block 2) as parameter and buffer holders, so ``state_dict``, ``train()`` / ``eval()`` and loading behave as in the reference;
the forward walks that Sequential on the fused HIP operators of realvsr_amd.functional:
  * conv (5x5, pad 2) + bias + LeakyReLU(0.2) -> one conv kernel;
  * conv (no bias) -> BatchNorm2d -> LeakyReLU(0.2) -> one conv kernel + the fused BN + LReLU operator;
  * the last conv (-> 1 channel, bias) -> one conv kernel.
Other norm layers, kernel sizes and the pixel / U-Net discriminators are not built (NotImplementedError).
"""
import torch.nn as nn

from .. import functional as RF


def _is_lrelu(m):
    return isinstance(m, nn.LeakyReLU)


def patch_forward(seq, x):
    """Run a PatchDiscriminator ``model`` Sequential on the HIP operators."""
    mods = list(seq)
    i, n = 0, len(mods)
    while i < n:
        m = mods[i]
        if not isinstance(m, nn.Conv2d):
            raise NotImplementedError('patch_forward: unexpected module %s at index %d' % (type(m).__name__, i))
        nxt = mods[i + 1] if i + 1 < n else None
        if isinstance(nxt, nn.BatchNorm2d):
            if i + 2 >= n or not _is_lrelu(mods[i + 2]):
                raise NotImplementedError('patch_forward: BatchNorm2d must be followed by LeakyReLU')
            x = RF.conv2d(x, m)
            x = RF.batch_norm_lrelu(x, nxt, mods[i + 2].negative_slope)
            i += 3
        elif nxt is not None and _is_lrelu(nxt):
            x = RF.conv2d(x, m, act=RF.ACT_LRELU, slope=nxt.negative_slope)
            i += 2
        else:
            x = RF.conv2d(x, m)
            i += 1
    return x


class PatchDiscriminator(nn.Module):
    """Defines a PatchGAN (NxN PatchGAN) discriminator"""

    def __init__(self, input_nc, ndf=64, n_block=2, norm_layer=nn.BatchNorm2d, kw=5, padw=2):
        super(PatchDiscriminator, self).__init__()
        if norm_layer is not nn.BatchNorm2d:
            raise NotImplementedError('PatchDiscriminator: only norm_layer=nn.BatchNorm2d is built')
        if kw != 5 or padw != 2:
            raise NotImplementedError('PatchDiscriminator: only kw=5, padw=2 is built')
        use_bias = False   # (BatchNorm2d has affine parameters)
        sequence = [nn.Conv2d(input_nc, ndf, kernel_size=kw, stride=1, padding=padw), nn.LeakyReLU(0.2, True)]
        nf_mult = 1
        for n in range(n_block):
            nf_mult_prev = nf_mult
            nf_mult = min(2 ** n, 8)
            sequence += [
                nn.Conv2d(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=2, padding=padw, bias=use_bias),
                norm_layer(ndf * nf_mult),
                nn.LeakyReLU(0.2, True),
                nn.Conv2d(ndf * nf_mult, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw, bias=use_bias),
                norm_layer(ndf * nf_mult),
                nn.LeakyReLU(0.2, True)
            ]
        nf_mult_prev = nf_mult
        nf_mult = min(2 ** n_block, 8)
        sequence += [
            nn.Conv2d(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw, bias=use_bias),
            norm_layer(ndf * nf_mult),
            nn.LeakyReLU(0.2, True),
            nn.Conv2d(ndf * nf_mult, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw, bias=use_bias),
            norm_layer(ndf * nf_mult),
            nn.LeakyReLU(0.2, True)
        ]
        sequence += [nn.Conv2d(ndf * nf_mult, 1, kernel_size=kw, stride=1, padding=padw)]  # output 1 channel prediction map
        self.model = nn.Sequential(*sequence)

    def forward(self, input):
        return patch_forward(self.model, input)


class MultiscaleDiscriminator_v4(nn.Module):
    """Multi-scale Discriminator (discriminators are of same architectures): ``forward(list)`` applies D_{num_D-1-i} to input[i].
    (The reference also constructs an AvgPool2d ``downsample`` that its forward never calls and that holds no state.)"""

    def __init__(self, input_nc, ndf=64, n_block=2, norm_layer=nn.BatchNorm2d, num_D=3, gan_type='patch'):
        super(MultiscaleDiscriminator_v4, self).__init__()
        if gan_type != 'patch':
            raise NotImplementedError("MultiscaleDiscriminator_v4: only gan_type='patch' is built (got %r)" % (gan_type,))
        self.num_D = num_D
        self.n_block = n_block
        for i in range(num_D):
            netD = PatchDiscriminator(input_nc, ndf, n_block, norm_layer)
            setattr(self, 'D_{}'.format(str(i)), netD.model)

    def forward(self, input):
        num_D = self.num_D
        assert len(input) == num_D
        return [patch_forward(getattr(self, 'D_{}'.format(str(num_D - 1 - i))), input[i]) for i in range(num_D)]
