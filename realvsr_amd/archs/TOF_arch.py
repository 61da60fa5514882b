"""TOF on the MI355X path: SpyNet optical-flow alignment followed by an MSRResNet reconstruction.  Mirrors
codes/models/archs/TOF_arch.py (SpyNet_Block :10-37, SpyNet :40-88, MSRResNet :91-145, TOF :148-189): same constructor arguments,
forward(x[B, T, C, H, W]) and state_dict keys (the reference's Sequential holders are kept, so its checkpoints load with strict=True);
every layer runs through realvsr_amd.functional.  The 7x7 convolutions of SpyNet run on the exact-f32 matrix-core kernels in every GEMM
mode; the pyramids, the flow upsampling and the warp are the operators of csrc/flow_kernels.hip.
"""
import functools

import torch
import torch.nn as nn

from . import arch_util
from .. import functional as RF


class SpyNet_Block(nn.Module):
    """Five 7x7 convs, BatchNorm + ReLU between them: [ref, nbr, flow] (B, ic, H, W) -> flow update (B, 2, H, W)."""

    def __init__(self, ic=8):
        super(SpyNet_Block, self).__init__()
        self.block = nn.Sequential(
            nn.Conv2d(in_channels=ic, out_channels=32, kernel_size=7, stride=1, padding=3),
            nn.BatchNorm2d(32), nn.ReLU(inplace=True),
            nn.Conv2d(in_channels=32, out_channels=64, kernel_size=7, stride=1, padding=3),
            nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.Conv2d(in_channels=64, out_channels=32, kernel_size=7, stride=1, padding=3),
            nn.BatchNorm2d(32), nn.ReLU(inplace=True),
            nn.Conv2d(in_channels=32, out_channels=16, kernel_size=7, stride=1, padding=3),
            nn.BatchNorm2d(16), nn.ReLU(inplace=True),
            nn.Conv2d(in_channels=16, out_channels=2, kernel_size=7, stride=1, padding=3))
        arch_util.initialize_weights(self.block, 0.1)

    def forward(self, x):
        h = x
        for i in range(0, 12, 3):
            h = RF.conv2d(h, self.block[i])
            h = RF.batch_norm_lrelu(h, self.block[i + 1], slope=0.0)   # BatchNorm + ReLU as one operator (LeakyReLU at slope 0)
        return RF.conv2d(h, self.block[12])


class SpyNet(nn.Module):
    """Ranjan et al., Optical Flow Estimation using a Spatial Pyramid Network: the flow of the coarsest of K + 1 pyramid levels, then
    per level upsample, warp and refine."""

    def __init__(self, K=3):
        super(SpyNet, self).__init__()
        self.K = K
        self.block0 = SpyNet_Block(ic=6)
        self.blocks = nn.ModuleList([SpyNet_Block(ic=8) for _ in range(K)])

    def forward(self, ref, nbr):
        """ref, nbr (B, 3, H, W) -> (nbr warped onto ref (B, 3, H, W), flow in pixels (B, 2, H, W))."""
        H, W = ref.shape[-2:]
        if H % (1 << self.K) or W % (1 << self.K):
            raise RuntimeError('SpyNet: a %d x %d frame; H and W must be divisible by 2**K = %d (pad the input)' % (H, W, 1 << self.K))
        ref, nbr = [ref], [nbr]
        for _ in range(self.K):
            ref.insert(0, RF.avg_pool2(ref[0]))
            nbr.insert(0, RF.avg_pool2(nbr[0]))
        flow = self.block0(torch.cat([ref[0], nbr[0]], 1))
        for i in range(self.K):
            flow_up = RF.upsample2_ac(flow, scale=2.0)
            flow = flow_up + self.blocks[i](torch.cat([ref[i + 1], RF.flow_warp(nbr[i + 1], flow_up.permute(0, 2, 3, 1)), flow_up], 1))
        return RF.flow_warp(nbr[-1], flow.permute(0, 2, 3, 1)), flow


class MSRResNet(nn.Module):
    """conv + nb residual blocks + PixelShuffle tail, added onto the bilinearly upsampled centre frame."""

    def __init__(self, in_nc=3, out_nc=3, nf=64, nb=16, upscale=4):
        super(MSRResNet, self).__init__()
        if upscale == 3:
            raise NotImplementedError('MSRResNet: upscale 3 needs PixelShuffle(3), which the conv epilogue on the MI355X path does not have')
        self.upscale = upscale
        self.conv_first = nn.Conv2d(in_nc, nf, 3, 1, 1, bias=True)
        self.recon_trunk = arch_util.make_layer(functools.partial(arch_util.ResidualBlock_noBN, nf=nf), nb)
        if self.upscale == 2:
            self.upconv1 = nn.Conv2d(nf, nf * 4, 3, 1, 1, bias=True)
            self.pixel_shuffle = nn.PixelShuffle(2)
        elif self.upscale == 4:
            self.upconv1 = nn.Conv2d(nf, nf * 4, 3, 1, 1, bias=True)
            self.upconv2 = nn.Conv2d(nf, nf * 4, 3, 1, 1, bias=True)
            self.pixel_shuffle = nn.PixelShuffle(2)
        self.HRconv = nn.Conv2d(nf, nf, 3, 1, 1, bias=True)
        self.conv_last = nn.Conv2d(nf, out_nc, 3, 1, 1, bias=True)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)
        # as in the reference: at upscale 1 only the residual blocks carry the 0.1 scale
        if self.upscale == 2 or self.upscale == 4:
            arch_util.initialize_weights([self.conv_first, self.upconv1, self.HRconv, self.conv_last], 0.1)
        if self.upscale == 4:
            arch_util.initialize_weights(self.upconv2, 0.1)

    def forward(self, x):
        C = x.size(1)
        x_base = x[:, C // 2 - 1:C // 2 + 2, :, :] if C > 3 else x   # multi-frame input: the centre frame
        out = self.recon_trunk(RF.conv2d(x, self.conv_first, RF.ACT_LRELU))
        if self.upscale == 4:
            out = RF.conv2d(out, self.upconv1, RF.ACT_LRELU, pixel_shuffle=True)
            out = RF.conv2d(out, self.upconv2, RF.ACT_LRELU, pixel_shuffle=True)
        elif self.upscale == 2:
            out = RF.conv2d(out, self.upconv1, RF.ACT_LRELU, pixel_shuffle=True)
        base = RF.upsample_bilinear(x_base, self.upscale) if self.upscale > 1 else x_base
        return RF.conv2d(RF.conv2d(out, self.HRconv, RF.ACT_LRELU), self.conv_last, residual=base)   # `out += base` in the epilogue


class TOF(nn.Module):
    """Video SR on SpyNet + MSRResNet: every neighbour is warped onto the centre frame, the warped clip is reconstructed.
    in_nc is the number of channels of ONE frame.  (B, T, C, H, W) -> (B, out_nc, s*H, s*W)."""

    def __init__(self, nframes=3, K=3, in_nc=3, out_nc=3, nf=32, nb=12, upscale=2):
        super(TOF, self).__init__()
        self.nframes = nframes
        self.align_arch = SpyNet(K=K)
        self.sr_arch = MSRResNet(in_nc=nframes * in_nc, out_nc=out_nc, nf=nf, nb=nb, upscale=upscale)

    def forward(self, x):
        B, T, C, H, W = x.size()
        assert T == self.nframes
        ref_index = T // 2
        ref_frame = x[:, ref_index].contiguous()
        y = []
        # one neighbour after the other, as in the reference: a batch of them would change the BatchNorm statistics
        for i in range(T):
            if i == ref_index:
                y.append(ref_frame)
            else:
                y.append(self.align_arch(ref_frame, x[:, i].contiguous())[0])
        return self.sr_arch(torch.cat(y, dim=1))
