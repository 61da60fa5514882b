"""RCAN on the MI355X path: the reference's attention baseline for RealVSR (train_RCAN_RealVSR_YCbCr_{Split,Combine}.yml).
Mirrors codes/models/archs/RCAN_arch.py (Upsample :8-27, ChannelAttention :30-48, RCAB :51-70, ResidualGroup :73-95, RCAN :98-163):
same constructor arguments, forward(x[B, N, C, H, W] or x[B, N*C, H, W]) and state_dict keys (the Sequential holders of the reference
are kept so checkpoints load with strict=True); every layer runs through realvsr_amd.functional.

  RCAB           one autograd node, RF.rcab: conv + ReLU, conv, the fused channel-attention operator with the block input as residual
  ResidualGroup  its closing conv takes the group input as fused residual
  RCAN           conv_after_body takes the long skip as fused residual; Upsample is the fused conv + PixelShuffle
"""
import math

import torch.nn as nn

from . import arch_util
from .. import functional as RF


class Upsample(nn.Sequential):
    """Holder of the (conv, PixelShuffle(2)) pairs for power-of-two scales; forward fuses each pair into one kernel.  Scale 3 (one
    conv + PixelShuffle(3) in the reference) is not on the MI355X path."""

    def __init__(self, scale, num_feat):
        m = []
        if (scale & (scale - 1)) == 0:
            for _ in range(int(math.log(scale, 2))):
                m.append(nn.Conv2d(num_feat, 4 * num_feat, 3, 1, 1))
                m.append(nn.PixelShuffle(2))
        elif scale == 3:
            raise NotImplementedError('Upsample: scale 3 (PixelShuffle(3)) is not on the MI355X path; only power-of-two scales are')
        else:
            raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
        super(Upsample, self).__init__(*m)

    def forward(self, x):
        for m in self:
            if isinstance(m, nn.Conv2d):
                x = RF.conv2d(x, m, pixel_shuffle=True)
        return x


class ChannelAttention(nn.Module):
    """x * sigmoid(conv(relu(conv(avg_pool(x))))).  `attention` holds the parameters under the reference's names (attention.1 / .3);
    forward is one fused operator.  residual / res_scale: out = residual + res_scale * (x * gate), the tail of an RCAB."""

    def __init__(self, num_feat, squeeze_factor=16):
        super(ChannelAttention, self).__init__()
        self.attention = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            nn.Conv2d(num_feat, num_feat // squeeze_factor, 1, padding=0),
            nn.ReLU(inplace=True),
            nn.Conv2d(num_feat // squeeze_factor, num_feat, 1, padding=0),
            nn.Sigmoid())

    def forward(self, x, residual=None, res_scale=1.0):
        return RF.channel_attention(x, self.attention[1], self.attention[3], x=residual, res_scale=res_scale)


class RCAB(nn.Module):
    """Residual channel attention block: x + res_scale * CA(conv(relu(conv(x))))."""

    def __init__(self, num_feat, squeeze_factor=16, res_scale=1):
        super(RCAB, self).__init__()
        self.res_scale = res_scale
        self.rcab = nn.Sequential(
            nn.Conv2d(num_feat, num_feat, 3, 1, 1), nn.ReLU(True),
            nn.Conv2d(num_feat, num_feat, 3, 1, 1),
            ChannelAttention(num_feat, squeeze_factor))

    def forward(self, x):
        att = self.rcab[3].attention
        return RF.rcab(x, self.rcab[0], self.rcab[2], att[1], att[3], self.res_scale)


class ResidualGroup(nn.Module):
    def __init__(self, num_feat, num_block, squeeze_factor=16, res_scale=1):
        super(ResidualGroup, self).__init__()
        self.residual_group = arch_util.make_layer(RCAB, num_block, num_feat=num_feat, squeeze_factor=squeeze_factor,
                                                   res_scale=res_scale)
        self.conv = nn.Conv2d(num_feat, num_feat, 3, 1, 1)

    def forward(self, x):
        return RF.conv2d(self.residual_group(x), self.conv, residual=x)


class RCAN(nn.Module):
    """Residual channel attention network: (B, N, C, H, W) or (B, N*C, H, W) -> (B, num_out_ch, s*H, s*W).  img_range / rgb_mean are
    accepted and unused, as in the reference (its normalisation lines are commented out)."""

    def __init__(self, num_in_ch, num_out_ch, num_frames, num_feat=64, num_group=10, num_block=16, squeeze_factor=16, upscale=4,
                 res_scale=1, img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040)):
        super(RCAN, self).__init__()
        self.conv_first = nn.Conv2d(num_in_ch * num_frames, num_feat, 3, 1, 1)
        self.body = arch_util.make_layer(ResidualGroup, num_group, num_feat=num_feat, num_block=num_block,
                                         squeeze_factor=squeeze_factor, res_scale=res_scale)
        self.conv_after_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.upsample = Upsample(upscale, num_feat)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)

    def forward(self, x):
        if x.dim() == 5:
            B, N, C, H, W = x.shape
            x = x.reshape(B, N * C, H, W)
        x = RF.conv2d(x, self.conv_first)
        res = RF.conv2d(self.body(x), self.conv_after_body, residual=x)
        return RF.conv2d(self.upsample(res), self.conv_last)
