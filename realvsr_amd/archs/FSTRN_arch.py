"""FSTRN on the MI355X path: the reference's 3-D baseline for RealVSR (train_FSTRN_RealVSR_YCbCr_{Split,Combine}.yml,
train_FSTRN_Vimeo90K.yml).  Mirrors codes/models/archs/FSTRN_arch.py (FRB :11-22, FSTRN :25-69): same constructor arguments, forward
(x[B, T, C, H, W] -> the centre frame [B, 3, H, W]) and state_dict keys -- the parameters live in the reference's nn.Conv3d /
nn.ConvTranspose3d / nn.PReLU / nn.Dropout holders, so its checkpoints load with strict=True; every layer runs through
realvsr_amd.functional.

Inside the network the activations are FRAME-MAJOR, [T, B, C, H, W] contiguous: a range of frames is a contiguous batch for the 2-D
kernels, and the three temporal taps of a pixel lie one frame apart.

  3x3x3 convs   RF.conv3d_frames: three accumulated 3x3 convolutions over frame ranges
  FRB           one autograd node, RF.frb: PReLU (from the previous block's kernel where there is one), the (1,3,3) convolution as a 3x3
                convolution over T * B images, the fused (3,1,1) temporal convolution with the block input as residual
  LSRNet        the long skip, PReLU and Dropout in one pass (RF.prelu); only the centre frame leaves the network, so conv3d_2 is
                computed at t = center alone, upsample and conv3d_1 at the frames it reads.  The other frames receive zero gradient in the
                reference too, so the gradients are the reference's.
k = 3 and scale = 1 are what every option file uses; other values are refused (strided ConvTranspose3d, trilinear upsampling).
"""
import torch
import torch.nn as nn

from .. import functional as RF


class FRB(nn.Module):
    """Fast spatio-temporal residual block: x + conv3d_2(conv3d_1(prelu(x))) on frame-major x [T, B, C, H, W]."""

    def __init__(self, k=3, nf=64):
        super(FRB, self).__init__()
        if k != 3:
            raise NotImplementedError('FRB: k = %r is not on the MI355X path; k = 3 is' % (k,))
        self.prelu = nn.PReLU()
        self.conv3d_1 = nn.Conv3d(nf, nf, (1, k, k), stride=(1, 1, 1), padding=(0, 1, 1), bias=True)
        self.conv3d_2 = nn.Conv3d(nf, nf, (k, 1, 1), stride=(1, 1, 1), padding=(1, 0, 0), bias=True)

    def forward(self, x, px=None, next_prelu=None):
        """px: prelu(x) when the previous block has produced it; next_prelu: the next block's PReLU, returns (out, next_prelu(out))."""
        return RF.frb(x, self.prelu, self.conv3d_1, self.conv3d_2, px=px, next_prelu=next_prelu)


class FSTRN(nn.Module):
    """Fast spatio-temporal residual network."""

    def __init__(self, k=3, nf=64, scale=4, nframes=5):
        super(FSTRN, self).__init__()
        if k != 3:
            raise NotImplementedError('FSTRN: k = %r is not on the MI355X path; k = 3 is' % (k,))
        if scale != 1:
            raise NotImplementedError('FSTRN: scale %r (strided ConvTranspose3d, trilinear upsampling) is not on the MI355X path; '
                                      'scale 1 is' % (scale,))
        self.k = k
        self.nf = nf
        self.scale = scale
        self.center = nframes // 2
        #### LFENet
        self.conv3d_fe = nn.Conv3d(3, nf, (k, k, k), stride=(1, 1, 1), padding=(1, 1, 1), bias=True)
        #### FRBs
        self.frb_1 = FRB(k=k, nf=nf)
        self.frb_2 = FRB(k=k, nf=nf)
        self.frb_3 = FRB(k=k, nf=nf)
        self.frb_4 = FRB(k=k, nf=nf)
        self.frb_5 = FRB(k=k, nf=nf)
        #### LSRNet
        self.prelu = nn.PReLU()
        self.dropout = nn.Dropout(p=0.3, inplace=False)
        self.conv3d_1 = nn.Conv3d(nf, nf, (k, k, k), stride=(1, 1, 1), padding=(1, 1, 1), bias=True)
        self.upsample = nn.ConvTranspose3d(nf, nf, (1, self.scale, self.scale), stride=(1, self.scale, self.scale), bias=True)
        self.conv3d_2 = nn.Conv3d(nf, 3, (k, k, k), stride=(1, 1, 1), padding=(1, 1, 1), bias=True)

    def dropout_keep_mask(self, like):
        """The keep mask of nn.Dropout(p) for a frame-major activation `like` [T, B, C, H, W]: a bool tensor drawn with torch on the
        device.  The one place a mask is drawn: a test replaces this method to inject a recorded mask."""
        return torch.rand(like.shape, device=like.device) >= self.dropout.p

    def forward(self, x):
        """x: [B, T, C, H, W] -> [B, 3, H, W], the centre frame."""
        T = x.shape[1]
        if not 0 <= self.center < T:
            raise RuntimeError('FSTRN: %d frames, centre frame %d' % (T, self.center))
        xf = x.transpose(0, 1).contiguous()   # frame-major
        #### LFENet
        lr_res = RF.conv3d_frames(xf, self.conv3d_fe)
        #### FRBs: every block's kernel also writes the next block's PReLU
        blocks = (self.frb_1, self.frb_2, self.frb_3, self.frb_4, self.frb_5)
        out, px = lr_res, None
        for i, blk in enumerate(blocks):
            nxt = blocks[i + 1].prelu if i + 1 < len(blocks) else None
            res = blk(out, px=px, next_prelu=nxt)
            out, px = res if nxt is not None else (res, None)
        #### LSRNet: lr_res + out, PReLU and Dropout in one pass
        training = self.training and self.dropout.p > 0
        keep = self.dropout_keep_mask(out) if training else None
        out = RF.prelu(out, self.prelu, b=lr_res, keep=keep, p=self.dropout.p if training else 0.0)
        # conv3d_2 at the centre frame reads upsample (per frame) at [u0, u1), which needs conv3d_1 there
        c = self.center
        u0, u1 = max(c - 1, 0), min(c + 2, T)
        out = RF.conv3d_frames(out, self.conv3d_1, frames=(u0, u1))
        out = RF.conv_transpose1x1(out, self.upsample)
        #### Cross-space residual connection: at scale 1 the trilinear resize is the identity
        out = RF.conv3d_frames(out, self.conv3d_2, frames=(c - u0, c - u0 + 1), residual=xf[c:c + 1])
        return out[0]
