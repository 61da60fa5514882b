"""Hot-path losses with the reference's class names and constructor arguments
(codes/models/loss.py:10-23 CharbonnierLoss, :160-192 PyramidLoss, :195-224 LapPyrLoss).

``lf_mode='ssim'`` / ``hf_mode='ssim'`` call the third-party ``IQA_pytorch.SSIM`` in the
reference (loss.py:7,203,209) -- an unpinned pip dependency that is not vendored and is absent
here.  ``SSIM`` below is this build's implementation of that package's published algorithm (one
fused HIP kernel each way); it is checked against the restatement in oracle/ssim_oracle.py, but
there is no copy of the package to pin either against: parity of the 'ssim' mode is UNPINNED.
Every other mode is pinned by fixtures generated from the reference's own loss.py."""
import torch
import torch.nn as nn

from . import functional as RF
from . import util


class CharbonnierLoss(nn.Module):
    """Charbonnier Loss (L1)"""

    def __init__(self, eps=1e-6, reduction='mean'):
        super(CharbonnierLoss, self).__init__()
        self.eps = eps
        self.reduction = reduction

    def forward(self, x, y):
        return RF.charbonnier(x, y, self.eps, 'mean' if self.reduction == 'mean' else 'sum')


class HuberLoss(nn.Module):
    """Huber Loss (codes/models/loss.py:26-40): 0.5 q^2 + delta (|d| - q), q = min(|d|, delta)."""

    def __init__(self, delta=1e-2, reduction='mean'):
        super(HuberLoss, self).__init__()
        self.delta = delta
        self.reduction = reduction

    def forward(self, x, y):
        return RF.pixel_loss(x, y, RF.PIX_HUBER, self.delta, 'mean' if self.reduction == 'mean' else 'sum')


class _ElementwiseLoss(nn.Module):
    """nn.L1Loss / nn.MSELoss stand-ins (loss.py:167-170) on the HIP reduction kernel."""
    mode = RF.PIX_L1

    def __init__(self, reduction='mean'):
        super(_ElementwiseLoss, self).__init__()
        if reduction not in ('mean', 'sum'):
            raise ValueError("reduction must be 'mean' or 'sum' (got %r)" % (reduction,))
        self.reduction = reduction

    def forward(self, x, y):
        return RF.pixel_loss(x, y, self.mode, 0.0, self.reduction)


class L1Loss(_ElementwiseLoss):
    mode = RF.PIX_L1


class MSELoss(_ElementwiseLoss):
    mode = RF.PIX_L2


class SSIM(nn.Module):
    """``IQA_pytorch.SSIM(channels)(X, Y, as_loss=True)`` -> 1 - mean SSIM (11x11 Gaussian window, sigma 1.5, valid
    correlation, C1 = 0.01^2, C2 = 0.03^2, contrast-structure map clamped at 0); ``as_loss=False`` returns the
    per-image score without a graph.  Third-party algorithm restated from its publication: parity unpinned."""

    def __init__(self, channels=3):
        super(SSIM, self).__init__()
        self.channels = channels

    def forward(self, X, Y, as_loss=True):
        assert X.shape == Y.shape
        if as_loss:
            return RF.ssim_loss(X, Y)
        with torch.no_grad():
            return torch.stack([1.0 - RF.ssim_loss(X[i:i + 1], Y[i:i + 1]) for i in range(X.shape[0])])


class GWLoss(nn.Module):
    """Gradient Weighted Loss (codes/models/loss.py:54-80) -- the CbCr term of the reference's training loss
    (VideoSR_AllPair_model_YCbCr_Split.py:184).  The Sobel filters are constants of the HIP kernel."""

    def __init__(self, w=4, reduction='mean'):
        super(GWLoss, self).__init__()
        self.w = w
        self.reduction = reduction

    def forward(self, x1, x2):
        return RF.gw_loss(x1, x2, self.w, 'mean' if self.reduction == 'mean' else 'sum')


class GANLoss(nn.Module):
    """GAN loss (codes/models/loss.py:102-133) for 'gan' and 'ragan': BCEWithLogitsLoss (mean) against a constant label, one HIP
    reduction.  ``other`` (an addition for RaGAN) scores ``input - mean(other)`` with the gradient reaching ``other`` through the mean,
    so the model never composes that difference from torch ops.  'lsgan' / 'wgan-gp' are not built (NotImplementedError)."""

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0):
        super(GANLoss, self).__init__()
        self.gan_type = gan_type.lower()
        self.real_label_val = real_label_val
        self.fake_label_val = fake_label_val
        if self.gan_type not in ('gan', 'ragan'):
            raise NotImplementedError('GAN type [{:s}] is not built (gan | ragan)'.format(self.gan_type))

    def forward(self, input, target_is_real, other=None):
        target = self.real_label_val if target_is_real else self.fake_label_val
        return RF.gan_criterion(input, target, other)


class PyramidLoss(nn.Module):
    """Pyramid Loss"""

    def __init__(self, num_levels=3, pyr_mode='gau', loss_mode='l1', reduction='mean'):
        super(PyramidLoss, self).__init__()
        self.num_levels = num_levels
        self.pyr_mode = pyr_mode
        self.loss_mode = loss_mode
        assert self.pyr_mode == 'gau' or self.pyr_mode == 'lap'
        if self.loss_mode == 'l1':
            self.loss = L1Loss(reduction=reduction)
        elif self.loss_mode == 'l2':
            self.loss = MSELoss(reduction=reduction)
        elif self.loss_mode == 'hb':
            self.loss = HuberLoss(reduction=reduction)
        elif self.loss_mode == 'cb':
            self.loss = CharbonnierLoss(reduction=reduction)
        else:
            raise ValueError()

    def forward(self, x, y):
        pyr = util.gau_pyramid if self.pyr_mode == 'gau' else util.lap_pyramid
        pyr_x = pyr(img=x, max_levels=self.num_levels)
        pyr_y = pyr(img=y, max_levels=self.num_levels)
        loss = 0
        for i in range(self.num_levels):
            loss = loss + self.loss(pyr_x[i], pyr_y[i])
        return loss


class LapPyrLoss(nn.Module):
    """Pyramid Loss"""

    def __init__(self, num_levels=3, lf_mode='ssim', hf_mode='cb', reduction='mean'):
        super(LapPyrLoss, self).__init__()
        self.num_levels = num_levels
        self.lf_mode = lf_mode
        self.hf_mode = hf_mode
        if lf_mode == 'ssim':
            self.lf_loss = SSIM(channels=1)
        elif lf_mode == 'cb':
            self.lf_loss = CharbonnierLoss(reduction=reduction)
        else:
            raise ValueError()
        if hf_mode == 'ssim':
            self.hf_loss = SSIM(channels=1)
        elif hf_mode == 'cb':
            self.hf_loss = CharbonnierLoss(reduction=reduction)
        else:
            raise ValueError()

    def forward(self, x, y):
        pyr_x = util.laplacian_pyramid(img=x, max_levels=self.num_levels)
        pyr_y = util.laplacian_pyramid(img=y, max_levels=self.num_levels)
        loss = self.lf_loss(pyr_x[-1], pyr_y[-1])
        for i in range(self.num_levels - 1):
            loss = loss + self.hf_loss(pyr_x[i], pyr_y[i])
        return loss
