"""Float64 references of the memory-bound operators of csrc/misc_kernels.hip and csrc/train_kernels.hip (test infrastructure).

Plain helper of test_glue_reference_host.py (which pins these functions to the reference project's own numbers, the committed
fixtures) and of test_gpu_glue_edges.py (which holds the HIP kernels to them at the edge shapes).  Every function is written from
the operation's definition in ordinary torch CPU operators and follows the dtype of its arguments; gradients come from autograd.
Nothing here looks at how a kernel indexes: reflection, zero insertion, clipping of a window at the border are F.pad / slicing.

  conv_gauss, pyr_down, pyr_upsample, pyr_updiff, laplacian_pyramid / lap_pyramid / gau_pyramid   (utils/util.py:503-554)
  upsample_bilinear, maxavgpool, tsa_temporal, tsa_output                                        (EDVR_arch.py:111-124,171-207)
  charbonnier, l1, l2, huber, gw_loss, ssim_loss                                                 (loss.py:10-80,203-209)
  adam_step                                                                                     (torch.optim.Adam, single tensor)
  augment_clips                                                                                 (augments_video_allpair.py)"""
import torch
import torch.nn.functional as F

from oracle import ssim_oracle


# ------------------------------------------------------------------------------------------ pyramids
def conv_gauss(x, gain=1.0):
    """Reflect-pad 2, depthwise 5 x 5 binomial outer([1, 4, 6, 4, 1]) / 256 * gain."""
    C = x.shape[1]
    k1 = torch.tensor([1., 4., 6., 4., 1.], dtype=x.dtype)
    k = (torch.outer(k1, k1) / 256. * gain).expand(C, 1, 5, 5)
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode='reflect'), k, groups=C)


def pyr_down(x):
    return conv_gauss(x)[..., ::2, ::2]


def pyr_upsample(x):
    """Zero-insert to twice the size (the samples sit at the even positions), then conv_gauss with gain 4."""
    B, C, H, W = x.shape
    z = x.new_zeros(B, C, 2 * H, 2 * W)
    z[..., ::2, ::2] = x
    return conv_gauss(z, 4.0)


def pyr_updiff(cur, down):
    return cur - pyr_upsample(down)


def laplacian_pyramid(img, max_levels=3):
    """max_levels - 1 band-pass levels and the low-pass residual."""
    current, pyr = img, []
    for _ in range(max_levels - 1):
        down = pyr_down(current)
        pyr.append(pyr_updiff(current, down))
        current = down
    pyr.append(current)
    return pyr


def lap_pyramid(img, max_levels=3):
    """max_levels band-pass levels, no residual."""
    current, pyr = img, []
    for _ in range(max_levels):
        down = pyr_down(current)
        pyr.append(pyr_updiff(current, down))
        current = down
    return pyr


def gau_pyramid(img, max_levels=3):
    current, pyr = img, [img]
    for _ in range(max_levels - 1):
        current = pyr_down(current)
        pyr.append(current)
    return pyr


PYRAMIDS = {'laplacian': laplacian_pyramid, 'lap': lap_pyramid, 'gau': gau_pyramid}


# ------------------------------------------------------------------------------------------ resampling / fusion
def upsample_bilinear(x, factor=2, scale=1.0):
    return F.interpolate(x, scale_factor=factor, mode='bilinear', align_corners=False) * scale


def maxavgpool(x):
    """cat(max_pool2d, avg_pool2d) with kernel 3, stride 2, padding 1 (the average counts the padding).  torch's CPU max_pool2d takes a
    new maximum only on `>`: the first maximum in scan order keeps the gradient (test_glue_reference_host.py checks that)."""
    return torch.cat([F.max_pool2d(x, 3, 2, 1), F.avg_pool2d(x, 3, 2, 1)], 1)


def first_max_routing(x, gmax):
    """Gradient of the max half alone, written out: every 3 x 2 x 1 window sends its output gradient to the first of its maxima in
    row-major scan order, positions outside the image never win.  x: (B, C, H, W), gmax: (B, C, Ho, Wo)."""
    B, C, H, W = x.shape
    Ho, Wo = gmax.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1), value=float('-inf'))
    gin = torch.zeros(B, C, H + 2, W + 2, dtype=gmax.dtype)
    for oy in range(Ho):
        for ox in range(Wo):
            win = xp[:, :, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3].reshape(B, C, 9)
            t = torch.argmax(win, dim=2)        # (the first of several maxima)
            for b in range(B):
                for c in range(C):
                    ti = int(t[b, c])
                    gin[b, c, 2 * oy + ti // 3, 2 * ox + ti % 3] += gmax[b, c, oy, ox]
    return gin[:, :, 1:-1, 1:-1]


def tsa_temporal(emb, emb_ref, aligned, frame_major=False):
    """aligned * sigmoid(<emb, emb_ref> over channels), as (B, N * C, H, W).  emb / aligned are (B, N, C, H, W), or (N, B, C, H, W) when
    frame_major; emb_ref is (B, C, H, W)."""
    if frame_major:
        emb, aligned = emb.transpose(0, 1), aligned.transpose(0, 1)
    B, N, C, H, W = aligned.shape
    prob = torch.sigmoid((emb * emb_ref.unsqueeze(1)).sum(2, keepdim=True))
    return (aligned * prob).reshape(B, N * C, H, W)


def tsa_correlation(emb, emb_ref, frame_major=False):
    """The argument of the sigmoid above, (B, N, H, W)."""
    if frame_major:
        emb = emb.transpose(0, 1)
    return (emb * emb_ref.unsqueeze(1)).sum(2)


def tsa_output(fea, att, att_add):
    return fea * torch.sigmoid(att) * 2 + att_add


# ------------------------------------------------------------------------------------------ losses
def _reduce(t, reduction):
    assert reduction in ('mean', 'sum')
    return t.mean() if reduction == 'mean' else t.sum()


def charbonnier(x, y, eps=1e-6, reduction='mean'):
    d = x - y
    return _reduce(torch.sqrt(d * d + eps), reduction)


def l1(x, y, reduction='mean'):
    return _reduce((x - y).abs(), reduction)


def l2(x, y, reduction='mean'):
    return _reduce((x - y) ** 2, reduction)


def huber(x, y, delta=1e-2, reduction='mean'):
    """0.5 q^2 + delta (|d| - q), q = min(|d|, delta)."""
    a = (x - y).abs()
    q = torch.minimum(a, torch.full_like(a, delta))
    return _reduce(0.5 * q ** 2 + delta * (a - q), reduction)


def gw_loss(x1, x2, w=4, reduction='mean'):
    """(1 + w |Sx x1 - Sx x2|) (1 + w |Sy x1 - Sy x2|) |x1 - x2|, Sx / Sy the depthwise 3 x 3 Sobel filters with zero padding 1."""
    dx = (sobel_x(x1) - sobel_x(x2)).abs()
    dy = (sobel_y(x1) - sobel_y(x2)).abs()
    return _reduce((1 + w * dx) * (1 + w * dy) * (x1 - x2).abs(), reduction)


def _depthwise3(t, k):
    C = t.shape[1]
    return F.conv2d(t, torch.tensor(k, dtype=t.dtype).expand(C, 1, 3, 3), padding=1, groups=C)


def sobel_x(t):
    return _depthwise3(t, [[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]])


def sobel_y(t):
    return _depthwise3(t, [[-1., -2., -1.], [0., 0., 0.], [1., 2., 1.]])


def ssim_loss(x, y):
    """oracle/ssim_oracle.py at the dtype of x: its window is built in float64 and rounded to float32 first, as the kernel's is."""
    return ssim_oracle.ssim_loss(x, y)


PIXEL_LOSSES = {'cb': charbonnier, 'l1': l1, 'l2': l2, 'hb': huber}


def pyramid_loss(x, y, num_levels, pyr_mode, loss_mode, reduction='mean'):
    """PyramidLoss (loss.py:160-192): the pixel loss summed over the levels of a 'gau' or 'lap' pyramid."""
    px, py = PYRAMIDS[pyr_mode](x, num_levels), PYRAMIDS[pyr_mode](y, num_levels)
    return sum(PIXEL_LOSSES[loss_mode](a, b, reduction=reduction) for a, b in zip(px, py))


def lap_pyr_loss_cb(x, y, num_levels, reduction='mean'):
    """LapPyrLoss(num_levels, 'cb', 'cb') (loss.py:195-224): Charbonnier on every level of laplacian_pyramid."""
    px, py = laplacian_pyramid(x, num_levels), laplacian_pyramid(y, num_levels)
    return sum(charbonnier(a, b, reduction=reduction) for a, b in zip(px, py))


# ------------------------------------------------------------------------------------------ optimizer / augmentation
def adam_step(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay):
    """Step t (1-based) of torch.optim.Adam (amsgrad=False, maximize=False) in the operation order of its single-tensor loop; returns the
    new (p, m, v)."""
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    denom = v.sqrt() / bc2 ** 0.5 + eps
    return p - (lr / bc1) * (m / denom), m, v


def augment_clips(im1, im2, perm=(0, 1, 2), box_mode=0, box=(0, 0, 0, 0)):
    """Channel permutation of both clips [..., 3, H, W]; box_mode 1: the second output is im2 with the box (y0, y1, x0, x1) taken from
    im1; box_mode 2: im1 with the box taken from im2."""
    a, b = im1[..., list(perm), :, :], im2[..., list(perm), :, :]
    y0, y1, x0, x1 = box
    o2 = b.clone()
    if box_mode == 1:
        o2[..., y0:y1, x0:x1] = a[..., y0:y1, x0:x1]
    elif box_mode == 2:
        o2 = a.clone()
        o2[..., y0:y1, x0:x1] = b[..., y0:y1, x0:x1]
    return a.clone(), o2
