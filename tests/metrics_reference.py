"""The validation metrics restated directly in numpy float64, for shapes tests/golden/metrics.npz does not hold: the quantisation of
codes/train.py:301-302 behind tensor2img's clamp, calculate_psnr and ssim of codes/utils/util.py:283-334, crop_border.  The SSIM
window is applied as written there -- the full 11 x 11 outer product, 121 taps per pixel, no separability -- so that the device's
separable evaluation is checked against a different summation.  test_metrics_host.py pins this file to the fixture the reference's
own functions recorded."""
import math

import numpy as np


def quantize(x):
    """float32 array -> uint8, the reference's chain: clamp (utils/util.py:157), (x * 255.0).round().astype(np.uint8) (train.py:301)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    return (np.clip(x, 0, 1) * 255.0).round().astype(np.uint8)


def gaussian_kernel():
    """cv2.getGaussianKernel(11, 1.5) by its documented formula, in double."""
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5) ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def crop(img, c):
    return img[c:img.shape[0] - c, c:img.shape[1] - c] if c else img


def psnr_u8(a, b):
    """calculate_psnr (utils/util.py:283-290) on uint8 arrays."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    mse = np.mean((a - b) ** 2)
    if mse == 0:
        return float('inf')
    return 20 * math.log10(255.0 / math.sqrt(mse))


def _valid(img, window):
    """The 'valid' part of cv2.filter2D(img, -1, window): correlation, every tap of the 11 x 11 window added in turn."""
    H, W = img.shape
    out = np.zeros((H - 10, W - 10), np.float64)
    for i in range(11):
        for j in range(11):
            out += window[i, j] * img[i:i + H - 10, j:j + W - 10]
    return out


def ssim_u8(a, b):
    """ssim (utils/util.py:293-313) on two-dimensional uint8 arrays."""
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a, b = a.astype(np.float64), b.astype(np.float64)
    k = gaussian_kernel()
    window = np.outer(k, k)
    mu1, mu2 = _valid(a, window), _valid(b, window)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = _valid(a ** 2, window) - mu1_sq
    sigma2_sq = _valid(b ** 2, window) - mu2_sq
    sigma12 = _valid(a * b, window) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return float(ssim_map.mean())


def psnr_plane(a, b, crop_border=0):
    """PSNR of two float32 planes in [0, 1] as the validation loop scores them."""
    return psnr_u8(crop(quantize(a), crop_border), crop(quantize(b), crop_border))


def ssim_plane(a, b, crop_border=0):
    return ssim_u8(crop(quantize(a), crop_border), crop(quantize(b), crop_border))


def ssim_image(a, b):
    """calculate_ssim (utils/util.py:316-334) for [C, H, W] float32 images: the mean of the per-plane values."""
    return float(np.mean([ssim_plane(a[c], b[c]) for c in range(a.shape[0])]))
