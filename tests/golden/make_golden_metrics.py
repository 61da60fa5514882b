#!/usr/bin/env python
"""Generate tests/golden/metrics.npz by IMPORTING the reference's utils/util.py (build container only).

Run from the repo root:   python tests/golden/make_golden_metrics.py
Needs /root/reference (read-only); imported the way make_golden.py does (import_reference: the absent third-party modules stubbed).

cv2 ITSELF IS NOT ON THE MACHINE.  util.ssim calls two of its functions, which the stubbed module gets as numpy stand-ins:
  * getGaussianKernel(11, 1.5): OpenCV's documented formula, exp(-(i - 5)^2 / (2 sigma^2)) scaled to sum 1, in float64
    (for this size and sigma OpenCV evaluates the formula; its fixed tables cover ksize <= 7 with sigma <= 0 only);
  * filter2D(src, -1, kernel): float64 correlation anchored at the kernel centre, per channel.  The reference crops [5:-5, 5:-5]
    from the result, so the border mode never reaches a recorded value.
The SSIM values below are therefore pinned to the reference's CODE -- window construction, the five filtered maps, the formula, the
crop, the mean, the channel handling of calculate_ssim -- not to OpenCV's binary.  The quantisation chain and calculate_psnr are the
reference's own code with nothing substituted.

Recorded for three pairs of [3, H, W] float32 images (noise beyond [0, 1], smooth + noise, flat regions):
  a<i>, b<i>        the inputs
  qa<i>, qb<i>      tensor2img(x, out_type=np.float32, reverse_channel=False) then (x * 255.0).round().astype(np.uint8)   (train.py:288-302)
  psnr<i>           calculate_psnr on channel 0 (train.py:305);  psnr3_<i> on the whole H x W x 3 image
  ssim2d_<i>        calculate_ssim on channel 0 as a 2-D array (test_RealVSR_wi_GT.py:143), ssim1_<i> as H x W x 1, ssim3_<i> on H x W x 3
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_golden import OUT, import_reference  # noqa: E402


def get_gaussian_kernel(ksize, sigma):
    i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2
    g = np.exp(-(i ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).reshape(ksize, 1)


def filter2d(src, ddepth, kernel):
    assert ddepth == -1 and src.dtype == np.float64
    kh, kw = kernel.shape
    pad = [(kh // 2, kh // 2), (kw // 2, kw // 2)] + [(0, 0)] * (src.ndim - 2)
    p = np.pad(src, pad, mode='reflect')
    out = np.zeros_like(src)
    for i in range(kh):
        for j in range(kw):
            out += kernel[i, j] * p[i:i + src.shape[0], j:j + src.shape[1]]
    return out


def pairs():
    rng = np.random.RandomState(20)
    a = (rng.rand(3, 16, 20) * 1.2 - 0.1).astype(np.float32)          # noise, some of it beyond [0, 1]
    b = (rng.rand(3, 16, 20) * 1.2 - 0.1).astype(np.float32)
    yield a, b
    y, x = np.mgrid[0:20, 0:17].astype(np.float32)
    s = np.stack([0.5 + 0.4 * np.sin(0.3 * x + 0.2 * y + c) for c in range(3)]).astype(np.float32)   # smooth + noise
    yield s, (s + 0.03 * rng.randn(3, 20, 17)).astype(np.float32)
    f = np.full((3, 24, 22), 0.25, np.float32)                          # flat regions: the variances cancel
    f[:, :, 11:] = 0.75
    g = f.copy()
    g[:, 12:, :] += 0.002                                               # below one quantisation step in places
    g[:, 5:9, 3:8] = rng.rand(3, 4, 5).astype(np.float32)
    yield f, g


def main():
    _, _, util, _ = import_reference()
    cv2 = sys.modules['cv2']
    assert not hasattr(cv2, 'filter2D'), 'a real cv2 is present: record with it instead of the stand-ins'
    cv2.getGaussianKernel, cv2.filter2D = get_gaussian_kernel, filter2d
    rec = {}
    for i, (a, b) in enumerate(pairs()):
        fake = util.tensor2img(torch.from_numpy(a.copy()), out_type=np.float32, reverse_channel=False)
        real = util.tensor2img(torch.from_numpy(b.copy()), out_type=np.float32, reverse_channel=False)
        fake = (fake * 255.0).round().astype(np.uint8)
        real = (real * 255.0).round().astype(np.uint8)
        rec.update({'a%d' % i: a, 'b%d' % i: b, 'qa%d' % i: fake, 'qb%d' % i: real,
                    'psnr%d' % i: np.float64(util.calculate_psnr(fake[:, :, 0], real[:, :, 0])),
                    'psnr3_%d' % i: np.float64(util.calculate_psnr(fake, real)),
                    'ssim2d_%d' % i: np.float64(util.calculate_ssim(fake[:, :, 0], real[:, :, 0])),
                    'ssim1_%d' % i: np.float64(util.calculate_ssim(fake[:, :, 0:1], real[:, :, 0:1])),
                    'ssim3_%d' % i: np.float64(util.calculate_ssim(fake, real))})
        print('pair %d %s: psnr %.6f ssim %.9f ssim3 %.9f' % (i, a.shape, rec['psnr%d' % i], rec['ssim2d_%d' % i], rec['ssim3_%d' % i]))
    np.savez_compressed(os.path.join(OUT, 'metrics.npz'), **rec)
    print('wrote metrics.npz (%d bytes)' % os.path.getsize(os.path.join(OUT, 'metrics.npz')))


if __name__ == '__main__':
    main()
