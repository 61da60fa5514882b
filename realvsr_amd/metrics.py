"""PSNR / SSIM of the reference's validation and test loops, computed on the GPU (csrc/metric_kernels.hip).

The definition is codes/train.py:288-305 with codes/utils/util.py:283-334:

  tensor2img(float32)            clamp to [0, 1]                                   utils/util.py:157
  (x * 255.0).round().astype(np.uint8)                                             train.py:301-302
  calculate_psnr                 20 log10(255 / sqrt(mean((a - b)^2))) in float64  utils/util.py:283-290
  calculate_ssim / ssim          11 x 11 Gaussian window (sigma 1.5), 'valid', f64 utils/util.py:293-334
  crop_border                    drop c pixels on every side first                 test_RealVSR_wi_GT.py:139

codes/test_RealVSR_wi_GT.py:136 is NOT reproduced: its YCbCr branch divides an image that is already in [0, 1] by 255 before the
`(x * 255.0).round()` of :140, so the script scores a 0/1 image.  

The images stay on the device: the kernels read the f32 planes in place (channel 0 of a [B, C, H, W] tensor through its batch stride),
and one device-to-host copy per call brings back 8 bytes per plane and metric.  The PSNR is exact -- the device returns the integer sum
of squared differences, the host finishes in float64 as the reference does -- and equals the reference's value with `==`; the SSIM
agrees with the reference's float64 evaluation to summation order (below 1e-9 by construction, ~1e-13 in practice).  NaN quantises
to 0 (numpy leaves NaN -> uint8 undefined).
"""
import math

import torch

from . import _lib
from .functional import _need_cuda, _p, _stream, _workspace


def psnr_from_sse(sse, n):
    """The host half of calculate_psnr (utils/util.py:287-290): `sse` the integer sum of squared differences of n pixels."""
    if sse == 0:
        return float('inf')
    mse = int(sse) / int(n)
    return 20 * math.log10(255.0 / math.sqrt(mse))


def center_border_average(values, border_frame):
    """The clip averages of codes/test_RealVSR_wi_GT.py:154-168: frames border_frame <= i < len - border_frame are centre frames, the
    rest border frames; returns {'avg', 'center', 'border'}.  An empty border set averages to 0 as in the script; so does an empty centre
    set, where the script divides by zero (a clip shorter than its window)."""
    n = len(values)
    center = [v for i, v in enumerate(values) if border_frame <= i < n - border_frame]
    border = [v for i, v in enumerate(values) if not border_frame <= i < n - border_frame]
    sum_c, sum_b = sum(center, 0.0), sum(border, 0.0)   # (accumulated separately, like the script's two running sums)
    return {'avg': (sum_c + sum_b) / n if n else 0,
            'center': sum_c / len(center) if center else 0,
            'border': sum_b / len(border) if border else 0}


def quantize_u8(x):
    """uint8(rint(clamp(x, 0, 1) * 255)) in float32, round-half-even: numpy's (np.clip(x, 0, 1) * 255.0).round().astype(np.uint8)."""
    _need_cuda(x)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().rvsr_quantize_u8(_p(x), _p(out), x.numel(), _stream()), 'quantize_u8')
    return out


def _planes(t, what):
    """A [P, H, W] view whose planes have contiguous rows -> (tensor kept alive, P, H, W, plane stride in elements)."""
    if t.dim() != 3:
        raise RuntimeError('%s: expected planes [P, H, W], got %s' % (what, tuple(t.shape)))
    P, H, W = t.shape
    if t.stride(2) != 1 or t.stride(1) != W or (P > 1 and t.stride(0) < H * W):
        t = t.contiguous()
    return t, P, H, W, (t.stride(0) if P > 1 else H * W)


def _score(a, b, crop_border, psnr, ssim, what):
    """PSNR and / or SSIM of the planes a, b ([P, H, W] views): ({'psnr': [...], 'ssim': [...]}), one device-to-host copy."""
    _need_cuda(a, b)
    if a.shape != b.shape:
        raise ValueError('Input images must have the same dimensions.')   # utils/util.py:321-322
    a, P, H, W, sa = _planes(a, what)
    b, _, _, _, sb = _planes(b, what)
    crop = int(crop_border)
    L = _lib.lib()
    nbytes = L.rvsr_metric_workspace_bytes(P, H, W, crop)
    ws = _workspace(nbytes, a.device)
    out = torch.empty(2, P, dtype=torch.int64, device=a.device)   # row 0: integer SSE, row 1: the bits of the double SSIM sums
    if psnr:
        _lib.check(L.rvsr_psnr_sse(_p(a), sa, _p(b), sb, P, H, W, crop, _p(out[0]), _p(ws), ws.numel(), _stream()), what + ' (psnr)')
    if ssim:
        _lib.check(L.rvsr_ssim_sum(_p(a), sa, _p(b), sb, P, H, W, crop, _p(out[1]), _p(ws), ws.numel(), _stream()), what + ' (ssim)')
    host = out.cpu()
    Hc, Wc = H - 2 * crop, W - 2 * crop
    res = {}
    if psnr:
        res['psnr'] = [psnr_from_sse(s, Hc * Wc) for s in host[0].tolist()]
    if ssim:
        res['ssim'] = [s / ((Hc - 10) * (Wc - 10)) for s in host[1].view(torch.float64).tolist()]
    return res


def _channel0(t, what):
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise RuntimeError('%s: expected [C, H, W] or [B, C, H, W], got %s' % (what, tuple(t.shape)))
    return t[:, 0]


def frame_metrics(fake, real, crop_border=0, ssim=True):
    """Channel 0 (Y) of `fake` against `real`, [C, H, W] or [B, C, H, W] f32 GPU tensors in [0, 1] -- what train.py:288-305 and
    test_RealVSR_wi_GT.py:139-143 compute per frame.  Returns {'psnr': [per sample], 'ssim': [per sample]} ('ssim' only when asked)."""
    return _score(_channel0(fake, 'frame_metrics'), _channel0(real, 'frame_metrics'), crop_border, True, ssim, 'frame_metrics')


def psnr_y(fake, real, crop_border=0):
    return _score(_channel0(fake, 'psnr_y'), _channel0(real, 'psnr_y'), crop_border, True, False, 'psnr_y')['psnr']


def ssim_y(fake, real, crop_border=0):
    return _score(_channel0(fake, 'ssim_y'), _channel0(real, 'ssim_y'), crop_border, False, True, 'ssim_y')['ssim']


def _image(t, what):
    if t.dim() == 2:
        return t.unsqueeze(0)
    if t.dim() == 3:
        return t
    raise ValueError('Wrong input image dimensions.')   # utils/util.py:333-334


def calculate_psnr(img1, img2):
    """util.calculate_psnr for an [H, W] or [C, H, W] f32 GPU image in [0, 1] (quantised here): one value over all its pixels."""
    a, b = _image(img1, 'calculate_psnr'), _image(img2, 'calculate_psnr')
    _need_cuda(a, b)
    if a.shape != b.shape:
        raise ValueError('Input images must have the same dimensions.')
    C, H, W = a.shape
    return _score(a.reshape(1, C * H, W), b.reshape(1, C * H, W), 0, True, False, 'calculate_psnr')['psnr'][0]


def calculate_ssim(img1, img2):
    """util.calculate_ssim for an [H, W] or [C, H, W] f32 GPU image in [0, 1]: for several channels the mean of the per-plane values
    (what utils/util.py:326-330 evaluates for an H x W x 3 array)."""
    vals = _score(_image(img1, 'calculate_ssim'), _image(img2, 'calculate_ssim'), 0, False, True, 'calculate_ssim')['ssim']
    return vals[0] if len(vals) == 1 else sum(vals) / len(vals)
