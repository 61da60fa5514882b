"""CPU-side checks of the validation metrics: the numpy restatement the GPU tests compare against is pinned to what the reference's
own functions recorded (tests/golden/metrics.npz), the library exports the new entry points, and the host halves of
realvsr_amd.metrics do what the reference's scripts do."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import metrics_reference as MR
from conftest import load_golden

NEW_ENTRIES = ('rvsr_metric_tile', 'rvsr_metric_workspace_bytes', 'rvsr_quantize_u8', 'rvsr_psnr_sse', 'rvsr_ssim_sum')


def test_reference_helper_matches_the_recorded_reference():
    """Quantisation bit for bit, PSNR with ==, SSIM to 1e-12 (the helper adds the 121 taps in another order than the recorded filter)."""
    g = load_golden('metrics')
    for i in range(3):
        a, b = g['a%d' % i], g['b%d' % i]
        assert np.array_equal(MR.quantize(a).transpose(1, 2, 0), g['qa%d' % i])
        assert np.array_equal(MR.quantize(b).transpose(1, 2, 0), g['qb%d' % i])
        assert MR.psnr_plane(a[0], b[0]) == float(g['psnr%d' % i])
        assert MR.psnr_u8(MR.quantize(a), MR.quantize(b)) == float(g['psnr3_%d' % i])
        assert abs(MR.ssim_plane(a[0], b[0]) - float(g['ssim2d_%d' % i])) <= 1e-12
        assert abs(MR.ssim_plane(a[0], b[0]) - float(g['ssim1_%d' % i])) <= 1e-12
        assert abs(MR.ssim_image(a, b) - float(g['ssim3_%d' % i])) <= 1e-12
    assert MR.psnr_plane(g['a0'][0], g['a0'][0]) == float('inf') and MR.ssim_plane(g['a0'][0], g['a0'][0]) == 1.0
    # crop_border: the same as scoring the cropped arrays
    a, b = g['a2'][0], g['b2'][0]
    assert MR.psnr_plane(a, b, 2) == MR.psnr_plane(np.ascontiguousarray(a[2:-2, 2:-2]), np.ascontiguousarray(b[2:-2, 2:-2]))
    assert MR.ssim_plane(a, b, 2) == MR.ssim_plane(np.ascontiguousarray(a[2:-2, 2:-2]), np.ascontiguousarray(b[2:-2, 2:-2]))


def test_library_exports_the_metric_entries():
    from realvsr_amd import _lib
    _lib.build()
    L = _lib.lib()
    S = _lib.SIGNATURES
    for name in NEW_ENTRIES:
        assert name in S and getattr(L, name) is not None
    p, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert S['rvsr_metric_tile'] == (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)])
    assert S['rvsr_metric_workspace_bytes'] == (z, [z, i, i, i])
    assert S['rvsr_quantize_u8'] == (C.c_int, [p, p, z, p])
    assert S['rvsr_psnr_sse'] == (C.c_int, [p, z, p, z, z, i, i, i, p, p, z, p])       # long long* result: a device pointer
    assert S['rvsr_ssim_sum'] == S['rvsr_psnr_sse']                                      # double* result: parses since 'double' may be pointed at
    # host-only entries run without a GPU
    th, tw = C.c_int(0), C.c_int(0)
    assert L.rvsr_metric_tile(C.byref(th), C.byref(tw)) == _lib.RVSR_OK and th.value > 0 and tw.value > 0
    tiles = lambda n, t: (n - 10 + t - 1) // t   # noqa: E731
    assert L.rvsr_metric_workspace_bytes(1, 16, 16, 0) == 1024 * 8
    assert L.rvsr_metric_workspace_bytes(3, 2160, 3840, 4) == 3 * max(1024, tiles(2152, th.value) * tiles(3832, tw.value)) * 8
    assert L.rvsr_metric_workspace_bytes(1, 8, 8, 4) == 0 and L.rvsr_metric_workspace_bytes(0, 8, 8, 0) == 0
    # refusals are decided before anything is launched
    assert L.rvsr_ssim_sum(None, 0, None, 0, 1, 16, 16, 0, None, None, 0, None) == _lib.RVSR_ERR_BAD_ARG
    one = C.c_void_p(8)   # (never dereferenced: the shape is refused first)
    assert L.rvsr_ssim_sum(one, 0, one, 0, 1, 18, 32, 4, one, one, 1 << 20, None) == _lib.RVSR_ERR_BAD_ARG
    assert b'smaller than the 11 x 11 window' in L.rvsr_last_error()
    assert L.rvsr_psnr_sse(one, 0, one, 0, 1, 8, 8, 4, one, one, 1 << 20, None) == _lib.RVSR_ERR_BAD_ARG
    assert L.rvsr_psnr_sse(one, 0, one, 0, 1, 64, 64, 0, one, one, 8, None) == _lib.RVSR_ERR_WORKSPACE


def test_psnr_from_sse():
    from realvsr_amd.metrics import psnr_from_sse
    assert psnr_from_sse(0, 100) == float('inf')
    assert psnr_from_sse(65025 * 50, 50) == 0.0
    assert psnr_from_sse(12345, 320) == 20 * math.log10(255.0 / math.sqrt(12345 / 320))
    g = load_golden('metrics')
    for i in range(3):
        qa, qb = g['qa%d' % i][:, :, 0].astype(np.int64), g['qb%d' % i][:, :, 0].astype(np.int64)
        assert psnr_from_sse(int(((qa - qb) ** 2).sum()), qa.size) == float(g['psnr%d' % i])
    # beyond 2^32, torch integers accepted
    assert psnr_from_sse(torch.tensor(65025 * 2 ** 22), 2 ** 22) == 0.0


def test_center_border_average():
    """codes/test_RealVSR_wi_GT.py:154-168 with border_frame = N // 2, against values worked out by hand."""
    from realvsr_amd.metrics import center_border_average as cba
    assert cba([30.0], 1) == {'avg': 30.0, 'center': 0, 'border': 30.0}                                   # T 1, N 3: no centre frame
    assert cba([30.0], 2) == {'avg': 30.0, 'center': 0, 'border': 30.0}                                   # T 1, N 5
    assert cba([30.0, 32.0, 37.0], 1) == {'avg': 33.0, 'center': 32.0, 'border': 33.5}                    # T 3, N 3
    assert cba([30.0, 32.0, 37.0], 2) == {'avg': 33.0, 'center': 0, 'border': 33.0}                       # T 3, N 5
    v = [10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 71.0]
    assert cba(v, 1) == {'avg': 281.0 / 7, 'center': 40.0, 'border': 40.5}                                # T 7, N 3
    assert cba(v, 2) == {'avg': 281.0 / 7, 'center': 40.0, 'border': 161.0 / 4}                           # T 7, N 5
    assert cba(v, 0) == {'avg': 281.0 / 7, 'center': 281.0 / 7, 'border': 0}                              # no border frame: 0, as the script
    # the script's order of summation: centre sum + border sum, not the running order of the frames
    w = [0.1, 0.7, 0.2, 0.3, 0.9]
    assert cba(w, 1)['avg'] == ((0.7 + 0.2 + 0.3) + (0.1 + 0.9)) / 5


def test_metrics_refuse_cpu_tensors():
    from realvsr_amd import metrics as M
    from realvsr_amd import infer
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    for call in (lambda: M.quantize_u8(a), lambda: M.psnr_y(a, b), lambda: M.ssim_y(a, b), lambda: M.frame_metrics(a, b),
                 lambda: M.calculate_psnr(a[0, 0], b[0, 0]), lambda: M.calculate_ssim(a[0], b[0]),
                 lambda: infer.evaluate_clip(None, a, b)):
        with pytest.raises(NotImplementedError):
            call()
