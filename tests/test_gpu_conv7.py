"""7x7 / stride-1 convolutions (SpyNet's blocks) through RF.conv2d against F.conv2d in float64 on the CPU: forward, data gradient,
weight and bias gradient, in both GEMM modes -- the exact-f32 kernels serve 7x7 in every mode, so both are held to the bound
tests/test_gpu_conv.py applies to its exact-f32 cases (TOLS['f32'] = 2e-5, test_gpu_conv.py:11).  -m gpu

Channel pairs: SpyNet's six layers (6 / 8 -> 32 -> 64 -> 32 -> 16 -> 2) and 64 -> 136 for the 128-row m-block.  Frames: 2 x 3 (smaller than
the kernel and than one tile), 5 x 9 (odd, W % 4 != 0), 8 x 32 (exactly one tile), 9 x 33 (one pixel into a second tile each way), 16 x 24."""
import zlib

import pytest
import torch
import torch.nn as nn

from gpu_util import check, dev, gemm_modes
from test_gpu_conv import TOLS, _ref

pytestmark = pytest.mark.gpu
TOL = TOLS['f32']
gemm_mode = gemm_modes()

PAIRS = [(6, 32), (8, 32), (32, 64), (64, 32), (32, 16), (16, 2), (64, 136)]
FRAMES = [(2, 3), (5, 9), (8, 32), (9, 33), (16, 24)]
# (C, Co, act, residual, B, H, W): every pair on every frame, B 1 and 2 alternating; one BN-free ReLU + residual epilogue
CASES = [(ci, co, 'none', False, 1 + (i + j) % 2, h, w) for i, (ci, co) in enumerate(PAIRS) for j, (h, w) in enumerate(FRAMES)]
CASES.append((32, 64, 'relu', True, 2, 9, 33))


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_conv7_forward_backward(case, gemm_mode):
    from realvsr_amd import functional as RF
    C, Co, act, use_res, B, H, W = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()) % 2 ** 31)
    conv = nn.Conv2d(C, Co, 7, 1, 3)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (7.0 * C ** 0.5))
        conv.bias.copy_(torch.randn(Co, generator=g) * 0.1)
    x = torch.randn(B, C, H, W, generator=g)
    res = torch.randn(B, Co, H, W, generator=g) if use_res else None
    gout = torch.randn(B, Co, H, W, generator=g)
    if act != 'none':   # keep the comparison away from the activation kink, as test_gpu_conv.py does
        with torch.no_grad():
            z = _ref(x.double(), None, conv.weight.double(), conv.bias.double(), None, 1, 'none', False)
            gout = gout * (z.abs() > 1e-3).float()

    xr = x.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if use_res else None
    wr, br = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    yr = _ref(xr, None, wr, br, rr, 1, act, False)
    yr.backward(gout.double())

    d = dev()
    conv = conv.to(d)
    xd = x.to(d).requires_grad_(True)
    rd = res.to(d).requires_grad_(True) if use_res else None
    y = RF.conv2d(xd, conv, {'none': RF.ACT_NONE, 'relu': RF.ACT_RELU}[act], 0.1, residual=rd)
    y.backward(gout.to(d))
    torch.cuda.synchronize()
    check('out', y, yr, TOL)
    check('grad_x', xd.grad, xr.grad, TOL)
    if use_res:
        check('grad_res', rd.grad, rr.grad, TOL)
    check('grad_weight', conv.weight.grad, wr.grad, TOL)
    check('grad_bias', conv.bias.grad, br.grad, TOL)


def test_conv7_gradients_are_deterministic(gemm_mode):
    from realvsr_amd import functional as RF
    d = dev()
    torch.manual_seed(0)
    conv = nn.Conv2d(32, 64, 7, 1, 3).to(d)
    x = torch.randn(2, 32, 24, 40, device=d).requires_grad_(True)
    grads = []
    for _ in range(2):
        conv.zero_grad()
        x.grad = None
        RF.conv2d(x, conv).square().sum().backward()
        grads.append((conv.weight.grad.clone(), conv.bias.grad.clone(), x.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*grads))
