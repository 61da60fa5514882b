"""The 1x1 and 3x3 / stride-2 conv blocks at small shapes, vs torch CPU float64.  -m gpu

Same comparison, distance from the activation kink and tolerances as test_gpu_conv.test_conv_block_forward_backward (which it calls).
The 1x1 shapes are chosen for the LDS-staged weight gradient (conv_wgrad1x1s): several 64-channel blocks and N tiles, channel counts
off the block, a concat on the block boundary, a ragged last pixel tile, fewer pixel tiles than partial-sum slots; their forward and
data gradient run conv_fwd2 as before.  The stride-2 cases, the shared-gradient-buffer case and the width off the vector path are
regression cover of the kernels that are there today (conv_fwd2, the zero-insert data gradient, conv_wgrad_s2): even and odd sizes, so
that any kernel that later treats the four pixel parities of a stride-2 data gradient separately meets a truncated last row or
column in every class."""
import pytest
import torch
import torch.nn as nn

from gpu_util import check, dev, gemm_modes
from test_gpu_conv import TOLS, test_conv_block_forward_backward as _block

pytestmark = pytest.mark.gpu

CASES = [
    # C1, C2, Co, k, stride, act, residual, pixel_shuffle, B, H, W
    (320, 0, 64, 1, 1, 'lrelu', False, False, 2, 9, 40),     # five chunks / 64-channel blocks; the backward is 64 -> 320: five m-blocks
    (48, 0, 16, 1, 1, 'none', False, False, 3, 8, 36),       # channel counts off the chunk and the block
    (64, 64, 80, 1, 1, 'lrelu', False, False, 2, 10, 36),    # concat on the boundary, two m-blocks of the weight gradient
    (64, 0, 64, 1, 1, 'relu', False, False, 1, 12, 30),      # W % 4 != 0 (H * W % 4 == 0: the weight gradient is still conv_wgrad1x1s)
    (64, 0, 64, 1, 1, 'lrelu', False, False, 1, 8, 8),       # one 64-pixel tile: fewer pixel units than partial-sum slots
    (320, 0, 64, 1, 1, 'lrelu', False, False, 3, 13, 24),    # 312 pixels per image: the last K tile is ragged (56 of 64)
    (64, 0, 64, 3, 2, 'lrelu', False, False, 2, 24, 40),
    (64, 0, 64, 3, 2, 'relu', False, False, 1, 23, 37),
    (16, 0, 24, 3, 2, 'none', False, False, 1, 18, 32),
    (64, 0, 64, 3, 2, 'lrelu', False, False, 1, 9, 68),
]

gemm_mode = gemm_modes()


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_smallk_forward_backward(case, gemm_mode):
    _block(case, gemm_mode)


def test_stride2_data_gradient_accumulates_into_a_held_gradient(gemm_mode):
    """x has two consumers that share a GradSink: a 3x3 / stride-1 conv deposits first, the stride-2 conv owns the sink and adds its data
    gradient into the buffer that already holds the other one.  The sum must be the reference's."""
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    g = torch.Generator().manual_seed(20261018)
    B, C, H, W = 2, 64, 23, 40
    s2, s1 = nn.Conv2d(C, 64, 3, 2, 1), nn.Conv2d(C, 16, 3, 1, 1)
    with torch.no_grad():
        for conv in (s2, s1):
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3.0 * (9 * C) ** 0.5))
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.1)
    x = torch.randn(B, C, H, W, generator=g)
    g2, g1 = torch.randn(B, 64, 12, 20, generator=g), torch.randn(B, 16, H, W, generator=g)

    xr = x.double().requires_grad_(True)
    p2 = [t.detach().double().requires_grad_(True) for t in (s2.weight, s2.bias)]
    p1 = [t.detach().double().requires_grad_(True) for t in (s1.weight, s1.bias)]
    y2r = torch.nn.functional.conv2d(xr, p2[0], p2[1], stride=2, padding=1)
    y1r = torch.nn.functional.conv2d(xr, p1[0], p1[1], stride=1, padding=1)
    torch.autograd.backward([y2r, y1r], [g2.double(), g1.double()])

    d = dev()
    s2, s1 = s2.to(d), s1.to(d)
    xg = x.to(d).requires_grad_(True)
    sink = RF.GradSink()
    y2 = RF.conv2d(xg, s2, RF.ACT_NONE, sink=sink)        # the owner: created first, runs last in backward
    y1 = RF.conv2d(xg, s1, RF.ACT_NONE, dep_sink=sink)    # the depositor
    torch.autograd.backward([y2, y1], [g2.to(d), g1.to(d)])
    torch.cuda.synchronize()
    assert sink.closed
    check('out_s2', y2, y2r, TOL)
    check('grad_x (sum of both consumers)', xg.grad, xr.grad, TOL)
    check('grad_weight_s2', s2.weight.grad, p2[0].grad, TOL)
    check('grad_bias_s2', s2.bias.grad, p2[1].grad, TOL)


@pytest.mark.parametrize('geo', [(320, 64, 1, 1, 2, 13, 24), (64, 64, 3, 2, 2, 23, 40)], ids=['1x1', 'stride2'])
def test_smallk_wgrad_is_deterministic(geo):
    """Two backward passes give bit-identical weight and bias gradients (fixed-order partial sums)."""
    from realvsr_amd import functional as RF
    C, Co, k, stride, B, H, W = geo
    d = dev()
    torch.manual_seed(0)
    conv = nn.Conv2d(C, Co, k, stride, k // 2).to(d)
    x = torch.randn(B, C, H, W, device=d)
    grads = []
    for _ in range(2):
        conv.zero_grad()
        RF.conv2d(x, conv, RF.ACT_LRELU).square().sum().backward()
        grads.append((conv.weight.grad.clone(), conv.bias.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
