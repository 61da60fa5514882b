"""PReLU with the fused second addend and dropout mask (RF.prelu, csrc/conv3d_kernels.hip) against float64 formulae: forward, backward with
and without the skip gradient, the slope gradient and its run-to-run identity, on and off the 16-byte path.  No matrix cores are
involved: the exact-f32 tolerance of test_gpu_conv.py holds in every GEMM mode.  -m gpu"""
import pytest
import torch
import torch.nn as nn

from gpu_util import check, dev
from test_gpu_conv import TOLS, _at_offset

pytestmark = pytest.mark.gpu
TOL = TOLS['f32']
P = 0.3

SHAPES = [(3, 2, 16, 8, 16),    # 12288 elements: the 16-byte path, three workgroups
          (5, 1, 3, 13, 22),    # 4290 elements, n % 4 == 2: the scalar path, two workgroups
          (1, 1, 1, 3, 5)]      # fewer elements than a workgroup has threads


def _inputs(shape, slope, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    keep = torch.rand(shape, generator=g) >= P
    gout, gres = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    act = nn.PReLU()
    with torch.no_grad():
        act.weight.fill_(slope)
    return a, b, keep, gout, gres, act


def _ref(a, b, keep, slope, scale):
    x = a if b is None else a + b
    y = torch.where(x > 0, x, slope * x)
    return x, (y if keep is None else y * keep.double() * scale)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('slope', [0.25, -1.43])
@pytest.mark.parametrize('use_b, use_keep', [(False, False), (True, False), (False, True), (True, True)])
def test_prelu_forward_backward(shape, slope, use_b, use_keep, offsets=(0, 0, 0)):
    """offsets: float offsets of a, b and the output gradient from a 16-byte boundary."""
    from realvsr_amd import functional as RF
    a, b, keep, gout, _, act = _inputs(shape, slope)
    b, keep = (b if use_b else None), (keep if use_keep else None)
    scale = float(torch.tensor(1.0 / (1.0 - P), dtype=torch.float32)) if use_keep else 1.0
    ar = a.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if use_b else None
    sr = act.weight.detach().double().requires_grad_(True)
    xr, yr = _ref(ar, br, keep, sr, scale)
    gout = gout * (xr.detach().abs() > 1e-3).float()   # the kink rule of test_gpu_conv.py
    yr.backward(gout.double())

    d = dev()
    act = act.to(d)
    ad, bd = _at_offset(a, offsets[0], d), _at_offset(b, offsets[1], d)
    y = RF.prelu(ad, act, b=bd, keep=None if keep is None else keep.to(d), p=P if use_keep else 0.0)
    y.backward(_at_offset(gout, offsets[2], d, leaf=False))
    torch.cuda.synchronize()
    check('y', y, yr, TOL)
    check('grad_a', ad.grad, ar.grad, TOL)
    if use_b:
        check('grad_b', bd.grad, br.grad, TOL)
    check('grad_slope', act.weight.grad, sr.grad, TOL)
    if use_keep:   # dropped elements are exactly zero, kept ones exactly the scaled activation
        assert (y.detach().cpu()[~keep] == 0).all() and (ad.grad.cpu()[~keep] == 0).all()


@pytest.mark.parametrize('offsets', [(1, 0, 0), (0, 1, 0), (0, 0, 1)], ids=lambda o: 'off%d%d%d' % o)
def test_prelu_off_a_16_byte_boundary(offsets):
    test_prelu_forward_backward(SHAPES[0], 0.25, True, True, offsets)


@pytest.mark.parametrize('shape', SHAPES[:2], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('use_keep', [False, True])
def test_prelu_backward_with_skip_gradient(shape, use_keep):
    """gx = g * [keep * scale] * prelu'(x) + gres, the form an FRB's backward uses; gres may be the output buffer."""
    from realvsr_amd import functional as RF
    a, b, keep, gout, gres, act = _inputs(shape, -0.4, seed=5)
    keep = keep if use_keep else None
    scale = 1.0 / (1.0 - P) if use_keep else 1.0
    x = a.double() + b.double()
    gout = gout * (x.abs() > 1e-3).float()
    gg = gout.double() * (keep.double() * scale if use_keep else 1.0)
    want = gg * torch.where(x > 0, 1.0, -0.4) + gres.double()
    want_slope = (gg * x * (x <= 0)).sum().reshape(1)
    d = dev()
    slope = act.weight.detach().to(d)
    gslope = torch.full((1,), 7.0, device=d)   # written, not accumulated
    kd = None if keep is None else keep.to(d)
    gx = RF._prelu_backward(gout.to(d), a.to(d), b.to(d), slope, kd, scale, gres=gres.to(d), gslope=gslope)
    check('gx', gx, want, TOL)
    check('gslope', gslope, want_slope, TOL)
    assert RF._prelu_backward(gout.to(d), a.to(d), b.to(d), slope, kd, scale, gres=gres.to(d), gslope=gslope, need_gx=False) is None
    check('gslope alone', gslope, want_slope, TOL)


def test_slope_gradient_is_bit_identical_over_repeats():
    from realvsr_amd import functional as RF
    a, b, keep, gout, gres, act = _inputs((5, 2, 32, 20, 36), 0.25)   # 230400 elements: 57 partial sums
    d = dev()
    a, b, keep, gout, gres, slope = a.to(d), b.to(d), keep.to(d), gout.to(d), gres.to(d), act.weight.detach().to(d)
    got = []
    for _ in range(5):
        gslope = torch.zeros(1, device=d)
        gx = RF._prelu_backward(gout, a, b, slope, keep, 1.0 / (1.0 - P), gres=gres, gslope=gslope)
        got.append((gx, gslope))
    assert got[0][1].item() != 0
    for gx, gslope in got[1:]:
        assert torch.equal(gx, got[0][0]) and torch.equal(gslope, got[0][1])
