"""SpyNet's resampling operators (csrc/flow_kernels.hip) against the float64 restatements of tests/flow_reference.py: the flow warp in
its four modes with both gradients, the 2 x 2 average pool, the x2 align_corners=True upsample.  Frames down to 1 x 1, one-row and
one-column frames, odd sizes, more than one workgroup; flows of zero, integer shifts, random sub-pixel and far outside the frame.  -m gpu

Assertions as in tests/test_gpu_glue_edges.py: bit for bit where float32 is exact (a zero or integer flow: weights 1 and 0; the pool on
integers), TOL = 1e-5 (its bound for the resampling kernels, maximum and L2 through gpu_util.check) elsewhere."""
import pytest
import torch

import flow_reference as G
from gpu_util import check, dev
from test_gpu_glue_edges import TOL, _exact, _gen, _same

pytestmark = pytest.mark.gpu


def _rf():
    from realvsr_amd import functional as RF
    return RF


def _warp_once(x, flow, gout, interp, padding, x_grad=True, flow_grad=True):
    d = dev()
    xd, fd = x.to(d).requires_grad_(x_grad), flow.to(d).requires_grad_(flow_grad)
    out = _rf().flow_warp(xd, fd, interp, padding)
    out.backward(gout.to(d))
    return out.detach(), xd.grad, fd.grad


@pytest.mark.parametrize('kind', ['zero', 'shift', 'random', 'far'])
@pytest.mark.parametrize('interp,padding', G.WARP_MODES, ids=['-'.join(m) for m in G.WARP_MODES])
def test_flow_warp(interp, padding, kind):
    for shape in G.WARP_SHAPES:
        B, C, H, W = shape
        gen = _gen('warp', shape, kind)
        x, gout = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
        flow = G.make_flow(kind, B, H, W, gen)
        name = 'warp %s %s %s %s' % (interp, padding, kind, 'x'.join(map(str, shape)))
        ref = G.warp(x, flow, interp, padding)
        gx_ref, gflow_ref = G.warp_backward(x, flow, gout, interp, padding)
        out, gx, gflow = _warp_once(x, flow, gout, interp, padding)
        if kind == 'zero':
            assert torch.equal(out.cpu(), x), name
        if kind in ('zero', 'shift') or interp == 'nearest':   # every weight is 1 or 0
            _same(name + ' out', out, ref)
        check(name + ' out', out, ref, TOL)
        check(name + ' gx', gx, gx_ref, TOL)          # float atomics: order-dependent in the last bits
        check(name + ' gflow', gflow, gflow_ref, TOL)
        if interp == 'nearest' or (kind == 'far' and padding == 'border'):
            assert not gflow.any(), name
        if kind == 'zero' and padding == 'border':   # a coordinate on the frame's edge counts as clipped, as grid_sample's does
            assert not gflow[:, :, 0, 0].any() and not gflow[:, :, -1, 0].any() and not gflow[:, 0, :, 1].any() and not gflow[:, -1, :, 1].any(), name
        if kind == 'far' and padding == 'zeros' and (H > 1 or W > 1):   # (a 1 x 1 frame samples coordinate 0 whatever the flow)
            assert not out.any() and not gx.any() and not gflow.any(), name
        # the flow gradient is a gather: the same bits from run to run, and with the image gradient skipped
        again = _warp_once(x, flow, gout, interp, padding)
        assert torch.equal(again[2], gflow), name
        alone = _warp_once(x, flow, gout, interp, padding, x_grad=False)
        assert alone[1] is None and torch.equal(alone[2], gflow), name
        only_x = _warp_once(x, flow, gout, interp, padding, flow_grad=False)
        assert only_x[2] is None
        check(name + ' gx alone', only_x[1], gx_ref, TOL)


def test_flow_warp_flow_gradient_on_one_pixel_axes():
    gen = _gen('warp one-pixel axes')
    for shape in ((1, 2, 1, 5), (2, 3, 5, 1), (1, 1, 1, 1)):
        B, C, H, W = shape
        x, gout = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
        out, _, gflow = _warp_once(x, G.make_flow('random', B, H, W, gen), gout, 'bilinear', 'zeros')
        if W == 1:
            assert not gflow[..., 0].any()
        if H == 1:
            assert not gflow[..., 1].any()
        if H == 1 and W == 1:
            assert torch.equal(out.cpu(), x)   # coordinate 0 whatever the flow


def test_flow_warp_non_finite_flow_stays_inside_the_frame():
    """Infinite and NaN displacements: zeros padding samples nothing, and nothing is written outside the gradient buffers."""
    d = dev()
    x = torch.randn(1, 2, 6, 8, device=d).requires_grad_(True)
    flow = torch.zeros(1, 6, 8, 2)
    flow[0, 1, 2, 0], flow[0, 2, 3, 1], flow[0, 3, 4, 0], flow[0, 4, 5, 1] = float('inf'), float('-inf'), float('nan'), 3e38
    out = _rf().flow_warp(x, flow.to(d), 'bilinear', 'zeros')
    out.backward(torch.ones_like(out))
    hit = torch.zeros(6, 8, dtype=torch.bool)
    hit[1, 2] = hit[2, 3] = hit[3, 4] = hit[4, 5] = True
    o, xc = out.detach().cpu()[0], x.detach().cpu()[0]
    assert not o[:, hit].any() and torch.equal(o[:, ~hit], xc[:, ~hit])
    assert torch.equal(x.grad.cpu()[0, 0], (~hit).float())


@pytest.mark.parametrize('shape', G.POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_avg_pool2_exact(shape):
    """Integers: four-term sums and the quarter are exact in float32.  Odd sizes floor; a one-pixel frame pools to an empty tensor."""
    RF = _rf()
    _exact('avg_pool2', RF.avg_pool2, G.avg_pool2, [shape], lambda s: s[:2] + (s[2] // 2, s[3] // 2), 31)
    x = torch.randn(shape).to(dev()).requires_grad_(True)
    y = RF.avg_pool2(x)
    assert tuple(y.shape) == shape[:2] + (shape[2] // 2, shape[3] // 2)
    y.sum().backward()
    want = torch.zeros(shape)
    want[..., :shape[2] // 2 * 2, :shape[3] // 2 * 2] = 0.25
    assert torch.equal(x.grad.cpu(), want)


@pytest.mark.parametrize('scale', [1.0, 2.0])
@pytest.mark.parametrize('shape', G.POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_upsample2_ac(shape, scale):
    RF = _rf()
    d = dev()
    gen = _gen('upsample2_ac', shape, scale)
    x = torch.randn(shape, generator=gen)
    gout = torch.randn(shape[:2] + (2 * shape[2], 2 * shape[3]), generator=gen)
    xd = x.to(d).requires_grad_(True)
    y = RF.upsample2_ac(xd, scale)
    y.backward(gout.to(d))
    name = 'upsample2_ac %s' % 'x'.join(map(str, shape))
    check(name + ' out', y, G.upsample2_ac(x, scale), TOL)
    check(name + ' grad', xd.grad, G.upsample2_ac_backward(x, gout, scale), TOL)
    first = xd.grad.clone()
    xd.grad = None
    RF.upsample2_ac(xd, scale).backward(gout.to(d))
    assert torch.equal(xd.grad, first)          # a gather in a fixed order
    # the corners are the input's corners (align_corners=True)
    assert torch.allclose(y[..., 0, 0], scale * xd.detach()[..., 0, 0], rtol=1e-6, atol=0)
    if min(shape[-2:]) > 1:
        assert torch.allclose(y[..., -1, -1], scale * xd.detach()[..., -1, -1], rtol=1e-5, atol=1e-6)
