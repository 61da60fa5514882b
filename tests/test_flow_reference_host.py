"""tests/flow_reference.py against torch's own operators on the CPU, in float64 with autograd for the gradients: F.grid_sample
(align_corners=True) behind the reference's normalisation (codes/models/archs/arch_util.py:47-80), F.avg_pool2d, F.interpolate.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import flow_reference as G

TOL = 1e-12


def _close(name, got, ref):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    assert err <= TOL * max(1.0, ref.abs().max().item() if ref.numel() else 1.0), (name, err)


def _torch_warp(x, flow, interp, padding):
    """arch_util.flow_warp, restated on float64 tensors."""
    B, C, H, W = x.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    vx = 2.0 * (xs + flow[..., 0]) / max(W - 1, 1) - 1.0
    vy = 2.0 * (ys + flow[..., 1]) / max(H - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((vx, vy), dim=3), mode=interp, padding_mode=padding, align_corners=True)


@pytest.mark.parametrize('kind', ['zero', 'shift', 'random', 'far'])
@pytest.mark.parametrize('interp,padding', G.WARP_MODES, ids=['-'.join(m) for m in G.WARP_MODES])
def test_warp_restatement(interp, padding, kind):
    gen = torch.Generator().manual_seed(3)
    for B, C, H, W in G.WARP_SHAPES:
        x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
        flow = G.make_flow(kind, B, H, W, gen).double()
        gout = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
        xr, fr = x.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        ref = _torch_warp(xr, fr, interp, padding)
        ref.backward(gout)
        name = '%s %s %s %s' % (interp, padding, kind, (B, C, H, W))
        _close(name + ' out', G.warp(x, flow, interp, padding), ref.detach())
        gx, gflow = G.warp_backward(x, flow, gout, interp, padding)
        _close(name + ' gx', gx, xr.grad)
        if kind == 'random' or interp == 'nearest':   # (at an integer coordinate the derivative is one-sided: which side is the operator's choice)
            _close(name + ' gflow', gflow, fr.grad)
        if kind == 'zero':
            assert torch.equal(G.warp(x, flow, interp, padding), x)
        if interp == 'nearest':
            assert not gflow.any()


@pytest.mark.parametrize('kind', ['zero', 'shift'])
@pytest.mark.parametrize('interp,padding', G.WARP_MODES, ids=['-'.join(m) for m in G.WARP_MODES])
def test_flow_gradient_at_integer_coordinates(interp, padding, kind):
    """Zero and integer flows on frames whose H - 1 and W - 1 are powers of two: the normalise / un-normalise round trip of an integer
    coordinate is exact in float64, so torch samples exactly on the pixels, edges included, and its one-sided flow gradient there -- zero
    on and beyond the edges under border -- is the restatement's."""
    gen = torch.Generator().manual_seed(6)
    for B, C, H, W in ((2, 3, 5, 9), (1, 2, 3, 17), (2, 2, 9, 5), (1, 3, 2, 2)):
        x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
        gout = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
        flow = G.make_flow(kind, B, H, W, gen).double()
        xr, fr = x.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        ref = _torch_warp(xr, fr, interp, padding)
        ref.backward(gout)
        name = '%s %s %s %s' % (interp, padding, kind, (B, C, H, W))
        gx, gflow = G.warp_backward(x, flow, gout, interp, padding)
        _close(name + ' out', G.warp(x, flow, interp, padding), ref.detach())
        _close(name + ' gx', gx, xr.grad)
        _close(name + ' gflow', gflow, fr.grad)
        if padding == 'border' and kind == 'zero':     # every pixel of the frame's rim has a clipped axis
            assert not gflow[:, :, 0, 0].any() and not gflow[:, :, -1, 0].any() and not gflow[:, 0, :, 1].any() and not gflow[:, -1, :, 1].any()
            if interp == 'bilinear' and min(H, W) > 2:
                assert gflow[:, 1:-1, 1:-1].any()


def test_flow_gradient_is_zero_where_the_border_clamps_and_on_one_pixel_axes():
    gen = torch.Generator().manual_seed(4)
    x, gout = torch.randn(1, 2, 6, 8, generator=gen), torch.randn(1, 2, 6, 8, generator=gen)
    flow = G.make_flow('far', 1, 6, 8, gen)
    assert not G.warp_backward(x, flow, gout, 'bilinear', 'border')[1].any()
    x, gout = torch.randn(1, 2, 1, 8, generator=gen), torch.randn(1, 2, 1, 8, generator=gen)
    gflow = G.warp_backward(x, G.make_flow('random', 1, 1, 8, gen), gout, 'bilinear', 'zeros')[1]
    assert not gflow[..., 1].any() and gflow[..., 0].any()


def test_pool_and_upsample_restatements():
    gen = torch.Generator().manual_seed(5)
    for shape in G.POOL_SHAPES:
        x = torch.randn(shape, generator=gen, dtype=torch.float64)
        if min(shape[-2:]) >= 2:
            xr = x.clone().requires_grad_(True)
            ref = F.avg_pool2d(xr, 2, 2)
            gout = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
            ref.backward(gout)
            _close('pool %s' % (shape,), G.avg_pool2(x), ref.detach())
            _close('pool backward %s' % (shape,), G.avg_pool2_backward(x, gout), xr.grad)
        else:   # (torch refuses an empty output; the floor rule gives one, and no gradient)
            empty = torch.zeros(shape[0], shape[1], shape[2] // 2, shape[3] // 2, dtype=torch.float64)
            assert G.avg_pool2(x).shape == empty.shape and not G.avg_pool2_backward(x, empty).any()
        xr = x.clone().requires_grad_(True)
        ref = 2.0 * F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=True)
        gout = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
        ref.backward(gout)
        _close('upsample %s' % (shape,), G.upsample2_ac(x, 2.0), ref.detach())
        _close('upsample backward %s' % (shape,), G.upsample2_ac_backward(x, gout, 2.0), xr.grad)
