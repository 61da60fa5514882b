"""The 16-byte paths of csrc/misc_kernels.hip -- upsample2_bwd_v4 (four input pixels per thread; the forward stays on the float2
kernel and runs here at the same shapes), pool_*_v4 (four outputs / inputs per thread) -- and the interior paths of the four pyramid stencils, at the smallest shapes that can break them.  -m gpu

The references and the kinds of assertion are those of test_gpu_glue_edges.py: integer-valued tensors must equal the float64 reference
of glue_reference.py bit for bit, random ones stay under TOL.  On top of that a vector kernel must equal, bit for bit and on random
values, what the kernel it replaces computes: the same call through the C ABI with every tensor 8 bytes off a 16-byte boundary takes
the older kernels (and must write nothing outside its views)."""
import pytest
import torch

import glue_reference as G
from gpu_util import check, dev
from test_gpu_glue_edges import TOL, _close, _exact, _gen, _ints, _rf, _same

pytestmark = pytest.mark.gpu
GUARD = -77.0


def _ids(s):
    return 'x'.join(map(str, s))


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _off8(t, d):
    """(buffer, view): `t` on the device 8 bytes behind a 16-byte boundary, guard values all around."""
    buf = torch.full((t.numel() + 8,), GUARD, device=d, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[2:2 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return buf, v


def _guards_intact(buf, n):
    return bool((buf[:2] == GUARD).all()) and bool((buf[2 + n:] == GUARD).all())


# ------------------------------------------------------------------------------------------ bilinear upsample x2
# W % 4 == 0: upsample2_bwd_v4; (1, 2, 4, 6): W % 4 == 2 stays on the float2 kernel; 1 x 4: one thread, every clamp at once;
# 4 x 1028 x 1024: 1 052 672 threads backward, four times as many forward -- past one trip of the capped grid (4096 x 256)
UP2_SHAPES = [(1, 1, 1, 4), (1, 2, 2, 4), (2, 3, 3, 8), (1, 2, 5, 12), (1, 2, 4, 6), (1, 4, 1028, 1024)]


@pytest.mark.parametrize('scale', [1.0, 2.0])
@pytest.mark.parametrize('shape', UP2_SHAPES, ids=_ids)
def test_upsample_x2_vector_exact(shape, scale):
    RF = _rf()
    _exact('upsample x2 v4', lambda x: RF.upsample_bilinear(x, 2, scale), lambda x: G.upsample_bilinear(x, 2, scale),
           [shape], lambda s: s[:2] + (2 * s[2], 2 * s[3]), 21)


def _upsample_abi(x, gout, scale, off):
    """rvsr_upsample_bilinear_forward / _backward through the C ABI, every tensor aligned (off = False) or 8 bytes off."""
    from realvsr_amd import _lib
    d, L, p = dev(), _lib.lib(), _lib._p
    B, C, H, W = x.shape
    place = (lambda t: _off8(t, d)) if off else (lambda t: (None, t.to(d).contiguous()))
    (_, xd), (_, gd) = place(x), place(gout)
    obuf, out = place(torch.full(gout.shape, GUARD))
    ibuf, gin = place(torch.full(x.shape, GUARD))
    _lib.check(L.rvsr_upsample_bilinear_forward(p(xd), p(out), B * C, H, W, 2, scale, _lib._stream()), 'upsample forward')
    _lib.check(L.rvsr_upsample_bilinear_backward(p(gd), p(gin), B * C, H, W, 2, scale, _lib._stream()), 'upsample backward')
    torch.cuda.synchronize()
    if off:
        assert _guards_intact(obuf, out.numel()) and _guards_intact(ibuf, gin.numel()), 'written outside the view'
    return out, gin


@pytest.mark.parametrize('shape', [(1, 2, 2, 4), (2, 3, 3, 8), (1, 2, 5, 12)], ids=_ids)
def test_upsample_x2_off_the_16_byte_boundary(shape):
    """Input and output 8 bytes off: the float2 kernels take the call, exact on integers, nothing written either side; and on random
    values the aligned call (upsample2_bwd_v4 backward) gives the same bits."""
    gen = _gen('upsample off8', shape)
    oshape = shape[:2] + (2 * shape[2], 2 * shape[3])
    x, gout = _ints(shape, 0, 15, gen), _ints(oshape, -8, 8, gen)
    xr = x.double().requires_grad_(True)
    yr = G.upsample_bilinear(xr, 2, 2.0)
    yr.backward(gout.double())
    out, gin = _upsample_abi(x, gout, 2.0, True)
    _same('x2 forward, 8 bytes off', out, yr)
    _same('x2 backward, 8 bytes off', gin, xr.grad)
    x, gout = torch.randn(shape, generator=gen), torch.randn(oshape, generator=gen)
    o1, g1 = _upsample_abi(x, gout, 2.0, True)
    o0, g0 = _upsample_abi(x, gout, 2.0, False)
    assert torch.equal(_bits(o0), _bits(o1)) and torch.equal(_bits(g0), _bits(g1))


def test_upsample_x2_vector_on_random_values():
    RF = _rf()
    _close('upsample x2 v4', lambda x: RF.upsample_bilinear(x, 2, 2.0), lambda x: G.upsample_bilinear(x, 2, 2.0),
           [(2, 3, 5, 12)], lambda s: s[:2] + (2 * s[2], 2 * s[3]), 22)


# ------------------------------------------------------------------------------------------ max + avg pool
def _pool_abi(x, gout, off):
    from realvsr_amd import _lib
    d, L, p = dev(), _lib.lib(), _lib._p
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    place = (lambda t: _off8(t, d)) if off else (lambda t: (None, t.to(d).contiguous()))
    (_, xd), (_, gd) = place(x), place(gout)
    obuf, out = place(torch.full((B, 2 * C, Ho, Wo), GUARD))
    ibuf, gin = place(torch.full(x.shape, GUARD))
    abuf = torch.full((B * C * Ho * Wo + 16,), 99, dtype=torch.uint8, device=d)
    arg = abuf[1 if off else 0:][:B * C * Ho * Wo].view(B, C, Ho, Wo)      # off: one byte behind the boundary
    _lib.check(L.rvsr_maxavgpool_forward(p(xd), p(out), p(arg), B, C, H, W, _lib._stream()), 'pool forward')
    _lib.check(L.rvsr_maxavgpool_backward(p(gd), p(arg), p(gin), B, C, H, W, _lib._stream()), 'pool backward')
    torch.cuda.synchronize()
    if off:
        assert _guards_intact(obuf, out.numel()) and _guards_intact(ibuf, gin.numel()), 'written outside the view'
    return out, gin, arg


# W % 8 == 0: pool_fwd_v4 and pool_bwd_v4; W = 4, 12: the backward alone is vectorised; H = 2, 3, 7, 8: the last window row is whole,
# cut, cut, whole; 4 x 1028 x 1024: second trip of the backward
POOL_SHAPES = [(1, 1, 2, 4), (1, 2, 3, 8), (2, 3, 7, 8), (1, 2, 8, 12), (1, 2, 5, 16), (1, 4, 1028, 1024)]


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=_ids)
def test_maxavgpool_vector_ties(shape):
    """As test_maxavgpool_ties: inputs from {0, 1, 2}, the max half and its gradient -- to the first maximum in scan order, once -- are
    exact, the avg half goes under TOL.  The aligned call must also equal the call 8 bytes off (older kernels) bit for bit, argmax
    included."""
    RF = _rf()
    d = dev()
    gen = _gen('pool v4', shape)
    B, C = shape[:2]
    x = _ints(shape, 0, 2, gen)
    xr = x.double().requires_grad_(True)
    yr = G.maxavgpool(xr)
    gmax = _ints(yr[:, :C].shape, -8, 8, gen)
    gavg = torch.randn(yr[:, C:].shape, generator=gen)
    g_max_only, g_all = torch.cat([gmax, torch.zeros_like(gmax)], 1), torch.cat([gmax, gavg], 1)
    gr_max, = torch.autograd.grad(yr, xr, g_max_only.double(), retain_graph=True)
    gr_all, = torch.autograd.grad(yr, xr, g_all.double())
    xd = x.to(d).requires_grad_(True)
    y = RF.maxavgpool(xd)
    gd_max, = torch.autograd.grad(y, xd, g_max_only.to(d), retain_graph=True)
    gd_all, = torch.autograd.grad(y, xd, g_all.to(d))
    _same('max half', y[:, :C], yr[:, :C])
    _same('gradient of the max half', gd_max, gr_max)
    check('avg half', y[:, C:], yr[:, C:], TOL)
    check('gradient of both halves', gd_all, gr_all, TOL)
    o0, g0, a0 = _pool_abi(x, g_all, False)
    o1, g1, a1 = _pool_abi(x, g_all, True)
    assert torch.equal(_bits(o0), _bits(o1)) and torch.equal(_bits(g0), _bits(g1)) and torch.equal(a0.cpu(), a1.cpu())
    assert torch.equal(_bits(o0), _bits(y)) and torch.equal(_bits(g0), _bits(gd_all))


def test_maxavgpool_vector_nan_wins():
    """One NaN: it is the maximum of every window that holds it (four here: row 3, column 5 are odd), their averages are NaN, and the
    max half routes those windows' gradients to it.  Aligned (v4) and misaligned (older kernels) calls agree bit for bit."""
    shape = (1, 2, 6, 16)
    gen = _gen('pool nan', shape)
    x = torch.randn(shape, generator=gen)
    x[0, 1, 3, 5] = float('nan')
    gout = torch.randn(1, 4, 3, 8, generator=gen)
    o0, g0, a0 = _pool_abi(x, gout, False)
    o1, g1, a1 = _pool_abi(x, gout, True)
    assert torch.equal(_bits(o0), _bits(o1)) and torch.equal(_bits(g0), _bits(g1)) and torch.equal(a0.cpu(), a1.cpu())
    yr = G.maxavgpool(x.double())
    nan = torch.isnan(yr)
    assert int(nan.sum()) == 8 and torch.equal(torch.isnan(o0.cpu()), nan)
    assert torch.equal(o0.cpu()[:, :2][~nan[:, :2]], yr.float()[:, :2][~nan[:, :2]])
    # the gradient at the NaN: the four windows' max gradients plus (NaN-free) average gradients / 9
    want = gout[0, 1, 1:3, 2:4].double().sum() + gout[0, 3, 1:3, 2:4].double().sum() / 9
    assert abs(g0.cpu()[0, 1, 3, 5].item() - want.item()) < 1e-5 * max(1.0, abs(want.item()))


def test_maxavgpool_vector_on_random_values():
    _close('maxavgpool v4', _rf().maxavgpool, G.maxavgpool, [(2, 3, 7, 16)], lambda s: (s[0], 2 * s[1], (s[2] + 1) // 2, (s[3] + 1) // 2), 23)


# ------------------------------------------------------------------------------------------ pyramid: interior and border paths
def _down_shape(s):
    return s[:2] + ((s[2] + 1) // 2, (s[3] + 1) // 2)


def _half(s):
    return s[:2] + (s[2] // 2, s[3] // 2)


# gauss_down_fwd: interior outputs 1 <= x, 2x + 2 < W (none for W <= 4, one column for W = 5, 6); gauss_down_bwd: interior inputs
# 3 <= s <= W - 4 (none for W <= 6, one column for W = 7); the same along H
PYR_DOWN = [(2, 3, 6, 8), (2, 3, 8, 8), (1, 2, 12, 20), (2, 3, 4, 12), (2, 3, 12, 4), (2, 3, 5, 5), (2, 3, 5, 12), (2, 3, 7, 7),
            (2, 3, 7, 12), (2, 3, 12, 7), (1, 2, 13, 21)]


@pytest.mark.parametrize('shape', PYR_DOWN, ids=_ids)
def test_pyr_down_paths_exact(shape):
    _exact('pyr_down', _rf().pyr_down, G.pyr_down, [shape], _down_shape, 24)


# lap_updiff_fwd: interior outputs 2 <= x <= W - 3 (none for W = 4, two columns for W = 6); lap_updiff_bwd: interior inputs
# 2 <= b <= W / 2 - 2 (none for W <= 6, one column for W = 8); the same along H
PYR_UPDIFF = [(2, 3, 6, 8), (2, 3, 8, 8), (1, 2, 12, 20), (2, 3, 4, 4), (2, 3, 4, 12), (2, 3, 12, 4), (2, 3, 6, 6), (2, 3, 8, 6),
              (2, 3, 6, 10), (1, 2, 14, 22)]


@pytest.mark.parametrize('out_shape', PYR_UPDIFF, ids=_ids)
def test_pyr_updiff_paths_exact(out_shape):
    _exact('pyr_updiff', _rf().pyr_updiff, G.pyr_updiff, [out_shape, _half(out_shape)], lambda a, b: a, 25)


def test_pyramid_paths_on_random_values():
    RF = _rf()
    for shape in [(2, 3, 12, 20), (2, 3, 13, 9)]:
        _close('pyr_down', RF.pyr_down, G.pyr_down, [shape], _down_shape, 26)
    for shape in [(2, 3, 12, 20), (2, 3, 8, 10)]:
        _close('pyr_updiff', RF.pyr_updiff, G.pyr_updiff, [shape, _half(shape)], lambda a, b: a, 26)
