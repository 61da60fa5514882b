"""The memory-bound kernels of csrc/misc_kernels.hip and csrc/train_kernels.hip against the float64 references of glue_reference.py, at
the shapes where such kernels go wrong: H or W of 1 .. 5 and odd (reflection folds taps, windows clip), sizes past one trip of the
capped grid (4096 x 256 threads, reductions 1024 x 256), pointers off their boundary, ties, zeros and saturation.  -m gpu

Three kinds of assertion:
  exact      integer-valued inputs (0 .. 15) and output gradients (-8 .. 8): every product and sum of the pyramid operators, the bilinear
             upsample (weights k / 64) and the max half of the pool is exact in float32, so the kernel equals the float64 reference
             cast to float32 bit for bit, forward and backward;
  tolerance  TOL = 1e-5 of test_gpu_misc.py for tensors (maximum and L2 through gpu_util.check), 2e-6 relative of test_gpu_train.py for
             scalar losses and the Adam buffers;
  SSIM       a bound taken from the float32 oracle's own error against the float64 oracle on the same inputs (see SSIM_FACTOR)."""
import ctypes
import functools
import zlib

import pytest
import torch

import glue_reference as G
from gpu_util import check, dev, l2_err
from conftest import rel_err
from test_gpu_conv import _at_offset

pytestmark = pytest.mark.gpu
TOL = 1e-5      # test_gpu_misc.py
LTOL = 2e-6     # test_gpu_train.py: scalar losses, Adam


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 2 ** 31)


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()


def _grid16(shape, gen, span=32):
    """Multiples of 1 / 16 in [-span / 16, span / 16]: differences, Sobel sums and their signs are exact in float32."""
    return torch.randint(-span, span + 1, tuple(shape), generator=gen).float() / 16.0


def _run(op, ref, xs, gout):
    """op on the device and ref in float64 on the same float32 values, each with one backward: (out, grads), (out_ref, grads_ref)."""
    xr = [x.double().requires_grad_(True) for x in xs]
    yr = ref(*xr)
    yr.backward(gout.double())
    xd = [x.to(dev()).requires_grad_(True) for x in xs]
    y = op(*xd)
    y.backward(gout.to(dev()))
    return (y, [x.grad for x in xd]), (yr.detach(), [x.grad for x in xr])


def _same(name, got, ref):
    got, want = got.detach().cpu(), ref.detach().cpu().float()
    assert tuple(got.shape) == tuple(want.shape), '%s: shape %s vs %s' % (name, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = got != want
        raise AssertionError('%s: %d of %d elements differ, max |diff| %.3e, first at %s'
                             % (name, int(bad.sum()), bad.numel(), float((got - want).abs().max()), bad.nonzero()[0].tolist()))


def _exact(name, op, ref, shapes_in, shape_out_of, seed):
    gen = _gen(name, shapes_in, seed)
    xs = [_ints(s, 0, 15, gen) for s in shapes_in]
    gout = _ints(shape_out_of(*shapes_in), -8, 8, gen)
    (y, gs), (yr, grs) = _run(op, ref, xs, gout)
    _same(name + ' out', y, yr)
    for i, (a, b) in enumerate(zip(gs, grs)):
        _same('%s grad %d' % (name, i), a, b)


def _close(name, op, ref, shapes_in, shape_out_of, seed):
    gen = _gen(name, shapes_in, seed)
    xs = [torch.randn(s, generator=gen) for s in shapes_in]
    gout = torch.randn(shape_out_of(*shapes_in), generator=gen)
    (y, gs), (yr, grs) = _run(op, ref, xs, gout)
    check(name + ' out', y, yr, TOL)
    for i, (a, b) in enumerate(zip(gs, grs)):
        check('%s grad %d' % (name, i), a, b, TOL)


def _rf():
    from realvsr_amd import functional as RF
    return RF


# ------------------------------------------------------------------------------------------ pyramid operators
def _down_shape(s):
    return s[:2] + ((s[2] + 1) // 2, (s[3] + 1) // 2)


def _up_shape(s):
    return s[:2] + (2 * s[2], 2 * s[3])


@pytest.mark.parametrize('shape', [(2, 3, 3, 3), (2, 3, 3, 8), (2, 3, 4, 3), (2, 3, 5, 7), (2, 3, 7, 5), (2, 3, 6, 6), (2, 3, 9, 4),
                                   (1, 5, 1031, 919)], ids=lambda s: 'x'.join(map(str, s)))
def test_pyr_down_exact(shape):
    """gauss_down_fwd / gauss_down_bwd: at H or W of 3 .. 5 both reflections land inside one 5-tap row, the 7-tap candidate window of the
    gather clips on both sides, odd sizes end on a centre tap; 1031 x 919: 1.19 M outputs, 4.7 M inputs (second trip both ways).
    (That window is wider than the operation needs: for every H from 3 to 199 only the outputs r / 2 - 1 .. r / 2 + 1 carry weight for
    input row r, so a kernel that scans 5 candidates from r / 2 - 2 is not wrong and passes; one that stops at r / 2 fails here.)"""
    _exact('pyr_down', _rf().pyr_down, G.pyr_down, [shape], _down_shape, 1)


# output sizes of the x2 operators (and the sizes conv_gauss runs at)
UP_OUT = [(2, 3, 4, 4), (2, 3, 4, 10), (2, 3, 6, 4), (2, 3, 10, 6), (1, 5, 1030, 920)]


def _half(s):
    return s[:2] + (s[2] // 2, s[3] // 2)


@pytest.mark.parametrize('out_shape', UP_OUT, ids=lambda s: 'x'.join(map(str, s)))
def test_pyr_updiff_exact(out_shape):
    """lap_updiff_fwd / lap_updiff_bwd (9-tap candidate window); 1030 x 920: n = planes * Hd * Wd = 1.18 M (second trip of the gather)."""
    _exact('pyr_updiff', _rf().pyr_updiff, G.pyr_updiff, [out_shape, _half(out_shape)], lambda a, b: a, 2)


@pytest.mark.parametrize('out_shape', UP_OUT, ids=lambda s: 'x'.join(map(str, s)))
def test_pyr_upsample_exact(out_shape):
    """gauss_full_fwd / gauss_full_bwd with zero insertion (up = 1); 4 x 4 is the upsample of a 2 x 2 image."""
    _exact('pyr_upsample', _rf().pyr_upsample, G.pyr_upsample, [_half(out_shape)], _up_shape, 3)


@pytest.mark.parametrize('gain', [1.0, 4.0])
@pytest.mark.parametrize('shape', UP_OUT + [(2, 3, 3, 3), (2, 3, 3, 9), (2, 3, 5, 4)], ids=lambda s: 'x'.join(map(str, s)))
def test_conv_gauss_exact(shape, gain):
    """gauss_full_fwd / gauss_full_bwd without zero insertion (5-tap candidate window), gain 1 and 4."""
    RF = _rf()
    _exact('conv_gauss', lambda x: RF.conv_gauss(x, gain), lambda x: G.conv_gauss(x, gain), [shape], lambda a: a, 4)


def test_pyramid_operators_on_random_values():
    RF = _rf()
    _close('pyr_down', RF.pyr_down, G.pyr_down, [(2, 3, 7, 5)], _down_shape, 5)
    _close('pyr_updiff', RF.pyr_updiff, G.pyr_updiff, [(2, 3, 6, 10), (2, 3, 3, 5)], lambda a, b: a, 5)
    _close('pyr_upsample', RF.pyr_upsample, G.pyr_upsample, [(2, 3, 3, 5)], _up_shape, 5)
    _close('conv_gauss', lambda x: RF.conv_gauss(x, 4.0), lambda x: G.conv_gauss(x, 4.0), [(2, 3, 5, 9)], lambda a: a, 5)


# ------------------------------------------------------------------------------------------ bilinear upsample
UPS_SHAPES = [(1, 1, 1, 1), (1, 2, 1, 5), (2, 3, 5, 1), (1, 3, 7, 9), (1, 7, 390, 387)]


@pytest.mark.parametrize('factor,scale', [(2, 1.0), (2, 2.0), (4, 1.0), (4, 2.0)])
@pytest.mark.parametrize('shape', UPS_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_upsample_bilinear_exact(shape, factor, scale):
    """x2: upsample2_fwd / upsample2_bwd (one thread per input pixel; 7 x 390 x 387 = 1.06 M: second trip); x4: the generic kernels.
    H or W of 1: both taps of a row clamp onto the same pixel."""
    RF = _rf()
    _exact('upsample x%d' % factor, lambda x: RF.upsample_bilinear(x, factor, scale), lambda x: G.upsample_bilinear(x, factor, scale),
           [shape], lambda s: s[:2] + (s[2] * factor, s[3] * factor), 6)


@pytest.mark.parametrize('shape', [(1, 2, 1, 5), (2, 3, 5, 1), (1, 3, 7, 9)], ids=lambda s: 'x'.join(map(str, s)))
def test_upsample_x2_generic_kernels_exact(shape):
    """A pointer 4 bytes behind an 8-byte boundary takes the x2 call off the float2 kernels: the output gradient so placed reaches
    upsample_bwd_kernel with its S == 2 window (rows 2y - 1 .. 2y + 2), an `out` so placed reaches upsample_fwd_kernel."""
    from realvsr_amd import _lib
    RF = _rf()
    d = dev()
    gen = _gen('upsample generic', shape)
    x = _ints(shape, 0, 15, gen)
    oshape = shape[:2] + (2 * shape[2], 2 * shape[3])
    gout = _ints(oshape, -8, 8, gen)
    xr = x.double().requires_grad_(True)
    yr = G.upsample_bilinear(xr, 2, 2.0)
    yr.backward(gout.double())
    xd = x.to(d).requires_grad_(True)
    y = RF.upsample_bilinear(xd, 2, 2.0)
    g_off = _at_offset(gout, 1, d, leaf=False)
    assert g_off.data_ptr() % 8 == 4 and g_off.is_contiguous()
    y.backward(g_off)
    _same('generic x2 backward', xd.grad, xr.grad)
    # forward: the C ABI with an output placed the same way
    n = yr.numel()
    buf = torch.full((n + 8,), -77.0, device=d)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + n].view(oshape)
    xc = x.to(d)
    _lib.check(_lib.lib().rvsr_upsample_bilinear_forward(_lib._p(xc), ctypes.c_void_p(out.data_ptr()), shape[0] * shape[1], shape[2],
                                                         shape[3], 2, 2.0, _lib._stream()), 'upsample_bilinear_forward')
    _same('generic x2 forward', out, yr)
    _same('generic x2 forward == float2 kernel', out, y)
    assert float(buf[0]) == -77.0 and bool((buf[1 + n:] == -77.0).all())      # nothing written either side of the view


def test_upsample_on_random_values():
    RF = _rf()
    for factor in (2, 4):
        _close('upsample x%d' % factor, lambda x: RF.upsample_bilinear(x, factor, 2.0), lambda x: G.upsample_bilinear(x, factor, 2.0),
               [(2, 3, 5, 7)], lambda s: s[:2] + (s[2] * factor, s[3] * factor), 7)


# ------------------------------------------------------------------------------------------ max + avg pool
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 2, 2, 2), (2, 3, 7, 9), (1, 2, 8, 6), (1, 5, 919, 921)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_maxavgpool_ties(shape):
    """Inputs from {0, 1, 2}: most windows hold their maximum several times.  The max half and its gradient -- routed to the first
    maximum in scan order, once -- are exact; the avg half (1 / 9 is not a float) goes under TOL.  919 x 921: 1.06 M outputs."""
    RF = _rf()
    d = dev()
    gen = _gen('pool', shape)
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


def test_maxavgpool_on_random_values():
    _close('maxavgpool', _rf().maxavgpool, G.maxavgpool, [(2, 3, 7, 9)], lambda s: (s[0], 2 * s[1], (s[2] + 1) // 2, (s[3] + 1) // 2), 8)


# ------------------------------------------------------------------------------------------ clip augmentation
def _augment_case(shape, perm, box_mode, box, seed):
    RF = _rf()
    gen = _gen('augment', shape, seed)
    a, b = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    o1, o2 = RF.augment_clips(a.to(dev()), b.to(dev()), perm=perm, box_mode=box_mode, box=box)
    r1, r2 = G.augment_clips(a, b, perm, box_mode, box)
    name = 'augment %s mode %d box %s' % (perm, box_mode, box)
    _same(name + ' out1', o1, r1)
    _same(name + ' out2', o2, r2)


@pytest.mark.parametrize('box_mode', [0, 1, 2])
def test_augment_clips_boxes_at_the_border(box_mode):
    """(y0, y1, x0, x1) on a 6 x 7 frame: touching row 0 and column 0, row H and column W, the whole frame, empty, inverted."""
    for box in [(0, 3, 0, 4), (2, 6, 3, 7), (0, 6, 0, 7), (3, 3, 2, 5), (4, 2, 5, 1), (5, 6, 6, 7)]:
        _augment_case((2, 2, 3, 6, 7), (2, 0, 1), box_mode, box, 9)


def test_augment_clips_second_trip():
    _augment_case((2, 3, 3, 245, 243), (1, 2, 0), 1, (17, 245, 0, 100), 10)       # 1.07 M elements
    _augment_case((2, 3, 3, 245, 243), (1, 0, 2), 2, (0, 200, 143, 243), 10)


# ------------------------------------------------------------------------------------------ TSA
def _tsa_inputs(B, N, C, H, W, seed, emb_scale=0.3, on_grid=False):
    gen = _gen('tsa', B, N, C, H, W, seed)
    emb, ref = torch.randn(B, N, C, H, W, generator=gen) * emb_scale, torch.randn(B, C, H, W, generator=gen)
    if on_grid:
        # integers times quarters: every product and the channel sum are exact in float32, so the kernel's correlation is the
        # reference's and the saturated set is the same on both sides
        emb, ref = emb.round(), (ref * 4).round() / 4
    else:
        ref = ref * 0.3
    aligned, gmod = torch.randn(B, N, C, H, W, generator=gen), torch.randn(B, N * C, H, W, generator=gen)
    return emb, ref, aligned, gmod


def _tsa_reference(emb, ref, aligned, gmod, frame_major=False):
    r = [t.double().requires_grad_(True) for t in (emb, ref, aligned)]
    out = G.tsa_temporal(*r, frame_major=frame_major)
    out.backward(gmod.double())
    return out.detach(), [t.grad for t in r]


def _tsa_abi(emb, ref, aligned, gmod, B, N, C, H, W, frame_major):
    """rvsr_tsa_temporal_forward / _backward called directly (the only way to the frame-major layout without the fused TSA block)."""
    from realvsr_amd import _lib
    d, L, p = dev(), _lib.lib(), _lib._p
    emb, ref, aligned, gmod = (t.to(d).contiguous() for t in (emb, ref, aligned, gmod))
    mod, prob = torch.empty(B, N * C, H, W, device=d), torch.empty(B, N, H, W, device=d)
    _lib.check(L.rvsr_tsa_temporal_forward(p(emb), p(ref), p(aligned), p(mod), p(prob), B, N, C, H, W, frame_major, _lib._stream()), 'fwd')
    galigned, gemb, gref = torch.empty_like(aligned), torch.empty_like(emb), torch.empty_like(ref)
    _lib.check(L.rvsr_tsa_temporal_backward(p(gmod), p(emb), p(ref), p(aligned), p(prob), p(galigned), p(gemb), p(gref), B, N, C, H, W,
                                            frame_major, _lib._stream()), 'bwd')
    return mod, prob, [gemb, gref, galigned]


@pytest.mark.parametrize('dims', [(2, 1, 3, 5, 7), (2, 5, 3, 5, 7), (2, 8, 3, 5, 7), (1, 2, 2, 1025, 1025)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_tsa_temporal_both_layouts(dims):
    """N = 1, 5, 8 (8: every slot of the backward's per-frame array) and B * HW = 1 050 625 (second trip of the backward, whose grid
    runs over B * HW), through RF.tsa_temporal ([B][N]) and through the C ABI with frame_major = 1 ([N][B])."""
    RF = _rf()
    B, N, C, H, W = dims
    emb, ref, aligned, gmod = _tsa_inputs(*dims, seed=11)
    outr, grs = _tsa_reference(emb, ref, aligned, gmod)
    t = [v.to(dev()).requires_grad_(True) for v in (emb, ref, aligned)]
    y = RF.tsa_temporal(*t)
    y.backward(gmod.to(dev()))
    check('mod', y, outr, TOL)
    for name, a, b in zip(('gemb', 'gemb_ref', 'galigned'), t, grs):
        check(name, a.grad, b, TOL)
    # frame-major: the same numbers with emb / aligned transposed in memory
    emb_t, al_t = emb.transpose(0, 1).contiguous(), aligned.transpose(0, 1).contiguous()
    outr2, grs2 = _tsa_reference(emb_t, ref, al_t, gmod, frame_major=True)
    assert torch.equal(outr2, outr)
    mod, _, gs = _tsa_abi(emb_t, ref, al_t, gmod, B, N, C, H, W, 1)
    check('mod (frame-major)', mod, outr2, TOL)
    for name, a, b in zip(('gemb', 'gemb_ref', 'galigned'), gs, grs2):
        check(name + ' (frame-major)', a, b, TOL)
    assert torch.equal(mod, y.detach())


def test_tsa_temporal_saturated():
    """emb scaled by 30: the correlation reaches +-100 and more.  Where it is above 18 the float32 sigmoid is exactly 1 (exp(-18) <
    2^-25), below -90 it is exactly 0 (exp(90) overflows float32): the output is `aligned` or 0 there, bit for bit, the gradients of emb
    are exactly 0, and everything stays finite; the rest is held to TOL like any other case."""
    RF = _rf()
    dims = (2, 5, 16, 9, 13)
    B, N, C, H, W = dims
    emb, ref, aligned, gmod = _tsa_inputs(*dims, seed=12, emb_scale=30.0, on_grid=True)
    cor = G.tsa_correlation(emb.double(), ref.double())                    # (B, N, H, W), exact
    one, zero = cor > 18, cor < -90
    assert int(one.sum()) > 100 and int(zero.sum()) > 100 and int((~one & ~zero).sum()) > 100
    outr, grs = _tsa_reference(emb, ref, aligned, gmod)
    t = [v.to(dev()).requires_grad_(True) for v in (emb, ref, aligned)]
    y = RF.tsa_temporal(*t)
    y.backward(gmod.to(dev()))
    check('mod', y, outr, TOL)
    for name, a, b in zip(('gemb', 'gemb_ref', 'galigned'), t, grs):
        check(name, a.grad, b, TOL)
    mod = y.detach().cpu().view(B, N, C, H, W)
    gemb, gal = t[0].grad.cpu(), t[2].grad.cpu()
    gm = gmod.view(B, N, C, H, W)
    m1, m0 = one.unsqueeze(2).expand_as(mod), zero.unsqueeze(2).expand_as(mod)
    assert torch.equal(mod[m1], aligned[m1]) and torch.equal(gal[m1], gm[m1])
    assert int(torch.count_nonzero(mod[m0])) == 0 and int(torch.count_nonzero(gal[m0])) == 0
    assert int(torch.count_nonzero(gemb[m1 | m0])) == 0
    # a pixel whose frames are all saturated passes nothing to emb_ref either
    allsat = (one | zero).all(1).unsqueeze(1).expand(B, C, H, W)
    assert int(allsat.sum()) > 0 and int(torch.count_nonzero(t[1].grad.cpu()[allsat])) == 0


def test_tsa_temporal_backward_refuses_nine_frames():
    """N = 9 > TSA_MAXN: the forward runs, the backward is refused with RuntimeError and launches nothing."""
    from realvsr_amd import _lib
    RF = _rf()
    dims = (1, 9, 2, 3, 5)
    B, N, C, H, W = dims
    emb, ref, aligned, gmod = _tsa_inputs(*dims, seed=13)
    outr, _ = _tsa_reference(emb, ref, aligned, gmod)
    t = [v.to(dev()).requires_grad_(True) for v in (emb, ref, aligned)]
    y = RF.tsa_temporal(*t)
    check('mod', y, outr, TOL)
    with pytest.raises(RuntimeError):
        y.backward(gmod.to(dev()))
    d, L, p = dev(), _lib.lib(), _lib._p
    outs = [torch.full(s, -77.0, device=d) for s in (aligned.shape, emb.shape, ref.shape)]
    prob = torch.rand(B, N, H, W, device=d)
    e, r, a, g = (v.to(d) for v in (emb, ref, aligned, gmod))
    rc = L.rvsr_tsa_temporal_backward(p(g), p(e), p(r), p(a), p(prob), p(outs[0]), p(outs[1]), p(outs[2]), B, N, C, H, W, 0, _lib._stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert all(bool((o == -77.0).all()) for o in outs)


@pytest.mark.parametrize('shape', [(2, 3, 7, 9), (1, 2, 731, 727)], ids=lambda s: 'x'.join(map(str, s)))
def test_tsa_output_saturated(shape):
    """|att| up to 90: exp(90) overflows float32, the sigmoid is exactly 0 there and the attention gradient 0 * 1; nothing is NaN.
    731 x 727: n = 1 062 874, not a multiple of 4 -- second trip of tsa_final_fwd / tsa_final_bwd, which are element-wise over n."""
    RF = _rf()
    gen = _gen('tsa_output', shape)
    fea, add, gout = (torch.randn(shape, generator=gen) for _ in range(3))
    att = (torch.rand(shape, generator=gen) * 2 - 1) * 90
    att.view(-1)[:6] = torch.tensor([90.0, -90.0, 89.5, -89.5, 0.0, -0.0])
    (y, gs), (yr, grs) = _run(RF.tsa_output, G.tsa_output, [fea, att, add], gout)
    check('tsa_output', y, yr, TOL)
    for name, a, b in zip(('gfea', 'gatt', 'gadd'), gs, grs):
        check(name, a, b, TOL)
    low = (att < -89).to(dev())
    assert int(low.sum()) >= 2 and int(torch.count_nonzero(gs[1][low])) == 0


# ------------------------------------------------------------------------------------------ element-wise losses
LOSS_SHAPES = [(1,), (255,), (257,), (1, 2, 731, 727)]     # 1.06 M: second trip of the reduction (1024 x 256) and of the backward


@functools.lru_cache(maxsize=None)
def _loss_inputs(shape, on_grid):
    gen = _gen('loss', shape, on_grid)
    if not on_grid:
        return torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    # 1 / 16 grid, a block with x == y (d == 0), and differences of exactly +-1 / 16 among the rest (|d| == delta for Huber)
    x, y = _grid16(shape, gen, 8), _grid16(shape, gen, 8)
    n = x.numel()
    y.view(-1)[n // 3:n // 3 + max(n // 5, 1)] = x.view(-1)[n // 3:n // 3 + max(n // 5, 1)]
    if n == 1:
        y = x + 1.0 / 16
    return x, y


def _loss_case(name, op, ref, shape, on_grid):
    x, y = _loss_inputs(shape, on_grid)
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    lr = ref(xr, yr)
    lr.backward()
    xd, yd = x.to(dev()).requires_grad_(True), y.to(dev()).requires_grad_(True)
    l = op(xd, yd)
    l.backward()
    print('%-44s %.9g vs %.9g' % (name, l.item(), lr.item()))
    assert abs(l.item() - lr.item()) <= LTOL * abs(lr.item()), (name, shape, l.item(), lr.item())
    check(name + ' gx', xd.grad, xr.grad, TOL)
    check(name + ' gy', yd.grad, yr.grad, TOL)
    if on_grid:
        zero = (x == y).to(dev())
        assert int(torch.count_nonzero(xd.grad[zero])) == 0 and int(torch.count_nonzero(yd.grad[zero])) == 0, name + ': gradient at d == 0'
    return x, y, xd.grad


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_charbonnier(shape, reduction):
    """charb_fwd / charb_bwd (RF.charbonnier) and mode 3 of the pixel-loss kernels, eps 1e-6 and 1e-3."""
    RF = _rf()
    for eps in (1e-6, 1e-3):
        _loss_case('charbonnier eps %g' % eps, lambda a, b: RF.charbonnier(a, b, eps, reduction),
                   lambda a, b: G.charbonnier(a, b, eps, reduction), shape, False)
        _loss_case('pixel_loss cb eps %g' % eps, lambda a, b: RF.pixel_loss(a, b, RF.PIX_CHARBONNIER, eps, reduction),
                   lambda a, b: G.charbonnier(a, b, eps, reduction), shape, False)


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_l1_l2_huber(shape, reduction):
    """L1 and Huber on the 1 / 16 grid: the block with x == y must get a gradient of exactly 0 (sign(0) = 0), and with delta = 1 / 16
    the elements with |d| == delta sit on the joint of the two Huber branches; L2 on random values."""
    RF = _rf()
    _loss_case('l1', lambda a, b: RF.pixel_loss(a, b, RF.PIX_L1, 0.0, reduction), lambda a, b: G.l1(a, b, reduction), shape, True)
    x, y, gx = _loss_case('huber', lambda a, b: RF.pixel_loss(a, b, RF.PIX_HUBER, 1.0 / 16, reduction),
                          lambda a, b: G.huber(a, b, 1.0 / 16, reduction), shape, True)
    joint = (x - y).abs() == 1.0 / 16
    assert int(joint.sum()) >= 1
    if x.numel() > 100:
        assert int(((x - y).abs() > 1.0 / 16).sum()) > 0 and int((x == y).sum()) > 0
    # at the joint both branches give delta * sign(d): exactly, in float32 (times 1 / n for 'mean')
    k = 1.0 / x.numel() if reduction == 'mean' else 1.0
    want = (torch.sign(x - y) / 16.0 * torch.tensor(k, dtype=torch.float32))[joint]
    assert torch.equal(gx.cpu()[joint], want)
    _loss_case('huber delta 1e-2', lambda a, b: RF.pixel_loss(a, b, RF.PIX_HUBER, 1e-2, reduction),
               lambda a, b: G.huber(a, b, 1e-2, reduction), shape, False)
    _loss_case('l2', lambda a, b: RF.pixel_loss(a, b, RF.PIX_L2, 0.0, reduction), lambda a, b: G.l2(a, b, reduction), shape, False)


# ------------------------------------------------------------------------------------------ GWLoss
@pytest.mark.parametrize('w,reduction', [(4, 'mean'), (2, 'sum')])
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 1, 1, 7), (1, 2, 5, 1), (2, 2, 9, 13), (1, 2, 731, 727)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_gw_loss_with_zeros(shape, w, reduction):
    """Inputs on the 1 / 16 grid with a block of x1 == x2: a fifth of the differences and a share of the Sobel responses are exactly 0,
    every Sobel sum is exact in float32, so no sign differs between the kernel and the reference and nothing is masked: the kernel's
    choice sign(0) = 0 is torch's.  H or W of 1: the whole Sobel window but its centre row / column is padding."""
    RF = _rf()
    gen = _gen('gw', shape)
    x1, x2 = _grid16(shape, gen, 8), _grid16(shape, gen, 8)
    n = x1.numel()
    if n > 4:
        x2.view(-1)[n // 3:n // 3 + max(n // 5, 1)] = x1.view(-1)[n // 3:n // 3 + max(n // 5, 1)]
    else:
        x2 = x1 + 3.0 / 16
    if n > 100:
        d = (x1 - x2).double()
        assert int((d == 0).sum()) > n // 6 and int((G.sobel_x(d) == 0).sum()) > 0
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    lr = G.gw_loss(a, b, w, reduction)
    lr.backward()
    ad, bd = x1.to(dev()).requires_grad_(True), x2.to(dev()).requires_grad_(True)
    l = RF.gw_loss(ad, bd, w, reduction)
    l.backward()
    print('gw_loss %s: %.9g vs %.9g' % (shape, l.item(), lr.item()))
    assert abs(l.item() - lr.item()) <= LTOL * abs(lr.item()), (shape, l.item(), lr.item())
    check('gw gx1', ad.grad, a.grad, TOL)
    check('gw gx2', bd.grad, b.grad, TOL)


def test_gw_loss_on_random_values():
    RF = _rf()
    gen = _gen('gw randn')
    x1, x2 = torch.randn(2, 3, 7, 11, generator=gen), torch.randn(2, 3, 7, 11, generator=gen)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    lr = G.gw_loss(a, b, 4, 'mean')
    lr.backward()
    ad = x1.to(dev()).requires_grad_(True)
    l = RF.gw_loss(ad, x2.to(dev()), 4, 'mean')
    l.backward()
    assert abs(l.item() - lr.item()) <= LTOL * abs(lr.item())
    check('gw gx1', ad.grad, a.grad, TOL)


# ------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, 4 * 1048576 + 3, 4 * (1048576 + 257) + 1])
def test_adam_step_tails(n, wd):
    """adam_step_kernel works on float4s and finishes n % 4 elements in a tail that FlatBuffers' padding to 64 never reaches: n = 1, 3,
    5, 1027 and 4 * 2^20 + 3 run it (the last with every thread of the capped grid busy), 4 has none, 4 * (2^20 + 257) + 1 makes the
    float4 loop take a second trip.  Three steps with fresh gradients against torch's operation order in float64."""
    RF = _rf()
    d = dev()
    gen = _gen('adam', n)
    lr, b1, b2, eps = 0.05, 0.9, 0.99, 1e-8
    p0 = torch.randn(n, generator=gen)
    p, m, v = p0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in (1, 2, 3):
        # |g| in [0.5, 1.5) * 0.5^(t - 1), either sign: clear of -wd * p (at most 0.06), where g + wd * p cancels, float32 keeps the sum to
        # 1e-7 of g only, and a sum of the order of eps makes the update as ill-conditioned as that
        g = (0.5 + torch.rand(n, generator=gen)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float() * 0.5 ** (t - 1)
        RF.adam_step_(p, g.to(d), m, v, lr / (1 - b1 ** t), b1, b2, eps, wd, (1 - b2 ** t) ** 0.5)
        pr, mr, vr = G.adam_step(pr, g.double(), mr, vr, t, lr, b1, b2, eps, wd)
    check('param', p, pr, LTOL)
    check('exp_avg', m, mr, LTOL)
    check('exp_avg_sq', v, vr, LTOL)
    # element-wise as well: the tail's few elements must not hide behind the maximum of a long buffer
    tail = slice(n - (n % 4 or 4), n)
    check('param tail', p[tail], pr[tail], LTOL)
    check('exp_avg tail', m[tail], mr[tail], LTOL)
    check('exp_avg_sq tail', v[tail], vr[tail], LTOL)


def test_adam_step_refuses_a_misaligned_buffer():
    RF = _rf()
    d = dev()
    n = 16
    buf = torch.rand(n + 8, device=d) + 0.5
    assert buf.data_ptr() % 16 == 0
    ok = [torch.rand(n, device=d) + 0.5 for _ in range(4)]       # (a step on these moves every one of p, m and v)
    before = [t.clone() for t in ok + [buf]]
    for i in range(4):
        bad = list(ok)
        bad[i] = buf[1:1 + n]
        with pytest.raises(RuntimeError):
            RF.adam_step_(bad[0], bad[1], bad[2], bad[3], 1e-3, 0.9, 0.99, 1e-8, 0.0, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ok + [buf], before))       # refused before anything was launched


# ------------------------------------------------------------------------------------------ SSIM
# The bound comes from the reference: the error of oracle/ssim_oracle.py run in float32 against the same oracle in float64 on the case's own
# inputs is what float32 arithmetic costs this computation (0.4 .. 2.1e-6 maximum, 0.6 .. 1.4e-6 L2 on random images, measured on the CPU).
# The kernel, also float32 but with another summation order of the 121-tap sums, is held to 8 times that and never looser than the
# 2e-4 / 2e-6 + 1e-5 |loss| of test_ssim_loss_vs_oracle.
#
# Errors of the kernel on the MI355X against the float64 oracle, gx and gy, maximum / L2 (in brackets the float32 oracle's), and of the loss:
#   1x1x11x11    gx 8.7e-7 / 9.2e-7 (9.7e-7 / 8.9e-7)   gy 8.3e-7 / 9.8e-7 (8.3e-7 / 1.1e-6)   loss 3.1e-7 (1.3e-7)
#   2x2x11x40    gx 1.3e-6 / 9.7e-7 (1.5e-6 / 1.0e-6)   gy 1.7e-6 / 1.2e-6 (1.6e-6 / 1.2e-6)   loss 7.7e-8 (7.7e-8)
#   1x1x40x11    gx 1.2e-6 / 8.4e-7 (1.1e-6 / 8.8e-7)   gy 9.9e-7 / 9.0e-7 (9.0e-7 / 9.6e-7)   loss 7.2e-8 (1.2e-7)
#   1x1x12x13    gx 1.4e-6 / 1.3e-6 (1.1e-6 / 1.2e-6)   gy 2.7e-6 / 1.9e-6 (2.3e-6 / 1.8e-6)   loss 6.3e-7 (6.3e-7)
#   1x2x731x727  gx 1.7e-6 / 9.3e-7 (1.5e-6 / 9.3e-7)   gy 1.6e-6 / 1.0e-6 (1.5e-6 / 1.0e-6)   loss 8.1e-8 (1.1e-7)
# The kernel sits at 0.9 .. 1.25 times the float32 oracle's error; nothing needs the factor.
SSIM_FACTOR = 8.0
SSIM_CASES = [(1, 1, 11, 11), (2, 2, 11, 40), (1, 1, 40, 11), (1, 1, 12, 13), (1, 2, 731, 727)]


def _ssim_grads(x, y, dtype):
    xr, yr = x.detach().to(dtype).clone().requires_grad_(True), y.detach().to(dtype).clone().requires_grad_(True)
    l = G.ssim_loss(xr, yr)
    l.backward()
    return l.detach(), xr.grad, yr.grad


@functools.lru_cache(maxsize=None)
def _ssim_case(shape):
    gen = _gen('ssim', shape)
    x = torch.rand(shape, generator=gen)
    y = (x + 0.2 * torch.randn(shape, generator=gen)).clamp(0, 1)
    return x, y, _ssim_grads(x, y, torch.float64), _ssim_grads(x, y, torch.float32)


def _ssim_kernel(x, y):
    RF = _rf()
    xd, yd = x.detach().to(dev()).requires_grad_(True), y.detach().to(dev()).requires_grad_(True)
    l = RF.ssim_loss(xd, yd)
    l.backward()
    return l.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()


@pytest.mark.parametrize('shape', SSIM_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_ssim_within_the_float32_oracles_error(shape):
    """11 x 11: one window; 11 x 40 / 40 x 11: one row / column of windows; 12 x 13: 2 x 3 windows; 731 x 727: 1.03 M windows, 1.06 M
    pixels (second trip of both kernels)."""
    x, y, (l64, gx64, gy64), (l32, gx32, gy32) = _ssim_case(shape)
    l, gx, gy = _ssim_kernel(x, y)
    e_loss = abs(l32.item() - l64.item())
    bound = min(SSIM_FACTOR * e_loss, 2e-6 + 1e-5 * abs(l64.item()))
    print('ssim %s loss %.9g vs %.9g: |diff| %.3e (float32 oracle %.3e, bound %.3e)'
          % (shape, l.item(), l64.item(), abs(l.item() - l64.item()), abs(l32.item() - l64.item()), bound))
    fails = []
    if not abs(l.item() - l64.item()) <= bound:
        fails.append('loss')
    for name, g, g32, g64 in (('gx', gx, gx32, gx64), ('gy', gy, gy32, gy64)):
        assert torch.isfinite(g).all()
        o_max, o_l2 = rel_err(g32, g64), l2_err(g32, g64)
        b_max = min(SSIM_FACTOR * o_max, 2e-4)
        b_l2 = min(SSIM_FACTOR * o_l2, 3 * 2e-4)
        k_max, k_l2 = rel_err(g, g64), l2_err(g, g64)
        print('ssim %s %s: rel_err %.3e (float32 oracle %.3e, bound %.3e)  l2_err %.3e (float32 oracle %.3e, bound %.3e)'
              % (shape, name, k_max, o_max, b_max, k_l2, o_l2, b_l2))
        if not (k_max <= b_max and (g.numel() == 1 or k_l2 <= b_l2)):
            fails.append(name)
    assert not fails, fails


def test_ssim_clamped_everywhere():
    """y = 1 - x: the covariance is minus the variance, every contrast-structure value is negative and relu clamps it: the loss is exactly
    1 and both gradients exactly 0."""
    for shape in [(1, 1, 12, 13), (1, 1, 37, 19)]:
        x = torch.rand(shape, generator=_gen('ssim clamp', shape))
        l, gx, gy = _ssim_kernel(x, 1 - x)
        assert l.item() == 1.0, l.item()
        assert int(torch.count_nonzero(gx)) == 0 and int(torch.count_nonzero(gy)) == 0


def test_ssim_degenerate_pairs():
    """Two constant images: zero variance, the float32 moments cancel to rounding noise (the float32 oracle's own gradient error is 3e-4
    there) -- everything must be finite.  x == y: the loss is 0 within 1e-6 and the gradients (1e-17 in exact arithmetic) finite.
    Seen on the MI355X for the constants (0.25, 0.75): loss 0.400219 against 0.399937 in float64 and 0.400189 from the float32 oracle,
    gx 3.5e-4 (float32 oracle 3.1e-4); for two equal constants 0.7 the loss comes out as -1.3e-4, not 0: the rounding noise of
    E[xx] - mu^2 (1e-7) stands against C2 = 9e-4 and numerator and denominator no longer cancel bit for bit -- a property of the
    zero-variance corner, not of images (x == y with a random image gives |loss| <= 1e-6, asserted below)."""
    shape = (2, 1, 13, 17)
    for cx, cy in [(0.25, 0.75), (0.7, 0.7), (0.0, 1.0), (0.0, 0.0)]:
        x, y = torch.full(shape, cx), torch.full(shape, cy)
        l, gx, gy = _ssim_kernel(x, y)
        l64, gx64, _ = _ssim_grads(x, y, torch.float64)
        l32, gx32, _ = _ssim_grads(x, y, torch.float32)
        print('ssim constants %g, %g: loss %.9g (float64 %.9g, float32 %.9g); gx rel_err %.3e (float32 oracle %.3e)'
              % (cx, cy, l.item(), l64.item(), l32.item(), rel_err(gx, gx64), rel_err(gx32, gx64)))
        assert torch.isfinite(l).all() and torch.isfinite(gx).all() and torch.isfinite(gy).all()
    x = torch.rand(shape, generator=_gen('ssim same'))
    l, gx, gy = _ssim_kernel(x, x.clone())
    assert abs(l.item()) <= 1e-6, l.item()
    assert torch.isfinite(gx).all() and torch.isfinite(gy).all()
