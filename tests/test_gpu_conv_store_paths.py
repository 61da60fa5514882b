"""The output-side paths of conv_fwd5 / conv_wgrad2 that have a vector-store form and an element form (csrc/conv2_kernels.hip):
the pixel-shuffle epilogue (8-byte stores), the split-output epilogue (16-byte stores), the LDS-staged partial sums of the weight gradient,
and the zero-insert data gradient that skips its zero rows.  Where the launcher can be steered onto the old path (an output displaced by
one float is neither 8- nor 16-byte aligned) the two paths are compared with torch.equal; every path is held to float64 at the tolerance
of tests/test_gpu_conv.py.  -m gpu

(The split output takes no residual: rvsr_conv2d_forward refuses the combination, so there is no such case to run.)"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from gpu_util import check, dev

pytestmark = pytest.mark.gpu
TOL = 1e-4                                          # tests/test_gpu_conv.py, bf16x3 (the default GEMM mode)
WG_TOLS = {'bf16x3': 1e-4, 'bf16x2': 2e-2, 'bf16': 2e-2}   # the same table, the three split modes of conv_wgrad2


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))   # (the same inputs in every process)


def _out(shape, off, d):
    """An output tensor `off` floats behind a 16-byte boundary (0: aligned, the vector path; 1: the element path)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 8,), float('nan'), device=d)
    assert buf.data_ptr() % 16 == 0
    return buf[off:off + n].view(shape)


def _lrelu64(y, act):
    return F.leaky_relu(y, 0.1) if act else y


# ------------------------------------------------------------------------------------------ pixel shuffle
PS_SHAPES = [
    (2, 64, 64, 16, 32),    # one full tile
    (2, 16, 12, 10, 36),    # a cut m-block, partial tiles on both edges
    (1, 64, 80, 17, 33),    # a second, cut m-block; odd sizes
    (3, 64, 256, 8, 64),    # four m-blocks
]


def _ps_run(shape, act, offs):
    from realvsr_amd import functional as RF
    B, C, Co, H, W = shape
    g, d = _gen('ps', shape), dev()
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (3.0 * C ** 0.5)
    b = torch.randn(Co, generator=g) * 0.1
    xd, wd, bd = x.to(d), w.to(d), b.to(d)
    outs = []
    for off in offs:
        o = _out((B, Co // 4, 2 * H, 2 * W), off, d)
        RF._conv(xd, wd, o, bias=bd, act=RF.ACT_LRELU if act else RF.ACT_NONE, slope=0.1, pixel_shuffle=True, what='ps forward')
        outs.append(o)
    torch.cuda.synchronize()
    return outs, (x, w, b)


@pytest.mark.parametrize('act', [False, True], ids=['none', 'lrelu'])
@pytest.mark.parametrize('shape', PS_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pixel_shuffle_vector_epilogue_equals_element_epilogue(shape, act):
    (vec, elem), (x, w, b) = _ps_run(shape, act, (0, 1))
    assert torch.equal(vec, elem)
    if shape == PS_SHAPES[2]:
        ref = _lrelu64(F.pixel_shuffle(F.conv2d(x.double(), w.double(), b.double(), padding=1), 2), act)
        check('pixel-shuffle forward', vec, ref, TOL)


# ------------------------------------------------------------------------------------------ split output
SPLIT_SHAPES = [(2, 64, 16, 32), (2, 16, 10, 36), (3, 64, 8, 64), (2, 64, 10, 40)]   # (B, C, H, W), W % 4 == 0


def _split_run(shape, Co1, Co2, xact, offs):
    from realvsr_amd import functional as RF
    B, C, H, W = shape
    g, d = _gen('split', shape, Co1, Co2, xact), dev()
    gout = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, Co1 + Co2, 3, 3, generator=g) / (3.0 * C ** 0.5)   # the forward conv's weight: (its Co, its C1 + C2, 3, 3)
    a = torch.randn(B, C, H, W, generator=g) if xact else None
    gd, wd, ad = gout.to(d), w.to(d), None if a is None else a.to(d)
    res = []
    for off in offs:
        o1, o2 = _out((B, Co1, H, W), off, d), _out((B, Co2, H, W), off, d)
        RF._conv(gd, wd, o1, transposed=True, xact=ad, xact_slope=0.1, out2=o2, what='split dgrad')
        res.append((o1, o2))
    torch.cuda.synchronize()
    gm = gout.double() if a is None else gout.double() * torch.where(a > 0, 1.0, 0.1).double()
    ref = F.conv_transpose2d(gm, w.double(), padding=1)
    return res, (ref[:, :Co1], ref[:, Co1:])


@pytest.mark.parametrize('xact', [False, True], ids=['plain', 'xact'])
@pytest.mark.parametrize('co', [(64, 64), (32, 32), (8, 24)], ids=lambda c: '%d+%d' % c)
@pytest.mark.parametrize('shape', SPLIT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_split_output_vector_epilogue_equals_element_epilogue(shape, co, xact):
    (vec, elem), ref = _split_run(shape, co[0], co[1], xact, (0, 1))
    assert torch.equal(vec[0], elem[0]) and torch.equal(vec[1], elem[1])
    if shape == SPLIT_SHAPES[1]:
        check('split out1', vec[0], ref[0], TOL)
        check('split out2', vec[1], ref[1], TOL)


def test_split_output_off_the_octet_boundary_keeps_the_element_epilogue():
    """Co1 = 20: a group of eight channels would straddle the two outputs, so the launcher must not choose the vector path."""
    (got,), ref = _split_run((2, 64, 10, 40), 20, 12, True, (0,))
    check('split out1 (Co1 = 20)', got[0], ref[0], TOL)
    check('split out2 (Co1 = 20)', got[1], ref[1], TOL)


# ------------------------------------------------------------------------------------------ weight gradient
# (B, C1, C2, Co): profiles/r13_notes.md section 3 (900 tiles of 4 x 32 on 10 x 40: partial on both edges, P = 256), its two-input case, and a
# fourth m-block cut at 24 of 64 rows
WG_SHAPES = [(150, 64, 0, 64), (150, 64, 64, 64), (4, 64, 0, 216)]


@functools.lru_cache(maxsize=None)
def _wgrad_case(shape, act, ps):
    """CPU tensors and the float64 gradients of one case, computed once for the GEMM modes that share it."""
    B, C1, C2, Co = shape
    H, W = 10, 40
    g = _gen('wgrad', shape, act, ps)
    x = torch.randn(B, C1 + C2, H, W, generator=g)
    gout = torch.randn(B, Co, H, W, generator=g)
    a = torch.randn(B, Co, H, W, generator=g) if act else None
    w64 = torch.zeros(Co, C1 + C2, 3, 3, dtype=torch.float64, requires_grad=True)
    b64 = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    gm = gout.double() if a is None else gout.double() * torch.where(a > 0, 1.0, 0.1).double()
    F.conv2d(x.double(), w64, b64, padding=1).backward(gm)
    if ps:   # the stored form of the output gradient and of the saved output
        gout = F.pixel_shuffle(gout, 2)
        a = None if a is None else F.pixel_shuffle(a, 2)
    return x, gout, a, w64.grad, b64.grad


def _wgrad_run(shape, act, ps, mode):
    from realvsr_amd import _lib
    from realvsr_amd import functional as RF
    B, C1, C2, Co = shape
    x, gout, a, gw64, gb64 = _wgrad_case(shape, act, ps)
    d = dev()
    x1 = x[:, :C1].contiguous().to(d)
    x2 = x[:, C1:].contiguous().to(d) if C2 else None
    w = torch.empty(Co, C1 + C2, 3, 3, device=d)
    b = torch.empty(Co, device=d)
    old = _lib.get_gemm_mode()
    _lib.set_gemm_mode(mode)
    try:
        gw, gb = RF._wgrad(x1, gout.to(d), w, b, x2=x2, gact=None if a is None else a.to(d), gact_slope=0.1, pixel_shuffled=ps,
                           what='wgrad store path')
        torch.cuda.synchronize()
    finally:
        _lib.set_gemm_mode(old)
    return gw, gb, gw64, gb64


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16x2', 'bf16'])
@pytest.mark.parametrize('ps', [False, True], ids=['plain', 'ps'])
@pytest.mark.parametrize('act', [False, True], ids=['lin', 'act'])
def test_wgrad_partial_sums_twelve_instantiations(act, ps, mode):
    gw, gb, gw64, gb64 = _wgrad_run(WG_SHAPES[0], act, ps, mode)
    check('grad_weight', gw, gw64, WG_TOLS[mode])
    check('grad_bias', gb, gb64, WG_TOLS[mode])


@pytest.mark.parametrize('shape', WG_SHAPES[1:], ids=lambda s: 'x'.join(map(str, s)))
def test_wgrad_partial_sums_second_input_and_cut_block(shape):
    gw, gb, gw64, gb64 = _wgrad_run(shape, True, False, 'bf16x3')
    check('grad_weight', gw, gw64, WG_TOLS['bf16x3'])
    check('grad_bias', gb, gb64, WG_TOLS['bf16x3'])


# ------------------------------------------------------------------------------------------ zero-insert data gradient
ZI_SHAPES = [(2, 64, 23, 40, 45, 80), (1, 64, 8, 16, 16, 32)]   # gout (B, 64, Hs, Ws) -> gx (B, 64, H, W)


def _zi_run(shape, xact):
    from realvsr_amd import functional as RF
    B, C, Hs, Ws, H, W = shape
    g, d = _gen('zi', shape, xact), dev()
    gout = torch.randn(B, C, Hs, Ws, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) / (3.0 * C ** 0.5)
    a = torch.randn(B, C, Hs, Ws, generator=g) if xact else None
    gx = _out((B, C, H, W), 0, d)
    RF._conv(gout.to(d), w.to(d), gx, transposed=True, xact=None if a is None else a.to(d), xact_slope=0.1, in_mode=1, what='s2 dgrad')
    torch.cuda.synchronize()
    gm = gout.double() if a is None else gout.double() * torch.where(a > 0, 1.0, 0.1).double()
    return gx, F.conv_transpose2d(gm, w.double(), stride=2, padding=1, output_padding=(H - (2 * Hs - 1), W - (2 * Ws - 1)))


@pytest.mark.parametrize('xact', [False, True], ids=['plain', 'xact'])
@pytest.mark.parametrize('shape', ZI_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_zero_insert_data_gradient(shape, xact):
    """The data gradient of a 64 -> 64 stride-2 conv, whose kernel issues no matrix work for the zero rows of the view."""
    gx, ref = _zi_run(shape, xact)
    check('zero-insert dgrad', gx, ref, TOL)
