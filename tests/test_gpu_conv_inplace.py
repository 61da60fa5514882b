"""rvsr_conv2d_forward with `residual` being `out1` itself -- the in-place accumulation of the GradSink owners and depositors, of
conv3d_frames' outer taps and of tsa_temporal_block's data gradients -- per kernel variant that can carry a residual.  -m gpu

Each case runs twice through functional._conv on the same inputs: with the residual r in a buffer of its own into a fresh output, and
into a buffer that holds r and is passed as both `residual` and `out1`.  The kernels are deterministic, so the two outputs are equal
bit for bit unless a lane reads a residual element that another lane has already stored; the first run is held to float64 at
TOLS[mode] of test_gpu_conv.py.

A case is (C1, C2, Co, k, stride, transposed, xact, B, H, W, x_off, out_off): the offsets are floats from a 16-byte boundary of the
inputs (x1, x2, xact) and of the residual + output.  The first block is the smallest shape found for each key (forward kernel,
16-byte stores, output off the boundary) of tests/test_conv_ledger_host.py::test_every_residual_epilogue_runs_in_place, in bf16x3
or in f32 mode; the second block repeats one variant per kernel family on several workgroups with a ragged last tile in both
directions, since aliasing goes wrong across tiles rather than inside one."""
import zlib

import pytest
import torch
import torch.nn.functional as F

import conv_ledger as CL
from gpu_util import check, dev, gemm_modes
from test_gpu_conv import SENTINEL, TOLS, _border_untouched, _padded

pytestmark = pytest.mark.gpu
gemm_mode = gemm_modes()
SLOPE = 0.1

INPLACE_CASES = [
    # ---- one per key
    # 3 -> 1 channel: the 32-row m-block of conv_fwd2 (1x1, stride 2) and conv_fwd5, element and 16-byte stores, with act' on the input
    (3, 0, 1, 1, 1, False, False, 1, 4, 7, 0, 0), (3, 0, 1, 1, 1, False, False, 1, 4, 7, 0, 1), (3, 0, 1, 1, 1, False, False, 1, 4, 12, 0, 0),
    (3, 0, 1, 3, 2, False, False, 1, 4, 7, 0, 0), (3, 0, 1, 3, 2, False, False, 1, 4, 7, 0, 1), (3, 0, 1, 3, 2, False, False, 1, 4, 12, 0, 0),
    (3, 0, 1, 3, 1, False, False, 1, 4, 7, 0, 0), (3, 0, 1, 3, 1, False, False, 1, 4, 7, 0, 1), (3, 0, 1, 3, 1, False, True, 1, 4, 7, 0, 0),
    (3, 0, 1, 3, 1, False, False, 1, 4, 12, 0, 0), (3, 0, 1, 3, 1, False, False, 1, 4, 12, 0, 1), (3, 0, 1, 3, 1, False, False, 1, 4, 12, 1, 0),
    (3, 0, 1, 3, 1, False, True, 1, 4, 12, 0, 0),
    # the vector-ALU kernel (8 channels in, at most 4 out)
    (8, 0, 1, 3, 1, False, False, 1, 4, 12, 0, 0),
    # a concat off the chunk: the exact-f32 kernel in bf16x3 mode, 32-, 64- and 128-row m-blocks
    (3, 16, 1, 1, 1, False, False, 1, 4, 7, 0, 0), (3, 16, 1, 1, 1, False, False, 1, 4, 7, 0, 1), (3, 16, 1, 3, 2, False, False, 1, 4, 7, 0, 0),
    (3, 16, 1, 3, 2, False, False, 1, 4, 7, 0, 1), (3, 16, 1, 3, 1, False, False, 1, 4, 7, 0, 0), (3, 16, 1, 3, 1, False, False, 1, 4, 7, 0, 1),
    (3, 16, 64, 1, 1, False, False, 1, 4, 7, 0, 0), (3, 16, 64, 1, 1, False, False, 1, 4, 7, 0, 1), (3, 16, 64, 3, 2, False, False, 1, 4, 7, 0, 0),
    (3, 16, 64, 3, 2, False, False, 1, 4, 7, 0, 1), (3, 16, 64, 3, 1, False, False, 1, 4, 7, 0, 0), (3, 16, 64, 3, 1, False, False, 1, 4, 7, 0, 1),
    (3, 16, 80, 1, 1, False, False, 1, 4, 7, 0, 0), (3, 16, 80, 1, 1, False, False, 1, 4, 7, 0, 1), (3, 16, 80, 3, 2, False, False, 1, 4, 7, 0, 0),
    (3, 16, 80, 3, 2, False, False, 1, 4, 7, 0, 1), (3, 16, 80, 3, 1, False, False, 1, 4, 7, 0, 0), (3, 16, 80, 3, 1, False, False, 1, 4, 7, 0, 1),
    # 64 output channels: the 64-row m-block of conv_fwd2 and conv_fwd5 (the exact-f32 kernel in f32 mode), the 8 x 64 tile
    (3, 0, 64, 1, 1, False, False, 1, 4, 7, 0, 0), (3, 0, 64, 1, 1, False, False, 1, 4, 7, 0, 1), (3, 0, 64, 1, 1, False, False, 1, 4, 12, 0, 0),
    (3, 0, 64, 3, 2, False, False, 1, 4, 7, 0, 0), (3, 0, 64, 3, 2, False, False, 1, 4, 7, 0, 1), (3, 0, 64, 3, 2, False, False, 1, 4, 12, 0, 0),
    (3, 0, 64, 3, 1, False, False, 1, 4, 7, 0, 0), (3, 0, 64, 3, 1, False, False, 1, 4, 7, 0, 1), (3, 0, 64, 3, 1, False, True, 1, 4, 7, 0, 0),
    (3, 0, 64, 3, 1, False, False, 1, 4, 12, 0, 0), (3, 0, 64, 3, 1, False, False, 1, 4, 12, 0, 1), (3, 0, 64, 3, 1, False, False, 1, 4, 12, 1, 0),
    (3, 0, 64, 3, 1, False, False, 1, 9, 12, 0, 0), (3, 0, 64, 3, 1, False, True, 1, 9, 12, 0, 0),
    # 80 output channels: the 128-row m-block of the exact-f32 kernel in f32 mode
    (3, 0, 80, 1, 1, False, False, 1, 4, 7, 0, 0), (3, 0, 80, 1, 1, False, False, 1, 4, 7, 0, 1), (3, 0, 80, 3, 2, False, False, 1, 4, 7, 0, 0),
    (3, 0, 80, 3, 2, False, False, 1, 4, 7, 0, 1), (3, 0, 80, 3, 1, False, False, 1, 4, 7, 0, 0), (3, 0, 80, 3, 1, False, False, 1, 4, 7, 0, 1),
    # ---- several workgroups, ragged last tiles: the calls of the in-place callers (data gradients: transposed weights)
    (64, 0, 64, 3, 1, True, True, 2, 17, 72, 0, 0),       # conv_fwd5, 16-byte stores (res_block dgrad1, a GradSink owner)
    (16, 0, 16, 3, 1, True, False, 2, 19, 70, 0, 1),      # conv_fwd5, element stores, off the boundary (tsa dgrad into the centre block)
    (16, 0, 3, 3, 1, True, False, 3, 19, 35, 1, 1),       # 665-float frames of three channels: x and out off, as in conv3d_frames
    (64, 0, 64, 1, 1, False, False, 2, 17, 72, 0, 0),     # conv_fwd2 1x1, 16-byte stores (tconv3 composed, conv3d_frames k = 1)
    (24, 0, 16, 1, 1, True, False, 2, 19, 70, 0, 1),      # conv_fwd2 1x1, element stores (conv_transpose1x1's forward)
    (16, 0, 24, 3, 2, False, False, 2, 35, 70, 0, 0),     # conv_fwd2 stride 2 (a stride-2 GradSink pair is test_gpu_conv_smallk's)
    (3, 16, 80, 3, 1, False, False, 2, 17, 70, 0, 1),     # the exact-f32 kernel, two m-blocks
    (8, 0, 4, 3, 1, False, False, 2, 17, 130, 0, 0),      # the vector-ALU kernel, two column tiles
]


def _id(case):
    return '-'.join(str(int(v)) for v in case)


def _holds(r, off, d):
    """(buffer, view): a device buffer that holds `r`, `off` floats behind a 16-byte boundary, sentinels around it -- what the in-place
    run gets as both residual and output."""
    return _padded(r, off, d)


@pytest.mark.parametrize('case', INPLACE_CASES, ids=_id)
def test_residual_may_be_the_output(case, gemm_mode):
    from realvsr_amd import functional as RF
    C1, C2, Co, k, stride, transposed, xact, B, H, W, x_off, out_off = case
    Ho, Wo = CL.out_size(H, W, k, stride)
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()) % 2 ** 31)
    Cin = C1 + C2
    x1 = torch.randn(B, C1, H, W, generator=g)
    x2 = torch.randn(B, C2, H, W, generator=g) if C2 else None
    xa = torch.randn(B, C1, H, W, generator=g) if xact else None
    w = torch.randn((Cin, Co, k, k) if transposed else (Co, Cin, k, k), generator=g) / (k * Cin ** 0.5)
    bias = torch.randn(Co, generator=g) * 0.1
    r = torch.randn(B, Co, Ho, Wo, generator=g)

    xin = x1.double() if xa is None else x1.double() * torch.where(xa.double() > 0, 1.0, SLOPE)
    xin = xin if x2 is None else torch.cat([xin, x2.double()], 1)
    weff = w.double().transpose(0, 1).flip(2, 3) if transposed else w.double()
    ref = F.conv2d(xin, weff, bias.double(), stride=stride, padding=k // 2) + r.double()

    d = dev()
    ins = [None if t is None else _padded(t, x_off, d)[1] for t in (x1, x2, xa)]
    wd, bd = w.to(d), bias.to(d)
    kw = dict(x2=ins[1], xact=ins[2], xact_slope=SLOPE, bias=bd, stride=stride, transposed=transposed)
    _, r_own = _padded(r, out_off, d)
    fresh_buf, fresh = _padded(torch.full(r.shape, SENTINEL), out_off, d)
    RF._conv(ins[0], wd, fresh, residual=r_own, what='own residual', **kw)
    both_buf, both = _holds(r, out_off, d)
    assert CL.fwd_call_of_args(ins[0], wd, both, residual=both, **kw) == CL.inplace_call(case)   # (the call the ledger test keys)
    RF._conv(ins[0], wd, both, residual=both, what='in place', **kw)
    torch.cuda.synchronize()
    assert torch.equal(r_own.cpu(), r), 'the residual was written'
    assert _border_untouched(fresh_buf, out_off, fresh.numel()) and _border_untouched(both_buf, out_off, both.numel())
    differ = int((fresh != both).sum())
    assert differ == 0, 'in place differs from out of place at %d of %d elements' % (differ, both.numel())
    check('out', fresh, ref, TOLS[gemm_mode])
