"""The (3,1,1) temporal convolution of FSTRN (RF.tconv3, csrc/conv3d_kernels.hip) against float64 CPU F.conv3d, in both GEMM modes at the
tolerances of test_gpu_conv.py: out, the fused PReLU output, every gradient, the transposed mode, run-to-run identity of the weight
gradient, and the fused kernel against the path composed from 1x1 convolutions.  -m gpu"""
import ctypes
import zlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gpu_util import check, dev, gemm_modes
from test_gpu_conv import TOLS, _at_offset

pytestmark = pytest.mark.gpu
gemm_mode = gemm_modes()

# T, B, Ci, Co, H, W, residual, slope of the second output (None: no second output)
CASES = [
    (3, 2, 64, 64, 8, 16, True, 0.25),      # the network's block: one work item per batch element
    (1, 1, 64, 64, 8, 16, True, -0.7),      # T = 1: both neighbours out of range
    (2, 1, 32, 32, 20, 36, False, None),    # T = 2: no frame has both neighbours; 6 work items, the last one partly filled
    (5, 1, 32, 32, 13, 22, True, 0.0),      # H * W % 4 != 0: the scalar path; frames travel ahead of the walk (T > 3)
    (3, 2, 16, 48, 9, 70, True, 1.0),       # ragged tiles off the vector path, one k-step, a partial m-tile
    (3, 1, 48, 16, 20, 36, True, -0.7),     # three k-steps, half an m-tile (the data gradient of the case above and back)
    (5, 2, 20, 12, 8, 16, True, 0.3),       # fused or composed, whichever the plan says: partial k-step and m-tile
    (3, 1, 64, 64, 13, 22, False, 0.25),    # 64 x 64 on the scalar path
    (2, 2, 64, 64, 9, 70, True, None),
    (5, 2, 64, 64, 20, 36, False, None),
    # 2 x 1030 = 2060 work items on the 1024 workgroups the plan caps the grid at: every workgroup walks two or three items with one weight
    # image; the last tile of a frame holds 56 pixels (two waves leave the walk's body at once, one is partly filled); the 16-byte path
    (2, 2, 16, 16, 364, 362, True, 0.25),
]
TC_SLOTS = 1024   # csrc/conv3d_plan.h


def _ref_tconv(s, w, b, res):
    """s, res: [T, B, C, H, W] float64; the reference's nn.Conv3d on [B, C, T, H, W]."""
    y = F.conv3d(s.permute(1, 2, 0, 3, 4), w, b, padding=(1, 0, 0)).permute(2, 0, 1, 3, 4)
    return y if res is None else y + res


def _make(case):
    T, B, Ci, Co, H, W, use_res, slope = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()) % 2 ** 31)
    conv = nn.Conv3d(Ci, Co, (3, 1, 1), padding=(1, 0, 0))
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3.0 * Ci) ** 0.5)
        conv.bias.copy_(torch.randn(Co, generator=g) * 0.1)
    s = torch.randn(T, B, Ci, H, W, generator=g)
    res = torch.randn(T, B, Co, H, W, generator=g) if use_res else None
    gout = torch.randn(T, B, Co, H, W, generator=g)
    # (mean 1: the slope gradient, sum gpout * out * [out <= 0], is then a sum of mostly like-signed terms.  With a zero-mean gpout its
    # ~10^4 .. 10^5 terms cancel to about 1 / sqrt(n) of their absolute sum, and the relative error of that remainder measures the
    # cancellation -- 2e-3 was seen for a 3e-6 error of `out` -- not the kernel.)
    gpout = 1.0 + torch.randn(T, B, Co, H, W, generator=g)
    act = None
    if slope is not None:
        act = nn.PReLU()
        with torch.no_grad():
            act.weight.fill_(slope)
    return conv, act, s, res, gout, gpout


def _run_case(case, gemm_mode, offsets=(0, 0, 0)):
    """offsets: float offsets of s, the output gradients and the residual from a 16-byte boundary."""
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    conv, act, s, res, gout, gpout = _make(case)
    # float64 CPU reference
    sr = s.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if res is not None else None
    wr, br = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    yr = _ref_tconv(sr, wr, br, rr)
    if act is not None:
        ar = act.weight.detach().double().requires_grad_(True)
        # the kink rule of test_gpu_conv.py: no gradient through the PReLU where the exact pre-activation is within 1e-3 of zero
        gpout = gpout * (yr.detach().abs() > 1e-3).float()
        pr = torch.where(yr > 0, yr, ar * yr)
        torch.autograd.backward([yr, pr], [gout.double(), gpout.double()])
    else:
        yr.backward(gout.double())

    d = dev()
    conv = conv.to(d)
    act = act.to(d) if act is not None else None
    sd, rd = _at_offset(s, offsets[0], d), _at_offset(res, offsets[2], d)
    y = RF.tconv3(sd, conv, residual=rd, prelu_mod=act)
    if act is not None:
        y, pout = y
        torch.autograd.backward([y, pout], [_at_offset(gout, offsets[1], d, leaf=False), _at_offset(gpout, offsets[1], d, leaf=False)])
    else:
        y.backward(_at_offset(gout, offsets[1], d, leaf=False))
    torch.cuda.synchronize()
    check('out', y, yr, TOL)
    if act is not None:
        check('pout', pout, pr, TOL)
        check('grad_slope', act.weight.grad, ar.grad, TOL)
    check('grad_s', sd.grad, sr.grad, TOL)
    if res is not None:
        check('grad_res', rd.grad, rr.grad, TOL)
    check('grad_weight', conv.weight.grad, wr.grad, TOL)
    check('grad_bias', conv.bias.grad, br.grad, TOL)
    return y.detach(), sd.grad.detach(), conv.weight.grad.detach().clone()


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_tconv3_forward_backward(case, gemm_mode):
    _run_case(case, gemm_mode)


@pytest.mark.parametrize('offsets', [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], ids=lambda o: 'off%d%d%d' % o)
def test_tconv3_off_a_16_byte_boundary(offsets, gemm_mode):
    """Input, output gradients and residual 4 bytes behind a 16-byte boundary: the plan takes the scalar path for that call."""
    _run_case(CASES[0], gemm_mode, offsets)


def test_the_fused_kernel_takes_the_network_shapes():
    """No quiet fallback: the plan grants every channel count the network and these tests use, on device addresses."""
    from realvsr_amd import _lib
    L = _lib.lib()
    t = torch.zeros(64, device=dev())
    a = ctypes.c_void_p(t.data_ptr())
    for case in CASES:
        T, B, Ci, Co, H, W = case[:6]
        vec, grid = ctypes.c_int(-1), ctypes.c_int(-1)
        assert L.rvsr_tconv3_plan(T, B, Ci, Co, H, W, a, a, a, a, ctypes.byref(vec), ctypes.byref(grid)) == 0, case
        assert vec.value == int(H * W % 4 == 0), case
        # one workgroup per work item (128 pixels of one batch element) up to the cap; beyond it the workgroups walk
        items = B * ((H * W + 127) // 128)
        assert grid.value == (TC_SLOTS if case[:6] == (2, 2, 16, 16, 364, 362) else items), (case, grid.value, items)
    assert sum(1 for c in CASES if c[1] * ((c[4] * c[5] + 127) // 128) > TC_SLOTS) == 1


@pytest.mark.parametrize('case', [CASES[0], CASES[3], CASES[4], CASES[6]], ids=lambda c: '-'.join(str(v) for v in c))
def test_tconv3_transposed_mode(case, gemm_mode):
    """transposed: the weight read as [ci, co, 2 - dt] -- the data gradient, with a fused residual (in-place accumulation included)."""
    from realvsr_amd import _lib, functional as RF
    TOL = TOLS[gemm_mode]
    conv, _, s, _, gout, acc = _make(case)
    sr = s.double().requires_grad_(True)
    _ref_tconv(sr, conv.weight.detach().double(), None, None).backward(gout.double())
    d = dev()
    w, g = conv.weight.detach().to(d), gout.to(d)
    gs, none = RF._tconv3_run(g, w, transposed=True)
    assert none is None
    check('transposed', gs, sr.grad, TOL)
    buf = torch.randn(s.shape, generator=torch.Generator().manual_seed(3))
    into = buf.to(d)
    out, _ = RF._tconv3_run(g, w, residual=into, transposed=True)
    check('transposed + residual', out, sr.grad + buf.double(), TOL)
    # the residual may be the output buffer itself
    T, B, Ci, Co, H, W = case[:6]
    _lib.check(_lib.lib().rvsr_tconv3_forward(_lib._p(g), _lib._p(w), None, _lib._p(into), None, _lib._p(into), None, T, B, Co, Ci, H, W, 1,
                                              _lib._stream()), 'tconv3 in place')
    assert torch.equal(into, out)


@pytest.mark.parametrize('case', [CASES[0], CASES[3], CASES[4], CASES[6]], ids=lambda c: '-'.join(str(v) for v in c))
def test_fused_against_composed(case, gemm_mode, monkeypatch):
    """The fused kernel and the operator composed from three 1x1 convolutions over frame ranges (_FUSE_TCONV3 off) agree within the
    tolerance each is held to against float64."""
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    y1, gs1, gw1 = _run_case(case, gemm_mode)
    monkeypatch.setattr(RF, '_FUSE_TCONV3', False)
    y0, gs0, gw0 = _run_case(case, gemm_mode)
    check('out fused vs composed', y1, y0, TOL)
    check('grad_s fused vs composed', gs1, gs0, TOL)
    check('grad_weight fused vs composed', gw1, gw0, TOL)


def test_weight_gradient_is_bit_identical_over_repeats(gemm_mode):
    from realvsr_amd import functional as RF
    conv, act, s, res, gout, gpout = _make(CASES[0])
    d = dev()
    conv, act, s, res, gout, gpout = conv.to(d), act.to(d), s.to(d), res.to(d), gout.to(d), gpout.to(d)
    got = []
    for _ in range(5):
        for p in (*conv.parameters(), *act.parameters()):
            p.grad = None
        y, pout = RF.tconv3(s, conv, residual=res, prelu_mod=act)
        torch.autograd.backward([y, pout], [gout, gpout])
        got.append([t.detach().clone() for t in (y, pout, conv.weight.grad, conv.bias.grad, act.weight.grad)])
    for rep in got[1:]:
        for a, b in zip(got[0], rep):
            assert torch.equal(a, b)
