"""conv_cat_bcast with conv_b's partial as a periodic addend of conv_a's epilogue (rvsr_conv2d_forward_addend, functional._FUSE_BCAST_ADDEND)
against the composed path -- conv_a, conv_b, rvsr_bcast_add_act -- on the same tensors.  -m gpu

The claim is equality of bits, not closeness: the fused epilogue rounds conv + bias to float32 before the partial joins, as the composed
path does by storing it, and applies the same activation expression afterwards; the backward is the same code on the same saved output.
So the output and all four gradients must satisfy torch.equal."""
import pytest
import torch
import torch.nn as nn

from gpu_util import dev

pytestmark = pytest.mark.gpu


def _run(fuse, shape, act, mode, seed=0):
    """Output and gradients (x, ref, weight, bias) of conv_cat_bcast with the fused route on or off; also whether conv_a ran fused."""
    from realvsr_amd import _lib
    from realvsr_amd import functional as RF
    N, B, C1, C2, Co, H, W = shape
    d = dev()
    gen = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(C1 + C2, Co, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * 0.05)
        conv.bias.copy_(torch.randn(Co, generator=gen) * 0.1)
    conv = conv.to(d)
    x = torch.randn(N * B, C1, H, W, generator=gen).to(d).requires_grad_(True)
    ref = torch.randn(B, C2, H, W, generator=gen).to(d).requires_grad_(True)
    gout = torch.randn(N * B, Co, H, W, generator=gen).to(d)
    fused_calls = []
    orig, old_switch, old_mode = RF._conv, RF._FUSE_BCAST_ADDEND, _lib.get_gemm_mode()

    def conv_spy(*a, **kw):
        ran = orig(*a, **kw)
        if kw.get('addend_period'):
            fused_calls.append(bool(ran))
        return ran
    RF._conv, RF._FUSE_BCAST_ADDEND = conv_spy, fuse
    _lib.set_gemm_mode(mode)
    try:
        y = RF.conv_cat_bcast(x, ref, conv, N, act, 0.1)
        y.backward(gout)
        torch.cuda.synchronize()
    finally:
        RF._conv, RF._FUSE_BCAST_ADDEND = orig, old_switch
        _lib.set_gemm_mode(old_mode)
    return [y.detach(), x.grad, ref.grad, conv.weight.grad, conv.bias.grad], fused_calls


def _compare(shape, act, mode, granted):
    got, attempts = _run(True, shape, act, mode)
    want, none = _run(False, shape, act, mode)
    assert none == [] and attempts == [granted], (attempts, granted)      # one attempt, granted or refused as the plan says
    for name, a, b in zip(('out', 'gx', 'gref', 'gw', 'gb'), got, want):
        assert torch.equal(a, b), '%s: %d of %d elements differ, max |diff| %.3e' % (name, int((a != b).sum()), a.numel(),
                                                                                    float((a - b).abs().max()))


# (N, B, C1, C2, Co, H, W): one 8 x 64 tile, 2 x 2 tiles, and 9 rows -- a second tile row with one live row
SHAPES = [(3, 2, 64, 64, 64, 8, 64), (3, 2, 64, 64, 64, 16, 128), (3, 2, 64, 64, 64, 9, 64)]


@pytest.mark.parametrize('mode', ['bf16x3', 'f32', 'bf16x2', 'bf16'])
@pytest.mark.parametrize('act', [0, 1, 2], ids=['none', 'relu', 'lrelu'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_fused_addend_equals_the_composed_path(shape, act, mode):
    """Every GEMM mode: the split modes run the fused epilogue with their own term count, exact f32 has none and falls back."""
    _compare(shape, act, mode, granted=mode != 'f32')


def test_fused_addend_with_a_cut_m_block():
    """Co = 216 (the DCN offset convs' width): the fourth 64-row m-block holds 24 live channels."""
    _compare((2, 2, 64, 64, 216, 8, 64), 2, 'bf16x3', granted=True)


@pytest.mark.parametrize('shape', [(3, 2, 64, 64, 32, 8, 64), (3, 2, 64, 64, 64, 8, 62)], ids=['Co=32', 'W=62'])
def test_refused_sites_fall_back(shape):
    """32 output channels (32-row m-blocks) and W % 4 != 0 (element stores) have no such epilogue: one refused attempt, then today's three
    calls, and the same bits."""
    _compare(shape, 2, 'bf16x3', granted=False)
