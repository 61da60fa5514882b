"""The GAN discriminator's operators vs torch CPU float64: 5x5 convolutions (stride 1 / 2, thin first / last layers), the fused
BatchNorm2d + LeakyReLU (train and eval), the BCE-with-logits GAN criterion (vanilla and relativistic).  -m gpu"""
import zlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gpu_util import check, dev, gemm_modes

pytestmark = pytest.mark.gpu
TOLS = {'f32': 2e-5, 'bf16x3': 1e-4}
gemm_mode = gemm_modes()

CONV5 = [
    # C, Co, stride, bias, act, B, H, W
    (1, 16, 1, True, 'lrelu', 2, 24, 32),
    (16, 16, 2, False, 'none', 2, 24, 32),
    (16, 16, 1, False, 'none', 1, 23, 37),
    (64, 64, 2, False, 'none', 1, 48, 48),
    (64, 64, 1, False, 'none', 2, 24, 32),
    (64, 128, 2, False, 'none', 1, 23, 37),
    (128, 256, 1, False, 'none', 1, 24, 32),
    (256, 1, 1, True, 'none', 2, 24, 32),
    (64, 64, 1, True, 'lrelu', 1, 48, 48),
    (16, 16, 2, True, 'lrelu', 1, 23, 37),
]


@pytest.mark.parametrize('case', CONV5, ids=lambda c: '-'.join(str(v) for v in c))
def test_conv5x5_forward_backward(case, gemm_mode):
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    C, Co, stride, bias, act, B, H, W = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    conv = nn.Conv2d(C, Co, 5, stride, 2, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (5.0 * C ** 0.5))
        if bias:
            conv.bias.copy_(torch.randn(Co, generator=g) * 0.1)
    x = torch.randn(B, C, H, W, generator=g)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gout = torch.randn(B, Co, Ho, Wo, generator=g)
    wr = conv.weight.detach().double().requires_grad_(True)
    br = conv.bias.detach().double().requires_grad_(True) if bias else None
    xr = x.double().requires_grad_(True)
    z = F.conv2d(xr, wr, br, stride=stride, padding=2)
    if act == 'lrelu':
        gout = gout * (z.detach().abs() > 1e-3).float()   # away from the kink (the derivative there depends on the last bits)
        yr = F.leaky_relu(z, 0.2)
    else:
        yr = z
    yr.backward(gout.double())

    d = dev()
    conv = conv.to(d)
    xt = x.to(d).requires_grad_(True)
    y = RF.conv2d(xt, conv, RF.ACT_LRELU if act == 'lrelu' else RF.ACT_NONE, 0.2)
    y.backward(gout.to(d))
    torch.cuda.synchronize()
    check('out', y, yr, TOL)
    check('grad_x', xt.grad, xr.grad, TOL)
    check('grad_weight', conv.weight.grad, wr.grad, TOL)
    if bias:
        check('grad_bias', conv.bias.grad, br.grad, TOL)


def test_conv5x5_weight_gradient_is_deterministic():
    from realvsr_amd import functional as RF
    d = dev()
    g = torch.Generator().manual_seed(3)
    for C, Co, stride in ((64, 128, 2), (16, 16, 1), (256, 1, 1)):
        conv = nn.Conv2d(C, Co, 5, stride, 2, bias=True).to(d)
        x = torch.randn(2, C, 48, 48, generator=g).to(d)
        gout = torch.randn(2, Co, 48 // stride, 48 // stride, generator=g).to(d)
        grads = []
        for _ in range(2):
            conv.weight.grad = conv.bias.grad = None
            RF.conv2d(x, conv).backward(gout)
            grads.append((conv.weight.grad.clone(), conv.bias.grad.clone()))
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def _bn_case(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g) * 1.7 + torch.randn(1, C, 1, 1, generator=g) * 3.0
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.3 * torch.randn(C, generator=g))
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_var.copy_(1.0 + 0.2 * torch.rand(C, generator=g))
    gy = torch.randn(B, C, H, W, generator=g)
    return x, bn, gy


# B*HW above 8192 splits every channel into several slices (up to 64 at the option file's shape: B*HW = 1.18 M)
@pytest.mark.parametrize('shape', [(2, 16, 12, 16), (4, 64, 24, 24), (1, 128, 23, 37), (32, 32, 17, 9), (8, 16, 64, 64),
                                   (32, 8, 96, 96)], ids=str)
def test_batchnorm_lrelu_train(shape):
    from realvsr_amd import functional as RF
    x, bn, gy = _bn_case(*shape, seed=sum(shape))
    ref = nn.BatchNorm2d(shape[1]).double()
    ref.load_state_dict(bn.state_dict())
    xr = x.double().requires_grad_(True)
    yr = F.leaky_relu(ref(xr), 0.2)
    yr.backward(gy.double())

    d = dev()
    bn = bn.to(d).train()
    xt = x.to(d).requires_grad_(True)
    y = RF.batch_norm_lrelu(xt, bn, 0.2)
    y.backward(gy.to(d))
    torch.cuda.synchronize()
    check('out', y, yr, 2e-5)
    check('grad_x', xt.grad, xr.grad, 2e-5)
    check('grad_gamma', bn.weight.grad, ref.weight.grad, 2e-5)
    check('grad_beta', bn.bias.grad, ref.bias.grad, 2e-5)
    assert (bn.running_mean.cpu().double() - ref.running_mean).abs().max().item() < 1e-6
    assert (bn.running_var.cpu().double() - ref.running_var).abs().max().item() < 1e-6
    assert int(bn.num_batches_tracked) == 1 == int(ref.num_batches_tracked)


def test_batchnorm_lrelu_eval():
    from realvsr_amd import functional as RF
    x, bn, gy = _bn_case(2, 32, 20, 28, seed=9)
    ref = nn.BatchNorm2d(32).double()
    ref.load_state_dict(bn.state_dict())
    ref.eval()
    xr = x.double().requires_grad_(True)
    yr = F.leaky_relu(ref(xr), 0.2)
    yr.backward(gy.double())
    d = dev()
    bn = bn.to(d).eval()
    rm0 = bn.running_mean.clone()
    xt = x.to(d).requires_grad_(True)
    y = RF.batch_norm_lrelu(xt, bn, 0.2)
    y.backward(gy.to(d))
    torch.cuda.synchronize()
    check('out', y, yr, 2e-5)
    check('grad_x', xt.grad, xr.grad, 2e-5)
    check('grad_gamma', bn.weight.grad, ref.weight.grad, 2e-5)
    assert torch.equal(bn.running_mean, rm0) and int(bn.num_batches_tracked) == 0


def test_batchnorm_lrelu_backward_is_deterministic():
    from realvsr_amd import functional as RF
    x, bn, gy = _bn_case(8, 64, 48, 48, seed=4)
    d = dev()
    bn = bn.to(d)
    x, gy = x.to(d), gy.to(d)
    outs = []
    for _ in range(2):
        xt = x.clone().requires_grad_(True)
        bn.weight.grad = bn.bias.grad = None
        y = RF.batch_norm_lrelu(xt, bn, 0.2)
        y.backward(gy)
        outs.append((y.detach().clone(), xt.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('relativistic', [False, True])
@pytest.mark.parametrize('target', [1.0, 0.0])
def test_gan_criterion(relativistic, target):
    from realvsr_amd.loss import GANLoss
    g = torch.Generator().manual_seed(int(relativistic) * 2 + int(target))
    a = torch.randn(4, 1, 23, 29, generator=g) * 6.0            # large logits: the stable form matters
    b = torch.randn(4, 1, 23, 29, generator=g) * 3.0 + 1.0
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    z = ar - torch.mean(br) if relativistic else ar
    lr = F.binary_cross_entropy_with_logits(z, torch.full_like(z, target))
    (0.7 * lr).backward()
    d = dev()
    at, bt = a.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    crit = GANLoss('ragan' if relativistic else 'gan', 1.0, 0.0)
    l = crit(at, target == 1.0, other=bt if relativistic else None)
    (0.7 * l).backward()
    torch.cuda.synchronize()
    check('loss', l, lr, 2e-6)
    check('grad_a', at.grad, ar.grad, 2e-5)
    if relativistic:
        check('grad_b', bt.grad, br.grad, 2e-5)
    else:
        assert bt.grad is None


def test_conv5x5_runs_on_the_bf16_matrix_cores_outside_f32_mode():
    """The default mode takes the bf16x3 kernels at KS = 5 (packed 25-tap weight image, conv_fwd2 / conv_wgrad5): a weight image exists,
    and forward, data gradient and weight gradient differ in their last bits from the exact-f32 kernels (both within TOLS of float64)."""
    import ctypes
    from realvsr_amd import _lib
    from realvsr_amd import functional as RF
    d = dev()
    L = _lib.lib()
    for Co, C in ((64, 64), (1, 256), (16, 1)):
        w = torch.randn(Co, C, 5, 5, device=d)
        for w_mode, (cin, cout) in ((0, (C, Co)), (1, (Co, C))):    # forward image; data-gradient image (transposed, flipped)
            nbytes = L.rvsr_conv2d_forward_workspace_bytes(cin, 0, cout, 5)
            buf = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=d)
            got = L.rvsr_conv2d_pack_weights(ctypes.c_void_p(w.data_ptr()), cin, cout, 5, w_mode, ctypes.c_void_p(buf.data_ptr()),
                                             buf.numel(), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert nbytes > 0 and got == nbytes
    g = torch.Generator().manual_seed(11)
    conv = nn.Conv2d(64, 64, 5, 1, 2, bias=True).to(d)
    x = torch.randn(2, 64, 24, 32, generator=g).to(d)
    gout = torch.randn(2, 64, 24, 32, generator=g).to(d)
    old = _lib.get_gemm_mode()
    res = {}
    try:
        for mode in ('f32', 'bf16x3'):
            _lib.set_gemm_mode(mode)
            conv.weight.grad = conv.bias.grad = None
            xt = x.clone().requires_grad_(True)
            y = RF.conv2d(xt, conv)
            y.backward(gout)
            res[mode] = (y.detach().clone(), xt.grad.clone(), conv.weight.grad.clone())
    finally:
        _lib.set_gemm_mode(old)
    for a, b in zip(res['f32'], res['bf16x3']):
        assert not torch.equal(a, b)
        assert ((a - b).abs().max() / a.abs().max()).item() < 1e-4
