"""The fused channel-attention operator (csrc/ca_kernels.hip, functional.channel_attention / rcab) against the same formulae written
from torch ops in float64 on the CPU.  -m gpu

The operator has no matrix-core path, so it meets the exact-f32 tolerances of test_gpu_net.py (5e-5 outputs, 3e-4 gradients, through
gpu_util.check: maximum and L2) in every GEMM mode; each case runs under 'f32' and 'bf16x3'.  Inputs: u = randn + a per-channel offset,
1x1 weights randn, biases 0.1 * randn -- the gates span nearly (0, 1) and half the hidden units are zero.  The shapes are the smallest
that reach each path of the kernels: scalar / 16-byte loads, a plane below one wave, Cr = 1 and 3, C not a multiple of 64, several
slices per plane, and a view that starts 4 bytes into its buffer."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_util import check, dev, gemm_modes
from test_gpu_net import TOLS, gcheck

gemm_mode = gemm_modes()
pytestmark = pytest.mark.gpu
TOL, TOL_G = 5e-5, 3e-4

#          B,  C,  r, H,  W,   offset view
SHAPES = {'scalar_odd': (2, 64, 16, 7, 13, False),
          'subwave_cr3': (3, 48, 16, 3, 5, False),
          'one_pixel_cr1': (1, 16, 16, 1, 1, False),
          'vector': (2, 64, 16, 8, 16, False),
          'sliced': (1, 16, 16, 96, 160, False),
          'offset_view': (2, 64, 16, 8, 16, True)}
# (one_pixel_cr1: a seed whose single hidden unit is alive -- with the unit dead the whole small-matrix backward is zero)
SEEDS = {'scalar_odd': 102, 'subwave_cr3': 104, 'one_pixel_cr1': 107, 'vector': 105, 'sliced': 103, 'offset_view': 100}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Seeded CPU inputs of a shape, made once and never written."""
    B, C, r, H, W, _ = SHAPES[name]
    Cr = C // r
    gen = torch.Generator().manual_seed(SEEDS[name])
    rn = lambda *s: torch.randn(*s, generator=gen)
    return dict(u=rn(B, C, H, W) + rn(1, C, 1, 1), x=rn(B, C, H, W), g=rn(B, C, H, W), w1=rn(Cr, C, 1, 1), b1=0.1 * rn(Cr),
                w2=rn(C, Cr, 1, 1), b2=0.1 * rn(C))


@functools.lru_cache(maxsize=None)
def _reference(name, with_x, res_scale):
    """The formulae of include/realvsr_hip.h section 8 in float64 under autograd."""
    t = {k: v.double().requires_grad_(k != 'g') for k, v in _inputs(name).items()}
    s = t['u'].mean((2, 3), keepdim=True)
    z = F.relu(F.conv2d(s, t['w1'], t['b1']))
    a = torch.sigmoid(F.conv2d(z, t['w2'], t['b2']))
    out = res_scale * t['u'] * a
    if with_x:
        out = out + t['x']
    out.backward(t['g'])
    ref = dict(out=out.detach(), pooled=s.detach().flatten(1), hidden=z.detach().flatten(1), gate=a.detach().flatten(1),
               gu=t['u'].grad, gw1=t['w1'].grad, gb1=t['b1'].grad, gw2=t['w2'].grad, gb2=t['b2'].grad)
    ref['gx'] = t['x'].grad if with_x else None
    ref['bcast'] = ref['gu'] - res_scale * a.detach() * t['g']     # gs, broadcast over the plane
    return ref


def _device_inputs(name):
    d = dev()
    t = {k: v.to(d) for k, v in _inputs(name).items()}
    if SHAPES[name][5]:    # u as a view that starts 4 bytes into its buffer: contiguous, but not 16-byte aligned
        buf = torch.empty(t['u'].numel() + 1, device=d)
        buf[1:].copy_(t['u'].flatten())
        t['u'] = buf[1:].view_as(t['u'])
        assert t['u'].is_contiguous() and t['u'].data_ptr() % 16 == 4
    return t


def _convs(t):
    Cr, C = t['w1'].shape[:2]
    down, up = torch.nn.Conv2d(C, Cr, 1).to(dev()), torch.nn.Conv2d(Cr, C, 1).to(dev())
    with torch.no_grad():
        for p, k in ((down.weight, 'w1'), (down.bias, 'b1'), (up.weight, 'w2'), (up.bias, 'b2')):
            p.copy_(t[k])
    return down, up


@pytest.mark.parametrize('res_scale', [1.0, 0.5])
@pytest.mark.parametrize('with_x', [True, False])
@pytest.mark.parametrize('name', list(SHAPES))
def test_channel_attention_vs_float64(gemm_mode, name, with_x, res_scale):
    from realvsr_amd import functional as RF
    from realvsr_amd import _lib
    B, C, r, H, W, _ = SHAPES[name]
    ref = _reference(name, with_x, res_scale)
    t = _device_inputs(name)
    # the plan takes the path the case is named for
    s_, v_ = ctypes.c_int(), ctypes.c_int()
    x_ptr = _lib._p(t['x']) if with_x else None
    assert _lib.lib().rvsr_channel_attention_plan(B, C, H, W, _lib._p(t['u']), x_ptr, _lib._p(t['g']), ctypes.byref(s_), ctypes.byref(v_)) == 0
    assert v_.value == int(name in ('vector', 'sliced')) and (s_.value > 1) == (name == 'sliced')
    # ---- the saved statistics, through the raw call
    out, pooled, hidden, gate = RF._ca_forward(t['u'], t['x'] if with_x else None, t['w1'], t['b1'], t['w2'], t['b2'], res_scale)
    check('out', out, ref['out'], TOL)
    check('pooled', pooled, ref['pooled'], TOL)
    check('hidden', hidden, ref['hidden'], TOL)
    check('gate', gate, ref['gate'], TOL)
    # ---- the autograd node
    down, up = _convs(t)
    u = t['u'].detach().requires_grad_(True)
    x = t['x'].detach().requires_grad_(True) if with_x else None
    y = RF.channel_attention(u, down, up, x=x, res_scale=res_scale)
    assert torch.equal(y, out)
    y.backward(t['g'])
    check('gu', u.grad, ref['gu'], TOL_G)
    if with_x:
        assert torch.equal(x.grad, t['g'])
    for got, k in ((down.weight.grad, 'gw1'), (down.bias.grad, 'gb1'), (up.weight.grad, 'gw2'), (up.bias.grad, 'gb2')):
        check(k, got, ref[k], TOL_G)
    # the broadcast term of gu on its own, relative to ITS maximum (a few percent of gu's: a wrong 1 / (H * W) or a dropped ReLU mask
    # would pass the whole-tensor check above)
    bcast = u.grad.double().cpu() - res_scale * gate.double().cpu().view(B, C, 1, 1) * _inputs(name)['g'].double()
    print('broadcast term: max %.3e of gu max %.3e' % (ref['bcast'].abs().max().item(), ref['gu'].abs().max().item()))
    check('gu - res_scale * a * g', bcast, ref['bcast'], TOL_G)


@pytest.mark.parametrize('name', ['scalar_odd', 'sliced'])
def test_parameter_gradient_pointers_may_be_null(name):
    """needs_input_grad: frozen parameters leave their gradient pointers NULL; the others and gu are what they were."""
    from realvsr_amd import functional as RF
    ref = _reference(name, True, 0.5)
    t = _device_inputs(name)
    for frozen in (('w1', 'b2'), ('b1', 'w2'), ('w1', 'b1', 'w2', 'b2')):
        down, up = _convs(t)
        params = {'w1': down.weight, 'b1': down.bias, 'w2': up.weight, 'b2': up.bias}
        for k in frozen:
            params[k].requires_grad_(False)
        u = t['u'].detach().requires_grad_(True)
        RF.channel_attention(u, down, up, x=t['x'], res_scale=0.5).backward(t['g'])
        check('gu', u.grad, ref['gu'], TOL_G)
        for k, p in params.items():
            if k in frozen:
                assert p.grad is None
            else:
                check('g' + k, p.grad, ref['g' + k], TOL_G)
    # parameters only: u needs no gradient
    down, up = _convs(t)
    RF.channel_attention(t['u'], down, up, x=t['x'], res_scale=0.5).backward(t['g'])
    check('gw1', down.weight.grad, ref['gw1'], TOL_G)
    check('gb2', up.bias.grad, ref['gb2'], TOL_G)


def test_bit_identical_from_run_to_run():
    """No atomics anywhere: out, gu and the four parameter gradients of the sliced shape repeat bit for bit."""
    from realvsr_amd import functional as RF
    t = _device_inputs('sliced')
    runs = []
    for _ in range(5):
        down, up = _convs(t)
        u = t['u'].detach().requires_grad_(True)
        y = RF.channel_attention(u, down, up, x=t['x'], res_scale=0.5)
        y.backward(t['g'])
        runs.append([y.detach(), u.grad, down.weight.grad, down.bias.grad, up.weight.grad, up.bias.grad])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


def test_refusals():
    from realvsr_amd import functional as RF
    d = dev()
    u = torch.randn(1, 16, 4, 4, device=d)
    with pytest.raises(RuntimeError):      # 1x1 convs that do not fit the tensor
        RF.channel_attention(u, torch.nn.Conv2d(8, 2, 1).to(d), torch.nn.Conv2d(2, 8, 1).to(d))
    with pytest.raises(NotImplementedError):
        RF.channel_attention(u.cpu(), torch.nn.Conv2d(16, 1, 1), torch.nn.Conv2d(1, 16, 1))
    with pytest.raises(TypeError):
        RF.channel_attention(u.double(), torch.nn.Conv2d(16, 1, 1).to(d).double(), torch.nn.Conv2d(1, 16, 1).to(d).double())


def _rcab_case(gemm_mode, C, B, H, W, frozen=()):
    """rcab(...) as one autograd node against the same block composed from RF.conv2d + channel_attention + x: output, gx and all
    eight parameter gradients.  Both sides run the same conv kernels: the tolerances of the running GEMM mode.  The inputs named in
    `frozen` ('x', 'conv1', 'conv2': both parameters of the conv) require no gradient in the node's run and must get None."""
    from realvsr_amd import functional as RF
    T, T_G, _ = TOLS[gemm_mode]
    d = dev()
    gen = torch.Generator().manual_seed(9)
    r = 16
    x0 = torch.randn(B, C, H, W, generator=gen).to(d)
    g = torch.randn(B, C, H, W, generator=gen).to(d)
    mods = [torch.nn.Conv2d(C, C, 3, 1, 1), torch.nn.Conv2d(C, C, 3, 1, 1), torch.nn.Conv2d(C, C // r, 1), torch.nn.Conv2d(C // r, C, 1)]
    with torch.no_grad():
        for m in mods:
            scale = 1.0 if m.kernel_size == (1, 1) else 0.5 / (9 * C) ** 0.5
            m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * scale)
            m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
    mods = [m.to(d) for m in mods]
    c1, c2, down, up = mods

    def run(fused):
        for m, n in zip(mods, ('conv1', 'conv2', 'down', 'up')):
            m.zero_grad(set_to_none=True)
            m.requires_grad_(not (fused and n in frozen))
        x = x0.detach().requires_grad_(not (fused and 'x' in frozen))
        if fused:
            y = RF.rcab(x, c1, c2, down, up, 0.5)
        else:
            y = RF.channel_attention(RF.conv2d(RF.conv2d(x, c1, RF.ACT_RELU), c2), down, up, res_scale=0.5) + x
        y.backward(g)
        return [y.detach(), x.grad] + [p.grad for m in mods for p in (m.weight, m.bias)]

    got, want = run(True), run(False)
    check('out', got[0], want[0], T)
    names = ['gx'] + ['g%s.%s' % (n, k) for n in ('conv1', 'conv2', 'down', 'up') for k in ('weight', 'bias')]
    for name, a, b in zip(names, got[1:], want[1:]):
        if name.split('.')[0][1:] in frozen:      # 'gx' -> 'x', 'gconv1.weight' -> 'conv1'
            assert a is None, name
        else:
            gcheck(gemm_mode, name, a, b, T_G)


def test_rcab_node_vs_composed(gemm_mode):
    _rcab_case(gemm_mode, 64, 2, 12, 20)


@pytest.mark.parametrize('frozen', ['x', 'conv1', 'conv2'])
def test_rcab_frozen_inputs_vs_composed(frozen, gemm_mode):
    """needs_input_grad of the node, as test_gpu_conv_nodes.test_res_block_frozen_inputs_vs_float64: the chain behind the channel
    attention skips conv1's data gradient, conv1's or conv2's weight gradient; what is still wanted is what it was."""
    _rcab_case(gemm_mode, 16, 1, 8, 12, (frozen,))
