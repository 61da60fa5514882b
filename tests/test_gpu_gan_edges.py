"""The two non-convolution operators of the GAN stage at their edges (csrc/gan_kernels.hip through functional.batch_norm_lrelu,
functional.gan_criterion and loss.GANLoss) against the float64 references of tests/gan_reference.py.  -m gpu

BatchNorm2d + LeakyReLU: the smallest shapes that reach every slicing of the per-channel reduction (one slice, two uneven slices, ragged
boundaries inside a plane and across batch elements, the cap at 64 slices), C = 1 / 65 / 130 against the 64 channels per workgroup of the
statistics kernels, every branch of the wrapper (no affine, no buffers, eval, frozen parameters, an input without gradient, other
momentum / eps / slope, non-contiguous views, one module applied three times in one graph -- also with its parameters in optim.FlatAdam),
the refusals, and three ill-conditioned inputs.  Where the case is named '_stats' the output gradient is built so that the two
statistics terms of gx are as large as gx, and gx - k1 * gz is compared on its own, relative to ITS maximum.

Criterion: na on both sides of the 1024-thread workgroup, nb != na, smoothed labels, saturated logits (bit-exact where float32 sigmoid
is exactly 0 or 1), a subnormal tail, every needs-grad combination, a non-contiguous operand, an upstream gradient other than 1.

Bounds: 2e-5 for tensors, 1e-6 absolute for the running statistics, 2e-6 for the criterion value (gpu_util.check: maximum and L2).
Where the operator itself is ill-conditioned in float32 (n = 2: gx is a difference of nearly equal terms; the ill_* inputs) the bound on
max |got - ref| per tensor is max(2e-5 * max |ref|, 8 x the error of torch's float32 CPU evaluation of the same inputs against float64);
both numbers are printed.  No matrix-core arithmetic is involved: one GEMM mode, except for the FlatAdam case."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import gan_reference as GR
from gpu_util import check, dev, gemm_modes

pytestmark = pytest.mark.gpu
gemm_mode = gemm_modes()
TOL, TOL_RUNNING, TOL_LOSS, TOL_CG = 2e-5, 1e-6, 2e-6, 2e-5


# ------------------------------------------------------------------------------------------ BatchNorm2d + LeakyReLU
def _module(t, affine=True, track=True, momentum=0.1, eps=1e-5):
    bn = nn.BatchNorm2d(t['x'].shape[1], eps=eps, momentum=momentum, affine=affine, track_running_stats=track)
    with torch.no_grad():
        if affine:
            bn.weight.copy_(t['weight'])
            bn.bias.copy_(t['bias'])
        if track:
            bn.running_mean.copy_(t['running_mean'])
            bn.running_var.copy_(t['running_var'])
    return bn.to(dev())


def _got(bn, y, gx):
    g = lambda p: None if p is None else p.grad     # noqa: E731
    return dict(y=y, gx=gx, ggamma=g(bn.weight), gbeta=g(bn.bias), running_mean=bn.running_mean, running_var=bn.running_var)


def _check_abs(name, got, ref, bound, note=''):
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all(), name
    e = (got - ref).abs().max().item()
    print('%-44s max_err %.3e (bound %.3e%s)' % (name, e, bound, note))
    assert e <= bound, '%s: max_err %.3e > %.3e' % (name, e, bound)


def _compare(name, got, ref, yard=None, only=GR.BN_TENSORS):
    """Every tensor of `only` that the reference has.  yard: {tensor: float32 yardstick error} for the tensors that go by the rule of
    the ill-conditioned cases."""
    for k in only:
        if ref[k] is None:
            assert got[k] is None, k
        elif yard is not None and k in yard:
            bound = GR.yardstick_bound(ref[k], yard[k])
            _check_abs('%s %s' % (name, k), got[k], ref[k], bound, ' = max(2e-5 * %.3e, 8 * yardstick %.3e)' % (ref[k].abs().max().item(), yard[k]))
        elif k.startswith('running'):
            _check_abs('%s %s' % (name, k), got[k], ref[k], TOL_RUNNING)
        else:
            check('%s %s' % (name, k), got[k], ref[k], TOL)


def _check_stat(name, gx, y, ref, slope):
    """The statistics part of the kernel's gx, gx - k1 * gz, with the float64 k1 and gz = gy * lrelu' taken from the kernel's saved y,
    against the reference's, relative to that part's own maximum."""
    yk = y.detach().cpu()
    one, sl = torch.ones((), dtype=torch.float64), torch.full((), float(slope), dtype=torch.float64)
    gz = ref['gy'].double() * torch.where(yk > 0, one, sl)
    part = gx.detach().cpu().double() - ref['k1'] * gz
    print('%s: statistics part max %.3e of gx max %.3e' % (name, ref['stat'].abs().max().item(), ref['gx'].abs().max().item()))
    check('%s gx - k1 * gz' % name, part, ref['stat'], TOL)


@pytest.mark.parametrize('name', list(GR.BN_CASES))
def test_batchnorm_lrelu_shapes(name):
    from realvsr_amd import functional as RF
    t, ref = GR.bn_inputs(name), GR.bn_case_reference(name)
    d = dev()
    bn = _module(t).train()
    xt = t['x'].to(d).requires_grad_(True)
    y = RF.batch_norm_lrelu(xt, bn, 0.2)
    y.backward(ref['gy'].to(d))
    torch.cuda.synchronize()
    yard = None
    if name in GR.ILL_CONDITIONED:
        yard = GR.bn_case_yardstick(name)
    elif name == 'n2':
        yard = {'gx': GR.bn_case_yardstick(name)['gx']}
    _compare(name, _got(bn, y, xt.grad), ref, yard)
    assert int(bn.num_batches_tracked) == 1
    if name.endswith('_stats'):
        _check_stat(name, xt.grad, y, ref, 0.2)


PATHS = {
    'affine_false': dict(affine=False),
    'no_buffers_train': dict(track=False),
    'no_buffers_eval': dict(track=False, train=False),
    'eval': dict(train=False),
    'eval_frozen': dict(train=False, freeze=True),
    'frozen_parameters': dict(freeze=True),
    'input_without_gradient': dict(x_grad=False),
    'momentum0.3_eps1e-3': dict(momentum=0.3, eps=1e-3),
    'slope0': dict(slope=0.0),
    'slope1': dict(slope=1.0),
    'noncontiguous': dict(views=True),
}


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('name', ['ragged_np2_stats', 'n6_stats'])
def test_batchnorm_lrelu_argument_paths(name, path):
    """Every branch of functional.batch_norm_lrelu at a sliced, ragged shape and at n = 6, with the structured output gradient."""
    from realvsr_amd import functional as RF
    cfg = dict(affine=True, track=True, train=True, freeze=False, x_grad=True, momentum=0.1, eps=1e-5, slope=0.2, views=False)
    cfg.update(PATHS[path])
    t = GR.bn_inputs(name)
    has = lambda k, on: t[k] if on else None     # noqa: E731
    ref = GR.bn_reference(t['x'], t['gy'], has('weight', cfg['affine']), has('bias', cfg['affine']), has('running_mean', cfg['track']),
                          has('running_var', cfg['track']), cfg['train'], cfg['momentum'], cfg['eps'], cfg['slope'])
    assert ref['share'] <= 0.01
    d = dev()
    bn = _module(t, cfg['affine'], cfg['track'], cfg['momentum'], cfg['eps']).train(cfg['train'])
    if cfg['freeze']:
        bn.requires_grad_(False)
    gy = ref['gy'].to(d)
    if cfg['views']:     # NCHW views of NHWC memory: the wrapper has to copy, forward and backward
        leaf = t['x'].to(d).permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        xin = leaf.permute(0, 3, 1, 2)
        gy = gy.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not xin.is_contiguous() and not gy.is_contiguous()
    else:
        leaf = xin = t['x'].to(d).requires_grad_(cfg['x_grad'])
    y = RF.batch_norm_lrelu(xin, bn, cfg['slope'])
    y.backward(gy)
    torch.cuda.synchronize()
    gx = None
    if cfg['x_grad']:
        gx = leaf.grad.permute(0, 3, 1, 2) if cfg['views'] else leaf.grad
    else:
        assert leaf.grad is None
    got = _got(bn, y, gx)
    skip = (() if cfg['x_grad'] else ('gx',)) + (('ggamma', 'gbeta') if cfg['freeze'] else ())
    _compare('%s %s' % (name, path), got, ref, only=[k for k in GR.BN_TENSORS if k not in skip])
    if cfg['freeze']:
        assert bn.weight.grad is None and bn.bias.grad is None
    if cfg['track']:
        assert int(bn.num_batches_tracked) == int(cfg['train'])
        if not cfg['train']:
            assert torch.equal(bn.running_mean.cpu(), t['running_mean']) and torch.equal(bn.running_var.cpu(), t['running_var'])
    else:
        assert bn.running_mean is None and bn.num_batches_tracked is None
    if gx is not None and (cfg['train'] or not cfg['track']):
        _check_stat('%s %s' % (name, path), gx, y, ref, cfg['slope'])


def _three_inputs_case(flat):
    from realvsr_amd import functional as RF
    from realvsr_amd.optim import FlatAdam
    first, xs, refs, rm, rv = GR.three_inputs_reference()
    d = dev()
    bn = _module(first).train()
    opt = None
    if flat:
        opt = FlatAdam(bn.parameters(), lr=1e-3)
        opt.zero_grad()
        assert bn.weight.grad is None and bn.bias.grad is None
    xts = [x.to(d).requires_grad_(True) for x in xs]
    ys = [RF.batch_norm_lrelu(xt, bn, 0.2) for xt in xts]
    torch.autograd.backward(ys, [r['gy'].to(d) for r in refs])
    torch.cuda.synchronize()
    for i, (xt, y, r) in enumerate(zip(xts, ys, refs)):
        check('input %d y' % i, y, r['y'], TOL)
        check('input %d gx' % i, xt.grad, r['gx'], TOL)
        _check_stat('input %d' % i, xt.grad, y, r, 0.2)
    if flat:
        fb = opt.buffers
        fb.rebind()
        fb.check_bound()
        for p in (bn.weight, bn.bias):
            assert p.grad.data_ptr() == fb.grad.data_ptr() + 4 * fb.offset[p]
    check('summed ggamma', bn.weight.grad, sum(r['ggamma'] for r in refs), TOL)
    check('summed gbeta', bn.bias.grad, sum(r['gbeta'] for r in refs), TOL)
    _check_abs('running_mean after three updates', bn.running_mean, rm, TOL_RUNNING)
    _check_abs('running_var after three updates', bn.running_var, rv, TOL_RUNNING)
    assert int(bn.num_batches_tracked) == 3
    return bn.weight.grad.clone(), bn.bias.grad.clone()


def test_batchnorm_lrelu_one_module_three_inputs_one_backward():
    _three_inputs_case(flat=False)


def test_batchnorm_lrelu_three_inputs_parameters_in_flat_adam(gemm_mode):
    """The gradient home is handed out once per zero_grad, the two later uses take temporaries: p.grad is the same sum, and after
    FlatBuffers.rebind() it sits in the flat buffer."""
    _three_inputs_case(flat=True)


def _bn_raw_call(L, t, *, rm=True, rv=True, short=0, train=1):
    """rvsr_bn_lrelu_forward on NaN-filled outputs -> (return code, y)."""
    from realvsr_amd._lib import _p, _stream
    d = dev()
    x = t['x'].to(d)
    B, C, H, W = x.shape
    dv = {k: t[k].to(d) for k in ('weight', 'bias', 'running_mean', 'running_var')}
    y = torch.full_like(x, float('nan'))
    mean, invstd = torch.full((C,), float('nan'), device=d), torch.full((C,), float('nan'), device=d)
    need = L.rvsr_bn_workspace_bytes(B, C, H * W)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=d)
    rc = L.rvsr_bn_lrelu_forward(_p(x), _p(dv['weight']), _p(dv['bias']), _p(dv['running_mean']) if rm else None,
                                 _p(dv['running_var']) if rv else None, None, _p(y), _p(mean), _p(invstd), B, C, H * W, train, 0.1, 1e-5,
                                 0.2, _p(ws), need - short, _stream())
    torch.cuda.synchronize()
    return rc, y, (x, dv, mean, invstd, ws, need)


def test_batchnorm_lrelu_refusals():
    from realvsr_amd import _lib
    from realvsr_amd import functional as RF
    from realvsr_amd._lib import _p, _stream
    d = dev()
    L = _lib.lib()
    bn = nn.BatchNorm2d(4).to(d).train()
    with pytest.raises(RuntimeError, match='more than one value per channel'):      # train mode, n = 1
        RF.batch_norm_lrelu(torch.randn(1, 4, 1, 1, device=d), bn)
    assert int(bn.num_batches_tracked) == 0
    RF.batch_norm_lrelu(torch.randn(1, 4, 1, 1, device=d), bn.eval())              # (eval takes n = 1)
    with pytest.raises(NotImplementedError):
        RF.batch_norm_lrelu(torch.randn(2, 4, 3, 3, device=d), nn.BatchNorm2d(4, momentum=None).to(d))
    with pytest.raises(TypeError):
        RF.batch_norm_lrelu(torch.randn(2, 4, 3, 3, device=d, dtype=torch.float64), bn)
    with pytest.raises(NotImplementedError):
        RF.batch_norm_lrelu(torch.randn(2, 4, 3, 3), nn.BatchNorm2d(4))
    # the raw ABI: error returns, nothing launched (the outputs keep their NaN fill)
    t = GR.bn_inputs('ill_const')
    rc, y, _ = _bn_raw_call(L, t)
    assert rc == 0 and torch.isfinite(y).all()
    for kw in (dict(rv=False), dict(rm=False)):
        rc, y, _ = _bn_raw_call(L, t, **kw)
        assert rc == _lib.RVSR_ERR_BAD_ARG and torch.isnan(y).all()
    rc, y, _ = _bn_raw_call(L, t, rm=False, rv=False, train=0)      # eval needs them
    assert rc == _lib.RVSR_ERR_BAD_ARG and torch.isnan(y).all()
    rc, y, (x, dv, mean, invstd, ws, need) = _bn_raw_call(L, t, short=1)
    assert rc == _lib.RVSR_ERR_WORKSPACE and torch.isnan(y).all() and torch.isnan(mean).all()
    B, C, H, W = x.shape
    gx, gw = torch.full_like(x, float('nan')), torch.full((C,), float('nan'), device=d)
    args = (_p(x), _p(x), _p(x), _p(dv['weight']), _p(dv['running_mean']), _p(dv['running_var']), _p(gx), _p(gw), None, B, C, H * W, 1, 0.2)
    assert L.rvsr_bn_lrelu_backward(*args, _p(ws), need - 1, _stream()) == _lib.RVSR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(gx).all() and torch.isnan(gw).all()
    assert L.rvsr_bn_lrelu_backward(*args, _p(ws), need, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(gx).all() and torch.isfinite(gw).all()


# ------------------------------------------------------------------------------------------ BCE-with-logits criterion
def _crit(name, target):
    """loss.GANLoss with `target` as its real label (1, 0.9) or as its fake label (0, 0.1)."""
    from realvsr_amd.loss import GANLoss
    kind = 'ragan' if name.startswith('rel_') else 'gan'
    is_real = target >= 0.5
    return GANLoss(kind, target if is_real else 1.0, 0.0 if is_real else target), is_real


def _f32_gradient_at_saturation(g, na, s, target):
    """g * scale * (s - t) as the kernel evaluates it in float32: (g * scale) * (s - t), scale = float32(1 / na)."""
    f = np.float32
    return float((f(g) * f(1.0 / na)) * (f(s) - f(target)))


@pytest.mark.parametrize('target', GR.CRIT_TARGETS)
@pytest.mark.parametrize('name', [n for n in GR.CRIT_CASES if n != 'rel_tail'])
def test_gan_criterion_sizes_targets_saturation(name, target):
    a, b = GR.crit_inputs(name)
    G = 0.7
    ref = GR.crit_reference(a, b, target, G)
    d = dev()
    at = a.to(d).requires_grad_(True)
    bt = None if b is None else b.to(d).requires_grad_(True)
    crit, is_real = _crit(name, target)
    loss = crit(at, is_real, other=bt)
    (G * loss).backward()
    torch.cuda.synchronize()
    assert loss.shape == () and at.grad.shape == a.shape
    check('%s t=%g loss' % (name, target), loss, ref['loss'], TOL_LOSS)
    check('%s t=%g ga' % (name, target), at.grad, ref['ga'], TOL_CG)
    if b is not None:
        assert bt.grad.shape == b.shape
        check('%s t=%g gb' % (name, target), bt.grad, ref['gb'], TOL_CG)
    if 'saturated' in name:
        zero, one = GR.saturation_masks(a, b)
        ga = at.grad.cpu()
        for mask, s in ((zero, 0.0), (one, 1.0)):
            want = torch.full((int(mask.sum()),), _f32_gradient_at_saturation(G, a.numel(), s, target), dtype=torch.float32)
            assert torch.equal(ga[mask].view(torch.int32), want.view(torch.int32)), (s, ga[mask], want)


def test_gan_criterion_subnormal_tail():
    """z in [-91, -89], label 0: sigmoid(z) = e^z / (1 + e^z) ~ 1e-39 is a float32 subnormal, 1 / (1 + e^-z) is 0 because e^89
    overflows.  The gradients ARE the sigmoid here (ga = sigmoid / na, gb = -sum(sigmoid) / (na nb)); float32 resolves them to 2e-6."""
    a, b = GR.crit_inputs('rel_tail')
    ref = GR.crit_reference(a, b, 0.0)
    d = dev()
    at, bt = a.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    crit, is_real = _crit('rel_tail', 0.0)
    loss = crit(at, is_real, other=bt)
    loss.backward()
    torch.cuda.synchronize()
    # torch's float64 BCE evaluates log(exp(-m) + exp(-z - m)) and returns 0 here: the value comes from log1p(e^z), the form
    # test_gan_reference_host.py holds to the module wherever the module resolves it
    loss_ref = torch.log1p(torch.exp(ref['z'])).mean()
    print('loss %.6e (ref %.6e, torch float64 %.1e), ga %s, gb %s (ref %.6e)' % (
        loss.item(), loss_ref.item(), ref['loss'].item(), at.grad.flatten().tolist(), bt.grad.flatten().tolist(), ref['gb'].flatten()[0].item()))
    assert 1e-40 < ref['gb'].abs().max().item() < 1e-38 and 1e-40 < ref['ga'].abs().min().item() and 1e-40 < loss_ref.item() < 1e-38
    # gpu_util's errors have 1e-30 in their denominators: compare at unit scale (2^130 is exact in float64)
    up = 2.0 ** 130
    check('tail loss', loss.cpu().double() * up, loss_ref * up, TOL_CG)      # (three subnormals: held as a gradient is, not to 2e-6)
    check('tail ga', at.grad.cpu().double() * up, ref['ga'] * up, TOL_CG)
    check('tail gb', bt.grad.cpu().double() * up, ref['gb'] * up, TOL_CG)


@pytest.mark.parametrize('name', ['rel_n1025', 'rel_nb1_na1025', 'rel_nb1025_na7', 'rel_saturated', 'n1025'])
def test_gan_criterion_needs_grad_combinations(name):
    """pred_d_real.detach() in the generator step: ga == NULL with gb wanted, and the reverse.  Each wanted gradient is bit for bit
    what it is when both are wanted; with neither the backward returns before it touches anything."""
    from realvsr_amd import functional as RF
    a, b = GR.crit_inputs(name)
    d = dev()

    def run(a_grad, b_grad):
        at = a.to(d).requires_grad_(a_grad)
        bt = None if b is None else b.to(d).requires_grad_(b_grad)
        loss = RF.gan_criterion(at, 0.9, bt)
        if not (a_grad or (b_grad and b is not None)):
            assert not loss.requires_grad
            return loss, None, None
        (-1.5 * loss).backward()
        return loss, at.grad, None if bt is None else bt.grad

    l0, ga0, gb0 = run(True, True)
    ref = GR.crit_reference(a, b, 0.9, -1.5)
    check('ga', ga0, ref['ga'], TOL_CG)
    l1, ga1, gb1 = run(True, False)
    assert torch.equal(l1, l0) and torch.equal(ga1, ga0) and gb1 is None
    l3, ga3, gb3 = run(False, False)
    assert torch.equal(l3, l0) and ga3 is None and gb3 is None
    if b is not None:
        check('gb', gb0, ref['gb'], TOL_CG)
        l2, ga2, gb2 = run(False, True)
        assert torch.equal(l2, l0) and ga2 is None and torch.equal(gb2, gb0)
    # neither wanted, the node called directly: it returns before it reads its saved tensors or calls the library
    ctx = types.SimpleNamespace(saved_tensors=(None, None), cfg=(0.9, 1.0 / a.numel(), 0 if b is None else b.numel(), None),
                                needs_input_grad=(False, False, False))
    assert RF._GANCriterion.backward(ctx, torch.ones((), device=d)) == (None, None, None)


def test_gan_criterion_noncontiguous_operands_and_upstream_gradient():
    from realvsr_amd.loss import GANLoss
    a, b = GR.crit_inputs('rel_nb1025_na7')
    a2, _ = GR.crit_inputs('rel_n1025')
    d = dev()
    for av, bv, G in ((a2, b, -2.5), (a, a2, 3.0)):
        ref = GR.crit_reference(av, bv, 0.1, G)
        # every second column of a wider tensor; b transposed
        wide = torch.zeros(av.shape[:-1] + (2 * av.shape[-1],), device=d)
        wide[..., ::2] = av.to(d)
        wide.requires_grad_(True)
        bleaf = bv.to(d).transpose(2, 3).contiguous().requires_grad_(True)
        aview, bview = wide[..., ::2], bleaf.transpose(2, 3)
        assert not aview.is_contiguous() and (bv.shape[2] == 1 or not bview.is_contiguous())
        loss = GANLoss('ragan', 1.0, 0.1)(aview, False, other=bview)
        (G * loss).backward()
        torch.cuda.synchronize()
        check('loss', loss, ref['loss'], TOL_LOSS)
        check('ga', wide.grad[..., ::2], ref['ga'], TOL_CG)
        assert not wide.grad[..., 1::2].any()
        check('gb', bleaf.grad.transpose(2, 3), ref['gb'], TOL_CG)


def test_gan_criterion_refusals():
    from realvsr_amd import _lib
    from realvsr_amd import functional as RF
    from realvsr_amd._lib import _p, _stream
    d = dev()
    L = _lib.lib()
    a = torch.randn(8, device=d)
    out, saved = torch.full((), float('nan'), device=d), torch.full((2,), float('nan'), device=d)
    assert L.rvsr_gan_loss_forward(_p(a), 0, None, 0, 1.0, 1.0, _p(out), _p(saved), _stream()) == _lib.RVSR_ERR_BAD_ARG
    assert L.rvsr_gan_loss_forward(_p(a), 8, _p(a), 0, 1.0, 0.125, _p(out), _p(saved), _stream()) == _lib.RVSR_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(saved).all()
    assert L.rvsr_gan_loss_forward(_p(a), 8, _p(a), 8, 1.0, 0.125, _p(out), _p(saved), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(saved).all()
    g, ga, gb = torch.ones((), device=d), torch.full((8,), float('nan'), device=d), torch.full((8,), float('nan'), device=d)
    assert L.rvsr_gan_loss_backward(_p(a), 0, 8, _p(saved), _p(g), 1.0, 0.125, _p(ga), _p(gb), _stream()) == _lib.RVSR_ERR_BAD_ARG
    assert L.rvsr_gan_loss_backward(_p(a), 8, 0, _p(saved), _p(g), 1.0, 0.125, _p(ga), _p(gb), _stream()) == _lib.RVSR_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(ga).all() and torch.isnan(gb).all()
    with pytest.raises(NotImplementedError):
        RF.gan_criterion(torch.randn(4), 1.0)
    with pytest.raises(TypeError):
        RF.gan_criterion(torch.randn(4, device=d, dtype=torch.float64), 1.0)
    with pytest.raises(NotImplementedError):
        from realvsr_amd.loss import GANLoss
        GANLoss('lsgan')
