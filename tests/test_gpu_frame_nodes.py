"""The autograd nodes built only from conv calls over frame ranges -- RF.conv3d_frames, RF.conv_transpose1x1, RF.tsa_temporal_block --
and FSTRN at the frame counts where a temporal tap meets nothing, vs the float64 references of tests/frame_reference.py.  -m gpu

The conv kernels are pinned per variant elsewhere (tests/test_conv_ledger_host.py); these cases are about the nodes' arithmetic: which
frame range a tap reads and writes, which slice of the weight gradient it fills, what is zero-filled, where an in-place accumulation
lands, and that nothing relies on a gradient buffer having been cleared.  A *flat* run puts the parameters into optim.FlatAdam,
zero_grad()s and then fills the flat gradient buffer with -77: no sentinel may survive in a gradient.

Tolerances: TOLS[mode] of test_gpu_conv.py for a quantity one split GEMM from its inputs, that many times TOLS for one that depends on
several (the rule of test_gpu_conv_nodes.py): 1 x for conv3d_frames and conv_transpose1x1; the TSA block's output 2 x (tAtt_1 and
tAtt_2 both feed it), its gradients 3 x (two forward GEMMs, then a gradient GEMM); FSTRN as tests/test_gpu_fstrn.py holds its fixtures."""
import zlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import frame_reference as FR
from gpu_util import check, dev, gemm_modes
from test_gpu_conv import TOLS

pytestmark = pytest.mark.gpu
gemm_mode = gemm_modes()
SENTINEL = -77.0


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 2 ** 31)


def _ids(cases):
    return ['-'.join(str(int(v)) if isinstance(v, bool) else str(v) for v in c).replace(' ', '') for c in cases]


def _flat(params):
    """The parameters inside FlatAdam's buffers after zero_grad(), the flat gradient buffer then filled with the sentinel."""
    from realvsr_amd.optim import FlatAdam
    opt = FlatAdam(list(params))
    opt.zero_grad()
    opt.buffers.grad.fill_(SENTINEL)
    return opt


def _flat_grads_are_home(opt, params):
    """After backward: rebind() (what the optimizer step does first) leaves every gradient in its flat view, with no sentinel in it."""
    opt.buffers.rebind()
    opt.buffers.check_bound()
    for name, p in params:
        assert p.grad is not None and p.grad.data_ptr() == opt.buffers.grad_view(p).data_ptr(), name
        assert not bool((p.grad == SENTINEL).any()), 'the gradient of %s relies on a cleared buffer' % name


def _check_or_zero(name, got, ref, tol):
    """check(), or exact zeros where the reference is exactly zero (a relative error has no scale there)."""
    if bool((ref == 0).all()):
        assert bool((got == 0).all()), '%s: expected exact zeros, max |.| %.3e' % (name, got.abs().max().item())
        print('%-44s exactly 0' % name)
    else:
        check(name, got, ref, tol)


# ------------------------------------------------------------------------------------------ conv3d_frames
# (T, f0, f1, B, Ci, Co, H, W, k, bias, residual).  With C = 3 and B = 1 a 5 x 7 frame holds 105 floats (9 x 33: 891): every frame slice
# after the first starts off a 16-byte boundary -- as input (Ci = 3), as output and in-place residual (Co = 3).
C3_CASES = [
    # T = 1: the outer taps meet no frame
    (1, 0, 1, 1, 3, 16, 5, 7, 3, True, False), (1, 0, 1, 2, 16, 16, 8, 12, 3, True, True), (1, 0, 1, 1, 16, 24, 9, 33, 3, True, True),
    # T = 2: each outer tap meets one frame
    (2, 0, 2, 1, 3, 16, 5, 7, 3, True, False), (2, 0, 2, 2, 16, 24, 8, 12, 3, True, True), (2, 0, 2, 1, 16, 3, 9, 33, 3, True, True),
    (2, 0, 1, 1, 16, 3, 5, 7, 3, True, True), (2, 0, 1, 1, 16, 16, 9, 33, 3, False, True),
    (2, 1, 2, 1, 3, 16, 5, 7, 3, True, True), (2, 1, 2, 2, 16, 16, 9, 33, 3, True, False),
    # T = 3: whole and interior (the ranges of the fixtures, on other channels and frames)
    (3, 0, 3, 1, 3, 16, 5, 7, 3, True, True), (3, 0, 3, 1, 16, 3, 5, 7, 3, True, False), (3, 0, 3, 2, 16, 16, 8, 12, 3, True, False),
    (3, 0, 3, 1, 64, 64, 8, 12, 3, True, True), (3, 0, 3, 1, 3, 16, 9, 33, 3, True, False),
    (3, 1, 2, 1, 16, 3, 5, 7, 3, True, True), (3, 1, 2, 2, 16, 24, 9, 33, 3, True, True),
    # T = 4, interior
    (4, 1, 3, 1, 3, 16, 5, 7, 3, True, False), (4, 1, 3, 2, 16, 16, 8, 12, 3, True, True), (4, 1, 3, 1, 16, 3, 9, 33, 3, True, True),
    # T = 5: whole, interior, the two edges, the centre
    (5, 0, 5, 1, 3, 16, 5, 7, 3, True, True), (5, 0, 5, 2, 16, 16, 8, 12, 3, True, False), (5, 0, 5, 1, 16, 3, 5, 7, 3, True, True),
    (5, 0, 5, 1, 16, 24, 9, 33, 3, True, True),
    (5, 1, 4, 1, 3, 16, 5, 7, 3, True, False), (5, 1, 4, 2, 16, 24, 8, 12, 3, True, True), (5, 1, 4, 1, 16, 16, 9, 33, 3, True, False),
    (5, 1, 4, 1, 16, 3, 5, 7, 3, True, True),
    (5, 0, 1, 1, 3, 16, 5, 7, 3, True, True), (5, 0, 1, 2, 16, 16, 8, 12, 3, True, False),
    (5, 4, 5, 1, 3, 16, 5, 7, 3, True, False), (5, 4, 5, 1, 16, 3, 9, 33, 3, True, True), (5, 4, 5, 2, 16, 24, 8, 12, 3, True, False),
    (5, 2, 3, 1, 3, 16, 5, 7, 3, True, True), (5, 2, 3, 2, 16, 16, 8, 12, 3, True, True), (5, 2, 3, 1, 16, 24, 9, 33, 3, True, False),
    # k = 1
    (3, 0, 3, 2, 16, 16, 8, 12, 1, True, True),
]
C3_FLAT = [C3_CASES[0], C3_CASES[1], C3_CASES[3], C3_CASES[11], C3_CASES[20], C3_CASES[31]]


def _c3_case(case, mode, flat=False, x_grad=True, frozen=()):
    from realvsr_amd import functional as RF
    TOL = TOLS[mode]
    T, f0, f1, B, Ci, Co, H, W, k, bias, use_res = case
    g = _gen('conv3d_frames', case)
    conv = nn.Conv3d(Ci, Co, (3, k, k), padding=(1, k // 2, k // 2), bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3 * k * k * Ci) ** 0.5)
        if bias:
            conv.bias.copy_(torch.randn(Co, generator=g) * 0.1)
    x = torch.randn(T, B, Ci, H, W, generator=g)
    res = torch.randn(f1 - f0, B, Co, H, W, generator=g) if use_res else None
    gout = torch.randn(f1 - f0, B, Co, H, W, generator=g)

    xr, wr = x.double().requires_grad_(True), conv.weight.detach().double().requires_grad_(True)
    br = conv.bias.detach().double().requires_grad_(True) if bias else None
    rr = res.double().requires_grad_(True) if use_res else None
    yr = FR.conv3d_frames_ref(xr, wr, br, rr, f0, f1)
    yr.backward(gout.double())

    d = dev()
    conv = conv.to(d)
    for n, p in conv.named_parameters():
        p.requires_grad_(n not in frozen)
    opt = _flat(conv.parameters()) if flat else None
    xg = x.to(d).requires_grad_(x_grad)
    rg = res.to(d).requires_grad_(True) if use_res else None
    gd = gout.to(d)
    y = RF.conv3d_frames(xg, conv, frames=(f0, f1), residual=rg)
    y.backward(gd)
    torch.cuda.synchronize()
    if flat:
        _flat_grads_are_home(opt, list(conv.named_parameters()))
    check('out', y, yr, TOL)
    if x_grad:
        check('grad_x', xg.grad, xr.grad, TOL)
        reached = [t for t in range(T) if f0 - 1 <= t <= f1]     # input frame t is read by the output frames t - 1, t, t + 1
        for t in set(range(T)) - set(reached):
            assert bool((xg.grad[t] == 0).all()), 'grad_x of frame %d, which no tap reaches, is not exactly 0' % t
            assert bool((xr.grad[t] == 0).all())
    else:
        assert xg.grad is None
    if 'weight' in frozen:
        assert conv.weight.grad is None
    else:
        met = FR.c3_taps_by_definition(T, f0, f1)
        for dt in range(3):
            assert bool((wr.grad[:, :, dt] == 0).all()) == (dt not in met)
            _check_or_zero('grad_weight[:, :, %d]' % dt, conv.weight.grad[:, :, dt], wr.grad[:, :, dt], TOL)
    if bias:
        check('grad_bias', conv.bias.grad, br.grad, TOL)
    if use_res:
        assert torch.equal(rg.grad, gd), 'grad_residual is not the output gradient bit for bit'


@pytest.mark.parametrize('case', C3_CASES, ids=_ids(C3_CASES))
def test_conv3d_frames_vs_float64(case, gemm_mode):
    """Output, grad_x (exactly 0 on frames no tap reaches), grad_weight per temporal slice (exactly 0 for a tap that meets no frame),
    grad_bias and grad_residual (bit-equal to the output gradient)."""
    _c3_case(case, gemm_mode)


@pytest.mark.parametrize('case', C3_FLAT, ids=_ids(C3_FLAT))
def test_conv3d_frames_writes_every_flat_gradient(case, gemm_mode):
    """The same with the parameters in FlatAdam and the flat gradient buffer full of sentinels: at T = 1 the dt = 0 and dt = 2 slices
    of the weight gradient are exactly 0 because the node wrote them."""
    _c3_case(case, gemm_mode, flat=True)


def test_conv3d_frames_computes_what_is_asked_for(gemm_mode):
    """x without a gradient; the weight frozen with the bias trainable (the bias gradient rides on the centre tap's weight-gradient
    call, whose weight output is then dropped)."""
    _c3_case((2, 1, 2, 1, 16, 16, 8, 12, 3, True, False), gemm_mode, x_grad=False)
    _c3_case((3, 1, 2, 1, 16, 16, 8, 12, 3, True, True), gemm_mode, frozen=('weight',))


def test_conv3d_frames_refusals():
    from realvsr_amd import functional as RF
    d = dev()
    x = torch.randn(3, 1, 16, 5, 7, device=d)
    conv = nn.Conv3d(16, 16, 3, padding=1).to(d)
    for frames in ((1, 1), (2, 1), (0, 4), (3, 4), (-1, 2)):
        with pytest.raises(RuntimeError, match='do not fit'):
            RF.conv3d_frames(x, conv, frames=frames)
    for shape in ((3, 1, 16, 5, 7), (2, 1, 16, 5, 8), (2, 1, 8, 5, 7), (2, 16, 5, 7)):
        with pytest.raises(RuntimeError, match='residual'):
            RF.conv3d_frames(x, conv, frames=(0, 2), residual=torch.randn(shape, device=d))
    for kt in (1, 5):
        with pytest.raises(RuntimeError, match='do not fit'):
            RF.conv3d_frames(x, nn.Conv3d(16, 16, (kt, 3, 3), padding=(kt // 2, 1, 1)).to(d))
    with pytest.raises(RuntimeError, match='do not fit'):
        RF.conv3d_frames(x, nn.Conv3d(8, 16, 3, padding=1).to(d))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ conv_transpose1x1
# (leading dimensions, Ci, Co, H, W, holder, bias): the weight is stored (Ci, Co) -- Ci != Co tells it from (Co, Ci)
CT_CASES = [
    ((3, 2), 16, 24, 5, 7, '3d', True), ((2,), 24, 16, 8, 12, '3d', True), ((1,), 64, 64, 9, 33, '3d', True),
    ((1, 1), 3, 8, 5, 7, '3d', True), ((2,), 24, 16, 8, 12, '2d', True), ((3, 2), 16, 24, 5, 7, '3d', False),
]


def _ct_case(case, mode, flat=False):
    from realvsr_amd import functional as RF
    TOL = TOLS[mode]
    lead, Ci, Co, H, W, holder, bias = case
    g = _gen('conv_transpose1x1', case)
    convt = (nn.ConvTranspose3d if holder == '3d' else nn.ConvTranspose2d)(Ci, Co, 1, bias=bias)
    assert tuple(convt.weight.shape[:2]) == (Ci, Co)
    with torch.no_grad():
        convt.weight.copy_(torch.randn(convt.weight.shape, generator=g) / Ci ** 0.5)
        if bias:
            convt.bias.copy_(torch.randn(Co, generator=g) * 0.1)
    x = torch.randn(*lead, Ci, H, W, generator=g)
    gout = torch.randn(*lead, Co, H, W, generator=g)
    xr, wr = x.double().requires_grad_(True), convt.weight.detach().double().requires_grad_(True)
    br = convt.bias.detach().double().requires_grad_(True) if bias else None
    yr = FR.conv_transpose1x1_ref(xr, wr, br)
    yr.backward(gout.double())

    d = dev()
    convt = convt.to(d)
    opt = _flat(convt.parameters()) if flat else None
    xg = x.to(d).requires_grad_(True)
    y = RF.conv_transpose1x1(xg, convt)
    y.backward(gout.to(d))
    torch.cuda.synchronize()
    if flat:
        _flat_grads_are_home(opt, list(convt.named_parameters()))
    check('out', y, yr, TOL)
    check('grad_x', xg.grad, xr.grad, TOL)
    check('grad_weight', convt.weight.grad, wr.grad, TOL)
    if bias:
        check('grad_bias', convt.bias.grad, br.grad, TOL)


@pytest.mark.parametrize('case', CT_CASES, ids=_ids(CT_CASES))
def test_conv_transpose1x1_vs_float64(case, gemm_mode):
    _ct_case(case, gemm_mode)


def test_conv_transpose1x1_writes_every_flat_gradient(gemm_mode):
    _ct_case(CT_CASES[0], gemm_mode, flat=True)


# ------------------------------------------------------------------------------------------ tsa_temporal_block
# (N, center, B, C, H, W); the last: C = 3, B = 1 on 5 x 7 puts the centre block 105 floats in -- a misaligned tAtt_2 input and a
# misaligned in-place data gradient
TSA_CASES = [(1, 0, 1, 16, 5, 7), (2, 1, 2, 16, 5, 7), (3, 1, 1, 64, 8, 12), (5, 2, 2, 16, 9, 33), (5, 0, 1, 16, 8, 12), (5, 4, 1, 16, 8, 12),
             (7, 3, 1, 64, 8, 64), (8, 7, 1, 16, 5, 7), (3, 1, 1, 3, 5, 7)]
TSA_PARAMS = ('w1', 'b1', 'w2', 'b2')


def _tsa_tensors(case, tag=''):
    """aligned, the two convs and the output gradient.  The weights are scaled so that emb and emb_ref have entries of order C^-1/4:
    their correlation over C channels is of order 1 and the sigmoid works on its slope (saturation is pinned at the kernel level,
    tests/test_gpu_glue_edges.py)."""
    N, center, B, C, H, W = case
    g = _gen('tsa_block', case, tag)
    aligned = torch.randn(N, B, C, H, W, generator=g)
    w1, w2 = (torch.randn(C, C, 3, 3, generator=g) / (3.0 * C ** 0.5 * C ** 0.25) for _ in range(2))
    b1, b2 = (torch.randn(C, generator=g) * 0.1 / C ** 0.25 for _ in range(2))
    gmod = torch.randn(B, N * C, H, W, generator=g)
    return aligned, (w1, b1, w2, b2), gmod


def _tsa_holders(params, d):
    from test_gpu_conv_nodes import _holder
    return _holder(params[0], params[1], d), _holder(params[2], params[3], d)


def _tsa_case(case, mode, flat=False, frozen=()):
    """frozen: of 'aligned', 'tAtt_1', 'tAtt_2' -- what wants no gradient; its gradient must be None, the others what they were."""
    from realvsr_amd import functional as RF
    TOL = TOLS[mode]
    N, center, B, C, H, W = case
    aligned, params, gmod = _tsa_tensors(case)
    ar = aligned.double().requires_grad_(True)
    pr = [p.double().requires_grad_(True) for p in params]
    yr = FR.tsa_block_ref(ar, center, *pr)
    cor = (F.conv2d(ar.detach().reshape(N * B, C, H, W), pr[0].detach(), pr[1].detach(), padding=1).reshape(N, B, C, H, W)
           * F.conv2d(ar.detach()[center], pr[2].detach(), pr[3].detach(), padding=1)).sum(2)
    assert 0.3 < cor.std().item() < 3.0 and cor.abs().max().item() < 12.0, 'the correlation is not of unit order'
    yr.backward(gmod.double())

    d = dev()
    t1, t2 = _tsa_holders(params, d)
    for p in t1.parameters():
        p.requires_grad_('tAtt_1' not in frozen)
    for p in t2.parameters():
        p.requires_grad_('tAtt_2' not in frozen)
    named = [('w1', t1.weight), ('b1', t1.bias), ('w2', t2.weight), ('b2', t2.bias)]
    opt = _flat([p for _, p in named]) if flat else None
    ag = aligned.to(d).requires_grad_('aligned' not in frozen)
    y = RF.tsa_temporal_block(ag, center, t1, t2)
    y.backward(gmod.to(d))
    torch.cuda.synchronize()
    if flat:
        _flat_grads_are_home(opt, named)
    check('mod', y, yr, 2 * TOL)
    if 'aligned' in frozen:
        assert ag.grad is None
    else:
        check('grad_aligned', ag.grad, ar.grad, 3 * TOL)
        if N > 1:   # the centre block alone receives tAtt_2's data gradient: held on its own, it cannot hide in the other frames
            check('grad_aligned[center]', ag.grad[center], ar.grad[center], 3 * TOL)
    for (name, p), ref in zip(named, pr):
        if ('tAtt_1' if name in ('w1', 'b1') else 'tAtt_2') in frozen:
            assert p.grad is None, name
        else:
            check('grad_' + name, p.grad, ref.grad, 3 * TOL)


@pytest.mark.parametrize('case', TSA_CASES, ids=_ids(TSA_CASES))
def test_tsa_temporal_block_vs_float64(case, gemm_mode):
    """mod and the gradients of aligned (the centre block also on its own), tAtt_1 and tAtt_2."""
    _tsa_case(case, gemm_mode)


@pytest.mark.parametrize('frozen', ['aligned', 'tAtt_1', 'tAtt_2'])
def test_tsa_temporal_block_frozen_inputs(frozen, gemm_mode):
    _tsa_case((3, 2, 2, 16, 8, 12), gemm_mode, frozen=(frozen,))


def test_tsa_temporal_block_writes_every_flat_gradient(gemm_mode):
    _tsa_case((5, 2, 2, 16, 9, 33), gemm_mode, flat=True)


def test_tsa_temporal_block_twice_in_one_backward(gemm_mode):
    """The same two modules applied to two inputs, parameters in FlatAdam: the flat home of a parameter is handed out once, the second
    use gets a temporary and autograd adds -- the parameter gradients are the sums, each input's gradient its own."""
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    case = (3, 0, 1, 16, 8, 12)
    N, center, B, C, H, W = case
    aligned, params, gmod = _tsa_tensors(case)
    aligned2, _, gmod2 = _tsa_tensors(case, 'second input')
    ar, ar2 = (a.double().requires_grad_(True) for a in (aligned, aligned2))
    pr = [p.double().requires_grad_(True) for p in params]
    (FR.tsa_block_ref(ar, center, *pr) * gmod.double()).sum().backward()
    first = [p.grad.clone() for p in pr]
    (FR.tsa_block_ref(ar2, center, *pr) * gmod2.double()).sum().backward()
    assert all((p.grad - f).abs().max() > 1e-3 * f.abs().max() for p, f in zip(pr, first))   # (the second use contributes)

    d = dev()
    t1, t2 = _tsa_holders(params, d)
    named = [('w1', t1.weight), ('b1', t1.bias), ('w2', t2.weight), ('b2', t2.bias)]
    opt = _flat([p for _, p in named])
    ag, ag2 = aligned.to(d).requires_grad_(True), aligned2.to(d).requires_grad_(True)
    y, y2 = RF.tsa_temporal_block(ag, center, t1, t2), RF.tsa_temporal_block(ag2, center, t1, t2)
    torch.autograd.backward([y, y2], [gmod.to(d), gmod2.to(d)])
    torch.cuda.synchronize()
    _flat_grads_are_home(opt, named)
    check('grad_aligned (first input)', ag.grad, ar.grad, 3 * TOL)
    check('grad_aligned (second input)', ag2.grad, ar2.grad, 3 * TOL)
    for (name, p), ref in zip(named, pr):
        check('grad_%s (sum of two uses)' % name, p.grad, ref.grad, 3 * TOL)


def test_tsa_temporal_block_of_nine_frames():
    """The backward kernel keeps one correlation gradient per frame in an array of 8: N = 9 runs forward and is refused backward."""
    from realvsr_amd import functional as RF
    case = (9, 4, 1, 16, 5, 7)
    aligned, params, gmod = _tsa_tensors(case)
    d = dev()
    t1, t2 = _tsa_holders(params, d)
    ag = aligned.to(d).requires_grad_(True)
    y = RF.tsa_temporal_block(ag, 4, t1, t2)
    with torch.no_grad():
        yr = FR.tsa_block_ref(aligned.double(), 4, *[p.double() for p in params])
    check('mod (N = 9)', y, yr, 2 * TOLS['bf16x3'])
    with pytest.raises(RuntimeError, match='nframes 9 > 8'):
        y.backward(gmod.to(d))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ FSTRN where a tap meets nothing
def _fstrn_ref(sd, x, T):
    """FSTRN.forward in float64 on x [B, T, 3, H, W]: LFENet, five FRBs (x + conv3d_2(conv3d_1(prelu(x))), FRB's docstring), the long
    skip + PReLU (eval: no dropout), conv3d_1 / the 1x1 upsample / conv3d_2 with the cross-space residual at the centre frame."""
    p = lambda k: sd[k]    # noqa: E731
    prelus = {}

    def prelu(z, name):
        y = F.prelu(z, p(name))
        y.retain_grad()
        prelus[name] = (z, y)    # (for the magnitude of the slope gradient, sum |g * z * [z <= 0]|, after backward)
        return y
    xf = x.transpose(0, 1)
    lr_res = FR.conv3d_frames_ref(xf, p('conv3d_fe.weight'), p('conv3d_fe.bias'))
    out = lr_res
    for i in range(1, 6):
        h = FR.conv3d_fm(prelu(out, 'frb_%d.prelu.weight' % i), p('frb_%d.conv3d_1.weight' % i), p('frb_%d.conv3d_1.bias' % i))
        out = out + FR.conv3d_fm(h, p('frb_%d.conv3d_2.weight' % i), p('frb_%d.conv3d_2.bias' % i))
    out = prelu(out + lr_res, 'prelu.weight')
    out = FR.conv3d_frames_ref(out, p('conv3d_1.weight'), p('conv3d_1.bias'))
    out = FR.conv_transpose1x1_ref(out, p('upsample.weight'), p('upsample.bias'))
    c = T // 2
    return FR.conv3d_frames_ref(out, p('conv3d_2.weight'), p('conv3d_2.bias'), xf[c:c + 1], c, c + 1)[0], prelus


@pytest.mark.parametrize('T', [1, 2])
def test_fstrn_at_the_tap_edges(T, gemm_mode):
    """FSTRN(nf=16, nframes=T) in eval mode for T = 1 (both outer taps of every temporal convolution meet nothing) and T = 2 (each
    meets one frame; the centre is the last frame): the output and the gradient of every parameter, at the tolerances
    tests/test_gpu_fstrn.py holds the fixtures to."""
    from weights import fill_state_dict
    from realvsr_amd.archs.FSTRN_arch import FSTRN
    from test_gpu_net import TOLS as NET_TOLS, gcheck
    TOL, TOL_G, _ = NET_TOLS[gemm_mode]
    B, H, W = 2, 8, 12
    g = _gen('fstrn', T)
    net = FSTRN(k=3, nf=16, scale=1, nframes=T)
    fill_state_dict(net, 61)
    net.eval()
    x = torch.rand(B, T, 3, H, W, generator=g)
    gout = torch.randn(B, 3, H, W, generator=g)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in net.state_dict().items()}
    xr = x.double().requires_grad_(True)
    yr, prelus = _fstrn_ref(sd, xr, T)
    yr.backward(gout.double())
    gradmag = {k: (y.grad * z * (z <= 0)).abs().sum().item() for k, (z, y) in prelus.items()}

    net = net.to(dev())
    xg = x.to(dev()).requires_grad_(True)
    y = net(xg)
    y.backward(gout.to(dev()))
    torch.cuda.synchronize()
    check('T = %d out' % T, y, yr, TOL)
    gcheck(gemm_mode, 'T = %d grad_x' % T, xg.grad, xr.grad, TOL_G)
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        ref = sd[k].grad
        if k.endswith('.weight') and p.dim() == 5 and p.shape[2] == 3:
            # a temporal slice that meets no frame has an exactly-zero gradient on both sides; the others are held one by one
            for dt in range(3):
                if bool((ref[:, :, dt] == 0).all()):
                    assert bool((p.grad[:, :, dt] == 0).all()), '%s[:, :, %d] is not exactly 0' % (k, dt)
                else:
                    gcheck(gemm_mode, 'T = %d %s[:, :, %d]' % (T, k, dt), p.grad[:, :, dt], ref[:, :, dt], TOL_G)
            if T == 1:
                assert bool((ref[:, :, 0] == 0).all()) and bool((ref[:, :, 2] == 0).all()), k
        elif p.numel() == 1:
            # a PReLU slope, a sum of terms g * z * [z <= 0] of both signs: as test_gpu_fstrn.py holds the fixtures' slopes, to TOL_G of
            # its own value and to TOL_G of the sum of the terms' magnitudes
            err = abs(p.grad.item() - ref.item())
            print('%-44s got %+.6f ref %+.6f |err| %.3e = %.3e of the value, %.3e of the magnitude %.2f'
                  % (k, p.grad.item(), ref.item(), err, err / abs(ref.item()), err / gradmag[k], gradmag[k]))
            assert err <= TOL_G * abs(ref.item()) and err <= TOL_G * gradmag[k], k
        else:
            gcheck(gemm_mode, 'T = %d %s' % (T, k), p.grad, ref, TOL_G)
