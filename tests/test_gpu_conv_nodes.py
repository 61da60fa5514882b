"""The fused conv nodes of functional.py -- res_block, a grad_premasked / x_premask pair, conv_cat_bcast -- vs torch CPU float64, on
frames the 8 x 64 mask epilogue takes and on frames it does not.  -m gpu

Kink-free by construction.  The conv whose *hidden* activation decides a gradient mask (conv1 of res_block, the producer of a pair)
gets integer inputs in [-4, 4], weights that are integers / 8 in [-1, 1] and a bias of odd multiples of 1/16: every product and every
partial sum is exact in f32 and in every operand format of the GEMM modes (<= 4 significant bits), and the pre-activation is an odd
multiple of 1/16 -- never within 1/16 of the kink, so float64 and the GPU take the same mask and the tolerance can stay at the block
tests'.  The slope of such an activation is 1/8, so the activation output is exact too and is compared bit for bit where it is
visible.  Everything downstream is ordinary random floats.

Tolerances: TOLS[mode] of test_gpu_conv.py for a quantity one split GEMM away from exact inputs, twice that for one that passes through
two (first-order errors add): res_block's grad_x and conv1 gradients, a pair's producer gradients."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from gpu_util import check, dev, gemm_modes
from test_gpu_conv import TOLS

pytestmark = pytest.mark.gpu
gemm_mode = gemm_modes()
SLOPE = 0.125   # of the kink-free activations (exact in every format)

# frames of the 8 x 64 tile's mask epilogue: px(8 x 64 tiles) <= px(16 x 32 tiles), W % 4 == 0 (csrc/conv_plan.h)
TAKEN = [(8, 64), (7, 64), (17, 60), (8, 68), (16, 40)]      # a ragged last row, a ragged last column tile
NOT_TAKEN = [(16, 24), (9, 68), (8, 62)]

# (C, B, H, W)
RES_BLOCKS = [(64, 1, 8, 64), (64, 1, 7, 64), (64, 1, 17, 60), (64, 1, 8, 68), (64, 2, 16, 40), (64, 1, 16, 24), (64, 1, 9, 68),
              (64, 1, 8, 62), (16, 1, 8, 64)]
# (producer, consumer): block cases (C1, C2, Co, k, stride, act, residual, pixel_shuffle, B, H, W), or a ('bcast', C1, C2, Co, act, N, B,
# H, W, x_sink, ref_sink) producer; the consumer runs on the producer's output
PAIRS = [
    ((64, 0, 64, 3, 1, 'lrelu', False, False, 1, 8, 64), (64, 0, 64, 3, 1, 'none', False, False, 1, 8, 64)),
    ((64, 0, 64, 3, 1, 'lrelu', False, False, 1, 17, 60), (64, 0, 64, 3, 1, 'lrelu', False, False, 1, 17, 60)),    # act' + mask, ragged
    ((64, 0, 64, 3, 1, 'relu', False, False, 2, 16, 40), (64, 0, 3, 3, 1, 'none', True, False, 2, 16, 40)),        # conv_last: residual
    ((64, 0, 64, 3, 1, 'lrelu', False, False, 1, 9, 68), (64, 0, 64, 3, 1, 'lrelu', False, False, 1, 9, 68)),      # not taken
    ((64, 0, 256, 3, 1, 'lrelu', False, True, 1, 4, 32), (64, 0, 64, 3, 1, 'lrelu', False, False, 1, 8, 64)),      # upconv2 -> HRconv
    ((16, 0, 64, 3, 1, 'lrelu', False, True, 1, 8, 12), (16, 0, 16, 3, 1, 'none', False, False, 1, 16, 24)),       # not taken
    ((64, 64, 64, 3, 1, 'lrelu', False, False, 1, 7, 64), (64, 0, 64, 3, 1, 'none', False, False, 1, 7, 64)),      # concat producer
    (('bcast', 64, 64, 64, 'lrelu', 3, 1, 8, 68, None, None), (64, 0, 64, 3, 1, 'none', False, False, 3, 8, 68)),
]
# (C1, C2, Co, act, N, B, H, W, x_sink, ref_sink): x_sink None / 'dep' / 'own', ref_sink None or the block of the sink's tensor that is ref
BCAST_CASES = [
    (64, 64, 64, 'lrelu', 3, 1, 8, 36, None, None),
    (16, 16, 16, 'none', 1, 2, 9, 20, None, None),
    (64, 64, 64, 'relu', 5, 1, 8, 12, 'dep', None),
    (16, 16, 32, 'lrelu', 3, 2, 8, 12, 'own', None),
    (64, 64, 64, 'none', 3, 1, 7, 30, None, 1),
    (16, 16, 16, 'relu', 5, 2, 5, 8, 'dep', 2),
]


def _ids(cases):
    return ['-'.join(str(v) for v in c).replace(' ', '').replace("'", '') for c in cases]


def _exact_conv(Co, Ci, g):
    """(weight, bias) whose products with small integers are exact: integers / 8 in [-1, 1], odd multiples of 1 / 16."""
    w = torch.randint(-8, 9, (Co, Ci, 3, 3), generator=g).float() / 8
    b = (2 * torch.randint(-8, 8, (Co,), generator=g) + 1).float() / 16
    return w, b


def _float_conv(Co, Ci, g):
    return torch.randn(Co, Ci, 3, 3, generator=g) / (3.0 * Ci ** 0.5), torch.randn(Co, generator=g) * 0.1


def _ints(shape, g):
    return torch.randint(-4, 5, shape, generator=g).float()


def _kink_free(x, w, b):
    """The pre-activation of an exact conv in float64; asserts that it keeps 1/16 from the kink and that f32 reproduces it exactly."""
    z = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert z.abs().min().item() >= 1.0 / 16
    assert torch.equal(F.conv2d(x, w, b, padding=1).double(), z)
    return z


def _holder(w, b, d):
    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    return conv.to(d)


def _act64(z, act, slope):
    return F.relu(z) if act == 'relu' else F.leaky_relu(z, slope) if act == 'lrelu' else z


def test_frames_of_the_mask_epilogue(gemm_mode):
    from realvsr_amd import functional as RF
    for H, W in TAKEN:
        assert RF.grad_mask_fusable(H, W) is (gemm_mode != 'f32'), (H, W)   # (the exact-f32 mode has no mask epilogue)
    for H, W in NOT_TAKEN:
        assert RF.grad_mask_fusable(H, W) is False, (H, W)


def _res_block_case(geo, gemm_mode, frozen=()):
    """x + conv2(relu(conv1(x))) against float64: the output and the five gradients; those of the inputs named in `frozen` (of x, w1,
    b1, w2, b2), which do not require one, must be None."""
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    C, B, H, W = geo
    g = torch.Generator().manual_seed(1000 * H + W + C)
    x = _ints((B, C, H, W), g)
    w1, b1 = _exact_conv(C, C, g)
    w2, b2 = _float_conv(C, C, g)
    gout = torch.randn(B, C, H, W, generator=g)
    _kink_free(x, w1, b1)

    r = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    yr = r[0] + F.conv2d(F.relu(F.conv2d(r[0], r[1], r[2], padding=1)), r[3], r[4], padding=1)
    yr.backward(gout.double())

    d = dev()
    c1, c2 = _holder(w1, b1, d), _holder(w2, b2, d)
    xg = x.to(d)
    leaves = {'x': xg, 'w1': c1.weight, 'b1': c1.bias, 'w2': c2.weight, 'b2': c2.bias}
    for k, t in leaves.items():
        t.requires_grad_(k not in frozen)
    y = RF.res_block(xg, c1, c2)
    y.backward(gout.to(d))
    torch.cuda.synchronize()
    check('out', y, yr, TOL)
    for k, ref, tol in (('w2', r[3], TOL), ('b2', r[4], TOL), ('x', r[0], 2 * TOL), ('w1', r[1], 2 * TOL), ('b1', r[2], 2 * TOL)):
        if k in frozen:
            assert leaves[k].grad is None, k
        else:
            check('grad_' + k, leaves[k].grad, ref.grad, tol)


@pytest.mark.parametrize('geo', RES_BLOCKS, ids=_ids(RES_BLOCKS))
def test_res_block_vs_float64(geo, gemm_mode):
    """x + conv2(relu(conv1(x))): the output and all five gradients."""
    _res_block_case(geo, gemm_mode)


# which inputs of a conv1 + ReLU, conv2 node need no gradient: the backward chain of res_block and rcab skips what only they need
FROZEN = {'x': ('x',), 'conv1': ('w1', 'b1'), 'conv2': ('w2', 'b2')}


@pytest.mark.parametrize('frozen', list(FROZEN))
def test_res_block_frozen_inputs_vs_float64(frozen, gemm_mode):
    """needs_input_grad of the node: x without a gradient (no dgrad1), conv1 frozen (no wgrad1), conv2 frozen (no wgrad2); the
    gradients still wanted are what they were, the others None."""
    _res_block_case((16, 1, 8, 12), gemm_mode, FROZEN[frozen])


def _bcast_ref(x, ref, w, b, N, act, slope):
    return _act64(F.conv2d(torch.cat([x, ref.repeat(N, 1, 1, 1)], 1), w, b, padding=1), act, slope)


@pytest.mark.parametrize('pair', PAIRS, ids=_ids(PAIRS))
def test_premask_pair_vs_float64(pair, gemm_mode):
    """conv2d(..., grad_premasked=True) -> conv2d(..., x_premask=...): the producer's output bit for bit, the consumer's output and
    gradients, the producer's gradients (which the consumer masked)."""
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    prod, cons = pair
    g = torch.Generator().manual_seed(zlib.crc32(repr(pair).encode()))
    code = {'none': RF.ACT_NONE, 'relu': RF.ACT_RELU, 'lrelu': RF.ACT_LRELU}
    d = dev()
    bcast = prod[0] == 'bcast'
    if bcast:
        _, C1, C2, Cp, pact, N, B, H, W, _, _ = prod
        ps = False
        ins = [_ints((N * B, C1, H, W), g), _ints((B, C2, H, W), g)]
    else:
        C1, C2, Cp, _, _, pact, _, ps, B, H, W = prod
        ins = [_ints((B, C1, H, W), g)] + ([_ints((B, C2, H, W), g)] if C2 else [])
    wp, bp = _exact_conv(Cp, C1 + C2, g)
    Cc, _, Co, _, _, cact, cres, _, Bc, Hc, Wc = cons
    wc, bc = _float_conv(Co, Cc, g)
    res = torch.randn(Bc, Co, Hc, Wc, generator=g) if cres else None
    gout = torch.randn(Bc, Co, Hc, Wc, generator=g)
    xcat = torch.cat([ins[0], ins[1].repeat(N, 1, 1, 1)], 1) if bcast else torch.cat(ins, 1)
    _kink_free(xcat, wp, bp)

    r = [t.double().requires_grad_(True) for t in ins + [wp, bp, wc, bc]]
    rin, (rwp, rbp, rwc, rbc) = r[:len(ins)], r[len(ins):]
    zp = F.conv2d(torch.cat([rin[0], rin[1].repeat(N, 1, 1, 1)], 1) if bcast else torch.cat(rin, 1), rwp, rbp, padding=1)
    pr = _act64(F.pixel_shuffle(zp, 2) if ps else zp, pact, SLOPE)
    zc = F.conv2d(pr, rwc, rbc, padding=1)
    if cact != 'none':   # the consumer's own activation is an ordinary one: keep the comparison away from its kink, as the block tests do
        gout = gout * (zc.detach().abs() > 1e-3).float()
    yr = _act64(zc, cact, 0.1)
    rres = None
    if cres:
        rres = res.double().requires_grad_(True)
        yr = yr + rres
    yr.backward(gout.double())

    convp, convc = _holder(wp, bp, d), _holder(wc, bc, d)
    t = [v.to(d).requires_grad_(True) for v in ins]
    if bcast:
        p = RF.conv_cat_bcast(t[0], t[1], convp, N, code[pact], SLOPE, grad_premasked=True)
    else:
        p = RF.conv2d(t[0], convp, code[pact], SLOPE, x2=t[1] if C2 else None, pixel_shuffle=ps, grad_premasked=True)
    tres = res.to(d).requires_grad_(True) if cres else None
    y = RF.conv2d(p, convc, code[cact], 0.1, residual=tres, x_premask=(code[pact], SLOPE))
    y.backward(gout.to(d))
    torch.cuda.synchronize()
    assert torch.equal(p.detach().cpu().double(), pr.detach()), 'the producer output of exact operands is not exact'
    check('out', y, yr, TOL)
    check('consumer grad_weight', convc.weight.grad, rwc.grad, TOL)
    check('consumer grad_bias', convc.bias.grad, rbc.grad, TOL)
    if cres:
        check('grad_res', tres.grad, rres.grad, TOL)
    for name, got, want in zip(('x1', 'x2'), t, rin):
        check('producer grad_' + name, got.grad, want.grad, 2 * TOL)
    check('producer grad_weight', convp.weight.grad, rwp.grad, 2 * TOL)
    check('producer grad_bias', convp.bias.grad, rbp.grad, 2 * TOL)


def test_premask_refusals():
    """What _Conv2dFused.forward refuses: x_premask with a second input, a GradSink, PixelShuffle or a stride; grad_premasked without an
    activation or with a residual."""
    from realvsr_amd import functional as RF
    d = dev()
    x = torch.randn(1, 16, 8, 12, device=d)
    conv, cat, s2 = (torch.nn.Conv2d(ci, 16, 3, s, 1).to(d) for ci, s in ((16, 1), (32, 1), (16, 2)))
    pm = (RF.ACT_LRELU, 0.1)
    for kw, c in ((dict(x2=x), cat), (dict(sink=RF.GradSink()), conv), (dict(dep_sink=RF.GradSink()), conv), (dict(pixel_shuffle=True), conv),
                  (dict(), s2)):
        with pytest.raises(RuntimeError, match='x_premask'):
            RF.conv2d(x, c, RF.ACT_NONE, x_premask=pm, **kw)
    with pytest.raises(RuntimeError, match='grad_premasked'):
        RF.conv2d(x, conv, RF.ACT_NONE, grad_premasked=True)
    with pytest.raises(RuntimeError, match='grad_premasked'):
        RF.conv2d(x, conv, RF.ACT_LRELU, residual=torch.randn(1, 16, 8, 12, device=d), grad_premasked=True)
    with pytest.raises(RuntimeError, match='grad_premasked'):
        RF._Conv2dFused.apply(x, None, conv.weight, conv.bias, torch.randn(1, 16, 8, 12, device=d), 1, RF.ACT_LRELU, 0.1, False, None, None,
                              None, True)


@pytest.mark.parametrize('case', BCAST_CASES, ids=_ids(BCAST_CASES))
def test_conv_cat_bcast_vs_float64(case, gemm_mode):
    """act(conv(cat([x, ref.repeat(N, 1, 1, 1)], 1))): output, gradients of x, ref, the full weight and the bias; a GradSink of x that
    this conv deposits into or owns (holding an earlier deposit either way), a ref_sink whose block is ref."""
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    C1, C2, Co, act, N, B, H, W, x_sink, ref_sink = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    x, ref = torch.randn(N * B, C1, H, W, generator=g), torch.randn(B, C2, H, W, generator=g)
    w, b = _float_conv(Co, C1 + C2, g)
    gout = torch.randn(N * B, Co, H, W, generator=g)
    held_x = torch.randn(x.shape, generator=g)                   # what another consumer of x deposited before
    held_ref = torch.randn(N * B, C2, H, W, generator=g)         # the sink of the tensor whose block ref_sink is ref
    r = [t.double().requires_grad_(True) for t in (x, ref, w, b)]
    if act != 'none':
        with torch.no_grad():
            gout = gout * (_bcast_ref(*r, N, 'none', 0.1).abs() > 1e-3).float()
    yr = _bcast_ref(*r, N, act, 0.1)
    yr.backward(gout.double())

    d = dev()
    conv = _holder(w, b, d)
    xg, refg = x.to(d).requires_grad_(True), ref.to(d).requires_grad_(True)
    xs = rs = None
    if x_sink:
        xs = RF.GradSink()
        xs.buf = held_x.to(d)
    if ref_sink is not None:
        rs = RF.GradSink((N * B, C2, H, W))
        rs.buf = held_ref.to(d)
    code = {'none': RF.ACT_NONE, 'relu': RF.ACT_RELU, 'lrelu': RF.ACT_LRELU}[act]
    y = RF.conv_cat_bcast(xg, refg, conv, N, code, 0.1, x_sink=xs, x_owner=x_sink == 'own', ref_sink=rs, ref_block=ref_sink or 0)
    y.backward(gout.to(d))
    torch.cuda.synchronize()
    check('out', y, yr, TOL)
    if x_sink == 'dep':      # deposited: autograd sees no gradient, the sink holds the sum and stays open for its owner
        assert xg.grad is None and not xs.closed
        check('x_sink', xs.buf, held_x.double() + r[0].grad, TOL)
    elif x_sink == 'own':    # the owner closes the sink and returns the sum
        assert xs.closed and xs.buf is None
        check('grad_x + deposit', xg.grad, held_x.double() + r[0].grad, TOL)
    else:
        check('grad_x', xg.grad, r[0].grad, TOL)
    if ref_sink is not None:
        assert refg.grad is None and not rs.closed
        want = held_ref.double().clone()
        want[ref_sink * B:(ref_sink + 1) * B] += r[1].grad
        check('ref_sink', rs.buf, want, TOL)
        other = torch.ones(N * B, dtype=torch.bool)
        other[ref_sink * B:(ref_sink + 1) * B] = False
        assert torch.equal(rs.buf.cpu()[other], held_ref[other]), 'a block of the sink that is not ref was written'
    else:
        check('grad_ref', refg.grad, r[1].grad, TOL)
    check('grad_weight', conv.weight.grad, r[2].grad, TOL)
    check('grad_bias', conv.bias.grad, r[3].grad, TOL)
