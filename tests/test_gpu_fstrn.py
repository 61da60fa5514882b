"""FSTRN on the HIP path against the reference's FSTRN (fixture fstrn.npz, tests/golden/make_golden_fstrn.py) in eval mode and in
training mode with the recorded dropout mask injected, one training step of it through VideoSRModel, and eval after training.  -m gpu"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import check, dev, gemm_modes
from test_gpu_net import TOLS, gcheck

gemm_mode = gemm_modes()
pytestmark = pytest.mark.gpu

CASES = {'t3': dict(k=3, nf=64, scale=1, nframes=3), 't5': dict(k=3, nf=32, scale=1, nframes=5)}
# The one slope gradient that the three-term split does not bring within TOL_G of its own value: -0.015736, what is left of terms whose
# magnitudes sum to 64.776 (2.4e-4 of them).  Measured: |err| 1.62e-4 = 1.03e-2 of the value against the bound of 5e-3, 2.5e-6 of the
# magnitude -- the same absolute error as its neighbour frb_3 (1.71e-4 on +0.227, 7.5e-4 of the value); exact-f32 mode: 3.6e-6 of the value.
# It stays under the magnitude-scaled bound; the other eleven meet the relative bound singly in both modes.
BF16X3_CANCELLED = (('t3', 'frb_2.prelu.weight'),)


def _net(tag):
    from weights import fill_state_dict
    from realvsr_amd.archs.FSTRN_arch import FSTRN
    net = FSTRN(**CASES[tag])
    fill_state_dict(net, 61)
    return net.to(dev())


def _recorded_mask(g, tag):
    """The fixture's keep mask, from the reference's [B, C, T, H, W] to frame-major [T, B, C, H, W]."""
    shape = [int(n) for n in g[tag + '.train.keep_shape']]
    keep = np.unpackbits(g[tag + '.train.keep'], count=int(np.prod(shape))).reshape(shape).astype(bool)
    return torch.from_numpy(keep).permute(2, 0, 1, 3, 4).contiguous().to(dev())


@pytest.mark.parametrize('mode', ['eval', 'train'])
@pytest.mark.parametrize('tag', ['t3', 't5'])
def test_fstrn_fixture(gemm_mode, tag, mode):
    TOL, TOL_G, _ = TOLS[gemm_mode]
    g = load_golden('fstrn')
    net = _net(tag).train(mode == 'train')
    if mode == 'train':
        keep = _recorded_mask(g, tag)
        assert 0.65 <= keep.float().mean().item() <= 0.75
        net.dropout_keep_mask = lambda like: keep
    else:
        net.dropout_keep_mask = None   # eval draws no mask
    x = torch.from_numpy(g[tag + '.x']).to(dev()).requires_grad_(True)
    out = net(x)
    out.backward(torch.from_numpy(g[tag + '.gout']).to(dev()))
    check('%s %s out' % (tag, mode), out, torch.from_numpy(g['%s.%s.out' % (tag, mode)]), TOL)
    gcheck(gemm_mode, '%s %s gx' % (tag, mode), x.grad, torch.from_numpy(g['%s.%s.gx' % (tag, mode)]), TOL_G)
    if mode == 'train':   # the stored parameter gradients are those of the training run
        params = dict(net.named_parameters())
        keys = [k for k in g if k.startswith(tag + '.grad.')]
        assert sum(k.endswith('prelu.weight') for k in keys) == 6 and sum(k.endswith('.bias') for k in keys) == 14 and len(keys) == 28
        for k in keys:
            if k.endswith('prelu.weight'):
                continue   # (below)
            ref = torch.from_numpy(g[k])
            got = params[k[len(tag) + 6:]].grad
            gcheck(gemm_mode, k, got[:ref.shape[0]] if got.shape != ref.shape else got, ref, TOL_G)   # (large weights: first 16 rows stored)
        # Every slope gradient singly, by gcheck's rule for a one-element tensor (|err| <= TOL_G * |ref|) in both modes, except the entry of
        # BF16X3_CANCELLED under the three-term split.  Each is a sum of 4e4 .. 3e5 terms g * x * [x <= 0] of both signs; the fixture stores
        # the sum of their magnitudes next to it (gradmag.*), the scale the rounding of such a sum lives on, and every one -- the exception
        # included -- is also held to TOL_G times that.
        worst = []
        for k in (k for k in keys if k.endswith('prelu.weight')):
            name = k[len(tag) + 6:]
            got, ref, mag = params[name].grad.item(), float(g[k][0]), float(g['%s.gradmag.%s' % (tag, name)][0])
            err = abs(got - ref)
            print('%-44s got %+.6f ref %+.6f |err| %.3e = %.3e of the value, %.3e of the magnitude %.2f'
                  % (k, got, ref, err, err / abs(ref), err / mag, mag))
            if err > TOL_G * mag:
                worst.append((k, 'magnitude', err / mag))
            if (gemm_mode == 'f32' or (tag, name) not in BF16X3_CANCELLED) and err > TOL_G * abs(ref):
                worst.append((k, 'value', err / abs(ref)))
        assert not worst, worst


def test_eval_after_training_is_the_eval_fixture(gemm_mode):
    TOL = TOLS[gemm_mode][0]
    g = load_golden('fstrn')
    net = _net('t5')
    x = torch.from_numpy(g['t5.x']).to(dev())
    with torch.no_grad():
        net.train()
        dropped = net(x)
        net.eval()
        out = net(x)
    check('t5 eval after train', out, torch.from_numpy(g['t5.eval.out']), TOL)
    assert (dropped - out).abs().max().item() > 0.01   # (the training forward did drop)


def _opt():
    net = dict(which_model_G='FSTRN', k=3, nf=64, nframes=3)
    return {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
            'network_G': net, 'path': {'pretrain_model_G': None, 'strict_load': True},
            'train': {'pixel_criterion_y': 'cb', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 0.5,
                      'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-3, 'beta1': 0.9, 'beta2': 0.99}}


def test_fstrn_training_step():
    """One VideoSRModel.optimize_parameters step with an FSTRN generator under a fixed torch seed (the dropout mask is drawn on the
    device): finite loss, every parameter moved, and the same parameters bit for bit as the step driven by hand under the same seed
    (forward, the two criteria, backward, FlatAdam) -- nothing in this network is atomic."""
    from weights import fill_state_dict
    from realvsr_amd import loss as L
    from realvsr_amd.VideoSR_archs import define_G
    from realvsr_amd.VideoSR_model import create_model
    from realvsr_amd.archs.FSTRN_arch import FSTRN
    from realvsr_amd.optim import FlatAdam
    torch.cuda.set_device(0)
    gen = torch.Generator().manual_seed(21)
    data = {'LQs': torch.rand(2, 3, 3, 32, 48, generator=gen), 'GT': torch.rand(2, 3, 3, 32, 48, generator=gen)}
    opt = _opt()
    model = create_model(opt)
    assert isinstance(model.netG, FSTRN) and model.netG.training
    fill_state_dict(model.netG, 61)              # in-place copy: parameters stay inside the flat buffer
    model.optimizer_G.buffers.check_bound()
    before = {k: v.detach().clone() for k, v in model.netG.named_parameters()}
    model.feed_data(data)
    torch.manual_seed(33)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert all(torch.isfinite(torch.tensor(v)) for v in log.values()) and log['l_pix'] > 0
    for k, p in model.netG.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[k]), k

    net = define_G(opt)
    fill_state_dict(net, 61)
    net = net.to(dev()).train()
    optim = FlatAdam([p for p in net.parameters()], lr=1e-3, weight_decay=0, betas=(0.9, 0.99))
    optim.zero_grad()
    lq, gt = data['LQs'].to(dev()), data['GT'].to(dev())[:, 1]
    torch.manual_seed(33)
    fake = net(lq)
    loss = 1.0 * L.CharbonnierLoss(reduction='mean')(fake[:, 0:1], gt[:, 0:1]) + 0.5 * L.GWLoss(w=4, reduction='mean')(fake[:, 1:3], gt[:, 1:3])
    loss.backward()
    optim.step()
    assert loss.item() == log['l_pix']
    for (k, p), q in zip(model.netG.named_parameters(), net.parameters()):
        assert torch.equal(p.detach(), q.detach()), k


def test_frb_computes_what_is_asked_for():
    """An FRB whose input or parameters want no gradient: the gradients that remain are bit for bit those of the full backward, the
    others are absent (the node skips the passes behind them)."""
    from realvsr_amd.archs.FSTRN_arch import FRB
    gen = torch.Generator().manual_seed(4)
    blk, nxt = FRB(3, 16).to(dev()), torch.nn.PReLU().to(dev())
    x0 = torch.randn(3, 2, 16, 8, 16, generator=gen).to(dev())
    gout, gpout = torch.randn(x0.shape, generator=gen).to(dev()), torch.randn(x0.shape, generator=gen).to(dev())
    names = [n for n, _ in blk.named_parameters()]

    def run(x_grad, frozen):
        for n, p in blk.named_parameters():
            p.grad = None
            p.requires_grad_(not n.startswith(frozen))
        nxt.weight.grad = None
        x = x0.clone().requires_grad_(x_grad)
        out, pout = blk(x, next_prelu=nxt)
        torch.autograd.backward([out, pout], [gout, gpout])
        got = {n: p.grad for n, p in blk.named_parameters()}
        got.update(x=x.grad, nxt=nxt.weight.grad)
        return got

    full = run(True, ('none',))
    assert all(full[n] is not None for n in names + ['x', 'nxt'])
    for x_grad, frozen in ((False, ('none',)), (False, ('prelu', 'conv3d_1')), (True, ('conv3d_1', 'conv3d_2')), (False, ('prelu',)),
                           (True, ('conv3d_2.weight',))):
        got = run(x_grad, frozen)
        for n in names + ['x', 'nxt']:
            wanted = x_grad if n == 'x' else not n.startswith(frozen)
            assert (got[n] is not None) == wanted, (x_grad, frozen, n)
            if wanted:
                assert torch.equal(got[n], full[n]), (x_grad, frozen, n)


def test_a_slope_per_channel_is_refused_on_the_device():
    from realvsr_amd import functional as RF
    x = torch.randn(3, 1, 16, 4, 8, device=dev())
    with pytest.raises(NotImplementedError, match='one slope'):
        RF.prelu(x, torch.nn.PReLU(16).to(dev()))
