"""RCAN on the HIP path against the reference's RCAN (fixture rcan.npz, tests/golden/make_golden_rcan.py), and one training step of it
through VideoSRModel.  -m gpu"""
import pytest
import torch

from conftest import load_golden
from gpu_util import check, dev, gemm_modes
from test_gpu_net import TOLS, gcheck

gemm_mode = gemm_modes()
pytestmark = pytest.mark.gpu

CASES = {'s1': dict(num_feat=64, squeeze_factor=16, num_group=2, num_block=2, upscale=1, res_scale=1),
         's2': dict(num_feat=32, squeeze_factor=8, num_group=2, num_block=2, upscale=2, res_scale=0.5)}


def fill_rcan(net):
    """The fixture's weights: the seeded fill, then the attention convs times 30 so that the gates span (0, 1)."""
    from weights import fill_state_dict
    fill_state_dict(net, 51)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if '.attention.' in name:
                p.mul_(30.0)
    return net


@pytest.mark.parametrize('tag', ['s1', 's2'])
def test_rcan_fixture(gemm_mode, tag):
    TOL, TOL_G, _ = TOLS[gemm_mode]
    from realvsr_amd.archs.RCAN_arch import RCAN
    g = load_golden('rcan')
    net = fill_rcan(RCAN(num_in_ch=3, num_out_ch=3, num_frames=3, **CASES[tag])).to(dev())
    out = net(torch.from_numpy(g[tag + '.x']).to(dev()))
    out.backward(torch.from_numpy(g[tag + '.gout']).to(dev()))
    check(tag + ' out', out, torch.from_numpy(g[tag + '.out']), TOL)
    params = dict(net.named_parameters())
    keys = [k for k in g if k.startswith(tag + '.grad.')]
    assert sum('.attention.' in k for k in keys) == 16 and len(keys) >= 16 + 14
    for k in keys:
        ref = torch.from_numpy(g[k])
        got = params[k[len(tag) + 6:]].grad
        gcheck(gemm_mode, k, got[:ref.shape[0]] if got.shape != ref.shape else got, ref, TOL_G)   # (large weights: first 16 rows stored)


def _opt():
    net = dict(which_model_G='RCAN', num_in_ch=3, num_out_ch=3, num_frames=3, num_feat=64, num_group=1, num_block=1, squeeze_factor=16,
               res_scale=1)
    return {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
            'network_G': net, 'path': {'pretrain_model_G': None, 'strict_load': True},
            'train': {'pixel_criterion_y': 'cb', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 0.5,
                      'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-3, 'beta1': 0.9, 'beta2': 0.99}}


def test_rcan_training_step():
    """One VideoSRModel.optimize_parameters step with an RCAN generator: finite loss, every parameter moved, and the same parameters
    bit for bit as the step driven by hand (forward, the two criteria, backward, FlatAdam) -- nothing in this network is atomic."""
    from realvsr_amd import loss as L
    from realvsr_amd.VideoSR_archs import define_G
    from realvsr_amd.VideoSR_model import create_model
    from realvsr_amd.archs.RCAN_arch import RCAN
    from realvsr_amd.optim import FlatAdam
    torch.cuda.set_device(0)
    gen = torch.Generator().manual_seed(21)
    data = {'LQs': torch.rand(2, 3, 3, 32, 48, generator=gen), 'GT': torch.rand(2, 3, 3, 32, 48, generator=gen)}
    opt = _opt()
    model = create_model(opt)
    assert isinstance(model.netG, RCAN)
    fill_rcan(model.netG)                        # in-place copy: parameters stay inside the flat buffer
    model.optimizer_G.buffers.check_bound()
    before = {k: v.detach().clone() for k, v in model.netG.named_parameters()}
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert all(torch.isfinite(torch.tensor(v)) for v in log.values()) and log['l_pix'] > 0
    for k, p in model.netG.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[k]), k

    net = fill_rcan(define_G(opt)).to(dev()).train()
    optim = FlatAdam([p for p in net.parameters()], lr=1e-3, weight_decay=0, betas=(0.9, 0.99))
    optim.zero_grad()
    fake = net(data['LQs'].to(dev()))
    gt = data['GT'].to(dev())[:, 1]
    loss = 1.0 * L.CharbonnierLoss(reduction='mean')(fake[:, 0:1], gt[:, 0:1]) + 0.5 * L.GWLoss(w=4, reduction='mean')(fake[:, 1:3], gt[:, 1:3])
    loss.backward()
    optim.step()
    assert loss.item() == log['l_pix']
    for (k, p), q in zip(model.netG.named_parameters(), net.parameters()):
        assert torch.equal(p.detach(), q.detach()), k
