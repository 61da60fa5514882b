"""TOF on the HIP path against the reference's TOF (fixtures tof.npz and tof_s4.npz, tests/golden/make_golden_tof.py): a training-mode forward + backward
(output, input gradient, the flow of every neighbour, the stored parameter gradients, the BatchNorm running statistics the step leaves),
then the eval forward on those statistics; and one training step of it through VideoSRModel.  -m gpu

TOLS / gcheck of tests/test_gpu_net.py.  The 7x7 convolutions are exact f32 in both GEMM modes; the 3x3 reconstruction follows the mode.
Measured on one MI355X, GEMM mode f32: outputs 1.2e-7 .. 2.0e-7, flows 1.5e-6 .. 3.0e-6, input gradient 1.5e-7 .. 2.3e-7, parameter
gradients <= 6e-6 (bounds 5e-5 / 5e-5 / 3e-4 / 3e-4): every quantity meets its bound in both modes.  The one kind held to another rule is
the bias of a conv in front of a training-mode BatchNorm (below): its exact gradient is zero."""
import pytest
import torch

from conftest import load_golden
from gpu_util import check, dev, gemm_modes
from test_gpu_net import TOLS, gcheck

gemm_mode = gemm_modes()
pytestmark = pytest.mark.gpu

# (constructor arguments, weight seed of the fixture)
CASES = {'k3': (dict(nframes=3, K=3, in_nc=3, out_nc=3, nf=32, nb=2, upscale=1), 378),
         'k2': (dict(nframes=3, K=2, in_nc=3, out_nc=3, nf=16, nb=1, upscale=1), 90),
         'k1s4': (dict(nframes=5, K=1, in_nc=3, out_nc=3, nf=16, nb=1, upscale=4), 3208)}
BN_STORED = ('align_arch.block0.block.1', 'align_arch.blocks.0.block.10')
# What a flipped ReLU looks like.  SpyNet has ~6e5 ReLU inputs per case and the closest to zero sits at 2e-7 (k2), 9e-7 (k1s4), 3e-6 (k3,
# bounded by the maker); the device forward is within ~1e-6 of the reference's.  Kernels that sum in another order (a bf16-split 7x7, a
# re-tiled f32 one) may put such an input on the other side of zero.  That is not an error of the kernels, and it has one signature: the
# outputs, the flows and the running statistics still pass at ~1e-6; so do the gradients of the layers BEHIND the BatchNorm named below
# (higher indices of its block, finer blocks, sr_arch); the gradients of that BatchNorm, of the layers in front of it in its block, of
# every coarser block, and the input gradient miss together, by 1e-3 .. 2e-1.  (Seed 90 did exactly this to k3 at
# align_arch.blocks.0.block.7.)  The cure is then another weight seed for that case in tests/golden/make_golden_tof.py, not a wider bound.
# A gradient that misses without this pattern -- alone, or with outputs or later layers off as well -- is a defect.
_KINK_NOTE = ('the ReLU input of this case closest to zero is %.2e from it, leaving %s: if every gradient behind that layer passes and those '
              'in front of it miss together while outputs and flows pass, a ReLU sign flipped (see the note above _KINK_NOTE)')


def _net(tag):
    from weights import fill_state_dict
    from realvsr_amd.archs.TOF_arch import TOF
    kw, seed = CASES[tag]
    net = TOF(**kw)
    fill_state_dict(net, seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.reset_running_stats()      # (the seeded fill draws negative variances)
    return net.to(dev())


@pytest.mark.parametrize('tag', list(CASES))
def test_tof_fixture(gemm_mode, tag):
    TOL, TOL_G, _ = TOLS[gemm_mode]
    g = {**load_golden('tof'), **load_golden('tof_s4')}      # (k3 and k2; k1s4)
    net = _net(tag).train()
    flows = []
    handle = net.align_arch.register_forward_hook(lambda mod, i, o: flows.append(o[1].detach()))
    x = torch.from_numpy(g[tag + '.x']).to(dev()).requires_grad_(True)
    out = net(x)
    out.backward(torch.from_numpy(g[tag + '.gout']).to(dev()))
    n_nbr = CASES[tag][0]['nframes'] - 1
    assert len(flows) == n_nbr
    check(tag + ' train out', out, torch.from_numpy(g[tag + '.train.out']), TOL)
    for j, f in enumerate(flows):
        check('%s flow %d' % (tag, j), f, torch.from_numpy(g['%s.train.flow.%d' % (tag, j)]), TOL)
    gcheck(gemm_mode, tag + ' train gx', x.grad, torch.from_numpy(g[tag + '.train.gx']), TOL_G)
    params = dict(net.named_parameters())
    keys = [k for k in g if k.startswith(tag + '.grad.')]
    assert len(keys) == len(params)
    for k in keys:
        ref = torch.from_numpy(g[k])
        got = params[k[len(tag) + 6:]].grad
        mag = g.get('%s.gradmag.%s' % (tag, k[len(tag) + 6:]))
        if mag is not None:
            # A conv bias in front of a training-mode BatchNorm: the gradient is zero in exact arithmetic (the batch mean is subtracted), the
            # reference's float32 leaves ~4e-7.  Channel c's is the sum of the conv's output gradient g over that channel; the fixture stores
            # that channel's sum |g| of the same run (float64), the scale the rounding of that sum lives on, and each channel's difference
            # is held to TOL_G times its own (the rule tests/test_gpu_fstrn.py applies to its slope gradients).
            err = (got.cpu().double() - ref.double()).abs()
            worst = int((err / torch.from_numpy(mag)).argmax())
            print('%-60s worst channel %d: |err| %.3e, |ref| %.3e, magnitude %.3e' % (k, worst, err[worst], ref[worst].abs(), mag[worst]))
            assert bool((err <= TOL_G * torch.from_numpy(mag)).all()), (k, worst, float(err[worst]), float(mag[worst]))
            continue
        try:
            gcheck(gemm_mode, k, got[:ref.shape[0]] if got.shape != ref.shape else got, ref, TOL_G)   # (conv weights: first 4 rows stored)
        except AssertionError as e:
            raise AssertionError('%s\n%s' % (e, _KINK_NOTE % (float(g[tag + '.min_preact'][0]), str(g[tag + '.min_preact_layer'])))) from None
    sd = net.state_dict()
    for name in BN_STORED:
        check('%s %s.running_mean' % (tag, name), sd[name + '.running_mean'], torch.from_numpy(g['%s.bn.%s.running_mean' % (tag, name)]), TOL)
        check('%s %s.running_var' % (tag, name), sd[name + '.running_var'], torch.from_numpy(g['%s.bn.%s.running_var' % (tag, name)]), TOL)
        assert int(sd[name + '.num_batches_tracked']) == int(g['%s.bn.%s.num_batches_tracked' % (tag, name)]) == n_nbr
    # the eval forward on the running statistics that step left
    net.eval()
    with torch.no_grad():
        out_eval = net(x.detach())
    handle.remove()
    check(tag + ' eval out', out_eval, torch.from_numpy(g[tag + '.eval.out']), TOL)
    assert (out_eval - out.detach()).abs().max().item() > 0.01        # (the two modes do differ)
    assert int(sd[BN_STORED[0] + '.num_batches_tracked']) == n_nbr    # (eval tracks nothing)


def _opt():
    # network_G and the criteria of train_TOF_RealVSR_YCbCr_Split.yml
    net = dict(which_model_G='TOF', nframes=3, K=3, nc=3, nf=64, nb=10)
    return {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
            'network_G': net, 'path': {'pretrain_model_G': None, 'strict_load': True},
            'train': {'pixel_criterion_y': 'lappyr', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0,
                      'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-4, 'beta1': 0.9, 'beta2': 0.99}}


def test_tof_training_step():
    """One VideoSRModel.optimize_parameters step with the option file's TOF: finite loss, every parameter and the running statistics
    moved; test() leaves the net in training mode and its output is an eval forward."""
    from realvsr_amd.VideoSR_model import create_model
    from realvsr_amd.archs.TOF_arch import TOF
    torch.cuda.set_device(0)
    torch.manual_seed(11)
    gen = torch.Generator().manual_seed(21)
    # 48 x 64: divisible by 2**K, and the low-pass band of the three-level pyramid, 12 x 16, holds the 11 x 11 SSIM window
    data = {'LQs': torch.rand(2, 3, 3, 48, 64, generator=gen), 'GT': torch.rand(2, 3, 3, 48, 64, generator=gen)}
    model = create_model(_opt())
    net = model.netG
    assert isinstance(net, TOF) and net.training
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert all(torch.isfinite(torch.tensor(v)) for v in log.values()) and log['l_pix'] > 0
    for k, p in net.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[k]), k
    for k, v in net.state_dict().items():
        if k.endswith('running_mean') or k.endswith('running_var'):
            assert torch.isfinite(v).all() and not torch.equal(v, before[k]), k
        elif k.endswith('num_batches_tracked'):
            assert int(v) == 2, k      # one SpyNet pass per neighbour
    model.test()
    assert net.training
    net.eval()
    with torch.no_grad():
        ref = net(data['LQs'].to(dev()))
    net.train()
    assert torch.equal(model.fake_H, ref)
    assert int(net.state_dict()[BN_STORED[0] + '.num_batches_tracked']) == 2
