"""Host-side checks of the GAN stage (no GPU): the discriminator's state_dict schema against the reference's, parameter counts,
and the refusals of VideoSRGANModel / define_D / GANLoss."""
import pytest
import torch

from conftest import load_golden


def _d_opt(nf=16, num_D=2, which='MultiscaleDiscriminator_v4'):
    return {'network_D': {'which_model_D': which, 'in_nc': 1, 'nf': nf, 'num_D': num_D, 'gan_type': 'patch'}}


def test_define_D_state_dict_matches_reference_schema():
    from realvsr_amd.VideoSR_archs import define_D
    g = load_golden('gan_step')
    sd = define_D(_d_opt()).state_dict()
    assert list(sd.keys()) == [str(k) for k in g['D.keys']]
    for (k, v), shp in zip(sd.items(), g['D.shapes']):
        assert list(v.shape) == [int(s) for s in shp[:v.dim()]] and all(int(s) == 0 for s in shp[v.dim():]), k
    assert sd['D_0.3.num_batches_tracked'].dtype == torch.int64


def test_discriminator_parameter_counts_and_layout():
    from realvsr_amd.VideoSR_archs import define_D
    from realvsr_amd.archs.discriminator_arch import PatchDiscriminator
    n64 = sum(p.numel() for p in define_D(_d_opt(nf=64)).parameters())
    assert n64 == 3286657 * 2
    assert sum(p.numel() for p in define_D(_d_opt(nf=16)).parameters()) == 414530
    assert len(define_D(_d_opt(nf=64)).state_dict()) == 80
    single = define_D(_d_opt(nf=64, which='PatchDiscriminator'))
    assert isinstance(single, PatchDiscriminator) and len(single.model) == 21
    convs = [m for m in single.model if isinstance(m, torch.nn.Conv2d)]
    assert [m.kernel_size for m in convs] == [(5, 5)] * 8 and [m.stride[0] for m in convs] == [1, 2, 1, 2, 1, 1, 1, 1]
    assert [m.bias is not None for m in convs] == [True] + [False] * 6 + [True]
    assert [m.out_channels for m in convs] == [64, 64, 64, 128, 128, 256, 256, 1]


def _gan_opt(**train):
    t = {'lr_G': 1e-3, 'beta1_G': 0.9, 'beta2_G': 0.99, 'lr_D': 1e-3, 'beta1_D': 0.9, 'beta2_D': 0.99, 'pixel_criterion_s': 'ssim',
         'pixel_weight_s': 1.0, 'pixel_criterion_d': 'cb', 'pixel_weight_d': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0,
         'feature_weight': 0, 'gan_type': 'ragan', 'gan_weight': 1e-4}
    t.update(train)
    opt = {'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'gpu_ids': [0], 'is_train': True, 'dist': False, 'scale': 1,
           'network_G': {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1,
                         'back_RBs': 1, 'w_TSA': False},
           'path': {'pretrain_model_G': None, 'strict_load': True}, 'train': t}
    opt.update(_d_opt())
    return opt


def test_gan_model_refusals(monkeypatch):
    from realvsr_amd.VideoSR_model import create_model
    # no CPU path, refused before any GAN key is read (an opt without network_D / train keys)
    with pytest.raises(NotImplementedError, match='no CPU path'):
        create_model({'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'gpu_ids': None, 'is_train': True, 'dist': False})
    with pytest.raises(NotImplementedError, match='no CPU path'):
        create_model(dict(_gan_opt(), gpu_ids=None))
    # the out-of-scope options are refused before any device is touched: reach them on a machine without a GPU too
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    with pytest.raises(NotImplementedError, match='distributed'):
        create_model(dict(_gan_opt(), dist=True))
    with pytest.raises(NotImplementedError, match='feature loss'):
        create_model(_gan_opt(feature_weight=1.0))
    for gt in ('lsgan', 'wgan-gp'):
        with pytest.raises(NotImplementedError, match='gan_type'):
            create_model(_gan_opt(gan_type=gt))


def test_define_D_and_gan_loss_refusals():
    from realvsr_amd.VideoSR_archs import define_D
    from realvsr_amd.loss import GANLoss
    from realvsr_amd.archs.discriminator_arch import MultiscaleDiscriminator_v4, PatchDiscriminator
    for which in ('discriminator_vgg_192', 'PixelDiscriminator', 'UNetDiscriminator', 'MultiscaleDiscriminator_v1'):
        with pytest.raises(NotImplementedError):
            define_D(_d_opt(which=which))
    with pytest.raises(NotImplementedError):
        MultiscaleDiscriminator_v4(1, 16, num_D=2, gan_type='pixel')
    with pytest.raises(NotImplementedError):
        PatchDiscriminator(1, 16, norm_layer=torch.nn.InstanceNorm2d)
    for gt in ('lsgan', 'wgan-gp', 'hinge'):
        with pytest.raises(NotImplementedError):
            GANLoss(gt, 1.0, 0.0)
    assert GANLoss('RaGAN').gan_type == 'ragan'


def test_gan_ops_refuse_cpu_tensors():
    from realvsr_amd import functional as RF
    from realvsr_amd.loss import GANLoss
    from realvsr_amd.archs.discriminator_arch import PatchDiscriminator
    with pytest.raises(NotImplementedError):
        GANLoss('ragan')(torch.zeros(2, 1, 4, 4), True, other=torch.zeros(2, 1, 4, 4))
    bn = torch.nn.BatchNorm2d(4)
    with pytest.raises(NotImplementedError):
        RF.batch_norm_lrelu(torch.zeros(2, 4, 3, 3), bn)
    with pytest.raises(NotImplementedError):
        PatchDiscriminator(1, 8)(torch.zeros(1, 1, 16, 16))
