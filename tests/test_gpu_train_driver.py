"""The training driver on the device: the schedule reaches the Adam kernel, a checkpoint resumes exactly and continues on the
uninterrupted run's path, the .state interchanges with torch.optim.Adam, the clip-wise validation equals the frame-wise loop, and
realvsr_amd.train.main trains, validates, checkpoints and resumes on a synthetic RealVSR tree.

Tiny networks (one residual block each; EDVR at nf 16, EDVR_NoUp at the nf 64 it is built for), batch 2, 16 x 16 LR frames (48 x 64 for
the GAN model: its recorded batch), Charbonnier criteria, f32 GEMM mode."""
import copy
import glob
import os
import pickle
import re

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

G = load_golden('lr_schedules')
THREE = {'lr_scheme': 'CosineAnnealingLR_Restart', 'T_period': [50, 30, 40], 'restarts': [50, 80], 'restart_weights': [1, 0.5],
         'eta_min': 1e-7}
BASE = 2e-4      # the rate the 'three_lr' fixture was recorded with


@pytest.fixture(autouse=True)
def f32_mode():
    from realvsr_amd import _lib
    old = _lib.get_gemm_mode()
    _lib.set_gemm_mode('f32')
    torch.cuda.set_device(0)
    yield
    _lib.set_gemm_mode(old)


def _sr_opt(root=None, lr=BASE, **train):
    net = dict(which_model_G='EDVR', nf=16, nc=3, nframes=3, groups=4, front_RBs=1, back_RBs=1, center=None, predeblur=False,
               HR_in=False, w_TSA=True)
    t = {'pixel_criterion_y': 'cb', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'cb', 'pixel_weight_c': 0.5, 'weight_decay_G': 0,
         'ft_tsa_only': 0, 'lr_G': lr, 'beta1': 0.9, 'beta2': 0.99}
    t.update(train)
    path = {'pretrain_model_G': None, 'strict_load': True}
    if root is not None:
        path.update(models=os.path.join(str(root), 'models'), training_state=os.path.join(str(root), 'training_state'),
                    val_images=os.path.join(str(root), 'val_images'))
        for k in ('models', 'training_state', 'val_images'):
            os.makedirs(path[k], exist_ok=True)
    return {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 4, 'augment': None,
            'network_G': net, 'path': path, 'train': t}


def _sr_model(opt):
    from realvsr_amd.VideoSR_model import create_model
    from weights import fill_state_dict
    model = create_model(opt)
    if opt['path'].get('pretrain_model_G') is None:
        fill_state_dict(model.netG, 808, offset_std=0.02)       # in place: the parameters stay in the flat buffer
    model.optimizer_G.buffers.check_bound()
    return model


def _batches(n, hr=(64, 64), lr_hw=(16, 16), seed=5):
    gen = torch.Generator().manual_seed(seed)
    return [{'LQs': torch.rand(2, 3, 3, *lr_hw, generator=gen), 'GT': torch.rand(2, 3, *hr, generator=gen)} for _ in range(n)]


def _steps(model, batches, first):
    for k, batch in enumerate(batches):
        model.update_learning_rate(first + k, warmup_iter=-1)
        model.feed_data(batch)
        model.optimize_parameters(first + k, log=False)


def _flat(optimizer):
    return optimizer.buffers.param.detach().clone()


# ---------------------------------------------------------------------------------------------------------------- the schedule
def test_schedule_reaches_the_param_groups():
    model = _sr_model(_sr_opt(**THREE))
    assert len(model.schedulers) == 1 and model.get_current_learning_rate() == [BASE]
    worst = 0.0
    for k in range(1, 91):
        model.update_learning_rate(k)
        got = [g['lr'] for g in model.optimizer_G.param_groups]
        worst = max(worst, abs(got[0] - G['three_lr'][k]) / BASE)
        assert model.get_current_learning_rate() == got
    print('largest deviation %.3g * base_lr' % worst)
    assert worst <= 1e-12
    assert model.optimizer_G.param_groups[0]['lr'] < 0.5 * BASE and model.schedulers[0].last_restart == 81
    assert _sr_model(_sr_opt()).schedulers == []        # no lr_scheme: as before
    with pytest.raises(NotImplementedError):
        _sr_model(_sr_opt(lr_scheme='MultiStepLR'))      # (the GAN constructor's spelling)


def test_first_step_after_a_clearing_restart_moves_by_the_scheduled_rate():
    """MultiStepLR_Restart(clear_state) empties optimizer.state at epoch restart + 1 = 3 and halves the rate: FlatAdam starts its moments
    over, and a first Adam step moves every touched parameter by the rate -- the scheduled one (the bound smoke() uses)."""
    model = _sr_model(_sr_opt(lr=1e-3, lr_scheme='MultiStepLR_Restart', lr_steps=[100], restarts=[2], restart_weights=[0.5],
                              lr_gamma=0.5, clear_state=True))
    batches = _batches(3)
    _steps(model, batches[:2], 1)
    assert model.optimizer_G._steps == [2] and model.optimizer_G.param_groups[0]['lr'] == 1e-3
    before = _flat(model.optimizer_G)
    _steps(model, batches[2:], 3)
    lr = model.optimizer_G.param_groups[0]['lr']
    assert lr == 0.5e-3 and model.optimizer_G._steps == [1]
    step = (_flat(model.optimizer_G) - before).abs().max().item()
    print('max |update| %.4e at lr %.1e' % (step, lr))
    assert 0.5 * lr < step <= 1.001 * lr


# ---------------------------------------------------------------------------------------------------------------- resume
@pytest.fixture(scope='module')
def resumed(tmp_path_factory):
    """A: 4 scheduled steps.  B: 2 steps, checkpoint.  C: built from the checkpoint -- a snapshot before any step -- then 2 more."""
    from realvsr_amd import _lib
    old = _lib.get_gemm_mode()
    _lib.set_gemm_mode('f32')
    torch.cuda.set_device(0)
    try:
        root = tmp_path_factory.mktemp('resume')
        batches = _batches(4)
        a = _sr_model(_sr_opt(**THREE))
        initial = _flat(a.optimizer_G)
        _steps(a, batches, 1)
        b = _sr_model(_sr_opt(root, **THREE))
        assert torch.equal(_flat(b.optimizer_G), initial)
        _steps(b, batches[:2], 1)
        b.save(2)
        b.save_training_state(0, 2)
        opt_c = _sr_opt(root, **THREE)
        opt_c['path']['pretrain_model_G'] = os.path.join(opt_c['path']['models'], '2_G.pth')
        state = torch.load(os.path.join(opt_c['path']['training_state'], '2.state'), map_location='cpu', weights_only=False)
        c = _sr_model(opt_c)
        c.resume_training(state)
        snap = {'param': _flat(c.optimizer_G), 'exp_avg': c.optimizer_G.exp_avg.clone(), 'exp_avg_sq': c.optimizer_G.exp_avg_sq.clone(),
                'sd': {k: v.clone() for k, v in c.netG.state_dict().items()}, 'steps': list(c.optimizer_G._steps),
                'groups': [(g['lr'], g['initial_lr']) for g in c.optimizer_G.param_groups],
                'last_epoch': [s.last_epoch for s in c.schedulers]}
        c.optimizer_G.buffers.check_bound()
        _steps(c, batches[2:], 3)
        return {'a': a, 'b': b, 'c': c, 'snap': snap, 'state': state, 'initial': initial, 'root': root}
    finally:
        _lib.set_gemm_mode(old)


def test_resume_is_exact_before_the_next_step(resumed):
    b, snap, state = resumed['b'], resumed['snap'], resumed['state']
    assert sorted(state) == ['epoch', 'iter', 'optimizers', 'schedulers'] and state['epoch'] == 0 and state['iter'] == 2
    assert torch.equal(snap['param'], _flat(b.optimizer_G))
    sd_b = b.netG.state_dict()
    assert list(snap['sd']) == list(sd_b)
    for k, v in sd_b.items():
        assert torch.equal(snap['sd'][k], v), k
    assert torch.equal(snap['exp_avg'], b.optimizer_G.exp_avg) and torch.equal(snap['exp_avg_sq'], b.optimizer_G.exp_avg_sq)
    assert float(snap['exp_avg'].abs().max()) > 0
    assert snap['steps'] == b.optimizer_G._steps == [2]
    assert snap['groups'] == [(g['lr'], g['initial_lr']) for g in b.optimizer_G.param_groups]
    assert snap['groups'][0][1] == BASE and abs(snap['groups'][0][0] - G['three_lr'][2]) <= 1e-12 * BASE
    assert snap['last_epoch'] == [s.last_epoch for s in b.schedulers] == [2]


def test_resumed_run_continues_like_the_uninterrupted_one(resumed):
    a, c, initial = resumed['a'], resumed['c'], resumed['initial']
    assert c.optimizer_G._steps == a.optimizer_G._steps == [4]
    assert c.optimizer_G.param_groups[0]['lr'] == a.optimizer_G.param_groups[0]['lr']
    d_ref = (_flat(a.optimizer_G) - initial).double()
    d_got = (_flat(c.optimizer_G) - initial).double()
    rel = float((d_got - d_ref).norm() / d_ref.norm())
    print('update after 4 steps, resumed vs uninterrupted: rel l2 err %.3e; |update| max %.3e' % (rel, float(d_ref.abs().max())))
    assert float(d_ref.abs().max()) > 2 * BASE       # (four steps at ~lr each: the update being compared is not small)
    assert rel <= 2e-2
    c.optimizer_G.buffers.check_bound()


def test_state_interchanges_with_torch_adam(resumed):
    b, state = resumed['b'], resumed['state']
    ours = b.optimizer_G
    params = ours.param_groups[0]['params']
    # our 'optimizers' entry -> torch.optim.Adam over same-shaped parameters
    clones = [torch.zeros_like(p) for p in params]
    adam = torch.optim.Adam(clones, lr=1.0)
    adam.load_state_dict(copy.deepcopy(state['optimizers'][0]))
    assert adam.param_groups[0]['lr'] == ours.param_groups[0]['lr'] and adam.param_groups[0]['betas'] == (0.9, 0.99)
    for p, q in zip(params, clones):
        assert torch.equal(adam.state[q]['exp_avg'], ours.state[p]['exp_avg'])
        assert torch.equal(adam.state[q]['exp_avg_sq'], ours.state[p]['exp_avg_sq'])
        assert float(adam.state[q]['step']) == 2.0
    # a torch.optim.Adam state_dict -> resume_training
    gen = torch.Generator().manual_seed(9)
    adam = torch.optim.Adam([p.detach().clone() for p in params], lr=3e-4, betas=(0.9, 0.99))
    for _ in range(3):
        for q in adam.param_groups[0]['params']:
            q.grad = torch.randn(q.shape, generator=gen).to(q.device)
        adam.step()
    adam.param_groups[0]['initial_lr'] = 3e-4       # (what a scheduler on it would have recorded)
    model = _sr_model(_sr_opt(**THREE))
    model.resume_training({'optimizers': [adam.state_dict()], 'schedulers': [model.schedulers[0].state_dict()]})
    mine = model.optimizer_G
    assert mine._steps == [3] and mine.param_groups[0]['lr'] == 3e-4
    for p, q in zip(mine.param_groups[0]['params'], adam.param_groups[0]['params']):
        assert torch.equal(mine.state[p]['exp_avg'], adam.state[q]['exp_avg'])
        assert torch.equal(mine.state[p]['exp_avg_sq'], adam.state[q]['exp_avg_sq'])
        o = mine.buffers.offset[p]
        assert mine.state[p]['exp_avg'].data_ptr() == mine.exp_avg.data_ptr() + 4 * o     # the flat moments, not copies
    mine.buffers.check_bound()


# ---------------------------------------------------------------------------------------------------------------- the GAN model
def _gan_opt(root=None, **train):
    t = {'lr_G': BASE, 'weight_decay_G': 0, 'beta1_G': 0.9, 'beta2_G': 0.99, 'lr_D': BASE, 'weight_decay_D': 0, 'beta1_D': 0.9,
         'beta2_D': 0.99, 'pixel_criterion_s': 'cb', 'pixel_weight_s': 1.0, 'pixel_criterion_d': 'cb', 'pixel_weight_d': 1.0,
         'pixel_criterion_c': 'cb', 'pixel_weight_c': 1.0, 'feature_criterion': 'cb', 'feature_weight': 0.0, 'gan_type': 'ragan',
         'gan_weight': 0.1}
    t.update(train)
    path = {'pretrain_model_G': None, 'pretrain_model_D': None, 'strict_load': True}
    if root is not None:
        path.update(models=os.path.join(str(root), 'models'), training_state=os.path.join(str(root), 'training_state'))
        for k in ('models', 'training_state'):
            os.makedirs(path[k], exist_ok=True)
    return {'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
            'network_G': {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1, 'back_RBs': 1,
                          'predeblur': False, 'HR_in': False, 'w_TSA': False, 'center': None},
            'network_D': {'which_model_D': 'MultiscaleDiscriminator_v4', 'in_nc': 1, 'nf': 16, 'num_D': 2, 'gan_type': 'patch'},
            'path': path, 'train': t}


def _gan_model(opt):
    from realvsr_amd.VideoSR_model import VideoSRGANModel, create_model
    from weights import fill_state_dict
    model = create_model(opt)
    assert isinstance(model, VideoSRGANModel)
    if opt['path'].get('pretrain_model_G') is None:
        fill_state_dict(model.netG, 505, offset_std=0.02)
        sd = {k: v.clone() for k, v in model.netD.state_dict().items()}     # the buffers (BatchNorm statistics) as constructed
        fill_state_dict(model.netD, 606)
        model.netD.load_state_dict({k: v for k, v in sd.items() if 'running_' in k or 'num_batches' in k}, strict=False)
    return model


def test_gan_model_schedules_saves_and_resumes_both_networks(tmp_path):
    b = _gan_model(_gan_opt(tmp_path, **THREE))
    assert len(b.schedulers) == 2 and [s.optimizer for s in b.schedulers] == [b.optimizer_G, b.optimizer_D]
    g = load_golden('gan_step')
    batch = {'LQs': torch.from_numpy(g['LQs']), 'GT': torch.from_numpy(g['GT'])}
    _steps(b, [batch, batch], 1)
    for o in b.optimizers:
        assert abs(o.param_groups[0]['lr'] - G['three_lr'][2]) <= 1e-12 * BASE and o._steps == [2]
    b.save(2)
    b.save_training_state(0, 2)
    models = b.opt['path']['models']
    assert sorted(os.listdir(models)) == ['2_D.pth', '2_G.pth'] and os.listdir(b.opt['path']['training_state']) == ['2.state']
    opt_c = _gan_opt(tmp_path, **THREE)
    opt_c['path'].update(pretrain_model_G=os.path.join(models, '2_G.pth'), pretrain_model_D=os.path.join(models, '2_D.pth'))
    c = _gan_model(opt_c)
    state = torch.load(os.path.join(opt_c['path']['training_state'], '2.state'), map_location='cpu', weights_only=False)
    assert len(state['optimizers']) == 2 and len(state['schedulers']) == 2
    c.resume_training(state)
    for net_b, net_c in ((b.netG, c.netG), (b.netD, c.netD)):
        sd_b, sd_c = net_b.state_dict(), net_c.state_dict()
        assert list(sd_b) == list(sd_c)
        for k in sd_b:
            assert torch.equal(sd_b[k], sd_c[k]), k
    stats = [k for k in b.netD.state_dict() if 'running_mean' in k]
    assert stats and all(float(b.netD.state_dict()[k].abs().max()) > 0 for k in stats)       # moved by the two steps, and compared above
    for o_b, o_c in zip(b.optimizers, c.optimizers):
        assert torch.equal(o_b.exp_avg, o_c.exp_avg) and torch.equal(o_b.exp_avg_sq, o_c.exp_avg_sq) and float(o_b.exp_avg.abs().max()) > 0
        assert o_b._steps == o_c._steps == [2]
        assert [(g['lr'], g['initial_lr']) for g in o_b.param_groups] == [(g['lr'], g['initial_lr']) for g in o_c.param_groups]
        o_c.buffers.check_bound()
    assert [s.last_epoch for s in c.schedulers] == [2, 2]


def test_gan_model_scheme_names():
    from realvsr_amd import lr_scheduler as S
    m = _gan_model(_gan_opt(lr_scheme='MultiStepLR', lr_steps=[2, 4], restarts=None, restart_weights=None, lr_gamma=0.5, clear_state=False))
    assert len(m.schedulers) == 2 and all(isinstance(s, S.MultiStepLR_Restart) for s in m.schedulers)
    for k in (1, 2):
        m.update_learning_rate(k)
    assert [o.param_groups[0]['lr'] for o in m.optimizers] == [BASE * 0.5] * 2
    assert _gan_model(_gan_opt()).schedulers == []
    with pytest.raises(NotImplementedError):
        _gan_model(_gan_opt(lr_scheme='MultiStepLR_Restart'))
    with pytest.raises(NotImplementedError):
        _gan_model(_gan_opt(lr_scheme='StepLR'))


# ---------------------------------------------------------------------------------------------------------------- validation
def _write_clips(root, folders, T, lq_hw, scale, seed=21):
    from PIL import Image
    rng = np.random.RandomState(seed)
    for which, s in (('LQ', 1), ('GT', scale)):
        for folder in folders:
            os.makedirs(os.path.join(str(root), which, folder))
            base = rng.randint(0, 256, size=(lq_hw[0] * s, lq_hw[1] * s, 3))
            for i in range(T):
                frame = np.clip(base + rng.randint(-40, 41, size=base.shape), 0, 255).astype(np.uint8)
                Image.fromarray(frame, 'RGB').save(os.path.join(str(root), which, folder, '%05d.png' % i))


def _val_set(root):
    from realvsr_amd import data
    return data.VideoTestDataset({'name': 'RealVSR_Test', 'mode': 'VideoTest', 'dataroot_GT': os.path.join(str(root), 'GT'),
                                  'dataroot_LQ': os.path.join(str(root), 'LQ'), 'cache_data': True, 'N_frames': 3, 'padding': 'new_info',
                                  'color': 'ycbcr', 'phase': 'val', 'scale': 1, 'data_type': 'img'})


@pytest.mark.parametrize('which', ['EDVR', 'RCAN'])
def test_validate_equals_the_frame_wise_loop(which, tmp_path):
    from PIL import Image
    from torch.utils.data import default_collate
    from realvsr_amd import infer, train
    scale = 4 if which == 'EDVR' else 1
    _write_clips(tmp_path, ('003', '017'), 5, (16, 24), scale)
    opt = _sr_opt(tmp_path)
    if which == 'RCAN':       # a generator without extract_features: one network call per window
        opt['scale'] = 1
        opt['network_G'] = dict(which_model_G='RCAN', num_in_ch=3, num_out_ch=3, num_frames=3, num_feat=64, num_group=1, num_block=1,
                                squeeze_factor=16, res_scale=1)
    model = _sr_model(opt)
    assert hasattr(model.netG, 'extract_features') == (which == 'EDVR')
    val_set = _val_set(tmp_path)
    assert len(val_set) == 10
    want, first = {}, {}
    for i in range(len(val_set)):
        sample = val_set[i]
        model.feed_data(default_collate([sample]))
        model.test()
        want.setdefault(sample['folder'], []).append(model.get_current_metrics()['psnr'][0])
        if sample['idx'].startswith('0/'):
            first[sample['folder']] = infer.ycbcr_to_bgr_u8(model.fake_H[0]).cpu().numpy()
    assert model.netG.training
    res = train.validate(model, val_set, 30)
    assert model.netG.training
    assert list(res['psnr']) == ['003', '017']
    for folder in want:
        print(folder, res['psnr'][folder])
        assert res['psnr'][folder] == want[folder]                     # == : the same kernels on the same numbers
        assert all(np.isfinite(v) and 3 < v < 60 for v in want[folder])
        assert res['psnr_avg'][folder] == sum(want[folder]) / len(want[folder])
    assert res['psnr_total'] == sum(res['psnr_avg'].values()) / 2
    images = sorted(os.path.relpath(p, opt['path']['val_images']) for p in glob.glob(os.path.join(opt['path']['val_images'], '*', '*')))
    # every fifth frame, counted over all folders: frame 0 of each 5-frame folder
    assert images == [os.path.join('003_000', '0000030.png'), os.path.join('017_000', '0000030.png')]
    for folder in want:
        with Image.open(os.path.join(opt['path']['val_images'], folder + '_000', '0000030.png')) as im:
            rgb = np.asarray(im.convert('RGB'))
        assert rgb.shape == (16 * scale, 24 * scale, 3) and np.array_equal(rgb[:, :, ::-1], first[folder])


# ---------------------------------------------------------------------------------------------------------------- end to end
def _write_option_file(root, resume_state=None):
    """The shipped EDVR option file with the sizes shrunk: a synthetic RealVSR tree (2 sequences x 10 frames of 40 x 24, keys for the
    frames whose window needs no redraw), the 'three_lr' schedule, 6 iterations."""
    from PIL import Image
    with open(os.path.join(GOLDEN, 'options', 'train_EDVR_woTSA_RealVSR_YCbCr_Split.yml')) as f:
        opt = yaml.safe_load(f)
    data_root = os.path.join(str(root), 'data')
    if not os.path.isdir(data_root):
        rng = np.random.RandomState(4)
        for which in ('GT', 'LQ'):
            for seq in ('000', '001'):
                os.makedirs(os.path.join(data_root, which, seq))
                for i in range(10):
                    Image.fromarray(rng.randint(0, 256, size=(40, 24, 3)).astype(np.uint8), 'RGB').save(
                        os.path.join(data_root, which, seq, '%05d.png' % i))
        with open(os.path.join(data_root, 'keys.pkl'), 'wb') as f:
            pickle.dump({'keys': ['%s_%05d' % (s, i) for s in ('000', '001') for i in range(1, 9)]}, f)
        _write_clips(os.path.join(data_root, 'val'), ('003', '017'), 5, (16, 24), 1)
    opt['name'] = 'e2e'
    opt['use_tb_logger'] = False
    opt['gpu_ids'] = [0]
    opt['datasets']['train'].update(dataroot_GT=os.path.join(data_root, 'GT'), dataroot_LQ=os.path.join(data_root, 'LQ'),
                                    cache_keys=os.path.join(data_root, 'keys.pkl'), remove_list=None, n_workers=0, batch_size=2,
                                    GT_size=16, LQ_size=16, frame_chw=[3, 40, 24])
    opt['datasets']['val'].update(dataroot_GT=os.path.join(data_root, 'val', 'GT'), dataroot_LQ=os.path.join(data_root, 'val', 'LQ'))
    opt['network_G'].update(front_RBs=1, back_RBs=1)      # (EDVR_NoUp is built for nf 64 only, like the reference's)
    opt['train'].update(lr_G=BASE, niter=6, val_freq=3, pixel_criterion_y='cb', pixel_criterion_c='cb',
                        T_period=THREE['T_period'], restarts=THREE['restarts'], restart_weights=THREE['restart_weights'])
    opt['logger'].update(print_freq=1, save_checkpoint_freq=3)
    opt['augment'] = None
    opt['path']['resume_state'] = resume_state
    path = os.path.join(str(root), 'e2e.yml')
    with open(path, 'w') as f:
        yaml.safe_dump(opt, f)
    return path


def _newest_log(exp):
    logs = sorted(glob.glob(os.path.join(exp, 'train_e2e_*.log')), key=os.path.getmtime)
    with open(logs[-1]) as f:
        return f.read()


ITER_LINE = re.compile(r'<epoch:\s*(\d+), iter:\s*([\d,]+), lr:\(([^)]*)\)>')


def test_main_trains_validates_checkpoints_and_resumes(tmp_path):
    from realvsr_amd import train
    exp = os.path.join(str(tmp_path), 'experiments', 'e2e')
    assert train.main(['-opt', _write_option_file(tmp_path), '--root', str(tmp_path)]) == 6
    assert sorted(os.listdir(os.path.join(exp, 'models'))) == ['3_G.pth', '6_G.pth', 'latest_G.pth']
    assert sorted(os.listdir(os.path.join(exp, 'training_state'))) == ['3.state', '6.state']
    log = _newest_log(exp)
    lines = ITER_LINE.findall(log)
    assert [int(v[1]) for v in lines] == [1, 2, 3, 4, 5, 6]
    for _, it, rates in lines:
        assert rates == '{:.3e},'.format(G['three_lr'][int(it)])
    assert 'l_pix_y:' in log and 'l_pix_c:' in log
    marks = [m.start() for m in re.finditer(r'# Validation # PSNR: \d+\.\d\d dB,  003: \d+\.\d\d dB,  017: \d+\.\d\d dB', log)]
    assert len(marks) == 2
    # validation at 3 and 6: after that iteration's log line, before the next one
    pos = {int(m.group(2)): m.start() for m in ITER_LINE.finditer(log)}
    assert pos[3] < marks[0] < pos[4] and pos[6] < marks[1]
    assert sorted(os.listdir(os.path.join(exp, 'val_images', '003_000'))) == ['0000003.png', '0000006.png']
    latest = torch.load(os.path.join(exp, 'models', 'latest_G.pth'), map_location='cpu')
    six = torch.load(os.path.join(exp, 'models', '6_G.pth'), map_location='cpu')
    assert all(torch.equal(latest[k], six[k]) for k in six)

    os.remove(os.path.join(exp, 'models', '6_G.pth'))
    os.remove(os.path.join(exp, 'training_state', '6.state'))
    resume = os.path.join(exp, 'training_state', '3.state')
    assert train.main(['-opt', _write_option_file(tmp_path, resume_state=resume), '--root', str(tmp_path)]) == 6
    log = _newest_log(exp)
    assert 'Resuming training from epoch: 0, iter: 3.' in log and '3_G.pth' in log
    lines = ITER_LINE.findall(log)
    assert [int(v[1]) for v in lines] == [4, 5, 6]
    assert lines[0][2] == '{:.3e},'.format(G['three_lr'][4])
    assert len(re.findall(r'# Validation # PSNR', log)) == 1
    assert sorted(os.listdir(os.path.join(exp, 'models'))) == ['3_G.pth', '6_G.pth', 'latest_G.pth']
    assert sorted(os.listdir(os.path.join(exp, 'training_state'))) == ['3.state', '6.state']
    state = torch.load(os.path.join(exp, 'training_state', '6.state'), map_location='cpu', weights_only=False)
    assert state['iter'] == 6 and state['schedulers'][0]['last_epoch'] == 6
    assert float(state['optimizers'][0]['state'][0]['step']) == 6.0       # 3 resumed + 3 taken
