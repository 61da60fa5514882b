"""realvsr_amd.options on two of the reference's shipped option files (tests/golden/options/, settings only)."""
import os

import pytest

from conftest import GOLDEN
from realvsr_amd import options

SR_FILE = os.path.join(GOLDEN, 'options', 'train_EDVR_woTSA_RealVSR_YCbCr_Split.yml')
GAN_FILE = os.path.join(GOLDEN, 'options', 'train_EDVR-GAN_woTSA_RealVSR_YCbCr_Split.yml')
SR_NAME = '001_EDVR_NoUp_woTSA_scratch_lr1e-4_150k_RealVSR_3frame_WiCutBlur_YCbCr_LapPyr+GW'


@pytest.mark.parametrize('path', [SR_FILE, GAN_FILE], ids=['sr', 'gan'])
def test_parse_training_file(path, tmp_path, monkeypatch):
    monkeypatch.setenv('CUDA_VISIBLE_DEVICES', 'untouched')
    opt = options.parse(path, is_train=True, root=tmp_path)
    assert os.environ['CUDA_VISIBLE_DEVICES'] == 'untouched'
    assert opt['is_train'] is True and opt['gpu_ids'] == [0, 1, 2, 3] and opt['scale'] == 1
    assert list(opt['datasets']) == ['train', 'val']
    for phase, mode in (('train', 'RealVSR_AllPair'), ('val', 'VideoTest')):
        d = opt['datasets'][phase]
        assert d['phase'] == phase and d['scale'] == 1 and d['data_type'] == 'img' and d['mode'] == mode and d['color'] == 'ycbcr'
    assert opt['datasets']['val']['cache_data'] is True and opt['datasets']['val']['padding'] == 'new_info'
    root = os.path.join(str(tmp_path), 'experiments', opt['name'])
    p = opt['path']
    assert p['root'] == str(tmp_path) and p['experiments_root'] == root and p['log'] == root
    assert p['models'] == os.path.join(root, 'models') and p['training_state'] == os.path.join(root, 'training_state')
    assert p['val_images'] == os.path.join(root, 'val_images')
    assert p['strict_load'] is True and p['resume_state'] is None
    assert opt['network_G']['scale'] == 1 and opt['network_G']['which_model_G'] == 'EDVR_NoUp'
    t = opt['train']
    assert t['lr_scheme'] == 'CosineAnnealingLR_Restart' and t['T_period'] == [150000] * 4 and t['restarts'] == [150000, 300000, 450000]
    assert t['eta_min'] == 1e-7 and isinstance(t['eta_min'], float) and t['val_freq'] == 1e4 and t['niter'] == 150000
    assert opt['logger'] == {'print_freq': 100, 'save_checkpoint_freq': 1e4}


def test_the_two_files_differ_where_expected(tmp_path):
    sr, gan = options.parse(SR_FILE, root=tmp_path), options.parse(GAN_FILE, root=tmp_path)
    assert sr['name'] == SR_NAME and sr['model'] == 'VideoSR_AllPair_YCbCr_Split' and sr['train']['lr_G'] == 1e-4
    assert sr['path']['pretrain_model_G'] is None and 'network_D' not in sr
    assert gan['model'] == 'VideoSRGAN_AllPair_YCbCr_Split' and gan['train']['lr_D'] == 5e-5 and gan['train']['gan_type'] == 'ragan'
    assert gan['network_D']['which_model_D'] == 'MultiscaleDiscriminator_v4'
    assert gan['path']['pretrain_model_G'].endswith('LapPyr+GW.pth')


def test_root_defaults_to_the_current_directory(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    opt = options.parse(SR_FILE)
    assert opt['path']['root'] == os.path.abspath(str(tmp_path))
    test_opt = options.parse(SR_FILE, is_train=False)
    assert test_opt['path']['results_root'] == os.path.join(os.path.abspath(str(tmp_path)), 'results', SR_NAME)
    assert test_opt['path']['log'] == test_opt['path']['results_root'] and 'models' not in test_opt['path']


def test_home_is_expanded(tmp_path, monkeypatch):
    monkeypatch.setenv('HOME', '/somewhere')
    text = open(SR_FILE).read().replace('/home/yangxi/datasets/RealVSR/GT_YCbCr_test_10', '~/val_GT').replace(
        'pretrain_model_G: ~', 'pretrain_model_G: ~/net.pth')
    (tmp_path / 'home.yml').write_text(text)
    opt = options.parse(str(tmp_path / 'home.yml'), root=tmp_path)
    assert opt['datasets']['val']['dataroot_GT'] == '/somewhere/val_GT' and opt['path']['pretrain_model_G'] == '/somewhere/net.pth'


def test_debug_overrides(tmp_path):
    text = open(SR_FILE).read().replace('name: 001_EDVR', 'name: debug_001_EDVR')
    (tmp_path / 'debug.yml').write_text(text)
    opt = options.parse(str(tmp_path / 'debug.yml'), root=tmp_path)
    assert opt['name'].startswith('debug_')
    assert opt['train']['val_freq'] == 8 and opt['logger'] == {'print_freq': 1, 'save_checkpoint_freq': 8}
    assert opt['path']['experiments_root'].endswith(os.path.join('experiments', opt['name']))


def test_lmdb_and_mc_data_types(tmp_path):
    text = open(SR_FILE).read().replace('RealVSR/GT_YCbCr\n', 'RealVSR/GT_YCbCr.lmdb\n').replace('mode: VideoTest', 'mode: VideoTest_mc')
    (tmp_path / 'types.yml').write_text(text)
    opt = options.parse(str(tmp_path / 'types.yml'), root=tmp_path)
    assert opt['datasets']['train']['data_type'] == 'lmdb'
    assert opt['datasets']['val']['data_type'] == 'mc' and opt['datasets']['val']['mode'] == 'VideoTest'


def test_nonedict():
    opt = options.dict_to_nonedict({'a': {'b': 1, 'l': [{'c': 2}, 3]}, 'n': None})
    assert isinstance(opt, options.NoneDict) and isinstance(opt['a'], options.NoneDict) and isinstance(opt['a']['l'][0], options.NoneDict)
    assert opt['missing'] is None and opt['a']['missing'] is None and opt['a']['l'][0]['missing'] is None
    assert opt['a']['b'] == 1 and opt['a']['l'][1] == 3 and opt.get('missing', 5) == 5
    parsed = options.dict_to_nonedict(options.parse(SR_FILE, root='/r'))
    assert parsed['train']['warmup_iter'] == -1 and parsed['train']['lr_steps'] is None and parsed['dist'] is None


def test_dict2str():
    s = options.dict2str({'a': 1, 'b': {'c': 'x', 'd': {'e': None}}})
    assert s == '  a: 1\n  b:[\n    c: x\n    d:[\n      e: None\n    ]\n  ]\n'


def test_check_resume(tmp_path):
    for path, model_d in ((SR_FILE, False), (GAN_FILE, True)):
        opt = options.parse(path, root=tmp_path)
        before = dict(opt['path'])
        options.check_resume(opt, 7000)
        assert opt['path'] == before                            # no resume_state: nothing happens
        opt['path']['resume_state'] = os.path.join(opt['path']['training_state'], '7000.state')
        options.check_resume(opt, 7000)
        assert opt['path']['pretrain_model_G'] == os.path.join(opt['path']['models'], '7000_G.pth')
        if model_d:
            assert opt['path']['pretrain_model_D'] == os.path.join(opt['path']['models'], '7000_D.pth')
        else:
            assert 'pretrain_model_D' not in opt['path']
