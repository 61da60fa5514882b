"""Option files: the YAML the reference trains from, parsed into the ``opt`` dictionary the models and data sets read.

Same results as codes/options/options.py (parse :9-68, dict2str :71-81, dict_to_nonedict :84-94, check_resume :97-111, NoneDict :114-116):
every data set gets its ``phase`` (the key up to the first '_'), the file's ``scale`` and a ``data_type`` ('lmdb' if a data root ends in
'lmdb', else 'img'; 'mc' for a mode ending in '_mc'), '~' is expanded in the data roots and in ``path``, a training run gets
``experiments_root``, ``models``, ``training_state``, ``log`` and ``val_images`` under ``<root>/experiments/<name>`` (a test run
``results_root`` and ``log`` under ``<root>/results/<name>``), a name containing 'debug' shortens ``val_freq``, ``print_freq`` and
``save_checkpoint_freq`` to 8, 1 and 8, and ``network_G`` gets the scale.

Deliberate differences:
  * ``root`` is an argument and defaults to the current directory; the reference derives it from where its own checkout lies.
  * CUDA_VISIBLE_DEVICES is NOT exported from ``gpu_ids``: a run is one process per GPU, and which device a process uses is the
    launcher's decision (python -m torch.distributed.run sets LOCAL_RANK), not the option file's.
  * check_resume recognises a GAN model by 'gan' in the LOWER-CASED model name.  The reference tests the name as written, and
    'VideoSRGAN_AllPair_YCbCr_Split' contains no lower-case 'gan': its resumed GAN run keeps the discriminator the option file names
    (or a fresh one) next to optimizer moments that belong to the checkpointed one.
"""
import logging
import os
import os.path as osp

import yaml


class NoneDict(dict):
    """A dict whose missing keys read as None."""

    def __missing__(self, key):
        return None


def parse(opt_path, is_train=True, root=None):
    with open(opt_path, mode='r') as f:
        opt = yaml.safe_load(f)   # (plain dicts keep the file's order)
    opt['is_train'] = is_train
    sr = opt['distortion'] == 'sr'

    for phase, dataset in opt['datasets'].items():
        dataset['phase'] = phase.split('_')[0]
        if sr:
            dataset['scale'] = opt['scale']
        is_lmdb = False
        for key in ('dataroot_GT', 'dataroot_LQ'):
            if dataset.get(key) is not None:
                dataset[key] = osp.expanduser(dataset[key])
                is_lmdb = is_lmdb or dataset[key].endswith('lmdb')
        dataset['data_type'] = 'lmdb' if is_lmdb else 'img'
        if dataset['mode'].endswith('mc'):   # memcached
            dataset['data_type'] = 'mc'
            dataset['mode'] = dataset['mode'].replace('_mc', '')

    for key, path in opt['path'].items():
        if path and key != 'strict_load':
            opt['path'][key] = osp.expanduser(path)
    opt['path']['root'] = osp.abspath(os.getcwd() if root is None else str(root))
    if is_train:
        experiments_root = osp.join(opt['path']['root'], 'experiments', opt['name'])
        opt['path']['experiments_root'] = experiments_root
        opt['path']['models'] = osp.join(experiments_root, 'models')
        opt['path']['training_state'] = osp.join(experiments_root, 'training_state')
        opt['path']['log'] = experiments_root
        opt['path']['val_images'] = osp.join(experiments_root, 'val_images')
        if 'debug' in opt['name']:
            opt['train']['val_freq'] = 8
            opt['logger']['print_freq'] = 1
            opt['logger']['save_checkpoint_freq'] = 8
    else:
        results_root = osp.join(opt['path']['root'], 'results', opt['name'])
        opt['path']['results_root'] = results_root
        opt['path']['log'] = results_root

    if sr:
        opt['network_G']['scale'] = opt['scale']
    return opt


def dict2str(opt, indent_l=1):
    """The option tree as indented text, for the log."""
    pad = ' ' * (indent_l * 2)
    msg = ''
    for k, v in opt.items():
        if isinstance(v, dict):
            msg += pad + k + ':[\n' + dict2str(v, indent_l + 1) + pad + ']\n'
        else:
            msg += pad + k + ': ' + str(v) + '\n'
    return msg


def dict_to_nonedict(opt):
    """The same tree with every dict a NoneDict (lists are walked, everything else is kept)."""
    if isinstance(opt, dict):
        return NoneDict((key, dict_to_nonedict(sub_opt)) for key, sub_opt in opt.items())
    if isinstance(opt, list):
        return [dict_to_nonedict(sub_opt) for sub_opt in opt]
    return opt


def check_resume(opt, resume_iter):
    """With path.resume_state set: point pretrain_model_G (and _D for a GAN model) at the checkpoint of `resume_iter` under path.models."""
    logger = logging.getLogger('base')
    if not opt['path'].get('resume_state'):
        return
    if opt['path'].get('pretrain_model_G') is not None or opt['path'].get('pretrain_model_D') is not None:
        logger.warning('pretrain_model path will be ignored when resuming training.')
    opt['path']['pretrain_model_G'] = osp.join(opt['path']['models'], '{}_G.pth'.format(resume_iter))
    logger.info('Set [pretrain_model_G] to ' + opt['path']['pretrain_model_G'])
    if 'gan' in opt['model'].lower():
        opt['path']['pretrain_model_D'] = osp.join(opt['path']['models'], '{}_D.pth'.format(resume_iter))
        logger.info('Set [pretrain_model_D] to ' + opt['path']['pretrain_model_D'])
