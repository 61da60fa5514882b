"""Train from a reference option file:

    python -m realvsr_amd.train -opt FILE [--launcher none|pytorch] [--dist-backend nccl|gloo] [--root DIR] [--model NAME]

The loop of codes/train.py in the same order -- schedule, data, step, log line, validation, checkpoint -- around the models of
realvsr_amd.VideoSR_model, whose step is the HIP hot path.  What differs from the reference is where the work happens, not what is done:

  * between two log lines the step is free of host synchronisation (optimize_parameters(step, log=False) keeps the loss terms on the
    device); the learning rate is host arithmetic that reaches the optimizer kernel as an argument;
  * validation runs clip by clip on the device (validate below): a clip is uploaded once as uint8, every frame's features are computed
    once (infer.SlidingWindowRunner) and only the per-frame PSNR scalars and every fifth frame's 3 bytes per pixel come back;
  * a RealVSR train data set with `resident: true` is decoded once into device memory and its batches are gathered there
    (realvsr_amd.resident: the same samples in the same order as the file loader with n_workers 0; resident_max_gb is the budget);
  * experiments go under --root (default: the current directory), CUDA_VISIBLE_DEVICES is left alone (realvsr_amd.options);
  * --model replaces the option file's `model` before create_model: the six Vimeo-90K files name 'VideoSR_AllPair', which no
    create_model knows (e.g. --model VideoSR_AllPair_YCbCr_Combine).

Distributed runs are started from outside, one process per GPU: python -m torch.distributed.run --nproc_per_node=K -m realvsr_amd.train
-opt FILE --launcher pytorch, for the PSNR models and the GAN model alike (the models broadcast rank 0's networks and all-reduce the
gradients; every rank resumes both optimizers from the .state file; rank 0 alone logs, validates and saves).  --dist-backend gloo lets a
one-GPU box rehearse that driver with all ranks on the same device (RCCL does not accept two ranks on one device); RVSR_DIST_CHECK=1 makes
every rank log a checksum of its flat parameter buffers at the end of the run.  This module never starts or replaces a process itself.
"""
import argparse
import logging
import math
import os
import random
import time
from collections import OrderedDict

import numpy as np
import torch

from . import options as option

DATASET_RATIO = 200   # distributed runs: one sampler "epoch" is the data set this many times over (codes/train.py:103)


# ---------------------------------------------------------------------------------------------------------------- helpers
def set_random_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def _timestamp():
    return time.strftime('%y%m%d-%H%M%S')


def mkdir_and_rename(path):
    """A fresh directory; one that exists is kept under a time-stamped name."""
    if os.path.exists(path):
        new_name = path + '_archived_' + _timestamp()
        logging.getLogger('base').info('Path already exists. Rename it to [{:s}]'.format(new_name))
        os.rename(path, new_name)
    os.makedirs(path)


def setup_logger(logger_name, root, phase, level=logging.INFO, screen=False, tofile=False):
    """The logger `logger_name` with the reference's line format, writing to <root>/<phase>_<time>.log and / or the screen.  Handlers
    of an earlier call are closed and replaced (two runs in one process do not write into each other's files)."""
    lg = logging.getLogger(logger_name)
    for h in list(lg.handlers):
        lg.removeHandler(h)
        h.close()
    formatter = logging.Formatter('%(asctime)s.%(msecs)03d - %(levelname)s: %(message)s', datefmt='%y-%m-%d %H:%M:%S')
    lg.setLevel(level)
    if tofile:
        fh = logging.FileHandler(os.path.join(root, phase + '_{}.log'.format(_timestamp())), mode='w')
        fh.setFormatter(formatter)
        lg.addHandler(fh)
    if screen:
        sh = logging.StreamHandler()
        sh.setFormatter(formatter)
        lg.addHandler(sh)
    return lg


def init_dist(backend='nccl', **kwargs):
    """One process per GPU, started by the launcher: RANK picks the device, then the process group (RCCL behind 'nccl')."""
    if torch.multiprocessing.get_start_method(allow_none=True) != 'spawn':
        torch.multiprocessing.set_start_method('spawn')
    rank = int(os.environ['RANK'])
    torch.cuda.set_device(rank % torch.cuda.device_count())
    torch.distributed.init_process_group(backend=backend, **kwargs)


def _tb_writer(opt):
    """A tensorboard SummaryWriter if the option file asks for one and the module is there, else None."""
    if not opt['use_tb_logger'] or 'debug' in opt['name']:
        return None
    try:
        from torch.utils.tensorboard import SummaryWriter
    except ImportError:
        logging.getLogger('base').info('tensorboard is not installed: no tensorboard log')
        return None
    return SummaryWriter(log_dir=os.path.join(opt['path']['root'], 'tb_logger', opt['name']))


# ---------------------------------------------------------------------------------------------------------------- validation
def validate(model, val_set, step, logger=None, tb_logger=None, save_images=True):
    """The video branch of the reference's validation (codes/train.py:272-320) on a VideoTestDataset, computed clip-wise on the device.

    For every folder: the cached uint8 clip is uploaded once, converted with clip_from_u8, super-resolved by a SlidingWindowRunner
    (N_frames and padding of the data set; per-frame features once for EDVR, one network call per window for the other generators) and
    scored by infer.evaluate_clip on channel 0 -- per frame exactly the PSNR that feed_data(sample) / test() / get_current_metrics()
    gives.  Every fifth frame (counted over all folders, as the reference counts) is written as
    <val_images>/<folder>_<idx:03d>/<step:07d>.png through ycbcr_to_bgr_u8 (save_images=False skips that; the PNG is deflated at level 1:
    the encoder runs on the host while the device waits).  netG is in eval() during the pass and in train() afterwards.
    A folder's mean is sum(v) / len(v), the total the mean of the folders' means.

    With opt['dist'] the caller (train below) has rank 0 validate while the other ranks wait at a barrier (run with two gloo ranks sharing
    one GPU, tests/test_gpu_gan_dist.py; never on several GPUs: a pass longer than the process group's timeout would end the run there).

    Returns {'psnr': {folder: [per frame]}, 'psnr_avg': {folder: mean}, 'psnr_total': mean of means}."""
    from PIL import Image
    from . import infer
    from .data import clip_from_u8
    net = model.netG
    runner = infer.SlidingWindowRunner(net, val_set.opt['N_frames'], val_set.opt['padding'])
    img_root = model.opt['path']['val_images']
    psnr_rlt, seen = OrderedDict(), 0
    net.eval()
    try:
        for folder in val_set.folders():
            lq_u8, gt_u8 = val_set.clip(folder)
            lq = clip_from_u8(lq_u8.to(model.device, non_blocking=True))
            gt = clip_from_u8(gt_u8.to(model.device, non_blocking=True))
            res = infer.evaluate_clip(runner, lq, gt, ssim=False, keep_output=True)
            psnr_rlt[folder] = list(res['psnr'])
            for i in range(-seen % 5, lq.shape[0], 5) if save_images else ():
                img_dir = os.path.join(img_root, '{}_{:03d}'.format(folder, i))
                os.makedirs(img_dir, exist_ok=True)
                bgr = infer.ycbcr_to_bgr_u8(res['output'][i]).cpu().numpy()
                Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(os.path.join(img_dir, '{:07d}.png'.format(step)),
                                                                         compress_level=1)
            seen += lq.shape[0]
            del res, lq, gt
    finally:
        net.train()
    psnr_avg = OrderedDict((k, sum(v) / len(v)) for k, v in psnr_rlt.items())
    psnr_total = sum(psnr_avg.values()) / len(psnr_avg)
    if logger is not None:
        log_s = '# Validation # PSNR: {:.2f} dB, '.format(psnr_total)
        for k, v in psnr_avg.items():
            log_s += ' {}: {:.2f} dB, '.format(k, v)
        logger.info(log_s)
    if tb_logger is not None:
        tb_logger.add_scalar('psnr_avg', psnr_total, step)
        for k, v in psnr_avg.items():
            tb_logger.add_scalar(k, v, step)
    return {'psnr': psnr_rlt, 'psnr_avg': psnr_avg, 'psnr_total': psnr_total}


# ---------------------------------------------------------------------------------------------------------------- the loop
def train(opt, model, train_loader, val_set=None, train_sampler=None, resume_state=None, total_epochs=None, rank=-1, logger=None,
          tb_logger=None):
    """The loop of codes/train.py:134-332.  Per batch, in this order:
        current_step += 1 (stop past train.niter); update_learning_rate(step, warmup_iter); feed_data; optimize_parameters(step, log = a
        print iteration); the log line (epoch, iter, learning rates, terms) every logger.print_freq; validate every train.val_freq if
        there is a val set; save + save_training_state every logger.save_checkpoint_freq on rank <= 0
    and save('latest') at the end.  `resume_state` (a loaded .state dictionary) goes through model.resume_training and makes the loop
    start at its iter + 1, in its epoch.  Returns the last step taken."""
    logger = logger or logging.getLogger('base')
    total_iters = int(opt['train']['niter'])
    if total_epochs is None:
        total_epochs = int(math.ceil(total_iters / max(1, len(train_loader))))
    warmup_iter = opt['train'].get('warmup_iter')
    warmup_iter = -1 if warmup_iter is None else warmup_iter
    print_freq, save_freq = opt['logger']['print_freq'], opt['logger']['save_checkpoint_freq']
    val_freq = opt['train'].get('val_freq')

    if resume_state:
        logger.info('Resuming training from epoch: {}, iter: {}.'.format(resume_state['epoch'], resume_state['iter']))
        start_epoch, current_step = resume_state['epoch'], resume_state['iter']
        model.resume_training(resume_state)
    else:
        start_epoch, current_step = 0, 0

    logger.info('Start training from epoch: {:d}, iter: {:d}'.format(start_epoch, current_step))
    done = current_step >= total_iters
    for epoch in range(start_epoch, total_epochs + 1):
        if done:
            break
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        for train_data in train_loader:
            current_step += 1
            if current_step > total_iters:
                current_step -= 1
                done = True
                break
            model.update_learning_rate(current_step, warmup_iter=warmup_iter)
            model.feed_data(train_data)
            printing = current_step % print_freq == 0
            model.optimize_parameters(current_step, log=printing)

            if printing:
                message = '<epoch:{:3d}, iter:{:8,d}, lr:('.format(epoch, current_step)
                for v in model.get_current_learning_rate():
                    message += '{:.3e},'.format(v)
                message += ')>, '
                for k, v in model.get_current_log().items():
                    message += '{:s}: {:.4e} '.format(k, v)
                    if tb_logger is not None and rank <= 0:
                        tb_logger.add_scalar(k, v, current_step)
                if rank <= 0:
                    logger.info(message)

            if val_set is not None and val_freq and current_step % val_freq == 0:
                if rank <= 0:
                    validate(model, val_set, current_step, logger=logger, tb_logger=tb_logger)
                if opt.get('dist'):
                    torch.distributed.barrier()  # the other ranks wait for rank 0's pass

            if current_step % save_freq == 0 and rank <= 0:
                logger.info('Saving models and training states.')
                model.save(current_step)
                model.save_training_state(epoch, current_step)

    if opt.get('dist') and os.environ.get('RVSR_DIST_CHECK', '0') == '1':
        # developer check: every rank's line must carry the same numbers (the sum of the parameters' bit patterns, per optimizer)
        sums = [int(o.buffers.param.view(torch.int32).sum(dtype=torch.int64)) for o in model.optimizers]
        logger.info('rank {:d}: iter {:d}, parameter checksums {}'.format(rank, current_step, ' '.join(str(v) for v in sums)))
    if rank <= 0:
        logger.info('Saving the final model.')
        model.save('latest')
        logger.info('End of training.')
    return current_step


def main(argv=None):
    parser = argparse.ArgumentParser(prog='python -m realvsr_amd.train', description=__doc__.split('\n\n')[0])
    parser.add_argument('-opt', type=str, required=True, help='path to the option YAML file')
    parser.add_argument('--launcher', choices=['none', 'pytorch'], default='none', help='pytorch: started by torch.distributed.run')
    parser.add_argument('--dist-backend', choices=['nccl', 'gloo'], default='nccl',
                        help='pytorch launcher: nccl = RCCL, one GPU per rank; gloo = rehearsal with all ranks on one GPU')
    parser.add_argument('--local_rank', type=int, default=0)
    parser.add_argument('--root', type=str, default=None, help='where experiments/<name> goes (default: the current directory)')
    parser.add_argument('--model', type=str, default=None, help="replaces the option file's `model`")
    args = parser.parse_args(argv)
    opt = option.parse(args.opt, is_train=True, root=args.root)
    if args.model:
        opt['model'] = args.model

    from .VideoSR_model import create_model
    from .data import DistIterSampler, create_dataloader, create_dataset

    world_size = 1
    if args.launcher == 'none':
        opt['dist'] = False
        rank = -1
    else:
        opt['dist'] = True
        init_dist(backend=args.dist_backend)
        world_size = torch.distributed.get_world_size()
        rank = torch.distributed.get_rank()

    resume_state = None
    if opt['path'].get('resume_state'):
        # (a .state file pickles the schedulers' Counter of milestones: not a weights-only file)
        resume_state = torch.load(opt['path']['resume_state'], map_location='cpu', weights_only=False)
        option.check_resume(opt, resume_state['iter'])

    if rank <= 0:
        if resume_state is None:
            mkdir_and_rename(opt['path']['experiments_root'])
            for key, path in opt['path'].items():
                if path and key not in ('experiments_root', 'strict_load', 'root') and 'pretrain_model' not in key and 'resume' not in key:
                    os.makedirs(path, exist_ok=True)
        logger = setup_logger('base', opt['path']['log'], 'train_' + opt['name'], level=logging.INFO, screen=True, tofile=True)
        logger.info(option.dict2str(opt))
        tb_logger = _tb_writer(opt)
    else:
        logger = setup_logger('base', opt['path']['log'], 'train', level=logging.INFO, screen=True)
        tb_logger = None

    opt = option.dict_to_nonedict(opt)

    seed = opt['train']['manual_seed']
    if seed is None:
        seed = random.randint(1, 10000)
    if rank <= 0:
        logger.info('Random seed: {}'.format(seed))
    set_random_seed(seed)

    train_loader = train_sampler = val_set = total_epochs = None
    total_iters = int(opt['train']['niter'])
    for phase, dataset_opt in opt['datasets'].items():
        if phase == 'train':
            train_set = create_dataset(dataset_opt)
            train_size = int(math.ceil(len(train_set) / dataset_opt['batch_size']))
            total_epochs = int(math.ceil(total_iters / train_size))
            if opt['dist']:
                train_sampler = DistIterSampler(train_set, world_size, rank, DATASET_RATIO)
                total_epochs = int(math.ceil(total_iters / (train_size * DATASET_RATIO)))
            if dataset_opt.get('resident'):   # (a key of ours: every frame decoded once into HBM, batches gathered on the device)
                from .resident import create_resident_loader
                train_loader = create_resident_loader(train_set, dataset_opt, opt, train_sampler)
            else:
                train_loader = create_dataloader(train_set, dataset_opt, opt, train_sampler)
            if rank <= 0:
                logger.info('Number of train images: {:,d}, iters: {:,d}'.format(len(train_set), train_size))
                logger.info('Total epochs needed: {:d} for iters {:,d}'.format(total_epochs, total_iters))
        elif phase == 'val':
            val_set = create_dataset(dataset_opt)   # (scored clip-wise from its cache: no loader)
            if rank <= 0:
                logger.info('Number of val images in [{:s}]: {:d}'.format(dataset_opt['name'], len(val_set)))
        else:
            raise NotImplementedError('Phase [{:s}] is not recognized.'.format(phase))
    assert train_loader is not None

    model = create_model(opt)
    try:
        return train(opt, model, train_loader, val_set=val_set, train_sampler=train_sampler, resume_state=resume_state,
                     total_epochs=total_epochs, rank=rank, logger=logger, tb_logger=tb_logger)
    finally:
        if tb_logger is not None:
            tb_logger.close()


if __name__ == '__main__':
    main()
