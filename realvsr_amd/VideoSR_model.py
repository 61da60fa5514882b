"""The caller of the hot path: one training / test step with the reference's model API.

Mirrors ``VideoSRModel`` of codes/models/VideoSR_AllPair_model_YCbCr_Split.py (:22-151 constructor, :154-157 feed_data,
:163-191 optimize_parameters, :193-197 test) and of ..._YCbCr_Combine.py (:187-221), plus ``create_model``
(codes/models/__init__.py:5-17): same ``opt`` dictionary keys, same method names, same step sequence

    zero_grad -> (augment) -> netG(var_L) -> w_y * cri_y(fake[:, 0:1], GT[:, c, 0:1]) + w_c * cri_c(fake[:, 1:3], GT[:, c, 1:3])
              -> backward -> Adam step

MI355X wiring instead of DataParallel / DistributedDataParallel + torch.optim.Adam:
  * parameters, gradients and Adam moments live in flat buffers (optim.FlatAdam): zero_grad is one memset, the
    optimizer step one kernel;
  * with ``opt['dist']`` every rank (one process per GPU) starts from rank 0's parameters and the gradient buffer is
    all-reduced in buckets over RCCL while backward is still running (dist.BucketedGradAllReduce);
  * augmentation runs as one kernel on the device-resident clip pair (augment.apply_augment).
The learning-rate schedule, checkpoints and resume of codes/models/base_model.py:38-67, 121-141 are ``_TrainingState`` below, shared by
both model classes through ``_VideoSRBase``, which holds everything else the two have in common; realvsr_amd.train is the loop that
calls them.  Out of scope: the VGG feature loss.
``VideoSRGANModel`` below is the GAN stage (VideoSRGAN_AllPair_model_YCbCr_Split.py) on the same machinery.
"""
import os
from collections import OrderedDict

import torch

from . import VideoSR_archs as networks
from . import augment as augments
from . import loss as L
from . import lr_scheduler
from .data import feed_packed
from .dist import BucketedGradAllReduce, broadcast_parameters
from .optim import FlatAdam


def _criterion(name, nc, role):
    """The loss table of the reference's constructor (..._Split.py:45-85, ..._Combine.py:44-82)."""
    if name == 'l1':
        return L.L1Loss(reduction='mean')
    if name == 'l2':
        return L.MSELoss(reduction='mean')
    if name == 'cb':
        return L.CharbonnierLoss(reduction='mean')
    if name == 'hb':
        return L.HuberLoss(reduction='mean')
    if name == 'gw' and role != 'combine':
        return L.GWLoss(w=4, reduction='mean')
    if name == 'pyr':
        return L.PyramidLoss(num_levels=3, pyr_mode='lap' if role == 'edge' else 'gau', loss_mode='cb', reduction='mean')
    if name == 'lappyr':
        return L.LapPyrLoss(num_levels=3, lf_mode='ssim', hf_mode='cb', reduction='mean')
    # 'msssim' (IQA_pytorch.MS_SSIM) is selected by no shipped option file and is not on the hot path
    raise NotImplementedError('Loss type [{:s}] is not recognized.'.format(str(name)))


class _TrainingState:
    """What the reference's BaseModel gives its training loop (codes/models/base_model.py:38-67, 121-141; codes/train.py:141, 156,
    326-327), for a class with ``opt``, ``optimizers``, ``schedulers``, ``netG`` and ``save_network``."""

    def _build_schedulers(self, train_opt, multistep_name):
        """One scheduler per optimizer from train_opt['lr_scheme'] (..._Split.py:127-150, VideoSRGAN_..._Split.py:163-181; the GAN
        constructor spells the multi-step scheme 'MultiStepLR').  Without the key: no scheduler, the rate stays what the optimizer got."""
        scheme = train_opt.get('lr_scheme')
        if scheme is None:
            return
        for optimizer in self.optimizers:
            if scheme == multistep_name:
                sched = lr_scheduler.MultiStepLR_Restart(optimizer, train_opt['lr_steps'], restarts=train_opt.get('restarts'),
                                                         weights=train_opt.get('restart_weights'), gamma=train_opt['lr_gamma'],
                                                         clear_state=train_opt.get('clear_state'))
            elif scheme == 'CosineAnnealingLR_Restart':
                sched = lr_scheduler.CosineAnnealingLR_Restart(optimizer, train_opt['T_period'], eta_min=train_opt['eta_min'],
                                                               restarts=train_opt.get('restarts'), weights=train_opt.get('restart_weights'))
            else:
                raise NotImplementedError('lr_scheme [{:s}] is not recognized ({:s} | CosineAnnealingLR_Restart)'.format(
                    str(scheme), multistep_name))
            # the loop steps the schedule BEFORE the optimizer (train.py:156, 160), as the reference does; torch's one-time
            # warning about that order assumes the opposite convention
            optimizer._opt_called = True
            self.schedulers.append(sched)

    def _set_lr(self, lr_groups_l):
        """Set the rates for warm-up; lr_groups_l: one list of rates per optimizer."""
        for optimizer, lr_groups in zip(self.optimizers, lr_groups_l):
            for param_group, lr in zip(optimizer.param_groups, lr_groups):
                param_group['lr'] = lr

    def _get_init_lr(self):
        """The initial rates, which the schedulers recorded in the groups."""
        return [[g['initial_lr'] for g in optimizer.param_groups] for optimizer in self.optimizers]

    def update_learning_rate(self, cur_iter, warmup_iter=-1):
        """Host scalars only: the rate reaches the device as an argument of FlatAdam's kernel."""
        for scheduler in self.schedulers:
            scheduler.step()
        if cur_iter < warmup_iter:
            self._set_lr([[v / warmup_iter * cur_iter for v in init_lr_g] for init_lr_g in self._get_init_lr()])

    def _networks_to_save(self):
        return [('G', self.netG)]

    def save(self, iter_step):
        for label, network in self._networks_to_save():
            self.save_network(network, os.path.join(self.opt['path']['models'], '{}_{}.pth'.format(iter_step, label)))

    def save_training_state(self, epoch, iter_step):
        """{'epoch', 'iter', 'schedulers', 'optimizers'} with torch.optim.Adam's state_dict layout, as the reference writes it."""
        state = {'epoch': epoch, 'iter': iter_step, 'schedulers': [s.state_dict() for s in self.schedulers],
                 'optimizers': [o.state_dict() for o in self.optimizers]}
        torch.save(state, os.path.join(self.opt['path']['training_state'], '{}.state'.format(iter_step)))

    def resume_training(self, resume_state):
        """Optimizers (into the flat moments: FlatAdam.load_state_dict) and schedulers; the networks come from pretrain_model_G / _D,
        which options.check_resume points at the checkpoint."""
        resume_optimizers = resume_state['optimizers']
        resume_schedulers = resume_state['schedulers']
        assert len(resume_optimizers) == len(self.optimizers), 'Wrong lengths of optimizers'
        assert len(resume_schedulers) == len(self.schedulers), 'Wrong lengths of schedulers'
        for i, o in enumerate(resume_optimizers):
            self.optimizers[i].load_state_dict(o)
        for i, s in enumerate(resume_schedulers):
            self.schedulers[i].load_state_dict(s)


def _is_packed(data):
    """Packed crops of realvsr_amd.data: the f32 batch is assembled on the device."""
    return 'GT_window' in data or data['LQs'].dtype == torch.uint8


class _VideoSRBase(_TrainingState):
    """What the two model classes share beyond the schedules and checkpoints: the set-up around their own refusals, the methods
    realvsr_amd.train calls on either of them, and the parts of a step that do not depend on its losses."""

    def __init__(self, opt):
        if opt.get('gpu_ids', 0) is None or not torch.cuda.is_available():
            raise NotImplementedError('realvsr_amd runs on MI355X only: there is no CPU path (gpu_ids=None)')
        self.opt = opt
        self.is_train = opt['is_train']
        self.dist = bool(opt.get('dist'))

    def _init_device_state(self):
        """The first device call of a constructor: after every refusal that reads only the options."""
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.rank = torch.distributed.get_rank() if self.dist else -1
        self.schedulers, self.optimizers = [], []
        self.log_dict = OrderedDict()

    def _build_reducer(self, buffers):
        """The bucketed all-reduce over one optimizer's flat gradient buffer (the parameters were broadcast when the network was built)."""
        train_opt = self.opt['train']
        return BucketedGradAllReduce(None, bucket_mb=float(os.environ.get('RVSR_BUCKET_MB', train_opt.get('bucket_mb', 4.0))),
                                     buffers=buffers, broadcast=False, force=bool(train_opt.get('force_allreduce')))

    # ------------------------------------------------------------------ data
    def feed_data(self, data, need_GT=True):
        if _is_packed(data):
            self.var_L, var_H = feed_packed(data, self.device, need_GT)
            if need_GT:
                self.var_H = var_H
            return
        self.var_L = data['LQs'].to(self.device)
        if need_GT:
            self.var_H = data['GT'].to(self.device)

    def _center_frame(self, clip):
        """[B, N, C, H, W] -> the centre frame, N being var_L's; a tensor that holds the centre frame only as is."""
        return clip[:, self.var_L.size(1) // 2] if clip.dim() == 5 else clip

    # ------------------------------------------------------------------ the parts of a step both models have
    @staticmethod
    def _zero_grad(optimizer, reducer, passes=1):
        if reducer is not None:
            reducer.zero_grad(passes=passes)
        else:
            optimizer.zero_grad()

    @staticmethod
    def _finish_and_step(optimizer, reducer):
        if reducer is not None:
            reducer.finish()
        optimizer.step()

    def _augment(self):
        aug = self.opt.get('augment')
        if aug:
            self.var_H, self.var_L = augments.apply_augment(self.var_H, self.var_L, aug['augs'], aug['probs'],
                                                            aug['alphas'], aug['mix_p'])

    def _keep_terms(self, terms, log):
        self.loss_terms = terms
        if log:
            for k, v in terms.items():
                self.log_dict[k] = v.item()

    def test(self):
        self.netG.eval()
        with torch.no_grad():
            self.fake_H = self.netG(self.var_L)
        self.netG.train()

    # ------------------------------------------------------------------ bookkeeping
    def get_current_log(self):
        return self.log_dict

    def get_current_visuals(self, need_GT=True):
        out = OrderedDict()
        out['LQs'] = self.var_L.detach()[0].float().cpu()
        out['HQ'] = self.fake_H.detach()[0].float().cpu()
        if need_GT:
            out['GT'] = self.var_H.detach()[0].float().cpu()
        return out

    def get_current_metrics(self, ssim=False, crop_border=0):
        """After feed_data + test(): {'psnr': [per sample], 'ssim': [per sample]} of fake_H against the GT (the centre frame of a
        five-dimensional var_H) on channel 0 -- the numbers the validation loop of codes/train.py:285-305 gets out of
        get_current_visuals + tensor2img + calculate_psnr, computed on the device (realvsr_amd.metrics): only the scalars come back."""
        from . import metrics
        gt = self._center_frame(self.var_H)
        res = metrics.frame_metrics(self.fake_H.detach(), gt.detach(), crop_border=crop_border, ssim=ssim)
        res.setdefault('ssim', [])
        return res

    def get_current_learning_rate(self):
        return [g['lr'] for g in self.optimizers[0].param_groups]

    def load(self):
        path = self.opt.get('path') or {}
        if path.get('pretrain_model_G') is not None:
            self.load_network(path['pretrain_model_G'], self.netG, path.get('strict_load', True))

    def load_network(self, load_path, network, strict=True):
        sd = torch.load(load_path, map_location='cpu')
        network.load_state_dict(OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in sd.items()),
                                strict=strict)

    def save_network(self, network, save_path):
        torch.save(OrderedDict((k, v.cpu()) for k, v in network.state_dict().items()), save_path)


class VideoSRModel(_VideoSRBase):
    def __init__(self, opt, split=True):
        super().__init__(opt)
        self.split = split
        self._init_device_state()
        train_opt = opt.get('train') or {}

        self.netG = networks.define_G(opt).to(self.device)
        self.load()
        if self.dist:
            broadcast_parameters(self.netG)
        self.reducer = None
        if not self.is_train:
            return
        self.netG.train()
        nc = opt['network_G'].get('nc', 3)
        if split:
            self.cri_pix_y = _criterion(train_opt['pixel_criterion_y'], nc, 'y')
            self.l_pix_w_y = train_opt['pixel_weight_y']
            self.cri_pix_c = _criterion(train_opt['pixel_criterion_c'], nc, 'c')
            self.l_pix_w_c = train_opt['pixel_weight_c']
        else:
            self.cri_pix = _criterion(train_opt['pixel_criterion'], nc, 'combine')
            self.l_pix_w = train_opt['pixel_weight']
            self.cri_edg = None
            if train_opt.get('edge_criterion') and train_opt.get('edge_weight'):
                self.cri_edg = _criterion(train_opt['edge_criterion'], nc, 'edge')
                self.l_edg_w = train_opt['edge_weight']
            if train_opt.get('feature_criterion') and train_opt.get('feature_weight'):
                raise NotImplementedError('the VGG feature loss is outside the hot path (SURVEY.md section 2)')

        trainable = [(k, v) for k, v in self.netG.named_parameters() if v.requires_grad]
        if train_opt.get('ft_tsa_only'):
            groups = [{'params': [v for k, v in trainable if 'tsa_fusion' not in k], 'lr': train_opt['lr_G']},
                      {'params': [v for k, v in trainable if 'tsa_fusion' in k], 'lr': train_opt['lr_G']}]
        else:
            groups = [v for _, v in trainable]
        self.optimizer_G = FlatAdam(groups, lr=train_opt['lr_G'], weight_decay=train_opt.get('weight_decay_G') or 0,
                                    betas=(train_opt['beta1'], train_opt['beta2']))
        self.optimizers.append(self.optimizer_G)
        self._build_schedulers(train_opt, 'MultiStepLR_Restart')
        if self.dist:
            self.reducer = self._build_reducer(self.optimizer_G.buffers)

    # ------------------------------------------------------------------ one optimisation step
    def set_params_lr_zero(self):
        self.optimizers[0].param_groups[0]['lr'] = 0

    def forward_loss(self):
        """netG forward + the weighted criteria; returns (total, OrderedDict of the named terms) as device scalars."""
        self.fake_H = self.netG(self.var_L)
        gt = self._center_frame(self.var_H)
        terms = OrderedDict()
        if self.split:
            terms['l_pix_y'] = self.l_pix_w_y * self.cri_pix_y(self.fake_H[:, 0:1], gt[:, 0:1])
            terms['l_pix_c'] = self.l_pix_w_c * self.cri_pix_c(self.fake_H[:, 1:3], gt[:, 1:3])
            total = terms['l_pix_y'] + terms['l_pix_c']
            terms['l_pix'] = total
        else:
            total = self.l_pix_w * self.cri_pix(self.fake_H, gt.contiguous())
            if self.cri_edg is not None:
                terms['l_edg'] = self.l_edg_w * self.cri_edg(self.fake_H, gt.contiguous())
                total = total + terms['l_edg']
            terms['l_tot'] = total
        return total, terms

    def optimize_parameters(self, step, log=True):
        """``log=False`` skips the .item() host syncs of the reference's log_dict (the values stay on the device in
        ``self.loss_terms``): the step is then free of host synchronisation."""
        train_opt = self.opt['train']
        if train_opt.get('ft_tsa_only') and step < train_opt['ft_tsa_only']:
            self.set_params_lr_zero()
        self._zero_grad(self.optimizer_G, self.reducer)
        self._augment()
        total, terms = self.forward_loss()
        total.backward()
        self._finish_and_step(self.optimizer_G, self.reducer)
        self._keep_terms(terms, log)


def _gan_pixel_criterion(name, channels):
    """The pixel-criterion table of the GAN model's constructor (VideoSRGAN_AllPair_model_YCbCr_Split.py:50-115)."""
    if name == 'ssim':
        return L.SSIM(channels=channels)
    if name == 'gw':
        return L.GWLoss(w=4, reduction='mean')
    if name in ('l1', 'l2', 'cb', 'hb'):
        return _criterion(name, 3, 'y')
    raise NotImplementedError('Loss type [{:s}] is not recognized.'.format(str(name)))


class VideoSRGANModel(_VideoSRBase):
    """``VideoSRGANModel`` of codes/models/VideoSRGAN_AllPair_model_YCbCr_Split.py (:23-183 constructor, :185-191 feed_data, :193-317
    optimize_parameters): G = the generator of define_G, D = define_D's patch discriminator on the two high-frequency Laplacian bands
    of Y; pixel terms on the pyramid (SSIM / Charbonnier on the bands, GWLoss on CbCr) + the ('ra')GAN term, then the D step (two
    backward passes: real, fake).  Both optimizers are FlatAdam; every operator is a HIP kernel (discriminator_arch, loss.GANLoss).
    The reference's call order of D -- hence the BatchNorm running statistics -- is kept: 5 forwards per RaGAN step, 3 per vanilla step,
    2 of them skipped on steps without a G update.

    With ``opt['dist']`` (one process per GPU, the reference's DistributedDataParallel around netG and netD) every rank starts from
    rank 0's parameters and buffers, and each optimizer's flat gradient buffer has its own dist.BucketedGradAllReduce: G's buckets
    leave during the G backward (D is frozen there, so only G's hooks fire); D's reducer is armed for two passes and its buckets leave
    during the second one (l_d_fake.backward()).  Steps without a G update issue no G collective on any rank (the condition depends on
    `step` alone).  BatchNorm in D normalises with the batch statistics of the rank's own shard, as the reference's plain BatchNorm2d
    under DDP does (no SyncBN); the running statistics are not exchanged -- D never runs in eval mode, so they never feed back into a
    step, and rank 0, which writes the checkpoints, saves its own (what the reference's per-forward re-broadcast of rank 0's buffers
    amounts to, without its traffic).  The logged terms are the local rank's.
    Out of scope (NotImplementedError): the CPU path, opt['dist'] without a process group, the VGG feature loss, 'lsgan' / 'wgan-gp'."""

    def __init__(self, opt):
        super().__init__(opt)
        if self.dist and not torch.distributed.is_initialized():
            raise NotImplementedError('VideoSRGANModel: distributed training needs an initialised process group, one process per GPU '
                                      '(python -m torch.distributed.run ... -m realvsr_amd.train -opt FILE --launcher pytorch)')
        train_opt = opt.get('train') or {}
        if self.is_train:
            if (train_opt.get('feature_weight') or 0) > 0:
                raise NotImplementedError('VideoSRGANModel: the VGG feature loss (feature_weight > 0) is not built')
            gan_type = train_opt['gan_type']
            if gan_type not in ('gan', 'ragan'):
                raise NotImplementedError('VideoSRGANModel: gan_type %r is not built (gan | ragan)' % (gan_type,))
        self._init_device_state()

        self.netG = networks.define_G(opt).to(self.device)
        self.netD = None
        if self.is_train:
            self.netD = networks.define_D(opt).to(self.device)
            self.netG.train()
            self.netD.train()
        self.load()
        if self.dist:
            broadcast_parameters(self.netG)
            if self.netD is not None:
                broadcast_parameters(self.netD)
        self.reducer_G = self.reducer_D = None
        if not self.is_train:
            return

        def crit(key, channels):
            if (train_opt.get('pixel_weight_' + key) or 0) > 0:
                return _gan_pixel_criterion(train_opt['pixel_criterion_' + key], channels), train_opt['pixel_weight_' + key]
            return None, 0
        self.cri_pix_s, self.l_pix_w_s = crit('s', 1)
        self.cri_pix_d, self.l_pix_w_d = crit('d', 1)
        self.cri_pix_c, self.l_pix_w_c = crit('c', 2)
        self.cri_gan = L.GANLoss(train_opt['gan_type'], 1.0, 0.0)
        self.l_gan_w = train_opt['gan_weight']
        self.D_update_ratio = train_opt.get('D_update_ratio') or 1
        self.D_init_iters = train_opt.get('D_init_iters') or 0

        self.optimizer_G = FlatAdam([v for v in self.netG.parameters() if v.requires_grad], lr=train_opt['lr_G'],
                                    weight_decay=train_opt.get('weight_decay_G') or 0, betas=(train_opt['beta1_G'], train_opt['beta2_G']))
        self.optimizers.append(self.optimizer_G)
        self.optimizer_D = FlatAdam(list(self.netD.parameters()), lr=train_opt['lr_D'], weight_decay=train_opt.get('weight_decay_D') or 0,
                                    betas=(train_opt['beta1_D'], train_opt['beta2_D']))
        self.optimizers.append(self.optimizer_D)
        self._build_schedulers(train_opt, 'MultiStepLR')
        if self.dist:
            self.reducer_G = self._build_reducer(self.optimizer_G.buffers)
            self.reducer_D = self._build_reducer(self.optimizer_D.buffers)

    # ------------------------------------------------------------------ data
    def feed_data(self, data, need_GT=True):
        super().feed_data(data, need_GT)
        if need_GT:
            if _is_packed(data):   # (a packed 'ref' is not defined: the GT is the reference)
                self.var_ref = self.var_H
            else:
                self.var_ref = (data['ref'] if 'ref' in data else data['GT']).to(self.device)

    # ------------------------------------------------------------------ one optimisation step
    def _set_requires_grad_D(self, flag):
        for p in self.netD.parameters():
            p.requires_grad = flag

    def optimize_parameters(self, step, log=True):
        """``log=False`` skips the .item() host syncs of the reference's log_dict (the device scalars stay in ``self.loss_terms``)."""
        from . import util
        # G
        self._set_requires_grad_D(False)
        self._zero_grad(self.optimizer_G, self.reducer_G)
        self._augment()
        self.fake_H = self.netG(self.var_L)
        gt, ref = self._center_frame(self.var_H), self._center_frame(self.var_ref)
        fake_y, fake_c = self.fake_H[:, 0:1], self.fake_H[:, 1:3]
        real_y, real_c = gt[:, 0:1].contiguous(), gt[:, 1:3].contiguous()
        fake_pyr = util.laplacian_pyramid(img=fake_y, max_levels=3)
        real_pyr = util.laplacian_pyramid(img=real_y, max_levels=3)
        ref_pyr = util.laplacian_pyramid(img=ref[:, 0:1].contiguous(), max_levels=3)
        ragan = self.cri_gan.gan_type == 'ragan'
        terms = OrderedDict()
        if step % self.D_update_ratio == 0 and step > self.D_init_iters:
            total = 0
            if self.cri_pix_s is not None:
                terms['l_g_pix_s'] = self.l_pix_w_s * self.cri_pix_s(fake_pyr[-1], real_pyr[-1])
                total = total + terms['l_g_pix_s']
            if self.cri_pix_d is not None:
                terms['l_g_pix_d'] = self.l_pix_w_d * self.cri_pix_d(fake_pyr[0], real_pyr[0]) + \
                    self.l_pix_w_d * self.cri_pix_d(fake_pyr[1], real_pyr[1])
                total = total + terms['l_g_pix_d']
            if self.cri_pix_c is not None:
                terms['l_g_pix_c'] = self.l_pix_w_c * self.cri_pix_c(fake_c, real_c)
                total = total + terms['l_g_pix_c']
            l_g_gan = 0
            if ragan:
                with torch.no_grad():   # (its outputs are detached in the reference: same values, same BN statistics, no graph)
                    pred_d_real = self.netD(ref_pyr[:-1])
                pred_g_fake = self.netD(fake_pyr[:-1])
                for i in range(len(pred_d_real)):
                    l_g_gan = l_g_gan + self.l_gan_w * (self.cri_gan(pred_d_real[i], False, other=pred_g_fake[i]) +
                                                        self.cri_gan(pred_g_fake[i], True, other=pred_d_real[i])) / 2
            else:
                pred_g_fake = self.netD(fake_pyr[:-1])
                for i in range(len(pred_g_fake)):
                    l_g_gan = l_g_gan + self.l_gan_w * self.cri_gan(pred_g_fake[i], True)
            terms['l_g_gan'] = l_g_gan
            total = total + l_g_gan
            terms['l_g_total'] = total
            total.backward()
            self._finish_and_step(self.optimizer_G, self.reducer_G)

        # D
        self._set_requires_grad_D(True)
        self._zero_grad(self.optimizer_D, self.reducer_D, passes=2)
        fake_in = [x.detach() for x in fake_pyr[:-1]]
        real_in = ref_pyr[:-1]
        l_d_real, l_d_fake = 0, 0
        if ragan:
            with torch.no_grad():
                pred_d_fake = self.netD(fake_in)
            pred_d_real = self.netD(real_in)
            for i in range(len(pred_d_fake)):
                l_d_real = l_d_real + self.cri_gan(pred_d_real[i], True, other=pred_d_fake[i]) * 0.5
            l_d_real.backward()
            pred_d_fake = self.netD(fake_in)
            for i in range(len(pred_d_fake)):
                l_d_fake = l_d_fake + self.cri_gan(pred_d_fake[i], False, other=pred_d_real[i].detach()) * 0.5
            l_d_fake.backward()
        else:
            pred_d_real = self.netD(real_in)
            for i in range(len(pred_d_real)):
                l_d_real = l_d_real + self.cri_gan(pred_d_real[i], True)
            l_d_real.backward()
            pred_d_fake = self.netD(fake_in)
            for i in range(len(pred_d_fake)):
                l_d_fake = l_d_fake + self.cri_gan(pred_d_fake[i], False)
            l_d_fake.backward()
        self._finish_and_step(self.optimizer_D, self.reducer_D)
        terms['l_d_real'] = l_d_real.detach()
        terms['l_d_fake'] = l_d_fake.detach()
        self._keep_terms(terms, log)

    # ------------------------------------------------------------------ bookkeeping
    def load(self):
        super().load()
        path = self.opt.get('path') or {}
        if self.is_train and path.get('pretrain_model_D') is not None:
            self.load_network(path['pretrain_model_D'], self.netD, path.get('strict_load', True))

    def _networks_to_save(self):
        return [('G', self.netG), ('D', self.netD)]


def create_model(opt):
    model = opt['model']
    if model == 'VideoSR_AllPair_YCbCr_Split':
        return VideoSRModel(opt, split=True)
    if model == 'VideoSR_AllPair_YCbCr_Combine':
        return VideoSRModel(opt, split=False)
    if model == 'VideoSRGAN_AllPair_YCbCr_Split':
        return VideoSRGANModel(opt)
    raise NotImplementedError('Model [{:s}] not recognized.'.format(str(model)))
