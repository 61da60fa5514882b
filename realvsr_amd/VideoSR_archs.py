"""define_G for the generators on the MI355X path (codes/models/VideoSR_archs.py:18-58: EDVR / EDVR_NoUp / TDAN / RCAN / FSTRN / TOF branches)."""
from .archs import EDVR_arch, FSTRN_arch, RCAN_arch, TDAN_arch, TOF_arch

_FSTRN_KEYS = ('k', 'nf', 'nframes')
_TOF_KEYS = ('nframes', 'K', 'nc', 'nf', 'nb')
_RCAN_KEYS = ('num_in_ch', 'num_out_ch', 'num_frames', 'num_feat', 'num_group', 'num_block', 'squeeze_factor', 'res_scale')


def define_G(opt):
    opt_net = opt['network_G']
    which_model = opt_net['which_model_G']
    if which_model in ('EDVR', 'EDVR_NoUp'):
        cls = EDVR_arch.EDVR if which_model == 'EDVR' else EDVR_arch.EDVR_NoUp
        get = opt_net.get if hasattr(opt_net, 'get') else (lambda k: opt_net[k])
        return cls(nf=opt_net['nf'], nc=opt_net['nc'], nframes=opt_net['nframes'], groups=opt_net['groups'],
                   front_RBs=opt_net['front_RBs'], back_RBs=opt_net['back_RBs'], center=get('center'),
                   predeblur=get('predeblur'), HR_in=get('HR_in'), w_TSA=get('w_TSA'))
    if which_model == 'TDAN':
        return TDAN_arch.TDAN(nf=opt_net['nf'], channel=opt_net['nc'], nframes=opt_net['nframes'], nb_f=opt_net['nb_f'],
                              nb_b=opt_net['nb_b'], groups=opt_net['groups'], scale=opt['scale'])
    if which_model == 'RCAN':
        # A block that only names the model is not a buildable request: the reference reads every one of these keys with [] and has no
        # defaults for them, so an incomplete block is refused like an unknown model (NotImplementedError) instead of a KeyError.
        missing = [k for k in _RCAN_KEYS if k not in opt_net] + ([] if 'scale' in opt else ['scale (in opt)'])
        if missing:
            raise NotImplementedError('Generator model [RCAN]: network_G lacks ' + ', '.join(missing))
        return RCAN_arch.RCAN(num_in_ch=opt_net['num_in_ch'], num_out_ch=opt_net['num_out_ch'], num_frames=opt_net['num_frames'],
                              num_feat=opt_net['num_feat'], num_group=opt_net['num_group'], num_block=opt_net['num_block'],
                              squeeze_factor=opt_net['squeeze_factor'], upscale=opt['scale'], res_scale=opt_net['res_scale'])
    if which_model == 'FSTRN':
        # as for RCAN: the reference reads k, nf, nframes and opt['scale'] with [] and has no defaults for them
        missing = [k for k in _FSTRN_KEYS if k not in opt_net] + ([] if 'scale' in opt else ['scale (in opt)'])
        if missing:
            raise NotImplementedError('Generator model [FSTRN]: network_G lacks ' + ', '.join(missing))
        return FSTRN_arch.FSTRN(k=opt_net['k'], nf=opt_net['nf'], nframes=opt_net['nframes'], scale=opt['scale'])
    if which_model == 'TOF':
        # as for RCAN: the reference reads these keys and opt['scale'] with [] and has no defaults for them
        missing = [k for k in _TOF_KEYS if k not in opt_net] + ([] if 'scale' in opt else ['scale (in opt)'])
        if missing:
            raise NotImplementedError('Generator model [TOF]: network_G lacks ' + ', '.join(missing))
        return TOF_arch.TOF(nframes=opt_net['nframes'], K=opt_net['K'], in_nc=opt_net['nc'], out_nc=opt_net['nc'], nf=opt_net['nf'],
                            nb=opt_net['nb'], upscale=opt['scale'])
    raise NotImplementedError('Generator model [{:s}] not recognized'.format(which_model))


def define_D(opt):
    """define_D (codes/models/VideoSR_archs.py:64-105) for the patch discriminators; every other branch is refused."""
    import torch.nn as nn
    from .archs import discriminator_arch
    opt_net = opt['network_D']
    which_model = opt_net['which_model_D']
    if which_model == 'PatchDiscriminator':
        return discriminator_arch.PatchDiscriminator(input_nc=opt_net['in_nc'], ndf=opt_net['nf'], norm_layer=nn.BatchNorm2d)
    if which_model == 'MultiscaleDiscriminator_v4':
        return discriminator_arch.MultiscaleDiscriminator_v4(input_nc=opt_net['in_nc'], ndf=opt_net['nf'], num_D=opt_net['num_D'],
                                                             norm_layer=nn.BatchNorm2d, gan_type=opt_net['gan_type'])
    raise NotImplementedError('Discriminator model [{:s}] is not built'.format(which_model))
