"""The input side of a training step: RealVSR clips as packed uint8 crops, assembled into the f32 batch on the device.

Mirrors codes/data/RealVSR_dataset.py (RealVSRDataset :15-177, RealVSRAllPairDataset :180-346) and the part of codes/data/util.py they
use (read_img :86-101, read_img_seq :104-122, augment :261-276), split where the bytes stop being integers:

  host (this module, numpy / CPU torch only)     choose the frames, draw the crop and the flips from `random` in the reference's order
                                                 (draw_sample), copy S uint8 rows per frame into pinned memory (ClipBatchStager)
  device (csrc/batch_kernels.hip)                float(u8) / 255, hflip / vflip / rot90, [2, 1, 0], HWC -> CHW, one launch per tensor
                                                 (assemble_batch); optionally the YCbCr conversion of scripts/prepare_data.py

The reference converts every WHOLE 1024 x 512 x 3 frame to float32 before it crops (util.py:95) and ships f32 over PCIe; here a quarter
of the bytes cross and no float is touched on the host.  Without the conversion the result equals the reference's chain bit for bit
(one correctly rounded division and a permutation); tests/test_data_host.py and tests/test_gpu_batch.py hold that with ==.

Vimeo-90K (codes/data/Vimeo90K_dataset.py; Vimeo90kDataset, Vimeo90kAllPairDataset below) goes the same way, and can do without its
second copy on disk: with opt['synthesize_LQ'] a sample carries a WINDOW of the GT frames (the crop plus the halo of the bicubic taps)
and the device computes the LQ crop from it (csrc/resize_kernels.hip, bicubic_u8): MATLAB's imresize chain of
scripts/generate_LR_BI_Vimeo90K.m in exact integers, bit-identical to cropping the degraded whole frame.

The datasets never load the HIP library or touch the device, so they are safe in DataLoader workers.
"""
import os
import pickle
import random

import numpy as np
import torch

RVSR_ASM_REVERSE = 1    # include/realvsr_hip.h, section 12 (tests/test_data_host.py holds the two copies together)
RVSR_ASM_TO_YCBCR = 2
RVSR_BIC_SAME = 0       # include/realvsr_hip.h, section 13 (tests/test_bicubic_host.py holds the copies together)
RVSR_BIC_DOWN = 1
BIC_MODES = {'same': RVSR_BIC_SAME, 'down': RVSR_BIC_DOWN}
# what rvsr_bicubic_halo returns: 3 s / 2 for 'down', 4 s - 1 for 'same', derived from the tap tables in csrc/resize_kernels.hip and
# tests/bicubic_reference.py (the tests hold the three together); a copy, because DataLoader workers must not load the library
BIC_HALO = {(2, RVSR_BIC_SAME): 7, (2, RVSR_BIC_DOWN): 3, (4, RVSR_BIC_SAME): 15, (4, RVSR_BIC_DOWN): 6}
FLAG_HFLIP, FLAG_VFLIP, FLAG_ROT90 = 1, 2, 4
VIMEO_FRAME_CHW = (3, 256, 448)   # the size the reference hard-codes for the crop range (Vimeo90K_dataset.py:95, 102, 221, 231)
FRAME_CHW = (3, 1024, 512)   # the size the reference hard-codes for the crop range (RealVSR_dataset.py:121, 130, 284, 297)
LAST_FRAME = 49              # clips have 50 frames (RealVSR_dataset.py:89, 105)


def _refuse_lr_input(opt):
    if opt['GT_size'] != opt['LQ_size']:
        raise NotImplementedError('LR_input (GT_size %r != LQ_size %r: scale > 1 crops) is not built; every shipped option file has '
                                  'scale 1' % (opt['GT_size'], opt['LQ_size']))


def _refuse_color_conversion(opt):
    """util.channel_convert (codes/data/util.py:312-323) converts for 'gray' and 'y' (and grey files for 'RGB') and passes everything
    else through -- 'ycbcr', what every shipped option file says, included: the data sets are stored pre-converted."""
    if opt.get('color') in ('gray', 'y'):
        raise NotImplementedError("opt['color'] = %r: the data sets are stored pre-converted (channel_convert is a no-op for every "
                                  'shipped option file)' % (opt['color'],))


def draw_sample(opt, key, rng=random, frame_chw=FRAME_CHW):
    """The random choices of one RealVSRDataset / RealVSRAllPairDataset sample for `key` ('017_00023'), drawn from `rng` in exactly the
    order of the reference's __getitem__ (RealVSR_dataset.py:72-163, 235-330; both classes draw alike):
      1. rng.choice(interval_list)
      2. border_mode: [random() < 0.5 and choice([0, 1])] under random_reverse      (:84-102)
         else:        the `while ... randint(0, 49)` redraw of the centre, then [random() < 0.5] under random_reverse   (:103-115)
      3. phase 'train': randint for the crop's row, then its column                  (:154-155)
      4. util.augment's three short-circuited draws: use_flip and random(), use_rot and random(), use_rot and random()   (util.py:263-265)
    Returns a dict: name_a (sequence), neighbor_list (frame indices of the LQ window -- and of the GT window of the all-pair class),
    center (the five-digit name of the single GT frame of RealVSRDataset), rnd_h, rnd_w (None outside phase 'train'), size, flags
    (bit 0 hflip, bit 1 vflip, bit 2 rot90), key."""
    _refuse_lr_input(opt)
    name_a, name_b = key.split('_')
    center = int(name_b)
    N = opt['N_frames']
    half = N // 2
    interval = rng.choice(opt['interval_list'])
    if opt['border_mode']:
        direction = 1
        if opt['random_reverse'] and rng.random() < 0.5:
            direction = rng.choice([0, 1])
        if center + interval * (N - 1) > LAST_FRAME:
            direction = 0
        elif center - interval * (N - 1) < 0:
            direction = 1
        step = interval if direction == 1 else -interval
        neighbor_list = list(range(center, center + step * N, step))
        name_b = '{:05d}'.format(neighbor_list[0])
    else:
        while center + half * interval > LAST_FRAME or center - half * interval < 0:
            center = rng.randint(0, LAST_FRAME)
        neighbor_list = list(range(center - half * interval, center + half * interval + 1, interval))
        if opt['random_reverse'] and rng.random() < 0.5:
            neighbor_list.reverse()
        name_b = '{:05d}'.format(neighbor_list[half])
    assert len(neighbor_list) == N, 'Wrong length of neighbor list: {}'.format(len(neighbor_list))
    rnd_h = rnd_w = None
    flags = 0
    if opt['phase'] == 'train':
        _, H, W = frame_chw
        size = opt['GT_size']
        rnd_h = rng.randint(0, max(0, H - size))
        rnd_w = rng.randint(0, max(0, W - size))
        if opt['use_flip'] and rng.random() < 0.5:
            flags |= FLAG_HFLIP
        if opt['use_rot'] and rng.random() < 0.5:
            flags |= FLAG_VFLIP
        if opt['use_rot'] and rng.random() < 0.5:
            flags |= FLAG_ROT90
    return {'key': key, 'name_a': name_a, 'neighbor_list': neighbor_list, 'center': name_b, 'rnd_h': rnd_h, 'rnd_w': rnd_w,
            'size': opt['GT_size'] if rnd_h is not None else None, 'flags': flags}


def crop_u8(frame, plan):
    """The plan's S x S crop of one uint8 frame [H, W] or [H, W, C] as a view [S, S, C] (the whole frame outside phase 'train').
    Raises ValueError if the crop leaves the frame: the reference would build ragged arrays and fail in np.stack."""
    if frame.dtype != np.uint8:
        raise ValueError('frames are uint8, got %s' % frame.dtype)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    if frame.shape[2] > 3:
        frame = frame[:, :, :3]   # (some images have 4 channels: util.py:98-100)
    if plan['rnd_h'] is not None:
        h, w, S = plan['rnd_h'], plan['rnd_w'], plan['size']
        if h < 0 or w < 0 or h + S > frame.shape[0] or w + S > frame.shape[1]:
            raise ValueError('the %d x %d crop at (%d, %d) leaves the %d x %d frame' % (S, S, h, w, frame.shape[0], frame.shape[1]))
        frame = frame[h:h + S, w:w + S]
    return frame


class ClipBatchStager(object):
    """Pinned staging of one batch of uint8 crops, `slots` deep.  A slot is ONE uint8 block holding, in this order, the flags
    (int32 [B]), LQ [B, frames_lq, S, S, C] and GT [B, frames_gt, S, S, C] (frames_gt = N for the all-pair class, 1 otherwise), so a
    batch crosses PCIe in a single copy; LQ and GT therefore start at whatever byte the sizes give (the kernel takes any alignment).
        for i, plan in enumerate(plans): stager.stage(i, lq_frames, gt_frames, plan)      # integer slicing only
        lq, gt, flags = stager.upload()                                                   # non_blocking, current stream
        var_L, var_H = assemble_batch(lq, flags), assemble_batch(gt, flags)
    upload() moves on to the next slot, so staging batch k+1 overlaps step k; before a slot is written again the copy issued from it
    `slots` uploads ago is waited for.  pin=False keeps everything in pageable host memory (host tests; upload() is then unavailable)."""

    def __init__(self, batch, frames_lq, frames_gt, size, C, pin=True, slots=2):
        self.batch, self.frames_lq, self.frames_gt, self.size, self.C = batch, frames_lq, frames_gt, size, C
        self.pin = pin
        n_flags = 4 * batch
        n_lq = batch * frames_lq * size * size * C
        n_gt = batch * frames_gt * size * size * C
        self._cuts = (n_flags, n_flags + n_lq, n_flags + n_lq + n_gt)
        self._host = [torch.zeros(self._cuts[2], dtype=torch.uint8, pin_memory=pin) for _ in range(slots)]
        self._dev = [None] * slots
        self._done = [None] * slots
        self._slot = 0

    def _views(self, block):
        a, b, c = self._cuts
        B, S, C = self.batch, self.size, self.C
        return (block[a:b].view(B, self.frames_lq, S, S, C), block[b:c].view(B, self.frames_gt, S, S, C), block[:a].view(torch.int32))

    def host_views(self):
        """(LQ, GT, flags) of the slot being staged, as CPU tensors sharing its memory."""
        return self._views(self._host[self._slot])

    def stage(self, i, lq_frames_u8, gt_frames_u8, plan):
        """Sample i of the batch: the plan's crop of every frame (numpy uint8 [H, W, C], in the byte order the files hold)."""
        if len(lq_frames_u8) != self.frames_lq or len(gt_frames_u8) != self.frames_gt:
            raise ValueError('expected %d LQ and %d GT frames, got %d and %d'
                             % (self.frames_lq, self.frames_gt, len(lq_frames_u8), len(gt_frames_u8)))
        lq, gt, flags = (v.numpy() for v in self.host_views())
        for dst, frames in ((lq[i], lq_frames_u8), (gt[i], gt_frames_u8)):
            for n, frame in enumerate(frames):
                crop = crop_u8(frame, plan)
                if crop.shape != dst[n].shape:
                    raise ValueError('the crop is %s, the stager holds %s' % (crop.shape, dst[n].shape))
                dst[n] = crop
        flags[i] = plan['flags']

    def upload(self):
        """Copy the staged slot to the device (non_blocking, current stream) -> device views (LQ uint8, GT uint8, flags int32)."""
        if not self.pin:
            raise RuntimeError('ClipBatchStager(pin=False) is for host tests: there is nothing to upload from')
        s = self._slot
        if self._dev[s] is None:
            self._dev[s] = torch.empty(self._cuts[2], dtype=torch.uint8, device='cuda')
        self._dev[s].copy_(self._host[s], non_blocking=True)
        self._done[s] = torch.cuda.Event()
        self._done[s].record()
        self._slot = (s + 1) % len(self._host)
        if self._done[self._slot] is not None:
            self._done[self._slot].synchronize()   # (issued `slots` uploads ago)
        return self._views(self._dev[s])


def assemble_batch(u8, flags=None, mode=RVSR_ASM_REVERSE, out=None):
    """uint8 [B, F, Hs, Ws, C] on the GPU -> float32 [B, F, C, Ho, Wo] (rvsr_assemble_clips, include/realvsr_hip.h section 12).
    flags: int32 [B] on the GPU (bit 0 hflip, bit 1 vflip, bit 2 rot90; square crops only) or None; mode: RVSR_ASM_REVERSE |
    RVSR_ASM_TO_YCBCR.  `u8` may start at any byte (a view into a larger block); it has to be contiguous."""
    from . import _lib
    from ._lib import _p, _stream
    if not torch.is_tensor(u8) or not u8.is_cuda:
        raise RuntimeError('assemble_batch runs on MI355X (HIP) tensors only')
    if u8.dtype != torch.uint8 or u8.dim() != 5:
        raise RuntimeError('assemble_batch: expected uint8 [B, F, H, W, C], got %s %s' % (u8.dtype, tuple(u8.shape)))
    if not u8.is_contiguous():
        raise RuntimeError('assemble_batch: the packed tensor has to be contiguous')
    B, F, Hs, Ws, C = u8.shape
    if flags is not None:
        if not flags.is_cuda or flags.device != u8.device or flags.dtype != torch.int32 or not flags.is_contiguous() or flags.numel() != B:
            raise RuntimeError('assemble_batch: flags have to be a contiguous int32 [B] tensor on the device of the frames')
    if out is None:
        out = torch.empty(B, F, C, Hs, Ws, dtype=torch.float32, device=u8.device)
    elif (not out.is_cuda or out.device != u8.device or out.dtype != torch.float32 or not out.is_contiguous()
          or tuple(out.shape) != (B, F, C, Hs, Ws)):
        raise RuntimeError('assemble_batch: out has to be a contiguous float32 %s tensor on the device of the frames' % ((B, F, C, Hs, Ws),))
    if out.numel() == 0:
        raise RuntimeError('assemble_batch: empty shape %s' % (tuple(u8.shape),))
    with torch.cuda.device(u8.device):
        _lib.check(_lib.lib().rvsr_assemble_clips(_p(u8), _p(out), _p(flags), B, F, C, Hs, Ws, int(mode), _stream()), 'assemble_clips')
    return out


def assemble_plan(out_ptr_or_tensor, B, F, C, Hs, Ws):
    """(variant, workgroups) of the assemble_batch call that writes there: variant 1 = 16-byte stores, 0 = scalar stores."""
    import ctypes
    from . import _lib
    ptr = out_ptr_or_tensor.data_ptr() if torch.is_tensor(out_ptr_or_tensor) else int(out_ptr_or_tensor)
    variant, blocks = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib().rvsr_assemble_plan(ctypes.c_void_p(ptr), B, F, C, Hs, Ws, ctypes.byref(variant), ctypes.byref(blocks)),
               'assemble_plan')
    return variant.value, blocks.value


def clip_from_u8(frames_u8, mode=RVSR_ASM_REVERSE):
    """uint8 [T, H, W, C] (GPU; C = 1 or 3, in cv2's byte order for the default mode) -> float32 [T, C, H, W]: util.read_img_seq
    (codes/data/util.py:104-122) for the validation / test scripts, without the f32 frames on the host."""
    if not torch.is_tensor(frames_u8) or frames_u8.dim() != 4:
        raise RuntimeError('clip_from_u8: expected uint8 [T, H, W, C]')
    return assemble_batch(frames_u8.unsqueeze(0), None, mode)[0]


def feed_packed(data, device, need_GT=True):
    """The uint8 branch of the models' feed_data: {'LQs': uint8 [B, N, S, S, C], 'GT': uint8 [B, N | 1, S, S, C], 'flags': [B] ints,
    optional 'mode'} -> (var_L [B, N, C, H, W], var_H [B, N, C, H, W] or [B, C, H, W] for a single GT frame; None without need_GT).
    A batch with 'GT_window' in place of 'LQs' and 'GT' (synthesize_LQ samples) has its LQ computed on the device: _feed_window."""
    mode = data.get('mode', RVSR_ASM_REVERSE)
    if torch.is_tensor(mode):
        mode = mode.reshape(-1)[0]
    mode = int(mode)
    if 'GT_window' in data:
        return _feed_window(data, device, need_GT, mode)
    lq = data['LQs']
    flags = data.get('flags')
    if flags is not None:
        flags = torch.as_tensor(flags)
        if lq.shape[2] != lq.shape[3]:   # whole frames (validation): nothing was flipped
            if not flags.is_cuda and bool((flags != 0).any()):
                raise RuntimeError('feed_data: flips / rot90 need square crops, got %d x %d' % (lq.shape[2], lq.shape[3]))
            flags = None
        else:
            flags = flags.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
    var_L = assemble_batch(lq.to(device, non_blocking=True).contiguous(), flags, mode)
    var_H = None
    if need_GT:
        var_H = assemble_batch(data['GT'].to(device, non_blocking=True).contiguous(), flags, mode)
        if var_H.size(1) == 1:
            var_H = var_H[:, 0]
    return var_L, var_H


def _first_int(v):
    return int(v.reshape(-1)[0]) if torch.is_tensor(v) else int(v)


def _feed_window(data, device, need_GT, mode):
    """The 'GT_window' form of feed_packed (synthesize_LQ samples of the Vimeo-90K classes): {'GT_window': uint8 [B, N, Hw, Ww, C],
    'geom': int [B, 4], 'flags': [B] ints, 'synth_scale', 'synth_mode', 'frame_h', 'frame_w', 'crop_size', 'gt_index'} -> one
    bicubic_u8 launch that writes the LQ crop and the GT crop, then the two assemble_batch calls of the packed path.  With
    RVSR_ASM_TO_YCBCR the degradation runs on the raw colour bytes and the conversion after it, like the stored _ycbcr copies."""
    win = data['GT_window'].to(device, non_blocking=True).contiguous()
    S = _first_int(data['crop_size'])
    frame_hw = (_first_int(data['frame_h']), _first_int(data['frame_w']))
    geom = torch.as_tensor(data['geom']).to(dtype=torch.int32).reshape(-1, 4)
    lq, gt = bicubic_u8(win, _first_int(data['synth_scale']), _first_int(data['synth_mode']), geom=geom, frame_hw=frame_hw,
                        crop_hw=(S, S) if S else frame_hw, want_crop=True)   # (crop_size 0: whole frames, outside phase 'train')
    flags = None
    if S:
        flags = torch.as_tensor(data['flags']).to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
    var_L = assemble_batch(lq, flags, mode)
    var_H = None
    if need_GT:
        g = _first_int(data.get('gt_index', -1))
        if g >= 0:   # the single-frame class: the GT is the crop of the centre frame only
            gt = gt[:, g:g + 1].contiguous()
        var_H = assemble_batch(gt, flags, mode)
        if var_H.size(1) == 1:   # (as in feed_packed)
            var_H = var_H[:, 0]
    return var_L, var_H


def bicubic_halo(scale, mode):
    """rvsr_bicubic_halo: how many frame rows / columns beyond the crop the bicubic chain reads (host-side integers only)."""
    mode = BIC_MODES.get(mode, mode)
    if (scale, mode) not in BIC_HALO:
        raise ValueError('bicubic: scale %r (2 or 4), mode %r (%s)' % (scale, mode, ' | '.join(sorted(BIC_MODES))))
    return BIC_HALO[(scale, mode)]


def _check_bicubic_frame(frame_hw, scale):
    Hf, Wf = frame_hw
    if Hf % scale or Wf % scale:
        raise ValueError('bicubic: the %d x %d frame is no multiple of the scale %d (modcrop it first)' % (Hf, Wf, scale))
    if Hf < 2 * scale or Wf < 2 * scale:
        raise ValueError('bicubic: the %d x %d frame has an edge below 2 * scale = %d: one reflection no longer suffices'
                         % (Hf, Wf, 2 * scale))


def check_bicubic_geometry(geom, window_hw, frame_hw, crop_hw, scale, mode):
    """The part of rvsr_bicubic_u8's contract that the entry point cannot see because geom is device memory, for one sample's
    (wy, wx, y0, x0): crop and window inside the frame, DOWN origins at multiples of the scale, and the window holding every frame
    pixel the crop's outputs touch after reflection.  Raises ValueError."""
    h = bicubic_halo(scale, mode)
    mode = BIC_MODES.get(mode, mode)
    wy, wx, y0, x0 = (int(v) for v in geom)
    for name, w0, W, c0, S, F in (('rows', wy, window_hw[0], y0, crop_hw[0], frame_hw[0]),
                                  ('columns', wx, window_hw[1], x0, crop_hw[1], frame_hw[1])):
        if S <= 0 or c0 < 0 or c0 + S > F:
            raise ValueError('bicubic: the crop %s [%d, %d) leave the frame (%d)' % (name, c0, c0 + S, F))
        if W > F or w0 < 0 or w0 + W > F:
            raise ValueError('bicubic: the window %s [%d, %d) leave the frame (%d)' % (name, w0, w0 + W, F))
        if mode == RVSR_BIC_DOWN and (c0 % scale or S % scale):
            raise ValueError('bicubic: DOWN needs crop %s at multiples of the scale %d, got origin %d, size %d' % (name, scale, c0, S))
        lo, hi = c0 - h, c0 + S - 1 + h        # what the outputs touch, before reflection
        need_lo, need_hi = max(lo, 0), min(hi, F - 1)
        if lo < 0:
            need_lo, need_hi = 0, max(need_hi, min(-1 - lo, F - 1))
        if hi >= F:
            need_lo, need_hi = min(need_lo, max(2 * F - 1 - hi, 0)), F - 1
        if w0 > need_lo or w0 + W - 1 < need_hi:
            raise ValueError('bicubic: the window %s [%d, %d) do not cover [%d, %d], the crop plus its halo of %d after reflection'
                             % (name, w0, w0 + W, need_lo, need_hi, h))


def degrade_window_plan(plan, frame_hw, scale, mode):
    """Host-side integers only: from a crop plan (rnd_h, rnd_w, size in GT frame coordinates; rnd_h None = the whole frame) the window
    the host uploads -> ((wy, wx), (Hw, Ww), (wy, wx, y0, x0)): rows [clamp(y0 - h, 0, Hf - (S + 2 h)), + S + 2 h) with h the chain's
    halo, or the whole frame where that is smaller, and columns alike; the last tuple is the sample's `geom` row."""
    h = bicubic_halo(scale, mode)
    _check_bicubic_frame(frame_hw, scale)
    Hf, Wf = frame_hw
    if plan['rnd_h'] is None:
        return (0, 0), (Hf, Wf), (0, 0, 0, 0)
    y0, x0, S = plan['rnd_h'], plan['rnd_w'], plan['size']
    Hw, Ww = min(Hf, S + 2 * h), min(Wf, S + 2 * h)
    wy, wx = min(max(y0 - h, 0), Hf - Hw), min(max(x0 - h, 0), Wf - Ww)
    geom = (wy, wx, y0, x0)
    check_bicubic_geometry(geom, (Hw, Ww), frame_hw, (S, S), scale, mode)
    return (wy, wx), (Hw, Ww), geom


def bicubic_u8(u8, scale, mode='same', geom=None, frame_hw=None, crop_hw=None, want_crop=False):
    """uint8 [B, F, Hw, Ww, C] windows of frames on the GPU -> the bicubic chain's uint8 bytes at the crop (rvsr_bicubic_u8,
    include/realvsr_hip.h section 13): mode 'same' [B, F, S_h, S_w, C] (shrink by `scale`, enlarge by `scale`, rounded once), 'down'
    [B, F, S_h / scale, S_w / scale, C].  geom: int [B, 4] rows (wy, wx, y0, x0) -- on the host (checked here per sample, then
    uploaded) or already on the device (then where the windows sit is the caller's contract) -- or None: the tensors are whole frames.
    frame_hw, crop_hw default to the window's size.  want_crop: also return the window's own bytes at the crop, (dst, crop)."""
    from . import _lib
    from ._lib import _p, _stream
    if not torch.is_tensor(u8) or not u8.is_cuda:
        raise RuntimeError('bicubic_u8 runs on MI355X (HIP) tensors only')
    if u8.dtype != torch.uint8 or u8.dim() != 5:
        raise RuntimeError('bicubic_u8: expected uint8 [B, F, H, W, C], got %s %s' % (u8.dtype, tuple(u8.shape)))
    if not u8.is_contiguous():
        raise RuntimeError('bicubic_u8: the packed tensor has to be contiguous')
    if mode not in BIC_MODES and mode not in BIC_MODES.values():
        raise RuntimeError('bicubic_u8: mode %r (%s)' % (mode, ' | '.join(sorted(BIC_MODES))))
    mode = BIC_MODES.get(mode, mode)
    B, F, Hw, Ww, C = u8.shape
    frame_hw = (Hw, Ww) if frame_hw is None else tuple(int(v) for v in frame_hw)
    crop_hw = (Hw, Ww) if crop_hw is None else tuple(int(v) for v in crop_hw)
    if geom is not None:
        geom = torch.as_tensor(geom)
        if geom.dtype != torch.int32 or tuple(geom.shape) != (B, 4):
            raise RuntimeError('bicubic_u8: geom has to be an int32 [B, 4] tensor, got %s %s' % (geom.dtype, tuple(geom.shape)))
        if not geom.is_cuda:
            if (scale, mode) in BIC_HALO:   # (anything else is the entry point's refusal)
                for row in geom.tolist():
                    check_bicubic_geometry(row, (Hw, Ww), frame_hw, crop_hw, scale, mode)
            geom = geom.to(u8.device, non_blocking=True)
        elif geom.device != u8.device:
            raise RuntimeError('bicubic_u8: geom has to be on the device of the frames')
        geom = geom.contiguous()
    scale = int(scale)
    out_hw = (crop_hw[0] // scale, crop_hw[1] // scale) if mode == RVSR_BIC_DOWN and scale > 0 else crop_hw
    if B * F * C == 0 or min(out_hw) <= 0:
        raise RuntimeError('bicubic_u8: empty shape %s, crop %s' % (tuple(u8.shape), crop_hw))
    dst = torch.empty((B, F) + out_hw + (C,), dtype=torch.uint8, device=u8.device)
    crop = torch.empty((B, F) + crop_hw + (C,), dtype=torch.uint8, device=u8.device) if want_crop else None
    with torch.cuda.device(u8.device):
        _lib.check(_lib.lib().rvsr_bicubic_u8(_p(u8), _p(dst), _p(crop), _p(geom), B, F, C, Hw, Ww, frame_hw[0], frame_hw[1], crop_hw[0],
                                              crop_hw[1], scale, mode, _stream()), 'bicubic_u8')
    return (dst, crop) if want_crop else dst


# ---------------------------------------------------------------------------------------------------------------- datasets
def _read_png_u8(path):
    """A file as cv2.imread(path, IMREAD_UNCHANGED) holds it for 8-bit grey / colour images: uint8 [H, W] or [H, W, 3] in B, G, R
    order -- read through PIL (R, G, B), reversed as a view; the copy happens once, on the crop."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ('L', 'RGB'):
            im = im.convert('RGB')
        a = np.asarray(im)
    return a if a.ndim == 2 else a[:, :, ::-1]


class _RealVSRBase(torch.utils.data.Dataset):
    """What the two classes share.  Option keys as in the reference: interval_list, random_reverse, N_frames, dataroot_GT, dataroot_LQ,
    data_type ('img' | 'lmdb'), GT_size, LQ_size, cache_keys, border_mode, phase, use_flip, use_rot, scale, color; one key of
    its own, frame_chw, replaces the (3, 1024, 512) the reference hard-codes for the crop range (data sets of another frame size).

    A sample is {'LQs': uint8 [N, S, S, C], 'GT': uint8 [N | 1, S, S, C], 'flags': int, 'key': str} in cv2's byte order (whole frames
    and flags 0 outside phase 'train'); torch's default collate stacks them, and VideoSRModel.feed_data takes the collated batch as it
    is.  Only integers are touched here: no float conversion, no flip, no transposition -- those are the device's (assemble_batch).

    Worker processes never load the HIP library or touch the device.  Keep it that way in subclasses: the shared MI355X machines cap
    the number of processes that have the GPU open at 16, and a DataLoader's workers count against nothing as long as they stay on the CPU."""
    ALL_PAIR = False

    def __init__(self, opt):
        super(_RealVSRBase, self).__init__()
        self.opt = opt
        _refuse_lr_input(opt)
        self.GT_root, self.LQ_root = opt['dataroot_GT'], opt['dataroot_LQ']
        self.data_type = opt['data_type']
        _refuse_color_conversion(opt)
        if self.data_type == 'lmdb':
            import lmdb  # noqa: F401  (ImportError if the module is not installed)
            with open(os.path.join(opt['dataroot_GT'], 'meta_info.pkl'), 'rb') as f:
                self.paths_GT = pickle.load(f)['keys']
        elif self.data_type == 'img':
            if not opt.get('cache_keys'):
                raise ValueError('Need to create cache keys (meta_info.pkl) by running [create_lmdb.py]')
            with open(opt['cache_keys'], 'rb') as f:
                self.paths_GT = pickle.load(f)['keys']
        else:
            raise ValueError('Wrong data type: {}'.format(self.data_type))
        self.paths_GT = self._remove_test_sequences(self.paths_GT)
        assert self.paths_GT, 'Error: GT path is empty.'
        self.GT_env = self.LQ_env = None

    def _read(self, which, name_a, frame):
        """One whole frame, uint8, in cv2's byte order."""
        if self.data_type == 'lmdb':
            if self.GT_env is None:
                import lmdb
                self.GT_env = lmdb.open(self.opt['dataroot_GT'], readonly=True, lock=False, readahead=False, meminit=False)
                self.LQ_env = lmdb.open(self.opt['dataroot_LQ'], readonly=True, lock=False, readahead=False, meminit=False)
            with (self.GT_env if which == 'GT' else self.LQ_env).begin(write=False) as txn:
                buf = txn.get('{}_{}'.format(name_a, frame).encode('ascii'))
            C, H, W = FRAME_CHW
            return np.frombuffer(buf, dtype=np.uint8).reshape(H, W, C)
        return _read_png_u8(os.path.join(self.GT_root if which == 'GT' else self.LQ_root, name_a, frame + '.png'))

    def __getitem__(self, index):
        key = self.paths_GT[index]
        plan = draw_sample(self.opt, key, frame_chw=self.opt.get('frame_chw') or FRAME_CHW)
        names = ['{:05d}'.format(v) for v in plan['neighbor_list']]
        gt_names = names if self.ALL_PAIR else [plan['center']]
        # (np.stack copies the crops -- 3 S^2 bytes each -- which also drops the reversed-channel view of _read_png_u8)
        gt = np.stack([crop_u8(self._read('GT', plan['name_a'], n), plan) for n in gt_names], axis=0)
        lq = np.stack([crop_u8(self._read('LQ', plan['name_a'], n), plan) for n in names], axis=0)
        return {'LQs': torch.from_numpy(lq), 'GT': torch.from_numpy(gt), 'flags': plan['flags'], 'key': key}

    def __len__(self):
        return len(self.paths_GT)


class RealVSRDataset(_RealVSRBase):
    """RealVSRDataset of codes/data/RealVSR_dataset.py:15-177: N LQ frames and the GT of the centre frame; the fifty test sequences the
    reference hard-codes (:51-58) are left out."""
    TEST_SEQUENCES = ('008', '026', '029', '031', '042', '055', '058', '077', '105', '113', '132', '135', '146', '155', '161', '167', '173',
                      '175', '180', '181', '189', '194', '195', '226', '232', '237', '241', '242', '247', '256', '268', '275', '293', '309',
                      '358', '371', '372', '379', '383', '401', '409', '413', '426', '438', '448', '471', '478', '484', '490', '498')

    def _remove_test_sequences(self, keys):
        return [v for v in keys if v.split('_')[0] not in self.TEST_SEQUENCES]


class RealVSRAllPairDataset(_RealVSRBase):
    """RealVSRAllPairDataset of codes/data/RealVSR_dataset.py:180-346: N LQ frames and the N GT frames of the same window;
    opt['remove_list'] names a pickle of sequences to leave out (:216-221)."""
    ALL_PAIR = True

    def _remove_test_sequences(self, keys):
        if self.opt.get('remove_list'):
            with open(self.opt['remove_list'], 'rb') as f:
                remove = pickle.load(f)
            return [v for v in keys if v.split('_')[0] not in remove]
        return keys


def vimeo_frame_list(n_frames):
    """Vimeo90K_dataset.py:53-56: N = 1 -> [4], 3 -> [3, 4, 5], 5 -> [2 .. 6], 7 -> [1 .. 7]."""
    return [i + (9 - n_frames) // 2 for i in range(n_frames)]


def draw_vimeo_sample(opt, key, frame_list, rng=random, frame_chw=VIMEO_FRAME_CHW):
    """The random choices of one Vimeo90kDataset / Vimeo90kAllPairDataset sample, drawn from `rng` in the order of the reference's
    __getitem__ (Vimeo90K_dataset.py:80-134, 206-262; both classes draw alike):
      1. random_reverse and random() < 0.5: frame_list.reverse() -- IN PLACE, on the list the data set keeps (:91-92, :217-218): the
         reversal persists into the following samples.  An oddity, but it decides which frames a seed yields.
      2. phase 'train': randint for the crop's row, then its column -- of the LQ frame.  With LR_input (GT_size != LQ_size) that is the
         frame shrunk by opt['scale'] and a crop of GT_size // scale (:114-121); the GT crop sits at scale times the origin.
      3. util.augment's three short-circuited draws (util.py:263-265).
    interval_list and border_mode are read by nobody (the reference's classes only log them).  Returns a dict: name_a, name_b,
    frame_list (a copy, after the reversal), rnd_h, rnd_w, size (the GT crop; None outside phase 'train'), lq_h, lq_w, lq_size (the LQ
    crop), scale (of LR_input, else 1), flags, key."""
    name_a, name_b = key.split('_')
    if opt['random_reverse'] and rng.random() < 0.5:
        frame_list.reverse()
    lr_input = opt['GT_size'] != opt['LQ_size']
    scale = opt['scale'] if lr_input else 1
    plan = {'key': key, 'name_a': name_a, 'name_b': name_b, 'frame_list': list(frame_list), 'rnd_h': None, 'rnd_w': None, 'size': None,
            'lq_h': None, 'lq_w': None, 'lq_size': None, 'scale': scale, 'flags': 0}
    if opt['phase'] == 'train':
        _, H, W = frame_chw
        GT_size = opt['GT_size']
        lq_size = GT_size // scale
        lq_h = rng.randint(0, max(0, H // scale - lq_size))
        lq_w = rng.randint(0, max(0, W // scale - lq_size))
        flags = 0
        if opt['use_flip'] and rng.random() < 0.5:
            flags |= FLAG_HFLIP
        if opt['use_rot'] and rng.random() < 0.5:
            flags |= FLAG_VFLIP
        if opt['use_rot'] and rng.random() < 0.5:
            flags |= FLAG_ROT90
        plan.update(rnd_h=int(lq_h * scale), rnd_w=int(lq_w * scale), size=GT_size, lq_h=lq_h, lq_w=lq_w, lq_size=lq_size, flags=flags)
    return plan


class _Vimeo90kBase(torch.utils.data.Dataset):
    """What the two Vimeo-90K classes share.  Option keys as in the reference: interval_list, random_reverse, N_frames, dataroot_GT,
    dataroot_LQ, data_type ('img' | 'lmdb'), GT_size, LQ_size, cache_keys, phase, use_flip, use_rot, scale; two keys of this project's
    own: frame_chw replaces the (3, 256, 448) the reference hard-codes, and synthesize_LQ (below).  Files are
    <root>/<name_a>/<name_b>/im<v>.png, lmdb keys <key>_<v>.

    A sample is {'LQs': uint8 [N, s, s, C], 'GT': uint8 [N | 1, S, S, C], 'flags': int, 'key': str} in cv2's byte order, s = S unless
    LR_input (GT_size != LQ_size: s = S // scale, the LQ files are the shrunk frames); VideoSRModel.feed_data takes the collated batch.

    synthesize_LQ: true -- dataroot_LQ is not read.  The LQ frames are MATLAB's bicubic chain of the GT frames, computed on the device
    (bicubic_u8): with GT_size == LQ_size shrink-and-enlarge ('same') at opt['scale_synth'] (default 2: the shipped option files'
    vimeo_septuplet_BIx2_same), otherwise 'down' at opt['scale'].  The sample carries, in place of 'LQs' and 'GT',
        'GT_window'  uint8 [N, Hw, Ww, C]: the window of every frame of frame_list (crop + 2 halo per edge, or the whole frame where
                     that is smaller; degrade_window_plan),  'geom' int32 [4]: (wy, wx, y0, x0),
        'synth_scale', 'synth_mode', 'frame_h', 'frame_w', 'crop_size': ints,  'gt_index': the frame whose crop is the GT (the centre
                     frame for Vimeo90kDataset), -1 = all of them (Vimeo90kAllPairDataset)
    and feed_packed computes both tensors from it.  Outside phase 'train' the window is the whole frame.

    Worker processes never load the HIP library or touch the device (see _RealVSRBase): the halo comes from BIC_HALO, not from the library."""
    ALL_PAIR = False

    def __init__(self, opt):
        super(_Vimeo90kBase, self).__init__()
        self.opt = opt
        self.GT_root, self.LQ_root = opt['dataroot_GT'], opt.get('dataroot_LQ')
        self.data_type = opt['data_type']
        self.LR_input = opt['GT_size'] != opt['LQ_size']
        self.synthesize = bool(opt.get('synthesize_LQ'))
        self.frame_chw = tuple(opt.get('frame_chw') or VIMEO_FRAME_CHW)
        self.frame_list = vimeo_frame_list(opt['N_frames'])
        self.center = opt['N_frames'] // 2
        if self.data_type == 'lmdb':
            import lmdb  # noqa: F401  (ImportError if the module is not installed)
            with open(os.path.join(opt['dataroot_GT'], 'meta_info.pkl'), 'rb') as f:
                self.paths_GT = pickle.load(f)['keys']
        elif opt.get('cache_keys'):
            with open(opt['cache_keys'], 'rb') as f:
                self.paths_GT = self._keys_of(pickle.load(f))
        else:
            raise ValueError('Need to create cache keys (meta_info.pkl) by running [create_lmdb.py]')
        assert self.paths_GT, 'Error: GT path is empty.'
        if self.data_type not in ('lmdb', 'img'):
            raise ValueError('Wrong data type: {}'.format(self.data_type))
        if self.synthesize:
            self.synth_scale = int(opt['scale'] if self.LR_input else opt.get('scale_synth') or 2)
            self.synth_mode = RVSR_BIC_DOWN if self.LR_input else RVSR_BIC_SAME
            bicubic_halo(self.synth_scale, self.synth_mode)
            _check_bicubic_frame(self.frame_chw[1:], self.synth_scale)
            if self.LR_input and opt['GT_size'] % self.synth_scale:
                raise ValueError('synthesize_LQ: GT_size %d is no multiple of the scale %d' % (opt['GT_size'], self.synth_scale))
        self.GT_env = self.LQ_env = None

    def _read(self, which, plan, v):
        """One whole frame, uint8, in cv2's byte order."""
        if self.data_type == 'lmdb':
            if self.GT_env is None:
                import lmdb
                self.GT_env = lmdb.open(self.opt['dataroot_GT'], readonly=True, lock=False, readahead=False, meminit=False)
                if not self.synthesize:
                    self.LQ_env = lmdb.open(self.opt['dataroot_LQ'], readonly=True, lock=False, readahead=False, meminit=False)
            with (self.GT_env if which == 'GT' else self.LQ_env).begin(write=False) as txn:
                buf = txn.get('{}_{}'.format(plan['key'], v).encode('ascii'))
            C, H, W = self.frame_chw
            s = plan['scale'] if which == 'LQ' else 1
            return np.frombuffer(buf, dtype=np.uint8).reshape(H // s, W // s, C)
        return _read_png_u8(os.path.join(self.GT_root if which == 'GT' else self.LQ_root, plan['name_a'], plan['name_b'],
                                         'im{}.png'.format(v)))

    def __getitem__(self, index):
        key = self.paths_GT[index]
        plan = draw_vimeo_sample(self.opt, key, self.frame_list, frame_chw=self.frame_chw)
        gt_frames = plan['frame_list'] if self.ALL_PAIR or self.synthesize else [4]   # (:99: im4, whatever N_frames)
        if self.synthesize:
            frame_hw = self.frame_chw[1:]
            (wy, wx), (Hw, Ww), geom = degrade_window_plan(plan, frame_hw, self.synth_scale, self.synth_mode)
            frames = []
            for v in gt_frames:
                f = self._read('GT', plan, v)
                if f.shape[:2] != tuple(frame_hw):
                    raise ValueError('%s frame %s is %d x %d, frame_chw says %d x %d' % ((key, v) + f.shape[:2] + tuple(frame_hw)))
                f = f[:, :, None] if f.ndim == 2 else f[:, :, :3]
                frames.append(f[wy:wy + Hw, wx:wx + Ww])
            return {'GT_window': torch.from_numpy(np.stack(frames, axis=0)), 'geom': torch.tensor(geom, dtype=torch.int32),
                    'flags': plan['flags'], 'key': key, 'synth_scale': self.synth_scale, 'synth_mode': self.synth_mode,
                    'frame_h': frame_hw[0], 'frame_w': frame_hw[1], 'crop_size': plan['size'] if plan['size'] is not None else 0,
                    'gt_index': -1 if self.ALL_PAIR else plan['frame_list'].index(4)}
        lq_plan = {'rnd_h': plan['lq_h'], 'rnd_w': plan['lq_w'], 'size': plan['lq_size']}
        gt = np.stack([crop_u8(self._read('GT', plan, v), plan) for v in gt_frames], axis=0)
        lq = np.stack([crop_u8(self._read('LQ', plan, v), lq_plan) for v in plan['frame_list']], axis=0)
        return {'LQs': torch.from_numpy(lq), 'GT': torch.from_numpy(gt), 'flags': plan['flags'], 'key': key}

    def __len__(self):
        return len(self.paths_GT)


class Vimeo90kDataset(_Vimeo90kBase):
    """Vimeo90kDataset of codes/data/Vimeo90K_dataset.py:24-147: N LQ frames and the GT of im4; cache_keys is a pickle {'keys': [...]} (:63)."""

    @staticmethod
    def _keys_of(pickled):
        return pickled['keys']


class Vimeo90kAllPairDataset(_Vimeo90kBase):
    """Vimeo90kAllPairDataset of codes/data/Vimeo90K_dataset.py:150-276: N LQ frames and the N GT frames of the same list; cache_keys is a
    pickle of the key list itself (:189)."""
    ALL_PAIR = True

    @staticmethod
    def _keys_of(pickled):
        return pickled


# ---------------------------------------------------------------------------------------------------------------- validation clips
def index_generation(crt_i, max_n, N, padding='reflection'):
    """Indices of the N frames centred on `crt_i` in a sequence of `max_n` frames (counted from 1).

    padding: replicate | reflection | new_info | circle; e.g. crt_i = 0, N = 5:
    [0, 0, 0, 1, 2] | [2, 1, 0, 1, 2] | [4, 3, 0, 1, 2] | [3, 4, 0, 1, 2]   (codes/data/util.py:169-214)."""
    last = max_n - 1
    half = N // 2
    if padding not in ('replicate', 'reflection', 'new_info', 'circle'):
        raise ValueError('Wrong padding mode')
    idx = []
    for i in range(crt_i - half, crt_i + half + 1):
        if i < 0:
            j = {'replicate': 0, 'reflection': -i, 'new_info': crt_i + half - i, 'circle': N + i}[padding]
        elif i > last:
            j = {'replicate': last, 'reflection': 2 * last - i, 'new_info': crt_i - half - (i - last),
                 'circle': i - N}[padding]
        else:
            j = i
        idx.append(j)
    return idx




class VideoTestDataset(torch.utils.data.Dataset):
    """VideoTestDataset of codes/data/VideoTestDataset.py (the 'VideoTest' mode of every shipped option file's `val` section): the
    sub-folders of dataroot_LQ / dataroot_GT are clips, every frame of every clip is one sample.  Option keys as in the reference: name
    (vid4 | reds4 | realvsr_test, any case), cache_data, N_frames, padding, dataroot_GT, dataroot_LQ, data_type, color.  'lmdb' is
    refused as there; cache_data has to be true (the reference's other branch is an empty TODO and fails on an unbound name).

    data_info is the reference's: path_LQ, path_GT, folder, idx ('i/max'), border (1 for the N_frames // 2 frames at either end).
    The cache holds every clip ONCE as uint8 [T, H, W, C] in cv2's byte order -- a quarter of the reference's f32 cache -- and a sample
    is {'LQs': uint8 [N, H, W, C] (the window of index_generation), 'GT': uint8 [1, H, W, C], 'folder', 'idx', 'border'}: the batch a
    DataLoader makes of it goes through the models' feed_data as it is (whole frames, no flags).  clip(folder) hands out a whole cached
    clip for the clip-wise validation pass of realvsr_amd.train.  Like the other data sets it never touches the device."""
    NAMES = ('vid4', 'reds4', 'realvsr_test')

    def __init__(self, opt):
        super(VideoTestDataset, self).__init__()
        self.opt = opt
        self.cache_data = opt['cache_data']
        self.half_N_frames = opt['N_frames'] // 2
        self.GT_root, self.LQ_root = opt['dataroot_GT'], opt['dataroot_LQ']
        self.data_type = opt['data_type']
        self.data_info = {'path_LQ': [], 'path_GT': [], 'folder': [], 'idx': [], 'border': []}
        if self.data_type == 'lmdb':
            raise ValueError('No need to use LMDB during validation/test.')
        if opt['name'].lower() not in self.NAMES:
            raise ValueError('Not support video test dataset [%s]. Support %s.' % (opt['name'], ', '.join(self.NAMES)))
        if not self.cache_data:
            raise NotImplementedError('VideoTestDataset: cache_data has to be true (reading per sample is not built)')
        _refuse_color_conversion(opt)
        index_generation(0, 1, opt['N_frames'], opt['padding'])   # (an unknown padding mode fails here, not in a worker)
        self.imgs_LQ, self.imgs_GT = {}, {}
        for sub_LQ, sub_GT in zip(self._listing(self.LQ_root), self._listing(self.GT_root)):
            folder = os.path.basename(sub_GT)
            paths_LQ, paths_GT = self._listing(sub_LQ), self._listing(sub_GT)
            max_idx = len(paths_LQ)
            assert max_idx == len(paths_GT), 'Different number of images in LQ and GT folders'
            self.data_info['path_LQ'].extend(paths_LQ)
            self.data_info['path_GT'].extend(paths_GT)
            self.data_info['folder'].extend([folder] * max_idx)
            self.data_info['idx'].extend('{}/{}'.format(i, max_idx) for i in range(max_idx))
            self.data_info['border'].extend(int(i < self.half_N_frames or i >= max_idx - self.half_N_frames) for i in range(max_idx))
            self.imgs_LQ[folder] = self._read_clip(paths_LQ)
            self.imgs_GT[folder] = self._read_clip(paths_GT)

    @staticmethod
    def _listing(root):
        """sorted(glob(root/*)): the entries in name order, hidden ones left out."""
        return [os.path.join(root, v) for v in sorted(os.listdir(root)) if not v.startswith('.')]

    @staticmethod
    def _read_clip(paths):
        frames = [_read_png_u8(p) for p in paths]
        frames = [f[:, :, None] if f.ndim == 2 else f[:, :, :3] for f in frames]
        return torch.from_numpy(np.stack(frames, axis=0))    # (the copy drops the reversed-channel view of _read_png_u8)

    def clip(self, folder):
        """(LQ uint8 [T, H, W, C], GT uint8 [T, H', W', C]) of one clip: the cached tensors themselves, not copies."""
        return self.imgs_LQ[folder], self.imgs_GT[folder]

    def folders(self):
        """The clips in the order their samples come."""
        return list(self.imgs_GT)

    def __getitem__(self, index):
        folder = self.data_info['folder'][index]
        idx, max_idx = (int(v) for v in self.data_info['idx'][index].split('/'))
        select_idx = index_generation(idx, max_idx, self.opt['N_frames'], padding=self.opt['padding'])
        return {'LQs': self.imgs_LQ[folder].index_select(0, torch.tensor(select_idx, dtype=torch.long)),
                'GT': self.imgs_GT[folder][idx:idx + 1], 'folder': folder, 'idx': self.data_info['idx'][index],
                'border': self.data_info['border'][index]}

    def __len__(self):
        return len(self.data_info['path_GT'])


MAX_WORKERS = 16   # a command gets 16 CPUs whatever the machine has; never sized by os.cpu_count()


def create_dataset(dataset_opt):
    """create_dataset of codes/data/__init__.py:28-49: the data set class that dataset_opt['mode'] names."""
    import logging
    modes = {'VideoTest': VideoTestDataset, 'Vimeo90k': Vimeo90kDataset, 'Vimeo90k_AllPair': Vimeo90kAllPairDataset,
             'RealVSR': RealVSRDataset, 'RealVSR_AllPair': RealVSRAllPairDataset}
    mode = dataset_opt['mode']
    if mode not in modes:
        raise NotImplementedError('Dataset [{:s}] is not recognized.'.format(str(mode)))
    dataset = modes[mode](dataset_opt)
    logging.getLogger('base').info('Dataset [{:s} - {:s}] is created.'.format(dataset.__class__.__name__, dataset_opt['name']))
    return dataset


def create_dataloader(dataset, dataset_opt, opt=None, sampler=None):
    """create_dataloader of codes/data/__init__.py:7-25.  Phase 'train': with opt['dist'] every rank loads batch_size // world samples
    with n_workers workers and the sampler's order, otherwise batch_size samples, shuffled, with n_workers per entry of gpu_ids;
    incomplete batches are dropped.  Any other phase: one sample at a time, in order, one worker.  At most MAX_WORKERS workers."""
    if dataset_opt['phase'] == 'train':
        if opt['dist']:
            world_size = torch.distributed.get_world_size()
            num_workers = dataset_opt['n_workers']
            assert dataset_opt['batch_size'] % world_size == 0
            batch_size = dataset_opt['batch_size'] // world_size
            shuffle = False
        else:
            num_workers = dataset_opt['n_workers'] * len(opt['gpu_ids'])
            batch_size = dataset_opt['batch_size']
            shuffle = True
        return torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=min(num_workers, MAX_WORKERS),
                                           sampler=sampler, drop_last=True, pin_memory=False)
    return torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False, num_workers=1, pin_memory=True)


class DistIterSampler(torch.utils.data.Sampler):
    """DistIterSampler of codes/data/data_sampler.py: a distributed sampler whose "epoch" is the data set `ratio` times over, so that
    the loader's workers restart `ratio` times less often.  Every rank draws the same randperm(total_size) from a generator seeded by
    the epoch (set_epoch), takes it modulo the data-set length and keeps every num_replicas-th entry from its own rank on;
    total_size = num_replicas * ceil(len(dataset) * ratio / num_replicas)."""

    def __init__(self, dataset, num_replicas=None, rank=None, ratio=100):
        if num_replicas is None:
            num_replicas = torch.distributed.get_world_size()
        if rank is None:
            rank = torch.distributed.get_rank()
        self.dataset, self.num_replicas, self.rank, self.epoch = dataset, num_replicas, rank, 0
        self.num_samples = -(-len(dataset) * ratio // num_replicas)
        self.total_size = self.num_samples * num_replicas

    def __iter__(self):
        g = torch.Generator()
        g.manual_seed(self.epoch)
        perm = torch.randperm(self.total_size, generator=g)
        return iter((perm[self.rank::self.num_replicas] % len(self.dataset)).tolist())

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch
