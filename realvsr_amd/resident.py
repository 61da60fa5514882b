"""The RealVSR training set resident in HBM: every frame decoded once, batches gathered from the store on the device.

The file loader of realvsr_amd.data decodes 2 * N whole 1024 x 512 PNG files per sample to cut an S x S crop out of each; at the shipped
batch of 32 x 3 frames, all-pair, that is 192 decodes per step, and the decode -- not the step -- sets the pace.  The training split is
450 sequences x 50 frames x 1.5 MiB = 35.4 GB per side, a quarter of an MI355X's HBM for LQ and GT together.  So:

  start-up (DeviceFrameStore.from_dataset)   every frame of every sequence of dataset.paths_GT, read through dataset._read in CPU-only
                                             DataLoader workers, uploaded in chunks through pinned memory into ONE uint8 tensor
                                             [n, H, W, C] per side, with a map (sequence, frame number) -> slot
  per batch, host (ResidentLoader)           the plans of data.draw_sample in the file loader's order; build_table turns them into
                                             int32 [B, frames + 3]: store slots, crop row, crop column, flags -- a few hundred bytes
  per batch, device (gather_batch)           rvsr_gather_clips (include/realvsr_hip.h section 12b; csrc/batch_kernels.hip): the tile body
                                             of rvsr_assemble_clips reading the crop where it sits in its frame; one launch per side

A ResidentLoader yields the f32 batch the models' feed_data takes through its float branch, equal bit for bit to what the file loader's
packed batch becomes in feed_packed, and consumes `random` and torch's generator exactly as create_dataloader does with n_workers 0: a
run with `resident: true` in its train data set (realvsr_amd.train) is the same run.

Not built: the Vimeo-90K classes (the GT alone is 155 GB, and bicubic_u8 wants windows), validation sets (VideoTestDataset caches its
clips already), a packed on-disk cache of the decoded frames, sharding the store across ranks (every rank holds the whole store).
"""
import logging
import os
import time

import numpy as np
import torch

from . import data
from .data import FRAME_CHW, LAST_FRAME, MAX_WORKERS, RVSR_ASM_REVERSE

RESIDENT_MAX_GB = 128   # default budget of one run's stores, under half of the 288 GB of HBM (the full split needs 70.8 GB)
UPLOAD_CHUNK = 16       # frames per pinned upload buffer (two buffers: 48 MiB at 1024 x 512 x 3)


def _as_hwc(frame):
    """One decoded frame as uint8 [H, W, C], C = 1 or 3 (a fourth channel is dropped: util.py:98-100)."""
    if frame.dtype != np.uint8:
        raise ValueError('frames are uint8, got %s' % frame.dtype)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    if frame.ndim != 3:
        raise ValueError('a frame is [H, W] or [H, W, C], got %s' % (frame.shape,))
    return frame[:, :, :3]


def _check_budget(nbytes, resident_max_gb, what):
    limit = RESIDENT_MAX_GB if resident_max_gb is None else resident_max_gb
    if nbytes > limit * 1e9:
        raise RuntimeError('%s: %.6g GB of frames exceed resident_max_gb = %g GB' % (what, nbytes / 1e9, limit))


class _FrameReader(torch.utils.data.Dataset):
    """Item i: frame `items[i]` = (sequence, frame number) of one side, as a contiguous uint8 tensor [H, W, C].  Runs in DataLoader
    workers: integers only, the HIP library is never loaded (see data._RealVSRBase)."""

    def __init__(self, dataset, which, items):
        self.dataset, self.which, self.items = dataset, which, items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        name, number = self.items[i]
        return torch.from_numpy(np.array(_as_hwc(self.dataset._read(self.which, name, '{:05d}'.format(number)))))   # (a writable copy)


def dataset_frames(dataset):
    """Every (sequence, frame number) a sample of `dataset` can read, sequences in the order dataset.paths_GT first names them: for
    'img' the <00000>.png files of the sequence's GT folder, for 'lmdb' frames 0 .. 49 (the clip length the reference hard-codes)."""
    names = list(dict.fromkeys(key.split('_')[0] for key in dataset.paths_GT))
    items = []
    for name in names:
        if dataset.data_type == 'lmdb':
            numbers = range(LAST_FRAME + 1)
        else:
            stems = (os.path.splitext(v) for v in os.listdir(os.path.join(dataset.GT_root, name)))
            numbers = sorted(int(stem) for stem, ext in stems if ext == '.png' and stem.isdigit())
        items.extend((name, int(v)) for v in numbers)
    return items


class DeviceFrameStore(object):
    """One side (LQ or GT) of a data set as ONE contiguous uint8 tensor [n, H, W, C] in cv2's byte order, and `index`, the map
    (sequence name, frame number) -> slot.  On the GPU it is what gather_batch reads; device='cpu' keeps it in pageable host memory
    for host tests and tools (build_table needs only the map and the shape)."""

    def __init__(self, frames, index, load_seconds=0.0):
        if frames.dtype != torch.uint8 or frames.dim() != 4 or not frames.is_contiguous():
            raise ValueError('a store is a contiguous uint8 [n, H, W, C] tensor, got %s %s' % (frames.dtype, tuple(frames.shape)))
        if len(index) != frames.shape[0] or sorted(index.values()) != list(range(frames.shape[0])):
            raise ValueError('the index has to name every slot of the store once')
        self.frames, self.index, self.load_seconds = frames, dict(index), load_seconds

    def __len__(self):
        return self.frames.shape[0]

    @property
    def frame_hwc(self):
        return tuple(self.frames.shape[1:])

    @property
    def nbytes(self):
        return self.frames.numel()

    @classmethod
    def _fill(cls, keys, batches, hw, device, resident_max_gb, what):
        """`batches`: an iterable of lists of uint8 [H, W, C] CPU tensors, len(keys) frames in all, in the order of `keys`; hw: the
        (H, W) every frame has to have, or None = that of the first frame.  The channel count is the first frame's."""
        t0 = time.perf_counter()
        device = torch.device(device)
        keys = [(str(name), int(number)) for name, number in keys]
        index = {key: slot for slot, key in enumerate(keys)}
        if len(index) != len(keys):
            raise ValueError('%s: a (sequence, frame) pair is named twice' % what)
        if not keys:
            raise ValueError('%s: no frames' % what)
        shape, store, pinned, done, slot, n = None, None, None, [None, None], 0, 0
        for batch in batches:
            if n + len(batch) > len(keys):
                raise ValueError('%s: more frames than keys' % what)
            for k, frame in enumerate(batch):
                if shape is None:
                    shape = (tuple(int(v) for v in hw) if hw is not None else tuple(frame.shape[:2])) + (int(frame.shape[2]),)
                    _check_budget(len(keys) * int(np.prod(shape)), resident_max_gb, what)   # (before a byte is allocated)
                if tuple(frame.shape[:2]) != shape[:2]:
                    raise ValueError('%s: frame %d of sequence %s is %d x %d, expected %d x %d'
                                     % ((what, keys[n + k][1], keys[n + k][0]) + tuple(frame.shape[:2]) + shape[:2]))
                if frame.shape[2] != shape[2]:
                    raise ValueError('%s: frame %d of sequence %s has %d channels, the frames before it %d'
                                     % (what, keys[n + k][1], keys[n + k][0], frame.shape[2], shape[2]))
            if store is None:
                store = torch.empty((len(keys),) + shape, dtype=torch.uint8, device=device)
            if device.type == 'cpu':
                for k, frame in enumerate(batch):
                    store[n + k] = frame
            else:
                if pinned is None:
                    pinned = [torch.empty((UPLOAD_CHUNK,) + shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
                for a in range(0, len(batch), UPLOAD_CHUNK):
                    part = batch[a:a + UPLOAD_CHUNK]
                    if done[slot] is not None:
                        done[slot].synchronize()   # (the copy issued from this buffer two chunks ago)
                    for k, frame in enumerate(part):
                        pinned[slot][k] = frame
                    store[n + a:n + a + len(part)].copy_(pinned[slot][:len(part)], non_blocking=True)
                    done[slot] = torch.cuda.Event()
                    done[slot].record()
                    slot ^= 1
            n += len(batch)
        if n != len(keys):
            raise ValueError('%s: %d frames for %d keys' % (what, n, len(keys)))
        if device.type != 'cpu':
            torch.cuda.synchronize(device)
        return cls(store, index, time.perf_counter() - t0)

    @classmethod
    def from_frames(cls, frames, keys, frame_chw=None, device='cuda', resident_max_gb=None):
        """A store of the numpy uint8 frames `frames` ([H, W] or [H, W, C] each, any iterable), frame i under keys[i] = (sequence name,
        frame number).  frame_chw (C, H, W): the H x W every frame has to have (None: that of the first).  ValueError for a frame of
        another size or a mixed channel count, RuntimeError for more than resident_max_gb."""
        batches = ([torch.from_numpy(np.array(_as_hwc(np.asarray(f))))] for f in frames)
        hw = None if frame_chw is None else (frame_chw[1], frame_chw[2])
        return cls._fill(list(keys), batches, hw, device, resident_max_gb, 'DeviceFrameStore.from_frames')

    @classmethod
    def from_dataset(cls, dataset, which, device='cuda', n_workers=0, resident_max_gb=None):
        """Every frame of every sequence of dataset.paths_GT (dataset_frames), side `which` ('LQ' | 'GT'), read once through
        dataset._read -- 'img' and 'lmdb' alike -- in at most min(n_workers, MAX_WORKERS) CPU-only DataLoader workers (0: in this
        process).  The size is opt['frame_chw'] or the reference's (3, 1024, 512); the budget is checked before a file is read.
        Neither `random` nor torch's default generator is touched (the DataLoader gets a generator of its own)."""
        if which not in ('LQ', 'GT'):
            raise ValueError("which is 'LQ' or 'GT', got %r" % (which,))
        items = dataset_frames(dataset)
        C, H, W = (int(v) for v in (dataset.opt.get('frame_chw') or FRAME_CHW))
        what = 'DeviceFrameStore.from_dataset(%s)' % which
        _check_budget(len(items) * H * W * C, resident_max_gb, what)
        loader = torch.utils.data.DataLoader(_FrameReader(dataset, which, items), batch_size=UPLOAD_CHUNK, shuffle=False,
                                             num_workers=min(max(int(n_workers or 0), 0), MAX_WORKERS), collate_fn=list, drop_last=False,
                                             pin_memory=False, generator=torch.Generator())
        return cls._fill(items, loader, (H, W), device, resident_max_gb, what)


def build_table(plans, store, single=None):
    """Host integers only: the data.draw_sample plans of one batch -> the int32 table [B, frames + 3] of rvsr_gather_clips for `store`
    (a CPU tensor): per sample the slots of plan['neighbor_list'] -- with `single` ONE column, the slot of plan['center'], the GT of
    RealVSRDataset -- then rnd_h, rnd_w, flags.  ValueError for a sequence or frame the store does not hold, for plans without a crop
    (outside phase 'train') or of differing shape, and for a crop that leaves the frame, as data.crop_u8 raises."""
    H, W, _ = store.frame_hwc
    rows = []
    for plan in plans:
        numbers = [int(plan['center'])] if single else [int(v) for v in plan['neighbor_list']]
        if plan['rnd_h'] is None:
            raise ValueError('a resident batch is made of crops: the plan of %s has none (phase other than train)' % (plan['key'],))
        h, w, S = int(plan['rnd_h']), int(plan['rnd_w']), int(plan['size'])
        if h < 0 or w < 0 or h + S > H or w + S > W:
            raise ValueError('the %d x %d crop at (%d, %d) leaves the %d x %d frame' % (S, S, h, w, H, W))
        slots = []
        for v in numbers:
            slot = store.index.get((plan['name_a'], v))
            if slot is None:
                raise ValueError('the store holds no frame %d of sequence %r' % (v, plan['name_a']))
            slots.append(slot)
        rows.append(slots + [h, w, int(plan['flags'])])
        if len(rows[-1]) != len(rows[0]) or S != int(plans[0]['size']):
            raise ValueError('the plans of one batch differ in frames or crop size')
    if not rows:
        raise ValueError('no plans')
    return torch.tensor(rows, dtype=torch.int32)


def gather_batch(store, table_dev, frames, S, mode=RVSR_ASM_REVERSE, out=None):
    """int32 [B, frames + 3] on the GPU (build_table) -> float32 [B, frames, C, S, S] gathered from `store` (rvsr_gather_clips,
    include/realvsr_hip.h section 12b): assemble_batch of the crops, without the crops."""
    from . import _lib
    from ._lib import _p, _stream
    u8 = store.frames
    if not u8.is_cuda:
        raise RuntimeError('gather_batch runs on MI355X (HIP) tensors only')
    frames, S = int(frames), int(S)
    if (not torch.is_tensor(table_dev) or not table_dev.is_cuda or table_dev.device != u8.device or table_dev.dtype != torch.int32
            or not table_dev.is_contiguous() or table_dev.dim() != 2 or table_dev.shape[1] != frames + 3 or table_dev.shape[0] == 0):
        raise RuntimeError('gather_batch: the table has to be a contiguous int32 [B, %d] tensor on the device of the store' % (frames + 3))
    n, H, W, C = u8.shape
    B = table_dev.shape[0]
    if out is None:
        out = torch.empty(B, frames, C, S, S, dtype=torch.float32, device=u8.device)
    elif (not out.is_cuda or out.device != u8.device or out.dtype != torch.float32 or not out.is_contiguous()
          or tuple(out.shape) != (B, frames, C, S, S)):
        raise RuntimeError('gather_batch: out has to be a contiguous float32 %s tensor on the device of the store' % ((B, frames, C, S, S),))
    if out.numel() == 0:
        raise RuntimeError('gather_batch: empty shape %s' % (tuple(out.shape),))
    with torch.cuda.device(u8.device):
        _lib.check(_lib.lib().rvsr_gather_clips(_p(u8), n, H, W, _p(table_dev), _p(out), B, frames, C, S, int(mode), _stream()),
                   'gather_clips')
    return out


def gather_plan(out_ptr_or_tensor, B, F, C, S):
    """(variant, workgroups) of the gather_batch call that writes there: variant 1 = 16-byte stores, 0 = scalar stores."""
    import ctypes
    from . import _lib
    ptr = out_ptr_or_tensor.data_ptr() if torch.is_tensor(out_ptr_or_tensor) else int(out_ptr_or_tensor)
    variant, blocks = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib().rvsr_gather_plan(ctypes.c_void_p(ptr), B, F, C, S, ctypes.byref(variant), ctypes.byref(blocks)), 'gather_plan')
    return variant.value, blocks.value


class _PlanView(torch.utils.data.Dataset):
    """The data set as its plans: item i is data.draw_sample for key i -- the draws of the file data set's __getitem__, no file read."""

    def __init__(self, dataset):
        self.opt, self.keys = dataset.opt, dataset.paths_GT
        self.frame_chw = tuple(dataset.opt.get('frame_chw') or FRAME_CHW)

    def __len__(self):
        return len(self.keys)

    def __getitem__(self, i):
        return data.draw_sample(self.opt, self.keys[i], frame_chw=self.frame_chw)


class ResidentLoader(object):
    """The training loader of a RealVSRDataset / RealVSRAllPairDataset whose frames are resident (DeviceFrameStore).  Iterating it
    iterates a torch DataLoader (num_workers 0, collate_fn = list, drop_last) over the data set's plans, so the index order -- shuffle,
    or a sampler such as DistIterSampler -- and every draw from `random` and from torch's generator are those of
    data.create_dataloader with n_workers 0.  Per batch: one table upload (the LQ table and, for the single-GT class, the one-column GT
    table behind it), one gather on the LQ store, one on the GT store.  Yields
        {'LQs': f32 cuda [B, N, C, S, S], 'GT': f32 cuda [B, N, C, S, S] (all-pair) or [B, C, S, S], 'key': [B strings]}
    which the models' feed_data takes through its float branch.  lq_store / gt_store: stores built elsewhere (they have to name the
    same frames); None: DeviceFrameStore.from_dataset on the current device, in n_workers workers.  plans() is the host half alone."""

    def __init__(self, dataset, batch_size, shuffle=False, sampler=None, mode=RVSR_ASM_REVERSE, lq_store=None, gt_store=None,
                 n_workers=0, resident_max_gb=None):
        if not isinstance(dataset, data._RealVSRBase):
            raise NotImplementedError('resident: RealVSR / RealVSR_AllPair data sets only, got %s' % type(dataset).__name__)
        if dataset.opt['phase'] != 'train':
            raise NotImplementedError('resident: training sets only (validation clips are cached by VideoTestDataset)')
        self.dataset, self.mode, self.all_pair = dataset, int(mode), bool(dataset.ALL_PAIR)
        self.frames, self.size = int(dataset.opt['N_frames']), int(dataset.opt['GT_size'])
        if lq_store is None or gt_store is None:
            items = dataset_frames(dataset)
            C, H, W = (int(v) for v in (dataset.opt.get('frame_chw') or FRAME_CHW))
            missing = (lq_store is None) + (gt_store is None)
            held = sum(s.nbytes for s in (lq_store, gt_store) if s is not None)
            _check_budget(held + missing * len(items) * H * W * C, resident_max_gb, 'ResidentLoader')   # both sides count
            if lq_store is None:
                lq_store = DeviceFrameStore.from_dataset(dataset, 'LQ', n_workers=n_workers, resident_max_gb=resident_max_gb)
            if gt_store is None:
                gt_store = DeviceFrameStore.from_dataset(dataset, 'GT', n_workers=n_workers, resident_max_gb=resident_max_gb)
        if lq_store.index != gt_store.index:
            raise ValueError('the LQ and the GT store have to hold the same frames in the same slots')
        if lq_store.frames.device != gt_store.frames.device:
            raise ValueError('the LQ and the GT store have to be on one device')
        self.lq_store, self.gt_store = lq_store, gt_store
        self.loader = torch.utils.data.DataLoader(_PlanView(dataset), batch_size=batch_size, shuffle=shuffle, num_workers=0,
                                                  sampler=sampler, drop_last=True, pin_memory=False, collate_fn=list)

    def __len__(self):
        return len(self.loader)

    def plans(self):
        """The batches as lists of data.draw_sample plans (host only; one pass = one epoch of the loader)."""
        return iter(self.loader)

    def tables(self, plans):
        """(LQ table, GT table) of one batch, int32 CPU tensors; the all-pair class uses the same table for both stores."""
        lq = build_table(plans, self.lq_store)
        return lq, lq if self.all_pair else build_table(plans, self.gt_store, single=True)

    def __iter__(self):
        device = self.lq_store.frames.device
        for plans in self.loader:
            lq_t, gt_t = self.tables(plans)
            if self.all_pair:
                lq_d = gt_d = lq_t.to(device, non_blocking=True)
            else:   # (the two views share their storage: one copy)
                block = torch.cat([lq_t.reshape(-1), gt_t.reshape(-1)]).to(device, non_blocking=True)
                lq_d, gt_d = block[:lq_t.numel()].view(lq_t.shape), block[lq_t.numel():].view(gt_t.shape)
            var_L = gather_batch(self.lq_store, lq_d, self.frames, self.size, self.mode)
            var_H = gather_batch(self.gt_store, gt_d, gt_d.shape[1] - 3, self.size, self.mode)
            yield {'LQs': var_L, 'GT': var_H if self.all_pair else var_H[:, 0], 'key': [p['key'] for p in plans]}


def create_resident_loader(dataset, dataset_opt, opt=None, sampler=None, lq_store=None, gt_store=None):
    """data.create_dataloader for a train data set with `resident: true`: batch_size // world_size samples per rank in the sampler's
    order under opt['dist'], otherwise batch_size samples, shuffled; the stores (unless handed in) are read with the workers the file
    loader would have had.  dataset_opt['resident_max_gb'] replaces the default budget."""
    if dataset_opt['phase'] != 'train':
        raise NotImplementedError('resident: training sets only')
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
    loader = ResidentLoader(dataset, batch_size, shuffle=shuffle, sampler=sampler, lq_store=lq_store, gt_store=gt_store,
                            n_workers=min(num_workers, MAX_WORKERS), resident_max_gb=dataset_opt.get('resident_max_gb'))
    logger = logging.getLogger('base')
    for which, store in (('LQ', loader.lq_store), ('GT', loader.gt_store)):
        logger.info('Resident {:s} store: {:,d} frames of {:d} x {:d} x {:d}, {:,d} bytes, loaded in {:.1f} s'.format(
            which, len(store), *store.frame_hwc, store.nbytes, store.load_seconds))
    return loader
