"""rvsr_gather_clips (csrc/batch_kernels.hip) and the resident loader (realvsr_amd/resident.py) on the GPU, against the numpy
restatement tests/resident_reference.py (crop, then batch_reference.assemble).

Every comparison is torch.equal.  Stores are carved out of larger 0xAB-filled uint8 buffers at byte offsets 0 to 3 and destinations out
of NaN-filled buffers whose margins have to stay NaN, as in tests/test_gpu_batch.py.  No test hands the device a table that points
outside its store: the kernel's clamp is there to be read, not provoked.
"""
import glob
import os
import random
import re

import numpy as np
import pytest
import torch
import yaml

import batch_reference as ref
import resident_reference as rref
from gpu_util import dev

pytestmark = pytest.mark.gpu

PAD = 8   # floats of NaN margin on either side of a destination (32 bytes: the destination stays 16-byte aligned)


def rand_u8(seed, *shape):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def carve(store_np, offset=0):
    """A DeviceFrameStore whose tensor starts `offset` bytes past a 16-byte boundary inside a larger buffer of 0xAB bytes and ENDS
    where the meaningful bytes end -> (store, buffer, first byte)."""
    from realvsr_amd import resident
    d = dev()
    store_np = np.ascontiguousarray(store_np)
    n = store_np.size
    buf = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=d)
    assert buf.data_ptr() % 16 == 0
    start = 16 + offset
    buf[start:start + n] = torch.from_numpy(store_np.reshape(-1)).to(d)
    store = resident.DeviceFrameStore(buf[start:start + n].view(store_np.shape), {('s', i): i for i in range(store_np.shape[0])})
    return store, buf, start


def run(carved, table, frames, S, mode=ref.REVERSE, dst_shift=0):
    """gather_batch from a carved store into a destination that starts PAD + dst_shift floats into a NaN-filled buffer; checks the
    destination's margins and the bytes around the store; returns (out on the CPU, variant)."""
    from realvsr_amd import resident
    store, buf, start = carved
    d = dev()
    table = np.asarray(table, dtype=np.int32)
    B, C = table.shape[0], store.frame_hwc[2]
    total = B * frames * C * S * S
    big = torch.full((total + 2 * PAD + dst_shift,), float('nan'), dtype=torch.float32, device=d)
    out = big[PAD + dst_shift:PAD + dst_shift + total].view(B, frames, C, S, S)
    variant, blocks = resident.gather_plan(out, B, frames, C, S)
    assert blocks == B * frames * ((S + 63) // 64) ** 2
    got = resident.gather_batch(store, torch.from_numpy(table).to(d), frames, S, mode, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.isnan(big[:PAD + dst_shift]).all() and torch.isnan(big[PAD + dst_shift + total:]).all(), 'a store left the destination'
    assert (buf[:start] == 0xAB).all() and (buf[start + store.nbytes:] == 0xAB).all()
    return out.cpu(), variant


def expect(store_np, table, frames, S, mode=ref.REVERSE):
    return torch.from_numpy(rref.gather(store_np, np.asarray(table), frames, S, mode))


# ---------------------------------------------------------------------------------------------------------------- the kernel
H, W, N_STORE = 70, 75, 6     # a row pitch of 225 bytes: odd, so the rows of a crop start at every alignment mod 16
SIZES = (1, 2, 3, 5, 7, 8, 31, 32, 33, 63, 64, 65, 67)
FLAGS = [0, 1, 2, 3, 4, 5, 6, 7, 5]


@pytest.fixture(scope='module')
def store70():
    store_np = rand_u8(70, N_STORE, H, W, 3)
    return store_np, [carve(store_np, offset) for offset in range(4)]


def table_for(S, F, H=H, W=W, n=N_STORE):
    """B = 9 rows with all flag values: the four corners of the frame -- row 1, at (H - S, W - S), ends in the LAST slot, on the last
    byte of the store -- and interior odd origins; slots repeat inside a sample (F = 5 > the distinct values of some rows) and across
    samples, the first and the last slot are used."""
    hi, wi = H - S, W - S
    origins = [(0, 0), (hi, wi), (0, wi), (hi, 0), (min(3, hi), min(5, wi)), (hi // 2 | (hi > 1), wi // 2 | (wi > 1)), (min(1, hi), wi),
               (hi, min(7, wi)), (hi // 3, wi // 3)]
    rows = []
    for b, (h, w) in enumerate(origins):
        slots = [(b * 2 + f * (1 + b % 3)) % n for f in range(F)]
        if b == 0:
            slots = [0] * F                 # a repeated slot, the first one
        if b == 1:
            slots[-1] = n - 1               # the crop that ends on the last byte of the store
        rows.append(slots + [min(h, hi), min(w, wi), FLAGS[b]])
    return rows


@pytest.mark.parametrize('S', SIZES)
def test_sizes_flags_origins_and_offsets(S, store70):
    """Every size around the 64-pixel tile and the 4-pixel store, B = 9 with all flag values mixed in one launch, F = 1, 3, 5 with
    repeated slots, the store at every byte offset mod 4."""
    store_np, carved = store70
    for F, offsets in ((3, range(4)), (1, (S % 4,)), (5, ((S + 1) % 4,))):
        table = table_for(S, F)
        assert table[1][F - 1] == N_STORE - 1 and table[1][F:F + 2] == [H - S, W - S] and table[0][:F] == [0] * F
        want = expect(store_np, table, F, S)
        for offset in offsets:
            got, variant = run(carved[offset], table, F, S)
            assert variant == (1 if S % 4 == 0 else 0)
            assert torch.equal(got, want), 'S %d F %d offset %d' % (S, F, offset)


def test_one_channel_and_mode_0():
    grey = rand_u8(33, 4, 33, 37, 1)
    for offset in (0, 3):
        carved = carve(grey, offset)
        for S, mode in ((5, 0), (32, 1), (33, 0)):
            table = table_for(S, 3, 33, 37, 4)
            got, _ = run(carved, table, 3, S, mode)
            assert tuple(got.shape) == (9, 3, 1, S, S) and torch.equal(got, expect(grey, table, 3, S, mode)), (S, mode, offset)
    store_np = rand_u8(34, N_STORE, H, W, 3)
    carved = carve(store_np, 1)
    for S in (20, 67):
        table = table_for(S, 3)
        got, _ = run(carved, table, 3, S, 0)
        assert torch.equal(got, expect(store_np, table, 3, S, 0)), S
        assert not torch.equal(got, expect(store_np, table, 3, S, ref.REVERSE))


def test_conversion_in_both_byte_orders():
    """RVSR_ASM_TO_YCBCR on rows of the frame that holds every (R, G, B): two 64-row bands as the store's frames, 64 x 64 and 20 x 20
    crops along them; the restatement applies batch_reference.ycbcr_int."""
    rgb = np.stack([ref.all_triples(slice(r0, r0 + 64)) for r0 in (1216, 3008)])
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    table64 = [[0, 1, 0, 0, 0], [1, 0, 0, 4032, 6], [0, 0, 0, 1999, 3], [1, 1, 0, 777, 5]]
    table20 = [[1, 0, 44, 4076, 7], [0, 1, 13, 255, 1], [0, 0, 0, 0, 4]]
    for src, mode in ((rgb, ref.TO_YCBCR), (bgr, ref.TO_YCBCR | ref.REVERSE)):
        carved = carve(src, mode)
        for table, S in ((table64, 64), (table20, 20)):
            got, _ = run(carved, table, 2, S, mode)
            assert torch.equal(got, expect(src, table, 2, S, mode)), (mode, S)
    assert torch.equal(expect(rgb, table64, 2, 64, ref.TO_YCBCR), expect(bgr, table64, 2, 64, ref.TO_YCBCR | ref.REVERSE))


def test_every_plan_variant_is_reached(store70):
    """Two variants, as for rvsr_assemble_plan: 16-byte stores, and scalar stores -- reached by an odd size and, at a size of 64, by a
    destination that is only 4-byte aligned."""
    store_np, carved = store70
    seen = {}
    for name, S, kw in (('vector', 64, {}), ('misaligned dst', 64, {'dst_shift': 1}), ('odd size', 66, {})):
        table = table_for(S, 2)
        got, seen[name] = run(carved[2], table, 2, S, **kw)
        assert torch.equal(got, expect(store_np, table, 2, S)), name
    assert seen == {'vector': 1, 'misaligned dst': 0, 'odd size': 0}


def test_a_store_past_4_gib():
    """2 800 slots of 1024 x 512 x 3: the last slot starts 4.40e9 bytes into the store, beyond what 32 bits hold.  Only the slots read
    are written; slots 68 and 69, where the last slot's bytes land modulo 2^32, hold other frames."""
    from realvsr_amd import resident
    d = dev()
    n, frame_bytes = 2800, 1024 * 512 * 3
    wrapped = ((n - 1) * frame_bytes) % 2 ** 32
    assert (n - 1) * frame_bytes > 2 ** 32 and wrapped // frame_bytes == 68 and wrapped % frame_bytes != 0
    frames = torch.empty(n, 1024, 512, 3, dtype=torch.uint8, device=d)
    written = (0, 68, 69, n - 1)
    small = np.stack([ref.frame('LQ', 7, 1), ref.frame('GT', 7, 2), ref.frame('GT', 9, 4), ref.frame('LQ', 8, 3)])
    for k, slot in enumerate(written):
        frames[slot] = torch.from_numpy(small[k]).to(d)
    store = resident.DeviceFrameStore(frames, {('s', i): i for i in range(n)})
    table = [[n - 1, 0, 960, 448, 5], [0, n - 1, 333, 111, 2], [68, 69, 0, 0, 0]]     # (row 0 ends on the last byte of the store)
    got = resident.gather_batch(store, torch.tensor(table, dtype=torch.int32, device=d), 2, 64).cpu()
    want = expect(small, [[written.index(r[0]), written.index(r[1])] + r[2:] for r in table], 2, 64)
    del store, frames
    torch.cuda.empty_cache()
    assert torch.equal(got, want)


def test_refusals():
    from realvsr_amd import resident
    d = dev()
    store, _, _ = carve(rand_u8(1, 2, 12, 10, 3))
    table = torch.zeros(2, 4, dtype=torch.int32, device=d)
    assert tuple(resident.gather_batch(store, table, 1, 10).shape) == (2, 1, 3, 10, 10)
    with pytest.raises(RuntimeError, match='leaves'):
        resident.gather_batch(store, table, 1, 11)
    with pytest.raises(RuntimeError, match='empty'):
        resident.gather_batch(store, table, 1, 0)
    with pytest.raises(RuntimeError, match='mode'):
        resident.gather_batch(store, table, 1, 8, 4)
    with pytest.raises(RuntimeError, match='table'):
        resident.gather_batch(store, table, 2, 8)
    with pytest.raises(RuntimeError, match='table'):
        resident.gather_batch(store, table.long(), 1, 8)
    with pytest.raises(RuntimeError, match='table'):
        resident.gather_batch(store, table.cpu(), 1, 8)
    with pytest.raises(RuntimeError, match='out'):
        resident.gather_batch(store, table, 1, 8, out=torch.zeros(2, 1, 3, 8, 9, device=d))
    two, _, _ = carve(rand_u8(2, 2, 12, 10, 2))
    with pytest.raises(RuntimeError, match='channels'):
        resident.gather_batch(two, table, 1, 8)
    grey, _, _ = carve(rand_u8(3, 2, 12, 10, 1))
    with pytest.raises(RuntimeError, match='YCbCr'):
        resident.gather_batch(grey, table, 1, 8, ref.TO_YCBCR)


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('resident_tree')
    return root, rref.write_tree(root)


def _net():
    return {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1, 'back_RBs': 1,
            'predeblur': False, 'HR_in': False, 'w_TSA': False, 'center': None}


@pytest.mark.parametrize('cls', ['RealVSRDataset', 'RealVSRAllPairDataset'])
def test_resident_batches_equal_the_file_loaders(cls, tree):
    """Three batches of the file loader (n_workers 0) through feed_packed == three batches of the ResidentLoader under the same seeds,
    from PNG files; VideoSRModel.feed_data takes a resident batch through its float branch to the same var_L / var_H."""
    from realvsr_amd import data, resident
    from realvsr_amd.VideoSR_model import create_model
    root, frames = tree
    torch.cuda.set_device(0)
    dataset_opt = rref.tree_opt(root)
    opt = {'dist': False, 'gpu_ids': [0]}
    ds = getattr(data, cls)(dataset_opt)
    random.seed(8)
    torch.manual_seed(8)
    packed = [b for b, _ in zip(data.create_dataloader(ds, dataset_opt, opt, None), range(3))]
    want = [data.feed_packed(b, dev()) for b in packed]
    random.seed(8)
    torch.manual_seed(8)
    loader = resident.create_resident_loader(ds, dataset_opt, opt, None)
    assert loader.lq_store.frames.is_cuda and len(loader.lq_store) == 100 and loader.gt_store.nbytes == 100 * 40 * 24 * 3
    slot = loader.gt_store.index['001', 17]
    assert torch.equal(loader.gt_store.frames[slot].cpu(), torch.from_numpy(np.ascontiguousarray(frames['GT', '001', 17])))
    got = [b for b, _ in zip(loader, range(3))]
    n_gt = (4, 3, 3, 16, 16) if cls == 'RealVSRAllPairDataset' else (4, 3, 16, 16)
    for k in range(3):
        assert got[k]['key'] == list(packed[k]['key'])
        assert got[k]['LQs'].is_cuda and got[k]['LQs'].dtype == torch.float32 and tuple(got[k]['LQs'].shape) == (4, 3, 3, 16, 16)
        assert tuple(got[k]['GT'].shape) == n_gt
        assert torch.equal(got[k]['LQs'], want[k][0]) and torch.equal(got[k]['GT'], want[k][1]), 'batch %d' % k
    assert not torch.equal(got[0]['LQs'], got[1]['LQs'])

    torch.manual_seed(0)
    model = create_model({'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1,
                          'augment': None, 'network_G': _net(), 'path': {'pretrain_model_G': None, 'strict_load': True},
                          'train': {'pixel_criterion_y': 'cb', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 0.5,
                                    'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-4, 'beta1': 0.9, 'beta2': 0.99}})
    model.feed_data(packed[1])
    var_L, var_H = model.var_L.clone(), model.var_H.clone()
    model.feed_data(got[1])
    assert torch.equal(model.var_L, var_L) and torch.equal(model.var_H, var_H)
    model.optimize_parameters(1)
    assert np.isfinite(model.get_current_log()['l_pix'])


LOSS_LINE = re.compile(r'<epoch:\s*\d+, iter:\s*([\d,]+), lr:\([^)]*\)>, (.*)')


def test_driver_logs_the_same_losses_with_and_without_resident(tmp_path):
    """realvsr_amd.train.main for 3 iterations on the tiny set-up of tests/test_gpu_train_driver.py (its option file and tree,
    n_workers 0, the seed of the option file), once with the file loader and once with `resident: true`: the log lines carry the same
    loss terms, compared as logged."""
    import test_gpu_train_driver as driver
    from realvsr_amd import _lib, train
    torch.cuda.set_device(0)
    with open(driver._write_option_file(tmp_path)) as f:
        base = yaml.safe_load(f)
    base['train'].update(niter=3, val_freq=None)
    base['logger'].update(save_checkpoint_freq=100)
    del base['datasets']['val']
    assert base['datasets']['train']['n_workers'] == 0 and base['train']['manual_seed'] is not None
    old = _lib.get_gemm_mode()
    _lib.set_gemm_mode('f32')
    logs = {}
    try:
        for name, resident_key in (('file', None), ('resident', True)):
            opt = dict(base, name='e2e_' + name)
            opt['datasets'] = {'train': dict(base['datasets']['train'])}
            if resident_key is not None:
                opt['datasets']['train']['resident'] = resident_key
            path = os.path.join(str(tmp_path), name + '.yml')
            with open(path, 'w') as f:
                yaml.safe_dump(opt, f)
            assert train.main(['-opt', path, '--root', str(tmp_path)]) == 3
            with open(glob.glob(os.path.join(str(tmp_path), 'experiments', 'e2e_' + name, 'train_e2e_%s_*.log' % name))[0]) as f:
                logs[name] = f.read()
    finally:
        _lib.set_gemm_mode(old)
    assert 'Resident LQ store: 20 frames of 40 x 24 x 3, 57,600 bytes' in logs['resident'] and 'Resident GT store' in logs['resident']
    assert 'Resident' not in logs['file']
    lines = {k: LOSS_LINE.findall(v) for k, v in logs.items()}
    for k in lines:
        print(k, lines[k])
    assert [it for it, _ in lines['file']] == ['1', '2', '3'] and all('l_pix_y:' in terms for _, terms in lines['file'])
    assert lines['resident'] == lines['file']
