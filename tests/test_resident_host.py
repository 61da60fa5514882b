"""Host side of the resident training set (realvsr_amd/resident.py), no GPU: the table build_table makes against the numpy gather of
tests/resident_reference.py, its refusals, the store's refusals and budget, and the order in which a ResidentLoader draws its plans --
that of data.create_dataloader with n_workers 0, for both data-set classes, shuffled and under a 2-replica DistIterSampler, with
border_mode on and off.  Stores live in host memory here (device='cpu'); tests/test_gpu_resident.py holds the kernel.
"""
import random

import numpy as np
import pytest
import torch

import batch_reference as ref
import resident_reference as rref
from realvsr_amd import _lib, data, resident


# ---------------------------------------------------------------------------------------------------------------- the table
def _formula_store(side):
    keys = [('%03d' % seq, idx) for seq in (3, 4) for idx in range(20, 25)]
    return resident.DeviceFrameStore.from_frames((ref.frame(side, s, i) for s, i in keys), keys, frame_chw=data.FRAME_CHW, device='cpu')


def _formula_plans(n_frames=3, size=8):
    opt = {'interval_list': [1], 'random_reverse': True, 'N_frames': n_frames, 'GT_size': size, 'LQ_size': size, 'border_mode': False,
           'phase': 'train', 'use_flip': True, 'use_rot': True}
    random.seed(23)
    return [data.draw_sample(opt, '%03d_%05d' % (3 + i % 2, 21 + i % 3)) for i in range(9)]


def test_build_table_against_the_reference_on_formula_frames():
    """The table's rows gathered by the restatement == the crops of data.crop_u8 on the same formula frames through
    batch_reference.assemble: slots, origins and flags all land where the packed path puts them."""
    plans = _formula_plans()
    assert len({p['flags'] for p in plans}) > 3 and len({p['name_a'] for p in plans}) == 2
    for side in ('LQ', 'GT'):
        store = _formula_store(side)
        assert len(store) == 10 and store.frame_hwc == (1024, 512, 3) and store.nbytes == 10 * 1024 * 512 * 3
        for single in (False, True):
            table = resident.build_table(plans, store, single=single)
            F = 1 if single else 3
            assert table.dtype == torch.int32 and tuple(table.shape) == (9, F + 3) and not table.is_cuda
            got = rref.gather(store.frames.numpy(), table.numpy(), F, 8)
            crops = np.stack([np.stack([data.crop_u8(ref.frame(side, p['name_a'], v), p)
                                        for v in ([int(p['center'])] if single else p['neighbor_list'])]) for p in plans])
            want = ref.assemble(crops, [p['flags'] for p in plans])
            assert got.shape == (9, F, 3, 8, 8) and (got == want).all()
            for row, p in zip(table.tolist(), plans):
                assert row[F:] == [p['rnd_h'], p['rnd_w'], p['flags']]
                assert row[:F] == [store.index[p['name_a'], v] for v in ([int(p['center'])] if single else p['neighbor_list'])]


def test_build_table_refusals():
    store = _formula_store('LQ')
    plan = _formula_plans()[0]
    assert tuple(resident.build_table([plan], store).shape) == (1, 6)
    with pytest.raises(ValueError, match='sequence'):
        resident.build_table([dict(plan, name_a='777')], store)
    with pytest.raises(ValueError, match='frame 30'):
        resident.build_table([dict(plan, neighbor_list=[22, 23, 30])], store)
    with pytest.raises(ValueError, match='frame 30'):
        resident.build_table([dict(plan, center='00030')], store, single=True)
    for bad in ({'rnd_h': 1024 - 7}, {'rnd_w': 512 - 7}, {'rnd_h': -1}, {'rnd_w': -1}):
        with pytest.raises(ValueError, match='leaves'):
            resident.build_table([dict(plan, **bad)], store)
    resident.build_table([dict(plan, rnd_h=1024 - 8, rnd_w=512 - 8)], store)
    with pytest.raises(ValueError, match='crop'):
        resident.build_table([dict(plan, rnd_h=None, rnd_w=None, size=None)], store)
    with pytest.raises(ValueError, match='differ'):
        resident.build_table([plan, dict(plan, neighbor_list=[22, 23])], store)
    with pytest.raises(ValueError):
        resident.build_table([], store)


# ---------------------------------------------------------------------------------------------------------------- the store
def test_store_refusals_and_budget():
    rng = np.random.RandomState(2)
    frames = [rng.randint(0, 256, size=(10, 12, 3)).astype(np.uint8) for _ in range(4)]
    keys = [('000', i) for i in range(4)]
    store = resident.DeviceFrameStore.from_frames(frames, keys, frame_chw=(3, 10, 12), device='cpu')
    assert store.index == {k: i for i, k in enumerate(keys)} and (store.frames[2].numpy() == frames[2]).all()
    grey = resident.DeviceFrameStore.from_frames([f[:, :, 0] for f in frames], keys, device='cpu')
    assert grey.frame_hwc == (10, 12, 1)
    with pytest.raises(ValueError, match='10 x 12'):
        resident.DeviceFrameStore.from_frames(frames, keys, frame_chw=(3, 12, 10), device='cpu')
    with pytest.raises(ValueError, match='10 x 11'):
        resident.DeviceFrameStore.from_frames(frames[:3] + [frames[3][:, :11]], keys, device='cpu')
    with pytest.raises(ValueError, match='channels'):
        resident.DeviceFrameStore.from_frames(frames[:3] + [frames[3][:, :, 0]], keys, device='cpu')
    with pytest.raises(ValueError, match='twice'):
        resident.DeviceFrameStore.from_frames(frames, keys[:3] + keys[:1], device='cpu')
    with pytest.raises(ValueError):
        resident.DeviceFrameStore.from_frames(frames, keys[:3], device='cpu')
    with pytest.raises(ValueError, match='uint8'):
        resident.DeviceFrameStore.from_frames([f.astype(np.int16) for f in frames], keys, device='cpu')
    # 4 frames of 360 bytes against a budget of 1 kB: both numbers are named
    with pytest.raises(RuntimeError, match=r'1\.44e-06 GB .* resident_max_gb = 1e-06 GB') as e:
        resident.DeviceFrameStore.from_frames(frames, keys, device='cpu', resident_max_gb=1e-6)
    print(e.value)
    resident.DeviceFrameStore.from_frames(frames, keys, device='cpu', resident_max_gb=1.44e-6)
    assert resident.RESIDENT_MAX_GB == 128


def test_constants_and_symbols_match_the_header():
    assert 'rvsr_gather_clips' in _lib.SIGNATURES and 'rvsr_gather_plan' in _lib.SIGNATURES
    assert resident.RVSR_ASM_REVERSE == _lib.RVSR_ASM_REVERSE


# ---------------------------------------------------------------------------------------------------------------- plan order
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('resident_tree')
    return root, rref.write_tree(root)


def test_from_dataset_reads_every_frame_once_and_leaves_the_generators_alone(tree):
    root, frames = tree
    ds = data.RealVSRAllPairDataset(rref.tree_opt(root))
    items = resident.dataset_frames(ds)
    assert items == [(s, i) for s in ('000', '001') for i in range(50)]
    random.seed(1)
    torch.manual_seed(1)
    py, th = random.getstate(), torch.get_rng_state()
    for side in ('LQ', 'GT'):
        store = resident.DeviceFrameStore.from_dataset(ds, side, device='cpu', n_workers=0)
        assert len(store) == 100 and store.frame_hwc == (40, 24, 3) and store.load_seconds > 0
        for (s, i), slot in store.index.items():
            assert (store.frames[slot].numpy() == frames[side, s, i]).all()
    in_workers = resident.DeviceFrameStore.from_dataset(ds, 'GT', device='cpu', n_workers=2)     # the same store, decoded in two workers
    assert in_workers.index == store.index and torch.equal(in_workers.frames, store.frames)
    assert random.getstate() == py and torch.equal(torch.get_rng_state(), th)
    with pytest.raises(RuntimeError, match='resident_max_gb'):
        resident.DeviceFrameStore.from_dataset(ds, 'LQ', device='cpu', resident_max_gb=1e-4)    # 288 kB of frames
    with pytest.raises(RuntimeError, match='resident_max_gb'):     # one side fits, the two of a loader do not
        resident.ResidentLoader(ds, 4, resident_max_gb=3e-4)
    with pytest.raises(ValueError, match='40 x 24'):
        resident.DeviceFrameStore.from_dataset(data.RealVSRAllPairDataset(rref.tree_opt(root, frame_chw=(3, 24, 40))), 'LQ', device='cpu')


@pytest.fixture(scope='module')
def stores(tree):
    root, _ = tree
    ds = data.RealVSRAllPairDataset(rref.tree_opt(root))
    return tuple(resident.DeviceFrameStore.from_dataset(ds, side, device='cpu') for side in ('LQ', 'GT'))


@pytest.mark.parametrize('border_mode', [False, True])
@pytest.mark.parametrize('order', ['shuffle', 'dist'])
@pytest.mark.parametrize('cls', ['RealVSRDataset', 'RealVSRAllPairDataset'])
def test_plans_come_in_the_file_loaders_order(cls, order, border_mode, tree, stores, monkeypatch):
    """One epoch of create_dataloader(n_workers 0) with data.draw_sample recorded, against one epoch of the ResidentLoader's plans under
    the same seeds: the same plans batch by batch, the same packed bytes from the tables, and `random` and torch's generator left in
    the same state."""
    root, _ = tree
    dataset_opt = rref.tree_opt(root, border_mode=border_mode)
    opt = {'dist': order == 'dist', 'gpu_ids': [0]}
    if order == 'dist':
        monkeypatch.setattr(torch.distributed, 'get_world_size', lambda: 2)
    ds = getattr(data, cls)(dataset_opt)

    def sampler():
        if order != 'dist':
            return None
        s = data.DistIterSampler(ds, 2, 1, ratio=2)
        s.set_epoch(3)
        return s

    recorded = []
    draw = data.draw_sample

    def recording(*a, **kw):
        recorded.append(draw(*a, **kw))
        return recorded[-1]

    random.seed(5)
    torch.manual_seed(5)
    monkeypatch.setattr(data, 'draw_sample', recording)
    file_batches = list(data.create_dataloader(ds, dataset_opt, opt, sampler()))
    monkeypatch.setattr(data, 'draw_sample', draw)
    file_state = (random.getstate(), torch.get_rng_state())
    B = 2 if order == 'dist' else 4
    assert len(file_batches) == 100 // B and len(recorded) == 100 and all(len(b['key']) == B for b in file_batches)

    random.seed(5)
    torch.manual_seed(5)
    loader = resident.create_resident_loader(ds, dataset_opt, opt, sampler(), lq_store=stores[0], gt_store=stores[1])
    assert len(loader) == len(file_batches)
    plan_batches = list(loader.plans())
    assert random.getstate() == file_state[0] and torch.equal(torch.get_rng_state(), file_state[1])

    assert len(plan_batches) == len(file_batches)
    assert [p for batch in plan_batches for p in batch] == recorded     # keys, frame lists, crop origins, flags: whole plans
    for k, (plans, fb) in enumerate(zip(plan_batches, file_batches)):
        assert [p['key'] for p in plans] == list(fb['key']) and [p['flags'] for p in plans] == fb['flags'].tolist()
        if k < 3:     # the tables name the bytes the file loader packed
            lq_t, gt_t = loader.tables(plans)
            assert (lq_t is gt_t) == (cls == 'RealVSRAllPairDataset') and tuple(gt_t.shape) == (B, 6 if lq_t is gt_t else 4)
            assert (rref.gather(stores[0].frames.numpy(), lq_t.numpy(), 3, 16) == ref.assemble(fb['LQs'].numpy(), fb['flags'].numpy())).all()
            assert (rref.gather(stores[1].frames.numpy(), gt_t.numpy(), gt_t.shape[1] - 3, 16)
                    == ref.assemble(fb['GT'].numpy(), fb['flags'].numpy())).all()
    if order == 'shuffle':
        assert [p['key'] for p in recorded] != sorted(p['key'] for p in recorded)
    if border_mode:
        assert any(p['neighbor_list'][0] == int(p['key'].split('_')[1]) for p in recorded)


def test_loader_refusals(tree, stores):
    root, _ = tree
    with pytest.raises(NotImplementedError, match='training'):
        resident.ResidentLoader(data.RealVSRAllPairDataset(rref.tree_opt(root, phase='val')), 4, lq_store=stores[0], gt_store=stores[1])
    with pytest.raises(NotImplementedError, match='RealVSR'):
        resident.ResidentLoader(object(), 4, lq_store=stores[0], gt_store=stores[1])
    other = resident.DeviceFrameStore(stores[1].frames[:99], {k: v for k, v in stores[1].index.items() if v < 99})
    with pytest.raises(ValueError, match='same frames'):
        resident.ResidentLoader(data.RealVSRAllPairDataset(rref.tree_opt(root)), 4, lq_store=stores[0], gt_store=other)
    with pytest.raises(RuntimeError, match='HIP'):
        resident.gather_batch(stores[0], torch.zeros(1, 6, dtype=torch.int32), 3, 16)
