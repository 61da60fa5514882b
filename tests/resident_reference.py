"""numpy restatement of rvsr_gather_clips (include/realvsr_hip.h section 12b) and the tiny RealVSR tree the resident tests share.

gather is DEFINED as crop, then batch_reference.assemble: the resident path may differ from the packed path only in where the bytes
come from.  tests/test_resident_host.py holds realvsr_amd.resident.build_table against it, tests/test_gpu_resident.py the kernel.
"""
import os
import pickle

import numpy as np

import batch_reference as ref


def gather(store, table, frames, S, mode=ref.REVERSE):
    """store uint8 [n, H, W, C], table int [B, frames + 3] (slots, row, column, flags) -> float32 [B, frames, C, S, S]."""
    store, table = np.asarray(store), np.asarray(table)
    assert table.ndim == 2 and table.shape[1] == frames + 3
    n, H, W, _ = store.shape
    crops = []
    for row in table:
        h, w = int(row[frames]), int(row[frames + 1])
        assert 0 <= h <= H - S and 0 <= w <= W - S and all(0 <= int(v) < n for v in row[:frames]), row
        crops.append(np.stack([store[int(v), h:h + S, w:w + S] for v in row[:frames]], axis=0))
    return ref.assemble(np.stack(crops, axis=0), table[:, frames + 2], mode)


def write_tree(root, sequences=('000', '001'), n_frames=50, hw=(40, 24), seed=11):
    """<root>/{GT,LQ}/<seq>/<00000>.png, random RGB bytes, and <root>/keys.pkl naming every frame -> {(side, seq, i): the frame as
    cv2.imread would return it (B, G, R)}."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    frames = {}
    for side in ('GT', 'LQ'):
        for seq in sequences:
            os.makedirs(os.path.join(str(root), side, seq))
            for i in range(n_frames):
                rgb = rng.randint(0, 256, size=hw + (3,)).astype(np.uint8)
                Image.fromarray(rgb, 'RGB').save(os.path.join(str(root), side, seq, '%05d.png' % i))
                frames[side, seq, i] = rgb[:, :, ::-1]
    with open(os.path.join(str(root), 'keys.pkl'), 'wb') as f:
        pickle.dump({'keys': ['%s_%05d' % (s, i) for s in sequences for i in range(n_frames)]}, f)
    return frames


def tree_opt(root, hw=(40, 24), **kw):
    """The data-set options of the shipped RealVSR files, shrunk to write_tree's frames."""
    opt = {'name': 'tiny', 'interval_list': [1, 2], 'random_reverse': True, 'N_frames': 3, 'dataroot_GT': os.path.join(str(root), 'GT'),
           'dataroot_LQ': os.path.join(str(root), 'LQ'), 'data_type': 'img', 'GT_size': 16, 'LQ_size': 16, 'remove_list': None,
           'border_mode': False, 'color': None, 'phase': 'train', 'use_flip': True, 'use_rot': True, 'scale': 1,
           'cache_keys': os.path.join(str(root), 'keys.pkl'), 'frame_chw': (3,) + tuple(hw), 'n_workers': 0, 'batch_size': 4}
    opt.update(kw)
    return opt
