#!/usr/bin/env python
"""Generate tests/golden/batch.npz by DRIVING the reference's own dataset classes (build container only).

Run from the repo root:   python tests/golden/make_golden_batch.py
Needs /root/reference (read-only); imported the way make_golden.py does (import_reference stubs cv2 and lmdb).

The one substitution: data.util.read_img, which would call cv2.imread, returns
    frame_of_path(path).astype(np.float32) / 255.
i.e. read_img's own value map (codes/data/util.py:95) on the synthetic frame that tests/batch_reference.py computes from the path
(root, sequence, frame index).  Frames are a formula and are never stored.  Everything after the read -- the frame choice, the crop,
util.augment, the stack, [2, 1, 0], the transposition, the tensors -- is the reference's RealVSRDataset.__getitem__ /
RealVSRAllPairDataset.__getitem__ under random.seed(k).

Recorded per sample k (meta: one JSON document; arrays s<k>.LQs, s<k>.GT):
  cls, opt      the class and its option set          key_index, seed     the index into the key list, random.seed
  paths         every path read_img was asked for, in order
  next_random   random.random() right after the sample: pins how much of the stream the sample consumed
"""
import json
import os
import pickle
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, import_reference  # noqa: E402
from batch_reference import frame_of_path  # noqa: E402

SEQUENCES = ('000', '003', '017')   # (none of them among the sequences RealVSRDataset leaves out)
FRAMES = (0, 1, 24, 48, 49)         # both clip ends (the redraw loop / the border branch) and the middle
KEYS = ['%s_%05d' % (s, f) for s in SEQUENCES for f in FRAMES]
SAMPLES = 64


def option_set(k):
    """Sample k's options: the bits of a bijection of k, so that every option is recorded on and off in many combinations."""
    b = (37 * k + 11) % 128
    size = 8 if b & 1 else 5
    return {'interval_list': [1, 2] if b & 4 else [1], 'random_reverse': bool(b & 8), 'N_frames': 3 if b & 2 else 5,
            'dataroot_GT': 'GT', 'dataroot_LQ': 'LQ', 'data_type': 'img', 'GT_size': size, 'LQ_size': size, 'remove_list': None,
            'border_mode': bool(b & 16), 'color': None, 'phase': 'train', 'use_flip': bool(b & 32), 'use_rot': bool(b & 64), 'scale': 1}


def main():
    import_reference()
    import data.util as data_util
    import data.RealVSR_dataset as ds

    asked = []

    def read_img(env, path, size=None):
        assert env is None
        asked.append(path.replace(os.sep, '/'))
        return frame_of_path(path).astype(np.float32) / 255.

    data_util.read_img = read_img
    tmp = tempfile.mkdtemp()
    keys_path = os.path.join(tmp, 'keys.pkl')
    with open(keys_path, 'wb') as f:
        pickle.dump({'keys': KEYS}, f)

    meta, arrays = [], {}
    pick = random.Random(2024)   # (its own generator: the key choice stays outside the stream the samples draw from)
    for k in range(SAMPLES):
        opt = option_set(k)
        cls = ('RealVSRAllPairDataset', 'RealVSRDataset')[k // 32]   # (each class sees all 32 combinations of the five low bits)
        dataset = getattr(ds, cls)(dict(opt, cache_keys=keys_path))
        assert dataset.paths_GT == KEYS
        key_index = pick.randrange(len(KEYS))
        del asked[:]
        random.seed(1000 + k)
        sample = dataset[key_index]
        next_random = random.random()
        assert sample['key'] == KEYS[key_index]
        arrays['s%d.LQs' % k] = sample['LQs'].numpy()
        arrays['s%d.GT' % k] = sample['GT'].numpy()
        meta.append({'cls': cls, 'opt': opt, 'key_index': key_index, 'seed': 1000 + k, 'paths': list(asked), 'next_random': next_random})
        assert arrays['s%d.LQs' % k].dtype == np.float32 and arrays['s%d.LQs' % k].shape == (opt['N_frames'], 3, opt['GT_size'], opt['GT_size'])
    path = os.path.join(OUT, 'batch.npz')
    np.savez_compressed(path, meta=np.array(json.dumps({'keys': KEYS, 'samples': meta})), **arrays)
    print('batch.npz %.1f KB, %d samples' % (os.path.getsize(path) / 1024, SAMPLES))


if __name__ == '__main__':
    main()
