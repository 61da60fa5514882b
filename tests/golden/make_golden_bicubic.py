#!/usr/bin/env python
"""Generate tests/golden/bicubic.npz by DRIVING the reference's imresize_np and its two Vimeo-90K dataset classes (build container only).

Run from the repo root:   python tests/golden/make_golden_bicubic.py
Needs /root/reference (read-only); imported the way make_golden_batch.py does (import_reference stubs cv2 and lmdb).

Part 1, the chains.  For every image below and every chain (scale 2 | 4, SAME | DOWN) that the image's size admits:
    <image>.src                 uint8 [H, W, 3]
    <image>.s<scale>.down       clip(round(255 * imresize_np(src / 255, 1 / scale)), 0, 255)                      (what imwrite stores)
    <image>.s<scale>.same       clip(round(255 * imresize_np(imresize_np(src / 255, 1 / scale), scale)), 0, 255)  (generate_LR_BI_Vimeo90K.m:28)
  and in meta['near_half'] the share of values whose EXACT result (tests/bicubic_reference.py) lies within 1e-3 of a half-integer, where
  the reference's float32 sums may round the other way; asserted <= 1 % here.  The step image is asserted to make both clamps fire.

Part 2, the data sets.  A synthetic tree of three septuplets of 32 x 48 noise frames (tree.GT uint8 [3, 7, 32, 48, 3] in cv2's byte
order, sequence s = 0, 1, 2 at 00001/000<s+1>/im<1..7>.png) and its two LQ copies written by the chains above (tree.LQ_same2: BIx2_same;
tree.LQ_down4: the x4 set-up).  The tree's seed is chosen so that the reference's LQ bytes EQUAL the exact model on every frame
(asserted), so the end-to-end comparisons of the tests can use ==.  (A seed with no value at all within 1e-3 of a half-integer does
not exist at this size: 0.1 - 0.3 % of noise values lie there; the recorded shares say how many.)
The reference's classes are driven with two substitutions: data.util.read_img returns tree[path].astype(np.float32) / 255. (read_img's
own value map, as in make_golden_batch.py), and the frame size the classes hard-code for the crop range, (3, 256, 448), reads
(3, 32, 48) -- the classes are executed from their own source with that one literal replaced.  One dataset object serves all samples of
a run, so the persistent frame_list.reverse() shows.  Recorded per run r (meta['runs'][r]): cls, opt, seed, indices and per sample
the paths asked for and random.random() right after; arrays r<r>.s<i>.LQs / .GT as uint8 (the float32 tensors times 255, exact).
"""
import inspect
import json
import os
import pickle
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, import_reference  # noqa: E402
import bicubic_reference as br  # noqa: E402

TREE_HW = (32, 48)
KEYS = ['00001_0001', '00001_0002', '00001_0003']


def images():
    rng = np.random.RandomState(18)
    out = {'noise_a': rng.randint(0, 256, (48, 64, 3)).astype(np.uint8), 'noise_b': rng.randint(0, 256, (96, 80, 3)).astype(np.uint8),
           'step': br.step_image(32, 48)}
    # the frames at the minimum edge hold 72 and 288 values, of which one is already more than 1 %: the first draw with none near a half
    for name, hw, scales in (('min2', (4, 6), (2,)), ('min4', (8, 12), (2, 4))):
        while True:
            out[name] = rng.randint(0, 256, hw + (3,)).astype(np.uint8)
            if not any(near_half_share(out[name], s, m) for s in scales for m in (br.SAME, br.DOWN)):
                break
    return out


def reference_chain(imresize_np, src, scale, mode):
    x = imresize_np(src.astype(np.float32) / np.float32(255.), 1 / scale)
    if mode == br.SAME:
        x = imresize_np(x, scale)
    return np.clip(np.round(255. * x.astype(np.float64)), 0, 255).astype(np.uint8)


def near_half_share(src, scale, mode):
    return float(br.near_half(br.numerators(src, scale, mode), br.shift_bits(scale, mode)).mean())


def run_options():
    base = {'interval_list': [1], 'random_reverse': True, 'border_mode': False, 'data_type': 'img', 'phase': 'train', 'color': None}
    same = dict(base, dataroot_GT='GT', dataroot_LQ='LQ_same2', GT_size=16, LQ_size=16, scale=1)
    down = dict(base, dataroot_GT='GT', dataroot_LQ='LQ_down4', GT_size=16, LQ_size=4, scale=4)
    runs = []
    for cls in ('Vimeo90kAllPairDataset', 'Vimeo90kDataset'):
        runs.append((cls, dict(same, N_frames=3, use_flip=True, use_rot=True)))
        runs.append((cls, dict(same, N_frames=7, use_flip=False, use_rot=True)))
        runs.append((cls, dict(down, N_frames=5, use_flip=True, use_rot=True)))
        runs.append((cls, dict(down, N_frames=1, use_flip=True, use_rot=False, random_reverse=False)))
    return runs


def main():
    import_reference()
    import data.util as data_util
    import data.Vimeo90K_dataset as vimeo

    meta, arrays = {'near_half': {}, 'keys': KEYS, 'tree_hw': list(TREE_HW)}, {}
    for name, src in images().items():
        arrays[name + '.src'] = src
        for scale in (2, 4):
            if min(src.shape[:2]) < 2 * scale or src.shape[0] % scale or src.shape[1] % scale:
                continue
            for mode, tag in ((br.DOWN, 'down'), (br.SAME, 'same')):
                key = '%s.s%d.%s' % (name, scale, tag)
                arrays[key] = reference_chain(data_util.imresize_np, src, scale, mode)
                meta['near_half'][key] = near_half_share(src, scale, mode)
                assert meta['near_half'][key] <= 0.01, (key, meta['near_half'][key])
                if name == 'step':
                    N, b = br.numerators(src, scale, mode), br.shift_bits(scale, mode)
                    assert (N + (1 << (b - 1)) < 0).any() and ((N + (1 << (b - 1))) >> b > 255).any(), key

    # the tree: the first seed whose reference LQ bytes equal the exact model everywhere
    for tree_seed in range(100):
        rng = np.random.RandomState(1000 + tree_seed)
        gt = rng.randint(0, 256, (3, 7) + TREE_HW + (3,)).astype(np.uint8)
        lq = {}
        for tag, scale, mode in (('LQ_same2', 2, br.SAME), ('LQ_down4', 4, br.DOWN)):
            lq[tag] = np.stack([np.stack([reference_chain(data_util.imresize_np, f, scale, mode) for f in seq]) for seq in gt])
        if all((lq[tag][s, f] == br.degrade_frame(gt[s, f], scale, mode)).all()
               for tag, scale, mode in (('LQ_same2', 2, br.SAME), ('LQ_down4', 4, br.DOWN)) for s in range(3) for f in range(7)):
            break
    else:
        raise AssertionError('no tree seed gives reference == exact model')
    meta['tree_seed'] = 1000 + tree_seed
    arrays['tree.GT'] = gt
    for tag, scale, mode in (('LQ_same2', 2, br.SAME), ('LQ_down4', 4, br.DOWN)):
        arrays['tree.' + tag] = lq[tag]
        meta['near_half']['tree.' + tag] = float(np.mean([near_half_share(f, scale, mode) for seq in gt for f in seq]))
        assert meta['near_half']['tree.' + tag] <= 0.01
    tree = dict(lq, GT=gt)
    asked = []

    def read_img(env, path, size=None):
        assert env is None
        parts = path.replace(os.sep, '/').split('/')
        asked.append('/'.join(parts[-4:]))
        assert parts[-3] == '00001'
        return tree[parts[-4]][int(parts[-2]) - 1, int(parts[-1][2:-4]) - 1].astype(np.float32) / 255.

    data_util.read_img = read_img
    source = inspect.getsource(vimeo)
    assert source.count('(3, 256, 448)') == 4 and source.count('(3, 256 // scale, 448 // scale)') == 2
    source = source.replace('(3, 256, 448)', '(3, %d, %d)' % TREE_HW).replace('(3, 256 // scale, 448 // scale)',
                                                                            '(3, %d // scale, %d // scale)' % TREE_HW)
    small = types.ModuleType('vimeo_small_frames')
    exec(compile(source, 'Vimeo90K_dataset.py (frame size replaced)', 'exec'), small.__dict__)

    tmp = tempfile.mkdtemp()
    single_keys, allpair_keys = os.path.join(tmp, 'single.pkl'), os.path.join(tmp, 'allpair.pkl')
    with open(single_keys, 'wb') as f:
        pickle.dump({'keys': KEYS}, f)      # Vimeo90K_dataset.py:63
    with open(allpair_keys, 'wb') as f:
        pickle.dump(KEYS, f)                # :189
    meta['runs'] = []
    for r, (cls, opt) in enumerate(run_options()):
        dataset = getattr(small, cls)(dict(opt, cache_keys=allpair_keys if 'AllPair' in cls else single_keys))
        assert dataset.paths_GT == KEYS
        seed = 500 + r
        random.seed(seed)
        indices, samples = [0, 2, 1, 1, 0], []
        for i, index in enumerate(indices):
            del asked[:]
            sample = dataset[index]
            samples.append(list(asked))
            for k in ('LQs', 'GT'):
                f32 = sample[k].numpy()
                u8 = np.rint(f32 * 255.).astype(np.uint8)
                assert (u8.astype(np.float32) / np.float32(255.) == f32).all()
                arrays['r%d.s%d.%s' % (r, i, k)] = u8
        run = {'cls': cls, 'opt': opt, 'seed': seed, 'indices': indices, 'samples': samples,
               'next_random': random.random()}
        meta['runs'].append(run)
    path = os.path.join(OUT, 'bicubic.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print('bicubic.npz %.1f KB, tree seed %d' % (os.path.getsize(path) / 1024, meta['tree_seed']))
    print(json.dumps(meta['near_half'], indent=1))


if __name__ == '__main__':
    main()
