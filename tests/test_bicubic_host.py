"""The exact bicubic model (tests/bicubic_reference.py), the host side of the degradation (realvsr_amd.data: degrade_window_plan, the two
Vimeo-90K data sets) and the recorded output of the reference (tests/golden/bicubic.npz, written by tests/golden/make_golden_bicubic.py
from imresize_np and from the reference's own Vimeo90kDataset / Vimeo90kAllPairDataset).  No GPU.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

import batch_reference as bref
import bicubic_reference as br
from conftest import load_golden

CHAINS = ((2, br.SAME), (2, br.DOWN), (4, br.SAME), (4, br.DOWN))
TAG = {br.SAME: 'same', br.DOWN: 'down'}


@pytest.fixture(scope='module')
def fixture():
    g = load_golden('bicubic')
    return g, json.loads(str(g['meta']))


def test_tables_denominators_and_halos():
    """The constants of the issue.  (It lists the x 2 rows by MATLAB's 1-based output parity; x 4 and everything here count from 0.)"""
    first, taps, den, up_first, up, up_den = br.tables(2)
    assert (first, taps, den) == (-3, [-3, -9, 29, 111, 111, 29, -9, -3], 256)
    assert up == [[-3, 29, 111, -9], [-9, 111, 29, -3]] and up_first == [-2, -1] and up_den == 128
    first, taps, den, up_first, up, up_den = br.tables(4)
    assert (first, taps, den) == (-6, [-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7], 4096)
    assert up == [[-45, 399, 745, -75], [-7, 93, 987, -49], [-49, 987, 93, -7], [-75, 745, 399, -45]]
    assert up_first == [-2, -2, -1, -1] and up_den == 1024
    for s in (2, 4):
        t = br.tables(s)
        assert sum(t[1]) == t[2] and all(sum(r) == t[5] for r in t[4]) and t[1] == t[1][::-1]
    assert [br.halo(s, m) for s, m in CHAINS] == [7, 3, 15, 6]
    assert [br.shift_bits(s, m) for s, m in CHAINS] == [30, 16, 44, 24]


def test_constants_agree_with_the_header_and_the_package():
    from realvsr_amd import _lib, data
    assert data.RVSR_BIC_SAME == _lib.RVSR_BIC_SAME == br.SAME and data.RVSR_BIC_DOWN == _lib.RVSR_BIC_DOWN == br.DOWN
    assert 'rvsr_bicubic_u8' in _lib.SIGNATURES and 'rvsr_bicubic_halo' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['rvsr_bicubic_u8'][1]) == 16
    assert data.BIC_HALO == {(s, m): br.halo(s, m) for s, m in CHAINS}
    assert [data.bicubic_halo(s, TAG[m]) for s, m in CHAINS] == [7, 3, 15, 6]
    with pytest.raises(ValueError):
        data.bicubic_halo(3, 'same')


def test_worst_case_numerator_fits_the_stated_types():
    """|N| < 2^53 in every chain; the one-stage x 1/4 numerator already exceeds 2^31, the x 1/2 one does not (the kernel's int32).
    With coefficients that sum to D and whose absolute values sum to at most A, bytes in 0 .. 255 give |N| <= 255 (D + A) / 2: the
    positive coefficients sum to (D + A) / 2 at most, and the negative ones weigh less."""
    for s in (2, 4):
        _, dn, dd, _, up, ud = br.tables(s)
        a = sum(abs(v) for v in dn)
        u = max(sum(abs(v) for v in r) for r in up)
        assert 255 * (dd * dd * ud * ud + a * a * u * u) // 2 < 2 ** 53
        assert (255 * a * a < 2 ** 31) == (s == 2) and 255 * a < 2 ** 31   # (the kernel's types rest on the cruder bound 255 A)
        assert (255 * (dd * dd + a * a) // 2 < 2 ** 31) == (s == 2)


def test_model_equals_the_reference_except_near_half(fixture):
    """The exact model against round(255 * imresize_np(...)) for every recorded chain: equal everywhere except where the exact value lies
    within 1e-3 of a half-integer; there the bytes differ by at most 1, and at most 1 % of an array's values are such."""
    g, meta = fixture
    seen = 0
    for key in sorted(k for k in g if k.endswith('.src')):
        name, src = key[:-4], g[key]
        for s, m in CHAINS:
            rec = '%s.s%d.%s' % (name, s, TAG[m])
            if rec not in g:
                assert min(src.shape[:2]) < 2 * s
                continue
            N, b = br.numerators(src, s, m), br.shift_bits(s, m)
            mine, near = br.round_u8(N, b), br.near_half(N, b)
            assert mine.shape == g[rec].shape
            share = float(near.mean())
            print('%s: near-half share %.4f, differing values %d' % (rec, share, int((mine != g[rec]).sum())))
            assert share <= 0.01 and abs(share - meta['near_half'][rec]) < 1e-12
            assert ((mine == g[rec]) | near).all(), rec
            assert np.abs(mine.astype(int) - g[rec].astype(int)).max() <= 1
            seen += 1
    assert seen == 18   # noise_a, noise_b, step, min4: four chains each; min2: scale 2 only
    for tag, s, m in (('LQ_same2', 2, br.SAME), ('LQ_down4', 4, br.DOWN)):   # the tree: equal outright
        for seq_gt, seq_lq in zip(g['tree.GT'], g['tree.' + tag]):
            for f_gt, f_lq in zip(seq_gt, seq_lq):
                assert (br.degrade_frame(f_gt, s, m) == f_lq).all()


def test_both_clamps_fire_on_the_step_image(fixture):
    g, _ = fixture
    assert (g['step.src'] == br.step_image(32, 48)).all()
    for s, m in CHAINS:
        N, b = br.numerators(g['step.src'], s, m), br.shift_bits(s, m)
        q = (N + (1 << (b - 1))) >> b
        assert q.min() < 0 and q.max() > 255, (s, m)
        assert br.round_u8(N, b).min() == 0 and br.round_u8(N, b).max() == 255


def test_minimum_frames(fixture):
    g, _ = fixture
    assert g['min2.src'].shape == (4, 6, 3) and g['min4.src'].shape == (8, 12, 3)
    assert (br.degrade_frame(g['min2.src'], 2, br.SAME) == g['min2.s2.same']).all()
    assert (br.degrade_frame(g['min4.src'], 4, br.SAME) == g['min4.s4.same']).all()
    assert (br.degrade_frame(g['min4.src'], 4, br.DOWN) == g['min4.s4.down']).all()


def _origins(F, S, step):
    """Crop origins along one axis: both ends, next to them, odd ones (multiples of `step` for DOWN), the middle."""
    last = F - S
    cand = {0, step, 3 * step, last // 2 // step * step, last - 3 * step, last - step, last}
    if step == 1:
        cand |= {1, 5, last - 5}
    return sorted(v for v in cand if 0 <= v <= last)


@pytest.mark.parametrize('scale,mode', CHAINS)
def test_window_form_equals_the_crop_of_the_whole_frame(scale, mode):
    """degrade_window_plan's window + geometry give, through the model's window form, exactly the crop of the degraded whole frame: at
    the four corners, along each edge, at odd origins and where the window is clamped at the frame's border."""
    from realvsr_amd import data
    Hf, Wf, S = 48, 64, 16
    frame = np.random.RandomState(scale * 10 + mode).randint(0, 256, (Hf, Wf, 3)).astype(np.uint8)
    whole = br.degrade_frame(frame, scale, mode)
    step = scale if mode == br.DOWN else 1
    h = br.halo(scale, mode)
    clamped = 0
    for y0 in _origins(Hf, S, step):
        for x0 in _origins(Wf, S, step):
            (wy, wx), (Hw, Ww), geom = data.degrade_window_plan({'rnd_h': y0, 'rnd_w': x0, 'size': S}, (Hf, Wf), scale, TAG[mode])
            assert (Hw, Ww) == (min(Hf, S + 2 * h), min(Wf, S + 2 * h)) and geom == (wy, wx, y0, x0)
            assert wy == min(max(y0 - h, 0), Hf - Hw) and wx == min(max(x0 - h, 0), Wf - Ww)
            clamped += wy != y0 - h or wx != x0 - h
            dst, crop = br.degrade_window(frame[wy:wy + Hw, wx:wx + Ww], geom, (Hf, Wf), (S, S), scale, mode)
            if mode == br.DOWN:
                want = whole[y0 // scale:(y0 + S) // scale, x0 // scale:(x0 + S) // scale]
            else:
                want = whole[y0:y0 + S, x0:x0 + S]
            assert (dst == want).all(), (y0, x0)
            assert (crop == frame[y0:y0 + S, x0:x0 + S]).all()
    assert clamped >= 12


def test_window_of_a_frame_smaller_than_the_halo_is_the_whole_frame():
    from realvsr_amd import data
    assert data.degrade_window_plan({'rnd_h': 4, 'rnd_w': 20, 'size': 16}, (32, 48), 4, 'same') == ((0, 2), (32, 46), (0, 2, 4, 20))
    assert data.degrade_window_plan({'rnd_h': None, 'rnd_w': None, 'size': None}, (32, 48), 2, 'same') == ((0, 0), (32, 48), (0, 0, 0, 0))


def test_refusals():
    from realvsr_amd import data
    plan = {'rnd_h': 4, 'rnd_w': 4, 'size': 8}
    for frame_hw, scale in (((31, 48), 2), ((32, 46), 4), ((2, 48), 2), ((32, 4), 4)):   # odd sizes, an edge below 2 * scale
        with pytest.raises(ValueError):
            data.degrade_window_plan(plan, frame_hw, scale, 'same')
        with pytest.raises(ValueError):
            br.check_frame(frame_hw[0], frame_hw[1], scale)
    with pytest.raises(ValueError):
        data.degrade_window_plan(plan, (32, 48), 3, 'same')
    for bad in ({'rnd_h': 5, 'rnd_w': 4, 'size': 8}, {'rnd_h': 4, 'rnd_w': 6, 'size': 8}, {'rnd_h': 4, 'rnd_w': 4, 'size': 6}):
        data.degrade_window_plan(bad, (32, 48), 2, 'same')   # (SAME takes any origin)
        with pytest.raises(ValueError, match='multiples of the scale'):
            data.degrade_window_plan(bad, (32, 48), 4, 'down')
    with pytest.raises(ValueError, match='leave the frame'):
        data.degrade_window_plan({'rnd_h': 28, 'rnd_w': 4, 'size': 8}, (32, 48), 2, 'same')
    # a window that does not cover the halo: one row / column short on either side, in the package's check and in the model's
    Hf, Wf, S, h = 64, 64, 8, 7
    good = (20 - h, 20 - h, 20, 20)
    for check in (data.check_bicubic_geometry, br.check_geometry):
        check(good, (S + 2 * h, S + 2 * h), (Hf, Wf), (S, S), 2, br.SAME)
        for geom, window_hw in (((20 - h + 1, 20 - h, 20, 20), (S + 2 * h, S + 2 * h)), ((20 - h, 20 - h - 1, 20, 20), (S + 2 * h, S + 2 * h)),
                                (good, (S + 2 * h - 1, S + 2 * h)), (good, (S + 2 * h, S + 2 * h - 1)),
                                ((0, 0, 0, 0), (S + h - 1, S + h))):
            with pytest.raises(ValueError, match='do not cover'):
                check(geom, window_hw, (Hf, Wf), (S, S), 2, br.SAME)
        check((0, 0, 0, 0), (S + h, S + h), (Hf, Wf), (S, S), 2, br.SAME)   # (at the origin the leading halo is all reflection)
    with pytest.raises(RuntimeError, match='HIP'):
        data.bicubic_u8(torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8), 2)


# ---------------------------------------------------------------------------------------------------------------- data sets
@pytest.fixture(scope='module')
def tree(fixture, tmp_path_factory):
    g, meta = fixture
    root = str(tmp_path_factory.mktemp('vimeo'))
    br.write_tree(g, meta, root)
    return root


def expected_paths(run, plan):
    """What the reference's read_img was asked for, in its order: GT first, then LQ."""
    a, b = plan['name_a'], plan['name_b']
    gt = plan['frame_list'] if 'AllPair' in run['cls'] else [4]
    return (['GT/%s/%s/im%d.png' % (a, b, v) for v in gt]
            + ['%s/%s/%s/im%d.png' % (run['opt']['dataroot_LQ'], a, b, v) for v in plan['frame_list']])


def test_datasets_reproduce_the_recorded_samples(fixture, tree):
    """Keys, frame lists (with the persistent reversal), crops and flags of both classes, both LR_input branches: the uint8 sample pushed
    through batch_reference.assemble is the reference's float32 sample, and the random stream is consumed alike."""
    from realvsr_amd import data
    g, meta = fixture
    assert len(meta['runs']) == 8
    reversed_seen = 0
    for r, run in enumerate(meta['runs']):
        ds = br.make_dataset(run, tree, meta)
        assert ds.paths_GT == meta['keys'] and len(ds) == 3
        shadow = data.vimeo_frame_list(run['opt']['N_frames'])
        state = random.Random(run['seed'])
        random.seed(run['seed'])
        for i, index in enumerate(run['indices']):
            sample = ds[index]
            plan = data.draw_vimeo_sample(run['opt'], meta['keys'][index], shadow, rng=state, frame_chw=(3,) + tuple(meta['tree_hw']))
            assert expected_paths(run, plan) == run['samples'][i], (r, i)
            assert shadow == ds.frame_list
            reversed_seen += shadow != sorted(shadow)
            assert sample['key'] == meta['keys'][index] and sample['flags'] == plan['flags']
            assert sample['LQs'].dtype == torch.uint8 and sample['GT'].dtype == torch.uint8
            for k in ('LQs', 'GT'):
                want = g['r%d.s%d.%s' % (r, i, k)]
                got = bref.assemble(sample[k].numpy()[None], [sample['flags']])[0]
                if k == 'GT' and 'AllPair' not in run['cls']:
                    got = got[0]
                assert got.shape == want.shape and (got == bref.u8_to_f32(want)).all(), (r, i, k)
        assert random.random() == run['next_random'], r
    assert reversed_seen >= 4


def test_synthesized_samples_give_the_recorded_LQ_through_the_model(fixture, tree):
    """synthesize_LQ: the same draws, no LQ file read; the window and geometry pushed through the exact model on the host give the
    recorded LQ and GT crops."""
    g, meta = fixture
    h_of = {False: br.halo(2, br.SAME), True: br.halo(4, br.DOWN)}
    for r, run in enumerate(meta['runs']):
        ds = br.make_dataset(run, tree, meta, synthesize=True)
        lr_input = run['opt']['GT_size'] != run['opt']['LQ_size']
        scale, mode = (4, br.DOWN) if lr_input else (2, br.SAME)
        assert (ds.synth_scale, ds.synth_mode) == (scale, mode)
        random.seed(run['seed'])
        for i, index in enumerate(run['indices']):
            s = ds[index]
            N, S, side = run['opt']['N_frames'], run['opt']['GT_size'], run['opt']['GT_size'] + 2 * h_of[lr_input]
            assert 'LQs' not in s and 'GT' not in s
            assert s['GT_window'].dtype == torch.uint8 and tuple(s['GT_window'].shape) == (N, side, side, 3)
            assert s['geom'].dtype == torch.int32 and tuple(s['geom'].shape) == (4,)
            assert (s['synth_scale'], s['synth_mode'], s['frame_h'], s['frame_w'], s['crop_size']) == (scale, mode, 32, 48, S)
            lq, gt = br.bicubic_u8(s['GT_window'].numpy()[None], [s['geom'].tolist()], (32, 48), (S, S), scale, mode)
            got_l = bref.assemble(lq, [s['flags']])[0]
            assert (got_l == bref.u8_to_f32(g['r%d.s%d.LQs' % (r, i)])).all(), (r, i)
            if 'AllPair' in run['cls']:
                assert s['gt_index'] == -1
                got_h = bref.assemble(gt, [s['flags']])[0]
            else:
                assert s['gt_index'] == N // 2
                got_h = bref.assemble(gt[:, N // 2:N // 2 + 1], [s['flags']])[0, 0]
            assert (got_h == bref.u8_to_f32(g['r%d.s%d.GT' % (r, i)])).all(), (r, i)
        assert random.random() == run['next_random'], r


def test_synthesize_refuses_what_the_operator_refuses(fixture, tree):
    _, meta = fixture
    run = meta['runs'][0]
    from realvsr_amd import data
    base = dict(run['opt'], dataroot_GT=os.path.join(tree, 'GT'), dataroot_LQ=None, cache_keys=os.path.join(tree, 'allpair.pkl'),
                synthesize_LQ=True)
    with pytest.raises(ValueError):
        data.Vimeo90kAllPairDataset(dict(base, frame_chw=(3, 31, 48)))
    with pytest.raises(ValueError):
        data.Vimeo90kAllPairDataset(dict(base, frame_chw=(3, 32, 48), scale_synth=3))
    with pytest.raises(ValueError):
        data.Vimeo90kAllPairDataset(dict(base, frame_chw=(3, 32, 48), LQ_size=4, scale=8))
    assert data.Vimeo90kAllPairDataset(dict(base, frame_chw=(3, 32, 48), scale_synth=4)).synth_scale == 4
