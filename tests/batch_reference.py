"""numpy restatement of csrc/batch_kernels.hip (rvsr_assemble_clips) and the synthetic frames of the batch fixture.

Everything here follows include/realvsr_hip.h section 12 literally: the float32 division, the flag semantics, the exact-integer YCbCr
conversion.  tests/test_data_host.py holds it against the recorded output of the reference's own dataset classes
(tests/golden/batch.npz) and against numpy's bgr2ycbcr; tests/test_gpu_batch.py holds the kernel against it with ==.
"""
import functools

import numpy as np

REVERSE, TO_YCBCR = 1, 2
FRAME_H, FRAME_W = 1024, 512


@functools.lru_cache(maxsize=1)
def _frame_base():
    y = np.arange(FRAME_H, dtype=np.int64)[:, None, None]
    x = np.arange(FRAME_W, dtype=np.int64)[None, :, None]
    c = np.arange(3, dtype=np.int64)[None, None, :]
    return ((7 * y + 13 * x + 3 * ((y * x) % 17) + 101 * c) & 255).astype(np.uint8)


@functools.lru_cache(maxsize=64)
def _frame(is_gt, seq, idx):
    # (7 y + 13 x + 3 (y x mod 17) + 101 c + 37 idx + 59 seq + 89 [GT]) mod 256; the uint8 addition wraps
    v = _frame_base() + np.uint8((37 * idx + 59 * seq + 89 * int(is_gt)) & 255)
    v.setflags(write=False)
    return v


def frame(root, seq, idx):
    """The synthetic 1024 x 512 x 3 uint8 frame `idx` of sequence `seq` under the 'LQ' or 'GT' root: a formula, never stored.  Every
    value 0 .. 255 occurs, and no flip, transposition, channel order, frame index, sequence or LQ / GT mix-up leaves it unchanged
    (the weights of y, x and c differ and are odd)."""
    assert root in ('LQ', 'GT'), root
    return _frame(root == 'GT', int(seq), int(idx))


def frame_of_path(path):
    """.../<LQ|GT>/<seq>/<00017>.png -> frame(...)"""
    parts = path.replace('\\', '/').split('/')
    return frame(parts[-3], parts[-2], parts[-1].split('.')[0])


def fixture_sample(draw_sample, meta, m):
    """Sample m of tests/golden/batch.npz replayed through `draw_sample` under its seed: (plan, GT paths, LQ paths, the next
    random.random())."""
    import random
    random.seed(m['seed'])
    plan = draw_sample(m['opt'], meta['keys'][m['key_index']])
    nxt = random.random()
    names = ['%05d' % v for v in plan['neighbor_list']]
    gt_names = names if m['cls'] == 'RealVSRAllPairDataset' else [plan['center']]
    return (plan, ['GT/%s/%s.png' % (plan['name_a'], n) for n in gt_names], ['LQ/%s/%s.png' % (plan['name_a'], n) for n in names], nxt)


def u8_to_f32(a):
    """read_img's value map (codes/data/util.py:95): one float32 division."""
    return a.astype(np.float32) / np.float32(255.)


# rows: Y, Cb, Cr; columns: R, G, B -- the matrix of util.bgr2ycbcr times 1000, and its offsets times 255000
YCC_M = np.array([[65481, 128553, 24966], [-37797, -74203, 112000], [112000, -93786, -18214]], dtype=np.int64)
YCC_O = np.array([16, 128, 128], dtype=np.int64) * 255000


def ycbcr_v(rgb):
    """uint8 [..., 3] in R, G, B order -> the exact integers v [..., 3] (Y, Cb, Cr) with value = v / 255000."""
    return rgb.astype(np.int64) @ YCC_M.T + YCC_O


def ycbcr_int(rgb):
    """round-half-even(v / 255000) in integers: uint8 [..., 3] (Y, Cb, Cr)."""
    v = ycbcr_v(rgb)
    q, r = np.divmod(v, 255000)
    q = q + ((r > 127500) | ((r == 127500) & ((q & 1) == 1)))
    assert q.min() >= 0 and q.max() <= 255
    return q.astype(np.uint8)


def ycbcr_ties(rgb):
    """True where v / 255000 is exactly half way between two integers (numpy's float64 answer there depends on its summation order)."""
    return ycbcr_v(rgb) % 255000 == 127500


def ycbcr_numpy(bgr):
    """util.bgr2ycbcr(uint8 B, G, R image, only_y=False) as the reference evaluates it (codes/data/util.py:367-373): float64."""
    rlt = np.matmul(bgr, [[24.966, 112.0, -18.214], [128.553, -74.203, -93.786], [65.481, -37.797, 112.0]]) / 255.0 + [16, 128, 128]
    return rlt.round().astype(np.uint8)


def assemble(u8, flags=None, mode=REVERSE):
    """uint8 [B, F, Hs, Ws, C] -> float32 [B, F, C, Ho, Wo]: rvsr_assemble_clips."""
    u8 = np.asarray(u8)
    B, F, Hs, Ws, C = u8.shape
    out = np.empty((B, F, C, Hs, Ws), dtype=np.float32)
    for b in range(B):
        f = int(flags[b]) if flags is not None else 0
        a = u8[b]
        if f & 2:
            a = a[:, ::-1]
        if f & 1:
            a = a[:, :, ::-1]
        if f & 4:
            assert Hs == Ws
            a = a.transpose(0, 2, 1, 3)
        if mode & TO_YCBCR:
            assert C == 3
            a = ycbcr_int(a[..., ::-1] if mode & REVERSE else a)
        elif mode & REVERSE:
            a = a[..., ::-1]
        out[b] = u8_to_f32(a).transpose(0, 3, 1, 2)
    return out


def read_img_seq(frames_u8):
    """util.read_img_seq (codes/data/util.py:104-122) on frames already decoded: [T, H, W, C] uint8 -> float32 [T, C, H, W]."""
    imgs = np.stack([u8_to_f32(f) for f in frames_u8], axis=0)
    imgs = imgs[:, :, :, [2, 1, 0]] if imgs.shape[-1] == 3 else imgs
    return np.ascontiguousarray(np.transpose(imgs, (0, 3, 1, 2)))


def all_triples(rows=slice(0, 4096)):
    """Rows of the 4096 x 4096 x 3 uint8 frame that holds every (R, G, B): R = y >> 4, G = ((y & 15) << 4) | (x >> 8), B = x & 255."""
    y = np.arange(4096, dtype=np.int64)[rows, None]
    x = np.arange(4096, dtype=np.int64)[None, :]
    t = np.empty((y.shape[0], 4096, 3), dtype=np.uint8)
    t[..., 0] = y >> 4
    t[..., 1] = ((y & 15) << 4) | (x >> 8)
    t[..., 2] = x & 255
    return t
