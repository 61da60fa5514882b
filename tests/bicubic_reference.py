"""The exact model of csrc/resize_kernels.hip (rvsr_bicubic_u8): MATLAB's antialiased bicubic imresize at the power-of-two factors, in
integers.

The reference's Vimeo-90K option files read `vimeo_septuplet_BIx2_same`, which codes/scripts/generate_LR_BI_Vimeo90K.m:28 writes as
imresize(imresize(img, 1/2, 'bicubic'), 2, 'bicubic') + imwrite; codes/data/util.py:511-710 is the reference's port of that imresize
(cubic :511-516, calculate_weights_indices :519-571, imresize_np :643-710).  Here the weights come out of the same formulas in
fractions.Fraction.  At the factors 1/2, 2, 1/4, 4 every normalised weight is k / D with D a power of two, so a chain's value is N / 2^b
with N an integer sum over the uint8 inputs, and the byte imwrite stores is
    clamp(floor((N + 2^(b-1)) / 2^b), 0, 255)          (the intermediate image is a double in MATLAB: it is not rounded).
tests/test_bicubic_host.py holds this against round(255 * imresize_np(...)) recorded from the reference (tests/golden/bicubic.npz);
tests/test_gpu_bicubic.py holds the kernel against this with ==.
"""
import functools
import math
import os
import pickle
from fractions import Fraction

import numpy as np

SAME, DOWN = 0, 1   # RVSR_BIC_SAME, RVSR_BIC_DOWN (include/realvsr_hip.h, section 13)


def cubic(x):
    """codes/data/util.py:511-516 (a = -0.5)."""
    x = abs(Fraction(x))
    if x <= 1:
        return Fraction(3, 2) * x ** 3 - Fraction(5, 2) * x ** 2 + 1
    if x <= 2:
        return Fraction(-1, 2) * x ** 3 + Fraction(5, 2) * x ** 2 - 4 * x + 2
    return Fraction(0)


def weights_of_output(i, scale):
    """calculate_weights_indices (util.py:519-571, antialiasing on) for the 0-based output i of a resize by `scale` (a Fraction):
    (first 0-based input index, the normalised weights of the consecutive inputs from there, zero end columns dropped)."""
    scale = Fraction(scale)
    kernel_width = Fraction(4) / scale if scale < 1 else Fraction(4)
    u = Fraction(i + 1) / scale + Fraction(1, 2) * (1 - 1 / scale)          # 1-based input coordinate
    left = math.floor(u - kernel_width / 2)
    P = math.ceil(kernel_width) + 2
    idx = [left + k for k in range(P)]
    w = [(scale * cubic((u - k) * scale)) if scale < 1 else cubic(u - k) for k in idx]
    total = sum(w)
    w = [v / total for v in w]
    while w[0] == 0:
        w, idx = w[1:], idx[1:]
    while w[-1] == 0:
        w, idx = w[:-1], idx[:-1]
    return idx[0] - 1, w


@functools.lru_cache(maxsize=None)
def tables(scale):
    """scale 2 | 4 -> (down_first, down_taps, down_den, up_first, up_taps, up_den):
    shrinking by `scale`: output j reads the 4 * scale inputs scale * j + down_first + t with weights down_taps[t] / down_den;
    enlarging by `scale`: output scale * m + p reads the 4 inputs m + up_first[p] + t with weights up_taps[p][t] / up_den.
    Every output of an axis has the same weights up to its phase (asserted over two periods)."""
    s = int(scale)
    rows = [weights_of_output(j, Fraction(1, s)) for j in range(4, 6)]
    assert all(first - s * j == rows[0][0] - s * 4 and w == rows[0][1] for j, (first, w) in zip(range(4, 6), rows))
    down_first = rows[0][0] - s * 4
    down_den = functools.reduce(lambda a, b: a * b // math.gcd(a, b), [w.denominator for w in rows[0][1]])
    down_taps = [int(w * down_den) for w in rows[0][1]]
    up_first, up_taps, dens = [], [], []
    for p in range(s):
        a, b = weights_of_output(4 * s + p, s), weights_of_output(5 * s + p, s)
        assert a[1] == b[1] and a[0] - 4 == b[0] - 5 and len(a[1]) == 4
        up_first.append(a[0] - 4)
        dens.extend(w.denominator for w in a[1])
        up_taps.append(a[1])
    up_den = functools.reduce(lambda a, b: a * b // math.gcd(a, b), dens)
    up_taps = [[int(w * up_den) for w in row] for row in up_taps]
    assert len(down_taps) == 4 * s and sum(down_taps) == down_den and all(sum(r) == up_den for r in up_taps)
    assert down_den & (down_den - 1) == 0 and up_den & (up_den - 1) == 0
    return down_first, down_taps, down_den, up_first, up_taps, up_den


def shift_bits(scale, mode):
    """b of the definition: 16 / 24 for DOWN at scale 2 / 4, 30 / 44 for SAME."""
    _, _, dd, _, _, ud = tables(scale)
    d = dd * dd * (ud * ud if mode == SAME else 1)
    assert d & (d - 1) == 0
    return d.bit_length() - 1


def halo(scale, mode):
    """How far, in frame pixels, an output's taps reach beyond the output pixel itself (DOWN: beyond the scale x scale source pixels of
    the output): the rows and columns the host adds around a crop.  Derived from the tap tables; 7, 3, 15, 6 for (2, SAME), (2, DOWN),
    (4, SAME), (4, DOWN)."""
    s = int(scale)
    df, dt, _, uf, ut, _ = tables(s)
    if mode == DOWN:   # output j owns rows s j .. s j + s - 1 and reads rows s j + df .. s j + df + 4 s - 1
        return max(-df, df + len(dt) - 1 - (s - 1))
    reach = 0
    for p in range(s):   # output y = s m + p reads intermediate rows m + uf[p] .. m + uf[p] + 3, each of which reads as above
        lo = s * uf[p] + df - p
        hi = s * (uf[p] + 3) + df + len(dt) - 1 - p
        reach = max(reach, -lo, hi)
    return reach


def reflect(i, n):
    """Symmetric reflection (-1 -> 0, n -> n - 1), continued periodically.  The reference reflects once (util.py:669-677); once is
    all that ever happens to a frame whose edges are >= 2 * scale, and the periodic form gives the once-reflected intermediate image
    its own reflection for free (the shrinking taps are symmetric)."""
    i = np.asarray(i) % (2 * n)
    return np.where(i >= n, 2 * n - 1 - i, i)


def check_frame(Hf, Wf, scale):
    if scale not in (2, 4):
        raise ValueError('scale %r (2 or 4)' % (scale,))
    if Hf % scale or Wf % scale:
        raise ValueError('the %d x %d frame is no multiple of the scale %d (modcrop it first)' % (Hf, Wf, scale))
    if Hf < 2 * scale or Wf < 2 * scale:
        raise ValueError('the %d x %d frame has an edge below 2 * scale = %d: one reflection no longer suffices' % (Hf, Wf, 2 * scale))


def _shrink_axis(a, scale, axis, positions):
    """int64 numerators of the shrunk image at the (unreflected) output `positions` of `axis`, reading `a` through reflect()."""
    first, taps, _, _, _, _ = tables(scale)
    n = a.shape[axis]
    out = 0
    for t, w in enumerate(taps):
        out = out + w * np.take(a, reflect(scale * positions + first + t, n), axis=axis)
    return out


def _enlarge_axis(a, scale, axis, positions):
    """int64 numerators of the enlarged image at the output `positions` (0 <= position < scale * n) of `axis`."""
    _, _, _, first, taps, _ = tables(scale)
    n = a.shape[axis]
    m, p = positions // scale, positions % scale
    shape = [1] * a.ndim
    shape[axis] = len(positions)
    out = 0
    for t in range(4):
        w = np.array([taps[q][t] for q in p], dtype=np.int64).reshape(shape)
        out = out + w * np.take(a, reflect(m + np.array([first[q] for q in p]) + t, n), axis=axis)
    return out


def numerators(frame, scale, mode, rows=None, cols=None):
    """The integer N of the definition for one uint8 frame [Hf, Wf, C] (or [Hf, Wf]) at the output rows / columns given (default: all):
    int64 [len(rows), len(cols), C].  For DOWN rows and columns index the shrunk image."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8:
        raise ValueError('frames are uint8, got %s' % frame.dtype)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    Hf, Wf = frame.shape[:2]
    check_frame(Hf, Wf, scale)
    a = frame.astype(np.int64)
    Hm, Wm = Hf // scale, Wf // scale
    if mode == DOWN:
        rows = np.arange(Hm) if rows is None else np.asarray(rows)
        cols = np.arange(Wm) if cols is None else np.asarray(cols)
        return _shrink_axis(_shrink_axis(a, scale, 0, rows), scale, 1, cols)
    rows = np.arange(Hf) if rows is None else np.asarray(rows)
    cols = np.arange(Wf) if cols is None else np.asarray(cols)
    mid = _shrink_axis(_shrink_axis(a, scale, 0, np.arange(Hm)), scale, 1, np.arange(Wm))   # exact: never rounded
    return _enlarge_axis(_enlarge_axis(mid, scale, 0, rows), scale, 1, cols)


def round_u8(N, b):
    """clamp(floor((N + 2^(b-1)) / 2^b), 0, 255) -> uint8 (>> on int64 is an arithmetic shift: floor)."""
    assert np.abs(N).max() < 2 ** 53
    return np.clip((N + (1 << (b - 1))) >> b, 0, 255).astype(np.uint8)


def near_half(N, b, eps=1e-3):
    """True where the exact value N / 2^b lies within eps of a half-integer (where a float evaluation may round the other way)."""
    frac = (N & ((1 << b) - 1)).astype(np.float64) / float(1 << b)
    return np.abs(frac - 0.5) <= eps


def degrade_frame(frame, scale, mode):
    """The whole-frame chain: uint8 [Hf, Wf, C] -> uint8 [Hf, Wf, C] (SAME) or [Hf / scale, Wf / scale, C] (DOWN)."""
    return round_u8(numerators(frame, scale, mode), shift_bits(scale, mode))


def check_geometry(geom, window_hw, frame_hw, crop_hw, scale, mode):
    """The window / geometry contract of rvsr_bicubic_u8 for one sample; raises ValueError where the entry point (or the Python
    wrapper, for what only the device sees) refuses."""
    wy, wx, y0, x0 = (int(v) for v in geom)
    (Hw, Ww), (Hf, Wf), (Sh, Sw) = window_hw, frame_hw, crop_hw
    check_frame(Hf, Wf, scale)
    h = halo(scale, mode)
    for name, w0, W, c0, S, F in (('rows', wy, Hw, y0, Sh, Hf), ('columns', wx, Ww, x0, Sw, Wf)):
        if S <= 0 or c0 < 0 or c0 + S > F:
            raise ValueError('the crop %s [%d, %d) leave the frame (%d)' % (name, c0, c0 + S, F))
        if W > F or w0 < 0 or w0 + W > F:
            raise ValueError('the window %s [%d, %d) leave the frame (%d)' % (name, w0, w0 + W, F))
        if mode == DOWN and (c0 % scale or S % scale):
            raise ValueError('DOWN needs crop %s at multiples of the scale %d, got origin %d, size %d' % (name, scale, c0, S))
        lo, hi = c0 - h, c0 + S - 1 + h        # what the outputs touch, before reflection
        need_lo, need_hi = max(lo, 0), min(hi, F - 1)
        if lo < 0:
            need_lo, need_hi = 0, max(need_hi, min(-1 - lo, F - 1))
        if hi >= F:
            need_lo, need_hi = min(need_lo, max(2 * F - 1 - hi, 0)), F - 1
        if w0 > need_lo or w0 + W - 1 < need_hi:
            raise ValueError('the window %s [%d, %d) do not cover [%d, %d], the crop plus its halo of %d after reflection'
                             % (name, w0, w0 + W, need_lo, need_hi, h))


def degrade_window(window, geom, frame_hw, crop_hw, scale, mode):
    """The window / geometry form for one image: `window` uint8 [Hw, Ww, C] holds the frame's rows wy .. wy + Hw - 1 and columns
    wx .. wx + Ww - 1; geom = (wy, wx, y0, x0).  Returns (dst, crop): dst is the whole-frame chain's value at the crop (SAME: uint8
    [Sh, Sw, C]; DOWN: [Sh / scale, Sw / scale, C]), crop the window's bytes at the crop.  Frame pixels outside the window are never
    read: the frame is rebuilt with a value (0) the result must not depend on, and check_geometry guarantees that it does not."""
    window = np.asarray(window)
    if window.ndim == 2:
        window = window[:, :, None]
    wy, wx, y0, x0 = (int(v) for v in geom)
    check_geometry(geom, window.shape[:2], frame_hw, crop_hw, scale, mode)
    Hf, Wf = frame_hw
    Sh, Sw = crop_hw
    frame = np.zeros((Hf, Wf, window.shape[2]), dtype=np.uint8)
    frame[wy:wy + window.shape[0], wx:wx + window.shape[1]] = window
    if mode == DOWN:
        rows, cols = np.arange(y0 // scale, (y0 + Sh) // scale), np.arange(x0 // scale, (x0 + Sw) // scale)
    else:
        rows, cols = np.arange(y0, y0 + Sh), np.arange(x0, x0 + Sw)
    dst = round_u8(numerators(frame, scale, mode, rows, cols), shift_bits(scale, mode))
    return dst, frame[y0:y0 + Sh, x0:x0 + Sw].copy()


def bicubic_u8(src, geom, frame_hw, crop_hw, scale, mode):
    """rvsr_bicubic_u8 on the host: src uint8 [B, F, Hw, Ww, C], geom int [B, 4] or None -> (dst, crop) uint8 [B, F, ., ., C]."""
    src = np.asarray(src)
    B, F = src.shape[:2]
    dst, crop = [], []
    for b in range(B):
        g = (0, 0, 0, 0) if geom is None else geom[b]
        pairs = [degrade_window(src[b, f], g, frame_hw, crop_hw, scale, mode) for f in range(F)]
        dst.append(np.stack([p[0] for p in pairs]))
        crop.append(np.stack([p[1] for p in pairs]))
    return np.stack(dst), np.stack(crop)


def step_image(H, W, C=3):
    """The 0 / 255 step edge (left half) plus checkerboard (right half) image: its over- and undershoots make both clamps fire.  The
    edges and the checkerboard's 4 x 4 squares sit at multiples of 4: an edge at the centre of a shrinking output's taps (an odd position
    at scale 2, 2 mod 4 at scale 4) puts half of the symmetric weights on either side and makes the value an exact tie, 127.5."""
    y, x = np.mgrid[0:H, 0:W]
    a = np.where(x < W // 2, np.where(x < W // 4, 0, 255), np.where((y // 4 + x // 4) % 2 == 0, 255, 0))
    a = np.where(y < H // 4, np.where(y < H // 8, 255, 0), a)
    return np.repeat(a[:, :, None], C, axis=2).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the fixture's tree
def write_tree(g, meta, root):
    """The synthetic Vimeo-90K tree of tests/golden/bicubic.npz as PNG files under `root` (GT, LQ_same2, LQ_down4) and its two key files."""
    from PIL import Image
    for tag in ('GT', 'LQ_same2', 'LQ_down4'):
        for s, key in enumerate(meta['keys']):
            a, b = key.split('_')
            os.makedirs(os.path.join(root, tag, a, b))
            for f in range(7):
                Image.fromarray(np.ascontiguousarray(g['tree.' + tag][s, f][:, :, ::-1])).save(   # (the arrays are in cv2's byte order)
                    os.path.join(root, tag, a, b, 'im%d.png' % (f + 1)))
    with open(os.path.join(root, 'single.pkl'), 'wb') as f:
        pickle.dump({'keys': meta['keys']}, f)
    with open(os.path.join(root, 'allpair.pkl'), 'wb') as f:
        pickle.dump(meta['keys'], f)


def make_dataset(run, root, meta, synthesize=False):
    """The data set of a recorded run on that tree; synthesize: with synthesize_LQ and no LQ root."""
    from realvsr_amd import data
    opt = dict(run['opt'], dataroot_GT=os.path.join(root, 'GT'), dataroot_LQ=os.path.join(root, run['opt']['dataroot_LQ']),
               cache_keys=os.path.join(root, 'allpair.pkl' if 'AllPair' in run['cls'] else 'single.pkl'),
               frame_chw=(3,) + tuple(meta['tree_hw']))
    if synthesize:
        opt = dict(opt, synthesize_LQ=True, dataroot_LQ=None)
    return getattr(data, run['cls'])(opt)
