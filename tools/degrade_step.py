#!/usr/bin/env python
"""One JSON line for the bicubic degradation of a training batch on the device (realvsr_amd.data.bicubic_u8, csrc/resize_kernels.hip) at
the shape of the reference's Vimeo-90K option files: --batch x --frames GT windows of (--size + 2 halo)^2 x 3 bytes out of 256 x 448
frames -> the LQ crops and the GT crops, --size^2 x 3 each ('same' at scale 2 by default: the BIx2_same copy; windows 206^2).

  degrade_ms       rvsr_bicubic_u8 alone, LQ and GT crop written (device events, warmed), and
  composed_ms      the LQ tensor from torch operators on the device in f32 (per stage two strided conv2d, or two conv_transpose2d, one
                   per axis; round, clamp, to uint8), the two timed ALTERNATING, --rounds samples each; *_min_max give the spread.
                   The composed path reflects nowhere and shares one tap phase across the batch, so the tool draws crops whose windows
                   are unclamped and start at one phase of the scale; composed_max_byte_diff is its distance from the kernel's bytes
                   (f32 sums against exact integers: at most 1)
  bytes_moved, degrade_tbps   window bytes in + LQ bytes + GT crop bytes out, over degrade_ms, next to the ~6.3 TB/s a stream reaches
  equals_model     the kernel's bytes == tests/bicubic_reference.py on the first sample
  host_ref_ms_per_frame   the reference's host chain on ONE 256 x 448 x 3 frame, restated here in its own shape (float32, symmetric
                   padding, one matrix-vector product per output row / column and channel: codes/data/util.py:643-710), single thread
The measurements run in a child process under --timeout; if it fails nothing further is started on the GPU and the line says so.

usage: python tools/degrade_step.py [--batch B] [--frames N] [--size S] [--scale 2|4] [--mode same|down] [--rounds R] [--inner K]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
FRAME_HW = (256, 448)

from step_timing import event_ms, median  # noqa: E402


def _host_resize(img, scale_num, scale_den):
    """imresize_np's own shape of computation on a float32 [H, W, C] image: weights per output from the cubic, symmetric padding, then
    one matrix-vector product per output row and channel, and the same along the width."""
    import numpy as np
    import bicubic_reference as br
    from fractions import Fraction
    scale = Fraction(scale_num, scale_den)
    for axis in (0, 1):
        n_in = img.shape[axis]
        n_out = int(n_in * scale)
        rows = [br.weights_of_output(i, scale) for i in range(n_out)]
        lo = min(f for f, _ in rows)
        hi = max(f + len(w) - 1 for f, w in rows)
        pad = np.take(img, br.reflect(np.arange(lo, hi + 1), n_in), axis=axis)
        out = np.empty(img.shape[:axis] + (n_out,) + img.shape[axis + 1:], dtype=np.float32)
        for i, (first, w) in enumerate(rows):
            w32 = np.array([float(v) for v in w], dtype=np.float32)
            for c in range(img.shape[2]):
                if axis == 0:
                    out[i, :, c] = pad[first - lo:first - lo + len(w), :, c].T @ w32
                else:
                    out[:, i, c] = pad[:, first - lo:first - lo + len(w), c] @ w32
        img = out
    return img


def _composed(win, scale, mode, h, S, w0=0):
    """The LQ bytes from torch operators: uint8 [B, F, Hw, Ww, C] -> uint8 [B, F, s, s, C]; every window starts at a frame row and
    column that is w0 modulo the scale."""
    import torch
    import torch.nn.functional as F
    import bicubic_reference as br
    first, dn, dd, up_first, up, ud = br.tables(scale)
    B, N, Hw, Ww, C = win.shape
    x = win.permute(0, 1, 4, 2, 3).reshape(B * N * C, 1, Hw, Ww).float()
    kd = torch.tensor(dn, dtype=torch.float32, device=win.device) / dd
    o = (first - w0) % scale             # window rows o, o + scale, ... start a shrunk output's taps
    j0 = (o - first + w0) // scale       # ... the output j0, counted from the multiple of the scale at or before the window
    x = F.conv2d(x[:, :, o:, :], kd.view(1, 1, -1, 1), stride=(scale, 1))
    x = F.conv2d(x[:, :, :, o:], kd.view(1, 1, 1, -1), stride=(1, scale))
    if mode == br.DOWN:
        a = (w0 + h) // scale - j0
        y = x[:, :, a:a + S // scale, a:a + S // scale]
    else:
        ku = torch.zeros(4 * scale, dtype=torch.float32, device=win.device)
        pad = 3 * scale // 2
        for p in range(scale):
            for t in range(4):
                ku[p - scale * (up_first[p] + t) + pad] = up[p][t] / ud
        x = F.conv_transpose2d(x, ku.view(1, 1, -1, 1), stride=(scale, 1), padding=(pad, 0))
        x = F.conv_transpose2d(x, ku.view(1, 1, 1, -1), stride=(1, scale), padding=(0, pad))
        a = w0 + h - scale * j0
        y = x[:, :, a:a + S, a:a + S]
    y = torch.floor(y + 0.5).clamp_(0, 255).to(torch.uint8)
    return y.reshape(B, N, C, y.shape[2], y.shape[3]).permute(0, 1, 3, 4, 2).contiguous()


def measure(B, N, S, scale, mode_name, rounds, inner):
    import random
    import numpy as np
    import torch
    import bicubic_reference as br
    from realvsr_amd import data
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    d = torch.device('cuda', 0)
    mode = data.BIC_MODES[mode_name]
    h = data.bicubic_halo(scale, mode)
    Hf, Wf = FRAME_HW
    rng = random.Random(18)
    geoms = []
    w0 = (-h) % scale if mode == br.DOWN else 0   # (DOWN crops start at multiples of the scale, their windows h before)
    for _ in range(B):   # unclamped windows that all start at w0 modulo the scale (what _composed can follow)
        wy = w0 + scale * rng.randint(0, (Hf - S - 2 * h - w0) // scale)
        wx = w0 + scale * rng.randint(0, (Wf - S - 2 * h - w0) // scale)
        (wy2, wx2), (Hw, Ww), geom = data.degrade_window_plan({'rnd_h': wy + h, 'rnd_w': wx + h, 'size': S}, FRAME_HW, scale, mode)
        assert (wy2, wx2) == (wy, wx) and (Hw, Ww) == (S + 2 * h, S + 2 * h)
        geoms.append(geom)
    g = torch.Generator(device='cuda').manual_seed(3)
    win = torch.randint(0, 256, (B, N, Hw, Ww, 3), device=d, generator=g, dtype=torch.uint8)
    geom = torch.tensor(geoms, dtype=torch.int32)
    for row in geoms:
        data.check_bicubic_geometry(row, (Hw, Ww), FRAME_HW, (S, S), scale, mode)
    geom = geom.to(d)
    res = {'window': [Hw, Ww], 'halo': h}

    def fused():
        return data.bicubic_u8(win, scale, mode, geom=geom, frame_hw=FRAME_HW, crop_hw=(S, S), want_crop=True)

    lq, gt = fused()
    want, _ = br.bicubic_u8(win[:1].cpu().numpy(), geoms[:1], FRAME_HW, (S, S), scale, mode)
    res['equals_model'] = bool((lq[:1].cpu().numpy() == want).all())
    res['crop_equals_window'] = bool(torch.equal(gt, win[:, :, h:h + S, h:h + S]))
    comp = _composed(win, scale, mode, h, S, w0)
    res['composed_max_byte_diff'] = int((comp.int() - lq.int()).abs().max()) if comp.shape == lq.shape else 'shape %s' % (tuple(comp.shape),)
    res['composed_differing_share'] = round(float((comp != lq).float().mean()), 6) if comp.shape == lq.shape else None
    for _ in range(3):
        fused()
        _composed(win, scale, mode, h, S, w0)
    a, b = [], []
    for _ in range(rounds):
        a.append(event_ms(fused, inner))
        b.append(event_ms(lambda: _composed(win, scale, mode, h, S, w0), max(1, inner // 4)))
    res['degrade_ms'], res['degrade_ms_min_max'] = round(median(a), 5), [round(min(a), 5), round(max(a), 5)]
    res['composed_ms'], res['composed_ms_min_max'] = round(median(b), 5), [round(min(b), 5), round(max(b), 5)]
    res['bytes_moved'] = win.numel() + lq.numel() + gt.numel()
    res['degrade_tbps'] = round(res['bytes_moved'] / (median(a) * 1e-3) / 1e12, 4)
    res['fused_below_composed_by_more_than_the_spread'] = bool(max(a) < min(b))

    frame = np.random.RandomState(5).randint(0, 256, FRAME_HW + (3,)).astype(np.uint8)
    s = []
    for _ in range(3):
        t = time.perf_counter()
        x = _host_resize(frame.astype(np.float32) / np.float32(255.), 1, scale)
        if mode == br.SAME:
            x = _host_resize(x, scale, 1)
        ref_bytes = np.clip(np.round(255. * x.astype(np.float64)), 0, 255).astype(np.uint8)
        s.append((time.perf_counter() - t) * 1e3)
    res['host_ref_ms_per_frame'] = round(median(s), 2)
    res['host_ref_differs_from_model'] = int((ref_bytes != br.degrade_frame(frame, scale, mode)).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--size', type=int, default=192)
    ap.add_argument('--scale', type=int, default=2, choices=(2, 4))
    ap.add_argument('--mode', default='same', choices=('same', 'down'))
    ap.add_argument('--rounds', type=int, default=7, help='alternating samples per path (at least five)')
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--timeout', type=float, default=300.0)
    ap.add_argument('--child', action='store_true', help='(internal) measure in this process')
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error('--rounds: at least five')
    if a.child:
        print(json.dumps(measure(a.batch, a.frames, a.size, a.scale, a.mode, a.rounds, a.inner)))
        return 0
    res = {'metric': 'degrade_step', 'batch': a.batch, 'frames': a.frames, 'size': a.size, 'scale': a.scale, 'mode': a.mode,
           'rounds': a.rounds, 'inner': a.inner, 'stream_tbps': 6.3}
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--batch', str(a.batch), '--frames', str(a.frames), '--size', str(a.size),
           '--scale', str(a.scale), '--mode', a.mode, '--rounds', str(a.rounds), '--inner', str(a.inner)]
    rc = 0
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.timeout, universal_newlines=True)
        if p.returncode != 0:
            res['failed'], rc = 'exit %d: %s' % (p.returncode, ' | '.join(p.stderr.strip().splitlines()[-3:])), 1
        else:
            res.update(json.loads(p.stdout.strip().splitlines()[-1]))
    except subprocess.TimeoutExpired:
        res['failed'], rc = 'no result within %g s' % a.timeout, 1
    print(json.dumps(res))
    return rc


if __name__ == '__main__':
    sys.exit(main())
