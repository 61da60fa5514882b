#!/usr/bin/env python
"""One JSON line for the input side of a training step: packed uint8 crops assembled on the device (realvsr_amd.data) against the
reference's host chain, at --batch x --frames x --size^2 x 3, all-pair (LQ + GT), frames from tests/batch_reference.py's formula held in
host memory as uint8.

  host_ref_ms      the reference's per-batch tail restated in numpy, in-process, single thread: per frame astype(float32) / 255 on the
                   WHOLE 1024 x 512 x 3 frame (data/util.py:95), crop, util.augment, stack, [2, 1, 0], transpose, ascontiguousarray,
                   from_numpy; the collate stack; .to(device); synchronise
  host_packed_ms   ClipBatchStager: stage the crops into pinned memory, upload, the two kernel launches, synchronise
  h2d_bytes_ref / h2d_bytes_packed   bytes each path copies to the device, from the shapes
  assemble_ms      rvsr_assemble_clips alone on the LQ tensor (device events, warmed), and
  composed_ms      the same tensor from torch operators on the device (u8.float() / 255 as a true division, flips, permute, contiguous), the two timed
                   ALTERNATING, --rounds samples each; *_min_max give the spread
  assemble_tbps    (uint8 in + f32 out) bytes over assemble_ms, next to the ~6.3 TB/s a stream reaches on MI355X
  val_*            the kernel numbers again for the validation shape (50 x 512 x 1024 x 3, flags = None)
The measurements run in a child process under --timeout; if it fails nothing further is started on the GPU and the line says so.

usage: python tools/input_step.py [--batch B] [--frames N] [--size S] [--rounds R] [--inner K] [--timeout S]
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

from step_timing import event_ms, median  # noqa: E402


def _composed(u8, flags_host, out=None):
    """The kernel's result from torch operators: [B, F, H, W, C] uint8 -> [B, F, C, H, W] float32, per-sample flips."""
    import torch
    # (a [1] tensor as the divisor: torch evaluates `tensor / python scalar` on the device as a multiplication by the reciprocal, which
    # is not the correctly rounded quotient for every byte value)
    x = u8.float() / torch.full((1,), 255., device=u8.device)
    res = []
    for b, f in enumerate(flags_host):
        a = x[b]
        if f & 2:
            a = a.flip(1)
        if f & 1:
            a = a.flip(2)
        if f & 4:
            a = a.transpose(1, 2)
        res.append(a.flip(3).permute(0, 3, 1, 2))
    return torch.stack(res).contiguous()


def _alternate(fused, composed, rounds, inner):
    for _ in range(3):
        fused()
        composed()
    a, b = [], []
    for _ in range(rounds):
        a.append(event_ms(fused, inner))
        b.append(event_ms(composed, max(1, inner // 4)))
    return a, b


def measure(B, N, S, rounds, inner):
    import random
    import numpy as np
    import torch
    import batch_reference as ref
    from realvsr_amd import data
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    d = torch.device('cuda', 0)
    opt = {'interval_list': [1], 'random_reverse': False, 'N_frames': N, 'GT_size': S, 'LQ_size': S, 'border_mode': False,
           'phase': 'train', 'use_flip': True, 'use_rot': True}
    random.seed(17)
    plans = [data.draw_sample(opt, '%03d_%05d' % (i % 4, 10 + i % 30)) for i in range(B)]
    frames = [([ref.frame('LQ', p['name_a'], v) for v in p['neighbor_list']], [ref.frame('GT', p['name_a'], v) for v in p['neighbor_list']])
              for p in plans]
    res = {}

    def host_ref():
        samples = []
        for p, (lq, gt) in zip(plans, frames):
            h, w, f = p['rnd_h'], p['rnd_w'], p['flags']
            imgs = [x.astype(np.float32) / 255. for x in lq + gt]
            imgs = [x[h:h + S, w:w + S, :] for x in imgs]

            def aug(img):
                if f & 1:
                    img = img[:, ::-1, :]
                if f & 2:
                    img = img[::-1, :, :]
                if f & 4:
                    img = img.transpose(1, 0, 2)
                return img
            imgs = [aug(x) for x in imgs]
            pair = []
            for part in (imgs[:N], imgs[N:]):
                st = np.stack(part, axis=0)[:, :, :, [2, 1, 0]]
                pair.append(torch.from_numpy(np.ascontiguousarray(np.transpose(st, (0, 3, 1, 2)))).float())
            samples.append(pair)
        lqs, gts = torch.stack([s[0] for s in samples]), torch.stack([s[1] for s in samples])
        out = lqs.to(d), gts.to(d)
        torch.cuda.synchronize()
        return out

    stager = data.ClipBatchStager(B, N, N, S, 3, pin=True, slots=2)

    def host_packed():
        for i, (p, (lq, gt)) in enumerate(zip(plans, frames)):
            stager.stage(i, lq, gt, p)
        lq, gt, flags = stager.upload()
        out = data.assemble_batch(lq, flags), data.assemble_batch(gt, flags)
        torch.cuda.synchronize()
        return out

    want, got = host_ref(), host_packed()
    res['paths_equal'] = bool(torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]))
    for name, fn in (('host_ref', host_ref), ('host_packed', host_packed)):
        s = []
        for _ in range(max(3, rounds)):
            t = time.perf_counter()
            fn()
            s.append((time.perf_counter() - t) * 1e3)
        res[name + '_ms'] = round(median(s), 3)
        res[name + '_ms_min_max'] = [round(min(s), 3), round(max(s), 3)]
    res['h2d_bytes_ref'] = 2 * B * N * 3 * S * S * 4
    res['h2d_bytes_packed'] = 2 * B * N * 3 * S * S + 4 * B

    def kernel_numbers(prefix, u8, flags, flags_host):
        out = torch.empty(u8.shape[0], u8.shape[1], u8.shape[4], u8.shape[2], u8.shape[3], device=d)
        res[prefix + 'composed_equal'] = bool(torch.equal(data.assemble_batch(u8, flags), _composed(u8, flags_host)))
        res[prefix + 'composed_scalar_div_equal'] = bool(torch.equal(data.assemble_batch(u8, None, 0), u8.float().div(255.).permute(0, 1, 4, 2, 3)))
        a, b = _alternate(lambda: data.assemble_batch(u8, flags, out=out), lambda: _composed(u8, flags_host), rounds, inner)
        res[prefix + 'assemble_ms'], res[prefix + 'assemble_ms_min_max'] = round(median(a), 5), [round(min(a), 5), round(max(a), 5)]
        res[prefix + 'composed_ms'], res[prefix + 'composed_ms_min_max'] = round(median(b), 5), [round(min(b), 5), round(max(b), 5)]
        res[prefix + 'assemble_tbps'] = round(u8.numel() * 5 / (median(a) * 1e-3) / 1e12, 3)
        res[prefix + 'fused_below_composed_by_more_than_the_spread'] = bool(max(a) < min(b))

    lq, _, flags = stager._views(stager._dev[0])
    kernel_numbers('', lq, flags, [p['flags'] for p in plans])
    g = torch.Generator(device='cuda').manual_seed(3)
    val = torch.randint(0, 256, (1, 50, 512, 1024, 3), device=d, generator=g, dtype=torch.uint8)
    kernel_numbers('val_', val, None, [0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--size', type=int, default=192)
    ap.add_argument('--rounds', type=int, default=7, help='alternating samples per path (at least five)')
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--timeout', type=float, default=300.0)
    ap.add_argument('--child', action='store_true', help='(internal) measure in this process')
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error('--rounds: at least five')
    if a.child:
        print(json.dumps(measure(a.batch, a.frames, a.size, a.rounds, a.inner)))
        return 0
    res = {'metric': 'input_step', 'batch': a.batch, 'frames': a.frames, 'size': a.size, 'rounds': a.rounds, 'inner': a.inner,
           'stream_tbps': 6.3}
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--batch', str(a.batch), '--frames', str(a.frames), '--size', str(a.size),
           '--rounds', str(a.rounds), '--inner', str(a.inner)]
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
