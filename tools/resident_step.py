#!/usr/bin/env python
"""One JSON line for the resident training set (realvsr_amd.resident): a batch gathered from frames that stay in HBM against what the
project could do before, at --batch x --frames x --size^2 x 3 out of 1024 x 512 x 3 frames, one side (LQ; the GT side is a second,
identical launch).

  gather_ms        rvsr_gather_clips from a store of --store-frames random frames, driven by a [batch, frames + 3] table
  composed_ms      the same tensor from what the project had on the device: index_select of the batch's frames, the per-sample slice,
                   contiguous(), then rvsr_assemble_clips
  assemble_ms      rvsr_assemble_clips alone on the crops already packed contiguously (the file loader's launch): the same bytes read
                   from rows --size * 3 bytes long at their own pitch instead of the frame's 1536
                   The three are timed ALTERNATING with device events, --rounds samples each, the medians reported, *_min_max the
                   spread; every launch uses the next of --tables tables (other slots, origins and flags), so that a launch does not
                   find its crops in a cache the launch before it filled.  *_equal: the three tensors are the same bits.
  gather_tbps      (uint8 crop bytes in + f32 bytes out) over gather_ms, next to the ~6.3 TB/s a stream reaches on MI355X
  gather_over_assemble   gather_ms / assemble_ms
  table_h2d_bytes  what a batch sends to the device per side: the table
  png_decode_ms_per_frame           data._read_png_u8 of one 1024 x 512 x 3 file of noise on one core of this host (the file loader
                                    does 2 * batch * frames of these per batch); png_decode_smooth_ms_per_frame: a formula frame
  store_load_s_per_1000_frames      DeviceFrameStore.from_dataset on a tree of --load-frames such files in --workers workers, scaled
The measurements run in a child process under --timeout; if it fails nothing further is started on the GPU and the line says so.

usage: python tools/resident_step.py [--batch B] [--frames N] [--size S] [--store-frames K] [--tables T] [--rounds R] [--inner I]
                                     [--load-frames L] [--workers W] [--timeout S]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from step_timing import event_ms, median  # noqa: E402

H, W, C = 1024, 512, 3


def _host_numbers(res, load_frames, workers, device='cuda'):
    """The PNG decode on one core, and a store loaded from a tree of whole-size files."""
    import numpy as np
    import torch
    from PIL import Image
    import batch_reference as ref
    import resident_reference as rref
    from realvsr_amd import data, resident
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.RandomState(1)
        for name, frame in (('noise', rng.randint(0, 256, size=(H, W, C)).astype(np.uint8)), ('smooth', ref.frame('LQ', 3, 7))):
            path = os.path.join(tmp, name + '.png')
            Image.fromarray(np.ascontiguousarray(frame), 'RGB').save(path)
            s = []
            for _ in range(7):
                t = time.perf_counter()
                np.ascontiguousarray(data._read_png_u8(path))
                s.append((time.perf_counter() - t) * 1e3)
            res['png_decode_ms_per_frame' if name == 'noise' else 'png_decode_smooth_ms_per_frame'] = round(median(s), 3)
        per_seq = 50
        sequences = tuple('%03d' % i for i in range(max(1, load_frames // per_seq)))
        tree = os.path.join(tmp, 'tree')
        os.makedirs(tree)
        rref.write_tree(tree, sequences, per_seq, (H, W))
        ds = data.RealVSRAllPairDataset(rref.tree_opt(tree, (H, W), GT_size=192, LQ_size=192))
        store = resident.DeviceFrameStore.from_dataset(ds, 'LQ', device=device, n_workers=workers)
        res['store_load_frames'], res['store_load_workers'] = len(store), workers
        res['store_load_s_per_1000_frames'] = round(store.load_seconds * 1000 / len(store), 3)
        slot = store.index[sequences[-1], 17]
        res['store_load_equal'] = bool(torch.equal(store.frames[slot].cpu(), torch.from_numpy(
            np.ascontiguousarray(data._read_png_u8(os.path.join(tree, 'LQ', sequences[-1], '00017.png'))))))
        del store


def measure(a):
    import torch
    from realvsr_amd import data, resident
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    d = torch.device('cuda', 0)
    B, N, S, K = a.batch, a.frames, a.size, a.store_frames
    res = {}
    _host_numbers(res, a.load_frames, a.workers)

    g = torch.Generator(device='cuda').manual_seed(3)
    frames = torch.empty(K, H, W, C, dtype=torch.uint8, device=d)
    for k in range(0, K, 50):
        frames[k:k + 50] = torch.randint(0, 256, frames[k:k + 50].shape, device=d, generator=g, dtype=torch.uint8)
    store = resident.DeviceFrameStore(frames, {('s', i): i for i in range(K)})
    res['store_bytes'] = store.nbytes

    cpu = torch.Generator().manual_seed(4)
    tables, crops, index, origins = [], [], [], []
    for _ in range(a.tables):
        first = torch.randint(0, K - N + 1, (B, 1), generator=cpu)
        t = torch.cat([first + torch.arange(N)[None], torch.randint(0, H - S + 1, (B, 1), generator=cpu),
                       torch.randint(0, W - S + 1, (B, 1), generator=cpu), torch.randint(0, 8, (B, 1), generator=cpu)], dim=1).int()
        tables.append(t.to(d))
        index.append(t[:, :N].reshape(-1).long().to(d))
        origins.append([(int(r[N]), int(r[N + 1])) for r in t])
        crops.append(torch.stack([frames[t[b, :N].long().to(d), h:h + S, w:w + S] for b, (h, w) in enumerate(origins[-1])]).contiguous())
    flags = [t[:, N + 2].contiguous() for t in tables]
    out = torch.empty(B, N, C, S, S, device=d)
    turn = {'gather': 0, 'composed': 0, 'assemble': 0}

    def nxt(name):
        turn[name] = (turn[name] + 1) % a.tables
        return turn[name]

    def gather(k=None):
        k = nxt('gather') if k is None else k
        return resident.gather_batch(store, tables[k], N, S, out=out)

    def composed(k=None):
        k = nxt('composed') if k is None else k
        picked = frames.index_select(0, index[k]).view(B, N, H, W, C)
        packed = torch.stack([picked[b, :, h:h + S, w:w + S] for b, (h, w) in enumerate(origins[k])]).contiguous()
        return data.assemble_batch(packed, flags[k], out=out)

    def assemble(k=None):
        k = nxt('assemble') if k is None else k
        return data.assemble_batch(crops[k], flags[k], out=out)

    want = gather(1).clone()
    res['composed_equal'] = bool(torch.equal(composed(1), want))
    res['assemble_equal'] = bool(torch.equal(assemble(1), want))
    for _ in range(3):
        gather(), composed(), assemble()
    s = {'gather': [], 'composed': [], 'assemble': []}
    for _ in range(a.rounds):
        s['gather'].append(event_ms(gather, a.inner))
        s['composed'].append(event_ms(composed, max(1, a.inner // 4)))
        s['assemble'].append(event_ms(assemble, a.inner))
    for name, v in s.items():
        res[name + '_ms'], res[name + '_ms_min_max'] = round(median(v), 5), [round(min(v), 5), round(max(v), 5)]
    res['gather_tbps'] = round(B * N * S * S * C * 5 / (median(s['gather']) * 1e-3) / 1e12, 3)
    res['gather_over_assemble'] = round(median(s['gather']) / median(s['assemble']), 3)
    res['gather_below_composed_by_more_than_the_spread'] = bool(max(s['gather']) < min(s['composed']))
    res['table_h2d_bytes'] = B * (N + 3) * 4
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--size', type=int, default=192)
    ap.add_argument('--store-frames', type=int, default=600, help='frames of the timed store (1.5 MiB each)')
    ap.add_argument('--tables', type=int, default=32, help='tables the timed launches rotate through')
    ap.add_argument('--rounds', type=int, default=7, help='alternating samples per path (at least five)')
    ap.add_argument('--inner', type=int, default=256)
    ap.add_argument('--load-frames', type=int, default=100, help='PNG files of the timed store load (a multiple of 50)')
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--timeout', type=float, default=420.0)
    ap.add_argument('--child', action='store_true', help='(internal) measure in this process')
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error('--rounds: at least five')
    if a.child:
        print(json.dumps(measure(a)))
        return 0
    res = {'metric': 'resident_step', 'frame_hwc': [H, W, C], 'stream_tbps': 6.3}
    keys = ('batch', 'frames', 'size', 'store_frames', 'tables', 'rounds', 'inner', 'load_frames', 'workers')
    res.update((k, getattr(a, k)) for k in keys)
    cmd = [sys.executable, os.path.abspath(__file__), '--child']
    for k in keys:
        cmd += ['--' + k.replace('_', '-'), str(getattr(a, k))]
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
