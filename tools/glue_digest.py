#!/usr/bin/env python
"""SHA-256 of the outputs and gradients of the glue operators, one child process per source tree, to show that a change to their kernels
moved no bit (profiles/r12_notes.md section 4).

    python tools/glue_digest.py TREE [TREE ...]        # each TREE: a checkout with realvsr_amd/csrc/librealvsr_hip.so built

Every tree runs the same seeded random inputs (values, not integers: a changed association or a changed fused multiply-add shows) through
realvsr_amd.functional: upsample_bilinear x2, maxavgpool, pyr_down, pyr_updiff and conv_cat_bcast, forward and backward, at the small
shapes of tests/test_gpu_glue_vector.py / tests/test_gpu_conv_addend.py plus one training-size shape each.  Prints one line per digest
and, with two or more trees, the names that differ from the first tree's (the expectation: none)."""
import hashlib
import json
import os
import subprocess
import sys


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def _holder(torch, Co, Ci, gen):
    conv = torch.nn.Conv2d(Ci, Co, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * 0.05)
        conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen) * 0.1)
    return conv.cuda()


def run_child():
    import torch
    sys.path.insert(0, os.getcwd())
    from realvsr_amd import functional as RF
    d = torch.device('cuda', 0)
    out = {}

    def case(name, op, shapes, seed):
        gen = torch.Generator().manual_seed(seed)
        xs = [torch.randn(s, generator=gen).to(d).requires_grad_(True) for s in shapes]
        y = op(*xs)
        g = torch.randn(y.shape, generator=gen).to(d)
        y.backward(g)
        out[name + ' out'] = _digest(y)
        for i, x in enumerate(xs):
            out['%s grad%d' % (name, i)] = _digest(x.grad)

    for s in [(1, 1, 1, 4), (1, 2, 2, 4), (2, 3, 3, 8), (1, 2, 5, 12), (1, 2, 4, 6), (40, 64, 90, 160)]:
        for scale in (1.0, 2.0):
            case('upsample2 %s x%g' % (s, scale), lambda x: RF.upsample_bilinear(x, 2, scale), [s], 1)
    for s in [(1, 1, 2, 4), (1, 2, 3, 8), (2, 3, 7, 8), (1, 2, 8, 12), (1, 2, 5, 16), (8, 64, 180, 320)]:
        case('maxavgpool %s' % (s,), RF.maxavgpool, [s], 2)
    for s in [(2, 3, 6, 8), (2, 3, 8, 8), (1, 2, 12, 20), (2, 3, 5, 5), (2, 3, 7, 12), (1, 2, 13, 21), (8, 1, 720, 1280)]:
        case('pyr_down %s' % (s,), RF.pyr_down, [s], 3)
    for s in [(2, 3, 6, 8), (2, 3, 8, 8), (1, 2, 12, 20), (2, 3, 4, 4), (2, 3, 8, 6), (8, 1, 720, 1280)]:
        case('pyr_updiff %s' % (s,), RF.pyr_updiff, [s, s[:2] + (s[2] // 2, s[3] // 2)], 4)
    for (N, B, C, H, W), act in [((3, 2, 64, 8, 64), RF.ACT_LRELU), ((3, 2, 64, 16, 128), RF.ACT_RELU), ((3, 2, 64, 9, 64), RF.ACT_NONE),
                                 ((5, 8, 64, 180, 320), RF.ACT_LRELU)]:
        gen = torch.Generator().manual_seed(5)
        conv = _holder(torch, C, 2 * C, gen)
        x = torch.randn(N * B, C, H, W, generator=gen).to(d).requires_grad_(True)
        ref = torch.randn(B, C, H, W, generator=gen).to(d).requires_grad_(True)
        y = RF.conv_cat_bcast(x, ref, conv, N, act, 0.1)
        y.backward(torch.randn(y.shape, generator=gen).to(d))
        name = 'conv_cat_bcast %s act %d' % ((N, B, C, H, W), act)
        for k, t in (('out', y), ('gx', x.grad), ('gref', ref.grad), ('gw', conv.weight.grad), ('gb', conv.bias.grad)):
            out['%s %s' % (name, k)] = _digest(t)
        del x, ref, y
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print('DIGESTS ' + json.dumps(out), flush=True)


def main(trees):
    tables = []
    for tree in trees:
        env = dict(os.environ, PYTHONPATH=tree)
        env.pop('RVSR_SO', None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], cwd=tree, env=env, stdout=subprocess.PIPE, text=True, timeout=300)
        lines = [l for l in r.stdout.splitlines() if l.startswith('DIGESTS ')]
        if r.returncode != 0 or not lines:
            print(r.stdout[-2000:])
            raise SystemExit('%s: child exited with %d' % (tree, r.returncode))
        tables.append(json.loads(lines[-1][8:]))
    for name in tables[0]:
        print('%-60s %s' % (name, '  '.join(t.get(name, '-') for t in tables)))
    unequal = [n for n in tables[0] if any(t.get(n) != tables[0][n] for t in tables[1:])]
    print('%d digests per tree, %d unequal%s' % (len(tables[0]), len(unequal), ''.join('\n  ' + n for n in unequal)))
    return 1 if unequal else 0


if __name__ == '__main__':
    if sys.argv[1:] == ['--child']:
        run_child()
    else:
        sys.exit(main(sys.argv[1:] or ['.']))
