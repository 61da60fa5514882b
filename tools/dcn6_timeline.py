"""s_memtime timeline of one wave (wave 3 of workgroup 77) of dcn_bwdin6_kernel (batch element 1) and of dcn_bwdw6_kernel (third tile of its stream) at the L1 shape.
   tools/build_variant.sh tl6 dcn6_kernels.hip -DRVSR_TIMELINE ; RVSR_SO=$PWD/realvsr_amd/csrc/librealvsr_tl6.so python tools/dcn6_timeline.py [ostd]"""
import ctypes, os, sys, torch
sys.path.insert(0, os.getcwd())
from realvsr_amd import functional as RF
# enum Bwdin6Stamp / Bwdw6Stamp of csrc/dcn6_kernels.hip
BI6_PROLOGUE, BI6_END, BI6_CHUNK, BI6_C1_ITER, BI6_C1_MTILE, BW6_TILE, BW6_ITER = 0, 9, 10, 50, 90, 128, 138
ostd = float(sys.argv[1]) if len(sys.argv) > 1 else 1.25
dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(0)
x = torch.randn(8, 64, 180, 320, generator=g).to(dev).requires_grad_(True)
om = torch.randn(8, 216, 180, 320, generator=g); om[:, :144] *= ostd; om = om.to(dev).requires_grad_(True)
w = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(dev).requires_grad_(True); b = torch.zeros(64, device=dev, requires_grad=True)
gout = torch.randn(8, 64, 180, 320, generator=g).to(dev)
for _ in range(2):
    out = RF.dcn_pack(x, om, w, b, 1, 1, 1, 8, RF.ACT_LRELU, 0.1)
    out.backward(gout)
torch.cuda.synchronize()
L = ctypes.CDLL(os.environ['RVSR_SO'])
buf = (ctypes.c_ulonglong * 256)()
print('rc', L.rvsr_timeline_read(buf, 256))
t = list(buf)
names = {BI6_PROLOGUE: 'prologue done (gOut fragments, gOut^T emitted, window zeroed, chunk 0 requested)', BI6_END: 'kernel end'}
for c in range(4):
    names[BI6_CHUNK + 8 * c + 0] = 'chunk%d top' % c
    names[BI6_CHUNK + 8 * c + 1] = 'chunk%d x tile committed' % c
    names[BI6_CHUNK + 8 * c + 2] = 'chunk%d vmcnt(0)' % c
    names[BI6_CHUNK + 8 * c + 3] = 'chunk%d barrier' % c
    names[BI6_CHUNK + 8 * c + 4] = 'chunk%d lane iterations done' % c
    names[BI6_CHUNK + 8 * c + 5] = 'chunk%d barrier' % c
    names[BI6_CHUNK + 8 * c + 6] = 'chunk%d next requests issued' % c
    names[BI6_CHUNK + 8 * c + 7] = 'chunk%d flush done' % c
for it in range(5):
    names[BI6_C1_ITER + 4 * it] = '  chunk1 iteration %d start' % it
    names[BI6_C1_ITER + 4 * it + 1] = '  chunk1 iteration %d reads + math + atomics issued' % it
for mt in range(3):
    names[BI6_C1_MTILE + mt] = '  chunk1 M tile %d MFMAs issued' % mt
print('--- dcn_bwdin6')
prev = t[BI6_PROLOGUE]
for i in sorted(names, key=lambda i: t[i]):
    if t[i] == 0:
        continue
    print('%-84s +%7d  (t=%d)' % (names[i], t[i] - prev, t[i] - t[BI6_PROLOGUE]))
    prev = t[i]
print('--- dcn_bwdw6 (third tile of one stream)')
nm = dict((BW6_TILE + k, s) for k, s in enumerate(('tile top', 'vmcnt(0): operands + x landed', 'x committed + barrier', 'next requests set up',
                                                   'iterations done', 'end barrier')))
for it in range(5):
    nm[BW6_ITER + 4 * it] = '  iteration %d start' % it
    nm[BW6_ITER + 4 * it + 1] = '  iteration %d column values blended' % it
    nm[BW6_ITER + 4 * it + 2] = '  iteration %d split + transposer issued' % it
prev = t[BW6_TILE]
for i in sorted(nm, key=lambda i: t[i]):
    if t[i] == 0:
        continue
    print('%-84s +%7d  (t=%d)' % (nm[i], t[i] - prev, t[i] - t[BW6_TILE]))
    prev = t[i]
