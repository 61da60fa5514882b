"""s_memtime timeline of one dcn_fwd3_kernel workgroup (thread 0 of workgroup 77 of batch element 1) at the L1 shape.
   tools/build_variant.sh tl3 dcn3_kernels.hip -DRVSR_TIMELINE ; RVSR_SO=$PWD/realvsr_amd/csrc/librealvsr_tl3.so python tools/dcn3_timeline.py [ostd]"""
import ctypes, os, sys, torch
sys.path.insert(0, os.getcwd())
from realvsr_amd import functional as RF
F3_START, F3_CHUNK, F3_EPILOGUE, F3_C1_TAP_END, F3_C1_TAP = 0, 0, 30, 40, 60   # enum Fwd3Stamp of csrc/dcn3_kernels.hip
dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(0)
ostd = float(sys.argv[1]) if len(sys.argv) > 1 else 0.1
x = torch.randn(40, 64, 180, 320, generator=g).to(dev)
om = torch.randn(40, 216, 180, 320, generator=g); om[:, :144] *= ostd; om = om.to(dev)
w = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(dev); b = torch.zeros(64, device=dev)
for _ in range(3):
    out = RF.dcn_pack(x, om, w, b, 1, 1, 1, 8, RF.ACT_LRELU, 0.1)
torch.cuda.synchronize()
L = ctypes.CDLL(os.environ['RVSR_SO'])
buf = (ctypes.c_ulonglong * 256)()
print('rc', L.rvsr_timeline_read(buf, 256), 'offset std', ostd)
t = list(buf)
names = {F3_START: 'start'}
for c in range(4):
    names[F3_CHUNK + 6 * c + 1] = 'chunk%d loads issued' % c
    names[F3_CHUNK + 6 * c + 3] = 'chunk%d x tile in LDS' % c
    names[F3_CHUNK + 6 * c + 4] = 'chunk%d barrier1' % c
    names[F3_CHUNK + 6 * c + 5] = 'chunk%d 9 taps' % c
    names[F3_CHUNK + 6 * c + 6] = 'chunk%d barrier2' % c
names[F3_EPILOGUE] = 'epilogue'
prev = t[F3_START]
for i in sorted(names):
    print('%-30s +%7d  (t=%d)' % (names[i], t[i] - prev, t[i] - t[0]))
    prev = t[i]
print('chunk1 taps:', [t[F3_C1_TAP_END + k] - (t[F3_CHUNK + 6 + 4] if k == 0 else t[F3_C1_TAP_END + k - 1]) for k in range(9)])
print('chunk1, inside each tap (cycles): offsets consumed + geometry + corner reads issued | corner reads back | blend (+ far path) | split | fragment reads + MFMAs issued')
for k in range(9):
    a = [t[F3_C1_TAP + 5 * k + j] for j in range(4)] + [t[F3_C1_TAP_END + k]]
    print('  tap %d: %s' % (k, ' | '.join('%5d' % (a[j + 1] - a[j]) for j in range(4))), ' (tap start at t=%d)' % (a[0] - t[0]))
