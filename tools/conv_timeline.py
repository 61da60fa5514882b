"""s_memtime timeline of conv_fwd5_kernel (workgroup 77: thread 0 over the last 8 stages, every wave at stages Q - 7 .. Q - 3) at the L1
shape.  Build the variant, then run against it:
   tools/build_variant.sh tl conv2_kernels.hip -DRVSR_TIMELINE ; RVSR_SO=$PWD/realvsr_amd/csrc/librealvsr_tl.so python tools/conv_timeline.py"""
import ctypes, os, sys, torch, torch.nn as nn
sys.path.insert(0, os.getcwd())
from realvsr_amd import functional as RF
# enum Fwd5Stamp of csrc/conv2_kernels.hip
F5_STAGE, F5_KERNEL_START, F5_KERNEL_END, F5_Q3_LOOP_END, F5_Q4_BARRIER, F5_Q4_LOOP_END, F5_Q6 = 0, 60, 61, 70, 80, 90, 300
dev = torch.device('cuda:0')
conv = nn.Conv2d(64, 64, 3, 1, 1).to(dev)
x = torch.randn(40, 64, 180, 320, device=dev)
for _ in range(3):
    y = RF.conv2d(x, conv, RF.ACT_LRELU)
torch.cuda.synchronize()
L = ctypes.CDLL(os.environ['RVSR_SO'])
buf = (ctypes.c_ulonglong * 512)()
print('rc', L.rvsr_timeline_read(buf, 512))
t = list(buf)
print('workgroup 77: kernel start -> end %d ticks' % (t[F5_KERNEL_END] - t[F5_KERNEL_START]))
print('stage Q-3 per wave: loop time after the common barrier release:', [int(t[F5_Q3_LOOP_END + w] - t[F5_Q4_BARRIER + w]) for w in range(8)])
print('stage Q-4 loop-end skew per wave:', [int(t[F5_Q4_LOOP_END + w] - min(t[F5_Q4_LOOP_END:F5_Q4_LOOP_END + 8])) for w in range(8)])
t0 = min(t[F5_Q6 + w * 12 + 11] for w in range(8))
print('stage Q-6, ticks since the first wave left the previous barrier; per wave: barrier passed | start of taps 0..8 | loop end | next barrier passed')
for w in range(8):
    r = [int(t[F5_Q6 + w * 12 + i] - t0) for i in (11, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)]
    print('  wave %d:' % w, r, ' per tap:', [r[i + 1] - r[i] for i in range(1, 10)])
# the last 8 stages of thread 0, in time order (slot q & 7 holds stage q)
names = {}
for sl in range(8):
    names[F5_STAGE + 3 * sl + 1] = 'slot%d start' % sl
    names[F5_STAGE + 3 * sl + 2] = 'slot%d mfma + staging slices done' % sl
    names[F5_STAGE + 3 * sl + 3] = 'slot%d barrier passed' % sl
order = sorted(names, key=lambda i: t[i])
prev = t[order[0]]
for i in order:
    print('%-36s +%7d' % (names[i], t[i] - prev))
    prev = t[i]
