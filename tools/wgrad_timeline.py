"""s_memtime timeline of conv_wgrad2_kernel (workgroup (77, 0, 0): thread 0 over the first six tiles and from the end of the tile loop to the
end of the kernel -- the partial sums --, every wave at tile 3) at the L1 shape.
Build the variant, then run against it:
   tools/build_variant.sh tl conv2_kernels.hip -DRVSR_TIMELINE ; RVSR_SO=$PWD/realvsr_amd/csrc/librealvsr_tl.so python tools/wgrad_timeline.py"""
import ctypes, os, sys, torch, torch.nn as nn
sys.path.insert(0, os.getcwd())
from realvsr_amd import functional as RF
WG2_T3_KSTEP, WG2_TILE, WG2_LOOP_END, WG2_KERNEL_END = 120, 200, 230, 231   # enum Wgrad2Stamp of csrc/conv2_kernels.hip
dev = torch.device('cuda:0')
conv = nn.Conv2d(64, 64, 3, 1, 1).to(dev)
x = torch.randn(40, 64, 180, 320, device=dev)
for _ in range(3):
    conv.weight.grad = None
    y = RF.conv2d(x, conv, RF.ACT_LRELU)
    y.backward(torch.randn_like(y))
torch.cuda.synchronize()
L = ctypes.CDLL(os.environ['RVSR_SO'])
buf = (ctypes.c_ulonglong * 512)()
print('rc', L.rvsr_timeline_read(buf, 512))
t = list(buf)
for ti in range(6):
    s = t[WG2_TILE + 4 * ti:WG2_TILE + 4 * ti + 4]
    nxt = t[WG2_TILE + 4 * (ti + 1)] if ti < 5 else None
    print('tile %d: commit %6d | barrier %6d | MFMA phase (+ next tile\'s loads) %6d | closing barrier %s' %
          (ti, s[1] - s[0], s[2] - s[1], s[3] - s[2], (nxt - s[3]) if nxt else '-'))
print('tile 0 top -> end of the tile loop %d | partial sums + bias partials (loop end -> kernel end) %d' %
      (t[WG2_LOOP_END] - t[WG2_TILE], t[WG2_KERNEL_END] - t[WG2_LOOP_END]))
t0 = min(t[WG2_T3_KSTEP + w * 10] for w in range(8))
print('tile 3, per wave: start of k-steps 0..7 | loop end (ticks since the first wave entered the loop); per k-step')
for w in range(8):
    r = [int(t[WG2_T3_KSTEP + w * 10 + i] - t0) for i in range(9)]
    print('  wave %d:' % w, r, [r[i + 1] - r[i] for i in range(8)])
