"""bench.py on the host: the arrays `--dump-outputs` writes (names, dtypes, the seeded sample of a large output, the 64 MB budget) and the
options of a plain and a --full run.  No GPU: the model is a stand-in with the attributes bench.dump_outputs reads."""
import os
import subprocess
import sys
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO


@pytest.fixture(scope='module')
def bench():
    keep = os.environ.get('OMP_NUM_THREADS')
    import bench as b   # (sets a default OMP_NUM_THREADS for its CPU baseline: not for the processes the other tests start)
    if keep is None:
        os.environ.pop('OMP_NUM_THREADS', None)
    return b


def _model(n_out):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Conv2d(4, 2, 1, bias=False))
    for p in net.parameters():
        p.grad = torch.randn(p.shape)
    net[1].weight.grad = None                      # a parameter without a gradient dumps zeros
    terms = OrderedDict([('l_pix_y', torch.tensor(0.25)), ('l_pix_c', torch.tensor(0.5)), ('l_pix', torch.tensor(0.75))])
    return SimpleNamespace(netG=net, fake_H=torch.arange(n_out, dtype=torch.float32).reshape(1, 1, -1), loss_terms=terms)


def test_dump_outputs_writes_the_last_step(bench, tmp_path):
    m = _model(1000)
    bench.dump_outputs(m, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['grads.npy', 'l_pix.npy', 'l_pix_c.npy', 'l_pix_y.npy', 'output.npy']
    out = np.load(tmp_path / 'output.npy')
    assert out.dtype == np.float32 and np.array_equal(out, np.arange(1000, dtype=np.float32))
    ps = list(m.netG.parameters())
    want_g = torch.cat([ps[0].grad.reshape(-1), ps[1].grad.reshape(-1), torch.zeros(ps[2].numel())]).numpy()
    assert np.array_equal(np.load(tmp_path / 'grads.npy'), want_g)
    for k, v in (('l_pix_y', 0.25), ('l_pix_c', 0.5), ('l_pix', 0.75)):
        a = np.load(tmp_path / (k + '.npy'))
        assert a.dtype == np.float64 and a.tolist() == [v]


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(bench, tmp_path):
    n = bench.DUMP_SAMPLE + 12345
    for d in ('a', 'b'):
        bench.dump_outputs(_model(n), str(tmp_path / d))
    a, b = np.load(tmp_path / 'a' / 'output.npy'), np.load(tmp_path / 'b' / 'output.npy')
    assert a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)
    # fake_H[i] = i: the sample is a set of distinct ascending positions, spread over the whole output
    assert np.all(np.diff(a) > 0) and a[0] < 0.01 * n and a[-1] > 0.99 * n
    # two sampled arrays + the loss scalars stay within 64 MB
    assert 2 * bench.DUMP_SAMPLE * 4 + 3 * 8 < 64 * 2 ** 20


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for opt in ('--gpus', '--steps', '--warmup', '--full', '--dump-outputs'):
        assert opt in out.stdout
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--config', '5', '--dump-outputs', 'x'], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2 and '--dump-outputs' in out.stderr
