"""BucketedGradAllReduce.zero_grad(passes=K): a step whose gradients are accumulated over several backward passes (the GAN stage's D step)
on two gloo ranks, CPU tensors, a toy of three Linear layers.  Both ranks run every scenario once (module fixture); the tests compare
what they sent back against float64 / against the plain arithmetic of a two-rank sum."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from rank_procs import run_ranks

WORLD = 2


def _toy(dtype=torch.float32):
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(6, 40), nn.Tanh(), nn.Linear(40, 40), nn.Tanh(), nn.Linear(40, 3)).to(dtype)


def _inputs(rank, dtype=torch.float32):
    g = torch.Generator().manual_seed(50 + rank)      # a different shard on every rank
    return torch.randn(5, 6, generator=g).to(dtype), torch.randn(5, 6, generator=g).to(dtype)


def _loss_a(net, x, rank):
    return net(x).square().mean() * (rank + 1)


def _loss_b(net, x, rank):
    return (net(x) * 0.3).sin().sum() * (2 - rank)


def _loss_head(net, x, rank):
    """Reaches the first Linear only: the other two layers receive no gradient in this pass."""
    return net[1](net[0](x)).square().sum() * (rank + 2)


def _grads(net):
    return torch.cat([p.grad.flatten() for p in net.parameters()]).clone()


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    from realvsr_amd.dist import BucketedGradAllReduce
    xa, xb = _inputs(rank)
    out = {}
    # the rank's own gradients, without a reducer
    net = _toy()
    _loss_a(net, xa, rank).backward()
    out['local_a'] = _grads(net).numpy()

    net = _toy()
    red = BucketedGradAllReduce(net.parameters(), bucket_mb=0.0002)
    out['buckets'] = len(red.buckets)
    for _ in range(2):          # twice: the pass count must be re-armed by every zero_grad
        red.zero_grad(passes=2)
        _loss_a(net, xa, rank).backward()
        out['issued_after_pass1'] = red.issued
        out['works_after_pass1'] = len(red._works)
        _loss_b(net, xb, rank).backward()
        out['issued_after_pass2'] = red.issued
        red.finish()
    out['two'] = _grads(net).numpy()
    out['two_stat'] = red.stats_issued_in_backward

    # the second pass reaches the first layer only
    red.zero_grad(passes=2)
    _loss_a(net, xa, rank).backward()
    _loss_head(net, xb, rank).backward()
    out['partial_issued_before_finish'] = red.issued
    red.finish()
    out['partial'] = _grads(net).numpy()

    # one pass: the argument spelled out, the default, and again after a two-pass step
    red.zero_grad(passes=1)
    _loss_a(net, xa, rank).backward()
    out['one_issued'] = red.issued
    red.finish()
    out['one'] = _grads(net).numpy()
    out['one_stat'] = red.stats_issued_in_backward
    red.zero_grad()
    _loss_a(net, xa, rank).backward()
    red.finish()
    out['default'] = _grads(net).numpy()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope='module')
def ranks():
    got = run_ranks(_worker, WORLD, limit=120)
    return {r: {k: (torch.from_numpy(v) if hasattr(v, 'dtype') else v) for k, v in d.items()} for r, d in got.items()}


def _ref64(second):
    """Mean over the ranks of the sum of both passes, float64."""
    total = 0
    for rank in range(WORLD):
        net = _toy(torch.float64)
        xa, xb = _inputs(rank, torch.float64)
        _loss_a(net, xa, rank).backward()
        second(net, xb, rank).backward()
        total = total + torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad).flatten() for p in net.parameters()])
    return total / WORLD


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def test_two_passes_issue_nothing_before_the_last_and_average_the_sum(ranks):
    ref = _ref64(_loss_b)
    for r in range(WORLD):
        d = ranks[r]
        assert d['buckets'] > 2
        assert d['issued_after_pass1'] == 0 and d['works_after_pass1'] == 0      # no collective before the final pass
        assert d['issued_after_pass2'] == d['buckets'] == d['two_stat']          # ... and all of them during it
        err = _rel(d['two'], ref)
        print('rank %d: two passes vs float64 mean of sums: rel l2 %.2e' % (r, err))
        assert err <= 1e-6
    assert torch.equal(ranks[0]['two'], ranks[1]['two'])


def test_parameter_with_one_gradient_in_two_passes_is_flushed_by_finish(ranks):
    ref = _ref64(_loss_head)
    for r in range(WORLD):
        d = ranks[r]
        # the buckets of the layers that the second pass did not reach never became ready in backward
        assert d['partial_issued_before_finish'] < d['buckets']
        err = _rel(d['partial'], ref)
        print('rank %d: one-pass parameters vs float64: rel l2 %.2e' % (r, err))
        assert err <= 1e-6
    assert torch.equal(ranks[0]['partial'], ranks[1]['partial'])


def test_one_pass_is_the_plain_reducer_bit_for_bit(ranks):
    # the reducer's arithmetic for one pass: the two-rank sum of the local gradients, times 1 / world, in float32
    want = (ranks[0]['local_a'] + ranks[1]['local_a']) * (1.0 / WORLD)
    for r in range(WORLD):
        d = ranks[r]
        assert torch.equal(d['one'], want) and torch.equal(d['default'], want)
        assert d['one_issued'] == d['buckets'] == d['one_stat']
