"""Start the rank processes of a multi-process test next to pytest and collect one result from each.

Every child gets a time limit; the first child that ends without having delivered its result, or with a non-zero exit code, ends the
wait for the others (they are terminated: nothing further is started after a failure)."""
import queue
import socket
import time

import torch.multiprocessing as mp


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_ranks(worker, world, args=(), limit=300):
    """worker(rank, world, port, q, *args) puts (rank, payload) into q once.  Returns {rank: payload}; asserts exit code 0 of every child."""
    assert world <= 2
    port = free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    got, deadline, failed = {}, time.monotonic() + limit, None
    try:
        while len(got) < world and failed is None:
            try:
                r, payload = q.get(timeout=0.5)
                got[r] = payload
                continue
            except queue.Empty:
                pass
            for r, p in enumerate(procs):
                if p.exitcode not in (None, 0) and r not in got:
                    failed = 'rank %d ended with exit code %s before delivering its result' % (r, p.exitcode)
            if time.monotonic() > deadline:
                failed = 'time limit of %d s' % limit
        if failed is None:
            for r, p in enumerate(procs):
                p.join(max(1.0, deadline - time.monotonic()))
                if p.exitcode != 0:
                    failed = 'rank %d: exit code %s' % (r, p.exitcode)
                    break
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
    assert failed is None, failed
    return got
