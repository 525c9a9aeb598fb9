"""One scan in a process of its own: `python -m tests.dense_hits_child <out.npz>`, for tests/test_gpu_dense_hits.py.

FGPU_REFRESH_DIV is read once per process, so the test that wants the walk to make its windows' planes again (walk_register's look-up over
the words of a window, w_first > 0, in front of the link pass) starts this child with the knob in its environment.  Windows of 5 000 positions on 6 000 reads in two
batches: some hundred windows that begin inside words.  The blob holds the map, the counters, fgpu_diag_prepared_refresh and the launch counts."""
import json
import sys

import numpy as np

from faucet_amd import _lib as L
from faucet_amd import api
from oracle import pyoracle as po
from tests.test_gpu_parity import _random_case, chunks


def workload():
    k = 25
    bases, offs = _random_case(6000, 100, k, 20_000, 0.012, 555, 0.002, 3)
    tai, nh = api.load_filter_shape(600_000, 120_000)
    return bases, offs, k, tai, nh


def run(out):
    bases, offs, k, tai, nh = workload()
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    po.load_two_filters(b1, b2, bases, offs, k)
    ctx = api.Context(k, tai, nh, profile=True, walk_window_span=5000)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 2))
    keys, recs = sc.junctions()
    np.savez(out, keys=keys, recs=recs, scan_stats=json.dumps(sst), prepared_refresh=json.dumps(ctx.diag_prepared_refresh()),
             kernel_times=json.dumps(ctx.kernel_times()))
    ctx.close()


if __name__ == "__main__":
    run(sys.argv[1])
