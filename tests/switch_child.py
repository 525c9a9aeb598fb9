"""One load and scan in a process of its own: `python -m tests.switch_child <workload> <out.npz>`.

Most FGPU_* switches are read once per process (function statics, a global set when the library loads), so tests/test_gpu_env_switches.py
starts one such child per setting, with the setting in the child's environment, and compares the blob written here with the oracle.  The
workloads are built from fixed seeds: the parent makes the same reads again for the oracle.  `<workload>` is a name of WORKLOADS, optionally
`+profile` (HIP events around every kernel; the blob then holds kernel_times()), or `repeats:<genome>:<copies>:<reads>` (the repeat set at
another size), or `delta_refresh` (the prepared-shard scenario, see delta_refresh()).  Nothing is printed."""
import json
import sys

import numpy as np

from faucet_amd import _lib as L
from faucet_amd import api, synth
from oracle import pyoracle as po
from tests.golden_util import Case
from tests.test_gpu_parity import _random_case, chunks

REPEATS = (3_000, 2, 1_200)      # genome length, copies of the 300-base repeat, reads of 100: see test_gpu_env_switches.test_the_repeat_set_...

# name -> how the reads are made and how they are run (E, S: what the filters are sized from; load / scan: batches; span 0: adaptive windows)
WORKLOADS = {
    "golden": dict(case="c1_k21", load=3, scan=2),
    "golden_mercy": dict(case="mercy_k21", load=3, scan=2),
    "clusters": dict(random=(20000, 110, 25, 50000, 0.012, 7, 0.002, 4), k=25, E=1_000_000, S=200_000, j=1, load=3, scan=3),
    "clusters_one": dict(random=(20000, 110, 25, 50000, 0.012, 7, 0.002, 4), k=25, E=1_000_000, S=200_000, j=1, load=1, scan=3),
    "tiny_genome": dict(random=(8000, 80, 15, 3000, 0.005, 1234 + 8000, 0.0, 2), k=15, E=300_000, S=60_000, j=0, load=3, scan=2),
    "repeats": dict(repeats=REPEATS, k=31, load=3, scan=3),
    "bits31": dict(random=(30000, 100, 31, 60000, 0.01, 2031 + 3, 0.001, 3), k=31, tai=1 << 31, nh=3, j=1, load=5, scan=3),
}


class Workload:
    """reads, filter shape and batching of one workload"""

    def __init__(self, name):
        name = name.split("+")[0]
        if name.startswith("repeats:"):
            w = dict(WORKLOADS["repeats"], repeats=tuple(int(v) for v in name.split(":")[1:]))
        else:
            w = WORKLOADS[name]
        self.case = None
        self.j, self.spacer, self.mercy = w.get("j", 1), 100, False
        if "case" in w:
            c = self.case = Case(w["case"])
            self.bases, self.offs = po.reads_from_lines(c.lines())
            self.k, self.j, self.spacer, self.mercy = c.k, c.j, c.spacer, c.mercy
            self.tai, self.nh = api.load_filter_shape(c.E, c.S, c.fp)
        elif "random" in w:
            self.bases, self.offs = _random_case(*w["random"])
            self.k = w["k"]
        else:
            G, copies, n_reads = w["repeats"]
            g = synth.make_genome(G, 91, repeats=copies, repeat_len=300)
            self.bases, self.offs = po.reads_from_matrix(synth.make_reads(g, n_reads, 100, 0.01, 92))
            self.k = w["k"]
            w = dict(w, E=G * 40 // 3, S=G * 10 // 3)      # (the proportions of the 150 kb set: E = 2 000 000, S = 500 000)
        if self.case is None:
            self.tai, self.nh = (w["tai"], w["nh"]) if "tai" in w else api.load_filter_shape(w["E"], w["S"])
        self.load_batches, self.scan_batches = w["load"], w["scan"]


def sparse(bits):
    """a filter as (indices of its nonzero bytes, those bytes): nothing is lost, and 2^31 bits stay small"""
    idx = np.flatnonzero(bits)
    return idx, bits[idx]


def run(name, out):
    w = Workload(name)
    ctx = api.Context(w.k, w.tai, w.nh, j=w.j, max_spacer_dist=w.spacer, mercy=w.mercy, profile="+profile" in name, walk_window_span=0)
    lst = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(w.bases, w.offs, w.load_batches))
    b1, b2 = ctx.bloom_download(L.BLOO1), ctx.bloom_download(L.BLOO2)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(w.bases, w.offs, w.scan_batches))
    keys, recs = sc.junctions()
    i1, v1 = sparse(b1)
    i2, v2 = sparse(b2)
    np.savez(out, bloo1_idx=i1, bloo1_val=v1, bloo2_idx=i2, bloo2_val=v2, bloom_bytes=np.int64(len(b2)), keys=keys, recs=recs,
             load_stats=json.dumps(lst), scan_stats=json.dumps(sst), ovw=json.dumps(ctx.diag_ovw()), replays=np.int64(ctx.diag_scan_replays()),
             kernel_times=json.dumps(ctx.kernel_times() if "+profile" in name else {}))
    ctx.close()


def delta_refresh(out):
    """The prepared-shard scenario of test_gpu_parity.test_a_fresher_preview_lets_the_walk_look_only_for_the_keys_created_since: shard A scans a
    third of the reads, B the next with A's table, C prepares the last third against an early preview of A's table, is shown A's final table,
    makes its planes again and walks when B's table arrives.  The blob holds C's map, counters and fgpu_diag_prepared_refresh."""
    import torch
    k, G = 21, 30_000
    bases, offs = _random_case(15_000, 100, k, G, 0.012, 911, 0.002, 3)
    tai, nh = api.load_filter_shape(20 * G, 4 * G)
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    po.load_two_filters(b1, b2, bases, offs, k)
    n = len(offs) - 1
    cut = [0, n // 3, 2 * n // 3, n]
    parts = [[api.ReadBatch(bases, offs[x:y + 1].copy()) for x, y in ((lo, (lo + hi) // 2), ((lo + hi) // 2, hi))] for lo, hi in zip(cut[:-1], cut[1:])]
    a, b, c = [api.Context(k, tai, nh) for _ in range(3)]
    for ctx in (a, b, c):
        ctx.bloom_upload(L.BLOO2, b2.bits())

    def export(ctx):
        m = ctx.table_entries()
        buf = torch.empty(max(m, 1) * L.TABLE_ENTRY_BYTES, dtype=torch.uint8, device="cuda")
        assert ctx.export_table(buf.data_ptr(), buf.numel()) == m
        torch.cuda.synchronize()
        return m, buf

    a.scan_begin()
    a.scan_batch(parts[0][0])
    n_early, early = export(a)
    a.scan_batch(parts[0][1])
    st_a = a.scan_end()
    n_a, t_a = export(a)
    b.scan_begin()
    b.import_table(t_a.data_ptr(), n_a, carried=st_a)
    for p in parts[1]:
        b.scan_batch(p)
    st_b = b.scan_end()
    n_b, t_b = export(b)
    c.scan_begin()
    c.import_hint(early.data_ptr(), n_early)
    for p in parts[2]:
        c.scan_prepare(p)
    c.import_hint(t_a.data_ptr(), n_a)
    c.scan_refresh_prepared()
    c.import_table(t_b.data_ptr(), n_b, carried=st_b)
    c.scan_walk_prepared()
    sst = c.scan_end()
    keys, recs = c.junctions()
    np.savez(out, keys=keys, recs=recs, scan_stats=json.dumps(sst), ovw=json.dumps(c.diag_ovw()), replays=np.int64(c.diag_scan_replays()),
             prepared_refresh=json.dumps(c.diag_prepared_refresh()), tables=np.array([n_early, n_a, n_b], dtype=np.int64))


if __name__ == "__main__":
    if sys.argv[1] == "delta_refresh":
        delta_refresh(sys.argv[2])
    else:
        run(sys.argv[1], sys.argv[2])
