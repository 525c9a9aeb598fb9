"""Pass 1 by filter slices (sharded.load_sliced, run_in_turn(protocol="slices")) on CPU: every rank loads the WHOLE stream into its slice of the
filters' bit positions, the ranks' fail planes are ORed, every rank sets its own bloo2 bits, the slices are gathered.  The backend here is a
TEST-ONLY stand-in with the method names of sharded.GpuShard: numpy bitmaps, a sequential walk over the k-mers in processing order.  What is
checked is the protocol -- which bits a rank may decide alone, what the OR of the planes means, what is gathered from where: filters and
to_bloo2 must equal the single-process oracle's, under gloo with 2 and 3 ranks and in turn with 4."""
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from faucet_amd import _lib as L
from faucet_amd import sharded
from oracle import pyoracle as po
from tests.golden_util import Case
from tests.test_sharded_gloo import OracleShard, _free_port

_SEG = re.compile(rb"[ACGT]+")
_positions_cache = {}


def kmer_positions(bases, offs, k, tai, nh):
    """per k-mer occurrence of the batch, in processing order (reads in file order, unambiguous segments left to right): its nh bit positions
    (hA + i hB) mod tai, the two hashes being the oracle's (that this IS where a pyoracle.Bloom puts a k-mer: test_positions_are_the_oracles)"""
    key = (bases.ctypes.data, offs.tobytes(), k, tai, nh)
    got = _positions_cache.get(key)
    if got is None:
        lib = po.lib()
        raw = bases.tobytes()
        got = []
        for a, z in zip(offs[:-1], offs[1:]):
            for m in _SEG.finditer(raw, int(a), int(z)):
                seg = m.group()
                for i in range(len(seg) - k + 1):
                    c = lib.fo_canon(lib.fo_encode(seg[i:i + k], k), k)
                    h_a, h_b = lib.fo_old_hash(c, 0, tai), lib.fo_old_hash(c, 1, tai)
                    got.append([(h_a + q * h_b) % tai for q in range(nh)])
        _positions_cache[key] = got
    return got


def test_positions_are_the_oracles():
    lib = po.lib()
    rng = np.random.default_rng(5)
    for k, tai, nh in ((21, 1 << 16, 3), (31, 1 << 14, 7), (5, 1 << 10, 1)):
        for x in rng.integers(0, 1 << (2 * k), size=40, dtype=np.uint64):
            c = lib.fo_canon(int(x), k)
            one = po.Bloom(tai, nh)
            one.add(c)
            want = set(np.flatnonzero(np.unpackbits(one.bits(), bitorder="little")).tolist())
            h_a, h_b = lib.fo_old_hash(c, 0, tai), lib.fo_old_hash(c, 1, tai)
            assert {(h_a + q * h_b) % tai for q in range(nh)} == want


class SliceShard(OracleShard):
    """OracleShard + the sliced pass: own bits [lo, hi) as one byte per bit, planes with one bit per k-mer occurrence of a batch"""

    def slice_load(self, batches, bit_lo, bit_hi):
        assert bit_lo % 512 == 0 and bit_hi % 512 == 0 and bit_lo <= bit_hi <= self.tai
        self.lo, self.hi = bit_lo, bit_hi
        self.own1 = bytearray(bit_hi - bit_lo)
        self.own2 = bytearray(bit_hi - bit_lo)
        self._stream, self._planes = [], []
        for bases, offs in batches:
            pos = kmer_positions(bases, offs, self.k, self.tai, self.nh)
            if not pos:
                continue
            fail = np.zeros(-(-len(pos) // 128) * 128, dtype=np.uint8)     # (padded: the planes travel in 16-byte granules)
            for t, hs in enumerate(pos):
                for h in hs:
                    if bit_lo <= h < bit_hi:
                        if not self.own1[h - bit_lo]:
                            fail[t] = 1               # one of MY bits was not set before this occurrence
                            self.own1[h - bit_lo] = 1
            self._stream.append(pos)
            self._planes.append(torch.from_numpy(np.packbits(fail, bitorder="little")))

    def slice_planes(self):
        return self._planes

    def slice_commit(self):
        self.to_bloo2 = self.kmers = 0
        for pos, plane in zip(self._stream, self._planes):
            fail = np.unpackbits(plane.numpy(), bitorder="little")
            for t, hs in enumerate(pos):
                self.kmers += 1
                if not fail[t]:                       # nobody failed it: the sequential run routes it to bloo2
                    self.to_bloo2 += 1
                    for h in hs:
                        if self.lo <= h < self.hi:
                            self.own2[h - self.lo] = 1

    def slice_end(self):
        for bloom, own in ((self.b1, self.own1), (self.b2, self.own2)):
            bloom.bits()[:] = 0
            bloom.bits()[self.lo // 8:self.hi // 8] = np.packbits(np.frombuffer(bytes(own), dtype=np.uint8), bitorder="little")
        return {"kmers": self.kmers, "to_bloo2": self.to_bloo2}


def _case(name):
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh, _, _ = po.sizing_from_cli(c.E, c.S, c.fp)
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    lst = po.load_two_filters(b1, b2, bases, offs, c.k)
    return c, bases, offs, tai, nh, b1, b2, lst


def _batches(bases, offs, n):
    cuts = np.linspace(0, len(offs) - 1, n + 1).astype(int)
    return [(bases, offs[a:z + 1].copy()) for a, z in zip(cuts[:-1], cuts[1:])]


def _worker(rank, world, port, name, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh, _, _ = po.sizing_from_cli(c.E, c.S, c.fp)
    be = SliceShard(c.k, tai, nh, c.j, c.spacer)
    st = sharded.load_sliced(be, _batches(bases, offs, 3), rank, world)
    np.save(os.path.join(out_dir, f"bloo1_{rank}.npy"), be.b1.bits().copy())
    np.save(os.path.join(out_dir, f"bloo2_{rank}.npy"), be.b2.bits().copy())
    np.save(os.path.join(out_dir, f"stats_{rank}.npy"), np.array([st["kmers"], st["to_bloo2"]]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name,world", [("c1_k21", 2), ("ragged_k31", 3), ("se_fp7_k21", 2), ("onehash_k25", 3)])
def test_load_sliced_under_gloo_equals_the_single_process_oracle(name, world, tmp_path):
    c, bases, offs, tai, nh, b1, b2, lst = _case(name)
    mp.spawn(_worker, args=(world, _free_port(), name, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):      # every rank ends with both global filters and the global counts
        assert np.array_equal(np.load(tmp_path / f"bloo1_{r}.npy"), b1.bits()), f"bloo1 on rank {r}"
        assert np.array_equal(np.load(tmp_path / f"bloo2_{r}.npy"), b2.bits()), f"bloo2 on rank {r}"
        assert list(np.load(tmp_path / f"stats_{r}.npy")) == [lst.kmers, lst.to_bloo2]
    assert np.array_equal(b2.bits(), c.bloom())      # ... which is the compiled reference's .bloom


@pytest.mark.parametrize("name", ["c1_k21", "ragged_k31", "twohash_k31_L150"])
def test_slices_in_turn_in_one_process_equal_the_sequential_run(name):
    """run_in_turn(protocol="slices") with 4 ranks: after_load once, with the last rank and the final filters; pass 2 goes on from them"""
    world = 4
    c, bases, offs, tai, nh, b1, b2, lst = _case(name)
    cuts = np.linspace(0, len(offs) - 1, world + 1).astype(int)
    shards = [_batches(bases, offs[cuts[r]:cuts[r + 1] + 1].copy(), 2) for r in range(world)]
    calls = []

    def after_load(r, stats, bloo1, bloo2):
        calls.append(r)
        assert np.array_equal(bloo1.numpy(), b1.bits()) and np.array_equal(bloo2.numpy(), b2.bits())
        assert (stats["kmers"], stats["to_bloo2"]) == (lst.kmers, lst.to_bloo2)

    load_stats, st, last = sharded.run_in_turn(lambda: SliceShard(c.k, tai, nh, c.j, c.spacer), shards, "slices", after_load)
    assert calls == [world - 1]
    assert len(load_stats) == world and all(s["to_bloo2"] == lst.to_bloo2 for s in load_stats)
    assert np.array_equal(b2.bits(), c.bloom())
    assert sorted(po.junction_lines(*last.junctions(), c.k)) == sorted(c.junction_lines())
    cn = c.counters
    assert (st["nb_processed"], st["nb_skipped"], st["reads_processed"]) == (cn["nb_processed"], cn["nb_skipped"], cn["scan_reads_processed"])


def _slices_before(nbytes, world):
    """the formula of sharded._slices before it took an alignment (a copy, on purpose)"""
    step = -(-nbytes // world)
    step = (step + 15) & ~15
    return [(min(q * step, nbytes), min((q + 1) * step, nbytes)) for q in range(world)]


def test_slices_alignment_argument():
    sizes = [16, 64, 80, 4096, 4112, 1 << 20, (1 << 20) + 16, 3 << 17, 1 << 30]
    for nbytes in sizes:
        for world in range(1, 10):
            assert sharded._slices(nbytes, world) == sharded._slices(nbytes, world, 16) == _slices_before(nbytes, world)
    for nbytes in [64, 128, 4096, 1 << 20, 3 << 17, 1 << 28, 1 << 30]:      # filters: powers of two and the like, multiples of 64 bytes
        for world in range(1, 10):
            sl = sharded._slices(nbytes, world, 64)
            assert len(sl) == world and sl[0][0] == 0 and sl[-1][1] == nbytes
            assert all(lo % 64 == 0 and hi % 64 == 0 and lo <= hi for lo, hi in sl)
            assert all(a[1] == b[0] for a, b in zip(sl[:-1], sl[1:]))       # disjoint, in order, no gap
