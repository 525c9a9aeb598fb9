"""Pass 1 by filter slices under --mercy (sharded.load_sliced and run_in_turn(protocol="slices") with a backend whose `mercy` is true) on CPU.
The lockstep -- batch, OR of its fail plane, probe; then the OR of the miss planes, the commit, the gather -- is driven with a TEST-ONLY
stand-in: own bits with their first-set times, numpy planes, the reference's per-segment state machine in Python.  What is checked is the
protocol: that a membership test of isJunction is a per-bit question its owner can answer, that the OR of the ranks' miss bits is "not in
bloo1", that a superset of the reference's tests is harmless.  Filters and to_bloo2 must equal po.load_two_filters(..., mercy=True), under
gloo with 2 and 3 ranks and in turn with 4, on the three mercy goldens and on random low-coverage reads."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from faucet_amd import sharded, synth
from oracle import pyoracle as po
from tests.golden_util import Case
from tests.test_sharded_gloo import _free_port
from tests.test_slices_cpu import _SEG, SliceShard, _batches

NEVER = np.iinfo(np.int64).max
_windows_cache = {}
_cand_cache = {}


def mercy_windows(bases, offs, k, tai, nh):
    """per k-mer occurrence of the batch, in the reference's processing order: (its nh bit positions, the k-mer as read, the k-mer of the
    window before it in its unambiguous segment or None for the segment's first window)"""
    key = (bases.ctypes.data, offs.tobytes(), k, tai, nh)
    got = _windows_cache.get(key)
    if got is None:
        lib = po.lib()
        raw = bases.tobytes()
        got = []
        for a, z in zip(offs[:-1], offs[1:]):
            # (getUnambiguousReads pushes to the FRONT of its list, utils/Kmer.cpp:77: the segments of a read are met right to left)
            for m in reversed(list(_SEG.finditer(raw, int(a), int(z)))):
                seg = m.group()
                prev = None
                for i in range(len(seg) - k + 1):
                    km = lib.fo_encode(seg[i:i + k], k)
                    got.append((bit_positions(lib.fo_canon(km, k), tai, nh), km, prev))
                    prev = km
        _windows_cache[key] = got
    return got


def bit_positions(canon, tai, nh):
    got = _cand_cache.get((canon, tai, nh))
    if got is None:
        lib = po.lib()
        h_a, h_b = lib.fo_old_hash(canon, 0, tai), lib.fo_old_hash(canon, 1, tai)
        got = _cand_cache[(canon, tai, nh)] = [(h_a + q * h_b) % tai for q in range(nh)]
    return got


def candidates(km, prev, contained, k):
    """(nt, extension) of isJunction as load_two_filters calls it at a window that is not the first of its segment (utils/Bloom.cpp:249-265):
    the cursor faces BACKWARD there, so the real extension is the reverse complement of the window before; a contained window is tested
    BACKWARD (its reverse complement is extended), any other FORWARD"""
    lib = po.lib()
    real_ext = lib.fo_revcomp(prev, k)
    frm = lib.fo_revcomp(km, k) if contained else km
    mask = (1 << (2 * k)) - 1
    for nt in range(4):
        e = ((frm << 2) | nt) & mask
        if e != real_ext:
            yield nt, e


class MercySliceShard(SliceShard):
    """SliceShard + the five-step protocol: first-set times of the own bits (the time of an occurrence = its index in the whole stream), the
    fail plane per batch, four miss planes per batch as one block, the mercy state machine at the commit.  counts = [positions this rank
    probed, high->low tests answered "junction", runs opened, low->high tests answered "junction", runs added, k-mers added by runs]"""
    mercy = True

    def slice_load(self, batches, bit_lo, bit_hi):
        raise AssertionError("a mercy backend is driven through slice_mercy_begin / _batch / _probe")

    def slice_mercy_begin(self, bit_lo, bit_hi):
        assert bit_lo % 512 == 0 and bit_hi % 512 == 0 and bit_lo <= bit_hi <= self.tai
        self.lo, self.hi = bit_lo, bit_hi
        self.first = np.full(bit_hi - bit_lo, NEVER, dtype=np.int64)
        self.own2 = bytearray(bit_hi - bit_lo)
        self._stream, self._planes, self._windows, self._t0, self._miss = [], [], [], [], []
        self._owed = False
        self._time = 0
        self.counts = [0] * 6

    def _own(self, hs):
        return [h - self.lo for h in hs if self.lo <= h < self.hi]

    def slice_mercy_batch(self, batch):
        if self._owed:
            raise RuntimeError("slice_mercy_batch while the probe of the previous batch is owed")
        win = mercy_windows(batch[0], batch[1], self.k, self.tai, self.nh)
        if not win:
            return None
        fail = np.zeros(-(-len(win) // 128) * 128, dtype=np.uint8)
        for t, (hs, _, _) in enumerate(win):
            for o in self._own(hs):
                if self.first[o] == NEVER:
                    fail[t] = 1                       # one of MY bits was not set before this occurrence
                    self.first[o] = self._time + t
        self._stream.append([w[0] for w in win])
        self._windows.append(win)
        self._t0.append(self._time)
        self._time += len(win)
        self._planes.append(torch.from_numpy(np.packbits(fail, bitorder="little")))
        self._owed = True
        return self._planes[-1]

    def slice_mercy_probe(self):
        if not self._owed:
            return
        win, t0 = self._windows[-1], self._t0[-1]
        fail = np.unpackbits(self._planes[-1].numpy(), bitorder="little")      # ORed across the ranks by now
        miss = np.zeros((4, len(fail)), dtype=np.uint8)
        for t, (_, km, prev) in enumerate(win):
            if prev is None:
                continue
            contained = not fail[t]
            if contained and not fail[t - 1]:
                continue                              # the superset: not contained, or contained behind a window that is not
            self.counts[0] += 1
            for nt, e in candidates(km, prev, contained, self.k):
                hs = bit_positions(po.lib().fo_canon(e, self.k), self.tai, self.nh)
                if any(self.first[o] > t0 + t for o in self._own(hs)):
                    miss[nt, t] = 1                   # an own bit of the candidate was not set by time t
        self._miss.append(torch.from_numpy(np.concatenate([np.packbits(m, bitorder="little") for m in miss])))
        self._owed = False

    def slice_mercy_planes(self):
        return self._miss

    def slice_commit(self):
        if self._owed:
            raise RuntimeError("slice_commit while a probe is owed")
        super().slice_commit()                        # the own bloo2 bits of contained occurrences, to_bloo2 = their number
        self.counts[1:] = [0] * 5
        for win, plane, block in zip(self._windows, self._planes, self._miss):
            fail = np.unpackbits(plane.numpy(), bitorder="little")
            miss = np.unpackbits(block.numpy(), bitorder="little").reshape(4, -1)
            have_last, run = False, None
            for t, (_, km, prev) in enumerate(win):
                if prev is None:
                    have_last, run = False, None
                contained = not fail[t]
                if contained:
                    have_last = True
                    if run is not None:               # came from low to high
                        if any(not miss[nt, t] for nt, _ in candidates(km, prev, True, self.k)):
                            self.counts[3] += 1
                        else:
                            self.counts[4] += 1
                            for q in range(run, t):
                                self.counts[5] += 1
                                for o in self._own(win[q][0]):
                                    self.own2[o] = 1
                        run = None
                elif have_last and run is None:       # came from high to low
                    if any(not miss[nt, t] for nt, _ in candidates(km, prev, False, self.k)):
                        self.counts[1] += 1
                    else:
                        self.counts[2] += 1
                        run = t

    def slice_end(self):
        self.own1 = bytearray((self.first != NEVER).astype(np.uint8).tobytes())
        return super().slice_end()


def oracle_pair(bases, offs, k, tai, nh):
    """the oracle's --mercy load, and whether the input exercises the feature at all: its bloo2 differs from the plain load's"""
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    lst = po.load_two_filters(b1, b2, bases, offs, k, mercy=True)
    p1, p2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    po.load_two_filters(p1, p2, bases, offs, k)
    assert np.array_equal(b1.bits(), p1.bits()), "bloo1 evolves the same with and without --mercy"
    assert not np.array_equal(b2.bits(), p2.bits()), "--mercy changes nothing on this input: it tests nothing"
    return b1, b2, lst


def golden_input(name):
    c = Case(name)
    assert c.mercy
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh, _, _ = po.sizing_from_cli(c.E, c.S, c.fp)
    return c, bases, offs, tai, nh


# (seed, world) of the random inputs: seeds of the recipe below on which all four kinds of answer occur and --mercy changes bloo2 (of the
# first twelve, seed 4 changes nothing and seed 6 has no "junction" answer); seed 10 has reads with N: several segments per read
FUZZ = [(1, 2), (3, 3), (7, 2), (10, 3), (11, 2)]


def fuzz_input(seed):
    """random low-coverage reads by the recipe of tests/test_gpu_parity.py::test_mercy_random_inputs_vs_oracle"""
    rng = np.random.default_rng(300 + seed)
    k = int(rng.choice([11, 21, 31]))
    G = int(rng.integers(3000, 30000))
    cov = float(rng.choice([2.0, 5.0, 12.0]))
    n = int(G * cov / 100)
    err, n_rate, repeats = float(rng.choice([0.0, 0.01, 0.03])), float(rng.choice([0.0, 0.003])), int(rng.integers(0, 4))
    g = synth.make_genome(G, 900 + seed, repeats=repeats, repeat_len=3 * k if repeats else 0)
    bases, offs = po.reads_from_matrix(synth.make_reads(g, n, 100, err, 900 + seed + 1, n_rate=n_rate))
    tai, nh = 1 << int(rng.integers(14, 20)), int(rng.integers(1, 5))
    return k, bases, offs, tai, nh


def _input(spec):
    if isinstance(spec, str):
        c, bases, offs, tai, nh = golden_input(spec)
        return c.k, bases, offs, tai, nh
    return fuzz_input(spec)


def _worker(rank, world, port, spec, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    k, bases, offs, tai, nh = _input(spec)
    be = MercySliceShard(k, tai, nh, 1, 100)
    st = sharded.load_sliced(be, _batches(bases, offs, 3), rank, world)
    np.save(os.path.join(out_dir, f"bloo1_{rank}.npy"), be.b1.bits().copy())
    np.save(os.path.join(out_dir, f"bloo2_{rank}.npy"), be.b2.bits().copy())
    np.save(os.path.join(out_dir, f"stats_{rank}.npy"), np.array([st["kmers"], st["to_bloo2"]] + be.counts))
    dist.barrier()
    dist.destroy_process_group()


def _check_under_gloo(spec, world, tmp_path):
    k, bases, offs, tai, nh = _input(spec)
    b1, b2, lst = oracle_pair(bases, offs, k, tai, nh)
    mp.spawn(_worker, args=(world, _free_port(), spec, str(tmp_path)), nprocs=world, join=True)
    counts = None
    for r in range(world):      # every rank ends with both global filters and the global counts
        assert np.array_equal(np.load(tmp_path / f"bloo1_{r}.npy"), b1.bits()), f"bloo1 on rank {r}"
        assert np.array_equal(np.load(tmp_path / f"bloo2_{r}.npy"), b2.bits()), f"bloo2 on rank {r}"
        st = [int(x) for x in np.load(tmp_path / f"stats_{r}.npy")]
        assert st[:2] == [lst.kmers, lst.to_bloo2]
        assert counts is None or st[3:] == counts, "the commit's counts are global: the same on every rank"
        counts = st[3:]
        assert st[2] > 0
    assert all(c > 0 for c in counts), f"the input does not bring out all four kinds of answer: {counts}"
    return b2


@pytest.mark.parametrize("name,world", [("mercy_k21", 2), ("mercy_k21", 3), ("pe_mercy_k21", 3), ("pe_mercy_fp6_k21", 2)])
def test_mercy_goldens_sliced_under_gloo_equal_the_oracle(name, world, tmp_path):
    b2 = _check_under_gloo(name, world, tmp_path)
    assert np.array_equal(b2.bits(), Case(name).bloom())      # ... which is the compiled reference's --mercy .bloom


@pytest.mark.parametrize("seed,world", FUZZ)
def test_mercy_random_low_coverage_inputs_sliced_under_gloo(seed, world, tmp_path):
    _check_under_gloo(seed, world, tmp_path)


@pytest.mark.parametrize("spec", ["mercy_k21", "pe_mercy_k21", "pe_mercy_fp6_k21", FUZZ[3][0], FUZZ[4][0]], ids=str)
def test_mercy_slices_in_turn_in_one_process_equal_the_oracle(spec):
    """run_in_turn(protocol="slices") with 4 mercy backends: the lockstep with its in-process ORs; after_load once, with the final filters"""
    world = 4
    k, bases, offs, tai, nh = _input(spec)
    b1, b2, lst = oracle_pair(bases, offs, k, tai, nh)
    cuts = np.linspace(0, len(offs) - 1, world + 1).astype(int)
    shards = [_batches(bases, offs[cuts[r]:cuts[r + 1] + 1].copy(), 2) for r in range(world)]
    calls, backs = [], []

    def after_load(r, stats, bloo1, bloo2):
        calls.append(r)
        assert np.array_equal(bloo1.numpy(), b1.bits()) and np.array_equal(bloo2.numpy(), b2.bits())
        assert (stats["kmers"], stats["to_bloo2"]) == (lst.kmers, lst.to_bloo2)

    def make():
        backs.append(MercySliceShard(k, tai, nh, 1, 100))
        return backs[-1]

    load_stats, _, _ = sharded.run_in_turn(make, shards, "slices", after_load)
    assert calls == [world - 1]
    assert len(load_stats) == world and all(s["to_bloo2"] == lst.to_bloo2 for s in load_stats)
    loaders = backs[:world]                           # (the backends after them are the scans')
    assert all(b.counts[1:] == loaders[0].counts[1:] for b in loaders)
    assert all(c > 0 for c in loaders[0].counts[1:]), loaders[0].counts
    assert sum(b.counts[0] for b in loaders) == world * loaders[0].counts[0], "every rank probes the same superset"


def test_one_rank_is_the_whole_filter_and_the_superset_is_a_superset():
    """[0, tai) on one rank: no exchange changes anything, the filters are the oracle's, and every test the state machine makes was probed"""
    c, bases, offs, tai, nh = golden_input("mercy_k21")
    b1, b2, lst = oracle_pair(bases, offs, c.k, tai, nh)
    be = MercySliceShard(c.k, tai, nh, 1, 100)
    st = sharded.load_sliced(be, _batches(bases, offs, 4), 0, 1)
    assert np.array_equal(be.b1.bits(), b1.bits()) and np.array_equal(be.b2.bits(), b2.bits())
    assert (st["kmers"], st["to_bloo2"]) == (lst.kmers, lst.to_bloo2)
    probed, hl_j, opened, lh_j, added, kmers = be.counts
    assert probed >= hl_j + opened + lh_j + added and kmers >= added > 0
    assert opened >= lh_j + added                     # a run that reaches the end of its segment is dropped


class _Spy:
    """records the slice_* methods a caller fetches from the backend, in order"""

    def __getattribute__(self, name):
        if name.startswith("slice_"):
            object.__getattribute__(self, "calls").append(name)
        return super().__getattribute__(name)


def test_the_lockstep_and_its_rule():
    """load_sliced drives a mercy backend batch by batch -- batch, (exchange,) probe -- and the miss planes before the commit; on the stand-in a
    batch or a commit before the owed probe raises, an empty batch keeps no plane and owes no probe, a probe with nothing owed does nothing.
    A backend without `mercy` (the stand-in of tests/test_slices_cpu.py) is called exactly as before."""
    c, bases, offs, tai, nh = golden_input("mercy_k21")
    batches = _batches(bases, offs[:201].copy(), 2)
    empty = (bases[:0], offs[:1].copy())

    class SpyMercy(_Spy, MercySliceShard):
        calls = []

    sharded.load_sliced(SpyMercy(c.k, tai, nh, 1, 100), [batches[0], empty, batches[1]], 0, 1)
    assert SpyMercy.calls == ["slice_mercy_begin", "slice_mercy_batch", "slice_mercy_probe", "slice_mercy_batch", "slice_mercy_batch",
                              "slice_mercy_probe", "slice_mercy_planes", "slice_commit", "slice_end"]

    class SpyPlain(_Spy, SliceShard):
        calls = []

    sharded.load_sliced(SpyPlain(c.k, tai, nh, 1, 100), batches, 0, 1)
    assert SpyPlain.calls == ["slice_load", "slice_planes", "slice_commit", "slice_end"]

    be = MercySliceShard(c.k, tai, nh, 1, 100)
    be.slice_mercy_begin(0, tai)
    assert be.slice_mercy_batch(batches[0]) is not None
    with pytest.raises(RuntimeError, match="owed"):
        be.slice_mercy_batch(batches[1])
    with pytest.raises(RuntimeError, match="owed"):
        be.slice_commit()
    be.slice_mercy_probe()
    be.slice_mercy_probe()                            # nothing owed: nothing done
    assert len(be.slice_mercy_planes()) == 1
    assert be.slice_mercy_batch(empty) is None
    be.slice_mercy_batch(batches[1])
    be.slice_mercy_probe()
    be.slice_commit()
    be.slice_end()
