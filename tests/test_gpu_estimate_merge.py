"""Pass 0 over read shards (fgpu_estimate_merge, fgpu_group_estimate_end, ShardedRun::estimate, `faucet -gpus N --estimate`): the sketches of
the shards merge into exactly the planes one device makes of all reads.  The device's planes are compared byte for byte, its counts to the last
counter, with the numpy restatement (tests/estimate_planes_ref.py, pinned by tests/test_estimate_merge_cpu.py); the command line with its own
first-device pass (FAUCET_ESTIMATE_SHARDS=0).  The box has one GPU: the ranks are threads with contexts on device 0 and the copy transport, as
in tests/test_gpu_multi.py.  Needs an MI355X."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from tests import estimate_planes_ref as P
from tests import estimate_ref as R
from tests.golden_util import Case
from tests.test_gpu_estimate import _cli, _round, _stable, _without_counts, host_arrays, placeholder

pytestmark = pytest.mark.gpu

K = 21
GOLDEN = "se_cleaning_k21"


# ---- two contexts, one merge ----------------------------------------------------------------------------------------------------------------
def two_read_sets():
    """A and B: 160 occurrences each at k = 21.  Each has a read twice (cells hit twice by one k-mer) and they share a read (cells hit once on
    both sides); the rest is random, and 2^8 cells per level are few enough for every pair of cell states to occur"""
    rng = np.random.default_rng(20261019)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = [acgt[rng.integers(0, 4, 60)].tobytes() for _ in range(5)]
    return [reads[0], reads[1], reads[1], reads[2]], [reads[2], reads[3], reads[4], reads[4]]


@pytest.fixture(scope="module")
def pair():
    a, b = two_read_sets()
    ca, cb = R.canon_kmers(a, K), R.canon_kmers(b, K)
    pa, pb, pab = P.planes(ca, 8), P.planes(cb, 8), P.planes(np.concatenate([ca, cb]), 8)
    # a condition on the input, not on the code: every combination of cell states occurs at level 0
    sa, sb = P.cell_states(pa, 8, 0), P.cell_states(pb, 8, 0)
    assert {(int(x), int(y)) for x, y in zip(sa, sb)} >= {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (0, 2), (1, 2), (2, 2)}
    assert 100 < len(ca) + len(cb) < 1000
    assert np.array_equal(P.merge(pa, pb), pab)
    for arr in (pa, pb, pab):
        arr.setflags(write=False)
    return a, b, pa, pb, pab


def open_pass(ctx, lines, r_bits):
    ctx.estimate_begin(r_bits)
    if lines:
        ctx.estimate_batch(api.ReadBatch(*host_arrays(lines)))


def test_merge_rule_on_every_pair_of_cell_states(pair):
    a, b, pa, pb, pab = pair
    ca, cb = placeholder(K), placeholder(K)
    open_pass(ca, a, 8)
    open_pass(cb, b, 8)
    assert np.array_equal(ca.estimate_download(), pa) and np.array_equal(cb.estimate_download(), pb)      # (both devices' streams waited for)
    peer, nbytes = cb.estimate_planes_devptr()
    assert nbytes == 256 and ca.estimate_planes_devptr()[1] == 256
    ca.estimate_merge(peer, 0, nbytes)
    got = ca.estimate_download()
    assert got.tobytes() == pab.tobytes()
    assert np.array_equal(cb.estimate_download(), pb)                 # the peer's planes are read, not written
    assert ca.estimate_kmers() == len(R.canon_kmers(a, K)) and cb.estimate_kmers() == len(R.canon_kmers(b, K))
    # the merged planes count as the planes of A + B (kmers stay each context's own)
    empty, once, _ = R.counts(np.concatenate([R.canon_kmers(a, K), R.canon_kmers(b, K)]), 8)
    end = ca.estimate_end()
    assert (end["empty"], end["once"], end["kmers"]) == (empty, once, len(R.canon_kmers(a, K)))
    cb.estimate_end()
    ca.close()
    cb.close()


@pytest.mark.parametrize("pieces", [[0, 80, 256], [0, 16, 80, 96, 208, 256], [208, 256, 0, 16, 96, 208, 16, 96]], ids=["two", "five", "any_order"])
def test_merge_in_pieces_whose_borders_are_not_level_borders(pair, pieces):
    """a level is 64 bytes at r_bits 8: 80, 16, 96 and 208 lie inside levels; a piece may cross one or two level borders"""
    a, b, pa, pb, pab = pair
    ca, cb = placeholder(K), placeholder(K)
    open_pass(ca, a, 8)
    open_pass(cb, b, 8)
    cb.estimate_download()
    peer, _ = cb.estimate_planes_devptr()
    ranges = list(zip(pieces[:-1], pieces[1:])) if pieces[0] == 0 and sorted(pieces) == pieces else list(zip(pieces[0::2], pieces[1::2]))
    assert sorted(ranges)[0][0] == 0 and sorted(ranges)[-1][1] == 256 and all(x[1] == y[0] for x, y in zip(sorted(ranges), sorted(ranges)[1:]))
    want = pa.copy()
    for lo, hi in ranges:
        ca.estimate_merge(peer + lo, lo, 0)                           # nothing at all, at every border
        ca.estimate_merge(peer + lo, lo, hi - lo)
        want[lo // 4:hi // 4] = pab[lo // 4:hi // 4]
        assert ca.estimate_download().tobytes() == want.tobytes(), (lo, hi)
    ca.estimate_merge(peer, 256, 0)                                   # ... and at the very end
    assert ca.estimate_download().tobytes() == pab.tobytes()
    ca.estimate_end()
    cb.estimate_end()
    ca.close()
    cb.close()


def test_merge_refusals(pair):
    a, b, pa, pb, pab = pair
    lib = L.load()
    ca, cb = placeholder(K), placeholder(K)
    open_pass(ca, a, 8)
    open_pass(cb, b, 8)
    cb.estimate_download()
    peer, _ = cb.estimate_planes_devptr()
    for args in ((peer, 8, 16), (peer, 0, 24), (peer + 8, 0, 16),                 # misaligned: the first byte, the length, the pointer
                 (peer, 240, 32), (peer, 272, 0), (peer, 0, 272), (peer, 16, (1 << 64) - 16),     # past the end of the planes
                 (None, 0, 16), (None, 0, 0)):                                    # no pointer
        assert lib.fgpu_estimate_merge(ca.h, args[0], args[1], args[2]) == L.ERR_ARG, args
    assert lib.fgpu_estimate_planes(ca.h, None, None) == L.ERR_ARG
    host = np.zeros(64, np.uint32)
    assert lib.fgpu_estimate_download(ca.h, host.ctypes.data, 128) == L.ERR_ARG and lib.fgpu_estimate_download(ca.h, None, 256) == L.ERR_ARG
    assert np.array_equal(ca.estimate_download(), pa)                 # nothing was merged
    ca.estimate_end()
    # outside a pass
    p, n = C.c_void_p(), C.c_uint64()
    assert lib.fgpu_estimate_planes(ca.h, C.byref(p), C.byref(n)) == L.ERR_STATE
    assert lib.fgpu_estimate_merge(ca.h, peer, 0, 16) == L.ERR_STATE
    assert lib.fgpu_estimate_download(ca.h, host.ctypes.data, 256) == L.ERR_STATE
    assert lib.fgpu_estimate_kmers(ca.h, C.byref(n)) == L.ERR_STATE
    ca.load_begin()
    assert lib.fgpu_estimate_merge(ca.h, peer, 0, 16) == L.ERR_STATE
    ca.load_end()
    cb.estimate_end()
    ca.close()
    cb.close()


# ---- the collective end ---------------------------------------------------------------------------------------------------------------------
def run_ranks(n, body, transport=L.TRANSPORT_COPY):
    """body(rank, ctx, group) on n threads with a context each on device 0, tied into one group; the results by rank"""
    lib = L.load()
    ctxs = [placeholder(K) for _ in range(n)]
    g = C.c_void_p()
    assert lib.fgpu_group_create(n, transport, C.byref(g)) == 0, lib.fgpu_group_last_error(g, -1)
    out, errs = [None] * n, []

    def rank(r):
        try:
            assert lib.fgpu_group_attach(g, r, ctxs[r].h) == 0, lib.fgpu_group_last_error(g, r)
            out[r] = body(r, ctxs[r], g)
        except BaseException as e:   # noqa: BLE001
            errs.append((r, e))
            lib.fgpu_group_abort(g)

    th = [threading.Thread(target=rank, args=(r,)) for r in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    lib.fgpu_group_destroy(g)
    for ctx in ctxs:
        ctx.close()
    assert not errs, errs
    return out


def deal(lines, n, empty_rank=None):
    """the records dealt contiguously over n ranks; empty_rank gets none at all"""
    holders = [r for r in range(n) if r != empty_rank]
    cuts = np.linspace(0, len(lines), len(holders) + 1).astype(int)
    shares = {r: lines[cuts[i]:cuts[i + 1]] for i, r in enumerate(holders)}
    return [shares.get(r, []) for r in range(n)]


def assert_whole_sketch(got, name, r_bits):
    empty, once, kmers = R.golden_counts(name, r_bits)
    assert (got["empty"], got["once"], got["kmers"], got["r_bits"]) == (empty, once, kmers, r_bits)
    level, f0, f1 = api.estimate_solve(empty, once, r_bits)
    assert (got["level"], got["f0"], got["f1"]) == (level, f0, f1)


@pytest.mark.parametrize("chunk", [None, 1024], ids=["one_chunk", "chunks_1KiB"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_collective_end_gives_every_rank_the_sketch_of_all_reads(n, chunk, monkeypatch):
    """2^8 cells per level: 16 granules of planes, which 3 does not divide (slices of 6, 6 and 4); 2^14: 16 KiB, in steps of 1 KiB when the
    staging chunk is forced down (8 steps at N = 2; at N = 3 slices of 5472, 5472 and 5440 bytes, so the last of 6 steps is short)"""
    if chunk:
        monkeypatch.setenv("FGPU_ESTIMATE_MERGE_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("FGPU_ESTIMATE_MERGE_CHUNK", raising=False)
    lines = Case(GOLDEN).lines()
    runs = [(r_bits, empty_rank) for r_bits in ([14] if chunk else [8, 14]) for empty_rank in (None, 1, n - 1)]
    lib = L.load()

    def body(r, ctx, g):
        got = []
        for r_bits, empty_rank in runs:
            open_pass(ctx, deal(lines, n, empty_rank)[r], r_bits)
            rc, est = api.group_estimate_end(g, r)
            assert rc == L.OK, lib.fgpu_group_last_error(g, r)
            got.append(est)
            # the pass is over: the calls of an open pass are refused, the next one begins from clean planes
            assert lib.fgpu_estimate_end(ctx.h, None) == L.ERR_STATE
        ctx.estimate_begin(8)
        assert ctx.estimate_end()["empty"] == [1 << 8] * 4
        return got

    out = run_ranks(n, body)
    for i, (r_bits, _) in enumerate(runs):
        for r in range(n):
            assert out[r][i] == out[0][i], (r_bits, r)
        assert_whole_sketch(out[0][i], GOLDEN, r_bits)


@pytest.mark.parametrize("transport", [L.TRANSPORT_COPY, L.TRANSPORT_RCCL], ids=["copy", "rccl"])
def test_a_group_of_one_rank_ends_as_estimate_end_does(transport):
    lines = Case(GOLDEN).lines()

    def body(r, ctx, g):
        open_pass(ctx, lines, 14)
        rc, est = api.group_estimate_end(g, r)
        assert rc == L.OK
        open_pass(ctx, lines, 14)
        assert ctx.estimate_end() == est
        return est

    assert_whole_sketch(run_ranks(1, body, transport)[0], GOLDEN, 14)


def test_ranks_that_do_not_agree_are_all_refused_and_their_passes_closed():
    lib = L.load()
    lines = Case(GOLDEN).lines()[:50]

    def body(r, ctx, g):
        got = []
        open_pass(ctx, lines, 8 if r == 0 else 10)              # different r_bits
        got.append(api.group_estimate_end(g, r)[0])
        got.append(lib.fgpu_estimate_end(ctx.h, None))
        if r != 1:                                              # rank 1 is not in a pass
            open_pass(ctx, lines, 8)
        got.append(api.group_estimate_end(g, r)[0])
        got.append(lib.fgpu_estimate_end(ctx.h, None))
        msg = lib.fgpu_group_last_error(g, r).decode()
        open_pass(ctx, deal(lines, 3)[r], 8)                    # the group is still good
        rc, est = api.group_estimate_end(g, r)
        assert rc == L.OK
        return got, msg, est

    out = run_ranks(3, body)
    for r in range(3):
        assert out[r][0] == [L.ERR_ARG, L.ERR_STATE, L.ERR_STATE, L.ERR_STATE], r
        assert "not in an estimate pass" in out[r][1]
        assert out[r][2] == out[0][2]
    empty, once, kmers = R.counts(R.canon_kmers(lines, K), 8)
    assert (out[0][2]["empty"], out[0][2]["once"], out[0][2]["kmers"]) == (empty, once, kmers)


def test_a_sketch_too_full_is_a_capacity_error_on_every_rank_with_the_counts_filled_in():
    """3 M random 31-mers over two ranks: level 3 holds a 16^-3 sample of them, some 730, in 2^8 cells -- a load of 2.9, about 15 cells left empty
    of the 32 the solve asks for"""
    k, rng = 31, np.random.default_rng(5)
    lines = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4000)].tobytes() for _ in range(750)]
    want = R.counts(R.canon_kmers(lines, k), 8)
    assert R.solve(want[0], want[1], 8) is None
    lib = L.load()
    ctxs = [placeholder(k) for _ in range(2)]
    g = C.c_void_p()
    assert lib.fgpu_group_create(2, L.TRANSPORT_COPY, C.byref(g)) == 0
    out, errs = [None] * 2, []

    def rank(r):
        try:
            assert lib.fgpu_group_attach(g, r, ctxs[r].h) == 0
            open_pass(ctxs[r], deal(lines, 2)[r], 8)
            rc, est = api.group_estimate_end(g, r)
            out[r] = (rc, est, lib.fgpu_group_last_error(g, r).decode(), lib.fgpu_estimate_end(ctxs[r].h, None))
        except BaseException as e:   # noqa: BLE001
            errs.append((r, e))
            lib.fgpu_group_abort(g)

    th = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    lib.fgpu_group_destroy(g)
    for ctx in ctxs:
        ctx.close()
    assert not errs, errs
    for r in range(2):
        rc, est, msg, after = out[r]
        assert rc == L.ERR_CAPACITY and "raise r_bits" in msg and after == L.ERR_STATE
        assert (est["empty"], est["once"], est["kmers"], est["level"]) == (want[0], want[1], want[2], -1)


# ---- the command line -----------------------------------------------------------------------------------------------------------------------
def _files(where):
    return {name: open(os.path.join(where, name), "rb").read() for name in sorted(os.listdir(where))}


def _ab(tmp_path, inp, args, gpus):
    """the same command with pass 0 over the read shards (the default) and on the first device alone"""
    args = args + ["--estimate", "-gpus", str(gpus)]
    s = _cli(str(tmp_path / f"shards_{gpus}"), inp, args, env={"FGPU_CLI_TIMES": "1"})
    o = _cli(str(tmp_path / f"first_{gpus}"), inp, args, env={"FGPU_CLI_TIMES": "1", "FAUCET_ESTIMATE_SHARDS": "0"})
    assert s.returncode == o.returncode, s.stdout[-2000:] + s.stderr[-3000:] + o.stderr[-3000:]
    assert _stable(s.stdout) == _stable(o.stdout)
    assert s.stdout.split("\n")[:2] == o.stdout.split("\n")[:2]
    fs, fo = _files(str(tmp_path / f"shards_{gpus}")), _files(str(tmp_path / f"first_{gpus}"))
    assert sorted(fs) == sorted(fo) and all(fs[name] == fo[name] for name in fs), sorted(fs)
    assert re.search(r"\[cli\] pass 0 \(shards\) +[0-9.]+ ms", s.stderr), s.stderr[-3000:]
    assert "pass 0 (read + estimate)" not in s.stderr and "pass 0 (shards)" not in o.stderr and "pass 0 (read + estimate)" in o.stderr
    by_rank = re.findall(r"^\[cli\]   rank (\d+): (\d+) k-mers sketched$", s.stderr, re.M)
    assert [int(r) for r, _ in by_rank] == list(range(gpus)), s.stderr[-3000:]
    return s, [int(v) for _, v in by_rank]


@pytest.mark.parametrize("gpus", [2, 3])
@pytest.mark.parametrize("name", ["se_cleaning_k21", "pe_fastq_k21"])
def test_cli_estimates_over_read_shards_as_on_the_first_device(name, gpus, tmp_path):
    c = Case(name)
    inp = str(tmp_path / ("reads.fq" if c.fastq else "reads.fa"))
    with open(inp, "wb") as f:
        f.write(c.reads_text())
    s, by_rank = _ab(tmp_path, inp, _without_counts(c.meta["args"]) + ["-estimate_bits", "14"], gpus)
    assert s.returncode == (0 if c.no_cleaning else 3), s.stdout[-2000:] + s.stderr[-3000:]
    empty, once, kmers = R.golden_counts(name, 14)
    _, f0, f1 = R.solve(empty, once, 14)
    assert s.stdout.split("\n")[:2] == [f"Estimated distinct k-mers (F0): {_round(f0)}", f"Estimated singletons (f1): {max(_round(f1), 1)}"]
    assert sum(by_rank) == kmers and all(v > 0 for v in by_rank)
    assert {"out.bloom", "out.junctions"} <= set(os.listdir(str(tmp_path / f"shards_{gpus}")))


def test_cli_default_bits_over_two_shards(tmp_path):
    """2^30 cells per level: 1 GiB of planes per rank, slices of 512 MiB merged through the bounded staging buffer in four steps"""
    c = Case("se_cleaning_k21")
    inp = str(tmp_path / "reads.fa")
    with open(inp, "wb") as f:
        f.write(c.reads_text())
    s, by_rank = _ab(tmp_path, inp, _without_counts(c.meta["args"]), 2)
    assert s.returncode == 3, s.stdout[-2000:] + s.stderr[-3000:]
    empty, once, kmers = R.golden_counts(c.name, 30)
    _, f0, f1 = R.solve(empty, once, 30)
    assert s.stdout.split("\n")[:2] == [f"Estimated distinct k-mers (F0): {_round(f0)}", f"Estimated singletons (f1): {max(_round(f1), 1)}"]
    assert sum(by_rank) == kmers


def test_cli_more_shards_than_records(tmp_path):
    """four shards of a two-record file: two ranks sketch nothing, and at 2^8 cells per level the last slices hold a level each"""
    c = Case("c1_k21")
    few = b"\n".join(c.reads_text().split(b"\n")[:4]) + b"\n"
    inp = str(tmp_path / "few.fa")
    with open(inp, "wb") as f:
        f.write(few)
    s, by_rank = _ab(tmp_path, inp, _without_counts(c.meta["args"]) + ["-estimate_bits", "8"], 4)
    lines = few.split(b"\n")[1:4:2]
    empty, once, kmers = R.counts(R.canon_kmers(lines, c.k), 8)
    _, f0, f1 = R.solve(empty, once, 8)
    assert s.stdout.split("\n")[:2] == [f"Estimated distinct k-mers (F0): {_round(f0)}", f"Estimated singletons (f1): {max(_round(f1), 1)}"]
    assert sum(by_rank) == kmers > 0 and sorted(by_rank)[:2] == [0, 0]
