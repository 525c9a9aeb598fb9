"""fgpu_stage3_build (JunctionMap::buildContigGraph's order-dependent contig list in one device call) against tests/graph_build_ref.py run over
the host walker with the oracle's probes (tests/test_graph_build_ref_cpu.py) -- never over the device's own walks: every call that is made, in
order, with its phase, far k-mer, string, distances, coverages and kills, the status and the stopping call, on every fixture and map order;
against faucet_amd/stage3.py's build_serial (one fgpu_stage3_contigs call per getContig, the map set again after every kill); and the edges of
the call."""
import ctypes as C

import numpy as np
import pytest

from faucet_amd import stage3
from tests import graph_build_ref as G
from tests.test_graph_build_ref_cpu import CASES, Finder, build_of
from tests.test_stage3_walker import _device, _fixture, _starts

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5A5A5A5A5


def _same_as_restatement(b, res):
    out, calls, strings, dists, covs, kills, info = res
    assert (info["status"], info["stop_call"], len(out), len(calls)) == (b.status, len(b.calls), len(b.calls), len(b.calls))
    for i, w in enumerate(b.calls):
        g, h, c = out[i], calls[i], w.contig
        assert (int(h["time"]), int(h["phase"]), int(h["start_kmer"])) == (w.t, w.phase, w.start), i
        assert (int(h["far_kmer"]), int(h["far_is_junction"]), int(h["far_is_start"])) == (w.far_kmer, w.far_is_junction, w.far_is_start), (i, w.t)
        assert int(g["status"]) == 0
        got = (int(g["ind1"]), int(g["ind2"]), int(g["end_kmer"]), int(g["end_node"]), strings[i], dists[i].tolist(), covs[i].tolist(), kills[i].tolist())
        assert got == tuple(c[1:]), (i, w.t)
        assert (int(g["len"]), int(g["n_seg"]), int(g["n_cov"])) == (len(c.string), len(c.distances), len(c.coverages)), (i, w.t)
    if b.n_times is not None:
        assert info["calls_possible"] == b.n_times
    assert 1 <= info["rounds"] <= info["calls_possible"] + 2 and info["rewalked"] >= len(b.calls) and info["rewalked_by_round"][0] >= len(b.calls)
    assert sum(info["rewalked_by_round"]) == info["rewalked"] or info["rounds"] > len(info["rewalked_by_round"])


@pytest.mark.parametrize("name, order", CASES)
def test_build_against_the_restatement(name, order):
    b, keys, recs, _, _ = build_of(name, order)
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    _same_as_restatement(b, ctx.stage3_build(_fixture(name).max_read_length))


@pytest.mark.parametrize("name", ["s3_k8", "twohash_k31_L150__shift", "s3_k8__drop70"])
def test_build_against_the_serial_loop_over_the_chain_call(name):
    """the fixed point pinned to the merged chain code alone: the literal loop, one fgpu_stage3_contigs per getContig on a map set again"""
    fx = _fixture(name)
    ctx = _device(name)
    want, status, sets = stage3.build_serial(ctx, fx.keys, fx.recs, fx.case.k, fx.max_read_length)
    assert sets > 1 or not want
    ctx.stage3_set_junctions(fx.keys, fx.recs)
    out, calls, strings, dists, covs, kills, info = ctx.stage3_build(fx.max_read_length)
    assert (info["status"], len(out)) == (status, len(want))
    if name == "s3_k8":
        assert info["regrown"] >= 1 and info["table_hits"] > 8 * info["calls_possible"] + 1024      # round 0 outgrew its array and was run again
    for i, w in enumerate(want):
        g, h = out[i], calls[i]
        got = dict(phase=int(h["phase"]), start=int(h["start_kmer"]), ind1=int(g["ind1"]), ind2=int(g["ind2"]), end_kmer=int(g["end_kmer"]), end_node=int(g["end_node"]),
                   string=strings[i], distances=dists[i].tolist(), coverages=covs[i].tolist(), kills=kills[i].tolist(), far_kmer=int(h["far_kmer"]),
                   far_is_junction=int(h["far_is_junction"]), far_is_start=int(h["far_is_start"]))
        assert got == w, i


def _custom(name, pick):
    fx = _fixture(name)
    paths = (np.asarray(fx.recs["cov"]) > 0).sum(axis=1)
    keys, recs = fx.keys[pick(paths)], fx.recs[pick(paths)]
    f = Finder(fx, keys, recs)
    b = G.build_contig_graph(lambda alive, km, ix: f.find(np.asarray(alive, dtype=bool), km, ix), keys, recs["cov"], fx.case.k)
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    return fx, b, ctx


def test_an_empty_map_a_map_without_and_a_map_of_only_complex_junctions():
    fx = _fixture("c1_k21")
    ctx = _device("c1_k21")
    ctx.stage3_set_junctions(fx.keys[:0], fx.recs[:0])
    out, calls, strings, dists, covs, kills, info = ctx.stage3_build(fx.max_read_length)
    assert len(out) == len(calls) == 0 and strings == [] and (info["status"], info["stop_call"], info["rounds"], info["probes"]) == (0, 0, 0, 0)
    assert ctx.lib.fgpu_stage3_build_take(ctx.h, None, None, 0, None, 0, None, None, 0, None, 0) == 0
    fx, b, ctx = _custom("c1_k21", lambda paths: paths == 1)
    assert b.calls and all(w.phase != G.BRANCHING for w in b.calls)
    _same_as_restatement(b, ctx.stage3_build(fx.max_read_length))
    fx, b, ctx = _custom("c1_k21", lambda paths: paths > 1)
    assert b.calls and all(w.phase == G.BRANCHING for w in b.calls)
    _same_as_restatement(b, ctx.stage3_build(fx.max_read_length))


def test_take_with_an_array_one_entry_short_keeps_the_results():
    from faucet_amd import _lib as L
    from faucet_amd import api
    name = "s3_k8__drop70"
    fx = _fixture(name)
    ctx = _device(name)
    ctx.stage3_set_junctions(fx.keys, fx.recs)
    want = ctx.stage3_build(fx.max_read_length, raw=True)
    totals = (C.c_uint64 * 4)()
    assert ctx.lib.fgpu_stage3_build(ctx.h, fx.max_read_length, totals, None) == L.OK
    n, nt, ns, nc = list(totals)
    assert (n, nt, ns, nc) == (len(want[0]), len(want[2]), len(want[4]), len(want[5])) and min(n, nt, ns, nc) > 1
    out, calls = np.full(n * api.CONTIG_DTYPE.itemsize, 0x5A, dtype=np.uint8), np.full(n * api.BUILD_DTYPE.itemsize, 0x5A, dtype=np.uint8)
    text, kmers = np.full(nt + 2, FILL, dtype=np.uint64), np.full(ns + 2, FILL, dtype=np.uint64)
    dist, cov = np.full(ns + 2, 0x5A, dtype=np.uint8), np.full(nc + 2, 0x5A, dtype=np.uint8)

    def take(short):
        return ctx.lib.fgpu_stage3_build_take(ctx.h, out.ctypes.data, calls.ctypes.data, n - short[0], text.ctypes.data, nt - short[1], kmers.ctypes.data,
                                              dist.ctypes.data, ns - short[2], cov.ctypes.data, nc - short[3])
    for short in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
        assert take(short) == L.ERR_ARG
        assert (out == 0x5A).all() and (calls == 0x5A).all() and (text == FILL).all() and (kmers == FILL).all() and (dist == 0x5A).all() and (cov == 0x5A).all()
    assert take((0, 0, 0, 0)) == L.OK
    assert out.tobytes() == want[0].tobytes() and calls.tobytes() == want[1].tobytes()
    assert np.array_equal(text[:nt], want[2]) and np.array_equal(kmers[:ns], want[3]) and np.array_equal(dist[:ns], want[4]) and np.array_equal(cov[:nc], want[5])
    assert (text[nt:] == FILL).all() and (kmers[ns:] == FILL).all() and (dist[ns:] == 0x5A).all() and (cov[nc:] == 0x5A).all()      # nothing behind the totals
    assert take((0, 0, 0, 0)) == L.OK and (text[nt:] == FILL).all()                       # taken: nothing left to copy


def test_the_static_calls_answer_as_before_a_build():
    """the build keeps its times to itself: fgpu_stage3_contigs and fgpu_stage3_find_neighbors on the same context and map answer as before it,
    and a build whose results nobody took does not get in the way of theirs"""
    name = "twohash_k31_L150__mrl10"
    fx = _fixture(name)
    ctx = _device(name)
    ctx.stage3_set_junctions(fx.keys, fx.recs)
    starts, idx = _starts(fx.calls)
    chains = ctx.stage3_contigs(starts, idx, fx.max_read_length, raw=True)
    walks = ctx.stage3_find_neighbors(starts, idx, fx.max_read_length, contigs=True)
    first = ctx.stage3_build(fx.max_read_length, raw=True)
    assert len(first[0]) > 100 and first[6]["rounds"] > 1
    totals = (C.c_uint64 * 4)()
    assert ctx.lib.fgpu_stage3_build(ctx.h, fx.max_read_length, totals, None) == 0 and totals[0] == len(first[0])        # (not taken)
    again = ctx.stage3_contigs(starts, idx, fx.max_read_length, raw=True)
    assert all(np.array_equal(a, b) for a, b in zip(chains[:5], again[:5])) and chains[5] == again[5]
    w2 = ctx.stage3_find_neighbors(starts, idx, fx.max_read_length, contigs=True)
    assert walks[0].tobytes() == w2[0].tobytes() and walks[1:] == w2[1:]
    second = ctx.stage3_build(fx.max_read_length, raw=True)
    assert all(np.array_equal(a, b) for a, b in zip(first[:6], second[:6])) and first[6] == second[6]
