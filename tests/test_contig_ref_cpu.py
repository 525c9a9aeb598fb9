"""tests/contig_ref.py (JunctionMap::getContig restated over a callable findNeighbor) pinned on the reference's recorded findNeighbor answers
(tests/golden/stage3_neighbors_*.jsonl.gz), and the host side of the contig chains -- faucet_amd/stage3.py's start lists and
NeighborWalker.contigs -- pinned on the restatement.  No GPU: the oracle answers the walker's probes, as in tests/test_stage3_walker.py."""
import collections

import numpy as np
import pytest

from faucet_amd import api, stage3
from tests import contig_ref as R
from tests.test_stage3_walker import FIXTURES, _fixture, _OracleProbe, _starts

UNVARIED = [n for n in FIXTURES if "__" not in n]
SAMPLED = ["s3_k8__drop30", "s3_k8__zero02", "s3_k8__zero2", "s3_k8__shift", "s3_k8__mrl10"]      # 500 recorded calls each, not every start
NEVER_ENDING = {"c1_k21__shift": 18, "ragged_k31__drop30": 13, "s3_k24_long__drop70": 11, "s3_k20__shift": 10, "twohash_k31_L150__shift": 7,
                "s3_k20__drop30": 2, "s3_k20__drop70": 2, "c1_k21__drop70": 1, "s3_k24_long__drop30": 1}
_chains = {}


def cov_of(fx):
    return {int(x): [int(v) for v in c] for x, c in zip(fx.keys, fx.recs["cov"])}


def chains_of(name):
    """[(start, index, Contig or None where a call was not recorded)] from every recorded start of a fixture; made once, shared, left unchanged"""
    if name not in _chains:
        fx = _fixture(name)
        cov, fn, out = cov_of(fx), R.recorded(fx.calls), []
        for e in fx.calls:
            start = int(e["start"], 16)
            try:
                out.append((start, e["index"], R.get_contig(fn, cov, fx.case.k, start, e["index"])))
            except R.NotRecorded:
                out.append((start, e["index"], None))
        _chains[name] = out
    return _chains[name]


def test_the_outcomes_of_every_recorded_start():
    assert len(UNVARIED) == 13 and sum(len(chains_of(name)) for name in FIXTURES) == 16101
    total, never = collections.Counter(), {}
    for name in FIXTURES:
        cov = cov_of(_fixture(name))
        for start, _, c in chains_of(name):
            if c is None:
                assert name in SAMPLED, name
                total["not recorded"] += 1
            elif c.status == 0:
                closed = c.end_node and c.end_kmer == start and R.paths_out(cov[c.end_kmer]) == 1
                total["start" if closed else "complex" if c.end_node else "sink"] += 1
                assert R.paths_out(cov[c.end_kmer]) != 1 if c.end_node and not closed else True
                assert len(c.distances) == len(c.kills) + 1 and len(c.coverages) == len(c.distances) + (1 if c.end_node else 0)
            else:
                assert c.status in (1, 3)
                total[c.status] += 1
                if c.status == 3:
                    never[name] = never.get(name, 0) + 1
    assert total == {"complex": 7957, "sink": 4385, "start": 631, 1: 1533, "not recorded": 1530, 3: 65}
    assert never == NEVER_ENDING
    assert max(len(c.string) for name in FIXTURES for _, _, c in chains_of(name) if c) == 6026


def test_chains_between_complex_junctions_read_the_same_from_both_ends():
    """a check of the restatement that does not rest on itself: on the maps as the scan left them, the chain from a complex junction to a
    complex junction is the chain walked back from there -- same ends and indices, reverse-complemented string, reversed distances"""
    n = 0
    for name in UNVARIED:
        fx = _fixture(name)
        cov, fn, k = cov_of(fx), R.recorded(fx.calls), fx.case.k
        for start, index in zip(*stage3.branching_starts(fx.keys, fx.recs, k)):
            start, index = int(start), int(index)
            c = R.get_contig(fn, cov, k, start, index)
            if c.status == 0 and c.end_node and R.paths_out(cov[c.end_kmer]) > 1:
                b = R.get_contig(fn, cov, k, c.end_kmer, c.ind2)
                assert (b.status, b.end_kmer, b.end_node, b.ind1, b.ind2) == (0, start, 1, c.ind2, c.ind1), (name, start, index)
                assert b.string == R.revcomp_string(c.string) and b.distances == c.distances[::-1], (name, start, index)
                n += 1
    assert n >= 1000


@pytest.mark.parametrize("name", ["c1_k21", "s3_k8", "s3_k24_long", "c1_k21__shift", "c1_k21__zero02"])
def test_host_walker_chains_equal_the_restatement(name):
    fx = _fixture(name)
    w = stage3.NeighborWalker(_OracleProbe(fx.case, fx.bloom), fx.keys, fx.recs, fx.case.k, fx.max_read_length)
    want = chains_of(name)
    assert all(c is not None for _, _, c in want)
    got = w.contigs(*_starts(fx.calls))
    assert len(got) == len(want) and w.rounds >= max(len(c.distances) for _, _, c in want)        # one round of calls per chain segment
    for g, (start, index, c) in zip(got, want):
        assert g["status"] == c.status, (start, index)
        assert (g["ind1"], g["ind2"], g["end_kmer"], g["end_node"], g["string"], g["distances"], g["coverages"], g["kills"]) == tuple(c[1:]), (start, index)
    missing = next(x for x in range(len(fx.keys) + 1) if x not in set(int(v) for v in fx.keys))
    bad = w.contigs(np.array([fx.keys[0], missing], dtype=np.uint64), [5, 0])
    assert [b["status"] for b in bad] == [2, 2]


def _hand_map(k, rows):
    keys = np.array([sum(R.NT.index(ch) << (2 * (k - 1 - i)) for i, ch in enumerate(s)) for s, _ in rows], dtype=np.uint64)
    recs = np.zeros(len(rows), dtype=api.JUNC_DTYPE)
    recs["cov"] = [c for _, c in rows]
    return keys, recs


@pytest.mark.parametrize("k, rows", [
    (5, [("ACGTA", (3, 0, 2, 0)), ("AAAAA", (4, 1, 0, 7)), ("CCCCC", (0, 9, 0, 2)), ("GGGGG", (0, 0, 5, 0)), ("TTTTT", (1, 1, 1, 1)), ("ACCTG", (0, 0, 0, 0)),
         ("GATTA", (0, 0, 0, 6)), ("TGCAT", (255, 255, 255, 255))]),
    (4, [("AAAA", (2, 0, 0, 0)), ("CCCC", (1, 1, 0, 0)), ("CACA", (0, 3, 3, 3)), ("TTTT", (0, 0, 8, 0)), ("GGGT", (0, 0, 0, 0))])])
def test_start_lists_against_the_reference_loops(k, rows):
    """buildBranchingPaths :36-50 and buildLinearRegions :105-118 on hand-made maps: complex, simple and dead junctions, and homopolymer k-mers
    whose own base's extension is left out (with the sum of the others as the backward coverage: CCCC's single other extension still starts
    at 4, a homopolymer with one path out is not touched)"""
    keys, recs = _hand_map(k, rows)
    got = stage3.branching_starts(keys, recs, k)
    want = R.branching_starts_ref(keys, recs["cov"], k)
    assert want and [(int(a), int(b)) for a, b in zip(*got)] == want
    assert any(len(set(R.print_kmer(x, k))) == 1 for x, _ in want)
    got = stage3.linear_starts(keys, recs)
    want = R.linear_starts_ref(keys, recs["cov"])
    assert want and [(int(a), int(b)) for a, b in zip(*got)] == want
