"""fgpu_stage3_contigs (whole JunctionMap::getContig chains on the device, many starts per call) against tests/contig_ref.py chained over the
reference's RECORDED findNeighbor answers (tests/golden/stage3_neighbors_*.jsonl.gz) -- never over the device's own: status, indices, end,
string, distances, coverages and kill list of every chain from every recorded start of every fixture, the layout of the text, and the edges
of the call."""
import ctypes as C

import numpy as np
import pytest

from faucet_amd import stage3
from tests import contig_ref as R
from tests.test_contig_ref_cpu import SAMPLED, chains_of
from tests.test_stage3_walker import FIXTURES, _device, _fixture, _starts

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5A5A5A5A5


def _same_as_restatement(want, out, strings, dists, covs, kills):
    """every chain the restatement decides; returns how many"""
    n = 0
    for i, (start, index, c) in enumerate(want):
        if c is None:
            continue
        g = out[i]
        assert int(g["status"]) == c.status, (start, index)
        got = (int(g["ind1"]), int(g["ind2"]), int(g["end_kmer"]), int(g["end_node"]), strings[i], dists[i].tolist(), covs[i].tolist(), kills[i].tolist())
        assert got == tuple(c[1:]), (start, index)
        assert (int(g["len"]), int(g["n_seg"]), int(g["n_cov"])) == (len(c.string), len(c.distances), len(c.coverages)), (start, index)
        n += 1
    return n


def _device_with_map(name):
    fx = _fixture(name)
    ctx = _device(name)
    ctx.stage3_set_junctions(fx.keys, fx.recs)
    return fx, ctx


@pytest.mark.parametrize("name", FIXTURES)
def test_chains_from_every_recorded_start_against_the_restatement(name):
    fx, ctx = _device_with_map(name)
    want = chains_of(name)
    res = ctx.stage3_contigs(*_starts(fx.calls), fx.max_read_length)
    checked = _same_as_restatement(want, *res[:5])
    if name in SAMPLED:
        assert checked >= 100
    else:
        assert checked == len(want)
    assert res[5] > 0


def test_text_layout_offsets_word_edges_and_untouched_words():
    """text_word ascending, one contig after the other; strings that end one base before, at and one base behind a word's edge; the bits behind
    `len` zero; and the words between two contigs -- there are none, so every word of the text belongs to exactly one contig, and the word
    behind the last stays as the caller left it"""
    edge = 0
    for name in ("c1_k21", "s3_k24_long__drop70", "s3_k8", "twohash_k31_L150__drop30"):
        fx, ctx = _device_with_map(name)
        starts, idx = _starts(fx.calls)
        out, text, kmers, dist, cov, _ = ctx.stage3_contigs(starts, idx, fx.max_read_length, raw=True)
        words = (out["len"].astype(np.uint64) + np.uint64(31)) // np.uint64(32)
        assert np.array_equal(out["text_word"], np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.uint64)) and len(text) == int(words.sum())
        assert np.array_equal(out["seg_first"], np.concatenate([[0], np.cumsum(out["n_seg"].astype(np.uint64))[:-1]]).astype(np.uint64)) and len(kmers) == len(dist) == int(out["n_seg"].sum())
        assert np.array_equal(out["cov_first"], np.concatenate([[0], np.cumsum(out["n_cov"].astype(np.uint64))[:-1]]).astype(np.uint64)) and len(cov) == int(out["n_cov"].sum())
        assert (np.diff(out["text_word"].astype(np.int64)) >= 0).all()
        for c in out[out["len"] % 32 != 0]:
            last = int(text[int(c["text_word"]) + int(c["len"]) // 32])
            assert last >> (2 * (int(c["len"]) % 32)) == 0
        edge += int(((out["len"] > 0) & np.isin(out["len"] % 32, (31, 0, 1))).sum())
        # the same call into arrays with a margin: nothing behind the totals is written
        totals = (C.c_uint64 * 3)()
        again = np.zeros(len(starts), dtype=out.dtype)
        assert ctx.lib.fgpu_stage3_contigs(ctx.h, starts.ctypes.data, idx.ctypes.data, len(starts), fx.max_read_length, again.ctypes.data, totals, None) == 0
        assert list(totals) == [len(text), len(dist), len(cov)] and again.tobytes() == out.tobytes()
        t2, k2 = np.full(len(text) + 3, FILL, dtype=np.uint64), np.full(len(kmers) + 3, FILL, dtype=np.uint64)
        d2, c2 = np.full(len(dist) + 3, 0x5A, dtype=np.uint8), np.full(len(cov) + 3, 0x5A, dtype=np.uint8)
        assert ctx.lib.fgpu_stage3_contigs_take(ctx.h, t2.ctypes.data, len(t2), k2.ctypes.data, d2.ctypes.data, len(d2), c2.ctypes.data, len(c2)) == 0
        assert np.array_equal(t2[:-3], text) and np.array_equal(k2[:-3], kmers) and np.array_equal(d2[:-3], dist) and np.array_equal(c2[:-3], cov)
        assert (t2[-3:] == FILL).all() and (k2[-3:] == FILL).all() and (d2[-3:] == 0x5A).all() and (c2[-3:] == 0x5A).all()
    assert edge >= 5


def test_no_start_one_start_and_starts_that_are_none():
    name = "c1_k21"
    fx, ctx = _device_with_map(name)
    want = chains_of(name)
    out, strings, dists, covs, kills, probes = ctx.stage3_contigs(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int8), fx.max_read_length)
    assert len(out) == 0 and strings == [] and probes == 0
    totals = (C.c_uint64 * 3)(7, 7, 7)
    assert ctx.lib.fgpu_stage3_contigs(ctx.h, None, None, 0, fx.max_read_length, None, totals, None) == 0 and list(totals) == [0, 0, 0]
    assert ctx.lib.fgpu_stage3_contigs_take(ctx.h, None, 0, None, None, 0, None, 0) == 0
    pick = next(i for i, (_, _, c) in enumerate(want) if c.status == 0 and len(c.distances) >= 3)
    start, index, c = want[pick]
    res = ctx.stage3_contigs([start], [index], fx.max_read_length)
    assert _same_as_restatement([want[pick]], *res[:5]) == 1 and int(res[0]["text_word"][0]) == 0
    missing = next(x for x in range(len(fx.keys) + 1) if x not in set(int(v) for v in fx.keys))
    res = ctx.stage3_contigs([start, missing, start, start], [index, 0, 5, -1], fx.max_read_length)
    assert res[0]["status"].tolist() == [0, 2, 2, 2]
    assert _same_as_restatement([want[pick]] + [(0, 0, R.failed(2))] * 3, *res[:5]) == 4


def test_starts_repeated_over_block_and_grid_edges_scale_exactly():
    """one call with the same starts repeated to 266 and to 65 550 entries (more than one block; more than 256 blocks with a last block and a last
    wave partly empty): every copy's entry equals the first but for its offsets, the arrays repeat, the totals scale exactly"""
    name = "twohash_k31_L150__shift"
    fx, ctx = _device_with_map(name)
    every = chains_of(name)
    pick = list(range(0, len(every), 13))
    pick[-1] = next(i for i, (_, _, c) in enumerate(every) if c.status == 3)          # (every status in the 38)
    want = [every[i] for i in pick]
    starts, idx = (a[pick] for a in _starts(fx.calls))
    assert len(starts) == 38 and {c.status for _, _, c in want} == {0, 1, 3}
    one = ctx.stage3_contigs(starts, idx, fx.max_read_length, raw=True)
    assert _same_as_restatement(want, *ctx.stage3_contigs(starts, idx, fx.max_read_length)[:5]) == 38
    calls = {1: one[5]}
    for reps in (7, 65536 // 38 + 1):
        out, text, kmers, dist, cov, probes = ctx.stage3_contigs(np.tile(starts, reps), np.tile(idx, reps), fx.max_read_length, raw=True)
        assert len(out) == 38 * reps and (reps == 7 or (len(out) > 65536 and len(out) % 64))
        for f in out.dtype.names:
            got = out[f].reshape(reps, 38)
            if f in ("text_word", "seg_first", "cov_first"):
                per = {"text_word": len(one[1]), "seg_first": len(one[3]), "cov_first": len(one[4])}[f]
                assert np.array_equal(got, one[0][f][None, :] + (np.arange(reps, dtype=np.uint64) * np.uint64(per))[:, None]), f
            else:
                assert (got == one[0][f][None, :]).all(), f
        assert np.array_equal(text, np.tile(one[1], reps)) and np.array_equal(kmers, np.tile(one[2], reps))
        assert np.array_equal(dist, np.tile(one[3], reps)) and np.array_equal(cov, np.tile(one[4], reps))
        calls[reps] = probes
    # the probes of a call: the map's segments once, whatever the number of starts, and each start's own first segment
    per_copy = (calls[7] - calls[1]) // 6
    assert 0 < per_copy <= calls[1] and all(p == calls[1] + (reps - 1) * per_copy for reps, p in calls.items())


def test_take_with_an_array_one_entry_short_keeps_the_results():
    from faucet_amd import _lib as L
    name = "s3_k20"
    fx, ctx = _device_with_map(name)
    starts, idx = _starts(fx.calls)
    want = ctx.stage3_contigs(starts, idx, fx.max_read_length, raw=True)
    out = np.zeros(len(starts), dtype=want[0].dtype)
    totals = (C.c_uint64 * 3)()
    assert ctx.lib.fgpu_stage3_contigs(ctx.h, starts.ctypes.data, idx.ctypes.data, len(starts), fx.max_read_length, out.ctypes.data, totals, None) == L.OK
    nt, ns, nc = list(totals)
    assert (nt, ns, nc) == (len(want[1]), len(want[3]), len(want[4])) and min(nt, ns, nc) > 1
    text, kmers = np.full(nt, FILL, dtype=np.uint64), np.full(ns, FILL, dtype=np.uint64)
    dist, cov = np.full(ns, 0x5A, dtype=np.uint8), np.full(nc, 0x5A, dtype=np.uint8)
    for short in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        rc = ctx.lib.fgpu_stage3_contigs_take(ctx.h, text.ctypes.data, nt - short[0], kmers.ctypes.data, dist.ctypes.data, ns - short[1], cov.ctypes.data, nc - short[2])
        assert rc == L.ERR_ARG
        assert (text == FILL).all() and (kmers == FILL).all() and (dist == 0x5A).all() and (cov == 0x5A).all()
    assert ctx.lib.fgpu_stage3_contigs_take(ctx.h, text.ctypes.data, nt, kmers.ctypes.data, dist.ctypes.data, ns, cov.ctypes.data, nc) == L.OK
    assert out.tobytes() == want[0].tobytes()
    assert np.array_equal(text, want[1]) and np.array_equal(kmers, want[2]) and np.array_equal(dist, want[3]) and np.array_equal(cov, want[4])


def test_a_new_map_gives_new_answers():
    """stage3_set_junctions again, on the same context: the chains follow the new map (the thinned one, under the same filter)"""
    fx, ctx = _device_with_map("c1_k21")
    res = ctx.stage3_contigs(*_starts(fx.calls), fx.max_read_length)
    assert _same_as_restatement(chains_of("c1_k21"), *res[:5]) == len(fx.calls)
    thin = _fixture("c1_k21__drop30")
    assert np.array_equal(thin.bloom, fx.bloom) and len(thin.keys) < len(fx.keys)
    ctx.stage3_set_junctions(thin.keys, thin.recs)
    res = ctx.stage3_contigs(*_starts(thin.calls), thin.max_read_length)
    assert _same_as_restatement(chains_of("c1_k21__drop30"), *res[:5]) == len(thin.calls)
    lost = [i for i, e in enumerate(fx.calls) if int(e["start"], 16) not in set(int(v) for v in thin.keys)]
    starts, idx = _starts(fx.calls)
    assert lost and (ctx.stage3_contigs(starts[lost], idx[lost], fx.max_read_length)[0]["status"] == 2).all()


def test_linear_regions_of_a_map_without_complex_junctions():
    """s3_k24_long__drop70: no junction with more than one path out; buildLinearRegions' starts give closed loops, sinks, and the chains on which
    the reference never returns"""
    name = "s3_k24_long__drop70"
    fx, ctx = _device_with_map(name)
    assert len(stage3.branching_starts(fx.keys, fx.recs, fx.case.k)[0]) == 0
    starts, idx = stage3.linear_starts(fx.keys, fx.recs)
    cov, fn = {int(x): [int(v) for v in c] for x, c in zip(fx.keys, fx.recs["cov"])}, R.recorded(fx.calls)
    want = [(int(s), int(i), R.get_contig(fn, cov, fx.case.k, int(s), int(i))) for s, i in zip(starts, idx)]
    res = ctx.stage3_contigs(starts, idx, fx.max_read_length)
    assert _same_as_restatement(want, *res[:5]) == len(want)
    status = res[0]["status"]
    assert int((status == 3).sum()) == 11 and int(((status == 0) & (res[0]["end_node"] == 1)).sum()) == 29
