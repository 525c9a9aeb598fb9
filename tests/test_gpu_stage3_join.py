"""Contigs joined on the device (faucet_amd/csrc/stage3_join.hip): fgpu_stage3_join on the hand-made lists of tests/join_cases.py against the
restatement (tests/detip_ref.py) and against what the compiled reference's ContigJuncList made of them (tests/golden/join_concat.json.gz), at
k = 8, 21 and 31; on the arrays of a build left on the device; the edges of the call.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import detip_ref as J
from tests.join_cases import cases
from tests.test_join_ref_cpu import KS, same_as_golden

pytestmark = pytest.mark.gpu
_ctx, _packed_of = {}, {}


def _context(k):
    from faucet_amd import api
    if k not in _ctx:
        _ctx[k] = api.Context(k, 1 << 19, 3)
    return _ctx[k]


def _packed(k):
    if k not in _packed_of:
        _packed_of[k] = J.pack(cases(k).contigs)
    return _packed_of[k]


def _joined(ctx, t, lists, **kw):
    return ctx.stage3_join(lists, *_packed(t.k), **kw)


def _as_tuples(got):
    _, strings, dists, covs, avgs = got
    return [(s, d.tolist(), c.tolist(), float(a)) for s, d, c, a in zip(strings, dists, covs, avgs)]


@pytest.mark.parametrize("k", KS)
def test_join_of_hand_made_lists_equals_the_restatement_and_the_reference(k):
    t, ctx = cases(k), _context(k)
    got = _as_tuples(_joined(ctx, t, t.lists))
    assert got == J.join(t.contigs, t.lists, k)
    same_as_golden(k, t.names, got)
    assert [g[0] for g in got] == t.masters
    # the layout: every string from a word of its own in list order, the bits behind `len` zero; the two lists dense, in list order
    rec, text, dist, cov = _joined(ctx, t, t.lists, raw=True)
    words = (rec["len"].astype(np.uint64) + np.uint64(31)) // np.uint64(32)
    assert rec["text_word"].tolist() == (np.cumsum(words) - words).tolist() and len(text) == int(words.sum())
    assert rec["dist_first"].tolist() == (np.cumsum(rec["n_dist"]) - rec["n_dist"]).tolist() and len(dist) == int(rec["n_dist"].sum())
    assert rec["cov_first"].tolist() == (np.cumsum(rec["n_cov"]) - rec["n_cov"]).tolist() and len(cov) == int(rec["n_cov"].sum())
    for r in rec:
        used = int(r["len"]) - 32 * ((int(r["len"]) - 1) // 32)                # bases in the string's last word
        assert int(text[int(r["text_word"]) + (int(r["len"]) - 1) // 32]) >> (2 * used) == 0
        assert int(r["cov_sum"]) == int(cov[int(r["cov_first"]):int(r["cov_first"]) + int(r["n_cov"])].sum(dtype=np.uint64))


@pytest.mark.parametrize("k", (8, 31))
def test_join_of_every_list_alone_and_of_slices(k):
    """other word offsets and other running sums for the same lists: each named list in a call of its own, some runs of lists, the reversed lists"""
    t, ctx = cases(k), _context(k)
    want = J.join(t.contigs, t.lists, k)
    named = [i for i, name in enumerate(t.names) if not name.startswith("random")]
    for i in named:
        assert _as_tuples(_joined(ctx, t, [t.lists[i]])) == [want[i]], t.names[i]
    for lo, hi in ((3, 9), (len(named) - 2, len(named) + 20), (50, 51)):
        assert _as_tuples(_joined(ctx, t, t.lists[lo:hi])) == want[lo:hi]
    back = [J.reverse_list(p) for p in t.lists]
    assert _as_tuples(_joined(ctx, t, back)) == J.join(t.contigs, back, k)


def test_join_of_no_lists():
    from faucet_amd import api
    t, ctx = cases(21), _context(21)
    rec, text, dist, cov = _joined(ctx, t, [], raw=True)
    assert len(rec) == len(text) == len(dist) == len(cov) == 0
    rec, text, dist, cov = ctx.stage3_join([], np.zeros(0, dtype=api.CONTIG_DTYPE), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), raw=True)
    assert len(rec) == len(text) == len(dist) == len(cov) == 0


def _raw_call(ctx, first, pieces, contigs, text, dist, cov):
    from faucet_amd import api
    first, pieces = np.ascontiguousarray(first, dtype=np.uint64), np.ascontiguousarray(pieces, dtype=api.JOIN_PIECE_DTYPE)
    out = np.zeros(max(len(first) - 1, 1), dtype=api.JOINED_DTYPE)
    totals = (C.c_uint64 * 3)(7, 7, 7)
    rc = ctx.lib.fgpu_stage3_join(ctx.h, first.ctypes.data, len(first) - 1, pieces.ctypes.data, len(pieces), contigs.ctypes.data, len(contigs), text.ctypes.data, len(text),
                                  dist.ctypes.data, len(dist), cov.ctypes.data, len(cov), out.ctypes.data, totals)
    return rc, list(totals), out


def test_join_refuses_lists_it_cannot_read():
    from faucet_amd import _lib as L
    from faucet_amd import api
    k = 21
    t, ctx = cases(k), _context(k)
    contigs, text, dist, cov = _packed(k)
    lists = t.lists
    first = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.uint64)
    pieces = np.array([(c, int(f)) for p in lists for c, f in p], dtype=api.JOIN_PIECE_DTYPE)
    rc, totals, _ = _raw_call(ctx, first, pieces, contigs, text, dist, cov)
    assert rc == L.OK and totals[0] > 0 and totals[2] > 0
    two = next(i for i, p in enumerate(lists) if len(p) == 2)
    row = int(pieces["call"][int(first[two])])                                # the first piece of a list of two

    def refused(first=first, pieces=pieces, contigs=contigs, text=text, dist=dist, cov=cov):
        rc, totals, _ = _raw_call(ctx, first, pieces, contigs, text, dist, cov)
        return rc == L.ERR_ARG and totals == [0, 0, 0] and b"fgpu_stage3_join" in ctx.lib.fgpu_last_error(ctx.h)
    for field, value in (("text_word", len(text)), ("len", 32 * len(text) + 1), ("len", 0), ("len", 1 << 30), ("seg_first", len(dist) + 1), ("n_seg", len(dist) + 1),
                         ("cov_first", len(cov)), ("n_cov", len(cov) + 1), ("n_cov", 0), ("len", k - 1)):    # past an array; no bases; no coverage; a joined piece below k
        bad = contigs.copy()
        bad[field][row] = value
        assert refused(contigs=bad), (field, value)
    assert refused(text=text[:-1]) and refused(dist=dist[:-1]) and refused(cov=cov[:-1])      # the arrays end before the last contig does
    for what, value in (("call", len(contigs)), ("flip", 2)):
        bad = pieces.copy()
        bad[what][3] = value
        assert refused(pieces=bad), what
    for bad in (first[:-1], np.concatenate([first[:5], first[4:]]), first + np.uint64(1), np.concatenate([first[:-1], [first[-1] + 1]])):   # not a CSR of the pieces; an empty list
        assert refused(first=np.ascontiguousarray(bad, dtype=np.uint64)), bad
    totals = (C.c_uint64 * 3)()
    out = np.zeros(len(lists), dtype=api.JOINED_DTYPE)
    assert ctx.lib.fgpu_stage3_join(ctx.h, first.ctypes.data, len(lists), pieces.ctypes.data, len(pieces), None, 0, None, 0, None, 0, None, 0, out.ctypes.data,
                                    totals) == L.ERR_STATE                    # no build whose contigs the pieces could index
    assert ctx.lib.fgpu_stage3_join(ctx.h, first.ctypes.data, len(lists), pieces.ctypes.data, len(pieces), None, 0, text.ctypes.data, len(text), None, 0, None, 0,
                                    out.ctypes.data, totals) == L.ERR_ARG
    # ... and none of this touched the results of the call that went through
    jt, jd, jc = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    assert ctx.lib.fgpu_stage3_join_take(ctx.h, jt.ctypes.data, 1, jd.ctypes.data, 1, jc.ctypes.data, 1) == L.ERR_ARG


def test_join_take_with_short_buffers_copies_nothing_and_keeps_the_results():
    from faucet_amd import _lib as L
    k = 21
    t, ctx = cases(k), _context(k)
    want = _joined(ctx, t, t.lists, raw=True)
    contigs, text, dist, cov = _packed(k)
    from faucet_amd import api
    first = np.concatenate([[0], np.cumsum([len(p) for p in t.lists])]).astype(np.uint64)
    pieces = np.array([(c, int(f)) for p in t.lists for c, f in p], dtype=api.JOIN_PIECE_DTYPE)
    rc, (nt, nd, nc), _ = _raw_call(ctx, first, pieces, contigs, text, dist, cov)
    assert rc == L.OK and (nt, nd, nc) == (len(want[1]), len(want[2]), len(want[3]))
    jt, jd, jc = np.full(nt + 2, 0x5A5A, dtype=np.uint64), np.full(nd + 2, 0x5A, dtype=np.uint8), np.full(nc + 2, 0x5A, dtype=np.uint8)

    def take(a, b, c):
        return ctx.lib.fgpu_stage3_join_take(ctx.h, jt.ctypes.data, a, jd.ctypes.data, b, jc.ctypes.data, c)
    for short in ((nt - 1, nd, nc), (nt, nd - 1, nc), (nt, nd, nc - 1)):
        assert take(*short) == L.ERR_ARG
        assert (jt == 0x5A5A).all() and (jd == 0x5A).all() and (jc == 0x5A).all()
    assert take(nt, nd, nc) == L.OK
    assert jt[:nt].tobytes() == want[1].tobytes() and jd[:nd].tobytes() == want[2].tobytes() and jc[:nc].tobytes() == want[3].tobytes()
    assert (jt[nt:] == 0x5A5A).all() and (jd[nd:] == 0x5A).all() and (jc[nc:] == 0x5A).all()
    assert take(0, 0, 0) == L.OK                                               # taken: nothing left


def test_join_over_the_build_left_on_the_device():
    """contigs == NULL: the pieces index the build's own calls.  The lists are what the reference joins at the end of the build -- per linear
    region backward->concatenate(forward, 1, 1) (utils/JunctionMap.cpp:120): the backward chain reversed, then the forward one -- and a few
    longer ones over the same contigs; the build is still there afterwards, and unchanged."""
    from faucet_amd import api
    from tests.test_gpu_raw_contigs import _take_build
    from tests.test_raw_contigs_ref_cpu import golden_build
    from tests.test_stage3_walker import _device, _fixture
    name = "twohash_k31_L150"
    keys, recs = golden_build(name)[1:3]
    fx = _fixture(name)
    ctx = _device(name)
    k = fx.case.k
    ctx.stage3_set_junctions(keys, recs)
    out, calls, strings, dists, covs, _, info = ctx.stage3_build(fx.max_read_length)
    assert info["status"] == 0
    contigs = [(s, d.tolist(), c.tolist()) for s, d, c in zip(strings, dists, covs)]
    forward = [i for i in range(len(calls) - 1) if calls["phase"][i] == api.BUILD_LINEAR_FORWARD and calls["phase"][i + 1] == api.BUILD_LINEAR_BACKWARD]
    assert forward
    lists = [[(i + 1, True), (i, False)] for i in forward]
    long_enough = [i for i in range(len(contigs)) if len(contigs[i][0]) >= k]
    lists += [[(c, bool((c + j) & 1)) for c in long_enough[j:j + 6]] for j in range(0, len(long_enough), 5)]     # (no overlaps here: the join does not ask for them)
    built = ctx.stage3_build(fx.max_read_length, take=False)
    got = _as_tuples(ctx.stage3_join(lists))
    assert got == J.join(contigs, lists, k)
    for (s, _, _, _), i in zip(got, forward):                                  # the two chains of a region do overlap: by the start k-mer
        assert J.R.revcomp_string(contigs[i + 1][0])[-k:] == contigs[i][0][:k] and len(s) == len(contigs[i + 1][0]) + len(contigs[i][0]) - k
    kept = _take_build(ctx, built["totals"])
    fresh = ctx.stage3_build(fx.max_read_length, raw=True)
    assert all(a.tobytes() == f.tobytes() for a, f in zip(kept, fresh[:6]))
