"""ContigGraph::printGraph on the device (faucet_amd/csrc/stage3_fastg.hip, stage3_emit.hip, clean_graph.h): the emitter alone through
fgpu_stage3_fastg on host-made records and text; fgpu_stage3_raw_graph, and fgpu_stage3_graph_fastg behind fgpu_stage3_detip and behind
fgpu_stage3_dechimera, on the 28 golden fixtures and on the seeded maps tests/test_gpu_stage3_fuzz.py uses, against tests/fastg_ref.py over THE
REFERENCE'S graph tables (the goldens' .graph.gz; oracle/_ref/detip_driver and chimera_driver asked on the spot).  Needs an MI355X.

Expected bytes never come from the code under test: the tables are the reference's, the letters are tests/detip_ref.join over the piece lists of the
Python restatements (tests/detip_plan_ref.py, dechimera_plan_ref.py, pinned to the reference elsewhere), and <this> -- a heap address in the
reference, a contig number here -- is renumbered by first appearance on both sides, as tests/test_binding_link.py does with the reference's own
FASTG.  That the number is unique per contig is held by tests/test_fastg_plan_cpu.py on the host plan, and here by the renumbering itself: two
contigs sharing a number would not renumber to the expected text."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import chimera_cases
from tests import dechimera_golden as G
from tests import dechimera_plan_ref as R2
from tests import detip_golden as D
from tests import detip_plan_ref as R1
from tests import detip_ref as J
from tests import fastg_cases as FC
from tests import fastg_ref as F
from tests import raw_contigs_ref as P
from tests import stage3_fuzz_cases as S
from tests.test_raw_contigs_ref_cpu import golden_build
from tests.test_stage3_walker import _device, _fixture

pytestmark = pytest.mark.gpu
NAMES = sorted(G.summary()["fixtures"])
TRAPS = ((200001, 200000), (1601, 16), (1, 100000), (0, 7), (255, 1), (23, 2), (0, 4294967295), (1, 4294967295), (9999995, 10000000), (1, 10000))
SEED = 1


# ---- the emitter alone ----
class HandMade:
    """about 300 records of every length from k to k + 300, neighbour counts 0..4 on each side, contig numbers of 1 to 8 hexadecimal digits and
    summaries from the traps: records, neighbours and text for fgpu_stage3_fastg, and the text tests/fastg_ref.py renders of them"""

    def __init__(self, k, seed, n=301):
        from faucet_amd import api
        rng = np.random.default_rng(seed)
        lengths = [k + i for i in rng.permutation(n)]
        self.seqs = ["".join("ACGT"[v] for v in rng.integers(0, 4, size=m)) for m in lengths]
        self.words, first = P.pack_text(self.seqs)
        tigs = set()
        self.recs = np.zeros(n, dtype=api.FASTG_REC_DTYPE)
        self.neighbours, contigs = [], []
        for i in range(n):
            digits = 1 + i % 8 if i < 64 else 2 + i % 7                        # (only 16 numbers have one digit)
            while True:
                tig = int(rng.integers(16 ** (digits - 1) if digits > 1 else 0, 16 ** digits))
                if tig not in tigs:
                    break
            tigs.add(tig)
            s, m = TRAPS[i % len(TRAPS)] if i % 3 else (int(rng.integers(0, 255 * 50 + 1)), 50)
            self.recs[i] = (tig, first[i], s, lengths[i], m)
            counts = (i % 5, (i // 5) % 5)
            self.neighbours.append(tuple([(int(rng.integers(0, n)), bool(rng.integers(0, 2))) for _ in range(c)] for c in counts))
            contigs.append(F.Contig(lengths[i], 0, 0, None, None, float(s) / float(m), False))
        self.graph = collections.namedtuple("Made", "contigs")(contigs)
        self.ids = [int(t) for t in self.recs["tig"]]

    def expected(self, which=None):
        which = range(len(self.recs)) if which is None else which
        return F.render(self.graph, [F.Record(i, *self.neighbours[i]) for i in which], self.seqs, self.ids)

    def kinds(self):
        """per byte of the expected file: h header, f base of the first strand, b base of the second, n newline"""
        out = []
        for i in range(len(self.recs)):
            lines = F.render(self.graph, [F.Record(i, *self.neighbours[i])], self.seqs, self.ids).decode().split("\n")[:4]
            for ln, kind in zip(lines, "hfhb"):
                out.append(kind * len(ln) + "n")
        return "".join(out)


_made = {}


def made(k):
    if k not in _made:
        _made[k] = HandMade(k, SEED + k)
    return _made[k]


@pytest.mark.parametrize("k", (8, 21, 31))
def test_the_emitter_on_hand_made_records_of_every_length(k):
    h = made(k)
    ctx = _device("c1_k21")
    got = ctx.stage3_fastg(h.recs, h.neighbours, h.words)
    assert got == h.expected()
    assert sorted(int(v) for v in h.recs["len"]) == list(range(k, k + 301))
    assert {(len(a), len(b)) for a, b in h.neighbours} == {(i, j) for i in range(5) for j in range(5)}
    assert {len("%x" % t) for t in h.ids} == set(range(1, 9))


def test_the_hand_made_files_put_every_kind_of_byte_on_both_edges_of_some_tile():
    """from the restated offsets alone: a header byte, a base of each strand and a newline each fall on the first and on the last byte of some tile of the
    text kernel (its tile size is exported)"""
    from faucet_amd import api
    tile = api.FASTG_TILE
    seen = set()
    for k in (8, 21, 31):
        kinds = made(k).kinds()
        assert len(kinds) == len(made(k).expected()) > 20 * tile
        seen |= {(kinds[at], "first") for at in range(0, len(kinds), tile)} | {(kinds[at], "last") for at in range(tile - 1, len(kinds), tile)}
    assert seen == {(kind, edge) for kind in "hfbn" for edge in ("first", "last")}, sorted(seen)


def test_the_emitter_on_no_record_on_one_record_and_what_it_refuses():
    from faucet_amd import _lib as L
    k = 21
    h = made(k)
    ctx = _device("c1_k21")
    assert ctx.stage3_fastg(h.recs[:0], [], h.words) == b""
    shortest = int(np.argmin(h.recs["len"]))
    one = h.recs[shortest:shortest + 1].copy()
    assert int(one["len"][0]) == k
    assert ctx.stage3_fastg(one, [([], [])], h.words) == F.render(h.graph, [F.Record(shortest, [], [])], h.seqs, h.ids)
    assert ctx.stage3_fastg(one, [([(0, True)], [(0, False), (0, True)])], h.words) == \
        F.render(h.graph, [F.Record(shortest, [(shortest, True)], [(shortest, False), (shortest, True)])], h.seqs, h.ids)
    # a file left on the device, and what is refused leaves it there
    nbytes = C.c_uint64(0)
    first = np.array([0, 0, 0], dtype=np.uint64)
    nbr = np.zeros(1, dtype=np.uint32)

    def call(recs=one, n=1, f=first, nb=None, n_nbr=0, words=h.words, n_words=None):
        nbytes.value = 7
        return ctx.lib.fgpu_stage3_fastg(ctx.h, recs.ctypes.data, n, f.ctypes.data, None if nb is None else nb.ctypes.data, n_nbr, words.ctypes.data,
                                         len(words) if n_words is None else n_words, C.byref(nbytes))
    assert call() == L.OK and nbytes.value == len(F.render(h.graph, [F.Record(shortest, [], [])], h.seqs, h.ids))
    kept = nbytes.value
    bad = one.copy()
    bad["len"][0] = 0
    assert call(recs=bad) == L.ERR_ARG and nbytes.value == 0 and b"fgpu_stage3_fastg" in ctx.lib.fgpu_last_error(ctx.h)          # no bases
    bad = one.copy()
    bad["text_word"][0] = len(h.words)
    assert call(recs=bad) == L.ERR_ARG                                         # past the text
    assert call(n_words=int(one["text_word"][0])) == L.ERR_ARG                 # the text ends before the record does
    bad = one.copy()
    bad["cov_n"][0] = 0
    assert call(recs=bad) == L.ERR_ARG                                         # a summary of no entries
    bad["cov_n"][0], bad["cov_sum"][0] = 2, 511
    assert call(recs=bad) == L.ERR_ARG                                         # ... of a sum no two bytes have
    nbr[0] = 1
    assert call(f=np.array([0, 1, 1], dtype=np.uint64), nb=nbr, n_nbr=1) == L.ERR_ARG and b"neighbour" in ctx.lib.fgpu_last_error(ctx.h)      # a neighbour index >= n
    nbr[0] = 1 | L.FASTG_PRIMED
    assert call(f=np.array([0, 0, 1], dtype=np.uint64), nb=nbr, n_nbr=1) == L.ERR_ARG
    nbr[0] = 0
    assert call(f=np.array([0, 1, 0], dtype=np.uint64), nb=nbr, n_nbr=1) == L.ERR_ARG      # no CSR: descending
    assert call(f=np.array([1, 1, 1], dtype=np.uint64), nb=nbr, n_nbr=1) == L.ERR_ARG      # ... not from 0
    assert call(f=np.array([0, 0, 1], dtype=np.uint64), nb=nbr, n_nbr=2) == L.ERR_ARG      # ... not to n_nbr
    five = np.zeros(5, dtype=np.uint32)
    assert call(f=np.array([0, 5, 5], dtype=np.uint64), nb=five, n_nbr=5) == L.ERR_ARG     # more than four neighbours
    assert ctx.stage3_fasta_take(kept) == F.render(h.graph, [F.Record(shortest, [], [])], h.seqs, h.ids)      # nothing was launched: the file is still the one record


# ---- the entry points over a build and over the live graph ----
def renumbered(text):
    """<this> renumbered by first appearance"""
    seen = {}
    return re.sub(rb"NODE_0x[0-9a-f]+_", lambda m: b"NODE_0x%x_" % seen.setdefault(m.group(0), len(seen)), text)


def expected_of(table, lists, calls, k, read_length):
    """(renumbered bytes, info) of tests/fastg_ref.py over a reference table whose contig c joins from lists[c]"""
    joined = J.join(D.triples_of(calls), lists, k) if lists else []
    graph = F.Graph(table)
    assert [(t.bases, "%.17g" % t.avg) for t in graph.contigs] == [(len(j[0]), "%.17g" % j[3]) for j in joined]
    recs, info = F.records(graph, read_length)
    return renumbered(F.render(graph, recs, [j[0] for j in joined], list(range(len(joined))))), info


def raw_lists(calls, keys, cov, k):
    """the piece lists of the contigs of the build's graph, in the order tests/fastg_cases.raw_table writes them"""
    nodes, _, isolated = P.graph_of(calls, keys, cov, k)
    seen, lists = set(), []
    for _, nd in nodes:
        for c in nd.contigs:
            if c is not None and c not in seen:
                seen.add(c)
                lists.append([(c, False)])
    return lists + [[(b, True), (f, False)] for b, f in isolated]


def run_steps(ctx, calls, keys, recs, k, read_length, tables, lists):
    """the three files of one context against the three tables; what fgpu_stage3_graph_fastg must leave alone"""
    from faucet_amd import _lib as L
    ctx.stage3_set_junctions(keys, recs)
    built = ctx.stage3_build(read_length, take=False)
    assert built["status"] == 0 and built["totals"][0] == len(calls)
    want = {step: expected_of(tables[step], lists[step], calls, k, read_length) for step in FC.STEPS}
    raw, raw_info = ctx.stage3_raw_graph(read_length)
    assert (renumbered(raw), raw_info) == want["raw"]
    assert ctx.stage3_raw_graph(read_length) == (raw, raw_info)                  # twice: the same file
    detip_file, tips = ctx.stage3_detip(read_length)
    got, info = ctx.stage3_graph_fastg()
    assert (renumbered(got), info) == want["detip"]
    assert ctx.stage3_graph_fastg() == (got, info)                               # ... and the graph is what it was
    assert ctx.stage3_raw_graph(read_length) == (raw, raw_info)                  # the build too, with a live graph beside it
    chimera_file, ci = ctx.stage3_dechimera()
    got2, info2 = ctx.stage3_graph_fastg()
    assert (renumbered(got2), info2) == want["dechimera"]
    assert ctx.stage3_graph_fastg() == (got2, info2)
    # a contig that survives the step keeps its number, so its name: only collapseNode makes a contig, one per node it takes out
    names = lambda text: set(re.findall(rb">(NODE_0x[0-9a-f]+_length_\d+_cov_[^';:]+)", text))      # noqa: E731
    assert len(names(got2) - names(got)) <= ci["collapsed"][0] + ci["collapsed"][1]
    table = ctx.stage3_graph_take()                                              # the graph behind all of it
    nbytes, fi = C.c_uint64(7), L.FastgInfo()
    assert ctx.lib.fgpu_stage3_graph_fastg(ctx.h, C.byref(nbytes), C.byref(fi)) == L.ERR_STATE and nbytes.value == 0
    assert b"fgpu_stage3_graph_fastg" in ctx.lib.fgpu_last_error(ctx.h)
    # the two steps without a call between them give the same files, info and graph
    assert ctx.stage3_detip(read_length) == (detip_file, tips)
    assert ctx.stage3_dechimera() == (chimera_file, ci)
    plain = ctx.stage3_graph_take()
    assert plain["lists"] == table["lists"] and plain["nodes"].tobytes() == table["nodes"].tobytes() and plain["contigs"].tobytes() == table["contigs"].tobytes()
    return detip_file, chimera_file


@pytest.mark.parametrize("name", NAMES)
def test_the_three_graphs_of_a_golden_fixture_equal_the_restatement_of_the_references_tables(name):
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    k, rl = fx.case.k, fx.max_read_length
    tables = dict(raw=FC.raw_table(b.calls, keys, recs["cov"], k), detip=D.golden(name, "graph").decode(), dechimera=G.golden(name, "graph").decode())
    lists = dict(raw=raw_lists(b.calls, keys, recs["cov"], k), detip=[t[6] for t in R1.plan(b.calls, keys, recs["cov"], k, rl)[1]],
                 dechimera=[t[6] for t in R2.plan(b.calls, keys, recs["cov"], k, rl)[1]])
    detip_file, chimera_file = run_steps(_device(name), b.calls, keys, recs, k, rl, tables, lists)
    assert detip_file == D.golden(name, "fasta") and chimera_file == G.golden(name, "fasta")


@pytest.mark.skipif(not S.chimera_driver_built(), reason="oracle/_ref/faucet_ref and the three Stage-3 drivers were not built (make -C oracle ref)")
@pytest.mark.parametrize("case_id", chimera_cases.GPU_IDS)
def test_the_three_graphs_of_a_seeded_map_with_the_drivers_asked_on_the_spot(case_id):
    from tests.test_gpu_stage3_fuzz import _account, _chimera
    from tests.test_stage3_walker import device_of, fixture_from
    a = _account(case_id)
    m = a.map
    fasta, table = _chimera(case_id)
    calls, cov = a.build.calls, a.recs["cov"]
    tables = dict(raw=FC.raw_table(calls, a.keys, cov, m.k), detip=a.answers.table, dechimera=table)
    lists = dict(raw=raw_lists(calls, a.keys, cov, m.k), detip=[t[6] for t in a.plan.contigs],
                 dechimera=[t[6] for t in R2.plan(calls, a.keys, cov, m.k, m.max_read_length)[1]])
    ctx = device_of(fixture_from(m.bloom, m.lines, m.k, m.n_hash, m.j, m.max_read_length))
    detip_file, chimera_file = run_steps(ctx, calls, a.keys, a.recs, m.k, m.max_read_length, tables, lists)
    assert detip_file == a.answers.detip_fasta and chimera_file == fasta


def test_graph_fastg_needs_a_live_graph_and_its_build():
    from faucet_amd import _lib as L
    name = "c1_k21"
    keys, recs = golden_build(name)[1:3]
    fx = _fixture(name)
    ctx = _device(name)
    nbytes, fi = C.c_uint64(7), L.FastgInfo()

    def call():
        nbytes.value = 7
        return ctx.lib.fgpu_stage3_graph_fastg(ctx.h, C.byref(nbytes), C.byref(fi))
    ctx.stage3_set_junctions(keys, recs)
    ctx.stage3_build(fx.max_read_length, take=False)
    ctx.stage3_detip(fx.max_read_length)
    ctx.stage3_graph_take()
    assert call() == L.ERR_STATE and nbytes.value == 0                          # taken
    ctx.stage3_detip(fx.max_read_length)
    ctx.stage3_build(fx.max_read_length, take=False)                            # another build: the graph is of one that is gone
    assert call() == L.ERR_STATE and b"build" in ctx.lib.fgpu_last_error(ctx.h)
    assert ctx.lib.fgpu_stage3_graph_fastg(ctx.h, None, C.byref(fi)) == L.ERR_ARG
    ctx.stage3_build(fx.max_read_length)                                        # taken: no build for the raw graph either
    assert ctx.lib.fgpu_stage3_raw_graph(ctx.h, fx.max_read_length, C.byref(nbytes), C.byref(fi)) == L.ERR_ARG
    assert b"fgpu_stage3_raw_graph" in ctx.lib.fgpu_last_error(ctx.h)
    ctx.stage3_set_junctions(keys[:0], recs[:0])                                # an empty map
    ctx.stage3_build(fx.max_read_length, take=False)
    assert ctx.stage3_raw_graph(fx.max_read_length) == (b"", dict(node_records=0, isolated_printed=0, isolated_listed=0, nodes=0))
    ctx.stage3_detip(fx.max_read_length)
    assert ctx.stage3_graph_fastg()[0] == b""
