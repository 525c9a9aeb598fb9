"""The pure stage's back half issued by ranges: results must not depend on the range size at all.  FGPU_SCAN_RANGE_LOG2
(read once per scan) forces ranges of 2^n positions -- at 256 positions a range holds two or three reads of the goldens, so pieces straddle range
ends, windows read past them and the batch's events are used several times over -- and 0 forces one range per batch.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from oracle import pyoracle as po
from tests.golden_util import CASES, Case
from tests.test_gpu_parity import _oracle_lists, _random_case, _scan_equals_oracle, chunks, oracle_run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = (("n_junctions", "distinct_junctions"), ("nb_jcheck_kmer", "nb_jcheck_kmer"), ("nb_processed", "nb_processed"), ("nb_skipped", "nb_skipped"),
            ("reads_processed", "scan_reads_processed"))
_reference = {}


def _case(name):
    """the golden, its reads and the oracle's junctions in creation order: made once per case, shared and left unchanged"""
    if name not in _reference:
        c = Case(name)
        bases, offs = po.reads_from_lines(c.lines())
        tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
        b2 = po.Bloom(tai, nh)
        b2.set_bits(c.bloom())
        osc = po.Scanner(c.k, c.j, c.spacer, b2)
        osc.scan_reads(bases, offs, paired_ends=False, no_cleaning=True)
        okeys, orecs = osc.junctions("creation")
        _reference[name] = (c, bases, offs, tai, nh, okeys, po.junction_lines(okeys, orecs, c.k))
    return _reference[name]


def _scan_golden(name, n_batches, span, eager=False):
    c, bases, offs, tai, nh, okeys, olines = _case(name)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, walk_window_span=span, eager_flags=eager)
    ctx.bloom_upload(L.BLOO2, c.bloom())
    sc = api.ReadScanner(ctx)
    st = sc.scanReads(chunks(bases, offs, n_batches))
    keys, recs = sc.junctions()
    lines = api.junction_lines(keys, recs, c.k)
    ctx.close()
    what = (name, n_batches, span, eager)
    for got, want in COUNTERS:
        assert st[got] == c.counters[want], (got, what)
    assert sorted(lines) == sorted(c.junction_lines()), what
    assert np.array_equal(keys, okeys) and lines == olines, what      # creation order: a function of piece number and half-step, not of the schedule
    return st


@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
@pytest.mark.parametrize("name", CASES)
def test_forced_small_ranges_give_the_goldens(name, eager, monkeypatch):
    for log2 in ("8", "12"):
        monkeypatch.setenv("FGPU_SCAN_RANGE_LOG2", log2)
        for span in (256, 1 << 16):
            for n_batches in (1, 5):
                _scan_golden(name, n_batches, span, eager)


@pytest.mark.parametrize("name", ["ragged_k31", "j2_spacer20_k15"])
def test_one_range_per_batch_is_the_old_schedule_and_gives_the_same(name, monkeypatch):
    monkeypatch.setenv("FGPU_SCAN_RANGE_LOG2", "0")
    for n_batches, span in ((1, 0), (5, 256)):
        _scan_golden(name, n_batches, span)


@pytest.mark.parametrize("value", ["", "5", "x", "12q", "41"])
def test_a_value_of_the_knob_without_a_meaning_is_refused(value, monkeypatch):
    monkeypatch.setenv("FGPU_SCAN_RANGE_LOG2", value)
    ctx = api.Context(21, 1 << 20, 3)
    with pytest.raises(Exception, match="FGPU_SCAN_RANGE_LOG2"):
        ctx.scan_begin()
    monkeypatch.setenv("FGPU_SCAN_RANGE_LOG2", "0")
    ctx.scan_begin()
    ctx.scan_end()
    ctx.close()


def test_pure_stage_far_ahead_of_a_stalled_walk_with_small_ranges(monkeypatch):
    """24 small batches, the walk stream held up 3 ms before every batch's walk, ranges of 1024 positions: the pure stage of the batches behind runs
    as far ahead of the walk as the host lets it, and every window still finds its ranges complete and the keys created since registered."""
    bases, offs = _random_case(30000, 100, 31, 40000, 0.01, 77, 0.0, 3)
    tai, nh = api.load_filter_shape(2_000_000, 400_000)
    b1, b2, lst, osc = oracle_run((bases, offs), 31, tai, nh, 1, 100)
    ctx = api.Context(31, tai, nh)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    monkeypatch.setenv("FGPU_DEBUG_WALK_STALL_US", "3000")
    monkeypatch.setenv("FGPU_SCAN_RANGE_LOG2", "10")
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 24))
    _scan_equals_oracle(sc, sst, osc)
    ctx.close()


def test_stop_lists_taken_after_every_batch_with_forced_ranges(monkeypatch):
    """The harvest waits for walk_done and reads planes of the pure stage: both events still have to mean what they meant."""
    monkeypatch.setenv("FGPU_SCAN_RANGE_LOG2", "8")
    c, bases, offs, tai, nh, okeys, olines = _case("ragged_k31")
    _, want = _oracle_lists(bases, offs, c.k, c.j, c.spacer, c.bloom(), tai, nh)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, record_stops=True, walk_window_span=256)
    ctx.bloom_upload(L.BLOO2, c.bloom())
    parts = chunks(bases, offs, 5)
    got, seqs = [], []

    def take():
        while True:
            t = ctx.take_stops()
            if t is None:
                return
            seq, st = t
            seqs.append(seq)
            lists = [[] for _ in range(parts[seq].n_reads)]
            for e in st:
                lists[int(e["read"])].append(int(e["ext"]))
            got.extend(lists)

    ctx.scan_begin()
    for part in parts:
        ctx.scan_batch(part)
        take()
    st = ctx.scan_end()
    take()
    assert seqs == list(range(len(parts)))
    assert got == want
    keys, recs = ctx.junctions()
    assert np.array_equal(keys, okeys) and api.junction_lines(keys, recs, c.k) == olines
    for g, w in COUNTERS:
        assert st[g] == c.counters[w], g
    ctx.close()


_CHILD = """
import sys
import numpy as np
from faucet_amd import _lib as L, api
from oracle import pyoracle as po
from tests.golden_util import Case
from tests.test_gpu_parity import chunks
c = Case(sys.argv[1])
bases, offs = po.reads_from_lines(c.lines())
tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
for n_batches, span in ((1, 256), (5, 256), (5, 1 << 16)):
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, walk_window_span=span)
    ctx.bloom_upload(L.BLOO2, c.bloom())
    sc = api.ReadScanner(ctx)
    st = sc.scanReads(chunks(bases, offs, n_batches))
    keys, recs = sc.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines()), (n_batches, span)
    for got, want in (("n_junctions", "distinct_junctions"), ("nb_jcheck_kmer", "nb_jcheck_kmer"), ("nb_processed", "nb_processed"),
                      ("nb_skipped", "nb_skipped"), ("reads_processed", "scan_reads_processed")):
        assert st[got] == c.counters[want], (got, n_batches, span, st[got], c.counters[want])
    print("replays", ctx.diag_scan_replays(), "filled", st["flags_filled"])
    ctx.close()
print("ranges ok")
"""


@pytest.mark.parametrize("knob,name", [("FGPU_DEBUG_NEED_DROP", "c1_k21"), ("FGPU_DEBUG_LAZY_FAIL", "ragged_k31")])
def test_preview_repair_and_replay_under_forced_ranges(knob, name):
    """The two debug knobs are read once per process, hence the child.  FGPU_DEBUG_NEED_DROP=1: the evaluation of half of the false tests is
    thrown away range by range and the walk evaluates them itself; FGPU_DEBUG_LAZY_FAIL=1: the lazy scan is voided and the journal replayed (one
    range per batch there) -- the same lines and counters as without either."""
    env = dict(os.environ, FGPU_SCAN_RANGE_LOG2="8")
    env[knob] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD, name], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and "ranges ok" in r.stdout, r.stdout + r.stderr
    if knob == "FGPU_DEBUG_NEED_DROP":
        assert all(int(line.split()[3]) > 0 for line in r.stdout.splitlines() if line.startswith("replays")), r.stdout      # the walk did fill tests in
    else:
        assert all(int(line.split()[1]) == 1 for line in r.stdout.splitlines() if line.startswith("replays")), r.stdout      # every scan was replayed once
