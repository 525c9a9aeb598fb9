"""The dense hand-out of sparse hits in k_walk_link and k_scan_valid (faucet_amd/csrc/dense_hits.h), at the shapes where a round of several
64-position words can go wrong.  Every scan here runs with FGPU_DEBUG_DELTA_CHECK=1: the per-lane form of each kernel runs behind the dense
one and the planes (lk, valid) are compared word for word -- no word may differ -- and the scan must equal the oracle:
junction keys and records in creation order, and the counters.  Needs an MI355X."""
import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api, synth
from oracle import pyoracle as po
from tests.golden_util import Case
from tests.test_gpu_parity import _random_case, _scan_equals_oracle, chunks, oracle_run

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _delta_check(monkeypatch):
    monkeypatch.setenv("FGPU_DEBUG_DELTA_CHECK", "1")      # read at every scan's begin


def _no_word_differs(ctx):
    assert ctx.diag_prepared_refresh()["mismatching_words"] == 0


def _load_and_scan(bases, offs, k, E, S, batches, j=1, span=0, scan_batches=None):
    """load and scan in one context (the scan of the loaded batches takes the load pass's sure plane), against the oracle of the same reads"""
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, j, 100)
    ctx = api.Context(k, tai, nh, j=j, walk_window_span=span)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), batches)
    assert st["kmers"] == lst.kmers and np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits())
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(scan_batches or batches)
    _scan_equals_oracle(sc, sst, osc)
    _no_word_differs(ctx)
    return ctx, sst, b2, osc


# ---- every position hits ----------------------------------------------------------------------------------------------------------------------
def _crowded(k):
    """10 000 reads of 100 bases of a 200-base genome with one substitution in 400 bases: at five-thousand-fold coverage every substitution
    is seen often enough to be in bloo2, so nearly every k-mer of the genome is a junction -- and nine windows in ten are free of errors,
    which is what bounds the share of positions in the map (at one error in 100 bases it is 0.82 / 0.74 for k = 21 / 31)"""
    g = synth.make_genome(200, 40 + k)
    return po.reads_from_matrix(synth.make_reads(g, 10_000, 100, 0.0025, 41 + k))


def _canon_kmers(mat, k):
    """canonical k-mers of every window of an (n, L) matrix of ACGT reads, in the project's 2-bit code (A0 C1 T2 G3)"""
    code = ((mat >> 1) & 3).astype(np.uint64)
    n, L_ = code.shape
    fwd = np.zeros((n, L_ - k + 1), dtype=np.uint64)
    rc = np.zeros_like(fwd)
    for t in range(k):
        fwd |= code[:, t:t + L_ - k + 1] << np.uint64(2 * (k - 1 - t))
        rc |= (code[:, t:t + L_ - k + 1] ^ np.uint64(2)) << np.uint64(2 * t)
    return np.minimum(fwd, rc)


def in_map_share(bases, offs, k, tai, nh):
    """Of the piece positions of a second pass over these reads, the share whose k-mer the first pass left in the junction map (oracle only)."""
    b1, b2, _, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    keys, _ = osc.junctions("creation")
    n = len(offs) - 1
    mat = bases.reshape(n, -1)
    canon = _canon_kmers(mat, k)
    in_piece = np.zeros(canon.shape, dtype=bool)
    for i in range(0, n, 10):      # (a tenth of the reads is sample enough)
        for start, length in osc.valid_pieces(mat[i].tobytes()):
            in_piece[i, start:start + length - k + 1] = True
    assert in_piece.sum() > 10_000
    return float(np.isin(canon[in_piece], keys).mean())


CROWD_E, CROWD_S = 40_000, 10_000


@pytest.fixture(scope="module", params=[21, 31], ids=["k21", "k31"])
def crowd(request):
    """the crowded reads, their filters and the oracle's scan of them, made once per k; the density is checked here, on the CPU, before any GPU run"""
    k = request.param
    bases, offs = _crowded(k)
    tai, nh = api.load_filter_shape(CROWD_E, CROWD_S)
    assert in_map_share(bases, offs, k, tai, nh) > 0.9
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    return k, tai, nh, bases, offs, b2, osc


def test_rounds_with_far_more_than_64_hits(crowd):
    """Nearly every position passes both filters: a 256-position round holds far more than 64 hits and needs several hand-out rounds.  The
    oracle alone says how dense: of the piece positions of a second pass, 0.923 (k = 21) and 0.909 (k = 31) are in the map after the first
    (measured on the CPU; the bar is 0.9, see the fixture), so the test cannot quietly degenerate into the sparse case.
    Load and scan in one context: the scan takes the load pass's sure plane."""
    k, tai, nh, bases, offs, b2, osc = crowd
    ctx, sst, _, _ = _load_and_scan(bases, offs, k, CROWD_E, CROWD_S, chunks(bases, offs, 3))
    assert sst["valid_reused"] > 0


def test_the_same_reads_twice_in_one_scan(crowd):
    """The first batch meets an empty map -- no hit anywhere --, the second a full one."""
    k, tai, nh, bases, offs, b2, osc = crowd
    twice = np.concatenate([bases, bases])
    offs2 = np.concatenate([offs, offs[1:] + offs[-1]])
    osc2 = po.Scanner(k, 1, 100, b2)
    osc2.scan_reads(twice, offs2)
    ctx = api.Context(k, tai, nh)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(twice, offs2, 2))
    _scan_equals_oracle(sc, sst, osc2)
    _no_word_differs(ctx)


def test_no_sure_plane_every_window_an_item_of_the_validity_pass(crowd):
    """After bloom_upload only: nothing is known from a load pass, every window that exists is probed."""
    k, tai, nh, bases, offs, b2, osc = crowd
    ctx = api.Context(k, tai, nh)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 2))
    assert sst["valid_reused"] == 0
    _scan_equals_oracle(sc, sst, osc)
    _no_word_differs(ctx)


# ---- ragged ends --------------------------------------------------------------------------------------------------------------------------------
def _reads_filling(n_words, seed, k):
    """reads (100 bases, some shorter than k, some with N) whose stream -- a read takes its bases and one separator -- ends 13 positions
    before the end of word n_words - 1"""
    T = n_words * 64 - 13
    rng = np.random.default_rng(seed)
    g = synth.make_genome(1500, 7)      # one genome for every size and batch: their k-mers meet in the map
    lines = []
    left = T
    while left > 0:
        n = min(left - 1, 100 if rng.random() > 0.1 else int(rng.integers(1, k)))
        if n <= 0:
            n, left = 1, 2      # (one position left: it goes to a one-base read's separator)
        s = int(rng.integers(0, len(g) - n + 1))
        r = g[s:s + n].copy()
        if rng.random() < 0.05:
            r[int(rng.integers(0, n))] = ord("N")
        lines.append(r.tobytes())
        left -= n + 1
    return lines


@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 255, 257, 1025, 1026, 1027, 1028, 1030, 1032])
def test_streams_that_end_inside_a_round(n_words):
    """One batch whose positions fill 1, 63, ... 1 025 words, and 1 025 to 1 028 (the stream ends in the first, second, third and fourth word of a
    four-word round), 1 030 and 1 032 (the sixth and last word of the validity pass's eight-word round); ok is false inside the rounds: reads
    shorter than k, reads with N."""
    k = 21
    bases, offs = po.reads_from_lines(_reads_filling(n_words, 100 + n_words, k))
    assert (int(offs[-1]) + len(offs) - 1 + 63) // 64 == n_words
    _load_and_scan(bases, offs, k, 40_000, 10_000, [api.ReadBatch(bases, offs)])


def test_five_batches_that_each_end_inside_another_word_of_a_round():
    """Five batches of 257 to 261 words in one load and one scan: every batch leaves another part of its last rounds empty."""
    k = 21
    parts = [po.reads_from_lines(_reads_filling(257 + i, 300 + i, k)) for i in range(5)]
    bases = np.concatenate([b for b, _ in parts])
    offs, batches = [np.zeros(1, dtype=np.uint64)], []
    for b, o in parts:
        batches.append(api.ReadBatch(bases, (o + offs[-1][-1]).astype(np.uint64)))
        offs.append(o[1:] + offs[-1][-1])
    _load_and_scan(bases, np.concatenate(offs).astype(np.uint64), k, 60_000, 15_000, batches)


# ---- windows off the word grid -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thirty_thousand():
    k, E, S = 31, 3_000_000, 600_000
    bases, offs = _random_case(30_000, 100, k, 60_000, 0.01, 4242, 0.002, 3)
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    return k, tai, nh, bases, offs, b2.bits(), osc


@pytest.mark.parametrize("span", [64, 1000, 1 << 14])
def test_windows_that_begin_and_end_inside_words(span, thirty_thousand):
    """walk_window_span 64, 1 000 and 2^14: a window's lo and pos_end fall inside words, and a word of lk is shared by two windows."""
    k, tai, nh, bases, offs, bits, osc = thirty_thousand
    ctx = api.Context(k, tai, nh, walk_window_span=span)
    ctx.bloom_upload(L.BLOO2, bits)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 2))
    _scan_equals_oracle(sc, sst, osc)
    _no_word_differs(ctx)


def test_a_window_whose_planes_the_walk_makes_again(tmp_path):
    """The walk's own look-up (walk_register with a large delta: k_need_lookup over the window's words, w_first > 0) in front of the dense link
    pass: the planes the link pass reads are made by another kernel, on the walk stream.  FGPU_REFRESH_DIV, the knob that decides it, is read
    once per process: a child of its own, tests/dense_hits_child.py.  With the knob at 2^30 every window with keys created before it takes
    that path; the child's launch counts say that it did."""
    from tests.test_gpu_env_switches import _clean_env, _started, CHILD_TIMEOUT, ROOT
    import json
    import subprocess
    import sys
    out = str(tmp_path / "blob.npz")
    env = {"FGPU_REFRESH_DIV": str(1 << 30), "FGPU_DEBUG_DELTA_CHECK": "1", "FGPU_PROFILE_WALK": "1"}
    r = _started("dense_hits_child", lambda: subprocess.run([sys.executable, "-m", "tests.dense_hits_child", out], capture_output=True, text=True, cwd=ROOT,
                                                            env=_clean_env(env), timeout=CHILD_TIMEOUT))
    assert r.returncode == 0 and r.stdout == "", r.stdout[-1000:] + r.stderr[-3000:]
    z = np.load(out)
    from tests import dense_hits_child
    bases, offs, k, tai, nh = dense_hits_child.workload()
    _, _, _, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)

    class Child:
        def junctions(self):
            return z["keys"], z["recs"]
    _scan_equals_oracle(Child(), json.loads(str(z["scan_stats"])), osc)
    assert json.loads(str(z["prepared_refresh"]))["mismatching_words"] == 0 and "differ" not in r.stderr
    times = json.loads(str(z["kernel_times"]))
    # a window registers with one launch under "walk_lookup"; one that makes its planes again has the look-up's launch under the same label
    assert times["walk_lookup"][0] > times["walk_link"][0] > 4


# ---- two goldens -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [256, 1 << 16])
@pytest.mark.parametrize("name", ["ragged_k31", "j2_spacer20_k15"])
def test_goldens_through_the_same_check(name, span):
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, walk_window_span=span)
    ctx.bloom_upload(L.BLOO2, c.bloom())
    sc = api.ReadScanner(ctx)
    st = sc.scanReads(chunks(bases, offs, 2))
    b2 = po.Bloom(tai, nh)
    b2.set_bits(c.bloom())
    osc = po.Scanner(c.k, c.j, c.spacer, b2)
    osc.scan_reads(bases, offs, paired_ends=False, no_cleaning=True)
    _scan_equals_oracle(sc, st, osc)
    keys, recs = sc.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())
    _no_word_differs(ctx)
