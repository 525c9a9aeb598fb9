"""INTEGRATION.md, "Environment switches": "results never depend on them".  Every switch below is set in a child process of its own
(tests/switch_child.py: most are read once per process) on the smallest workloads at which the code it steers exists at all, and the child's
filters, load counters, junction map in creation order and scan counters are compared with the ORACLE (and, for the golden workloads, with the
compiled reference's recorded files and counters) -- never with another run of the library.  A row that cannot have taken its path fails: where
the library has an observable (scan counters, fgpu_diag_ovw, launches per label of a profiled child, stderr) it is asserted; where it has none
(a grid size leaves no trace) the test's docstring argues from the code and the input-side condition is asserted.  Needs an MI355X."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from faucet_amd import api
from tests import switch_child
from tests.golden_util import Case
from tests.test_gpu_estimate_stream import output_files, written_input
from tests.test_gpu_filter_shapes import _case_2g
from tests.test_gpu_parity import _random_case, _scan_equals_oracle, oracle_run
from tests.test_gpu_scan_kept_cli import golden_bytes, ok_code, run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120
KO16 = {"FGPU_WALK_KO": "16", "FGPU_WALK_KO_ALWAYS": "1"}
KO64 = {"FGPU_WALK_KO": "64", "FGPU_WALK_KO_ALWAYS": "1"}
PROFILED = {"FGPU_PROFILE_WALK": "1"}      # (the walk stage's kernels are timed under their own labels only with it: fgpu_stage_scan_walk)

# ---- the latch: after a child that crashed or hung nothing more is started ------------------------------------------------------------------
_casualty = []


def _clean_env(env):
    base = {k: v for k, v in os.environ.items() if not k.startswith(("FGPU_", "FAUCET_"))}
    return dict(base, **env)


def _started(what, start):
    """start() -> CompletedProcess, under the latch: a child that ended on a signal, aborted (134), segfaulted (139) or ran into its time limit
    fails this test and every later one of the module, which start nothing"""
    if _casualty:
        pytest.fail(f"not started: an earlier child of this module crashed or hung -- {_casualty[0]}")
    try:
        r = start()
    except subprocess.TimeoutExpired as e:
        _casualty.append(f"{what}: no end after {e.timeout} s")
        pytest.fail(_casualty[0])
    if r.returncode < 0 or r.returncode in (134, 139):
        _casualty.append(f"{what}: ended with {r.returncode}; stderr ends: {r.stderr[-1500:]}")
        pytest.fail(_casualty[0])
    return r


class Blob:
    """what a child wrote; junctions() as a ReadScanner's, for _scan_equals_oracle"""

    def __init__(self, path, stderr):
        z = np.load(path)
        self.z, self.stderr = z, stderr
        self.keys, self.recs = z["keys"], z["recs"]
        self.scan = json.loads(str(z["scan_stats"]))
        self.ovw = json.loads(str(z["ovw"]))
        self.replays = int(z["replays"])
        self.load = json.loads(str(z["load_stats"])) if "load_stats" in z.files else None
        self.times = json.loads(str(z["kernel_times"])) if "kernel_times" in z.files else {}

    def junctions(self):
        return self.keys, self.recs

    def launches(self, label):
        return self.times.get(label, (0, 0.0))[0]


def child(workload, env, tmp_path, tag="blob"):
    out = str(tmp_path / f"{tag}.npz")
    what = f"switch_child {workload} with {env}"
    r = _started(what, lambda: subprocess.run([sys.executable, "-m", "tests.switch_child", workload, out], capture_output=True, text=True, cwd=ROOT,
                                              env=_clean_env(env), timeout=CHILD_TIMEOUT))
    assert r.returncode == 0, what + "\n" + r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout == ""
    return Blob(out, r.stderr)


# ---- the references: computed once per workload ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(name):
    """(workload, oracle filters, oracle load counters, oracle scanner) of a workload of switch_child"""
    w = switch_child.Workload(name)
    if name == "bits31":
        k, tai, bases, offs, b1, b2, lst, osc = _case_2g(3, False)
        assert (k, tai) == (w.k, w.tai) and np.array_equal(bases, w.bases) and np.array_equal(offs, w.offs)
        return w, b1, b2, lst, osc
    return (w,) + oracle_run((w.bases, w.offs), w.k, w.tai, w.nh, w.j, w.spacer, mercy=w.mercy)


def equals_the_oracle(blob, name):
    """every field of the blob the oracle (and a golden's recorded run) has"""
    w, b1, b2, lst, osc = expected(name.split("+")[0])
    for which, ob in (("bloo1", b1), ("bloo2", b2)):
        idx, val = switch_child.sparse(ob.bits())
        assert int(blob.z["bloom_bytes"]) == len(ob.bits())
        assert np.array_equal(blob.z[which + "_idx"], idx) and np.array_equal(blob.z[which + "_val"], val), which + " differs from the oracle's"
    for key in ("reads_processed", "unambiguous_reads", "kmers", "to_bloo2"):
        assert blob.load[key] == getattr(lst, key), key
    _scan_equals_oracle(blob, blob.scan, osc)
    c = w.case
    if c is not None:
        bits = np.zeros(len(c.bloom()), dtype=np.uint8)
        bits[blob.z["bloo2_idx"]] = blob.z["bloo2_val"]
        assert np.array_equal(bits, c.bloom()), "bloo2 differs from the reference's .bloom file"
        cn = c.counters
        assert blob.load["reads_processed"] == cn["load_reads_processed"] and blob.load["unambiguous_reads"] == cn["load_unambiguous"]
        for mine, theirs in (("n_junctions", "distinct_junctions"), ("nb_jcheck_kmer", "nb_jcheck_kmer"), ("nb_no_juncs", "nb_no_juncs"),
                             ("nb_processed", "nb_processed"), ("nb_skipped", "nb_skipped"), ("reads_no_errors", "reads_no_errors"),
                             ("reads_processed", "scan_reads_processed"), ("unambiguous_reads", "scan_unambiguous")):
            assert blob.scan[mine] == cn[theirs], mine
        assert sorted(api.junction_lines(blob.keys, blob.recs, c.k)) == sorted(c.junction_lines())
    print(name, {k: blob.scan[k] for k in ("n_junctions", "reads_no_errors", "walk_windows", "walk_followers", "walk_max_cluster", "walk_parallel",
                                           "flag_positions", "flags_filled")}, blob.ovw, "replays", blob.replays)


_baselines = {}


def baseline(name, env, tmp_path_factory):
    """a run without the switch under test whose COUNTERS a guard compares with (its results are held to the oracle like any other's)"""
    key = (name, tuple(sorted(env.items())))
    if key not in _baselines:
        b = child(name, env, tmp_path_factory.mktemp("baseline"))
        equals_the_oracle(b, name)
        _baselines[key] = b
    return _baselines[key]


def pieces(blob):
    return blob.scan["reads_no_errors"]      # (the scan's valid pieces: fgpu_scan_end)


def cases(workloads, settings):
    return [pytest.param(w, s, id=w + "-" + "-".join(f"{k.replace('FGPU_', '')}={v}" for k, v in s.items())) for s in settings for w in workloads]


# ---- the walk stage's grids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", cases(["clusters", "tiny_genome", "golden"], [{"FGPU_WALK_DYN_GRID": "1"}, {"FGPU_WALK_DYN_GRID": "3"}]))
def test_walk_dyn_of_one_and_three_waves(name, env, tmp_path):
    """k_walk_dyn gets min(blocks(max_pieces, 64), FGPU_WALK_DYN_GRID) waves of 64 lanes (walk_clusters, scan_walk.hip); every lane draws a leader
    from the window's root_list, walks the leader's followers from the pool cluster_followers fills, and draws again when its cluster is done.
    A grid leaves no trace, so the input side is asserted: far more pieces than a wave has lanes, and
    - `clusters`: the clusters left to k_walk_dyn (pieces less followers less the pieces of the large-cluster walks) are more per window, on
      average, than the grid has lanes -- some window then has more, and its lanes were refilled;
    - `tiny_genome`, `golden` (a few clusters of hundreds of pieces: no refill to speak of): most pieces are followers and the largest cluster
      exceeds a wave, so what one or three waves walk here are the long follower lists."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    lanes = 64 * int(env["FGPU_WALK_DYN_GRID"])
    leaders = pieces(b) - b.scan["walk_followers"] - b.scan["walk_parallel"]
    assert b.scan["n_junctions"] > 64 and pieces(b) > 10 * 64
    if name == "clusters":
        assert leaders > lanes * b.scan["walk_windows"], (leaders, b.scan["walk_windows"], lanes)
    else:
        assert 2 * b.scan["walk_followers"] > pieces(b) and b.scan["walk_max_cluster"] > 64, b.scan


@pytest.mark.parametrize("name,env", cases(["clusters", "tiny_genome"], [{"FGPU_CLUSTER_GRID": "1"}]))
def test_walk_cluster_in_one_block(name, env, tmp_path):
    """k_walk_cluster gets min(FGPU_CLUSTER_GRID, blocks(max_pieces, 256)) blocks (fgpu_stage_scan_walk) and strides over the window's pieces; its
    wave-aggregated reservation into root_list then comes from one block's waves, trip after trip, the last one partly empty.  Input side: a
    scan's first window spans 2^18 positions (fgpu_scan_begin: the controller starts there and has not looked yet), and more than 512 reads
    of the first batch start in its first three quarters -- the one block makes several trips over that window."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    w = expected(name)[0]
    first_batch = w.offs[:(len(w.offs) - 1) // w.scan_batches + 1]
    assert int(np.searchsorted(first_batch, (1 << 18) * 3 // 4)) > 512 and first_batch[-1] > 1 << 18


@pytest.mark.parametrize("name,env", cases(["clusters"], [{"FGPU_DELTA_PER_BLOCK": "1"}, {"FGPU_DELTA_PER_BLOCK": "1000000"}]))
def test_walk_register_delta_blocks(name, env, tmp_path):
    """walk_register gives k_walk_register's delta part min(4096, max(64, delta_est / FGPU_DELTA_PER_BLOCK)) blocks, delta_est being the keys the
    earlier batches created plus three per piece of the batch's earlier windows: with 1 a block per key up to 4096 (most of them with nothing
    to do, the last partly filled), with 10^6 the 64 of the lower bound.  Input side: three scan batches and more created keys than 64."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    assert expected(name)[0].scan_batches == 3 and b.scan["n_junctions"] > 64


@pytest.mark.parametrize("name,env", cases(["clusters", "golden"], [{"FGPU_REFRESH_DIV": "1"}, {"FGPU_REFRESH_DIV": "1000000000"}]))
def test_walk_register_refreshes_never_and_always(name, env, tmp_path):
    """refresh_window = delta_est > window positions / FGPU_REFRESH_DIV (walk_register): with 1 only where more keys were created than the
    window has positions, with 10^9 whenever delta_est > 0 -- every window but the first of a batch whose predecessors' keys the host has not
    counted yet.  A refreshed window launches k_need_lookup AND k_walk_register under the label walk_lookup, the others k_walk_register alone;
    k_walk_dyn ("walk") runs once per window.  So lookups - windows windows were refreshed: with 10^9 all but one per batch at the most, with 1
    at least two were not (more than the scan's first, whose delta is empty: a delta was registered)."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    p = child(name + "+profile", dict(env, **PROFILED), tmp_path, "profiled")
    equals_the_oracle(p, name)
    windows, lookups = p.launches("walk"), p.launches("walk_lookup")
    print(name, env, "windows", windows, "walk_lookup launches", lookups)
    assert windows == p.scan["walk_windows"] >= 2 and windows <= lookups <= 2 * windows
    if env["FGPU_REFRESH_DIV"] == "1":
        assert 2 * windows - lookups >= 2, (lookups, windows)
    else:
        assert lookups >= 2 * windows - expected(name)[0].scan_batches and lookups > windows, (lookups, windows)


@pytest.mark.parametrize("name,env", cases(["clusters", "golden"], [{"FGPU_MAX_SPAN_LOG2": "12"}]))
def test_windows_of_at_most_4096_positions(name, env, tmp_path, tmp_path_factory):
    """the adaptive controller under a bound of 2^12 positions (fgpu_create): dozens of windows per batch, pieces that reach past their window.
    Guard: at least a window per 4096 positions, and several times the default run's windows."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    w = expected(name)[0]
    default = baseline(name, {}, tmp_path_factory)
    assert b.scan["walk_windows"] >= len(w.bases) // 4096 and b.scan["walk_windows"] >= 3 * default.scan["walk_windows"], \
        (b.scan["walk_windows"], default.scan["walk_windows"])


@pytest.mark.parametrize("name,env", cases(["clusters", "repeats"], [{"FGPU_NO_OVERLAP": "1"}]) + cases(["repeats"], [dict(KO16, FGPU_NO_OVERLAP="1")]))
def test_walk_stage_on_the_main_stream(name, env, tmp_path):
    """FGPU_NO_OVERLAP=1: the stage's kernels, the optimistic rounds included (ovw_stream = walk_stream), on the context's stream"""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    if "FGPU_WALK_KO" in env:
        assert b.ovw["pieces"] > 0 and b.scan["walk_parallel"] > 0, (b.ovw, b.scan)


# ---- older kernels kept as fallbacks, state machines under a block cap ------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", cases(["clusters", "golden", "tiny_genome"], [{"FGPU_NEED_TIGHT": "0"}, {"FGPU_NEED_TIGHT": "1"}]))
def test_older_forms_of_the_need_prewalk(name, env, tmp_path, tmp_path_factory):
    """k_need_prewalk with tight = 0 / 1 marks what tight = 2 marks and more (the in-map junction's own position; the rest of a piece that
    lands between junctions): the pure stage then evaluates more positions (flag_positions), never fewer."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    default = baseline(name, {}, tmp_path_factory)
    print(name, env, "flag_positions", b.scan["flag_positions"], "default", default.scan["flag_positions"])
    assert b.scan["flag_positions"] > default.scan["flag_positions"]


@pytest.mark.parametrize("name,env", cases(["clusters", "tiny_genome", "golden"], [{"FGPU_FLAGS_SM_BLOCKS": "0"}, {"FGPU_FLAGS_SM_BLOCKS": "1"}]))
def test_flag_kernels(name, env, tmp_path):
    """scan_pure_flags (scan_pure.hip): j <= 1 and FGPU_FLAGS_SM_BLOCKS > 0 picks k_scan_flags_sm<1> on min(words / 256, that many) blocks, else
    k_scan_flags.  With 0 the old kernel runs for j = 0 and 1, with 1 one block's 256 lanes take every word of a range.  Both carry the label
    scan_flags; input side: j <= 1, and a scan batch of more than 512 words, so that a range of it is more than one block's worth."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    w = expected(name)[0]
    assert w.j <= 1 and len(w.bases) // w.scan_batches // 64 > 512 and b.scan["flag_positions"] > 0


@pytest.mark.parametrize("name,env", cases(["clusters_one", "clusters", "golden"], [{"FGPU_RESOLVE_SM": "0"}, {"FGPU_RESOLVE_SM": "1"}]))
def test_resolve_kernels(name, env, tmp_path):
    """load_batch (load.hip): at most 4 hash functions, no fail plane and FGPU_RESOLVE_SM != 0 picks k_load_resolve_sm on min(words / 256,
    max(that, 64)) blocks, else k_load_resolve.  With 0 the generic kernel resolves a three-function filter; with 1 the cap is 64 blocks, which
    binds only for a batch of more than 64 x 256 words: the one-batch load of `clusters_one`."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    w = expected(name)[0]
    assert w.nh <= 4 and not w.mercy and b.load["to_bloo2"] > 0
    if name == "clusters_one":
        n_words = len(w.bases) // 64
        assert w.load_batches == 1 and n_words > 16384, n_words


@pytest.mark.parametrize("name,env", cases(["clusters", "golden", "golden_mercy"], [{"FGPU_CARRY_MODE": "set"}]))
def test_carry_by_rehashing_below_2_to_the_31_bits(name, env, tmp_path):
    """FGPU_CARRY_MODE=set: k_carry_set after every batch and first-set times that restart at 0 (tb = 0), which --mercy's k_load_mercy reads"""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    p = child(name + "+profile", env, tmp_path, "profiled")
    equals_the_oracle(p, name)
    w = expected(name)[0]
    assert w.tai < 1 << 31 and p.launches("carry_update") == w.load_batches, p.times
    assert p.launches("load_mercy") == (w.load_batches if w.mercy else 0)


def test_carry_by_sweeps_at_2_to_the_31_bits(tmp_path):
    """FGPU_CARRY_MODE=sweep at the one size that never sweeps by itself (fgpu_load_pass_policy).  k_carry_set and the sweep (k_carry_from_first)
    share the label carry_update: by re-hashing it is launched once per batch, five times here (load_batch); sweeps close epochs of batches,
    so they are fewer.  (One child, the profiled one.)"""
    p = child("bits31+profile", {"FGPU_CARRY_MODE": "sweep"}, tmp_path)
    equals_the_oracle(p, "bits31")
    assert expected("bits31")[0].tai == 1 << 31 and 1 <= p.launches("carry_update") < 5 == p.launches("load_mark"), p.times


# ---- who walks the large clusters ---------------------------------------------------------------------------------------------------------------
def test_the_repeat_set_reaches_both_large_cluster_walks(tmp_path_factory):
    """`repeats` (switch_child.REPEATS) is the smallest of the sizes tried at which, with FGPU_WALK_KO=16 FGPU_WALK_KO_ALWAYS=1 and nothing else
    set, the optimistic walk takes pieces and the large-cluster walks report them.  Measured (genome, copies of the 300-base repeat, reads of
    100 -> fgpu_diag_ovw pieces = walk_parallel, largest cluster, pieces in all): 30 000 / 10 / 12 000 -> 7 685, 1 342, 9 328;
    15 000 / 5 / 6 000 -> 4 412, 886, 4 599; 9 000 / 3 / 3 600 -> 2 685, 756, 2 775; 6 000 / 4 / 2 400 -> 1 811, 378, 1 853;
    6 000 / 2 / 2 400 -> 1 788, 263, 1 843; 3 000 / 2 / 1 200 -> 899, 280, 938 (kept: two copies are the fewest that make a repeat, and 40x of
    3 kb leaves each of the three scan batches some 300 pieces)."""
    b = baseline("repeats", KO16, tmp_path_factory)
    assert b.ovw["pieces"] > 0 and b.scan["walk_parallel"] > 0, (b.ovw, b.scan)


@pytest.mark.parametrize("name,env", cases(["repeats", "clusters"], [
    dict(KO64, FGPU_WALK_KO_WEIGHT="1"), dict(KO64, FGPU_WALK_KO_WEIGHT="48"), dict(KO64, FGPU_WALK_KO_WEIGHT="128", FGPU_WALK_KO_AVG="0"),
    dict(KO64, FGPU_WALK_KO_WEIGHT="128", FGPU_WALK_KO_AVG="1", FGPU_WALK_KO_AVG_MIN="1")]))
def test_large_clusters_by_weight(name, env, tmp_path, tmp_path_factory):
    """ko_cluster's three clauses one at a time (heavy_w: bar in all | positions per piece << 16 | bar for repeat pieces << 24): everything that
    holds an lk position; the CLI's bars at 48; the bar in all alone (per piece 0 switches the third clause off); the third clause alone in
    effect (1 per piece, 1 in all).  The clusters taken by weight are walked by k_ovw_round / k_walk_ko, so walk_parallel exceeds what the
    same workload shows with the rule off (64 pieces and more only)."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    off = baseline(name, KO64, tmp_path_factory)
    print(name, env, "walk_parallel", b.scan["walk_parallel"], "rule off", off.scan["walk_parallel"])
    assert b.scan["walk_parallel"] > off.scan["walk_parallel"]


def test_optimistic_walk_reports_its_followers(tmp_path):
    """FGPU_OVW_FOLLOWERS=1: k_ovw_commit's pieces count as queueing ones for the window-size controller; the windows may differ, the map not"""
    b = child("repeats", dict(KO16, FGPU_OVW_FOLLOWERS="1"), tmp_path)
    equals_the_oracle(b, "repeats")
    assert b.ovw["pieces"] > 0 and b.scan["walk_parallel"] > 0, (b.ovw, b.scan)


# ---- where the filter pair lies -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", cases(["clusters", "golden"], [{"FGPU_PAIR_PLACE": "1", "FGPU_DEBUG_PLACE": "1"}, {"FGPU_DEBUG_ALLOC_FIRST": "1"},
                                                                     {"FGPU_PAIR_PLACE": "1", "FGPU_DEBUG_PLACE": "1", "FGPU_DEBUG_ALLOC_FIRST": "1"}]))
def test_placing_the_filter_pair_at_small_sizes(name, env, tmp_path):
    """fgpu_place_pair (diag.hip) times random loads and atomicMin on the pass's own pair and first[] before the pass initialises them, and may
    keep another allocation of the pair: whatever it wrote and kept, both filters are the oracle's.  It says what it did on stderr."""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    assert ("[place] filter pair:" in b.stderr) == ("FGPU_PAIR_PLACE" in env), b.stderr[-2000:]


# ---- diagnostics --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", cases(["golden", "tiny_genome"], [{"FGPU_TRACE": "1"}]))
def test_every_kernel_named_and_waited_for(name, env, tmp_path):
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    for label in ("load_mark", "load_resolve", "scan_flags", "need_prewalk", "walk_lookup", "walk_link", "walk_cluster", "walk"):
        assert f"[fgpu] {label} grid " in b.stderr, label
    assert b.stderr.count(" grid ") == b.stderr.count(" ... done\n") > 50


def test_the_talkative_switches_together(tmp_path):
    env = {"FGPU_DEBUG_SPAN": "1", "FGPU_DEBUG_HOST": "1", "FGPU_DEBUG_WAITS": "1", "FGPU_PROFILE_WALK": "1"}
    b = child("golden+profile", env, tmp_path)
    equals_the_oracle(b, "golden")
    assert b.stderr.strip() != "" and b.launches("walk") == b.scan["walk_windows"] > 0, (b.stderr[-1000:], b.times)


EXTREMES = {"FGPU_WALK_DYN_GRID": "1", "FGPU_CLUSTER_GRID": "1", "FGPU_DELTA_PER_BLOCK": "1", "FGPU_REFRESH_DIV": "1000000000", "FGPU_MAX_SPAN_LOG2": "12",
            "FGPU_FLAGS_SM_BLOCKS": "1", "FGPU_NEED_TIGHT": "0"}


@pytest.mark.parametrize("name,env", [pytest.param("clusters", EXTREMES, id="clusters"), pytest.param("repeats", dict(EXTREMES, **KO16), id="repeats-KO16")])
def test_the_extremes_together(name, env, tmp_path):
    """(repeats: in windows of 4096 positions no cluster reaches 16 pieces, so FGPU_WALK_KO_ALWAYS launches the large-cluster walks' kernels on
    windows that hold nothing for them)"""
    b = child(name, env, tmp_path)
    equals_the_oracle(b, name)
    assert b.scan["walk_windows"] >= len(expected(name)[0].bases) // 4096


# ---- read shards and the command line -----------------------------------------------------------------------------------------------------------
def test_prepared_shard_without_the_delta_refresh(tmp_path):
    """FGPU_NO_DELTA_REFRESH=1 in the scenario of test_gpu_parity's test_a_fresher_preview_lets_the_walk_look_only_for_the_keys_created_since
    (switch_child.delta_refresh): the refreshed planes are NOT merged with the keys created since, both prepared batches' planes are made
    again in full -- and the third shard's map and counters are the oracle's of the whole input."""
    out = str(tmp_path / "blob.npz")
    env = {"FGPU_NO_DELTA_REFRESH": "1"}
    r = _started("switch_child delta_refresh", lambda: subprocess.run([sys.executable, "-m", "tests.switch_child", "delta_refresh", out], capture_output=True,
                                                                      text=True, cwd=ROOT, env=_clean_env(env), timeout=CHILD_TIMEOUT))
    assert r.returncode == 0 and r.stdout == "", r.stdout[-1000:] + r.stderr[-3000:]
    b = Blob(out, r.stderr)
    k, G = 21, 30_000
    bases, offs = _random_case(15_000, 100, k, G, 0.012, 911, 0.002, 3)
    tai, nh = api.load_filter_shape(20 * G, 4 * G)
    osc = oracle_run((bases, offs), k, tai, nh)[3]
    _scan_equals_oracle(b, b.scan, osc)
    d = json.loads(str(b.z["prepared_refresh"]))
    n_early, n_a, n_b = (int(v) for v in b.z["tables"])
    assert 0 < n_early < n_a < n_b
    assert d["batches_merged"] == 0 and d["batches_in_full"] == 2, d


def cli(cwd, args, env):
    return _started(f"faucet {' '.join(args)} with {env}", lambda: run(cwd, args, env=env, timeout=CHILD_TIMEOUT))


def assert_golden_run(c, r, cwd):
    assert r.returncode == ok_code(c), r.stdout[-2000:] + r.stderr[-3000:]
    for ext in output_files(c):
        with open(os.path.join(cwd, "out." + ext), "rb") as f:
            assert f.read() == golden_bytes(c, ext), ext


@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21"])
def test_read_shards_without_the_late_hint(name, tmp_path):
    """FAUCET_LATE_HINT=0, `faucet -gpus 2`: no fresher preview passed up the chain; every output file is the compiled reference's"""
    c = Case(name)
    inp = written_input(c, tmp_path)
    cwd = str(tmp_path / "run")
    r = cli(cwd, ["-read_load_file", inp, "-read_scan_file", inp, "-gpus", "2"] + c.meta["args"], {"FAUCET_LATE_HINT": "0"})
    assert_golden_run(c, r, cwd)


@pytest.mark.parametrize("switch", ["FGPU_CLI_NO_MMAP", "FGPU_CLI_TIDY"])
@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21"])
def test_command_line_reading_without_a_mapping_and_leaving_the_long_way(name, switch, tmp_path):
    c = Case(name)
    inp = written_input(c, tmp_path)
    cwd = str(tmp_path / "run")
    r = cli(cwd, ["-read_load_file", inp, "-read_scan_file", inp] + c.meta["args"], {switch: "1"})
    assert_golden_run(c, r, cwd)
