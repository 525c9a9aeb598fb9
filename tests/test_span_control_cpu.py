"""The window-span controller of the ordered walk (faucet_amd/csrc/walk_span.h) without a GPU.

tests/host/span_control_check.cpp includes nothing of the project but walk_span.h and drives the controller from a script: the start of a scan,
the host's three counters after a batch, the three values read back behind a window, the end of a scan.  After every step it prints the span,
the looks left, the vote and the rest of the state.

The expected numbers were worked out by hand from the controller as it stood before it became a struct (commit 3531838): `api` = that commit's
faucet_amd/csrc/api.hip (fgpu_scan_begin 793-804, adapt_window 822-876, fgpu_scan_end 1444), `walk` = its scan_walk.hip (walk_span_look
3102-3142).  The line beside each step is the one the numbers follow from.  Counters are totals of the scan, as the device counts them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

NEVER = (1 << 64) - 1      # span_ceiling of a scan whose large-cluster tables have not overflowed


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("span_control") / "span_control_check")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "faucet_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "span_control_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _play(exe, steps):
    """steps: (command, span, looks, vote[, {other field: value}]); every step's line is compared"""
    r = subprocess.run([exe], input="".join(s[0] + "\n" for s in steps), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(steps), r.stdout
    for n, (step, line) in enumerate(zip(steps, lines)):
        got = {k: int(v) for k, v in (f.split("=") for f in line.split())}
        want = dict(span=step[1], looks=step[2], vote=step[3], **(step[4] if len(step) > 4 else {}))
        assert {k: got[k] for k in want} == want, (n, step[0], line)


def test_a_share_above_a_half_shrinks_at_once(check):
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),                                   # the context's defaults (fgpu_ctx.h 371-373, 413)
        ("begin 0", 1 << 18, 16, 0, dict(ceiling=NEVER)),                        # api 793-796, 803
        ("batch 400 1000 0 0", 1 << 18, 16, 0, dict(proven=1 << 18)),            # api 841-842: 0.4 asks for nothing; 846
        ("look 440 1100 0", 1 << 18, 0, 0),                                      # walk 3131-3132: settled
        # 0.6: not clear (api 841: 3000 > 4000 is false), the half size has been walked (api 860: 2^17 > proven 2^18 is false): no looks
        ("batch 1000 2000 0 0", 1 << 17, 0, 0, dict(proven=1 << 17)),            # api 856-861
        ("batch 1900 3000 0 0", 1 << 16, 8, 0, dict(proven=1 << 16)),            # 0.9 > 4/5 is clear: api 841, 860
    ])
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        ("batch 600 1000 0 0", 1 << 17, 8, 0, dict(proven=0)),                   # 0.6 on a context that has proven no size: api 860 (2^17 > 0)
    ])
    _play(check, [
        ("new 4096", 1 << 17, 0, 0),
        ("begin 0", 4096, 16, 0),                                                # api 795: capped by max_span
        ("batch 900 1000 0 0", 4096, 16, 0),                                     # api 856: never below 4096
    ])


def test_b_growing_takes_a_clear_share_or_two_batches_running(check):
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        ("look 40 100 0", 1 << 18, 0, 0),                                        # walk 3131-3132
        ("batch 250 1000 0 0", 1 << 18, 0, 1, dict(proven=1 << 18)),             # 0.25: api 842 (5000 < 3000 is false), 844-846: a vote
        ("batch 500 2000 0 0", 1 << 19, 2, 0, dict(proven=1 << 18)),             # the second running: api 844, 863-867 (2^19 > proven: 2 looks)
        ("batch 600 3000 0 0", 1 << 20, 2, 0, dict(proven=1 << 19)),             # 0.1 < 3/20 is clear: at once, api 842, 846, 866-867
    ])
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        ("batch 250 1000 0 0", 1 << 18, 16, 1),                                  # api 845
        ("batch 650 2000 0 0", 1 << 18, 16, 0),                                  # 0.4 in between takes the vote back: api 845
        ("batch 900 3000 0 0", 1 << 18, 16, 1),                                  # ... so 0.25 is a first time again
    ])
    _play(check, [
        ("new %d" % (1 << 20), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        ("batch 100 1000 0 0", 1 << 19, 16, 0),                                  # api 866-867: max(16, 2) looks
        ("batch 200 2000 0 0", 1 << 20, 16, 0),                                  # api 838: usual = min(max_span, FGPU_USUAL_SPAN, ceiling) = 2^20
        ("batch 300 3000 0 0", 1 << 20, 16, 0),                                  # api 863: not past it
        ("batch 310 4000 0 0", 1 << 20, 16, 0),                                  # 0.01: api 869, not past min(max_span, ceiling) either
    ])


def test_c_an_overflow_of_the_large_cluster_tables_quarters_the_span(check):
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        ("batch 100 1000 1 0", 1 << 16, 0, 0, dict(ceiling=1 << 17, proven=1 << 16)),      # api 847-854 (whatever the share asks for)
        ("batch 200 2000 1 0", 1 << 17, 2, 0, dict(ceiling=1 << 17)),            # api 838: usual = the ceiling; 866-867
        ("batch 300 3000 1 0", 1 << 17, 2, 0, dict(proven=1 << 17)),             # api 863: the size that overflowed (2^18) is not reached again
        ("batch 310 4000 1 0", 1 << 17, 2, 0),                                   # api 869: nor by the rule for thin coverage
        ("look 100 4000 2", 1 << 15, 4, 0, dict(ceiling=1 << 16, proven=1 << 15)),         # walk 3110-3121: the same in a look, 4 looks at least
        ("look 110 5000 2", 1 << 16, 3, 0),                                      # walk 3127, 3129: x4 stops at the ceiling
        ("look 120 6000 2", 1 << 16, 0, 0),                                      # walk 3129-3132: nowhere to grow, settled
    ])
    _play(check, [
        ("new 8192", 1 << 17, 0, 0),
        ("begin 0", 8192, 16, 0),
        ("batch 100 1000 1 0", 4096, 0, 0, dict(ceiling=8192)),                  # api 850: never below 4096
    ])


def test_d_a_fixed_span_makes_every_decision_inert(check):
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),
        ("begin 16384", 16384, 16, 0),                                           # api 794
        ("batch 900 1000 5 16384", 16384, 16, 0, dict(ceiling=NEVER, proven=0, adapt_pieces=0)),      # api 836: before any bookkeeping
        ("end 16384 100", 16384, 16, 0, dict(settled=0)),                        # api 1444
        ("begin 10", 64, 16, 0),                                                 # api 794: at least 64 ...
        ("begin %d" % (1 << 30), 1 << 26, 16, 0),                                # ... at most max_span
    ])


def test_e_a_second_scan_starts_a_quarter_below_where_the_first_settled(check):
    grow = [("batch %d %d 0 0" % (100 * i, 1000 * i), 1 << (18 + i), 16, 0) for i in range(1, 5)]      # 0.1 is clear: api 842, 866
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        grow[0],
        ("end 0 8", 1 << 19, 16, 0, dict(settled=0)),                            # api 1444: more than 8 windows
        ("begin 0", 1 << 18, 16, 0, dict(adapt_pieces=0, proven=1 << 18)),       # api 793: max(2^18, 0 / 4); what the context has proven stays
        *grow,
        ("end 0 9", 1 << 22, 16, 0, dict(settled=1 << 22)),                      # api 1444
        ("begin 0", 1 << 20, 16, 0, dict(ceiling=NEVER, adapt_pieces=0)),        # api 793-795: max(2^18, 2^22 / 4)
        ("end 0 9", 1 << 20, 16, 0, dict(settled=1 << 20)),
        ("begin 0", 1 << 18, 16, 0),                                             # api 793: max(2^18, 2^20 / 4)
    ])
    _play(check, [
        ("new %d" % (1 << 16), 1 << 17, 0, 0),
        ("begin 0", 1 << 16, 16, 0),                                             # api 795: capped by max_span
    ])


def test_f_the_look_at_a_window(check):
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        ("look 10 63 0", 1 << 18, 16, 0, dict(calib_pieces=0)),                  # walk 3123: fewer than 64 pieces decide nothing
        ("look 10 100 0", 1 << 20, 15, 0, dict(calib_pieces=100)),               # walk 3129, 3132: x4
        ("look 20 200 0", 1 << 22, 0, 0),                                        # walk 3136: 2^22 ends the looks
        ("batch 10 1000 0 0", 1 << 23, 2, 0, dict(proven=1 << 22)),              # api 866-867
        ("look 110 300 0", 1 << 22, 1, 0),                                       # walk 3128, 3136: a halving; the look shrank, so the looks go on
        ("look 120 400 0", 1 << 24, 0, 0),                                       # walk 3129, 3136
    ])
    _play(check, [
        ("new %d" % (1 << 26), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        ("look 40 100 0", 1 << 18, 0, 0),                                        # walk 3131-3132: "settled" ends the looks
    ])
    _play(check, [
        ("new %d" % (1 << 19), 1 << 17, 0, 0),
        ("begin 0", 1 << 18, 16, 0),
        ("look 10 100 0", 1 << 19, 15, 0),                                       # walk 3127, 3129: x4 up to the usual size
        ("look 20 200 0", 1 << 19, 0, 0),                                        # walk 3129-3131
    ])
    _play(check, [
        ("new 4096", 1 << 17, 0, 0),
        ("begin 0", 4096, 16, 0),
        ("look 90 100 0", 4096, 0, 0),                                           # walk 3128: no halving below 4096
    ])
