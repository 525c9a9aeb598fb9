"""The join of contigs restated (tests/detip_ref.py) against the compiled reference's ContigJuncList, without a device: join() -- reverse and
concatenate as the reference words them -- equals tests/golden/join_concat.json.gz (made by tests/golden/make_join_golden.py from the same
hand-made lists, tests/join_cases.py) list for list, and join_by_entry() -- the index arithmetic of faucet_amd/csrc/stage3_join.hip's kernels,
every output element on its own -- equals join()."""
import gzip
import json
import os

import pytest

from tests import contig_ref as R
from tests import detip_ref as J
from tests.join_cases import cases

KS = (8, 21, 31)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "join_concat.json.gz")
_golden = {}


def golden(k):
    if not _golden:
        with gzip.open(GOLDEN, "rt") as f:
            _golden.update(json.load(f))
    return _golden[str(k)]


def same_as_golden(k, names, got):
    """got: (sequence, distances, coverages, average) per list"""
    want = {g["name"]: g for g in golden(k)}
    assert len(want) == len(golden(k))
    for name, (s, d, c, avg) in zip(names, got):
        g = want[name]
        assert (s, list(d), list(c), "%.17g" % avg) == (g["seq"], g["dist"], g["cov"], g["avg"]), name


@pytest.mark.parametrize("k", KS)
def test_restated_join_equals_the_compiled_references(k):
    t = cases(k)
    assert t.names == [g["name"] for g in golden(k)]
    got = J.join(t.contigs, t.lists, k)
    same_as_golden(k, t.names, got)
    assert [g[0] for g in got] == t.masters                                    # pieces that overlap by k bases give back what they were cut from
    for pieces, (s, d, c, _) in zip(t.lists, got):
        assert len(d) == sum(len(t.contigs[p][1]) for p, _ in pieces) and len(c) == sum(len(t.contigs[p][2]) for p, _ in pieces) - (len(pieces) - 1)


@pytest.mark.parametrize("k", KS)
def test_join_found_entry_by_entry_equals_the_join_left_to_right(k):
    t = cases(k)
    assert J.join_by_entry(t.contigs, t.lists, k) == J.join(t.contigs, t.lists, k)


def test_the_lists_reach_what_they_are_for():
    t = cases(21)
    by_name = dict(zip(t.names, J.join(t.contigs, t.lists, 21)))
    pieces = dict(zip(t.names, t.lists))
    covs = [t.contigs[c][2] for c, _ in pieces["run_of_4"]]
    assert [len(c) for c in covs] == [3, 1, 1, 2] and len(by_name["run_of_4"][2]) == 4
    run = [covs[0][2], covs[1][0], covs[2][0], covs[3][0]]                     # (neither end piece is flipped)
    assert by_name["run_of_4"][2][2] == min(run)
    assert {len(by_name["len%d_three" % n][0]) for n in (31, 32, 33, 63, 64, 65)} == {31, 32, 33, 63, 64, 65}
    assert len(by_name["all_single_coverages"][2]) == 1
    assert max(len(g[2]) for g in by_name.values()) > 64 and max(len(p) for p in t.lists) >= 5


@pytest.mark.parametrize("k", KS)
def test_reversing_a_joined_contig_reverses_its_list_and_toggles_the_flips(k):
    t = cases(k)
    forward = J.join(t.contigs, t.lists, k)
    backward = J.join(t.contigs, [J.reverse_list(p) for p in t.lists], k)
    for name, (s, d, c, avg), (rs, rd, rc, ravg) in zip(t.names, forward, backward):
        assert (rs, rd, rc, ravg) == (R.revcomp_string(s), d[::-1], c[::-1], avg), name


def test_records_as_the_library_lays_them_out():
    from faucet_amd import api
    assert api.JOIN_PIECE_DTYPE.itemsize == 8 and api.JOINED_DTYPE.itemsize == 48
    assert hasattr(api.Context, "stage3_join")
