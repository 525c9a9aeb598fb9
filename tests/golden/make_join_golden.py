#!/usr/bin/env python3
"""What the compiled reference's ContigJuncList makes of the hand-made piece lists of tests/join_cases.py:
    make -C oracle ref && python tests/golden/make_join_golden.py
tests/golden/join_driver.cpp (our own text: it includes the reference's headers and calls public functions -- ContigJuncList::reverse,
::concatenate, ::getAvgCoverage) is built against the compiled reference's objects under oracle/_ref/obj, as make_raw_contigs_golden.py builds
its driver; the binary goes to oracle/_ref/ and is never committed.  Stored: join_concat.json.gz -- per k (8, 21, 31) and list its name and
the joined sequence, distances, coverages and average coverage (17 significant digits).  The inputs are not stored: the tests make them again
from the same seed and fail if a name or a count differs.  The script fails unless the set holds a join of five pieces, a flipped piece
inside a chain, a middle piece without bases of its own, a coverage entry that is the minimum over four and more, and joined lengths of 31,
32, 33, 63, 64 and 65 bases."""
import glob
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import join_cases  # noqa: E402
from tests.golden.make_raw_contigs_golden import OUT, reference_tree  # noqa: E402

DRIVER = os.path.join(OUT, "join_driver")
KS = (8, 21, 31)


def build_driver():
    objs = [o for o in sorted(glob.glob(os.path.join(OUT, "obj", "*.o")))
            if os.path.basename(o) not in ("Faucet.o", "Faucet_nomain.o", "binding.o", "wrap_shim.o")]
    assert objs, "make -C oracle ref first"
    subprocess.run(["g++", "-std=c++11", "-O1", "-w", "-include", "vector", "-include", "cmath", "-I" + reference_tree(),
                    os.path.join(HERE, "join_driver.cpp")] + objs + ["-o", DRIVER], check=True)


def reference_joins(t):
    text = ["%d %d" % (t.k, len(t.lists))]
    for pieces in t.lists:
        text.append(str(len(pieces)))
        for c, flip in pieces:
            s, d, v = t.contigs[c]
            text.append(" ".join(map(str, [int(flip), s, len(d)] + d + [len(v)] + v)))
    r = subprocess.run([DRIVER], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert len(lines) == 4 * len(t.lists) + 1 and lines[-1] == ""
    return [dict(name=name, seq=lines[4 * i], dist=[int(x) for x in lines[4 * i + 1].split()], cov=[int(x) for x in lines[4 * i + 2].split()], avg=lines[4 * i + 3])
            for i, name in enumerate(t.names)]


def main():
    build_driver()
    stored = {}
    reached = dict.fromkeys(("five_pieces", "flip_inside", "middle_without_bases", "minimum_over_4", "len31", "len32", "len33", "len63", "len64", "len65"), 0)
    for k in KS:
        t = join_cases.cases(k)
        stored[str(k)] = got = reference_joins(t)
        for pieces, g in zip(t.lists, got):
            reached["five_pieces"] += len(pieces) >= 5
            reached["flip_inside"] += any(flip for _, flip in pieces[1:-1])
            reached["middle_without_bases"] += any(len(t.contigs[c][0]) == k for c, _ in pieces[1:-1])
            single = [len(t.contigs[c][2]) == 1 for c, _ in pieces[1:-1]]
            reached["minimum_over_4"] += any(a and b for a, b in zip(single, single[1:]))
            if "len%d" % len(g["seq"]) in reached:
                reached["len%d" % len(g["seq"])] += 1
    print(reached)
    assert all(reached.values()), f"the lists do not reach: {[key for key, v in reached.items() if not v]}"
    with gzip.GzipFile(os.path.join(HERE, "join_concat.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(stored, sort_keys=True).encode())
    assert os.path.getsize(os.path.join(HERE, "join_concat.json.gz")) < 200 << 10


if __name__ == "__main__":
    main()
