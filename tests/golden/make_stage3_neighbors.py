#!/usr/bin/env python3
"""Known answers of the reference's OWN JunctionMap::findNeighbor (utils/JunctionMap.cpp:231-412):
    make -C oracle ref && python tests/golden/make_stage3_neighbors.py
For every junction of a `.junctions` (reloaded with JunctionMap::buildFromFile) and every extension a contig would be built on,
oracle/_ref/ref_kat neighbors runs findNeighbor against a `.bloom` and prints the result; stored as stage3_neighbors_<name>.jsonl.gz.

The inputs:
  GOLDEN   the golden cases' own filter and map (static maps of a clean scan);
  FRESH    runs of the compiled reference made here at even and small k -- their reads, .bloom and .junctions become golden cases of the
           usual layout (tests/golden/<name>/), served by tests/golden_util.Case;
  VARIANTS seeded variants of some of both (tests/stage3_variants.py: thinned maps, damaged filters, shifted distances, a small
           max_read_length).  Only the reference's answers are stored for them; the tests derive the input again by the same recipe.

Every stored call is put into classes by the reference's answer and the map alone (tests/stage3_variants.py::classes_of); the counts per
fixture go to stage3_neighbors_summary.json, and the script fails unless every class is reached often enough over the whole set."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from faucet_amd import synth  # noqa: E402
from tests import stage3_variants as V  # noqa: E402
from tests.golden_util import Case  # noqa: E402

KAT = os.path.join(ROOT, "oracle", "_ref", "ref_kat")
# name: (k, genome length, planted repeats, repeat length, reads, read length, error rate, seed, further arguments)
FRESH = {
    "s3_k20": (20, 4000, 4, 150, 500, 100, 0.01, 61, []),
    "s3_k30": (30, 5000, 3, 200, 500, 120, 0.01, 63, []),
    "s3_k8": (8, 2500, 3, 60, 300, 80, 0.005, 65, ["-j", "2"]),
    "s3_k24_long": (24, 6000, 1, 100, 400, 200, 0.002, 67, ["-max_spacer_dist", "125"]),      # few junctions, spacers far apart: long walks
}
MAX_VARIANT_CALLS = 500          # stored per variant: every call of the classes a clean map hardly reaches and a seeded draw of the others
RARE = ("junction_before_maxdist", "junction_past_maxdist", "len_over_128", "dist_over_255")       # (the class minima are checked afterwards)


def written_here(path):
    rel = os.path.relpath(path, HERE).split(os.sep)
    return rel[0] in FRESH or rel[0].startswith("stage3_neighbors_")


def check_sizes():
    """no file this script writes is larger than the largest file under tests/golden that it does not write"""
    sizes = {os.path.join(d, f): os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(HERE) for f in fs}
    limit = max(n for p, n in sizes.items() if not written_here(p))
    too_large = {os.path.relpath(p, HERE): n for p, n in sizes.items() if written_here(p) and n > limit}
    assert not too_large, (limit, too_large)


def fresh_runs():
    import make_golden as G
    with tempfile.TemporaryDirectory() as td:
        for name, (k, glen, rep, replen, n, rl, err, seed, more) in FRESH.items():
            g = synth.make_genome(glen, seed, repeats=rep, repeat_len=replen)
            p = os.path.join(td, name + ".fa")
            synth.write_fasta(p, synth.make_reads(g, n, rl, err, seed + 1))
            G.run_case(name, p, False, ["-size_kmer", str(k), "-max_read_length", str(rl), "-estimated_kmers", "30000", "-singletons", "6000",
                                        "--no_cleaning"] + more)


def reference_calls(c, bloom, lines, max_read_length):
    """the lines `ref_kat neighbors` prints for this filter and map"""
    with tempfile.TemporaryDirectory() as td:
        b, j = os.path.join(td, "b.bloom"), os.path.join(td, "j.junctions")
        open(b, "wb").write(bloom.tobytes())
        open(j, "w").write("\n".join(lines) + "\n")
        tai = len(bloom) * 8
        r = subprocess.run([KAT, "neighbors", b, str(tai - 1), str(c.counters["n_hash"]), str(c.k), str(c.j), j, str(max_read_length)],
                           capture_output=True, text=True)
    out = [ln for ln in r.stdout.splitlines() if ln.startswith('{"kat":"neighbor"')]
    assert r.returncode == 0 and out, (c.name, r.returncode, r.stderr[-500:])
    return out


def store(name, out, lines, k, summary):
    """the fixture file, and its line of the summary"""
    path = os.path.join(HERE, f"stage3_neighbors_{name}.jsonl.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(("\n".join(out) + "\n").encode())
    n = summary[name] = dict(calls=len(out), **V.count_classes([json.loads(ln) for ln in out], lines, k))
    print(name, len(out), "calls,", n["abort"], "aborted by the reference's asserts;", n["len_over_128"], "long,", n["dist_over_255"], "far")


def main():
    assert tuple(FRESH) == V.FRESH_CASES
    fresh_runs()
    summary = {}
    for name in V.GOLDEN_CASES + V.FRESH_CASES:
        c = Case(name)
        out = reference_calls(c, c.bloom(), c.junction_lines(), c.max_read_length)
        store(name, out, c.junction_lines(), c.k, summary)
    for base, kinds in V.VARIANTS.items():
        c = Case(base)
        for kind in kinds:
            seed = V.seed_of(base, kind)
            bloom, lines, mrl = V.apply(kind, seed, c.bloom(), c.junction_lines(), c.max_read_length)
            out = reference_calls(c, bloom, lines, mrl)
            if len(out) > MAX_VARIANT_CALLS:
                keys, _, dist, _ = V.parse_map(lines)
                row = {int(x): i for i, x in enumerate(keys)}
                calls = [json.loads(ln) for ln in out]
                rare = np.array([any(cl in RARE for cl in V.classes_of(e, int(dist[row[int(e["start"], 16)], e["index"]]), c.k)) for e in calls])
                rest = np.nonzero(~rare)[0]
                take = np.random.default_rng(seed + 1).choice(rest, size=max(0, MAX_VARIANT_CALLS - int(rare.sum())), replace=False) if len(rest) else rest
                keep = np.sort(np.concatenate([np.nonzero(rare)[0], take]))
                out = [out[i] for i in keep]
            store(V.variant_name(base, kind), out, lines, c.k, summary)
    total = {cl: sum(s[cl] for s in summary.values()) for cl in V.CLASSES}
    print("total", total)
    short = {cl: (n, V.MINIMUM[cl]) for cl, n in total.items() if n < V.MINIMUM[cl]}
    assert not short, f"classes the fixtures do not reach often enough (have, need): {short} -- change seeds or fractions"
    with open(os.path.join(HERE, "stage3_neighbors_summary.json"), "w") as f:
        json.dump({"minimum": V.MINIMUM, "total": dict(calls=sum(s["calls"] for s in summary.values()), **total), "fixtures": summary}, f, indent=1)
        f.write("\n")
    check_sizes()


if __name__ == "__main__":
    main()
