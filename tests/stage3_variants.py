"""Inputs of JunctionMap::findNeighbor beyond the static map of a clean scan: seeded variants of a case's (.bloom, .junctions, max_read_length).

A golden case gives findNeighbor the map exactly as the scan left it and the filter exactly as the load left it, so no walk meets a junction
that is not where a distance says, a filter bit that is missing, or a distance that is off.  The contig-graph stage does: it removes junctions
as it goes, and nothing ties a `.junctions` file to the `.bloom` it is read next to.  Each recipe below makes one such input from a case by a
seeded draw.  tests/golden/make_stage3_neighbors.py applies them before it asks the compiled reference, tests/test_stage3_walker.py applies
them before it asks the walker and the kernel -- so only the reference's ANSWERS are stored for a variant, never its input.

    drop30, drop70   30 % / 70 % of the junctions removed (the map as the contig-graph stage thins it: walks run on past maxDist)
    zero02, zero2    about 0.2 % / 2 % of the filter's bytes zeroed (true k-mers vanish: the reference's asserts trip)
    shift            about 30 % of the non-zero distances moved by -3..+3, clamped to 1..255 (junctions before, at and past maxDist)
    mrl10            called with max_read_length 10, far below the run's (the walk past maxDist gives up early)

A .junctions line is "<k-mer> d d d d d  c c c c csum  l l l l l " (utils/Junction.cpp:74-89), extensions A, C, T, G, back."""
import zlib

import numpy as np

KINDS = ("drop30", "drop70", "zero02", "zero2", "shift", "mrl10")
# the fixtures tests/golden/stage3_neighbors_<name>.jsonl.gz: golden cases as they are, runs of the reference made for these tests (even and
# small k, long walks; tests/golden/make_stage3_neighbors.py::FRESH), and the variants stored of some of both
GOLDEN_CASES = ("c1_k21", "ragged_k31", "twohash_k31_L150", "j2_spacer20_k15", "j0_k15", "j6_k21", "j8_k23", "onehash_k25", "se_fp7_k21")
FRESH_CASES = ("s3_k20", "s3_k30", "s3_k8", "s3_k24_long")
VARIANTS = {"c1_k21": KINDS, "twohash_k31_L150": KINDS, "s3_k20": KINDS, "s3_k8": KINDS,
            "ragged_k31": ("drop30", "drop70"), "j0_k15": ("drop30", "drop70"), "s3_k30": ("drop30", "drop70"),
            "s3_k24_long": ("drop30", "drop70", "shift")}
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}


def seed_of(case_name, kind):
    """the seed of variant `kind` of case `case_name` (a CRC of both names: stable across runs and Python versions)"""
    return zlib.crc32(f"{case_name}/{kind}".encode())


def variant_name(case_name, kind):
    return f"{case_name}__{kind}"


def fixture_names():
    return list(GOLDEN_CASES + FRESH_CASES) + [variant_name(base, kind) for base, kinds in VARIANTS.items() for kind in kinds]


def inputs_of(name, case):
    """(filter bytes, .junctions lines, max_read_length) of fixture `name`; case = tests.golden_util.Case of the part before "__" """
    bloom, lines, mrl = case.bloom(), case.junction_lines(), case.max_read_length
    if "__" in name:
        base, kind = name.split("__")
        bloom, lines, mrl = apply(kind, seed_of(base, kind), bloom, lines, mrl)
    return bloom, lines, mrl


def apply(kind, seed, bloom, lines, max_read_length):
    """variant `kind` of (filter bytes, .junctions lines, max_read_length), drawn from `seed`; the inputs are left as they are"""
    rng = np.random.default_rng(seed)
    bloom = np.array(bloom, dtype=np.uint8)
    lines = list(lines)
    if kind in ("drop30", "drop70"):
        keep = rng.random(len(lines)) >= (0.3 if kind == "drop30" else 0.7)
        lines = [ln for ln, kp in zip(lines, keep) if kp]
    elif kind in ("zero02", "zero2"):
        bloom[rng.random(len(bloom)) < (0.002 if kind == "zero02" else 0.02)] = 0
    elif kind == "shift":
        out = []
        for ln in lines:
            f = ln.split()
            d = [int(v) for v in f[1:6]]
            move = rng.random(5) < 0.3
            by = rng.integers(-3, 4, size=5)
            d = [min(255, max(1, v + int(b))) if (v and m) else v for v, m, b in zip(d, move, by)]
            out.append(f"{f[0]} {' '.join(map(str, d))}  {' '.join(f[6:11])}  {' '.join(f[11:16])} ")
        lines = out
    elif kind == "mrl10":
        max_read_length = 10
    else:
        raise ValueError(kind)
    return bloom, lines, max_read_length


def parse_map(lines):
    """(keys, cov[n, 4], dist[n, 5], linked[n, 5]) of .junctions lines, keys as JunctionMap keys them"""
    keys = np.zeros(len(lines), dtype=np.uint64)
    cov, dist, linked = np.zeros((len(lines), 4), np.uint8), np.zeros((len(lines), 5), np.uint8), np.zeros((len(lines), 5), np.uint8)
    for i, ln in enumerate(lines):
        f = ln.split()
        x = 0
        for ch in f[0]:
            x = (x << 2) | CODE[ch]
        keys[i] = x
        dist[i], cov[i], linked[i] = [int(v) for v in f[1:6]], [int(v) for v in f[6:10]], [int(v) for v in f[11:16]]
    return keys, cov, dist, linked


# ---- the classes of calls the fixtures have to reach (decided from the reference's answer and the map alone) ----
CLASSES = ("abort", "junction_before_maxdist", "junction_at_maxdist", "junction_past_maxdist", "sink", "len_over_128", "dist_over_255",
           "len_at_word_edge", "even_k", "start_index_4", "start_index_below_4")
MINIMUM = dict({c: 5 for c in CLASSES}, abort=100)


def classes_of(call, maxdist, k):
    """the classes one recorded call (a line of `ref_kat neighbors`) belongs to; `maxdist` = the start junction's dist[index]
    (junction_before_maxdist takes in the junctions the first one or two k-mers return at dist 1 or 2 as well as those of the scan loop)"""
    out = ["start_index_4" if call["index"] == 4 else "start_index_below_4"]
    if k % 2 == 0:
        out.append("even_k")
    if call.get("abort"):
        return out + ["abort"]
    if call["node"]:
        out.append("junction_before_maxdist" if call["dist"] < maxdist else "junction_at_maxdist" if call["dist"] == maxdist else "junction_past_maxdist")
    else:
        out.append("sink")
    if call["len"] > 128:
        out.append("len_over_128")
    if call["dist"] > 255:
        out.append("dist_over_255")
    if call["len"] % 32 in (31, 0, 1):
        out.append("len_at_word_edge")
    return out


def count_classes(calls, lines, k):
    keys, _, dist, _ = parse_map(lines)
    row = {int(x): i for i, x in enumerate(keys)}
    n = dict.fromkeys(CLASSES, 0)
    for e in calls:
        for c in classes_of(e, int(dist[row[int(e["start"], 16)], e["index"]]), k):
            n[c] += 1
    return n
