#!/usr/bin/env python3
"""Goldens at the filter shapes the other makers never reach, made by the compiled reference with make_golden.run_case's recipe:
    make -C oracle ref && python tests/golden/make_shapes_golden.py
  se_fp7_k21            single ends with cleaning, -fp for 7 hash functions, -estimated_kmers near the real count (bloo2 about a third full)
  pe_mercy_fp6_k21      interleaved FASTQ, --mercy, -fp for 6 hash functions
  onehash_k25           -singletons 0.95 x -estimated_kmers: one hash function
  j6_k21, j8_k23        -j 6 and -j 8 at three hash functions on sparse filters.  The reference's JChecker keeps at most 1000 k-mers per
                        level (utils/JChecker.cpp:92-93); every jcheck the scan could make here (from every extension in the filter of every
                        k-mer of the reads, both strands) is replayed on the reference's .bloom and the largest level is stored as
                        "max_jcheck_level" in case.json -- it has to stay far below that limit
  restart_bloomfile_fp6_k21   -bloom_file with -fp 0.01: the restarted filter is sized from -fp alone (6 hash functions); the .bloom handed in
                        comes from a run at six hash functions of the same size (make_restart_golden.py's layout)
Each case records the hash count the reference printed; the maker checks it is the one aimed at."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import make_restart_golden as R  # noqa: E402
from faucet_amd import synth  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests.golden_util import Case, fp_for  # noqa: E402


def write_records(path, lines, fastq):
    with open(path, "wb") as f:
        for i, s in enumerate(lines):
            f.write((b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n") if fastq else (b">r%d\n" % i + s + b"\n"))


def nh_from_reads(E, S, fp):
    return po.sizing_from_cli(E, S, fp)[1]


def max_jcheck_level(c):
    """the largest level JChecker::jcheck (utils/JChecker.cpp:51-80) fills for any extension in bloo2 of any k-mer of the reads"""
    lib = po.lib()
    tai, nh, _, _ = po.sizing_from_cli(c.E, c.S, c.fp)
    b = po.Bloom(tai, nh)
    b.set_bits(c.bloom())
    k, mask = c.k, (1 << (2 * c.k)) - 1
    has = lambda x: lib.fo_bloom_old_contains(b.h, lib.fo_canon(x, k))      # noqa: E731
    best = 0
    for line in c.lines():
        s = line.upper()
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if any(ch not in b"ACGT" for ch in w):
                continue
            x = lib.fo_encode(w, k)
            for kmer in (x, lib.fo_revcomp(x, k)):
                for nt in range(4):
                    e = ((kmer << 2) | nt) & mask
                    if not has(e):
                        continue
                    level = [e]
                    for _ in range(c.j):
                        level = [n for y in level for n in (((y << 2) | t) & mask for t in range(4)) if has(n)]
                        best = max(best, len(level))
                        if not level:
                            break
    return best


def make(name, path, fastq, args, want_nh):
    G.run_case(name, path, fastq, args, tolerate_crash=True)
    c = Case(name)
    assert c.counters["n_hash"] == want_nh == nh_from_reads(c.E, c.S, c.fp), (name, c.counters["n_hash"], want_nh)
    if c.j >= 5:
        m = max_jcheck_level(c)
        assert m < 100, (name, m)
        c.meta["max_jcheck_level"] = m
        with open(os.path.join(c.dir, "case.json"), "w") as f:
            json.dump(c.meta, f, indent=1)
            f.write("\n")
    print(name, c.counters["n_hash"], c.meta.get("max_jcheck_level"))


def main():
    with tempfile.TemporaryDirectory() as td:
        g = synth.make_genome(5000, 101, repeats=3, repeat_len=150)
        r = synth.make_reads(g, 1000, 100, 0.01, 102)
        p = os.path.join(td, "se.fa")
        write_records(p, [bytes(x) for x in np.ascontiguousarray(r)], False)
        E, S = 9000, 1800
        make("se_fp7_k21", p, False, ["-size_kmer", "21", "-max_read_length", "100", "-estimated_kmers", str(E), "-singletons", str(S),
                                      "-fp", str(fp_for(E, S, 7, nh_from_reads))], 7)

        g = synth.make_genome(6000, 111, repeats=3, repeat_len=180)
        r = synth.make_pairs(g, 320, 100, 280, 25, 0.02, 112)
        p = os.path.join(td, "pem.fq")
        write_records(p, [bytes(x) for x in np.ascontiguousarray(r)], True)
        E, S = 100000, 20000
        make("pe_mercy_fp6_k21", p, True, ["-size_kmer", "21", "-max_read_length", "100", "-estimated_kmers", str(E), "-singletons", str(S),
                                           "-fp", str(fp_for(E, S, 6, nh_from_reads)), "--fastq", "--paired_ends", "--mercy"], 6)

        g = synth.make_genome(5000, 121, repeats=3, repeat_len=150)
        r = synth.make_reads(g, 800, 100, 0.01, 122)
        p = os.path.join(td, "one.fa")
        write_records(p, [bytes(x) for x in np.ascontiguousarray(r)], False)
        make("onehash_k25", p, False, ["-size_kmer", "25", "-max_read_length", "100", "-estimated_kmers", "100000", "-singletons", "95000"], 1)

        for name, k, j, seed in (("j6_k21", 21, 6, 131), ("j8_k23", 23, 8, 141)):
            g = synth.make_genome(5000, seed, repeats=3, repeat_len=150)
            r = synth.make_reads(g, 800, 100, 0.015, seed + 1)
            p = os.path.join(td, name + ".fq")
            write_records(p, [bytes(x) for x in np.ascontiguousarray(r)], True)
            make(name, p, True, ["-size_kmer", str(k), "-max_read_length", "100", "-estimated_kmers", "200000", "-singletons", "40000",
                                 "-j", str(j), "--fastq", "--no_cleaning"], 3)

        # -bloom_file at -fp 0.01: a 6-function .bloom of the size create_bloom_filter_optimal(E, 0.01) gives
        E, S = 40000, 8000
        _, tai, nh = po.size_optimal(E, np.float32(0.01))
        fp6 = fp_for(E, S, 6, nh_from_reads)
        assert nh == 6 and po.sizing_from_cli(E, S, fp6)[:2] == (tai, 6)
        g = synth.make_genome(4000, 151, repeats=3, repeat_len=150)
        r = synth.make_reads(g, 1000, 100, 0.01, 152)
        fa = os.path.join(td, "reads.fa")
        synth.write_fasta(fa, r)
        common = ["-size_kmer", "21", "-max_read_length", "100", "-estimated_kmers", str(E), "-singletons", str(S)]
        io = ["-read_load_file", fa, "-read_scan_file", fa]
        R.run(io + ["-file_prefix", os.path.join(td, "first"), "-fp", str(fp6), "--no_cleaning"] + common)
        bloom = open(os.path.join(td, "first.bloom"), "rb").read()
        assert len(bloom) == tai // 8
        name = "restart_bloomfile_fp6_k21"
        out = os.path.join(HERE, name)
        os.makedirs(out, exist_ok=True)
        args = common + ["-fp", "0.01", "--no_cleaning"]
        text = R.run(io + ["-file_prefix", os.path.join(td, name), "-bloom_file", os.path.join(td, "first.bloom")] + args)
        cn = R.counters(text)
        assert cn["n_hash"] == 6 and cn["distinct_junctions"] > 50, cn
        R.gz(os.path.join(out, "reads.fa.gz"), open(fa, "rb").read())
        R.gz(os.path.join(out, "in.bloom.gz"), bloom)
        R.gz(os.path.join(out, "out.junctions.gz"), open(os.path.join(td, name + ".junctions"), "rb").read())
        with open(os.path.join(out, "case.json"), "w") as f:
            json.dump({"name": name, "fastq": False, "args": args, "counters": cn}, f, indent=1)
            f.write("\n")
        print(name, cn)


if __name__ == "__main__":
    main()
