#!/usr/bin/env python3
"""The reference's OWN <prefix>.raw_contigs.fasta (ContigGraph::printContigs on the graph JunctionMap::buildContigGraph returns,
src/Faucet.cpp:314) for the Stage-3 fixtures:
    make -C oracle ref && python tests/golden/make_raw_contigs_golden.py
tests/golden/raw_contigs_driver.cpp (our own text: it includes the reference's headers and calls public functions) is built by
oracle/Makefile (target ref) against the compiled reference's objects under oracle/_ref/obj; the binary goes to oracle/_ref/ and is
never committed.  For every fixture of tests/stage3_variants.py the driver reloads the map with JunctionMap::buildFromFile, writes the map's
iteration order (NOT the file's line order, and buildContigGraph depends on it), builds the graph and prints the contigs.  Stored:
raw_contigs_<name>.fasta.gz and raw_contigs_<name>.order.gz (hex k-mers, one per line).  The 13 unvaried fixtures must return; a variant is
kept only where the reference exits 0 within the time limit (its asserts, its endless loops and the crashes of its pointer reads are listed in
raw_contigs_summary.json under not_returned).  The script fails unless the set holds bubble records, kept and dropped isolated contigs, a
far_is_start contig, a sequence of exactly k bases and sequences on both sides of 32 and of 64 bases."""
import glob
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import stage3_variants as V  # noqa: E402
from tests.golden_util import Case  # noqa: E402

OUT = os.path.join(ROOT, "oracle", "_ref")


def reference_tree():
    """where the reference's sources lie: $REF, or what oracle/Makefile builds the objects from"""
    if os.environ.get("REF"):
        return os.environ["REF"]
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        return next(ln.split("?=")[1].strip() for ln in f if ln.startswith("REF") and "?=" in ln)


DRIVER = os.path.join(OUT, "raw_contigs_driver")
TIME_LIMIT = 10          # seconds per run (the unvaried fixtures take well under one)


def written_here(path):
    return os.path.relpath(path, HERE).startswith("raw_contigs_") and not path.endswith(".cpp")


def check_sizes():
    """no file this script writes is larger than the largest file under tests/golden that it does not write"""
    sizes = {os.path.join(d, f): os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(HERE) for f in fs}
    limit = max(n for p, n in sizes.items() if not written_here(p))
    too_large = {os.path.relpath(p, HERE): n for p, n in sizes.items() if written_here(p) and n > limit}
    assert not too_large, (limit, too_large)


def build_driver(driver=DRIVER):
    """oracle/Makefile holds the one recipe of both drivers"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "REF=" + reference_tree(), os.path.relpath(driver, os.path.join(ROOT, "oracle"))], check=True)


def reference_file(c, bloom, lines, max_read_length):
    """(fasta bytes, order text) of the driver on this filter and map, or (None, why) where the reference does not return"""
    with tempfile.TemporaryDirectory() as td:
        b, j, fa, od = (os.path.join(td, n) for n in ("b.bloom", "j.junctions", "out.fasta", "out.order"))
        open(b, "wb").write(bloom.tobytes())
        open(j, "w").write("\n".join(lines) + "\n")
        try:
            r = subprocess.run([DRIVER, b, str(len(bloom) * 8 - 1), str(c.counters["n_hash"]), str(c.k), str(c.j), j, str(max_read_length), fa, od],
                               capture_output=True, timeout=TIME_LIMIT)
        except subprocess.TimeoutExpired:
            return None, "no return within %d s" % TIME_LIMIT
        if r.returncode != 0:
            return None, "exit %d" % r.returncode
        return open(fa, "rb").read(), open(od).read()


def main():
    from tests import raw_contigs_ref as P
    from tests import test_raw_contigs_ref_cpu as T
    build_driver()
    for p in glob.glob(os.path.join(HERE, "raw_contigs_*.gz")):
        os.remove(p)
    kept, not_returned = {}, {}
    for name in V.fixture_names():
        c = Case(name.split("__")[0])
        bloom, lines, mrl = V.inputs_of(name, c)
        fasta, order = reference_file(c, bloom, lines, mrl)
        if fasta is None:
            assert "__" in name, (name, order)              # the unvaried fixtures return
            not_returned[name] = order
            print(name, "not kept:", order)
            continue
        assert len(order.split()) == len(lines)
        for kind, data in (("fasta", fasta), ("order", order.encode())):
            with gzip.GzipFile(os.path.join(HERE, f"raw_contigs_{name}.{kind}.gz"), "wb", mtime=0) as f:
                f.write(data)
        seqs = fasta.decode().split("\n")[1::2]
        kept[name] = dict(k=c.k, read_length=mrl, junctions=len(lines), bytes=len(fasta), shortest=min(map(len, seqs)), longest=max(map(len, seqs)))
    total = dict.fromkeys(("bubble_records", "isolated_kept", "isolated_dropped", "far_is_start", "exactly_k", "below_32", "above_32", "below_64", "above_64"), 0)
    for name, s in kept.items():
        b, keys, recs = T.golden_build(name)[:3]
        assert b.status == 0, name
        records, info = P.plan(b.calls, keys, recs["cov"], s["k"], s["read_length"])
        seqs = T.golden_fasta(name).decode().split("\n")[1::2]
        s.update(info, far_is_start=sum(w.far_is_start for w in b.calls), exactly_k=sum(len(x) == s["k"] for x in seqs), below_32=sum(len(x) < 32 for x in seqs),
                 above_32=sum(len(x) > 32 for x in seqs), below_64=sum(len(x) < 64 for x in seqs), above_64=sum(len(x) > 64 for x in seqs))
        assert info["records"] == len(seqs), (name, info, len(seqs))
        for key in total:
            total[key] += s[key]
        print(name, {key: s[key] for key in ("records", "bubble_records", "node_contigs", "isolated_kept", "isolated_dropped", "far_is_start", "exactly_k")})
    print("total", total)
    assert all(total.values()), f"the goldens do not reach: {[key for key, v in total.items() if not v]}"
    with open(os.path.join(HERE, "raw_contigs_summary.json"), "w") as f:
        json.dump({"total": total, "fixtures": kept, "not_returned": not_returned}, f, indent=1, sort_keys=True)
        f.write("\n")
    check_sizes()


if __name__ == "__main__":
    main()
