#!/usr/bin/env python3
"""Regenerate tests/golden/input_side/ from the COMPILED REFERENCE: what the reference's reading loop makes of malformed FASTA / FASTQ text.

Run in the build container only (needs oracle/_ref/faucet_ref):
    make -C oracle ref && python tests/golden/make_input_golden.py

Every case is a directory in the layout of the other goldens (tests/golden_util.py: Case):
  <case>/reads.f[aq].gz      the input text, byte for byte
  <case>/case.json           the arguments, the counters, and the reference's counter lines as printed ("counter_lines")
  <case>/out.bloom.gz, out.junctions.gz

The texts are built so that a wrong split cannot hide: headers, '+' lines and quality lines are ACGT strings with k-mers of their own
(k = 21), 20 of the 30 reads are 10 reads written twice (bloo2 and the junctions' coverages are not empty), and the filters stay at most
half full (asserted from "Weights after load").

Besides writing the fixtures this script pins tests/getline_ref.py to the reference, with no project code in between: the reference run on
the NORMALISED file -- every read of getline_ref.reads(text) written as ">\\nREAD\\n" -- gives the same .bloom, .junctions and counters.
And it asserts that the fixtures can tell: on the cases built for it, the normalised file made under the rule "an absent read is empty"
and the one made from the lines shifted by one give different reference output.

Only calls to the binary: no reference source text is read or stored."""
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import getline_ref as G  # noqa: E402

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "faucet_ref")
OUT = os.path.join(HERE, "input_side")
K = 21
BASE_ARGS = ["-size_kmer", str(K), "-max_read_length", "100", "-estimated_kmers", "20000", "-singletons", "4000", "--no_cleaning"]
COUNTER_LINES = ("Reads processed:", "Unambiguous reads:", "Weights after load:", "Distinct junctions:", "Empty count:")


def gz_write(path, data: bytes):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)


def acgt(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def make_records(fastq, seed, n_records=30):
    """records as lists of lines: header, read[, plus, quality], every line ACGT; reads 0..9 come back as reads 10..19"""
    rng = np.random.default_rng(seed)
    genome = acgt(rng, 700)                              # reads overlap: junctions need k-mers seen from several reads
    uniq = []
    for _ in range(n_records - 10):
        at, ln = int(rng.integers(0, 640)), int(rng.integers(36, 60))
        uniq.append(genome[at:at + ln])
    rd = uniq[:10] + uniq[:10] + uniq[10:]
    recs = []
    for r in rd:
        rec = [acgt(rng, int(rng.integers(22, 30))), r]
        if fastq:
            rec += [acgt(rng, int(rng.integers(22, 30))), acgt(rng, len(r))]
        recs.append(rec)
    return recs


def join(recs, eol=b"\n"):
    return b"".join(line + eol for rec in recs for line in rec)


def texts(fastq):
    """name -> (text, tags): "eof_header" = the last line is an unterminated header, "shift" = a blank line moves every line's role"""
    recs = make_records(fastq, 7 if fastq else 5)
    full = join(recs)
    once = recs[25][1]                                   # a read that occurs once: as the reused header it goes into bloo2
    extra = make_records(fastq, 11)[29]
    t = {
        "wellformed": (full, ["shift"]),
        "no_final_newline": (full[:-1], []),
        "header_unterminated": (full + once, ["eof_header"]),              # 31 records: odd
        "header_terminated": (full + once + b"\n", []),
        "sequence_unterminated": (full + extra[0] + b"\n" + extra[1], []),
        "blank_front": (b"\n" + full, ["shift"]),
        "blank_middle": (join(recs[:11]) + b"\n" + join(recs[11:]), ["shift"]),
        "blank_end": (full + b"\n\n\n", []),
        "crlf": (join(recs, b"\r\n"), []),
        "single_line": (recs[0][1], ["eof_header"]),
        "newline_alone": (b"\n", []),
    }
    if fastq:
        head = full + extra[0] + b"\n" + extra[1] + b"\n"
        t["ends_in_plus"] = (head + extra[2], [])
        t["ends_in_plus_newline"] = (head + extra[2] + b"\n", [])
        t["ends_inside_quality"] = (head + extra[2] + b"\n" + extra[3][:30], [])
        t["blank_middle_unterminated"] = (join(recs[:11]) + b"\n" + join(recs[11:])[:-1], ["eof_header"])   # the shift makes the last line a header
    return t


def run_reference(text, fastq, args, td, tag):
    inp = os.path.join(td, tag + (".fq" if fastq else ".fa"))
    with open(inp, "wb") as f:
        f.write(text)
    prefix = os.path.join(td, tag)
    p = subprocess.run(["stdbuf", "-o0", REF_BIN, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix] + args,
                       capture_output=True, text=True, errors="replace", timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"{tag}: reference exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    # (the scan's progress line "\rreads scanned: N" has no newline of its own: "Empty count" follows it on the same line)
    lines = [m.group(0).strip() for ln in p.stdout.replace("\r", "\n").splitlines() for m in [re.search("(%s).*" % "|".join(COUNTER_LINES), ln)] if m]
    with open(prefix + ".bloom", "rb") as f:
        bloom = f.read()
    with open(prefix + ".junctions", "rb") as f:
        junctions = f.read()
    return {"bloom": bloom, "junctions": junctions, "lines": lines}


def normalised(reads):
    return b"".join(b">\n" + r + b"\n" for r in reads)


def absent_read_is_empty(text, fastq):
    """the rule the project had: the reads, but a last header line without its newline is followed by an empty read"""
    reads = G.reads(text, fastq)
    if text and not text.endswith(b"\n") and text.count(b"\n") % (4 if fastq else 2) == 0:
        reads[-1] = b""
    return reads


def main():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    total = 0
    with tempfile.TemporaryDirectory() as td:
        for fastq in (False, True):
            for name, (text, tags) in texts(fastq).items():
                assert len(text) < 8192, (name, len(text))
                for paired in (False, True):
                    case = f"{'fq' if fastq else 'fa'}_{name}_{'pe' if paired else 'se'}"
                    args = BASE_ARGS + (["--fastq"] if fastq else []) + (["--paired_ends"] if paired else [])
                    norm_args = BASE_ARGS + (["--paired_ends"] if paired else [])
                    ref = run_reference(text, fastq, args, td, case)
                    rp = [int(x) for x in re.findall(r"Reads processed: (\d+)", "\n".join(ref["lines"]))]
                    ur = [int(x) for x in re.findall(r"Unambiguous reads: (\d+)", "\n".join(ref["lines"]))]
                    w = re.findall(r"Weights after load: ([0-9.]+), ([0-9.]+)", "\n".join(ref["lines"]))[0]
                    assert float(w[0]) <= 0.5 and float(w[1]) <= 0.5, (case, w)
                    assert len(rp) == 2 and len(ur) == 2 and len(ref["lines"]) == 7, ref["lines"]
                    # the restatement against the reference, nothing of the project in between
                    reads = G.reads(text, fastq)
                    assert rp == [len(reads)] * 2, (case, rp, len(reads))
                    assert run_reference(normalised(reads), False, norm_args, td, case + "_norm") == ref, case
                    if "eof_header" in tags:
                        assert reads[-1] and run_reference(normalised(absent_read_is_empty(text, fastq)), False, norm_args, td, case + "_old") != ref, case
                    if "shift" in tags:
                        shifted = G.reads(text[text.index(b"\n") + 1:], fastq)
                        assert run_reference(normalised(shifted), False, norm_args, td, case + "_shift") != ref, case
                    out = os.path.join(OUT, case)
                    os.makedirs(out)
                    gz_write(os.path.join(out, "reads.fq.gz" if fastq else "reads.fa.gz"), text)
                    gz_write(os.path.join(out, "out.bloom.gz"), ref["bloom"])
                    gz_write(os.path.join(out, "out.junctions.gz"), ref["junctions"])
                    counters = {"load_reads_processed": rp[0], "scan_reads_processed": rp[1], "load_unambiguous": ur[0], "scan_unambiguous": ur[1],
                                "weights_after_load": list(w)}
                    with open(os.path.join(out, "case.json"), "w") as f:
                        json.dump({"name": case, "fastq": fastq, "args": args, "tags": tags, "ref_exit": 0, "counters": counters,
                                   "counter_lines": ref["lines"]}, f, indent=1)
                        f.write("\n")
                    size = sum(os.path.getsize(os.path.join(out, x)) for x in os.listdir(out))
                    total += size
                    print(case, len(text), "bytes of text,", len(reads), "reads,", ur, w, ref["junctions"].count(b"\n"), "junctions,", size, "bytes")
    print("total", total, "bytes")
    assert total < 150_000, total


if __name__ == "__main__":
    main()
