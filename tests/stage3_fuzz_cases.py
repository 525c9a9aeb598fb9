"""Stage-3 inputs made on the spot: from a case id to (reads file, arguments), all seeded, to the map the compiled reference's `faucet_ref`
writes on those reads (.bloom, .junctions), and to what the reference's own Stage 3 says of that map (oracle/_ref/raw_contigs_driver,
detip_driver and, asked apart by chimera_answers, chimera_driver: tests/golden/*.cpp built by `make -C oracle ref`).  Nothing is stored but the
list of ids (tests/golden/stage3_fuzz_ids.json, written by tests/golden/make_stage3_fuzz_list.py, which also says which candidates the reference
did not return on and why).

A case id is "<family>-<seed>" or "<family>-<seed>__<kind>": kind is a recipe of tests/stage3_variants.py (drop30, shift, mrl10) applied to the
reference's own files before they go to the drivers -- the maps the contig-graph stage thins.  Families:

    rand      tests.test_oracle_vs_reference_fuzz.random_run as it is: single and paired end, FASTQ, --mercy, N, truncated reads
    tandem    a random unit of period 3, 7, 16, 53 or 120 tiled over about 1 500 bases between two random flanks
    runs      a random genome with A x 80, AT x 40, G x 50, ACGT x 20, CA x 45, T x 33 spliced in
    hairpin   five blocks of k+5 .. 4k bases, each followed by its own reverse complement after a spacer of 0 .. 5 bases
    circle    a genome of 2 .. 6 read lengths with its first read length appended, at extreme coverage

The four low-complexity families draw k from 8, 12, 15, 20, 21, 24, 31 and the error rate from 0, 0.005, 0.02; even seeds run with --no_cleaning.
These are the shapes a contig walk goes wrong on: cycles, homopolymer starts, sequences that are their own reverse complement, contigs that
return to their start."""
import atexit
import collections
import json
import os
import pathlib
import re
import shutil
import subprocess
import tempfile

import numpy as np

from tests import stage3_variants as V
from tests.golden_util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
REF_BIN, RAW_DRIVER, DETIP_DRIVER, CHIMERA_DRIVER = (os.path.join(REF, n) for n in ("faucet_ref", "raw_contigs_driver", "detip_driver", "chimera_driver"))
LIST = os.path.join(GOLDEN, "stage3_fuzz_ids.json")
FAMILIES = ("rand", "tandem", "runs", "hairpin", "circle")
LOW_K = (8, 12, 15, 20, 21, 24, 31)
ERRORS = (0.0, 0.005, 0.02)
KINDS = ("drop30", "shift", "mrl10")
TIME_LIMIT = 10          # seconds per run of a reference binary (each takes well under one)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

Map = collections.namedtuple("Map", "bloom lines k n_hash j max_read_length")
Answers = collections.namedtuple("Answers", "raw_fasta order detip_fasta table")


class NotReturned(Exception):
    """a reference binary did not exit 0 within the time limit on this id"""


def binaries_built():
    return all(os.path.exists(p) for p in (REF_BIN, RAW_DRIVER, DETIP_DRIVER))


def chimera_driver_built():
    """asked apart from binaries_built(): an oracle/_ref from before the driver had a recipe there still serves the tests of the two other drivers"""
    return binaries_built() and os.path.exists(CHIMERA_DRIVER)


def listed():
    """the committed list: {"ids": [...], "gpu_ids": [...], "rejected": {id: why}, "reached": {class: [ids]}}"""
    if not os.path.exists(LIST):                     # (only while tests/golden/make_stage3_fuzz_list.py is making it)
        return {"ids": [], "gpu_ids": [], "rejected": {}, "reached": {}}
    with open(LIST) as f:
        return json.load(f)


def split(case_id):
    """(family, seed, kind or None)"""
    base, _, kind = case_id.partition("__")
    family, seed = base.split("-")
    assert family in FAMILIES and (not kind or kind in KINDS), case_id
    return family, int(seed), kind or None


def _random(rng, n):
    return bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=n))


def _rc(s):
    return s.translate(_COMP)[::-1]


def genome_of(family, rng, k, read_length):
    if family == "tandem":
        unit = _random(rng, int(rng.choice([3, 7, 16, 53, 120])))
        return _random(rng, int(rng.integers(500, 1500))) + (unit * (1500 // len(unit) + 1))[:1500] + _random(rng, int(rng.integers(500, 1500)))
    if family == "runs":
        g = _random(rng, int(rng.integers(3000, 6000)))
        for run in (b"A" * 80, b"AT" * 40, b"G" * 50, b"ACGT" * 20, b"CA" * 45, b"T" * 33):
            at = int(rng.integers(0, len(g) + 1))
            g = g[:at] + run + g[at:]
        return g
    if family == "hairpin":
        g = _random(rng, int(rng.integers(150, 400)))
        for _ in range(5):
            block = _random(rng, int(rng.integers(k + 5, 4 * k + 1)))
            g += block + _random(rng, int(rng.integers(0, 6))) + _rc(block) + _random(rng, int(rng.integers(150, 400)))
        return g
    if family == "circle":
        g = _random(rng, int(rng.integers(2, 7)) * read_length)
        return g + g[:read_length]
    raise ValueError(family)


def reads_of(case_id, tmp_path):
    """(path of the reads file, fastq, arguments) of the id's run, written under `tmp_path`"""
    from faucet_amd import synth
    family, seed, _ = split(case_id)
    tmp_path = pathlib.Path(tmp_path)
    if family == "rand":
        from tests.test_oracle_vs_reference_fuzz import random_run
        return random_run(seed, tmp_path)
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    k, err, rl = int(rng.choice(LOW_K)), float(rng.choice(ERRORS)), int(rng.choice([60, 100, 150]))
    g = np.frombuffer(genome_of(family, rng, k, rl), dtype=np.uint8)
    n = 1500 if family == "circle" else int(rng.integers(300, 1501))
    reads = synth.make_reads(g, n, rl, err, 7000 + seed)
    path = str(tmp_path / "in.fa")
    synth.write_fasta(path, reads)
    args = ["-size_kmer", str(k), "-max_read_length", str(rl), "-estimated_kmers", "100000", "-singletons", "20000"]
    return path, False, args + (["--no_cleaning"] if seed % 2 == 0 else [])


def option(args, flag, default):
    return type(default)(args[args.index(flag) + 1]) if flag in args else default


def reference_run(path, args, out_dir):
    """`faucet_ref` on the reads: the CompletedProcess.  The reference goes on into its own contig graph where cleaning is on and may crash there,
    after its files were written; no end within the time limit is NotReturned"""
    os.makedirs(out_dir, exist_ok=True)
    try:
        return subprocess.run(["stdbuf", "-o0", REF_BIN, "-read_load_file", path, "-read_scan_file", path, "-file_prefix", os.path.join(out_dir, "out")] + args,
                              capture_output=True, text=True, errors="replace", timeout=TIME_LIMIT)
    except subprocess.TimeoutExpired:
        raise NotReturned("faucet_ref: no return within %d s" % TIME_LIMIT)


def map_from(out_dir, stdout, args, kind=None, seed=0):
    """the Map of a run's own files (`stdout`: the run's, for the hash count), variant `kind` applied"""
    bloom = np.fromfile(os.path.join(out_dir, "out.bloom"), dtype=np.uint8)
    with open(os.path.join(out_dir, "out.junctions")) as f:
        lines = f.read().split("\n")[:-1]
    mrl = option(args, "-max_read_length", 0)
    if kind:
        bloom, lines, mrl = V.apply(kind, seed, bloom, lines, mrl)
    n_hash = int(re.search(r"Number of hash functions: (\d+)", stdout).group(1))
    return Map(bloom, lines, option(args, "-size_kmer", 0), n_hash, option(args, "-j", 1), mrl)


def _driver(exe, m, td, outs):
    b, j = os.path.join(td, "b.bloom"), os.path.join(td, "j.junctions")
    m.bloom.tofile(b)
    with open(j, "w") as f:
        f.write("".join(ln + "\n" for ln in m.lines))
    try:
        r = subprocess.run([exe, b, str(len(m.bloom) * 8 - 1), str(m.n_hash), str(m.k), str(m.j), j, str(m.max_read_length)] + [os.path.join(td, o) for o in outs],
                           capture_output=True, timeout=TIME_LIMIT)
    except subprocess.TimeoutExpired:
        raise NotReturned("%s: no return within %d s" % (os.path.basename(exe), TIME_LIMIT))
    if r.returncode != 0:
        raise NotReturned("%s: exit %d" % (os.path.basename(exe), r.returncode))
    return r.stdout.decode(errors="replace")


def answers_of(m):
    """what the reference's Stage 3 says of a Map: its raw contig file, the order its reloaded map iterated in (keys), its file after
    deleteTipsAndClean and the graph table with the counts line (tests/detip_golden.py says how it reads)"""
    with tempfile.TemporaryDirectory() as td:
        _driver(RAW_DRIVER, m, td, ["raw.fasta", "raw.order"])
        with open(os.path.join(td, "raw.fasta"), "rb") as f:
            raw = f.read()
        with open(os.path.join(td, "raw.order")) as f:
            order = np.array([int(x, 16) for x in f.read().split()], dtype=np.uint64)
        said = _driver(DETIP_DRIVER, m, td, ["detip.fasta", "detip.graph"])
        tips = re.search(r"Deleted (\d+) tips\. (\d+) nodes left", said)
        removed = re.search(r"removed (\d+) collapsible nodes\.\s+(\d+) nodes left", said)
        counts = "counts %s %s %s\n" % (tips.group(1), removed.group(2) if removed else tips.group(2), removed.group(1) if removed else -1)
        with open(os.path.join(td, "detip.fasta"), "rb") as f:
            detip = f.read()
        with open(os.path.join(td, "detip.graph")) as f:
            table = f.read() + counts
    assert len(order) == len(m.lines)
    return Answers(raw, order, detip, table)


def chimera_answers_of(m):
    """what the reference says of a Map after removeChimerasAndClean behind deleteTipsAndClean (oracle/_ref/chimera_driver): (its contig file, its graph
    table with the counts line; tests/dechimera_golden.py says how it reads)"""
    from tests.dechimera_golden import counts_said
    with tempfile.TemporaryDirectory() as td:
        said = _driver(CHIMERA_DRIVER, m, td, ["chimera.fasta", "chimera.graph"])
        with open(os.path.join(td, "chimera.fasta"), "rb") as f:
            fasta = f.read()
        with open(os.path.join(td, "chimera.graph")) as f:
            return fasta, f.read() + counts_said(said)


# ---- one run of the reference per id and process -----------------------------------------------------------------------------------------------
_made, _runs, _chimera = {}, {}, {}
_scratch = []


def _scratch_dir():
    if not _scratch:
        _scratch.append(tempfile.mkdtemp(prefix="stage3_fuzz_"))
        atexit.register(shutil.rmtree, _scratch[0], ignore_errors=True)
    return _scratch[0]


def case_of(case_id):
    """(path of the reads, arguments, directory of faucet_ref's files, Map, Answers) of an id; made once, shared, left unchanged.  NotReturned where
    a reference binary does not return on it"""
    if case_id not in _made:
        try:
            _made[case_id] = _make(case_id)
        except NotReturned as e:
            _made[case_id] = e
    if isinstance(_made[case_id], NotReturned):
        raise _made[case_id]
    return _made[case_id]


def chimera_answers(case_id):
    """(fasta bytes, graph table with its counts line) of the chimera driver on an id's Map; made once, shared, left unchanged.  NotReturned as
    case_of"""
    if case_id not in _chimera:
        try:
            _chimera[case_id] = chimera_answers_of(case_of(case_id)[3])
        except NotReturned as e:
            _chimera[case_id] = e
    if isinstance(_chimera[case_id], NotReturned):
        raise _chimera[case_id]
    return _chimera[case_id]


def reference_stdout(case_id):
    """what `faucet_ref` printed on the reads of an id"""
    case_of(case_id)
    return _runs[case_id.partition("__")[0]][2]


def _make(case_id):
    family, seed, kind = split(case_id)
    base = case_id.partition("__")[0]
    d = os.path.join(_scratch_dir(), base)
    if base not in _runs:
        os.makedirs(d, exist_ok=True)
        path, _, args = reads_of(base, d)
        try:
            _runs[base] = (path, args, reference_run(path, args, os.path.join(d, "ref")).stdout)
        except NotReturned as e:
            _runs[base] = e
    if isinstance(_runs[base], NotReturned):
        raise _runs[base]
    path, args, stdout = _runs[base]
    if not os.path.exists(os.path.join(d, "ref", "out.junctions")):
        raise NotReturned("faucet_ref: wrote no .junctions")
    m = map_from(os.path.join(d, "ref"), stdout, args, kind, V.seed_of(base, kind) if kind else 0)
    return path, args, os.path.join(d, "ref"), m, answers_of(m)

