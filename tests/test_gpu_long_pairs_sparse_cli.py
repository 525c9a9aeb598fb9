"""The `faucet` command line with the long pair filter's sparse state (first-set times per batch instead of 4 bytes per filter bit,
faucet_amd/csrc/pairs.hip): on one GPU by FGPU_LONG_PAIRS_STATE=sparse, over 2 and 3 contexts through the automatic choice when the dense
form "does not fit" (FGPU_DEBUG_LONG_PAIRS_DENSE_NOMEM).  Every file is the compiled reference's golden, byte for byte, and the hosts say
on stderr which form the filter took.  Needs an MI355X."""
import pytest

from tests.golden_util import Case
from tests.test_gpu_multi import _run, _same_files

pytestmark = pytest.mark.gpu

PAIRED = ["pe_fastq_k21", "pe_repeats_k25", "pe_fasta_highcov_k31"]
NOTE = "keeps its first-set times per batch (sparse state)"


def _check(c, prefix, r):
    assert r.returncode == (0 if c.no_cleaning else 3), r.stdout[-2000:] + r.stderr[-3000:]
    _same_files(c, prefix)
    cn = c.counters
    assert f"Empty count: {cn['empty_count']}, not empty count: {cn['not_empty_count']}" in r.stdout
    assert r.stderr.count(NOTE) == 1 and "note: the long pair filter (" in r.stderr, r.stderr[-3000:]
    assert "the paired-end loop runs on the host" not in r.stderr


@pytest.mark.parametrize("case", PAIRED)
def test_cli_with_the_sparse_state_writes_the_reference_files(case, tmp_path):
    c = Case(case)
    prefix, r = _run(c, tmp_path, 1, env={"FGPU_LONG_PAIRS_STATE": "sparse", "FGPU_CLI_TIMES": "1"})
    _check(c, prefix, r)
    assert "first-set times sparse, at most " in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("gpus", [2, 3])
@pytest.mark.parametrize("case", PAIRED)
def test_sharded_cli_falls_to_the_sparse_state_and_writes_the_reference_files(case, gpus, tmp_path):
    c = Case(case)
    prefix, r = _run(c, tmp_path, gpus, env={"FGPU_DEBUG_LONG_PAIRS_DENSE_NOMEM": "1"})
    _check(c, prefix, r)
