"""tests/fastg_ref.py and the host plan held to THE REFERENCE'S OWN FASTG: `faucet_ref` run from the goldens' reads WITH cleaning writes
<prefix>.cleaned_graph_unitigs.fastg.  Where the reference's final graph IS its dechimered graph -- decided from reference data only
(tests/fastg_cases.reference_final_graph) -- the file has to be what the restatement prints from oracle/_ref/chimera_driver's table on the same
run's .bloom / .junctions.  The reference's file comes from its in-process map, whose nodeMap order and contig orientations are not those of the
reloaded map the driver sees, so the comparison is free of order and orientation: every header/sequence half becomes (own (length, coverage
text), the neighbours' (length, coverage text), sequence), and the multisets must be equal.  Primes and file order are held by
tests/test_fastg_plan_cpu.py.  The sequences are tests/detip_ref.join over the piece lists of the host plan (tests/host/fastg_plan_check.cpp, under
the sanitizers).  No GPU; skipped where oracle/_ref was not built."""
import shutil

import pytest

from tests import fastg_cases as FC
from tests import fastg_ref as F
from tests import stage3_fuzz_cases as S

pytestmark = pytest.mark.skipif(not S.chimera_driver_built(), reason="oracle/_ref/faucet_ref and the three Stage-3 drivers were not built (make -C oracle ref)")


def test_the_restatement_prints_the_references_final_graph_where_it_is_the_dechimered_graph(tmp_path):
    from tests.test_stage3_fuzz_cpu import restated
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = FC.compile_check(str(tmp_path / "fastg_plan_check"))
    qualified, left = [], {}
    for name in FC.golden_reads():
        why, _, _, text, m, table = FC.reference_final_graph(name, tmp_path / name)
        if why:
            left.setdefault(why, []).append(name)
            continue
        a = restated(m, S.answers_of(m))
        plan = FC.run_plan(exe, str(tmp_path / name / "plan.bin"), a.keys, a.recs, a.build.calls, m.k, m.max_read_length, "dechimera")
        assert plan.status == 0, name
        want = FC.expected(table, plan.contigs, a.build.calls, m.k, m.max_read_length)[0]
        assert plan.text == want, name
        assert F.halves(want) == F.halves(text), name
        qualified.append((name, sum(FC.names_of(text).values())))
    print("qualified", qualified, "left out", left)
    assert len(qualified) >= 4, (qualified, left)
