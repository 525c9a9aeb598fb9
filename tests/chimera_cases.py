"""Seeded maps for ContigGraph::removeChimerasAndClean beside the goldens: ids of tests/stage3_fuzz_cases.py (the reads, the reference's own map of
them and its answers are made on the spot where oracle/_ref is built; nothing but the ids is stored).

The 28 goldens reach every outcome of the step but one: on none of them does validateNoneCollapsible, run behind the step, erase a node.  The
seeded maps do -- VALIDATION_IDS: the reference's own count line says so on each ("removed N collapsible nodes", N > 0: long tandem repeats,
hairpins and circles at extreme coverage, where one cut leaves a node with a single path out that the loop has already passed) -- and
SPOT_IDS are the 24 maps tests/test_dechimera_plan_cpu.py asks the compiled reference about on the spot: every family, thinned variants, maps the
step leaves alone, and the VALIDATION_IDS."""
VALIDATION_IDS = ["tandem-9", "hairpin-4", "circle-0", "circle-6", "circle-7", "circle-9__mrl10"]
SPOT_IDS = VALIDATION_IDS + ["rand-100", "rand-101", "rand-104", "rand-108", "rand-113", "tandem-0", "tandem-2", "runs-1", "runs-6", "hairpin-7", "hairpin-9",
                             "circle-1", "circle-4", "rand-100__drop30", "rand-108__mrl10", "tandem-0__drop30", "hairpin-7__drop30", "circle-5__shift"]
assert len(SPOT_IDS) == len(set(SPOT_IDS)) == 24
