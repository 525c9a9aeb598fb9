"""Seeded maps for ContigGraph::removeChimerasAndClean beside the goldens: ids of tests/stage3_fuzz_cases.py (the reads, the reference's own map of
them and its answers -- oracle/_ref/chimera_driver's among them, S.chimera_answers -- are made on the spot where oracle/_ref is built; nothing but
the ids is stored).

The 28 goldens reach every outcome of the step but one: on none of them does validateNoneCollapsible, run behind the step, erase a node.  The
seeded maps do -- VALIDATION_IDS: the reference's own count line says so on each ("removed N collapsible nodes", N > 0: long tandem repeats,
hairpins and circles at extreme coverage, where one cut leaves a node with a single path out that the loop has already passed) -- and
SPOT_IDS are the 24 maps tests/test_dechimera_plan_cpu.py asks the compiled reference about on the spot: every family, thinned variants, maps the
step leaves alone, and the VALIDATION_IDS.  On each of them the restatement, fgpu_chimera_plan and the live-graph path of the device
(CleanGraph::set_cov on the detipped graph, as a CPU program) have to write the driver's two files; LONGEST_LIST_ID is the one whose graph holds
the longest piece list.

GPU_IDS: the ids tests/test_gpu_stage3_fuzz.py holds fgpu_stage3_cov_calls and fgpu_stage3_dechimera to the driver on -- the GPU subset of
tests/golden/stage3_fuzz_ids.json and the SPOT_IDS, 36 maps, the six VALIDATION_IDS among them."""
from tests.stage3_fuzz_cases import listed

VALIDATION_IDS = ["tandem-9", "hairpin-4", "circle-0", "circle-6", "circle-7", "circle-9__mrl10"]
SPOT_IDS = VALIDATION_IDS + ["rand-100", "rand-101", "rand-104", "rand-108", "rand-113", "tandem-0", "tandem-2", "runs-1", "runs-6", "hairpin-7", "hairpin-9",
                             "circle-1", "circle-4", "rand-100__drop30", "rand-108__mrl10", "tandem-0__drop30", "hairpin-7__drop30", "circle-5__shift"]
assert len(SPOT_IDS) == len(set(SPOT_IDS)) == 24
LONGEST_LIST_ID = "hairpin-7"
GPU_IDS = list(dict.fromkeys(listed()["gpu_ids"] + SPOT_IDS))
assert len(GPU_IDS) == 36 or not listed()["gpu_ids"]         # (no list: only while tests/golden/make_stage3_fuzz_list.py is making it)
