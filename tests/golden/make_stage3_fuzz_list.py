#!/usr/bin/env python3
"""The list of Stage-3 fuzz ids (tests/golden/stage3_fuzz_ids.json) for tests/test_stage3_fuzz_cpu.py and tests/test_gpu_stage3_fuzz.py:
    make -C oracle ref && python tests/golden/make_stage3_fuzz_list.py
Every candidate id of tests/stage3_fuzz_cases.py -- random_run seeds 100-115, ten seeds of each low-complexity family, and the three variant
kinds on a subset of both -- goes through `faucet_ref` and both drivers with the time limit.  "ids": the candidates on which all three return, in
candidate order; "rejected": the others with the reason (exit code or no return), the way raw_contigs_summary.json lists its not_returned;
"reached": per class of tests/test_stage3_fuzz_cpu.py the ids that reach it; "gpu_ids": a subset for the GPU tests, picked greedily so that it
holds every family, every k, both cleaning settings, every variant kind and every class the list reaches, then filled in candidate order.
No input is bent towards a class: the script fails if a required class is not reached, and says which optional one is not."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import stage3_fuzz_cases as S  # noqa: E402

GPU_SUBSET = 24
RAND = range(100, 116)
LOW = range(10)
VARIED = {"rand": (100, 103, 108), "tandem": (0, 3, 5), "runs": (1, 4), "hairpin": (2, 7), "circle": (6, 9)}      # kind by position, in turn
# the reference seldom returns on a map whose distances were moved (its asserts, its endless loops): more candidates of that kind
SHIFTED = ("rand-102", "rand-105", "rand-109", "tandem-1", "tandem-6", "hairpin-0", "hairpin-3", "circle-4", "circle-5")


def candidates():
    ids = ["rand-%d" % s for s in RAND] + ["%s-%d" % (f, s) for f in S.FAMILIES[1:] for s in LOW]
    n = 0
    for family, seeds in VARIED.items():
        for s in seeds:
            ids.append("%s-%d__%s" % (family, s, S.KINDS[n % len(S.KINDS)]))
            n += 1
    return ids + [i + "__shift" for i in SHIFTED]


def main():
    from tests import test_stage3_fuzz_cpu as T
    assert S.binaries_built(), "make -C oracle ref first"
    ids, rejected, features = [], {}, {}
    for i in candidates():
        try:
            a = T.account_of(i)
        except S.NotReturned as e:
            rejected[i] = str(e)
            print(i, "rejected:", e)
            continue
        family, _, kind = S.split(i)
        args = S.case_of(i)[1]
        ids.append(i)
        features[i] = {"family:" + family, "k:%d" % a.map.k, "cleaning:%d" % ("--no_cleaning" not in args), "kind:%s" % kind,
                       "paired:%d" % ("--paired_ends" in args)} | set(T.classes_of(a))
        print(i, "k", a.map.k, "junctions", len(a.map.lines), sorted(f for f in features[i] if ":" not in f))
    reached = {cl: [i for i in ids if cl in features[i]] for cl in T.CLASSES + T.OPTIONAL}
    missing = [cl for cl in T.CLASSES if not reached[cl]]
    assert not missing, f"the list does not reach: {missing}"
    print("not reached (optional):", [cl for cl in T.OPTIONAL if not reached[cl]])
    # ---- the GPU tests' subset: greedy cover of every feature, rarest first, then filled in candidate order
    want = set().union(*features.values()) - set(T.OPTIONAL)
    gpu = []
    while want:
        rarest = min(sorted(want), key=lambda f: sum(f in features[i] for i in ids))
        best = max((i for i in ids if rarest in features[i]), key=lambda i: len(features[i] & want))
        gpu.append(best)
        want -= features[best]
    kinds = [i for i in ids if S.split(i)[2] and i not in gpu]
    while sum(1 for i in gpu if S.split(i)[2]) < 4:
        gpu.append(kinds.pop(0))
    rest = {f: [i for i in ids if S.split(i)[0] == f and i not in gpu] for f in S.FAMILIES}
    while len(gpu) < GPU_SUBSET and any(rest.values()):                       # the families in turn, the low-complexity ones first
        for f in S.FAMILIES[1:] + S.FAMILIES[:1]:
            if rest[f] and len(gpu) < GPU_SUBSET:
                gpu.append(rest[f].pop(0))
    gpu = [i for i in ids if i in gpu]
    with open(S.LIST, "w") as f:
        json.dump({"ids": ids, "gpu_ids": gpu, "rejected": rejected, "reached": reached}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(ids), "ids,", len(gpu), "for the GPU tests,", len(rejected), "rejected")


if __name__ == "__main__":
    main()
