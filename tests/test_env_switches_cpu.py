"""The environment switches the sources read are the ones INTEGRATION.md names, and retired ones are gone.

Read = the string argument of getenv("...") or of the walk stage's env_int / env_is_one helpers in faucet_amd/csrc, faucet_amd/host and
integration/*.cpp.  Named = every FGPU_... / FAUCET_... word of INTEGRATION.md from "## Environment switches" to the end of the file, less
the names that are no variables: flag and error constants, the names a measurement BUILD takes, and FGPU_LONG_PAIRS_FILTER (a flag value)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"(?:FGPU|FAUCET)_[A-Z0-9_]+"
NOT_VARIABLES = {"FGPU_EXTRA_CXXFLAGS", "FGPU_KO_TRACE", "FGPU_KO_WAIT_S", "FGPU_LONG_PAIRS_FILTER"}
RETIRED = ["FGPU_WALK_HEAVY", "FGPU_DEBUG_WALK", "FGPU_PREPARED_REFRESH", "FGPU_OVW_SERIAL", "FGPU_SERIAL_CLEAN", "FGPU_NO_WHOLE_BATCH", "FGPU_KO_TICKET",
           "FGPU_WBITS_LOG2", "FGPU_JFILTER_LOG2", "FGPU_DELTA_FILTER_MULT", "FGPU_FLAGS_SM_SLOTS", "FGPU_KO_TIMING", "FGPU_KO_TIMING_PRINT", "FGPU_KO_ONE_XCD",
           "k_walk_par", "WALK_PROBE", "WALK_COMMIT"]
SOURCE_SUFFIXES = (".hip", ".h", ".cpp", ".c", ".py", ".sh")


def _text(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _read_from_the_environment():
    files = glob.glob(os.path.join(ROOT, "faucet_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "faucet_amd", "host", "*")) + \
        glob.glob(os.path.join(ROOT, "integration", "*.cpp"))
    names = set()
    for path in files:
        names.update(re.findall(r'\b(?:getenv|env_int|env_is_one)\(\s*"(' + NAME + r')"', _text(path)))
    return names


def _named_in_the_document():
    doc = _text(os.path.join(ROOT, "INTEGRATION.md"))
    section = doc[doc.index("## Environment switches"):]
    names = set(re.findall(r"\b" + NAME + r"\b", section))
    return {n for n in names if not n.startswith(("FGPU_FLAG_", "FGPU_ERR_")) and n not in NOT_VARIABLES}


def test_the_document_names_exactly_the_switches_the_sources_read():
    read, named = _read_from_the_environment(), _named_in_the_document()
    assert len(read) > 40                      # (the search itself still finds them)
    assert sorted(read - named) == [], "read from the environment, not named in INTEGRATION.md"
    assert sorted(named - read) == [], "named in INTEGRATION.md, read nowhere"


def test_retired_switches_are_named_nowhere_in_the_sources():
    me = os.path.abspath(__file__)
    files = [os.path.join(ROOT, "bench.py")]
    for top in ("faucet_amd", "scripts", "tests"):
        for d, _, fs in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(d, f) for f in fs if f.endswith(SOURCE_SUFFIXES)]
    retired = re.compile(r"(?<![A-Za-z0-9_])(?:" + "|".join(RETIRED) + r")(?![A-Za-z0-9_])")
    found = []
    for path in files:
        if os.path.abspath(path) == me:
            continue
        found += [(os.path.relpath(path, ROOT), n) for n in sorted(set(retired.findall(_text(path))))]
    assert found == []


# Switches no test sets, each with the reason.  Every other switch the sources read is set (or at least named) by some tests/test_*.py or by
# tests/switch_child.py: "results never depend on them" is checked where a test can set them (tests/test_gpu_env_switches.py for most).
NOT_SET_BY_ANY_TEST = {
    "FAUCET_TRANSPORT": "the RCCL transport between ranks that share one device cannot run on a one-GPU box; fgpu_group_selftest covers it at world size 1",
}


def _named_by_the_tests():
    me = os.path.abspath(__file__)
    files = [p for p in glob.glob(os.path.join(ROOT, "tests", "test_*.py")) if os.path.abspath(p) != me] + [os.path.join(ROOT, "tests", "switch_child.py")]
    names = set()
    for path in files:
        names.update(re.findall(r"\b" + NAME + r"\b", _text(path)))
    return names


def test_every_switch_is_set_by_a_test_or_listed_with_a_reason():
    read, named = _read_from_the_environment(), _named_by_the_tests()
    assert len(named) > 40                     # (the search itself still finds them)
    assert all(reason.strip() for reason in NOT_SET_BY_ANY_TEST.values())
    assert sorted(read - named - set(NOT_SET_BY_ANY_TEST)) == [], "read from the environment, set by no test and not listed in NOT_SET_BY_ANY_TEST"
    assert sorted(set(NOT_SET_BY_ANY_TEST) & named) == [], "listed in NOT_SET_BY_ANY_TEST, but a test names it: the table is stale"
    assert sorted(set(NOT_SET_BY_ANY_TEST) - read) == [], "listed in NOT_SET_BY_ANY_TEST, read nowhere"
