"""CPU-only checks of pass 0's kept reads: the library exports the four entry points with the prototypes the ctypes mirror binds, the packed
block's description has not changed, and the Python mirror has its four methods.  (That the command line linked against the tests' stand-in
-- which has none of the four -- still refuses a pipe is tests/test_estimate_cpu.py::test_estimate_needs_a_regular_load_file.)"""
import ctypes as C
import os
import re

from faucet_amd import _lib as L
from faucet_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "fgpu_estimate_keep": "fgpu_ctx* ctx, uint64_t budget_bytes",
    "fgpu_estimate_keep_state": "fgpu_ctx* ctx, int* keeping, uint64_t* n_blocks, uint64_t* bytes",
    "fgpu_estimate_take_kept": "fgpu_ctx* ctx, fgpu_packed* out, uint64_t cap, uint64_t* n_out",
    "fgpu_load_batch_packed": "fgpu_ctx* ctx, const fgpu_packed* b",
}
CTYPES_OF = {"fgpu_ctx*": C.c_void_p, "uint64_t": C.c_uint64, "int*": C.POINTER(C.c_int), "uint64_t*": C.POINTER(C.c_uint64),
             "fgpu_packed*": C.POINTER(L.Packed), "const fgpu_packed*": C.POINTER(L.Packed)}


def test_the_library_exports_the_four_entry_points_as_the_mirror_binds_them():
    hdr = open(os.path.join(ROOT, "include", "faucet_gpu.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, params in ENTRY_POINTS.items():
        assert hasattr(lib, name), name
        m = re.search(r"^int " + name + r"\(([^)]*)\);", hdr, re.M)
        assert m and m.group(1) == params, name
        want = [CTYPES_OF[p.rsplit(" ", 1)[0]] for p in params.split(", ")]
        assert L.SIGNATURES[name] == (C.c_int, want), name
    assert re.search(r"#define FGPU_ABI_VERSION 3\b", hdr)
    L.load()


def test_the_packed_description_is_unchanged():
    assert C.sizeof(L.Packed) == 32
    assert [(n, t) for n, t in L.Packed._fields_] == [("block_dev", C.c_void_p), ("nbytes", C.c_uint64), ("T", C.c_uint64), ("n_reads", C.c_uint64)]


def test_the_context_mirrors_them():
    for name in ("estimate_keep", "estimate_keep_state", "estimate_take_kept", "load_batch_packed"):
        assert callable(getattr(api.Context, name))
