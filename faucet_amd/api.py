"""Host-side mirror of the reference interface for the hot path, on top of the C ABI.

Names follow the reference so that the parity tests read like its own:

    Bloom.create_bloom_filter_optimal / create_bloom_filter_2_hash     utils/Bloom.cpp:206-247
    load_two_filters(bloo1, bloo2, reads)                               utils/Bloom.cpp:267-350
    ReadScanner(...).scanReads(reads) / printScanSummary fields         src/ReadScanner.cpp:19-27,284-359
    JunctionMap.writeToFile                                             utils/JunctionMap.cpp:579-596

All compute runs in libfaucet_gpu.so on the MI355X; nothing here computes k-mers, hashes or junctions on the
host, and nothing falls back to a CPU path: without the library or without a gfx950 device the calls raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


class FaucetGpuError(RuntimeError):
    pass


def _check(rc, ctx=None):
    if rc != L.OK:
        msg = L.load().fgpu_last_error(ctx).decode(errors="replace") if ctx is not None else L.load().fgpu_last_error(None).decode()
        raise FaucetGpuError(f"libfaucet_gpu error {rc}: {msg}")


# ---- sizing (src/Faucet.cpp:197-219) --------------------------------------------------------------
def solve_p1(estimated_kmers: int, singletons: int, fp: float = 0.04) -> float:
    it = C.c_int32(0)
    p1 = L.load().fgpu_solve_p1(estimated_kmers, singletons, C.c_float(fp), C.byref(it))
    if p1 < 0:
        raise ValueError("p1 solver: root not bracketed (singletons must be > 0 and < estimated_kmers)")
    return p1


def size_optimal(estimated: int, fp: float):
    b, t, h = C.c_int32(), C.c_uint64(), C.c_int32()
    L.load().fgpu_size_optimal(estimated, C.c_float(fp), C.byref(b), C.byref(t), C.byref(h))
    return b.value, t.value, h.value


def size_two_hash(estimated: int, fp: float):
    b, t, h = C.c_int32(), C.c_uint64(), C.c_int32()
    L.load().fgpu_size_two_hash(estimated, C.c_float(fp), C.byref(b), C.byref(t), C.byref(h))
    return b.value, t.value, h.value


def estimate_solve(empty, once, r_bits: int):
    """(level, F0, f1) from the counts of a sketch of 2^r_bits cells per level (fgpu_estimate_solve: host arithmetic, no device): empty[l] cells of
    level l never hit, once[l] hit exactly once.  ValueError for r_bits outside 8..34 or counts no sketch gives; FaucetGpuError when even the
    thinnest level is too full (raise r_bits)."""
    e = L.Estimate()
    e.empty[:] = [int(x) for x in empty]
    e.once[:] = [int(x) for x in once]
    e.r_bits = int(r_bits)
    rc = L.load().fgpu_estimate_solve(C.byref(e))
    if rc == L.ERR_CAPACITY:
        raise FaucetGpuError(f"libfaucet_gpu error {rc}: the sketch is too full even at its thinnest level: raise r_bits")
    if rc != L.OK:
        raise ValueError("estimate_solve: r_bits must be in 8..34 and empty[l] + once[l] at most 2^r_bits")
    return int(e.level), float(e.f0), float(e.f1)


def load_filter_shape(estimated_kmers: int, singletons: int, fp: float = 0.04):
    """(tai, n_hash) of bloo1/bloo2 as getBloomFilterFromReads sizes them (src/Faucet.cpp:204-219)."""
    p1 = solve_p1(estimated_kmers, singletons, fp)
    _, tai, nh = size_optimal(estimated_kmers, np.float32(p1))
    return tai, nh


# ---- read batches -----------------------------------------------------------------------------------
class ReadBatch:
    """Sequence lines in file order.  Host numpy arrays or device pointers (e.g. torch tensors' data_ptr())."""

    def __init__(self, bases, offsets, n_reads=None, on_device=False, keepalive=None, starts=None, n_positions=None):
        self.on_device = bool(on_device)
        self.n_positions = n_positions          # bases + one separator per read, when the caller knows it (device batches)
        self._keep = (bases, offsets, keepalive)
        self.starts_ptr = int(starts) if starts else None      # device batches whose reads lie inside raw text
        if on_device:
            self.bases_ptr, self.offsets_ptr = int(bases), int(offsets)
            self.n_reads = int(n_reads)
        else:
            self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
            self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            self.bases_ptr = self.bases.ctypes.data
            self.offsets_ptr = self.offsets.ctypes.data
            self.n_reads = len(self.offsets) - 1
            self.n_positions = int(self.offsets[-1] - self.offsets[0]) + self.n_reads

    @classmethod
    def from_lines(cls, lines):
        offs = np.zeros(len(lines) + 1, dtype=np.uint64)
        if lines:
            offs[1:] = np.cumsum([len(x) for x in lines], dtype=np.uint64)
        data = b"".join(lines)
        bases = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, np.uint8)
        return cls(bases, offs)

    @classmethod
    def from_matrix(cls, mat: np.ndarray):
        n, ln = mat.shape
        return cls(np.ascontiguousarray(mat).reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(ln))

    def c_struct(self):
        # device batches: the total the caller knows (n_positions = bases + one separator per read) spares the library a read-back of two
        # offsets, i.e. a wait for everything it has queued, per call
        total = self.n_positions - self.n_reads if (self.on_device and self.n_positions is not None) else 0
        return L.Reads(self.bases_ptr, self.offsets_ptr, self.n_reads, int(self.on_device), total if 0 < total < 1 << 32 else 0, self.starts_ptr)


STOP_DTYPE = np.dtype([("ext", "<u8"), ("read", "<u4"), ("info", "<u4")])
JUNC_DTYPE = np.dtype([("cov", np.uint8, 4), ("dist", np.uint8, 5), ("linked", np.uint8, 5)])
NEIGHBOR_DTYPE = np.dtype([("kmer", "<u8"), ("dist", "<i4"), ("len", "<i4"), ("node", "i1"), ("rindex", "i1"), ("abort", "i1"), ("reserved", "i1"),
                           ("reserved2", "<i4")])   # fgpu_neighbor
CONTIG_DTYPE = np.dtype([("end_kmer", "<u8"), ("text_word", "<u8"), ("seg_first", "<u8"), ("cov_first", "<u8"), ("len", "<u4"), ("n_seg", "<u4"),
                         ("n_cov", "<u4"), ("ind1", "i1"), ("ind2", "i1"), ("end_node", "i1"), ("status", "i1")])   # fgpu_contig

BUILD_DTYPE = np.dtype([("start_kmer", "<u8"), ("far_kmer", "<u8"), ("time", "<u4"), ("phase", "u1"), ("far_is_junction", "u1"), ("far_is_start", "u1"),
                        ("reserved", "u1")])   # fgpu_build_call
BUILD_BRANCHING, BUILD_LINEAR_FORWARD, BUILD_LINEAR_BACKWARD = range(3)
FASTA_SEQ_DTYPE = np.dtype([("text_word", "<u8", (2,)), ("len", "<u4", (2,)), ("flip", "u1", (2,)), ("pieces", "u1"), ("reserved", "u1"),
                            ("number", "<u4")])   # fgpu_fasta_seq
JOIN_PIECE_DTYPE = np.dtype([("call", "<u4"), ("flip", "<u4")])   # fgpu_join_piece
TIPS_NODE_DTYPE = np.dtype([("key", "<u8"), ("cov", np.uint8, 4), ("slot", "<i4", (5,))])   # fgpu_tips_node
TIPS_CONTIG_DTYPE = np.dtype([("node1", "<u8"), ("node2", "<u8"), ("len", "<u4"), ("has1", "u1"), ("has2", "u1"), ("ind1", "u1"), ("ind2", "u1"),
                              ("isolated", "u1"), ("reserved", "u1", (7,))])   # fgpu_tips_contig
JOINED_DTYPE = np.dtype([("text_word", "<u8"), ("dist_first", "<u8"), ("cov_first", "<u8"), ("cov_sum", "<u8"), ("len", "<u4"), ("n_dist", "<u4"),
                         ("n_cov", "<u4"), ("reserved", "<u4")])   # fgpu_joined
COV_SUMMARY_DTYPE = np.dtype([("sum", "<u8"), ("n", "<u4"), ("first", "u1"), ("last", "u1"), ("reserved", "u1", (2,))])   # fgpu_cov_summary (csrc/cov_summary.h)
FASTG_REC_DTYPE = np.dtype([("tig", "<u8"), ("text_word", "<u8"), ("cov_sum", "<u8"), ("len", "<u4"), ("cov_n", "<u4")])   # fgpu_fastg_rec
FASTG_PRIMED, FASTG_TILE = L.FASTG_PRIMED, L.FASTG_TILE   # a primed neighbour entry; bytes of output per workgroup of the text kernel


class _PinnedMemory:
    """The owner of one fgpu_host_alloc block: the ONLY place that frees it, and only when the last reference is gone -- the HostBuffer
    that made it, or any numpy view handed out over it (every view's base chain ends in a ctypes array that holds this object)."""

    def __init__(self, lib, nbytes):
        self.lib = lib
        self.ptr = lib.fgpu_host_alloc(nbytes)
        if not self.ptr:
            raise FaucetGpuError("fgpu_host_alloc failed")

    def __del__(self):
        ptr, self.ptr = getattr(self, "ptr", None), None
        if ptr:
            self.lib.fgpu_host_free(ptr)


class HostBuffer:
    """Page-locked host memory (fgpu_host_alloc) seen as numpy arrays: device-to-host copies into it run at link speed and asynchronously.
    Views keep the memory alive (a view that outlived its buffer pointed into hipHostFree'd memory): free() and __del__ only
    drop THIS object's reference, the block goes back when the last view is gone too."""

    def __init__(self, nbytes: int):
        self.lib = L.load()
        self.nbytes = int(nbytes)
        self._mem = _PinnedMemory(self.lib, max(self.nbytes, 1))
        self.ptr = self._mem.ptr
        self._raw = (C.c_uint8 * max(self.nbytes, 1)).from_address(self.ptr)
        self._raw._owner = self._mem          # numpy view -> .base = this ctypes array -> the block's owner

    def view(self, dtype=np.uint8, count=None) -> np.ndarray:
        if self._raw is None:
            raise FaucetGpuError("HostBuffer.view() after free()")
        return np.frombuffer(self._raw, dtype=dtype, count=-1 if count is None else count)

    def free(self):
        """give this object's reference up; the memory itself is released once no view of it is left"""
        self._raw = self._mem = self.ptr = None

    def __del__(self):
        self.free()


class Context:
    """One fgpu_ctx: one MI355X, one pair of load filters, one junction map."""

    def __init__(self, k, tai, n_hash, j=1, max_spacer_dist=100, device=0, profile=False, junction_capacity=0,
                 max_batch_bases=0, stream=None, walk_window_span=0, eager_flags=False, keep_resident=True, record_stops=False, mercy=False,
                 key_order_from_start=False):
        self.lib = L.load()
        flags = ((L.FLAG_PROFILE if profile else 0) | (L.FLAG_EAGER_FLAGS if eager_flags else 0)
                 | (0 if keep_resident else L.FLAG_NO_RESIDENT) | (L.FLAG_RECORD_STOPS if record_stops else 0)
                 | (L.FLAG_MERCY if mercy else 0) | (L.FLAG_KEY_ORDER_FROM_START if key_order_from_start else 0))
        p = L.Params(k, j, max_spacer_dist, n_hash, tai, device, flags, junction_capacity,
                     max_batch_bases, stream, walk_window_span)
        h = C.c_void_p()
        _check(self.lib.fgpu_create(C.byref(p), C.byref(h)))
        self.h = h
        self.k, self.tai, self.n_hash, self.j = k, tai, n_hash, j
        self.mercy = bool(mercy)
        self.stream = int(stream) if stream else None    # the caller's stream the library runs on (None: a stream of its own)
        self.device = int(device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.fgpu_destroy(self.h)
            self.h = None
        for b in getattr(self, "_pinned", {}).values():
            b.free()
        self._pinned = {}

    def __del__(self):
        self.close()

    def _c(self, rc):
        _check(rc, self.h)

    # pass 0: -estimated_kmers (F0) and -singletons (f1) from a sketch of the reads (faucet_gpu.h, fgpu_estimate_*)
    def estimate_begin(self, r_bits: int = 0):
        """a pass of its own over the reads: 2^r_bits cells per level, 2^r_bits bytes of device memory until estimate_end (0 = the default, 30)"""
        self._c(self.lib.fgpu_estimate_begin(self.h, int(r_bits)))

    def estimate_batch(self, batch: ReadBatch):
        s = batch.c_struct()
        self._c(self.lib.fgpu_estimate_batch(self.h, C.byref(s)))

    def estimate_end(self) -> dict:
        """{"empty": [4], "once": [4], "kmers", "r_bits", "level", "f0", "f1"}; the pass is over and its memory free whatever happens.  A sketch
        too full to solve raises (raise r_bits) with the counts left in self.last_estimate."""
        e = L.Estimate()
        rc = self.lib.fgpu_estimate_end(self.h, C.byref(e))
        self.last_estimate = e.as_dict() if rc in (L.OK, L.ERR_CAPACITY) else None
        self._c(rc)
        return self.last_estimate

    def estimate_planes_devptr(self):
        """(device pointer, bytes) of the open pass' planes: 2^r_bits bytes, level l in the l-th quarter, 16 cells per 32-bit word"""
        p, n = C.c_void_p(), C.c_uint64()
        self._c(self.lib.fgpu_estimate_planes(self.h, C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def estimate_merge(self, peer_dev_ptr, first_byte: int, nbytes: int):
        """bytes [first_byte, first_byte + nbytes) of another sketch with the same r_bits, held at peer_dev_ptr on this device, merged into the same
        bytes of this context's planes (saturating addition of the cells; whole 16-byte granules), on the context's stream"""
        self._c(self.lib.fgpu_estimate_merge(self.h, peer_dev_ptr, int(first_byte), int(nbytes)))

    def estimate_download(self) -> np.ndarray:
        """the open pass' planes as they stand behind everything queued (uint32 words)"""
        _, n = self.estimate_planes_devptr()
        out = np.empty(n // 4, np.uint32)
        self._c(self.lib.fgpu_estimate_download(self.h, out.ctypes.data, n))
        return out

    def estimate_kmers(self) -> int:
        """the occurrences the open pass has sketched so far on this context"""
        n = C.c_uint64()
        self._c(self.lib.fgpu_estimate_kmers(self.h, C.byref(n)))
        return int(n.value)

    # ... that keeps what it packs: one reading of the stream serves pass 0 and pass 1 (faucet_gpu.h, fgpu_estimate_keep)
    def estimate_keep(self, budget: int):
        """between estimate_begin and the first batch: every non-empty batch is packed into a block of its own and held, charged to `budget`
        bytes at 4 bits per stream position; a batch that does not fit ends the keeping, never the pass"""
        self._c(self.lib.fgpu_estimate_keep(self.h, int(budget)))

    def estimate_keep_state(self):
        """(is every non-empty batch so far held?, blocks held, bytes they are charged); does not wait for the device"""
        keeping, n, b = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        self._c(self.lib.fgpu_estimate_keep_state(self.h, C.byref(keeping), C.byref(n), C.byref(b)))
        return bool(keeping.value), int(n.value), int(b.value)

    def estimate_take_kept(self) -> list:
        """after estimate_end: the blocks in batch order (L.Packed).  They are the caller's now: load_batch_packed hands one on to a context,
        fgpu_device_free of any context on the device releases it; they outlive this context"""
        n = C.c_uint64(0)
        self.lib.fgpu_estimate_keep_state(self.h, None, C.byref(n), None)
        out = (L.Packed * max(1, int(n.value)))()
        self._c(self.lib.fgpu_estimate_take_kept(self.h, out, int(n.value), C.byref(n)))
        blocks = []
        for i in range(int(n.value)):      # copies: the array is not kept alive by its elements' users
            pk = L.Packed()
            C.memmove(C.byref(pk), C.byref(out[i]), C.sizeof(L.Packed))
            blocks.append(pk)
        return blocks

    def estimate_keep_reads(self):
        """after estimate_keep, before the first batch: the pass also keeps every batch's read offsets beside its block (charged to the budget)"""
        self._c(self.lib.fgpu_estimate_keep_reads(self.h))

    def estimate_take_kept_reads(self) -> list:
        """after estimate_take_kept: the kept blocks' reads in block order (L.KeptReads); the caller's, like the blocks, until
        load_batch_packed_reads hands them on"""
        n = C.c_uint64(0)
        rc = self.lib.fgpu_estimate_take_kept_reads(self.h, None, 0, C.byref(n))
        if rc == L.OK or not n.value:
            self._c(rc)
            return []
        out = (L.KeptReads * int(n.value))()
        self._c(self.lib.fgpu_estimate_take_kept_reads(self.h, out, int(n.value), C.byref(n)))
        reads = []
        for i in range(int(n.value)):
            kr = L.KeptReads()
            C.memmove(C.byref(kr), C.byref(out[i]), C.sizeof(L.KeptReads))
            reads.append(kr)
        return reads

    # pass 1
    def load_begin(self, keep_carry=False, shard_times=False, shard_planes=False, keep_reads=False):
        """keep_reads: every resident batch also keeps its read offsets, for a scan of the kept batches (scan_batch_kept)"""
        self._c(self.lib.fgpu_load_begin(self.h, (L.LOAD_KEEP_CARRY if keep_carry else 0) | (L.LOAD_SHARD_TIMES if shard_times else 0) |
                                         (L.LOAD_SHARD_PLANES if shard_planes else 0) | (L.LOAD_KEEP_READS if keep_reads else 0)))

    def load_fixup(self, prefix_dev_ptr) -> dict:
        """multi-GPU: re-evaluate what this shard's own pass kept out of bloo2 against the OR of the lower ranks' bloo1"""
        st = L.LoadStats()
        self._c(self.lib.fgpu_load_fixup(self.h, prefix_dev_ptr, C.byref(st)))
        return st.as_dict()

    def load_fixup_state(self):
        """(can fgpu_load_fixup complete the load pass that has just ended?, bytes the context keeps load batches resident in)"""
        ready, budget = C.c_int(0), C.c_uint64(0)
        self._c(self.lib.fgpu_load_fixup_state(self.h, C.byref(ready), C.byref(budget)))
        return bool(ready.value), int(budget.value)

    # pass 1 by filter slices: the whole stream into the bits [bit_lo, bit_hi) (faucet_gpu.h, fgpu_load_slice_*)
    def load_slice_begin(self, bit_lo: int, bit_hi: int):
        self._c(self.lib.fgpu_load_slice_begin(self.h, bit_lo, bit_hi))

    def load_slice_batch(self, batch: ReadBatch):
        s = batch.c_struct()
        self._c(self.lib.fgpu_load_slice_batch(self.h, C.byref(s)))

    def load_slice_plane(self, i: int):
        """(device pointer, bytes) of the fail plane of the i-th non-empty batch: to be ORed across the ranks in place"""
        p, n = C.c_void_p(), C.c_uint64()
        self._c(self.lib.fgpu_load_slice_plane(self.h, i, C.byref(p), C.byref(n)))
        return p.value, n.value

    def load_slice_commit(self):
        self._c(self.lib.fgpu_load_slice_commit(self.h))

    def load_slice_end(self) -> dict:
        st = L.LoadStats()
        self._c(self.lib.fgpu_load_slice_end(self.h, C.byref(st)))
        return st.as_dict()

    def load_slice_state(self):
        """(inside a sliced pass that is not committed yet?, device bytes of the slice state, planes load_slice_plane can hand out)"""
        ready, wb, nb = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        self._c(self.lib.fgpu_load_slice_state(self.h, C.byref(ready), C.byref(wb), C.byref(nb)))
        return bool(ready.value), int(wb.value), int(nb.value)

    # ... under --mercy: batch, exchange of its fail plane, probe, in lockstep; the miss planes are exchanged before the commit
    def load_slice_mercy_begin(self, bit_lo: int, bit_hi: int):
        self._c(self.lib.fgpu_load_slice_mercy_begin(self.h, bit_lo, bit_hi))

    def load_slice_mercy_probe(self):
        """the latest batch, after its fail plane has been ORed across the ranks: its four miss planes, then the batch joins the carry"""
        self._c(self.lib.fgpu_load_slice_mercy_probe(self.h))

    def load_slice_mercy_planes(self, i: int):
        """(device pointer, bytes) of the four miss planes of the i-th non-empty batch, one block: to be ORed across the ranks in place"""
        p, n = C.c_void_p(), C.c_uint64()
        self._c(self.lib.fgpu_load_slice_mercy_planes(self.h, i, C.byref(p), C.byref(n)))
        return p.value, n.value

    def diag_slice_mercy(self):
        """the last mercy pass by slices: [positions this rank probed, high->low tests answered "junction", runs opened, low->high tests
        answered "junction", runs added, k-mers added by runs] -- all but the first the same on every rank"""
        out = (C.c_uint64 * 6)()
        self._c(self.lib.fgpu_diag_slice_mercy(self.h, out))
        return [int(x) for x in out]

    # ... from packed batches: packed once (here or on a peer), moved device to device, loaded from the packed form
    def load_slice_pack(self, batch: ReadBatch) -> "L.Packed":
        """pack the batch into a block of the sliced pass (digest and T in its trailer); to be sent to the peers and loaded by load_slice_batch_packed"""
        s, pk = batch.c_struct(), L.Packed()
        self._c(self.lib.fgpu_load_slice_pack(self.h, C.byref(s), C.byref(pk)))
        return pk

    def load_slice_expect(self, T: int, n_reads: int) -> "L.Packed":
        """an empty block for a batch of T stream positions that is packed elsewhere: the caller fills its nbytes before loading it"""
        pk = L.Packed()
        self._c(self.lib.fgpu_load_slice_expect(self.h, T, n_reads, C.byref(pk)))
        return pk

    def load_slice_batch_packed(self, pk: "L.Packed"):
        """mark + resolve of a packed batch against the slice: what load_slice_batch does behind its packing"""
        self._c(self.lib.fgpu_load_slice_batch_packed(self.h, C.byref(pk)))

    # ... a sliced pass that keeps reads: the offsets of the packed batches travel beside the blocks (faucet_gpu.h)
    def load_slice_keep_reads(self):
        """inside a sliced pass, before its first batch: load_slice_pack also keeps every batch's read offsets beside its block"""
        self._c(self.lib.fgpu_load_slice_keep_reads(self.h))

    def load_slice_packed_reads(self, pk: "L.Packed") -> "L.KeptReads":
        """the read offsets of a block this context packed (device pointer, n_reads, the longest read it packed: known once the pass has ended)"""
        kr = L.KeptReads()
        self._c(self.lib.fgpu_load_slice_packed_reads(self.h, C.byref(pk), C.byref(kr)))
        return kr

    def load_slice_expect_reads(self, pk: "L.Packed") -> "L.KeptReads":
        """an empty (n_reads + 1) x 8-byte allocation beside a block from load_slice_expect: the caller fills it, then load_slice_adopt_reads"""
        kr = L.KeptReads()
        self._c(self.lib.fgpu_load_slice_expect_reads(self.h, C.byref(pk), C.byref(kr)))
        return kr

    def load_slice_adopt_reads(self, pk: "L.Packed", kr: "L.KeptReads"):
        """the filled allocation becomes the resident batch's offsets; checked on the device against the block (reported by the next synchronising call)"""
        self._c(self.lib.fgpu_load_slice_adopt_reads(self.h, C.byref(pk), C.byref(kr)))

    def scan_resident_base(self, first_batch: int):
        """between the passes: batch i of the next scan pairs with the load pass' resident batch first_batch + i"""
        self._c(self.lib.fgpu_scan_resident_base(self.h, first_batch))

    def load_batch(self, batch: ReadBatch):
        s = batch.c_struct()
        self._c(self.lib.fgpu_load_batch(self.h, C.byref(s)))

    def load_batch_packed(self, pk: "L.Packed"):
        """one batch of the plain pass from a packed block (estimate_take_kept): what load_batch does behind its packing; the context adopts the block"""
        self._c(self.lib.fgpu_load_batch_packed(self.h, C.byref(pk)))

    def load_batch_packed_reads(self, pk: "L.Packed", kr: "L.KeptReads"):
        """load_batch_packed in a pass begun with keep_reads, plus the adoption of the block's read offsets (estimate_take_kept_reads)"""
        self._c(self.lib.fgpu_load_batch_packed_reads(self.h, C.byref(pk), C.byref(kr)))

    def presence_batch(self, batch: ReadBatch):
        s = batch.c_struct()
        self._c(self.lib.fgpu_presence_batch(self.h, C.byref(s)))

    def load_end(self) -> dict:
        st = L.LoadStats()
        self._c(self.lib.fgpu_load_end(self.h, C.byref(st)))
        return st.as_dict()

    def bloom_download(self, which=L.BLOO2) -> np.ndarray:
        out = np.empty(self.tai // 8, dtype=np.uint8)
        self._c(self.lib.fgpu_bloom_download(self.h, which, out.ctypes.data, out.nbytes))
        return out

    def bloom_download_begin(self, which, into: HostBuffer) -> np.ndarray:
        """Start the copy of a filter into page-locked memory; it runs beside whatever is submitted next (the scan).  The array
        returned is complete after bloom_download_wait()."""
        if into.nbytes < self.tai // 8:
            raise ValueError("host buffer smaller than the filter")
        self._c(self.lib.fgpu_bloom_download_begin(self.h, which, into.ptr, self.tai // 8))
        return into.view(np.uint8, self.tai // 8)

    def bloom_download_wait(self):
        self._c(self.lib.fgpu_bloom_download_wait(self.h))

    def _pinned_buffer(self, tag, nbytes) -> HostBuffer:
        if not hasattr(self, "_pinned"):
            self._pinned = {}
        b = self._pinned.get(tag)
        if b is None or b.nbytes < nbytes:
            # a tagged buffer is never regrown in place: the old block stays with whoever still holds a view of it (HostBuffer)
            b = self._pinned[tag] = HostBuffer(nbytes + nbytes // 4)
        return b

    def bloom_upload(self, which, data: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        self._c(self.lib.fgpu_bloom_upload(self.h, which, data.ctypes.data, data.nbytes))

    def bloom_weight(self, which=L.BLOO2) -> float:
        w = C.c_float()
        self._c(self.lib.fgpu_bloom_weight(self.h, which, C.byref(w)))
        return w.value

    def bloom_devptr(self, which):
        p, n = C.c_void_p(), C.c_uint64()
        self._c(self.lib.fgpu_bloom_devptr(self.h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bitmap_or(self, dst_ptr, src_ptr, nbytes):
        self._c(self.lib.fgpu_bitmap_or(self.h, dst_ptr, src_ptr, nbytes))

    # pass 2
    def scan_begin(self):
        self._c(self.lib.fgpu_scan_begin(self.h))

    def scan_batch(self, batch: ReadBatch):
        s = batch.c_struct()
        self._c(self.lib.fgpu_scan_batch(self.h, C.byref(s)))

    def scan_kept_state(self) -> dict:
        """after a load pass: did it keep every non-empty batch with its reads (load_begin(keep_reads=True))?  Host state, never waits"""
        c, nb, nr, by = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._c(self.lib.fgpu_scan_kept_state(self.h, C.byref(c), C.byref(nb), C.byref(nr), C.byref(by)))
        return {"complete": bool(c.value), "n_batches": int(nb.value), "n_reads": int(nr.value), "bytes": int(by.value)}

    def scan_batch_kept(self, i: int) -> int:
        """scan_batch of the reads kept batch i was loaded from, without their text; returns the batch's number of reads"""
        n = C.c_uint64(0)
        self._c(self.lib.fgpu_scan_batch_kept(self.h, int(i), C.byref(n)))
        return int(n.value)

    def scan_kept_range(self, lo: int, hi: int, max_read_len: int = 0) -> bool:
        """between the passes: are the kept batches [lo, hi) all resident with their read offsets?  Waits; max_read_len = the pass' longest read over all ranks"""
        c = C.c_int(0)
        self._c(self.lib.fgpu_scan_kept_range(self.h, int(lo), int(hi), int(max_read_len), C.byref(c)))
        return bool(c.value)

    def scan_prepare_kept(self, i: int) -> int:
        """scan_prepare of the reads kept batch i was loaded from, without their text; returns the batch's number of reads"""
        n = C.c_uint64(0)
        self._c(self.lib.fgpu_scan_prepare_kept(self.h, int(i), C.byref(n)))
        return int(n.value)

    def scan_prepare(self, batch: ReadBatch):
        s = batch.c_struct()
        self._c(self.lib.fgpu_scan_prepare(self.h, C.byref(s)))

    def scan_walk_prepared(self):
        self._c(self.lib.fgpu_scan_walk_prepared(self.h))

    def scan_end(self) -> dict:
        st = L.ScanStats()
        self._c(self.lib.fgpu_scan_end(self.h, C.byref(st)))
        return st.as_dict()

    def junctions(self, pinned=False):
        """(keys uint64[n], records[n]) in creation order.  pinned=True: into page-locked buffers owned by this context (the
        copy then runs at link speed); the arrays are valid until the next such call or close()."""
        n = C.c_uint64()
        self._c(self.lib.fgpu_scan_junction_count(self.h, C.byref(n)))
        cap = max(n.value, 1)
        if pinned:
            keys = self._pinned_buffer("jkeys", cap * 8).view(np.uint64, cap)
            recs = self._pinned_buffer("jrecs", cap * JUNC_DTYPE.itemsize).view(JUNC_DTYPE, cap)
        else:
            keys = np.zeros(cap, dtype=np.uint64)
            recs = np.zeros(cap, dtype=JUNC_DTYPE)
        got = C.c_uint64()
        self._c(self.lib.fgpu_scan_download_junctions(self.h, keys.ctypes.data, recs.ctypes.data, len(keys), C.byref(got)))
        self._n_downloaded = int(got.value)
        return keys[: got.value], recs[: got.value]

    def scan_dump_order(self, counts, buckets, n=None) -> np.ndarray:
        """The reference's dump order of the first n junctions of the last junctions() call (default: all of them), computed on the device
        from the caller's rehash schedule: counts[j] nodes are present when the container goes to buckets[j] buckets, first entry
        (0, buckets of the empty container).  order[i] = index in creation order of the i-th junction dumped (faucet_gpu.h,
        fgpu_scan_dump_order)."""
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        buckets = np.ascontiguousarray(buckets, dtype=np.uint64)
        if counts.ndim != 1 or counts.shape != buckets.shape:
            raise ValueError("scan_dump_order: counts and buckets are two lists of the same length")
        n = getattr(self, "_n_downloaded", 0) if n is None else int(n)
        order = np.zeros(max(n, 1), dtype=np.uint32)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        self._c(self.lib.fgpu_scan_dump_order(self.h, counts.ctypes.data_as(u64p), buckets.ctypes.data_as(u64p), len(counts), n,
                                              order.ctypes.data_as(u32p)))
        return order[:n]

    def table_entries(self) -> int:
        n = C.c_uint64()
        self._c(self.lib.fgpu_scan_table_entries(self.h, C.byref(n)))
        return n.value

    def export_table(self, dev_ptr, nbytes) -> int:
        n = C.c_uint64()
        self._c(self.lib.fgpu_scan_export_table(self.h, dev_ptr, nbytes, C.byref(n)))
        return n.value

    def import_hint(self, dev_ptr, n_entries):
        """a preview of the table this shard will be handed (an earlier state of it): lets scan_prepare evaluate lazily"""
        self._c(self.lib.fgpu_scan_import_hint(self.h, dev_ptr, n_entries))

    def import_table(self, dev_ptr, n_entries, carried: dict = None):
        st = None
        if carried is not None:
            st = L.ScanStats(**{k: int(v) for k, v in carried.items()})
        self._c(self.lib.fgpu_scan_import_table(self.h, dev_ptr, n_entries, C.byref(st) if st is not None else None))

    # probes / profiling
    def probe_hash(self, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        n = len(kmers)
        c, a, b = (np.zeros(n, np.uint64) for _ in range(3))
        self._c(self.lib.fgpu_probe_hash(self.h, kmers.ctypes.data, n, c.ctypes.data, a.ctypes.data, b.ctypes.data))
        return c, a, b

    def probe_contains(self, which, canon):
        canon = np.ascontiguousarray(canon, dtype=np.uint64)
        out = np.zeros(len(canon), np.uint8)
        self._c(self.lib.fgpu_probe_contains(self.h, which, canon.ctypes.data, len(canon), out.ctypes.data))
        return out.astype(bool)

    def synchronize(self):
        self._c(self.lib.fgpu_synchronize(self.h))

    def text_reserve(self, max_chunk_bytes: int):
        """the largest chunk text_split will be handed: its buffers are sized for it once instead of growing with the first chunks"""
        self._c(self.lib.fgpu_text_reserve(self.h, int(max_chunk_bytes)))

    def text_split(self, text, fastq: bool, final_chunk: bool, text_on_device: bool = False, nbytes: int = None):
        """Record splitting of raw FASTA/FASTQ text on the device (the reference's getline loops).  Returns (ReadBatch that
        points into the device copy of the text and is valid until the next text_split, bytes consumed).
        text_on_device: `text` is the address of `nbytes` bytes of text in device memory, written in the order of the context's stream (or
        complete); the batch then points into the caller's text, which has to stay as long as the batch is used."""
        out, used = L.Reads(), C.c_uint64(0)
        if text_on_device:
            self._c(self.lib.fgpu_text_split(self.h, int(text), int(nbytes), 1, int(fastq), int(final_chunk), C.byref(out), C.byref(used)))
        else:
            buf = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, np.uint8)
            self._c(self.lib.fgpu_text_split(self.h, buf.ctypes.data, len(text), 0, int(fastq), int(final_chunk), C.byref(out), C.byref(used)))
        rb = ReadBatch(out.bases or 0, out.offsets or 0, n_reads=int(out.n_reads), on_device=True, starts=out.starts)
        return rb, int(used.value)

    def scan_set_eager(self, on: bool):
        self._c(self.lib.fgpu_scan_set_eager(self.h, int(on)))

    def take_stops(self):
        """scanInputRead's lists of the next scanned batch: (batch number, structured array) or None when none is left"""
        n, seq = C.c_uint64(0), C.c_int64(0)
        rc = self.lib.fgpu_scan_take_stops(self.h, None, 0, C.byref(n), C.byref(seq))
        if rc not in (L.OK, L.ERR_CAPACITY) or (rc == L.ERR_CAPACITY and seq.value < 0):     # (no batch: the junction table is full)
            self._c(rc)
        if seq.value < 0:
            return None
        if rc == L.OK:                      # an empty batch fits any buffer and has been consumed
            return int(seq.value), np.zeros(0, dtype=STOP_DTYPE)
        out = np.zeros(max(int(n.value), 1), dtype=STOP_DTYPE)
        self._c(self.lib.fgpu_scan_take_stops(self.h, out.ctypes.data, len(out), C.byref(n), C.byref(seq)))
        return int(seq.value), out[:int(n.value)]

    def _probe_stage3(self, fn, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        out = np.zeros(len(kmers), dtype=np.int8)
        self._c(fn(self.h, kmers.ctypes.data, len(kmers), out.ctypes.data))
        return out

    def probe_jcheck(self, kmers):                   # JChecker::jcheck(kmer_type), batched
        return self._probe_stage3(self.lib.fgpu_probe_jcheck, kmers)

    def probe_valid_extension(self, kmers):          # JunctionMap::getValidJExtension, batched
        return self._probe_stage3(self.lib.fgpu_probe_valid_extension, kmers)

    def probe_bloom_junction(self, kmers):           # JunctionMap::isBloomJunction, batched
        return self._probe_stage3(self.lib.fgpu_probe_bloom_junction, kmers)

    def diag_walk_probe(self):
        """four zeros: the out-of-order walk these counted is retired (the entry point stays for the ABI)"""
        out = (C.c_uint64 * 4)()
        self._c(self.lib.fgpu_diag_walk_probe(self.h, out))
        return [int(v) for v in out]

    def scan_short_pairs(self, tai: int, n_hash: int, lists_to_host: bool = True):
        """keep the short pair filter (scan_forward's addPair rules) on the device from the next scan on; tai = 0 switches it off"""
        self._c(self.lib.fgpu_scan_short_pairs(self.h, int(tai), int(n_hash), 1 if lists_to_host else 0))

    def scan_short_pairs_download(self, tai: int):
        out = np.zeros(tai // 8, dtype=np.uint8)
        self._c(self.lib.fgpu_scan_short_pairs_download(self.h, out.ctypes.data, len(out)))
        return out

    def scan_long_pairs(self, tai: int, n_hash: int, mode: int = 2):
        """keep the long pair filter (scanReads' paired-end loop, src/ReadScanner.cpp:317-343) on the device from the next scan on;
        mode 0 = off, 1 = only the empty / not-empty pair counts (--no_cleaning), 2 = counts and filter (first-set times dense where their
        4 bytes per bit fit, else per batch), 3 = counts and filter, first-set times always per batch (sparse); FGPU_LONG_PAIRS_STATE =
        dense | sparse | auto overrides what mode 2 takes"""
        self._c(self.lib.fgpu_scan_long_pairs(self.h, int(tai), int(n_hash), int(mode)))

    def scan_long_pairs_download(self, tai: int = 0):
        """(filter bytes or None, empty count, not-empty count) after scan_end"""
        out = np.zeros(tai // 8, dtype=np.uint8) if tai else None
        e, ne = C.c_uint64(0), C.c_uint64(0)
        self._c(self.lib.fgpu_scan_long_pairs_download(self.h, out.ctypes.data if tai else None, len(out) if tai else 0, C.byref(e), C.byref(ne)))
        return out, int(e.value), int(ne.value)

    def scan_pairs_devptr(self, which: int):
        """(device pointer, bytes) of a pair filter as it stands while a scan is open: 0 the short one, 1 the long one"""
        p, n = C.c_void_p(), C.c_uint64()
        self._c(self.lib.fgpu_scan_pairs_devptr(self.h, int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    def diag_long_pairs(self):
        out = (C.c_uint64 * 6)()
        self._c(self.lib.fgpu_diag_long_pairs(self.h, out))
        return dict(zip(("items", "paired_by_carry", "inserts", "rounds", "max_rounds", "batches"), (int(v) for v in out)))

    def diag_long_pairs_state(self):
        """the form of the long pair filter's first-set times: form None / "dense" / "sparse", working bytes beyond the bits, the most table
        slots a batch of the last scan had (sparse), the internal-error flag (sparse)"""
        out = (C.c_uint64 * 4)()
        self._c(self.lib.fgpu_diag_long_pairs_state(self.h, out))
        return {"form": (None, "dense", "sparse")[int(out[0])], "working_bytes": int(out[1]), "table_slots_high": int(out[2]), "error": int(out[3])}

    def diag_ovw(self):
        """the optimistic walk of large clusters during the last scan: pieces walked, rounds run, windows settled, windows left to the key-ordered walk"""
        out = (C.c_uint64 * 6)()
        self._c(self.lib.fgpu_diag_ovw(self.h, out))
        return dict(zip(("pieces", "rounds", "windows", "fallback_windows", "kept_piece_rounds", "table_overflow_windows"), (int(v) for v in out)))

    def scan_refresh_prepared(self):
        """the in-map planes of every prepared batch made again against the preview in the table (after a fresher import_hint)"""
        self._c(self.lib.fgpu_scan_refresh_prepared(self.h))

    def diag_prepared_refresh(self):
        out = (C.c_uint64 * 4)()
        self._c(self.lib.fgpu_diag_prepared_refresh(self.h, out))
        return dict(zip(("batches_in_full", "batches_merged", "new_keys", "mismatching_words"), (int(v) for v in out)))

    def diag_sparse_link(self):
        """windows of prepared batches (read shards) whose link pass visited candidate positions only / every position"""
        out = (C.c_uint64 * 2)()
        self._c(self.lib.fgpu_diag_sparse_link(self.h, out))
        return {"windows_sparse": int(out[0]), "windows_in_full": int(out[1])}

    def diag_ovw_tables(self):
        """event tables of the optimistic walk: the most entries a round of the last scan held, and the entries per table as they stand"""
        hw, cap = C.c_uint64(), C.c_uint64()
        self._c(self.lib.fgpu_diag_ovw_tables(self.h, C.byref(hw), C.byref(cap)))
        return {"high_water": int(hw.value), "capacity": int(cap.value)}

    def stage3_set_junctions(self, keys, recs):
        """the junction map Stage 3's walks look into (keys as JunctionMap keys them; records as junctions() returns them)"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        recs = np.ascontiguousarray(recs, dtype=JUNC_DTYPE)
        assert len(keys) == len(recs)
        self._c(self.lib.fgpu_stage3_set_junctions(self.h, keys.ctypes.data, recs.ctypes.data, len(keys)))

    def stage3_find_neighbors(self, start_kmers, indices, max_read_length: int, contigs: bool = False):
        """JunctionMap::findNeighbor for every (start k-mer, extension index) pair, whole walks on the device; returns (NEIGHBOR_DTYPE array,
        number of getValidJExtension evaluations) and, with contigs=True, the list of contig strings (BfSearchResult::contig) as third item"""
        start_kmers = np.ascontiguousarray(start_kmers, dtype=np.uint64)
        indices = np.ascontiguousarray(indices, dtype=np.int8)
        assert len(start_kmers) == len(indices)
        n = len(start_kmers)
        out = np.zeros(n, dtype=NEIGHBOR_DTYPE)
        probes = C.c_uint64(0)
        stride = int(self.lib.fgpu_stage3_contig_words(self.k, int(max_read_length))) if contigs else 0
        text = np.zeros(max(n * stride, 1), dtype=np.uint64)
        self._c(self.lib.fgpu_stage3_find_neighbors(self.h, start_kmers.ctypes.data, indices.ctypes.data, n, int(max_read_length), out.ctypes.data,
                                                    C.byref(probes), text.ctypes.data if contigs else None, stride))
        if not contigs:
            return out, int(probes.value)
        codes = (text.reshape(n, stride)[:, :, None] >> (2 * np.arange(32, dtype=np.uint64))[None, None, :]) & np.uint64(3)
        chars = np.frombuffer(b"ACTG", dtype=np.uint8)[codes.reshape(n, stride * 32).astype(np.int64)]
        return out, int(probes.value), [chars[i, :int(out["len"][i])].tobytes().decode() for i in range(n)]

    def stage3_contigs(self, start_kmers, indices, max_read_length: int, raw: bool = False):
        """JunctionMap::getContig for every (start k-mer, start index) pair, whole chains on the device against the map of
        stage3_set_junctions as it stands.  Returns (CONTIG_DTYPE array, strings, distances, coverages, kills, probes): per chain the contig
        string, the distance and coverage lists as uint8 arrays and kmers_to_destroy as a uint64 array (all empty for a status other than 0),
        and the number of getValidJExtension evaluations of the call.  raw=True: (CONTIG_DTYPE array, text words, segment k-mers, segment
        distances, coverages, probes), the arrays as the library lays them out."""
        start_kmers = np.ascontiguousarray(start_kmers, dtype=np.uint64)
        indices = np.ascontiguousarray(indices, dtype=np.int8)
        assert len(start_kmers) == len(indices)
        n = len(start_kmers)
        out = np.zeros(n, dtype=CONTIG_DTYPE)
        totals = (C.c_uint64 * 3)()
        probes = C.c_uint64(0)
        self._c(self.lib.fgpu_stage3_contigs(self.h, start_kmers.ctypes.data, indices.ctypes.data, n, int(max_read_length), out.ctypes.data, totals, C.byref(probes)))
        text, kmers = np.zeros(totals[0], dtype=np.uint64), np.zeros(totals[1], dtype=np.uint64)
        dist, cov = np.zeros(totals[1], dtype=np.uint8), np.zeros(totals[2], dtype=np.uint8)
        self._c(self.lib.fgpu_stage3_contigs_take(self.h, text.ctypes.data, len(text), kmers.ctypes.data, dist.ctypes.data, len(dist), cov.ctypes.data, len(cov)))
        if raw:
            return out, text, kmers, dist, cov, int(probes.value)
        chars = np.frombuffer(b"ACTG", dtype=np.uint8)[((text[:, None] >> (2 * np.arange(32, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)].reshape(-1)
        strings, dists, covs, kills = [], [], [], []
        for c in out:
            t, s, v, ns = int(c["text_word"]), int(c["seg_first"]), int(c["cov_first"]), int(c["n_seg"])
            strings.append(chars[32 * t:32 * t + int(c["len"])].tobytes().decode())
            dists.append(dist[s:s + ns])
            covs.append(cov[v:v + int(c["n_cov"])])
            kills.append(kmers[s:s + max(ns - 1, 0)])
        return out, strings, dists, covs, kills, int(probes.value)

    def stage3_build(self, max_read_length: int, raw: bool = False, take: bool = True):
        """JunctionMap::buildContigGraph's contig list (utils/JunctionMap.cpp:11-129) in one call: every getContig call of buildBranchingPaths and
        buildLinearRegions that the reference makes, each on the map of stage3_set_junctions as it stands at that moment, in the reference's
        order.  Returns (CONTIG_DTYPE array, BUILD_DTYPE array, strings, distances, coverages, kills, info): one entry per call that is made,
        the lists as stage3_contigs gives them, and info = dict(status, stop_call, calls_possible, rounds, rewalked, rewalked_by_round, probes, table_hits, regrown)
        -- status 0: the build ran to its end; 1 / 3: the call with number stop_call, which is not output, trips an assert / never returns.
        raw=True: (CONTIG_DTYPE array, BUILD_DTYPE array, text words, segment k-mers, segment distances, coverages, info).
        take=False: the results stay on the device (for stage3_raw_contigs, or a later fgpu_stage3_build_take); returns info alone, with the
        four totals under "totals"."""
        totals = (C.c_uint64 * 4)()
        bi = L.BuildInfo()
        self._c(self.lib.fgpu_stage3_build(self.h, int(max_read_length), totals, C.byref(bi)))
        if not take:
            return dict(status=int(bi.status), stop_call=int(bi.stop_call), calls_possible=int(bi.calls_possible), rounds=int(bi.rounds), rewalked=int(bi.rewalked),
                        rewalked_by_round=[int(v) for v in bi.rewalked_by_round[:min(int(bi.rounds), L.BUILD_ROUNDS_KEPT)]], probes=int(bi.probes),
                        table_hits=int(bi.table_hits), regrown=int(bi.regrown), totals=[int(v) for v in totals])
        out, calls = np.zeros(totals[0], dtype=CONTIG_DTYPE), np.zeros(totals[0], dtype=BUILD_DTYPE)
        text, kmers = np.zeros(totals[1], dtype=np.uint64), np.zeros(totals[2], dtype=np.uint64)
        dist, cov = np.zeros(totals[2], dtype=np.uint8), np.zeros(totals[3], dtype=np.uint8)
        self._c(self.lib.fgpu_stage3_build_take(self.h, out.ctypes.data, calls.ctypes.data, len(out), text.ctypes.data, len(text), kmers.ctypes.data,
                                                dist.ctypes.data, len(dist), cov.ctypes.data, len(cov)))
        info = dict(status=int(bi.status), stop_call=int(bi.stop_call), calls_possible=int(bi.calls_possible), rounds=int(bi.rounds), rewalked=int(bi.rewalked),
                    rewalked_by_round=[int(v) for v in bi.rewalked_by_round[:min(int(bi.rounds), L.BUILD_ROUNDS_KEPT)]], probes=int(bi.probes), table_hits=int(bi.table_hits), regrown=int(bi.regrown))
        if raw:
            return out, calls, text, kmers, dist, cov, info
        chars = np.frombuffer(b"ACTG", dtype=np.uint8)[((text[:, None] >> (2 * np.arange(32, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)].reshape(-1)
        strings, dists, covs, kills = [], [], [], []
        for c in out:
            t, s, v, ns = int(c["text_word"]), int(c["seg_first"]), int(c["cov_first"]), int(c["n_seg"])
            strings.append(chars[32 * t:32 * t + int(c["len"])].tobytes().decode())
            dists.append(dist[s:s + ns])
            covs.append(cov[v:v + int(c["n_cov"])])
            kills.append(kmers[s:s + max(ns - 1, 0)])
        return out, calls, strings, dists, covs, kills, info

    def stage3_fasta_take(self, nbytes: int) -> bytes:
        out = np.zeros(max(int(nbytes), 1), dtype=np.uint8)
        self._c(self.lib.fgpu_stage3_fasta_take(self.h, out.ctypes.data, int(nbytes)))
        return out[:int(nbytes)].tobytes()

    def stage3_fasta(self, seqs, text=None) -> bytes:
        """FASTA_SEQ_DTYPE records joined, oriented and printed on the device (fgpu_stage3_fasta): every record ">Contig<number>\n", then the
        one piece or the first piece without its last k bases and the second, as canon_contig leaves it, and "\n".  text: 2-bit words (A 0,
        C 1, T 2, G 3, 32 bases per word, first base lowest) the pieces index; None: the text of the last stage3_build(take=False)."""
        seqs = np.ascontiguousarray(seqs, dtype=FASTA_SEQ_DTYPE)
        if text is not None:
            text = np.ascontiguousarray(text, dtype=np.uint64)
        nbytes = C.c_uint64(0)
        self._c(self.lib.fgpu_stage3_fasta(self.h, seqs.ctypes.data, len(seqs), None if text is None else text.ctypes.data, 0 if text is None else len(text),
                                           C.byref(nbytes)))
        return self.stage3_fasta_take(nbytes.value)

    def stage3_raw_contigs(self, read_length: int):
        """the reference's <prefix>.raw_contigs.fasta (ContigGraph::printContigs on the graph of buildContigGraph, src/Faucet.cpp:314) of the build
        stage3_build(max_read_length, take=False) left on the device: (the file's bytes, info = dict(records, bubble_records, node_contigs,
        isolated_kept, isolated_dropped, nodes)).  The build stays where it is."""
        nbytes = C.c_uint64(0)
        ri = L.RawInfo()
        self._c(self.lib.fgpu_stage3_raw_contigs(self.h, int(read_length), C.byref(nbytes), C.byref(ri)))
        return self.stage3_fasta_take(nbytes.value), ri.as_dict()

    def stage3_join(self, lists, contigs=None, text=None, dist=None, cov=None, raw: bool = False):
        """Contigs that are joins of contigs (fgpu_stage3_join): ContigJuncList::concatenate, applied left to right over every list of
        (contig, flip) pieces -- a flipped piece is read as ContigJuncList::reverse leaves it; consecutive pieces overlap by k bases; the last
        coverage of the left side and the first of the right become their minimum.  contigs=None: the pieces index the calls of the last
        stage3_build(take=False), whose arrays are read where they lie on the device; otherwise a CONTIG_DTYPE array with the text words,
        distances and coverages it indexes (stage3_contigs(raw=True)'s layout).  Returns (JOINED_DTYPE array, strings, distances, coverages,
        average coverages): per list the joined string, the two lists as uint8 arrays, and cov_sum / n_cov as a float64, which is
        ContigJuncList::getAvgCoverage.  raw=True: (JOINED_DTYPE array, text words, distances, coverages), as the library lays them out."""
        lists = [list(pl) for pl in lists]
        first = np.zeros(len(lists) + 1, dtype=np.uint64)
        first[1:] = np.cumsum([len(pl) for pl in lists], dtype=np.uint64)
        pieces = np.zeros(int(first[-1]), dtype=JOIN_PIECE_DTYPE)
        flat = [pc for pl in lists for pc in pl]
        pieces["call"], pieces["flip"] = [c for c, _ in flat], [int(f) for _, f in flat]
        args = [None, 0, None, 0, None, 0, None, 0]
        if contigs is not None:
            contigs = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE)
            text, dist, cov = np.ascontiguousarray(text, dtype=np.uint64), np.ascontiguousarray(dist, dtype=np.uint8), np.ascontiguousarray(cov, dtype=np.uint8)
            args = [x for a in (contigs, text, dist, cov) for x in (a.ctypes.data, len(a))]
        out = np.zeros(len(lists), dtype=JOINED_DTYPE)
        totals = (C.c_uint64 * 3)()
        self._c(self.lib.fgpu_stage3_join(self.h, first.ctypes.data, len(lists), pieces.ctypes.data, len(pieces), *args, out.ctypes.data, totals))
        jtext, jdist, jcov = np.zeros(totals[0], dtype=np.uint64), np.zeros(totals[1], dtype=np.uint8), np.zeros(totals[2], dtype=np.uint8)
        self._c(self.lib.fgpu_stage3_join_take(self.h, jtext.ctypes.data, len(jtext), jdist.ctypes.data, len(jdist), jcov.ctypes.data, len(jcov)))
        if raw:
            return out, jtext, jdist, jcov
        chars = np.frombuffer(b"ACTG", dtype=np.uint8)[((jtext[:, None] >> (2 * np.arange(32, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)].reshape(-1)
        strings = [chars[32 * int(j["text_word"]):32 * int(j["text_word"]) + int(j["len"])].tobytes().decode() for j in out]
        dists = [jdist[int(j["dist_first"]):int(j["dist_first"]) + int(j["n_dist"])] for j in out]
        covs = [jcov[int(j["cov_first"]):int(j["cov_first"]) + int(j["n_cov"])] for j in out]
        return out, strings, dists, covs, out["cov_sum"].astype(np.float64) / out["n_cov"].astype(np.float64)

    def stage3_cov_calls(self, contigs=None, cov=None):
        """What a cleaning step reads of every contig's coverage list (fgpu_stage3_cov_calls): a COV_SUMMARY_DTYPE array, per record the sum,
        the number of entries, the first and the last entry; sum / n as float64 is ContigJuncList::getAvgCoverage.  contigs=None: the calls of the
        last stage3_build(take=False), whose coverages are read where they lie on the device; otherwise a CONTIG_DTYPE array (cov_first and
        n_cov are read) and the coverage bytes it indexes."""
        if contigs is None:
            if cov is not None:
                raise ValueError("coverages without the records that index them")
            totals = (C.c_uint64 * 4)()
            self._c(self.lib.fgpu_stage3_build_totals(self.h, totals))        # (the library's own count: how many records the call writes)
            out = np.zeros(int(totals[0]), dtype=COV_SUMMARY_DTYPE)
            self._c(self.lib.fgpu_stage3_cov_calls(self.h, None, 0, None, 0, out.ctypes.data))
            return out
        contigs = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE)
        cov = np.ascontiguousarray(cov, dtype=np.uint8)
        out = np.zeros(len(contigs), dtype=COV_SUMMARY_DTYPE)
        self._c(self.lib.fgpu_stage3_cov_calls(self.h, contigs.ctypes.data, len(contigs), cov.ctypes.data, len(cov), out.ctypes.data))
        return out

    def stage3_fasta_joined(self, joined, numbers, text=None) -> bytes:
        """JOINED_DTYPE records oriented and printed on the device (fgpu_stage3_fasta_joined): record i is ">Contig<numbers[i]>\n", its len bases
        from word text_word of the text as canon_contig leaves them, and "\n".  text: the joined 2-bit words (stage3_join(raw=True)'s); None: the
        joined text the last fgpu_stage3_join left on the device, read where it lies."""
        joined = np.ascontiguousarray(joined, dtype=JOINED_DTYPE)
        numbers = np.ascontiguousarray(numbers, dtype=np.uint32)
        if len(numbers) != len(joined):
            raise ValueError("one number per record")
        if text is not None:
            text = np.ascontiguousarray(text, dtype=np.uint64)
        nbytes = C.c_uint64(0)
        self._c(self.lib.fgpu_stage3_fasta_joined(self.h, joined.ctypes.data, numbers.ctypes.data, len(joined), None if text is None else text.ctypes.data,
                                                  0 if text is None else len(text), C.byref(nbytes)))
        return self.stage3_fasta_take(nbytes.value)

    def stage3_graph_take(self) -> dict:
        """the graph the last stage3_detip left (fgpu_stage3_graph_take): dict(nodes TIPS_NODE_DTYPE in map order, contigs TIPS_CONTIG_DTYPE,
        lists = per contig its [(call, flip)] over the calls of the build: valid input to stage3_join)"""
        out = L.TipsOut()
        first = np.zeros(1, dtype=np.uint64)
        out.list_first = first.ctypes.data
        rc = self.lib.fgpu_stage3_graph_take(self.h, C.byref(out))          # (no room: how much is needed)
        if rc == 0:                                                          # an empty graph: taken
            return dict(nodes=np.zeros(0, dtype=TIPS_NODE_DTYPE), contigs=np.zeros(0, dtype=TIPS_CONTIG_DTYPE), lists=[])
        if rc != L.ERR_ARG:
            self._c(rc)
        return _tips_graph(out, lambda: self._c(self.lib.fgpu_stage3_graph_take(self.h, C.byref(out))))

    def stage3_detip(self, read_length: int):
        """ContigGraph::deleteTipsAndClean (src/ContigGraph.cpp:168-175) and printContigs behind it, on the build stage3_build(max_read_length,
        take=False) left on the device (fgpu_stage3_detip): (the file's bytes, info = dict(nodes_before, tips, back_tips, collapsed, degenerate,
        validated, changed, print = stage3_raw_contigs' info of this file)).  The build stays where it is; stage3_graph_take() gives the graph
        left.  Join results and a file that were not taken before the call are dropped."""
        nbytes = C.c_uint64(0)
        ti = L.TipsInfo()
        self._c(self.lib.fgpu_stage3_detip(self.h, int(read_length), C.byref(nbytes), C.byref(ti)))
        return self.stage3_fasta_take(nbytes.value), ti.as_dict()

    def stage3_dechimera(self):
        """ContigGraph::removeChimerasAndClean (src/ContigGraph.cpp:177-184) on the live graph the last stage3_detip left, and printContigs behind
        it (fgpu_stage3_dechimera): (the file's bytes, info = dict(nodes_before, removed, cut_near, cut_far, cut_both, collapsed, degenerate,
        collapsed_after_cut, skipped, validated, changed, print)).  The build stays where it is; stage3_graph_take() gives the graph after the
        step.  Join results and a file that were not taken before the call are dropped; a second call without a new stage3_detip is an error."""
        nbytes = C.c_uint64(0)
        ci = L.ChimeraInfo()
        self._c(self.lib.fgpu_stage3_dechimera(self.h, C.byref(nbytes), C.byref(ci)))
        return self.stage3_fasta_take(nbytes.value), ci.as_dict()

    def stage3_fastg(self, recs, neighbours, text=None) -> bytes:
        """FASTG_REC_DTYPE records printed as ContigGraph::printGraph prints contigs (fgpu_stage3_fastg): per record the primed header, its len
        bases from word text_word of the text, the other header, and the reverse complement.  neighbours: per record (primed header's, other
        header's), each a list of at most four (record, primed).  text: joined 2-bit words (stage3_join(raw=True)'s); None: the joined text the
        last fgpu_stage3_join left on the device, read where it lies."""
        recs = np.ascontiguousarray(recs, dtype=FASTG_REC_DTYPE)
        if len(neighbours) != len(recs):
            raise ValueError("two neighbour lists per record")
        flat = [lst for pair in neighbours for lst in pair]
        first = np.zeros(2 * len(recs) + 1, dtype=np.uint64)
        first[1:] = np.cumsum([len(lst) for lst in flat], dtype=np.uint64)
        nbr = np.array([int(r) | (FASTG_PRIMED if p else 0) for lst in flat for r, p in lst], dtype=np.uint32)
        return self.stage3_fastg_csr(recs, first, nbr, text)

    def stage3_fastg_csr(self, recs, first, nbr, text=None) -> bytes:
        """stage3_fastg with the neighbour lists as the library takes them: first (2 n + 1 uint64), nbr (uint32, record | FASTG_PRIMED)"""
        recs = np.ascontiguousarray(recs, dtype=FASTG_REC_DTYPE)
        first, nbr = np.ascontiguousarray(first, dtype=np.uint64), np.ascontiguousarray(nbr, dtype=np.uint32)
        if text is not None:
            text = np.ascontiguousarray(text, dtype=np.uint64)
        nbytes = C.c_uint64(0)
        self._c(self.lib.fgpu_stage3_fastg(self.h, recs.ctypes.data, len(recs), first.ctypes.data, nbr.ctypes.data if len(nbr) else None, len(nbr),
                                           None if text is None else text.ctypes.data, 0 if text is None else len(text), C.byref(nbytes)))
        return self.stage3_fasta_take(nbytes.value)

    def stage3_raw_graph(self, read_length: int):
        """the reference's <prefix>.raw_graph.fastg (ContigGraph::printGraph on the graph of buildContigGraph, src/Faucet.cpp:313) of the build
        stage3_build(max_read_length, take=False) left on the device (fgpu_stage3_raw_graph): (the file's bytes, info = dict(node_records,
        isolated_printed, isolated_listed, nodes)).  The build and a live graph stay as they are.  Join results and a file that were not taken
        before the call are dropped."""
        nbytes = C.c_uint64(0)
        fi = L.FastgInfo()
        self._c(self.lib.fgpu_stage3_raw_graph(self.h, int(read_length), C.byref(nbytes), C.byref(fi)))
        return self.stage3_fasta_take(nbytes.value), fi.as_dict()

    def stage3_graph_fastg(self):
        """ContigGraph::printGraph on the live graph the last stage3_detip or stage3_dechimera left (fgpu_stage3_graph_fastg): (the file's bytes,
        info as stage3_raw_graph's).  The graph is not changed and the call may be repeated.  Join results and a file that were not taken before
        the call are dropped."""
        nbytes = C.c_uint64(0)
        fi = L.FastgInfo()
        self._c(self.lib.fgpu_stage3_graph_fastg(self.h, C.byref(nbytes), C.byref(fi)))
        return self.stage3_fasta_take(nbytes.value), fi.as_dict()

    def kernel_times(self) -> dict:
        arr = (L.KernelTime * 64)()
        n = self.lib.fgpu_kernel_times(self.h, arr, 64)
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(min(n, 64))}

    def profile_enable(self, on: bool):
        """HIP events around every kernel on / off (between passes)"""
        self._c(self.lib.fgpu_profile_enable(self.h, int(on)))

    def kernel_times_reset(self):
        self._c(self.lib.fgpu_kernel_times_reset(self.h))

    def diag_stream_copy(self, nbytes: int, iters: int = 5) -> float:
        """measured streaming-copy rate of this device, GB/s (read + write)"""
        out = C.c_double(0)
        self._c(self.lib.fgpu_diag_stream_copy(self.h, nbytes, iters, C.byref(out)))
        return out.value

    def diag_scan_replays(self) -> int:
        """how often the library has scanned a pass again by itself because the lazy junction-test preview could not be repaired"""
        n = C.c_uint64(0)
        self._c(self.lib.fgpu_diag_scan_replays(self.h, C.byref(n)))
        return int(n.value)

    def diag_late_flags(self) -> dict:
        """after scan_end: late junction tests that came out true at an unregistered k-mer, and how many of them voided the scan"""
        out = (C.c_uint64 * 3)()
        self._c(self.lib.fgpu_diag_late_flags(self.h, out))
        return {"noted": int(out[0]), "conflicts": int(out[1]), "swept": int(out[2])}

    def diag_load_split(self) -> dict:
        """where the last load pass settled its occurrences: routed to bloo2 by the marking kernel itself / left to the resolution"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._c(self.lib.fgpu_diag_load_split(self.h, C.byref(a), C.byref(b)))
        return {"in_mark": int(a.value), "pending": int(b.value)}

    def diag_binned_probes(self, table_bytes: int, n_probes: int, slice_bytes: int = 4 << 20, iters: int = 3) -> dict:
        """direct random bit probes vs probes binned by filter slice (NS1's query-side blocking), same addresses; rates in probes/s"""
        v = [C.c_double(0) for _ in range(4)]
        self._c(self.lib.fgpu_diag_binned_probes(self.h, table_bytes, n_probes, slice_bytes, iters, *[C.byref(x) for x in v]))
        return dict(zip(("direct_per_s", "binned_per_s", "bin_ms", "probe_ms"), [float(x.value) for x in v]))

    def diag_binned_chain(self, table_bytes: int, n_items: int, slice_bytes: int = 4 << 20, n_hash: int = 3, fill_byte: int = 0x29, iters: int = 3) -> dict:
        """Bloom::contains chains directly vs first level binned by filter slice + survivors handed back (NS1, whole chain); ms per pass"""
        v = [C.c_double(0) for _ in range(5)]
        eq = C.c_int(0)
        self._c(self.lib.fgpu_diag_binned_chain(self.h, table_bytes, n_items, slice_bytes, n_hash, fill_byte, iters, *[C.byref(x) for x in v], C.byref(eq)))
        d = dict(zip(("direct_ms", "bin_ms", "first_ms", "rest_ms", "survivors_share"), [float(x.value) for x in v]))
        d["equal"] = bool(eq.value)
        return d

    def diag_ko_trace(self) -> np.ndarray:
        """(n, 4) uint64: piece number, start, end, waited | lk positions << 48 of every piece the key-ordered walk walked (-DFGPU_KO_TRACE builds)"""
        out = np.zeros((1 << 21, 4), dtype=np.uint64)
        n = C.c_uint64(0)
        self._c(self.lib.fgpu_diag_ko_trace(self.h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def diag_ko_stamps(self) -> np.ndarray:
        """(pieces, 1024) uint64: per-step time stamps of one key-ordered piece in 16 (-DFGPU_KO_TRACE builds); word 0 = piece << 16 | stamps"""
        out = np.zeros((4096, 1024), dtype=np.uint64)
        n = C.c_uint64(0)
        self._c(self.lib.fgpu_diag_ko_stamps(self.h, out.ctypes.data, out.size, C.byref(n)))
        return out[: n.value].copy()

    def diag_device_attr(self) -> dict:
        v = [C.c_int32(0) for _ in range(4)]
        self._c(self.lib.fgpu_diag_device_attr(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("memory_clock_khz", "memory_bus_bits", "l2_bytes", "compute_units"), [int(x.value) for x in v]))

    def diag_random_access(self, table_bytes: int, n_access: int, mode: int = 0, iters: int = 3) -> float:
        """measured independent random 32-bit accesses/s into a table of table_bytes (0 load, 1 atomicMin, 2 test+atomicOr)"""
        out = C.c_double(0)
        self._c(self.lib.fgpu_diag_random_access(self.h, table_bytes, n_access, mode, iters, C.byref(out)))
        return out.value


# ---- reference-shaped front end -------------------------------------------------------------------------------------
class Bloom:
    """Handle on one of the two load filters of a Context (utils/Bloom.h: tai, n_hash_func, blooma)."""

    def __init__(self, ctx: Context, which: int):
        self.ctx, self.which = ctx, which
        self.tai, self.n_hash_func = ctx.tai, ctx.n_hash

    def weight(self) -> float:                       # Bloom::weight
        return self.ctx.bloom_weight(self.which)

    def blooma(self) -> np.ndarray:                  # the raw bit array
        return self.ctx.bloom_download(self.which)

    def dump(self, path: str):                       # Bloom::dump (utils/Bloom.cpp:571-578)
        self.blooma().tofile(path)

    def load(self, path: str):                       # Bloom::load (utils/Bloom.cpp:580-587)
        self.ctx.bloom_upload(self.which, np.fromfile(path, dtype=np.uint8, count=self.tai // 8))

    def oldContains(self, canon_kmers):              # Bloom::oldContains (utils/Bloom.h:162-173), batched
        return self.ctx.probe_contains(self.which, canon_kmers)


def group_allgather(group, rank: int, buf_dev_ptr, nbytes: int, bounds) -> int:
    """fgpu_group_allgather on a group made with fgpu_group_create: rank q holds the bytes [bounds[q], bounds[q+1]) of the buffer, afterwards every
    rank holds all of them.  Returns the status (the caller reads fgpu_group_last_error)."""
    arr = (C.c_uint64 * len(bounds))(*[int(b) for b in bounds])
    return L.load().fgpu_group_allgather(group, rank, buf_dev_ptr, nbytes, arr)


def group_estimate_end(group, rank: int):
    """fgpu_group_estimate_end, called by every rank's thread in place of Context.estimate_end: (status, the dict estimate_end gives -- the same on
    every rank, that of one sketch of all the ranks' reads; None unless the status is OK or ERR_CAPACITY).  The pass is over on every rank whatever
    the status (the caller reads fgpu_group_last_error)."""
    e = L.Estimate()
    rc = L.load().fgpu_group_estimate_end(group, rank, C.byref(e))
    return rc, (e.as_dict() if rc in (L.OK, L.ERR_CAPACITY) else None)


def load_two_filters(bloo1: Bloom, bloo2: Bloom, batches) -> dict:
    """load_two_filters (utils/Bloom.cpp:267-350): `batches` is an iterable of ReadBatch in file order."""
    ctx = bloo1.ctx
    assert bloo2.ctx is ctx and bloo1.which == L.BLOO1 and bloo2.which == L.BLOO2
    ctx.load_begin()
    for b in batches:
        ctx.load_batch(b)
    return ctx.load_end()


class ReadScanner:
    """ReadScanner (src/ReadScanner.h:30-92) on the device junction map of a Context."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.stats = None
        self.fell_back_to_eager = False

    def scanReads(self, batches):                    # src/ReadScanner.cpp:284-359
        replays = self.ctx.diag_scan_replays()
        st = self._scan(batches)
        # (the library scanned its journal again because the lazy junction-test preview could not be repaired: DESIGN.md section 4)
        self.fell_back_to_eager = self.ctx.diag_scan_replays() > replays
        return st

    def _scan(self, batches):
        self.ctx.scan_begin()
        for b in batches:
            self.ctx.scan_batch(b)
        self.stats = self.ctx.scan_end()
        return self.stats

    def junctions(self):
        return self.ctx.junctions()


_DEC = np.frombuffer(b"ACTG", dtype=np.uint8)


def _tips_graph(out, fill):
    """room for what `out` (an L.TipsOut whose n_* are set) needs, `fill()` run on it, and the graph as a dict"""
    nodes, contigs = np.zeros(out.n_nodes, dtype=TIPS_NODE_DTYPE), np.zeros(out.n_contigs, dtype=TIPS_CONTIG_DTYPE)
    first, pieces = np.zeros(out.n_contigs + 1, dtype=np.uint64), np.zeros(out.n_pieces, dtype=JOIN_PIECE_DTYPE)
    out.nodes, out.nodes_cap = nodes.ctypes.data, len(nodes)
    out.contigs, out.list_first, out.contigs_cap = contigs.ctypes.data, first.ctypes.data, len(contigs)
    out.pieces, out.pieces_cap = pieces.ctypes.data, len(pieces)
    fill()
    return dict(nodes=nodes, contigs=contigs, lists=_lists_of(first, pieces))


def _lists_of(first, pieces):
    return [[(int(p["call"]), bool(p["flip"])) for p in pieces[int(a):int(b)]] for a, b in zip(first[:-1], first[1:])]


def tips_plan(keys, recs, contigs, calls, k: int, read_length: int):
    """fgpu_tips_plan, host only: which piece lists ContigGraph::deleteTipsAndClean leaves of a finished build (keys and JUNC_DTYPE records in map
    order, the CONTIG_DTYPE and BUILD_DTYPE arrays of stage3_build) and which of them printContigs prints.  Returns (status, graph, records,
    info): graph as Context.stage3_graph_take gives it, records = [(number, [(call, flip)])] in file order, info as Context.stage3_detip's;
    graph and records are None unless status is PLAN_OK (0)."""
    lib = L.load()
    keys, recs = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(recs, dtype=JUNC_DTYPE)
    contigs, calls = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE), np.ascontiguousarray(calls, dtype=BUILD_DTYPE)
    out, ti = L.TipsOut(), L.TipsInfo()
    args = (keys.ctypes.data, recs.ctypes.data, len(keys), contigs.ctypes.data, calls.ctypes.data, len(contigs), int(k), int(read_length), C.byref(out), C.byref(ti))
    status = lib.fgpu_tips_plan(*args)                                    # (no room: how much is needed)
    if status not in (L.PLAN_OK, L.PLAN_SHORT):
        return status, None, None, ti.as_dict()
    first, number = np.zeros(out.n_print + 1, dtype=np.uint64), np.zeros(out.n_print, dtype=np.uint32)
    pieces = np.zeros(out.n_print_pieces, dtype=JOIN_PIECE_DTYPE)
    out.print_first, out.print_number, out.print_cap = first.ctypes.data, number.ctypes.data, len(number)
    out.print_pieces, out.print_pieces_cap = pieces.ctypes.data, len(pieces)
    state = {}

    def fill():
        state["status"] = lib.fgpu_tips_plan(*args)
    graph = _tips_graph(out, fill)
    if state["status"] != L.PLAN_OK:
        return state["status"], None, None, ti.as_dict()
    return L.PLAN_OK, graph, list(zip((int(v) for v in number), _lists_of(first, pieces))), ti.as_dict()


def chimera_plan(keys, recs, contigs, calls, cov_calls, k: int, read_length: int):
    """fgpu_chimera_plan, host only: which piece lists ContigGraph::deleteTipsAndClean and then removeChimerasAndClean leave of a finished build
    (tips_plan's arguments and cov_calls, one COV_SUMMARY_DTYPE record per call: Context.stage3_cov_calls' output) and which of them printContigs
    prints.  Returns (status, graph, records, info, tips_info): graph and records as tips_plan gives them, after the second step; info as
    Context.stage3_dechimera's; tips_info the first step's account (its print part is empty).  graph and records are None unless status is
    PLAN_OK (0)."""
    lib = L.load()
    keys, recs = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(recs, dtype=JUNC_DTYPE)
    contigs, calls = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE), np.ascontiguousarray(calls, dtype=BUILD_DTYPE)
    cov_calls = np.ascontiguousarray(cov_calls, dtype=COV_SUMMARY_DTYPE)
    if len(cov_calls) != len(contigs):
        raise ValueError("one coverage summary per call")
    out, ti, ci = L.TipsOut(), L.TipsInfo(), L.ChimeraInfo()
    args = (keys.ctypes.data, recs.ctypes.data, len(keys), contigs.ctypes.data, calls.ctypes.data, len(contigs), cov_calls.ctypes.data, int(k), int(read_length),
            C.byref(out), C.byref(ti), C.byref(ci))
    status = lib.fgpu_chimera_plan(*args)                                 # (no room: how much is needed)
    if status not in (L.PLAN_OK, L.PLAN_SHORT):
        return status, None, None, ci.as_dict(), ti.as_dict()
    first, number = np.zeros(out.n_print + 1, dtype=np.uint64), np.zeros(out.n_print, dtype=np.uint32)
    pieces = np.zeros(out.n_print_pieces, dtype=JOIN_PIECE_DTYPE)
    out.print_first, out.print_number, out.print_cap = first.ctypes.data, number.ctypes.data, len(number)
    out.print_pieces, out.print_pieces_cap = pieces.ctypes.data, len(pieces)
    state = {}

    def fill():
        state["status"] = lib.fgpu_chimera_plan(*args)
    graph = _tips_graph(out, fill)
    if state["status"] != L.PLAN_OK:
        return state["status"], None, None, ci.as_dict(), ti.as_dict()
    return L.PLAN_OK, graph, list(zip((int(v) for v in number), _lists_of(first, pieces))), ci.as_dict(), ti.as_dict()


def print_kmer(kmer: int, k: int) -> str:            # print_kmer / code2seq (utils/Kmer.cpp:217)
    return "".join(chr(_DEC[(int(kmer) >> (2 * (k - 1 - i))) & 3]) for i in range(k))


def junction_lines(keys, recs, k):
    """The `.junctions` line of every record (Junction::toString, utils/Junction.cpp:74-89)."""
    out = []
    for key, r in zip(keys, recs):
        cv = [int(x) for x in r["cov"]]
        out.append("%s %s  %s  %s " % (print_kmer(int(key), k), " ".join(str(int(x)) for x in r["dist"]),
                                       " ".join(str(x) for x in cv + [sum(cv)]), " ".join(str(int(x)) for x in r["linked"])))
    return out


_ENC = {"A": 0, "C": 1, "T": 2, "G": 3}


def parse_junction_lines(lines, k):
    """Inverse of junction_lines: the `.junctions` text back to (keys, records), the way a restart with `-junctions_file` reads it
    (JunctionMap::buildFromFile utils/JunctionMap.cpp:619-639 + Junction(string) utils/Junction.cpp:102-118: k-mer word, 5 dists,
    4 coverages, one total that is skipped, 5 link flags, all whitespace-separated)."""
    lines = [ln for ln in lines if ln.strip()]
    keys = np.zeros(len(lines), dtype=np.uint64)
    recs = np.zeros(len(lines), dtype=JUNC_DTYPE)
    for i, ln in enumerate(lines):
        w = ln.split()
        if len(w) != 16 or len(w[0]) != k:
            raise ValueError(f"junction line {i}: expected a {k}-mer and 15 numbers, got {ln!r}")
        key = 0
        for ch in w[0]:
            key = (key << 2) | _ENC[ch]
        keys[i] = key
        v = [int(x) for x in w[1:]]
        recs[i]["dist"], recs[i]["cov"], recs[i]["linked"] = v[0:5], v[5:9], v[10:15]
    return keys, recs
