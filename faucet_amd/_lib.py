"""ctypes loader for libfaucet_gpu.so (the C ABI of include/faucet_gpu.h).

Fails loudly: if the shared library is missing or does not export the ABI there is no fallback of any kind.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libfaucet_gpu.so")

OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_CAPACITY, ERR_NOMEM, ERR_INTERNAL = range(7)
BLOO1, BLOO2 = 0, 1
FLAG_PROFILE = 1
FLAG_EAGER_FLAGS = 2
FLAG_NO_RESIDENT = 4
FLAG_RECORD_STOPS = 8
FLAG_MERCY = 16
FLAG_KEY_ORDER_FROM_START = 32
STOP_POS_MASK, STOP_FORWARD, STOP_FIRST, STOP_FAKE = 0x0FFFFFFF, 1 << 28, 1 << 29, 1 << 30
TABLE_ENTRY_BYTES = 32


class Params(C.Structure):
    _fields_ = [("k", C.c_int32), ("j", C.c_int32), ("max_spacer_dist", C.c_int32), ("n_hash", C.c_int32),
                ("tai", C.c_uint64), ("device", C.c_int32), ("flags", C.c_int32), ("junction_capacity", C.c_uint64),
                ("max_batch_bases", C.c_uint64), ("stream", C.c_void_p), ("walk_window_span", C.c_uint64)]


LOAD_KEEP_CARRY, LOAD_SHARD_TIMES, LOAD_SHARD_PLANES, LOAD_KEEP_READS = 1, 2, 4, 8


class Reads(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_reads", C.c_uint64), ("on_device", C.c_int32),
                ("total_bases", C.c_uint32), ("starts", C.c_void_p)]


class Packed(C.Structure):
    """fgpu_packed: one packed batch of a sliced pass as a device block"""
    _fields_ = [("block_dev", C.c_void_p), ("nbytes", C.c_uint64), ("T", C.c_uint64), ("n_reads", C.c_uint64)]


class KeptReads(C.Structure):
    """fgpu_kept_reads: the read offsets of one packed batch (device), its read count, the longest read of its pass"""
    _fields_ = [("offsets_dev", C.c_void_p), ("n_reads", C.c_uint64), ("max_read_len", C.c_uint64)]


class LoadStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads_processed", "unambiguous_reads", "kmers", "to_bloo2")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


EST_LEVELS, EST_SHIFT, EST_MIN_BITS, EST_MAX_BITS, EST_DEFAULT_BITS = 4, 4, 8, 34, 30


class Estimate(C.Structure):
    """fgpu_estimate: the counts of a sketch of the reads (pass 0) and what fgpu_estimate_solve makes of them"""
    _fields_ = [("empty", C.c_uint64 * 4), ("once", C.c_uint64 * 4), ("kmers", C.c_uint64), ("r_bits", C.c_int32), ("level", C.c_int32),
                ("f0", C.c_double), ("f1", C.c_double)]

    def as_dict(self):
        return {"empty": [int(x) for x in self.empty], "once": [int(x) for x in self.once], "kmers": int(self.kmers), "r_bits": int(self.r_bits),
                "level": int(self.level), "f0": float(self.f0), "f1": float(self.f1)}


class ScanStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads_processed", "unambiguous_reads", "reads_no_errors", "nb_jcheck_kmer", "nb_no_juncs",
                                          "nb_processed", "nb_skipped", "n_junctions", "kmers", "walk_windows", "walk_followers",
                                          "walk_max_cluster", "flag_positions", "piece_positions", "valid_reused", "flags_filled", "walk_parallel")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


BUILD_ROUNDS_KEPT = 32


class RawInfo(C.Structure):
    """fgpu_raw_info: what the raw contigs file holds"""
    _fields_ = [(n, C.c_uint64) for n in ("records", "bubble_records", "node_contigs", "isolated_kept", "isolated_dropped", "nodes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


PLAN_OK, PLAN_UNSET, PLAN_INPUT, PLAN_SHORT = range(4)


class TipsInfo(C.Structure):
    """fgpu_tips_info: what ContigGraph::deleteTipsAndClean did, and what the file printed behind it holds"""
    _fields_ = [("nodes_before", C.c_uint64), ("tips", C.c_uint64), ("back_tips", C.c_uint64), ("collapsed", C.c_uint64 * 2), ("degenerate", C.c_uint64 * 2),
                ("validated", C.c_uint32), ("changed", C.c_uint32), ("print", RawInfo)]

    def as_dict(self):
        return dict(nodes_before=int(self.nodes_before), tips=int(self.tips), back_tips=int(self.back_tips), collapsed=[int(v) for v in self.collapsed],
                    degenerate=[int(v) for v in self.degenerate], validated=int(self.validated), changed=int(self.changed), print=self.print.as_dict())


class ChimeraInfo(C.Structure):
    """fgpu_chimera_info: what ContigGraph::removeChimerasAndClean did, and what the file printed behind it holds"""
    _fields_ = [("nodes_before", C.c_uint64), ("removed", C.c_uint64), ("cut_near", C.c_uint64), ("cut_far", C.c_uint64), ("cut_both", C.c_uint64),
                ("collapsed", C.c_uint64 * 2), ("degenerate", C.c_uint64 * 2), ("collapsed_after_cut", C.c_uint64), ("skipped", C.c_uint64 * 6),
                ("validated", C.c_uint32), ("changed", C.c_uint32), ("print", RawInfo)]

    def as_dict(self):
        return dict(nodes_before=int(self.nodes_before), removed=int(self.removed), cut_near=int(self.cut_near), cut_far=int(self.cut_far), cut_both=int(self.cut_both),
                    collapsed=[int(v) for v in self.collapsed], degenerate=[int(v) for v in self.degenerate], collapsed_after_cut=int(self.collapsed_after_cut),
                    skipped=[int(v) for v in self.skipped], validated=int(self.validated), changed=int(self.changed), print=self.print.as_dict())


class FastgInfo(C.Structure):
    """fgpu_fastg_info: ContigGraph::printGraph's counts"""
    _fields_ = [(n, C.c_uint64) for n in ("node_records", "isolated_printed", "isolated_listed", "nodes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


FASTG_PRIMED, FASTG_TILE, FASTG_NAME_STRIDE = 0x80000000, 4096, 64


class TipsOut(C.Structure):
    """fgpu_tips_out: the arrays fgpu_tips_plan and fgpu_stage3_graph_take fill, their room, and how much was needed"""
    _fields_ = [("nodes", C.c_void_p), ("nodes_cap", C.c_uint64), ("n_nodes", C.c_uint64),
                ("contigs", C.c_void_p), ("list_first", C.c_void_p), ("contigs_cap", C.c_uint64), ("n_contigs", C.c_uint64),
                ("pieces", C.c_void_p), ("pieces_cap", C.c_uint64), ("n_pieces", C.c_uint64),
                ("print_first", C.c_void_p), ("print_number", C.c_void_p), ("print_cap", C.c_uint64), ("n_print", C.c_uint64),
                ("print_pieces", C.c_void_p), ("print_pieces_cap", C.c_uint64), ("n_print_pieces", C.c_uint64)]


class BuildInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("rounds", C.c_uint32), ("stop_call", C.c_uint64), ("calls_possible", C.c_uint64), ("rewalked", C.c_uint64),
                ("probes", C.c_uint64), ("table_hits", C.c_uint64), ("regrown", C.c_uint64), ("rewalked_by_round", C.c_uint64 * BUILD_ROUNDS_KEPT)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double)]


# every symbol include/faucet_gpu.h declares: (restype, argtypes)
_u64, _i32, _vp, _f32, _f64 = C.c_uint64, C.c_int32, C.c_void_p, C.c_float, C.c_double
_P = C.POINTER
SIGNATURES = {
    "fgpu_abi_version": (C.c_int, []),
    "fgpu_device_count": (C.c_int, []),
    "fgpu_create": (C.c_int, [_P(Params), _P(_vp)]),
    "fgpu_destroy": (None, [_vp]),
    "fgpu_last_error": (C.c_char_p, [_vp]),
    "fgpu_synchronize": (C.c_int, [_vp]),
    "fgpu_solve_p1": (_f64, [_u64, _u64, _f32, _P(_i32)]),
    "fgpu_bloom_tai": (_u64, [_u64]),
    "fgpu_size_optimal": (None, [_u64, _f32, _P(_i32), _P(_u64), _P(_i32)]),
    "fgpu_size_two_hash": (None, [_u64, _f32, _P(_i32), _P(_u64), _P(_i32)]),
    "fgpu_estimate_begin": (C.c_int, [_vp, _i32]),
    "fgpu_estimate_batch": (C.c_int, [_vp, _P(Reads)]),
    "fgpu_estimate_end": (C.c_int, [_vp, _P(Estimate)]),
    "fgpu_estimate_solve": (C.c_int, [_P(Estimate)]),
    "fgpu_estimate_planes": (C.c_int, [_vp, _P(_vp), _P(_u64)]),
    "fgpu_estimate_merge": (C.c_int, [_vp, _vp, _u64, _u64]),
    "fgpu_estimate_download": (C.c_int, [_vp, _vp, _u64]),
    "fgpu_estimate_kmers": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_estimate_keep": (C.c_int, [_vp, _u64]),
    "fgpu_estimate_keep_state": (C.c_int, [_vp, _P(C.c_int), _P(_u64), _P(_u64)]),
    "fgpu_estimate_take_kept": (C.c_int, [_vp, _P(Packed), _u64, _P(_u64)]),
    "fgpu_estimate_keep_reads": (C.c_int, [_vp]),
    "fgpu_estimate_take_kept_reads": (C.c_int, [_vp, _P(KeptReads), _u64, _P(_u64)]),
    "fgpu_load_batch_packed_reads": (C.c_int, [_vp, _P(Packed), _P(KeptReads)]),
    "fgpu_scan_kept_state": (C.c_int, [_vp, _P(C.c_int), _P(_u64), _P(_u64), _P(_u64)]),
    "fgpu_scan_batch_kept": (C.c_int, [_vp, _u64, _P(_u64)]),
    "fgpu_scan_kept_range": (C.c_int, [_vp, _u64, _u64, _u64, _P(C.c_int)]),
    "fgpu_scan_prepare_kept": (C.c_int, [_vp, _u64, _P(_u64)]),
    "fgpu_load_slice_keep_reads": (C.c_int, [_vp]),
    "fgpu_load_slice_packed_reads": (C.c_int, [_vp, _P(Packed), _P(KeptReads)]),
    "fgpu_load_slice_expect_reads": (C.c_int, [_vp, _P(Packed), _P(KeptReads)]),
    "fgpu_load_slice_adopt_reads": (C.c_int, [_vp, _P(Packed), _P(KeptReads)]),
    "fgpu_load_begin": (C.c_int, [_vp, C.c_int]),
    "fgpu_load_batch": (C.c_int, [_vp, _P(Reads)]),
    "fgpu_load_batch_packed": (C.c_int, [_vp, _P(Packed)]),
    "fgpu_load_end": (C.c_int, [_vp, _P(LoadStats)]),
    "fgpu_presence_batch": (C.c_int, [_vp, _P(Reads)]),
    "fgpu_load_fixup": (C.c_int, [_vp, _vp, _P(LoadStats)]),
    "fgpu_load_fixup_state": (C.c_int, [_vp, _P(C.c_int), _P(C.c_uint64)]),
    "fgpu_load_slice_begin": (C.c_int, [_vp, _u64, _u64]),
    "fgpu_load_slice_batch": (C.c_int, [_vp, _P(Reads)]),
    "fgpu_load_slice_plane": (C.c_int, [_vp, _u64, _P(_vp), _P(_u64)]),
    "fgpu_load_slice_commit": (C.c_int, [_vp]),
    "fgpu_load_slice_end": (C.c_int, [_vp, _P(LoadStats)]),
    "fgpu_load_slice_state": (C.c_int, [_vp, _P(C.c_int), _P(_u64), _P(_u64)]),
    "fgpu_load_slice_mercy_begin": (C.c_int, [_vp, _u64, _u64]),
    "fgpu_load_slice_mercy_probe": (C.c_int, [_vp]),
    "fgpu_load_slice_mercy_planes": (C.c_int, [_vp, _u64, _P(_vp), _P(_u64)]),
    "fgpu_diag_slice_mercy": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_load_slice_pack": (C.c_int, [_vp, _P(Reads), _P(Packed)]),
    "fgpu_load_slice_expect": (C.c_int, [_vp, _u64, _u64, _P(Packed)]),
    "fgpu_load_slice_batch_packed": (C.c_int, [_vp, _P(Packed)]),
    "fgpu_scan_resident_base": (C.c_int, [_vp, _u64]),
    "fgpu_scan_dump_order": (C.c_int, [_vp, _P(C.c_uint64), _P(C.c_uint64), C.c_uint64, C.c_uint64, _P(C.c_uint32)]),
    "fgpu_bloom_download": (C.c_int, [_vp, C.c_int, _vp, _u64]),
    "fgpu_bloom_download_begin": (C.c_int, [_vp, C.c_int, _vp, _u64]),
    "fgpu_bloom_download_wait": (C.c_int, [_vp]),
    "fgpu_bloom_upload": (C.c_int, [_vp, C.c_int, _vp, _u64]),
    "fgpu_bloom_weight": (C.c_int, [_vp, C.c_int, _P(_f32)]),
    "fgpu_bloom_devptr": (C.c_int, [_vp, C.c_int, _P(_vp), _P(_u64)]),
    "fgpu_bitmap_or": (C.c_int, [_vp, _vp, _vp, _u64]),
    "fgpu_host_alloc": (_vp, [_u64]),
    "fgpu_host_free": (None, [_vp]),
    "fgpu_text_reserve": (C.c_int, [_vp, _u64]),
    "fgpu_text_split": (C.c_int, [_vp, _vp, _u64, C.c_int, C.c_int, C.c_int, _P(Reads), _P(_u64)]),
    "fgpu_scan_begin": (C.c_int, [_vp]),
    "fgpu_scan_batch": (C.c_int, [_vp, _P(Reads)]),
    "fgpu_scan_prepare": (C.c_int, [_vp, _P(Reads)]),
    "fgpu_scan_walk_prepared": (C.c_int, [_vp]),
    "fgpu_scan_end": (C.c_int, [_vp, _P(ScanStats)]),
    "fgpu_scan_set_eager": (C.c_int, [_vp, C.c_int]),
    "fgpu_scan_take_stops": (C.c_int, [_vp, _vp, _u64, _P(_u64), _P(C.c_int64)]),
    "fgpu_scan_junction_count": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_scan_download_junctions": (C.c_int, [_vp, _vp, _vp, _u64, _P(_u64)]),
    "fgpu_scan_table_entries": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_scan_export_table": (C.c_int, [_vp, _vp, _u64, _P(_u64)]),
    "fgpu_scan_import_table": (C.c_int, [_vp, _vp, _u64, _P(ScanStats)]),
    "fgpu_scan_import_hint": (C.c_int, [_vp, _vp, _u64]),
    "fgpu_scan_short_pairs": (C.c_int, [_vp, _u64, _i32, _i32]),
    "fgpu_scan_short_pairs_download": (C.c_int, [_vp, _vp, _u64]),
    "fgpu_scan_long_pairs": (C.c_int, [_vp, _u64, _i32, _i32]),
    "fgpu_scan_long_pairs_download": (C.c_int, [_vp, _vp, _u64, _P(_u64), _P(_u64)]),
    "fgpu_diag_long_pairs": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_diag_long_pairs_state": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_diag_ovw": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_diag_ovw_tables": (C.c_int, [_vp, _P(_u64), _P(_u64)]),
    "fgpu_scan_refresh_prepared": (C.c_int, [_vp]),
    "fgpu_diag_prepared_refresh": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_diag_sparse_link": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_probe_hash": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "fgpu_probe_contains": (C.c_int, [_vp, C.c_int, _vp, _u64, _vp]),
    "fgpu_probe_jcheck": (C.c_int, [_vp, _vp, _u64, _vp]),
    "fgpu_probe_valid_extension": (C.c_int, [_vp, _vp, _u64, _vp]),
    "fgpu_probe_bloom_junction": (C.c_int, [_vp, _vp, _u64, _vp]),
    "fgpu_stage3_set_junctions": (C.c_int, [_vp, _vp, _vp, _u64]),
    "fgpu_stage3_find_neighbors": (C.c_int, [_vp, _vp, _vp, _u64, _i32, _vp, _P(_u64), _vp, _u64]),
    "fgpu_stage3_contig_words": (_u64, [_i32, _i32]),
    "fgpu_stage3_contigs": (C.c_int, [_vp, _vp, _vp, _u64, _i32, _vp, _P(_u64), _P(_u64)]),
    "fgpu_stage3_contigs_take": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64]),
    "fgpu_stage3_build": (C.c_int, [_vp, _i32, _P(_u64), _P(BuildInfo)]),
    "fgpu_stage3_build_take": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _u64]),
    "fgpu_raw_plan": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, _i32, _i32, _vp, _u64, _P(_u64), _P(RawInfo)]),
    "fgpu_stage3_fasta": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _P(_u64)]),
    "fgpu_stage3_fasta_take": (C.c_int, [_vp, _vp, _u64]),
    "fgpu_stage3_raw_contigs": (C.c_int, [_vp, _i32, _P(_u64), _P(RawInfo)]),
    "fgpu_stage3_join": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _P(_u64)]),
    "fgpu_stage3_join_take": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _vp, _u64]),
    "fgpu_stage3_build_totals": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_stage3_cov_calls": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "fgpu_tips_plan": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, _i32, _i32, _P(TipsOut), _P(TipsInfo)]),
    "fgpu_stage3_fasta_joined": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _P(_u64)]),
    "fgpu_stage3_detip": (C.c_int, [_vp, _i32, _P(_u64), _P(TipsInfo)]),
    "fgpu_stage3_graph_take": (C.c_int, [_vp, _P(TipsOut)]),
    "fgpu_chimera_plan": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _i32, _i32, _P(TipsOut), _P(TipsInfo), _P(ChimeraInfo)]),
    "fgpu_stage3_dechimera": (C.c_int, [_vp, _P(_u64), _P(ChimeraInfo)]),
    "fgpu_stage3_fastg": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _P(_u64)]),
    "fgpu_stage3_raw_graph": (C.c_int, [_vp, _i32, _P(_u64), _P(FastgInfo)]),
    "fgpu_stage3_graph_fastg": (C.c_int, [_vp, _P(_u64), _P(FastgInfo)]),
    "fgpu_diag_fastg_times": (C.c_int, [_vp, _P(_f64)]),
    "fgpu_kernel_times": (C.c_int, [_vp, _P(KernelTime), C.c_int]),
    "fgpu_kernel_times_reset": (C.c_int, [_vp]),
    "fgpu_profile_enable": (C.c_int, [_vp, C.c_int]),
    "fgpu_diag_stream_copy": (C.c_int, [_vp, _u64, C.c_int, _P(_f64)]),
    "fgpu_diag_random_access": (C.c_int, [_vp, _u64, _u64, C.c_int, C.c_int, _P(_f64)]),
    "fgpu_diag_ko_trace": (C.c_int, [_vp, _vp, _u64, _P(_u64)]),
    "fgpu_diag_ko_stamps": (C.c_int, [_vp, _vp, _u64, _P(_u64)]),
    "fgpu_diag_binned_chain": (C.c_int, [_vp, _u64, _u64, _u64, C.c_int, C.c_int, C.c_int, _P(_f64), _P(_f64), _P(_f64), _P(_f64), _P(_f64), _P(C.c_int)]),
    "fgpu_diag_device_attr": (C.c_int, [_vp, _P(_i32), _P(_i32), _P(_i32), _P(_i32)]),
    "fgpu_diag_walk_probe": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_diag_load_split": (C.c_int, [_vp, _P(_u64), _P(_u64)]),
    "fgpu_diag_scan_replays": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_diag_host_waits": (C.c_int, [_vp, _P(_u64), _P(_f64)]),
    "fgpu_diag_load_tables": (C.c_int, [_vp, _u64, _P(_f64), _P(_f64), _P(_f64)]),
    "fgpu_diag_pair_placements": (C.c_int, [_vp, C.c_int, _u64, _P(_f64)]),
    "fgpu_diag_late_flags": (C.c_int, [_vp, _P(_u64)]),
    "fgpu_diag_binned_probes": (C.c_int, [_vp, _u64, _u64, _u64, C.c_int, _P(_f64), _P(_f64), _P(_f64), _P(_f64)]),
    "fgpu_scan_pairs_devptr": (C.c_int, [_vp, C.c_int, _P(_vp), _P(_u64)]),
    "fgpu_device_alloc": (C.c_int, [_vp, _u64, _P(_vp)]),
    "fgpu_device_free": (C.c_int, [_vp, _vp]),
    "fgpu_device_copy": (C.c_int, [_vp, _vp, _vp, _u64]),
    "fgpu_device_zero": (C.c_int, [_vp, _vp, _u64]),
    "fgpu_group_create": (C.c_int, [C.c_int, C.c_int, _P(_vp)]),
    "fgpu_group_destroy": (None, [_vp]),
    "fgpu_group_attach": (C.c_int, [_vp, C.c_int, _vp]),
    "fgpu_group_abort": (None, [_vp]),
    "fgpu_group_last_error": (C.c_char_p, [_vp, C.c_int]),
    "fgpu_group_barrier": (C.c_int, [_vp, C.c_int]),
    "fgpu_group_or_allreduce": (C.c_int, [_vp, C.c_int, _vp, _u64]),
    "fgpu_group_exclusive_prefix_or": (C.c_int, [_vp, C.c_int, _vp, _vp, _u64]),
    "fgpu_group_allgather": (C.c_int, [_vp, C.c_int, _vp, _u64, _P(_u64)]),
    "fgpu_group_estimate_end": (C.c_int, [_vp, C.c_int, _P(Estimate)]),
    "fgpu_group_send": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _u64]),
    "fgpu_group_send_async": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _u64]),
    "fgpu_group_flush": (C.c_int, [_vp, C.c_int]),
    "fgpu_group_recv": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _u64]),
    "fgpu_group_probe": (C.c_int, [_vp, C.c_int, C.c_int, _P(C.c_int), _P(_u64)]),
    "fgpu_group_selftest": (C.c_int, [_vp, C.c_int, _u64, _P(C.c_int)]),
}
TRANSPORT_COPY, TRANSPORT_RCCL = 0, 1

_lib = None


def load():
    """Load the shared library (once).  Raises if it is missing or incomplete — never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m faucet_amd.build` (hipcc, gfx950). "
                           "There is no CPU fallback.")
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7.  If torch is going to be used in this
    # process (bench.py, torch.distributed) it must be loaded FIRST so that our NEEDED libamdhip64.so.7 binds to
    # the copy already mapped; two runtimes in one process leave the second one without a device.
    if os.environ.get("FAUCET_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    # FAUCET_GPU_LIB: another build of the SAME library (host code under AddressSanitizer: scripts/asan_gpu_fuzz.sh); never a fallback
    lib = C.CDLL(os.environ.get("FAUCET_GPU_LIB") or LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.fgpu_abi_version() != 3:
        raise RuntimeError("libfaucet_gpu.so ABI version mismatch")
    _lib = lib
    return lib
