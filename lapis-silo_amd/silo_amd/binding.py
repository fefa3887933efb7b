"""ctypes binding of include/silo_gpu.h (the C-ABI drop-in boundary).

This is the stub a maintainer of a Python host would write; the reference's own host is C++ and binds
the same symbols directly.  There is no CPU fallback: if the HIP library is missing or
no GPU is visible every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import alphabet

_LIB_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib")
_LIB_PATH = os.path.join(_LIB_DIR, "libsilo_gpu.so")

c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_u16p = ctypes.POINTER(ctypes.c_uint16)
c_u32p = ctypes.POINTER(ctypes.c_uint32)
c_u64p = ctypes.POINTER(ctypes.c_uint64)


class SiloGpuError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"silo_gpu error {code}: {message}")
        self.code = code


class SeqStoreDesc(ctypes.Structure):
    _fields_ = [
        ("alphabet", ctypes.c_uint32),
        ("positions", ctypes.c_uint32),
        ("reference", c_u8p),
        ("n_scan_symbols", ctypes.c_uint32),
        ("scan_symbols", c_u8p),
        ("n_extra_symbols", ctypes.c_uint32),
        ("extra_symbols", c_u8p),
    ]


class StoreDesc(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("sequence_count", ctypes.c_uint32),
        ("n_seqstores", ctypes.c_uint32),
        ("seqstores", ctypes.POINTER(SeqStoreDesc)),
    ]


class SynthDesc(ctypes.Structure):
    _fields_ = [
        ("seed", ctypes.c_uint64),
        ("n_lineages", ctypes.c_uint32),
        ("lineage_of_sequence", c_u16p),
        ("lead_gap", c_u32p),
        ("trail_gap", c_u32p),
        ("missing_start", c_u32p),
        ("missing_len", c_u32p),
        ("lineage_symbol", c_u8p),
        ("private_threshold", ctypes.c_uint32),
        ("ambiguous_threshold", ctypes.c_uint32),
        ("position_offset", ctypes.c_uint32),
        ("total_positions", ctypes.c_uint32),
    ]


class RoaringPayload(ctypes.Structure):
    _fields_ = [("symbol", ctypes.c_uint32), ("bytes", ctypes.c_char_p), ("n_bytes", ctypes.c_size_t)]


class ScanTiming(ctypes.Structure):
    """silo_gpu_scan_timing: one plane-scan launch of the thread's last Mutations scan."""
    _fields_ = [("kernel", ctypes.c_char * 64), ("plane_rows", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("filters", ctypes.c_uint32),
                ("blocks", ctypes.c_uint32), ("ms", ctypes.c_float)]


def scan_timings(capacity=64):
    """Per-launch timings of this thread's last scan (SILO_GPU_TUNE_SCAN_TIMING = knob 7 set to 1 before it)."""
    lib = load_library()
    out = (ScanTiming * capacity)()
    n = ctypes.c_uint32()
    _check(lib.silo_gpu_scan_timings(out, capacity, ctypes.byref(n)))
    return [dict(kernel=out[k].kernel.decode(), plane_rows=int(out[k].plane_rows), bytes=int(out[k].bytes), filters=int(out[k].filters), blocks=int(out[k].blocks),
                 ms=float(out[k].ms))
            for k in range(min(capacity, n.value))]


class BitProg(ctypes.Structure):
    _fields_ = [
        ("n_instructions", ctypes.c_uint32),
        ("code", c_u32p),
        ("n_leaves", ctypes.c_uint32),
        ("leaves", ctypes.POINTER(ctypes.c_void_p)),
        ("n_slots", ctypes.c_uint32),
    ]


# every symbol include/silo_gpu.h declares; tests check the library exports all of them
EXPORTED_SYMBOLS = [
    "silo_gpu_store_create", "silo_gpu_store_destroy", "silo_gpu_store_set_options", "silo_gpu_store_sequence_count",
    "silo_gpu_store_row_words", "silo_gpu_store_device_bytes", "silo_gpu_store_append_sequences",
    "silo_gpu_store_finalize", "silo_gpu_store_generate_synthetic", "silo_gpu_bitset_alloc",
    "silo_gpu_bitset_upload", "silo_gpu_bitset_download", "silo_gpu_bitset_from_lineages", "silo_gpu_upload_u32",
    "silo_gpu_bitset_from_value_ids", "silo_gpu_free",
    "silo_gpu_malloc", "silo_gpu_memcpy_d2h", "silo_gpu_memcpy_h2d", "silo_gpu_stream_synchronize", "silo_gpu_stream_create", "silo_gpu_set_device", "silo_gpu_stream_destroy", "silo_gpu_store_plane",
    "silo_gpu_store_sparse_plane", "silo_gpu_filter_eval", "silo_gpu_filter_eval_batch", "silo_gpu_popcount", "silo_gpu_mutations_scan", "silo_gpu_mutations_scan_batch", "silo_gpu_mutations_scan_ranges", "silo_gpu_mutations_grouped", "silo_gpu_store_scan_planes", "silo_gpu_store_scan_escapes", "silo_gpu_store_scan_overflow_keys", "silo_gpu_store_scan_rows", "silo_gpu_store_scan_runs", "silo_gpu_row_slot_create", "silo_gpu_row_slot_destroy", "silo_gpu_mutations_select_to_slot", "silo_gpu_row_slot_wait", "silo_gpu_store_scan_sparse_keys", "silo_gpu_store_finalize_seqstore", "silo_gpu_store_build_pass", "silo_gpu_store_build_mode", "silo_gpu_store_memory_info", "silo_gpu_store_import_position", "silo_gpu_store_import_missing_rows",
    "silo_gpu_memset_async", "silo_gpu_event_create", "silo_gpu_event_record", "silo_gpu_event_elapsed_ms",
    "silo_gpu_event_destroy", "silo_gpu_event_synchronize", "silo_gpu_host_alloc", "silo_gpu_host_free", "silo_gpu_memcpy_d2h_async", "silo_gpu_mutations_select", "silo_gpu_upload_bytes", "silo_gpu_upload_column", "silo_gpu_bitset_from_compare", "silo_gpu_group_count", "silo_gpu_group_count_hashed", "silo_gpu_reconstruct_sequences", "silo_gpu_bitset_from_pairs", "silo_gpu_count_pairs", "silo_gpu_count_slot_create", "silo_gpu_count_slot_destroy", "silo_gpu_filter_eval_count", "silo_gpu_count_slot_wait", "silo_gpu_tune", "silo_gpu_last_scan_kernel", "silo_gpu_last_escape_items", "silo_gpu_scan_timings", "silo_gpu_stream_read_probe", "silo_gpu_last_error",
    "silo_gpu_comm_unique_id", "silo_gpu_comm_create", "silo_gpu_comm_destroy", "silo_gpu_comm_rank", "silo_gpu_comm_world",
    "silo_gpu_allreduce_counts", "silo_gpu_broadcast_bytes",
    "silo_gpu_mutations_scan_select",
    "silo_gpu_mutations_scan_ranges_min_proportion", "silo_gpu_store_scan_prunable_granules", "silo_gpu_store_scan_prunable_rows",
    "silo_gpu_store_scan_covered_rows", "silo_gpu_store_scan_end_events", "silo_gpu_store_scan_residual_keys",
    "silo_gpu_filters_grouped", "silo_gpu_filters_cross",
    "silo_gpu_distance_pack", "silo_gpu_distance_pairs", "silo_gpu_distance_within", "silo_gpu_adjacency_components",
    "silo_gpu_distance_weights", "silo_gpu_spanning_forest", "silo_gpu_distance_listed_pairs",
    "silo_gpu_distance_cross", "silo_gpu_nearest_columns",
    "silo_gpu_consensus_call",
    "silo_gpu_query_distances", "silo_gpu_nearest_rows", "silo_gpu_bitset_from_distances",
    "silo_gpu_position_symbols", "silo_gpu_haplotype_ids",
    "silo_gpu_mutations_compare",
    "silo_gpu_sequence_differences",
    "silo_gpu_sample_key", "silo_gpu_sample_groups", "silo_gpu_sample_begin", "silo_gpu_sample_count", "silo_gpu_sample_advance",
    "silo_gpu_sample_select",
    "silo_gpu_row_hash_term", "silo_gpu_row_hashes", "silo_gpu_store_row_hashes", "silo_gpu_distinct_begin", "silo_gpu_distinct_insert",
    "silo_gpu_distinct_select",
    "silo_gpu_distinct_count", "silo_gpu_distinct_classes", "silo_gpu_smallest_keys",
    "silo_gpu_row_cell_counts", "silo_gpu_store_row_cell_counts", "silo_gpu_bitset_from_cell_counts", "silo_gpu_cell_count_histogram",
    "silo_gpu_region_cell_values", "silo_gpu_bitset_from_values", "silo_gpu_count_values",
    "silo_gpu_table_pair_sums",
]

_lib = None


def load_library():
    """Loads lib/libsilo_gpu.so; raises loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The product path has no CPU fallback."
        )
    lib = ctypes.CDLL(_LIB_PATH)
    vp = ctypes.c_void_p
    lib.silo_gpu_store_create.argtypes = [ctypes.POINTER(StoreDesc), ctypes.POINTER(vp)]
    lib.silo_gpu_store_destroy.argtypes = [vp]
    lib.silo_gpu_store_destroy.restype = None
    lib.silo_gpu_store_sequence_count.argtypes = [vp]
    lib.silo_gpu_store_sequence_count.restype = ctypes.c_uint32
    lib.silo_gpu_store_row_words.argtypes = [vp]
    lib.silo_gpu_store_row_words.restype = ctypes.c_uint32
    lib.silo_gpu_store_device_bytes.argtypes = [vp]
    lib.silo_gpu_store_device_bytes.restype = ctypes.c_uint64
    lib.silo_gpu_store_append_sequences.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_store_finalize.argtypes = [vp]
    lib.silo_gpu_store_generate_synthetic.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(SynthDesc)]
    lib.silo_gpu_bitset_alloc.argtypes = [vp, ctypes.POINTER(vp)]
    lib.silo_gpu_bitset_upload.argtypes = [vp, vp, vp, ctypes.c_size_t, vp]
    lib.silo_gpu_bitset_download.argtypes = [vp, vp, vp, ctypes.c_size_t, vp]
    lib.silo_gpu_bitset_from_lineages.argtypes = [vp, vp, vp, ctypes.c_uint32, vp]
    lib.silo_gpu_free.argtypes = [vp]
    lib.silo_gpu_free.restype = None
    lib.silo_gpu_malloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.silo_gpu_memcpy_d2h.argtypes = [vp, vp, ctypes.c_size_t, vp]
    lib.silo_gpu_memcpy_h2d.argtypes = [vp, vp, ctypes.c_size_t, vp]
    lib.silo_gpu_upload_u32.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.silo_gpu_bitset_from_value_ids.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, vp]
    lib.silo_gpu_stream_synchronize.argtypes = [vp]
    lib.silo_gpu_stream_create.argtypes = [ctypes.POINTER(vp)]
    lib.silo_gpu_stream_destroy.argtypes = [vp]
    lib.silo_gpu_stream_destroy.restype = None
    lib.silo_gpu_store_plane.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    lib.silo_gpu_store_plane.restype = vp
    lib.silo_gpu_store_sparse_plane.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_filter_eval.argtypes = [vp, ctypes.POINTER(BitProg), vp, vp, vp]
    lib.silo_gpu_popcount.argtypes = [vp, vp, vp, vp]
    lib.silo_gpu_mutations_scan.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_mutations_scan_batch.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(vp), vp]
    lib.silo_gpu_store_scan_planes.argtypes = [vp, ctypes.c_uint32]
    lib.silo_gpu_store_scan_planes.restype = ctypes.c_uint32
    lib.silo_gpu_store_scan_escapes.argtypes = [vp, ctypes.c_uint32]
    lib.silo_gpu_store_scan_escapes.restype = ctypes.c_uint64
    lib.silo_gpu_store_scan_overflow_keys.argtypes = [vp, ctypes.c_uint32]
    lib.silo_gpu_store_scan_overflow_keys.restype = ctypes.c_uint64
    lib.silo_gpu_mutations_scan_ranges.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(vp), ctypes.c_uint32, ctypes.POINTER(vp), vp]
    lib.silo_gpu_mutations_scan_ranges_min_proportion.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(vp), ctypes.c_uint32,
                                                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(vp), vp]
    lib.silo_gpu_mutations_scan_select.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(vp), ctypes.c_uint32,
                                                   ctypes.POINTER(ctypes.c_double), ctypes.POINTER(vp), ctypes.POINTER(SelectSink), vp]
    lib.silo_gpu_store_scan_prunable_granules.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, ctypes.POINTER(ctypes.c_uint64),
                                                          ctypes.POINTER(ctypes.c_uint64)]
    lib.silo_gpu_store_scan_prunable_rows.argtypes = lib.silo_gpu_store_scan_prunable_granules.argtypes
    for name in ("silo_gpu_store_scan_covered_rows", "silo_gpu_store_scan_end_events", "silo_gpu_store_scan_residual_keys"):
        getattr(lib, name).argtypes = [vp, ctypes.c_uint32]
        getattr(lib, name).restype = ctypes.c_uint64
    lib.silo_gpu_mutations_grouped.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_filters_grouped.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_filters_cross.argtypes = [vp, vp, ctypes.POINTER(vp), vp, ctypes.c_uint32, ctypes.POINTER(vp), vp, ctypes.c_uint32, vp, vp,
                                           ctypes.c_uint32, ctypes.c_uint32, vp]
    lib.silo_gpu_distance_pack.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_distance_pairs.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_distance_within.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_adjacency_components.argtypes = [vp, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_distance_weights.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_spanning_forest.argtypes = [vp, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_distance_listed_pairs.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_distance_cross.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint32,
                                            ctypes.c_uint32, vp, vp]
    lib.silo_gpu_nearest_columns.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_consensus_call.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_double, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_query_distances.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
    lib.silo_gpu_nearest_rows.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp]
    lib.silo_gpu_bitset_from_distances.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_position_symbols.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_haplotype_ids.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp,
                                           ctypes.POINTER(vp), vp, vp]
    lib.silo_gpu_mutations_compare.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_double, ctypes.c_double,
                                               ctypes.c_uint32, vp, vp]
    lib.silo_gpu_sequence_differences.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
    lib.silo_gpu_sample_key.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    lib.silo_gpu_sample_key.restype = ctypes.c_uint32
    lib.silo_gpu_sample_groups.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_sample_begin.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, vp]
    lib.silo_gpu_sample_count.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp]
    lib.silo_gpu_sample_advance.argtypes = [vp, ctypes.c_uint32, vp]
    lib.silo_gpu_sample_select.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_row_hash_term.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    lib.silo_gpu_row_hash_term.restype = ctypes.c_uint64
    lib.silo_gpu_row_hashes.argtypes = [vp, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_store_row_hashes.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(vp), vp]
    lib.silo_gpu_distinct_begin.argtypes = [vp, ctypes.c_uint32, vp]
    lib.silo_gpu_distinct_insert.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_distinct_select.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_distinct_count.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_distinct_classes.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint32, vp, ctypes.c_uint32,
                                              vp, vp]
    lib.silo_gpu_smallest_keys.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp]
    lib.silo_gpu_row_cell_counts.argtypes = [vp, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_store_row_cell_counts.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(vp), vp]
    lib.silo_gpu_bitset_from_cell_counts.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_cell_count_histogram.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_region_cell_values.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
    lib.silo_gpu_bitset_from_values.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_count_values.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp]
    lib.silo_gpu_table_pair_sums.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_memset_async.argtypes = [vp, ctypes.c_int, ctypes.c_size_t, vp]
    lib.silo_gpu_upload_column.argtypes = [vp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(vp)]
    lib.silo_gpu_bitset_from_compare.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.silo_gpu_group_count.argtypes = [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, vp, vp]
    lib.silo_gpu_mutations_select.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_upload_bytes.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.silo_gpu_count_slot_create.argtypes = [ctypes.POINTER(vp)]
    lib.silo_gpu_count_slot_destroy.argtypes = [vp]
    lib.silo_gpu_count_slot_destroy.restype = None
    lib.silo_gpu_filter_eval_count.argtypes = [vp, ctypes.POINTER(BitProg), vp, vp, vp]
    lib.silo_gpu_count_slot_wait.argtypes = [vp, c_u64p, vp]
    lib.silo_gpu_row_slot_create.argtypes = [ctypes.c_uint32, ctypes.POINTER(vp)]
    lib.silo_gpu_row_slot_destroy.argtypes = [vp]
    lib.silo_gpu_row_slot_destroy.restype = None
    lib.silo_gpu_mutations_select_to_slot.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, vp, vp]
    lib.silo_gpu_row_slot_wait.argtypes = [vp, ctypes.POINTER(vp), c_u32p, vp]
    lib.silo_gpu_bitset_from_pairs.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp]
    lib.silo_gpu_count_pairs.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_group_count_hashed.argtypes = [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint32), vp]
    lib.silo_gpu_reconstruct_sequences.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp]
    lib.silo_gpu_event_create.argtypes = [ctypes.POINTER(vp)]
    lib.silo_gpu_event_record.argtypes = [vp, vp]
    lib.silo_gpu_event_elapsed_ms.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float)]
    lib.silo_gpu_event_destroy.argtypes = [vp]
    lib.silo_gpu_event_destroy.restype = None
    lib.silo_gpu_tune.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.silo_gpu_last_scan_kernel.restype = ctypes.c_char_p
    lib.silo_gpu_last_escape_items.argtypes = []
    lib.silo_gpu_last_escape_items.restype = ctypes.c_uint32
    lib.silo_gpu_store_build_pass.argtypes = [vp, ctypes.c_uint32, ctypes.c_int]
    lib.silo_gpu_store_build_pass.restype = ctypes.c_int
    lib.silo_gpu_store_build_mode.argtypes = [vp, ctypes.c_uint32]
    lib.silo_gpu_store_build_mode.restype = ctypes.c_int
    lib.silo_gpu_scan_timings.argtypes = [ctypes.POINTER(ScanTiming), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.silo_gpu_scan_timings.restype = ctypes.c_int
    lib.silo_gpu_last_error.restype = ctypes.c_char_p
    lib.silo_gpu_stream_read_probe.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)]
    lib.silo_gpu_stream_read_probe.restype = ctypes.c_int
    lib.silo_gpu_store_scan_rows.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    lib.silo_gpu_store_scan_rows.restype = ctypes.c_uint64
    for name in ("silo_gpu_store_scan_runs", "silo_gpu_store_scan_sparse_keys"):
        getattr(lib, name).argtypes = [vp, ctypes.c_uint32]
        getattr(lib, name).restype = ctypes.c_uint64
    lib.silo_gpu_store_finalize_seqstore.argtypes = [vp, ctypes.c_uint32]
    lib.silo_gpu_store_import_position.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(RoaringPayload), ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_uint32]
    lib.silo_gpu_store_import_missing_rows.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(RoaringPayload)]
    lib.silo_gpu_filter_eval_batch.argtypes = [vp, ctypes.POINTER(BitProg), ctypes.c_uint32, ctypes.POINTER(vp), c_u64p, vp]
    lib.silo_gpu_comm_unique_id.argtypes = [vp]
    lib.silo_gpu_comm_create.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(vp)]
    lib.silo_gpu_comm_destroy.argtypes = [vp]
    lib.silo_gpu_comm_destroy.restype = None
    lib.silo_gpu_comm_rank.argtypes = [vp]
    lib.silo_gpu_comm_rank.restype = ctypes.c_uint32
    lib.silo_gpu_comm_world.argtypes = [vp]
    lib.silo_gpu_comm_world.restype = ctypes.c_uint32
    lib.silo_gpu_allreduce_counts.argtypes = [vp, vp, ctypes.c_size_t, vp]
    lib.silo_gpu_broadcast_bytes.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_uint32, vp]
    _lib = lib
    return lib


COMM_ID_BYTES = 128


def comm_unique_id():
    """The opaque id one rank creates and hands to the others out of band (silo_gpu_comm_unique_id)."""
    buffer = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _check(load_library().silo_gpu_comm_unique_id(buffer))
    return bytes(buffer)


class Comm:
    """silo_gpu_comm: the native RCCL communicator behind silo_gpu_allreduce_counts / silo_gpu_broadcast_bytes."""

    def __init__(self, unique_id, rank, world, device=0):
        self.lib = load_library()
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("a communicator id has %d bytes" % COMM_ID_BYTES)
        handle = ctypes.c_void_p()
        _check(self.lib.silo_gpu_comm_create((ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id), rank, world, device, ctypes.byref(handle)))
        self.handle = handle
        self.rank, self.world = rank, world

    def all_reduce_counts(self, device_ptr, n, stream=None):
        _check(self.lib.silo_gpu_allreduce_counts(self.handle, device_ptr, n, stream))

    def broadcast_bytes(self, device_ptr, nbytes, root, stream=None):
        _check(self.lib.silo_gpu_broadcast_bytes(self.handle, device_ptr, nbytes, root, stream))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.silo_gpu_comm_destroy(self.handle)
            self.handle = None


def _check(rc):
    if rc != 0:
        raise SiloGpuError(rc, load_library().silo_gpu_last_error().decode())


def _ptr(array):
    return array.ctypes.data_as(ctypes.c_void_p)


class GpuEvent:
    """hipEvent on a caller-chosen stream (None = the null stream)."""

    def __init__(self):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        _check(self.lib.silo_gpu_event_create(ctypes.byref(self.handle)))

    def record(self, stream=None):
        _check(self.lib.silo_gpu_event_record(self.handle, stream))

    def elapsed_ms(self, stop):
        ms = ctypes.c_float()
        _check(self.lib.silo_gpu_event_elapsed_ms(self.handle, stop.handle, ctypes.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.silo_gpu_event_destroy(self.handle)
            self.handle = None


class GpuStream:
    """A non-blocking HIP stream (silo_gpu_stream_create); pass `.handle` wherever a stream is taken."""

    def __init__(self):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        _check(self.lib.silo_gpu_stream_create(ctypes.byref(self.handle)))

    def synchronize(self):
        _check(self.lib.silo_gpu_stream_synchronize(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.silo_gpu_stream_destroy(self.handle)
            self.handle = None


class CountSlot:
    """silo_gpu_count_slot: where the blocks of GpuStore.filter_eval_count deliver their parts of the cardinality (page-locked
    host memory); one slot serves one launch at a time."""

    def __init__(self):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        _check(self.lib.silo_gpu_count_slot_create(ctypes.byref(self.handle)))

    def wait(self, stream=None):
        """The cardinality of the slot's last launch (`stream`: the one it was launched on)."""
        count = ctypes.c_uint64()
        _check(self.lib.silo_gpu_count_slot_wait(self.handle, ctypes.byref(count), stream))
        return int(count.value)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.silo_gpu_count_slot_destroy(self.handle)
            self.handle = None


class SelectSink(ctypes.Structure):
    """silo_gpu_select_sink: where silo_gpu_mutations_scan_select leaves one filter's table and rows."""
    _fields_ = [("table_dev", ctypes.c_void_p), ("total_positions", ctypes.c_uint32), ("n_symbols", ctypes.c_uint32),
                ("reference_index_dev", ctypes.c_void_p), ("slot", ctypes.c_void_p)]


class RowSlot:
    """silo_gpu_row_slot: a page-locked host buffer of `capacity` rows that GpuStore.mutations_select_to_slot writes into."""

    def __init__(self, capacity):
        self.lib = load_library()
        self.capacity = int(capacity)
        self.handle = ctypes.c_void_p()
        _check(self.lib.silo_gpu_row_slot_create(self.capacity, ctypes.byref(self.handle)))

    def wait(self, stream=None):
        """(n_selected, a copy of rows[min(n, capacity)] as (position, symbol, count, total)) of the slot's last launch."""
        rows, n = ctypes.c_void_p(), ctypes.c_uint32()
        _check(self.lib.silo_gpu_row_slot_wait(self.handle, ctypes.byref(rows), ctypes.byref(n), stream))
        delivered = min(n.value, self.capacity)
        table = np.frombuffer(ctypes.string_at(rows.value, 16 * delivered), dtype=np.uint32).reshape(-1, 4)
        return int(n.value), table

    def close(self):
        if getattr(self, "handle", None):
            self.lib.silo_gpu_row_slot_destroy(self.handle)
            self.handle = None


# bit-program opcodes (include/silo_gpu.h)
(OP_LOAD, OP_ZERO, OP_ONES, OP_NOT, OP_AND, OP_OR, OP_ANDNOT, OP_CNT_ADD, OP_CNT_GE, OP_CNT_EQ, OP_MOV,
 OP_OR_N, OP_AND_N, OP_CNT_ADD_N, OP_CNT_ADD_NOT_N) = range(15)


COUNT_SHARDS = 64   # SILO_GPU_COUNT_SHARDS
LEAF_OPERAND = 32   # SILO_GPU_LEAF_OPERAND


def encode(op, dst=0, a=0, b=0, imm=0):
    return [op | (dst << 8) | (a << 16) | (b << 24), imm]


class PreparedPrograms:
    """A batch of bit-programs marshalled once (ctypes arrays), so that repeated launches cost no Python work."""

    def __init__(self, programs, out_bitsets=None):
        self.n = len(programs)
        self.array = (BitProg * max(1, self.n))()
        self._keep = []
        for k, (code, leaves, n_slots) in enumerate(programs):
            code = np.ascontiguousarray(code, dtype=np.uint32)
            leaf_array = (ctypes.c_void_p * max(1, len(leaves)))(*[(l.value if isinstance(l, ctypes.c_void_p) else l) for l in leaves])
            self._keep += [code, leaf_array]
            self.array[k] = BitProg(len(code) // 2, code.ctypes.data_as(c_u32p), len(leaves), leaf_array, n_slots)
        self.outs = None
        if out_bitsets is not None:
            self.outs = (ctypes.c_void_p * max(1, self.n))(*[(o.value if isinstance(o, ctypes.c_void_p) else o) for o in out_bitsets])
        self.counts = np.zeros(max(1, self.n), dtype=np.uint64)

    def launch(self, store_handle, stream=None):
        _check(load_library().silo_gpu_filter_eval_batch(store_handle, self.array, self.n, self.outs, self.counts.ctypes.data_as(c_u64p), stream))
        return [int(c) for c in self.counts[:self.n]]


SYMBOL_NONE = 0xFF


def import_position(store_handle, seqstore_id, position, payloads, flipped=None, deleted=None):
    """silo_gpu_store_import_position: payloads = {symbol id: portable-format roaring bytes} of one reference Position."""
    items = sorted(payloads.items())
    array = (RoaringPayload * max(1, len(items)))(*[RoaringPayload(symbol, data, len(data)) for symbol, data in items])
    _check(load_library().silo_gpu_store_import_position(
        store_handle, seqstore_id, position, array, len(items), SYMBOL_NONE if flipped is None else flipped, SYMBOL_NONE if deleted is None else deleted))


def import_missing_rows(store_handle, seqstore_id, first_sequence, payloads):
    """silo_gpu_store_import_missing_rows: payloads[r] = portable-format roaring bytes of the POSITIONS where row first_sequence + r is missing."""
    array = (RoaringPayload * max(1, len(payloads)))(*[RoaringPayload(0, data, len(data)) for data in payloads])
    _check(load_library().silo_gpu_store_import_missing_rows(store_handle, seqstore_id, first_sequence, len(payloads), array))


def filter_eval_batch(store_handle, programs, out_bitsets=None, stream=None):
    """silo_gpu_filter_eval_batch on a raw store handle.  programs: list of (code, leaves, n_slots) with code a flat list of
    uint32 (2 per instruction) and leaves device pointers; returns the cardinalities (one launch for all of them)."""
    return PreparedPrograms(programs, out_bitsets).launch(store_handle, stream)


MAX_DATE_RANGES = 1024         # SILO_GPU_MAX_DATE_RANGES
MAX_GROUPED_MUTATIONS = 4096   # SILO_GPU_MAX_GROUPED_MUTATIONS
MAX_GROUPED_FILTERS = 2048     # SILO_GPU_MAX_GROUPED_FILTERS
MAX_CROSS_FILTERS = 1024      # SILO_GPU_MAX_CROSS_FILTERS, per side
CROSS_TILE = 8                 # SILO_GPU_CROSS_TILE: filters per side that a block of K9 counts
CROSS_CHUNK_WORDS = 1024       # SILO_GPU_CROSS_CHUNK_WORDS: row words that a block of K9 covers
_OWN_SCRATCH = object()


def grouped_scratch_bytes(row_words, n_ranges, n_mutations):
    """SILO_GPU_GROUPED_SCRATCH_BYTES: the scratch silo_gpu_mutations_grouped needs."""
    return row_words * 128 + n_mutations * 32 + n_ranges * 16 + n_ranges * 4 * (1 + 3 * n_mutations) + 1024


def filters_grouped_scratch_bytes(row_words, n_ranges, n_filters):
    """SILO_GPU_FILTERS_GROUPED_SCRATCH_BYTES: the scratch silo_gpu_filters_grouped needs."""
    return row_words * 128 + n_filters * 8 + n_ranges * 16 + 1024


def filters_cross_scratch_bytes(n_rows, n_cols):
    """SILO_GPU_FILTERS_CROSS_SCRATCH_BYTES: the scratch silo_gpu_filters_cross needs."""
    return (n_rows + n_cols) * 16 + 1024


MAX_DISTANCE_ROWS = 2048       # SILO_GPU_MAX_DISTANCE_ROWS
DISTANCE_TILE = 16             # SILO_GPU_DISTANCE_TILE: rows per side of the pair tile that a block of K10 owns
DISTANCE_CHUNK_WORDS = 32      # SILO_GPU_DISTANCE_CHUNK_WORDS: words of every plane of a row that a block of K10 stages at a time


def _abi_alphabet(name_or_id):
    return alphabet.ALPHABETS[name_or_id].abi_id if isinstance(name_or_id, str) else int(name_or_id)


def distance_planes(alphabet_id):
    """SILO_GPU_DISTANCE_PLANES: the valid plane and the code bits (nucleotide 1 + 3, amino acid 1 + 5)."""
    return 6 if _abi_alphabet(alphabet_id) == 1 else 4


def distance_words(positions):
    """SILO_GPU_DISTANCE_WORDS: 64-bit words per plane of a row."""
    return (positions + 63) // 64


def device_malloc(nbytes, fill=None, stream=None):
    """A device allocation that belongs to no store (free with device_free); fill: the byte every byte of it is set to."""
    lib = load_library()
    ptr = ctypes.c_void_p()
    _check(lib.silo_gpu_malloc(max(1, nbytes), ctypes.byref(ptr)))
    if fill is not None and nbytes:
        _check(lib.silo_gpu_memset_async(ptr, fill, nbytes, stream))
    return ptr


def device_free(ptr):
    load_library().silo_gpu_free(ptr)


def device_read(ptr, dtype, count, stream=None):
    out = np.empty(count, dtype=dtype)
    if count:
        _check(load_library().silo_gpu_memcpy_d2h(_ptr(out), ptr, out.nbytes, stream))
    return out


def distance_pack(alphabet_id, chars, fill=None, stream=None):
    """silo_gpu_distance_pack (K10): chars uint8 [n][P] -> a device pointer to the planes uint64 [n][PLANES][WORDS] (free with
    device_free, read with device_read).  alphabet_id: 'nuc' / 'aa' or the id of the C ABI.  fill: the byte the plane buffer is
    filled with before the launch, so a test can see that every word is written."""
    lib = load_library()
    chars = np.ascontiguousarray(chars, dtype=np.uint8)
    n_rows, positions = chars.shape
    abi = _abi_alphabet(alphabet_id)
    planes = device_malloc(n_rows * distance_planes(abi) * distance_words(positions) * 8, fill, stream)
    chars_dev = device_malloc(chars.size)
    try:
        if chars.size:
            _check(lib.silo_gpu_memcpy_h2d(chars_dev, _ptr(chars), chars.size, stream))
        _check(lib.silo_gpu_distance_pack(abi, chars_dev, n_rows, positions, planes, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
    except Exception:
        device_free(planes)
        raise
    finally:
        device_free(chars_dev)
    return planes


def distance_pairs(alphabet_id, planes_ptr, n_rows, positions, fill=None, stream=None):
    """silo_gpu_distance_pairs (K10) over planes as distance_pack leaves them: uint32 [n][n][2], cell (i, j) = (differing,
    compared) for i <= j.  Cells with i > j are not written: they hold the byte `fill` repeated (the output is filled with it
    before the launch), or whatever the allocation held."""
    lib = load_library()
    cells = n_rows * n_rows * 2
    out = device_malloc(cells * 4, fill, stream)
    try:
        _check(lib.silo_gpu_distance_pairs(_abi_alphabet(alphabet_id), planes_ptr, n_rows, positions, out, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint32, cells, stream).reshape(n_rows, n_rows, 2)
    finally:
        device_free(out)


MAX_CLUSTER_ROWS = 8192        # SILO_GPU_MAX_CLUSTER_ROWS
WITHIN_TILE_ROWS = 16          # SILO_GPU_WITHIN_TILE_ROWS: rows of the pair tile that a block of K12 owns
WITHIN_TILE_COLS = 64          # SILO_GPU_WITHIN_TILE_COLS: its columns, one adjacency word
WITHIN_CHUNK_WORDS = 16        # SILO_GPU_WITHIN_CHUNK_WORDS: words of every plane of a row that a block of K12 stages at a time
COMPONENTS_THREADS = 1024      # SILO_GPU_COMPONENTS_THREADS: the one block of silo_gpu_adjacency_components


def adjacency_words(n_rows):
    """SILO_GPU_ADJACENCY_WORDS: 64-bit words per row of the bit matrix of K12."""
    return (n_rows + 63) // 64


def distance_pack_rows(alphabet_id, chars, fill=None, stream=None):
    """distance_pack for any number of rows: silo_gpu_distance_pack in batches of at most MAX_DISTANCE_ROWS rows into the rows of
    ONE plane buffer uint64 [n][PLANES][WORDS], as the Clusters action packs (free with device_free)."""
    lib = load_library()
    chars = np.ascontiguousarray(chars, dtype=np.uint8)
    n_rows, positions = chars.shape
    abi = _abi_alphabet(alphabet_id)
    row_bytes = distance_planes(abi) * distance_words(positions) * 8
    planes = device_malloc(n_rows * row_bytes, fill, stream)
    chars_dev = device_malloc(min(n_rows, MAX_DISTANCE_ROWS) * positions)
    try:
        for begin in range(0, n_rows, MAX_DISTANCE_ROWS):
            batch = chars[begin:begin + MAX_DISTANCE_ROWS]
            if batch.size:
                _check(lib.silo_gpu_memcpy_h2d(chars_dev, _ptr(batch), batch.size, stream))
            _check(lib.silo_gpu_distance_pack(abi, chars_dev, len(batch), positions, ctypes.c_void_p(planes.value + begin * row_bytes), stream))
            _check(lib.silo_gpu_stream_synchronize(stream))  # the next batch overwrites the characters
    except Exception:
        device_free(planes)
        raise
    finally:
        device_free(chars_dev)
    return planes


def distance_within(alphabet_id, planes_ptr, n_rows, positions, max_distance, min_compared, fill=None, guard_words=0, stream=None):
    """silo_gpu_distance_within (K12) over planes as distance_pack / distance_pack_rows leave them: the n_rows * adjacency_words(n_rows)
    words of the bit matrix, bit (i, j) = i != j and differing <= max_distance and compared >= min_compared, followed by
    `guard_words` words behind them that the call must not touch: those hold the byte `fill` repeated (the whole allocation is
    filled with it before the launch), or whatever the allocation held."""
    lib = load_library()
    words = n_rows * adjacency_words(n_rows) + int(guard_words)
    out = device_malloc(words * 8, fill, stream)
    try:
        _check(lib.silo_gpu_distance_within(_abi_alphabet(alphabet_id), planes_ptr, n_rows, positions, max_distance, min_compared, out, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint64, words, stream)
    finally:
        device_free(out)


def adjacency_components(adjacency, n_rows, fill=None, stream=None):
    """silo_gpu_adjacency_components (K12) over a host bit matrix uint64 [n_rows * adjacency_words(n_rows)] as
    silo_gpu_distance_within leaves it: (labels uint32 [n_rows], rounds) — labels[i] the lowest row of i's component.  The labels
    and the round count are filled with the byte `fill` before the launch."""
    lib = load_library()
    adjacency = np.ascontiguousarray(adjacency, dtype=np.uint64).reshape(-1)
    adjacency_dev = device_malloc(adjacency.nbytes)
    labels = device_malloc(n_rows * 4, fill, stream)
    rounds = device_malloc(4, fill, stream)
    try:
        if adjacency.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(adjacency_dev, _ptr(adjacency), adjacency.nbytes, stream))
        _check(lib.silo_gpu_adjacency_components(adjacency_dev, n_rows, labels, rounds, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(labels, np.uint32, n_rows, stream), int(device_read(rounds, np.uint32, 1, stream)[0])
    finally:
        for ptr in (adjacency_dev, labels, rounds):
            device_free(ptr)


MAX_SPANNING_ROWS = 8192       # SILO_GPU_MAX_SPANNING_ROWS
SPANNING_THREADS = 1024        # SILO_GPU_SPANNING_THREADS: the one block of silo_gpu_spanning_forest
SPANNING_KEY_ROW_BITS = 13     # SILO_GPU_SPANNING_KEY_ROW_BITS: a row of an edge's key
SPANNING_KEY_WEIGHT_SHIFT = 26  # SILO_GPU_SPANNING_KEY_WEIGHT_SHIFT: the weight lies above the two rows
NO_EDGE = 0xFFFFFFFF           # a cell of the matrix of K13 that is no edge; as max_distance: no bound


def spanning_key(weight, i, j):
    """SILO_GPU_SPANNING_KEY: weight << 26 | i << 13 | j for the edge i < j."""
    return (int(weight) << SPANNING_KEY_WEIGHT_SHIFT) | (int(i) << SPANNING_KEY_ROW_BITS) | int(j)


def spanning_key_fields(keys):
    """(weight, i, j) of keys as silo_gpu_spanning_forest writes them (uint64 arrays in, uint64 arrays out)."""
    keys = np.asarray(keys, dtype=np.uint64)
    row_mask = np.uint64(MAX_SPANNING_ROWS - 1)
    return keys >> np.uint64(SPANNING_KEY_WEIGHT_SHIFT), (keys >> np.uint64(SPANNING_KEY_ROW_BITS)) & row_mask, keys & row_mask


def distance_weights(alphabet_id, planes_ptr, n_rows, positions, max_distance, min_compared, fill=None, guard_words=0, stream=None):
    """silo_gpu_distance_weights (K13) over planes as distance_pack / distance_pack_rows leave them: the n_rows * n_rows cells uint32
    of the matrix, cell (i, j) = differing where i != j and differing <= max_distance and compared >= min_compared, NO_EDGE
    elsewhere, followed by `guard_words` uint32 behind them that the call must not touch: those hold the byte `fill` repeated (the
    whole allocation is filled with it before the launch), or whatever the allocation held."""
    lib = load_library()
    cells = n_rows * n_rows + int(guard_words)
    out = device_malloc(cells * 4, fill, stream)
    try:
        _check(lib.silo_gpu_distance_weights(_abi_alphabet(alphabet_id), planes_ptr, n_rows, positions, max_distance, min_compared, out, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint32, cells, stream)
    finally:
        device_free(out)


def spanning_forest(weights, n_rows, fill=None, guard_words=0, stream=None):
    """silo_gpu_spanning_forest (K13) over a host matrix uint32 [n_rows * n_rows] as silo_gpu_distance_weights leaves it: (edges
    uint64 [max(n_rows - 1, 0) + guard_words], count uint32 [1]) — edges[:count] the keys of the forest, ascending; the entries at or
    past the count, and the count where nothing is written, hold the byte `fill` repeated (both are filled with it before the
    launch)."""
    lib = load_library()
    weights = np.ascontiguousarray(weights, dtype=np.uint32).reshape(-1)
    slots = max(n_rows - 1, 0) + int(guard_words)
    weights_dev = device_malloc(weights.nbytes)
    edges = device_malloc(slots * 8, fill, stream)
    count = device_malloc(4, fill, stream)
    try:
        if weights.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(weights_dev, _ptr(weights), weights.nbytes, stream))
        _check(lib.silo_gpu_spanning_forest(weights_dev, n_rows, edges, count, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(edges, np.uint64, slots, stream), device_read(count, np.uint32, 1, stream)
    finally:
        for ptr in (weights_dev, edges, count):
            device_free(ptr)


def distance_listed_pairs(alphabet_id, planes_ptr, n_rows, positions, edges, count, max_pairs, fill=None, guard_words=0, stream=None):
    """silo_gpu_distance_listed_pairs (K13) over planes as distance_pack / distance_pack_rows leave them, for the host keys `edges`
    uint64 and the count `count`: uint32 [max_pairs + guard_words][2] — row e = (differing, compared) of the pair in the low 26 bits
    of edges[e], for e < min(count, max_pairs); the rows at or past that hold the byte `fill` repeated (the whole allocation is
    filled with it before the launch)."""
    lib = load_library()
    edges = np.ascontiguousarray(edges, dtype=np.uint64).reshape(-1)
    count = np.array([count], dtype=np.uint32)
    rows = int(max_pairs) + int(guard_words)
    edges_dev = device_malloc(edges.nbytes)
    count_dev = device_malloc(4)
    out = device_malloc(rows * 8, fill, stream)
    try:
        if edges.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(edges_dev, _ptr(edges), edges.nbytes, stream))
        _check(lib.silo_gpu_memcpy_h2d(count_dev, _ptr(count), 4, stream))
        _check(lib.silo_gpu_distance_listed_pairs(_abi_alphabet(alphabet_id), planes_ptr, n_rows, positions, edges_dev, count_dev, max_pairs, out, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint32, rows * 2, stream).reshape(rows, 2)
    finally:
        for ptr in (edges_dev, count_dev, out):
            device_free(ptr)


MAX_CROSS_ROWS = 2048          # SILO_GPU_MAX_CROSS_ROWS: the rows (subjects) of the rectangle of K14
MAX_CROSS_COLUMNS = 8192       # SILO_GPU_MAX_CROSS_COLUMNS: its columns (candidates)
MAX_NEIGHBOUR_COLUMNS = 64     # SILO_GPU_MAX_NEIGHBOUR_COLUMNS: k of silo_gpu_nearest_columns
NEIGHBOUR_THREADS = 1024       # SILO_GPU_NEIGHBOUR_THREADS: the block that owns a row in silo_gpu_nearest_columns
NEIGHBOUR_KEY_COLUMN_BITS = 13  # SILO_GPU_NEIGHBOUR_KEY_COLUMN_BITS: the column of a key, below the distance
NOT_ELIGIBLE = 0xFFFFFFFF      # both words of a cell of K14 that is not eligible; as a self column: none; as max_distance: no bound


def distance_cross(alphabet_id, row_planes_ptr, n_rows, column_planes_ptr, n_columns, positions, self_columns, max_distance, min_compared,
                   fill=None, guard_words=0, stream=None):
    """silo_gpu_distance_cross (K14) over two plane buffers as distance_pack / distance_pack_rows leave them: the n_rows * n_columns
    cells uint32 [2] of the rectangle, cell (i, j) = (differing, compared) where j != self_columns[i] and differing <= max_distance
    and compared >= min_compared, (NOT_ELIGIBLE, NOT_ELIGIBLE) elsewhere, followed by `guard_words` uint32 behind them that the call
    must not touch: those hold the byte `fill` repeated (the whole allocation is filled with it before the launch), or whatever the
    allocation held.  self_columns: None (NULL) or n_rows uint32."""
    lib = load_library()
    words = n_rows * n_columns * 2 + int(guard_words)
    out = device_malloc(words * 4, fill, stream)
    self_dev = None
    try:
        if self_columns is not None:
            self_columns = np.ascontiguousarray(self_columns, dtype=np.uint32).reshape(-1)
            self_dev = device_malloc(self_columns.nbytes)
            if self_columns.nbytes:
                _check(lib.silo_gpu_memcpy_h2d(self_dev, _ptr(self_columns), self_columns.nbytes, stream))
        _check(lib.silo_gpu_distance_cross(_abi_alphabet(alphabet_id), row_planes_ptr, n_rows, column_planes_ptr, n_columns, positions, self_dev,
                                           max_distance, min_compared, out, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint32, words, stream)
    finally:
        device_free(out)
        if self_dev is not None:
            device_free(self_dev)


def nearest_columns(cells, n_rows, n_columns, k, fill=None, guard_words=0, stream=None):
    """silo_gpu_nearest_columns (K14) over host cells uint32 [n_rows * n_columns * 2] as silo_gpu_distance_cross leaves them: (lists
    uint32 [n_rows * k * 3 + guard_words], counts uint32 [n_rows + guard_words]) — entry r < counts[i] of row i = (column, distance,
    compared), ascending by (distance, column); the entries at or past a row's count, the guard words and everything where nothing
    is written hold the byte `fill` repeated (both are filled with it before the launch)."""
    lib = load_library()
    cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1)
    list_words = n_rows * int(k) * 3 + int(guard_words)
    count_words = n_rows + int(guard_words)
    cells_dev = device_malloc(cells.nbytes)
    lists = device_malloc(list_words * 4, fill, stream)
    counts = device_malloc(count_words * 4, fill, stream)
    try:
        if cells.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(cells_dev, _ptr(cells), cells.nbytes, stream))
        _check(lib.silo_gpu_nearest_columns(cells_dev, n_rows, n_columns, k, lists, counts, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(lists, np.uint32, list_words, stream), device_read(counts, np.uint32, count_words, stream)
    finally:
        for ptr in (cells_dev, lists, counts):
            device_free(ptr)


MAX_CONSENSUS_TABLES = 64      # SILO_GPU_MAX_CONSENSUS_TABLES: the count tables (groups) of one silo_gpu_consensus_call
CONSENSUS_THREADS = 256        # SILO_GPU_CONSENSUS_THREADS: positions of one table that a block of K15 owns
CONSENSUS_SUMMARY_WORDS = 4    # per table: ambiguous, low-coverage and deleted positions, differences from the reference


def consensus_call(alphabet_id, counts, reference_index, threshold, min_depth, fill=None, guard_bytes=0, calls=1, null=(), stream=None):
    """silo_gpu_consensus_call (K15) over host counts uint32 [n_tables][n_positions][n_symbols] and reference_index uint8
    [n_positions]: (chars uint8 [n_tables * n_positions + guard_bytes], summary uint32 [n_tables * 4 + guard_bytes / 4], the status
    of the last call).  Both outputs are filled with the byte `fill` before the first of `calls` launches, so a test can see what
    is written, that nothing behind it is, and that a second call adds nothing.  A status other than 0 is returned, not raised:
    the refusals leave the outputs as they were.  null: which of "counts", "reference", "chars", "summary" the call gets as NULL."""
    lib = load_library()
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n_tables, n_positions = counts.shape[:2]
    reference_index = np.ascontiguousarray(reference_index, dtype=np.uint8)
    char_bytes = n_tables * n_positions + int(guard_bytes)
    summary_words = n_tables * CONSENSUS_SUMMARY_WORDS + int(guard_bytes) // 4
    counts_dev = device_malloc(counts.nbytes)
    reference_dev = device_malloc(reference_index.nbytes)
    chars = device_malloc(char_bytes, fill, stream)
    summary = device_malloc(summary_words * 4, fill, stream)
    try:
        if counts.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(counts_dev, _ptr(counts), counts.nbytes, stream))
        if reference_index.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(reference_dev, _ptr(reference_index), reference_index.nbytes, stream))
        status = 0
        for _ in range(calls):
            status = lib.silo_gpu_consensus_call(
                _abi_alphabet(alphabet_id), None if "counts" in null else counts_dev, n_tables, n_positions, None if "reference" in null else reference_dev,
                threshold, min_depth, None if "chars" in null else chars, None if "summary" in null else summary, stream)
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(chars, np.uint8, char_bytes, stream), device_read(summary, np.uint32, summary_words, stream), status
    finally:
        for ptr in (counts_dev, reference_dev, chars, summary):
            device_free(ptr)


MAX_COMPARISON_TABLES = 64     # SILO_GPU_MAX_COMPARISON_TABLES: the count tables (groups) of one silo_gpu_mutations_compare
COMPARE_THREADS = 256          # SILO_GPU_COMPARE_THREADS: the positions that a block of K17 owns
COMPARE_HEADER_WORDS = 4       # word 0: the selected cells; the others 0


def mutations_compare(alphabet_id, counts, reference_index, min_proportion, min_difference, capacity, fill=None, guard_bytes=0, calls=1, null=(),
                      n_tables=None, stream=None):
    """silo_gpu_mutations_compare (K17) over host counts uint32 [n_tables][n_positions][n_symbols] and reference_index uint8
    [n_positions]: (out uint32 [4 + capacity * 2 + capacity * n_tables * 2 + guard_bytes / 4], the status of the last call).  The
    output is filled with the byte `fill` before the first of `calls` launches, so a test can see what is written, that nothing
    behind it is, and that a second call adds nothing.  A status other than 0 is returned, not raised: the refusals leave the output
    as it was.  null: which of "counts", "reference", "out" the call gets as NULL.  n_tables: what the call is told instead of the
    number of tables there are (fewer, or a number the call refuses)."""
    lib = load_library()
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    tables, n_positions = counts.shape[:2]
    told = tables if n_tables is None else int(n_tables)
    reference_index = np.ascontiguousarray(reference_index, dtype=np.uint8)
    words = COMPARE_HEADER_WORDS + int(capacity) * 2 + int(capacity) * tables * 2 + int(guard_bytes) // 4
    counts_dev = device_malloc(counts.nbytes)
    reference_dev = device_malloc(reference_index.nbytes)
    out = device_malloc(words * 4, fill, stream)
    try:
        if counts.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(counts_dev, _ptr(counts), counts.nbytes, stream))
        if reference_index.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(reference_dev, _ptr(reference_index), reference_index.nbytes, stream))
        status = 0
        for _ in range(calls):
            status = lib.silo_gpu_mutations_compare(
                _abi_alphabet(alphabet_id), None if "counts" in null else counts_dev, told, n_positions, None if "reference" in null else reference_dev,
                min_proportion, min_difference, capacity, None if "out" in null else out, stream)
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint32, words, stream), status
    finally:
        for ptr in (counts_dev, reference_dev, out):
            device_free(ptr)


MAX_PAIR_SUM_TABLES = 64       # SILO_GPU_MAX_PAIR_SUM_TABLES: the count tables (groups) of one silo_gpu_table_pair_sums
MAX_PAIR_SUM_RANGES = 256      # SILO_GPU_MAX_PAIR_SUM_RANGES: its ranges of positions
PAIR_SUM_WORDS = 5             # SILO_GPU_PAIR_SUM_WORDS: uint64 words of a record: diff_lo, diff_hi, cmp_lo, cmp_hi, sites
PAIR_SUM_TILE = 16             # SILO_GPU_PAIR_SUM_TILE: a block of K24 owns a tile of 16 x 16 pairs of tables
PAIR_SUM_POSITION_TILE = 16    # SILO_GPU_PAIR_SUM_POSITION_TILE: the positions it stages through LDS at a time
PAIR_SUM_CHUNK = 128           # SILO_GPU_PAIR_SUM_CHUNK: the positions of a range that a block owns


def table_pair_sums(alphabet_id, counts, ranges, fill=None, guard_bytes=0, calls=1, null=(), n_tables=None, n_positions=None, n_ranges=None, stream=None):
    """silo_gpu_table_pair_sums (K24) over host counts uint32 [n_tables][n_positions][n_symbols] and ranges [n_ranges][2] (0-based
    first, end): (out uint64 [n_ranges * G (G + 1) / 2 * 5 + guard_bytes / 8], the status of the last call).  The output is filled
    with the byte `fill` before the first of `calls` launches, so a test can see what is written, that nothing behind it is, and that
    a second call gives the same bytes.  A status other than 0 is returned, not raised: the refusals leave the output as it was.
    null: which of "counts", "ranges", "out" the call gets as NULL.  n_tables / n_positions / n_ranges: what the call is told instead
    of what there is (fewer, or a number the call refuses)."""
    lib = load_library()
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    tables, positions = counts.shape[:2]
    ranges = np.ascontiguousarray(ranges, dtype=np.uint32).reshape(-1, 2)
    words = len(ranges) * (tables * (tables + 1) // 2) * PAIR_SUM_WORDS + int(guard_bytes) // 8
    counts_dev = device_malloc(max(counts.nbytes, 4))
    out = device_malloc(max(words, 1) * 8, fill, stream)
    try:
        if counts.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(counts_dev, _ptr(counts), counts.nbytes, stream))
        status = 0
        for _ in range(calls):
            status = lib.silo_gpu_table_pair_sums(
                _abi_alphabet(alphabet_id), None if "counts" in null else counts_dev, tables if n_tables is None else int(n_tables),
                positions if n_positions is None else int(n_positions), None if "ranges" in null or not len(ranges) else _ptr(ranges),
                len(ranges) if n_ranges is None else int(n_ranges), None if "out" in null else out, stream)
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint64, words, stream), status
    finally:
        for ptr in (counts_dev, out):
            device_free(ptr)


MAX_DIFFERENCE_ROWS = 10000            # SILO_GPU_MAX_DIFFERENCE_ROWS: the rows of one silo_gpu_sequence_differences
MAX_DIFFERENCE_POSITIONS = 1 << 23     # SILO_GPU_MAX_DIFFERENCE_POSITIONS: a position lies above the 9 low bits of a record word
DIFFERENCE_STATS = 4                   # SILO_GPU_DIFFERENCE_STATS: substitution, deleted, missing, ambiguous cells of a row
DIFFERENCE_CHUNK = 4096                # SILO_GPU_DIFFERENCE_CHUNK: bytes of a row per block of K18, 256 threads x 16 bytes


def difference_chunks(positions):
    """SILO_GPU_DIFFERENCE_CHUNKS: the most chunks a row can have (it starts up to 15 bytes past a 16-byte boundary)."""
    return (positions + 15 + DIFFERENCE_CHUNK - 1) // DIFFERENCE_CHUNK


def differences_scratch_bytes(n_rows, positions):
    """SILO_GPU_DIFFERENCES_SCRATCH_BYTES: per (row, chunk) the words and the four cell counts."""
    return n_rows * difference_chunks(positions) * (1 + DIFFERENCE_STATS) * 4


def sequence_differences(alphabet_id, chars, reference, capacity, fill=None, guard_bytes=0, calls=1, null=(), n_rows=None, positions=None,
                         chars_offset=0, stream=None):
    """silo_gpu_sequence_differences (K18) over host chars uint8 [n][P] and reference uint8 [P]: (offsets uint32 [n + 1 + guard],
    stats uint32 [n * 4 + guard], records uint32 [capacity + guard], the status of the last call), guard = guard_bytes / 4 words
    behind each.  The three outputs are filled with the byte `fill` before the first of `calls` launches, so a test can see what
    is written, that nothing behind it is, and that a second call gives the same bytes.  A status other than 0 is returned, not
    raised: the refusals leave the outputs as they were.  null: which of "chars", "reference", "offsets", "stats", "records",
    "scratch" the call gets as NULL.  n_rows / positions: what the call is told instead of the matrix's shape (a shape it
    refuses).  chars_offset: the bytes the first row starts past a 256-byte boundary."""
    lib = load_library()
    chars = np.ascontiguousarray(chars, dtype=np.uint8)
    rows, width = chars.shape
    reference = np.ascontiguousarray(reference, dtype=np.uint8)
    guard = int(guard_bytes) // 4
    offset_words, stat_words, record_words = rows + 1 + guard, rows * DIFFERENCE_STATS + guard, int(capacity) + guard
    chars_dev = device_malloc(chars.size + int(chars_offset))
    reference_dev = device_malloc(reference.size)
    offsets = device_malloc(offset_words * 4, fill, stream)
    stats = device_malloc(stat_words * 4, fill, stream)
    records = device_malloc(record_words * 4, fill, stream)
    scratch = device_malloc(differences_scratch_bytes(rows, width))
    try:
        chars_at = ctypes.c_void_p(chars_dev.value + int(chars_offset))
        if chars.size:
            _check(lib.silo_gpu_memcpy_h2d(chars_at, _ptr(chars), chars.size, stream))
        if reference.size:
            _check(lib.silo_gpu_memcpy_h2d(reference_dev, _ptr(reference), reference.size, stream))
        status = 0
        for _ in range(calls):
            status = lib.silo_gpu_sequence_differences(
                _abi_alphabet(alphabet_id), None if "chars" in null else chars_at, rows if n_rows is None else int(n_rows),
                width if positions is None else int(positions), None if "reference" in null else reference_dev, int(capacity),
                None if "offsets" in null else offsets, None if "stats" in null else stats, None if "records" in null else records,
                None if "scratch" in null else scratch, stream)
        _check(lib.silo_gpu_stream_synchronize(stream))
        return (device_read(offsets, np.uint32, offset_words, stream), device_read(stats, np.uint32, stat_words, stream),
                device_read(records, np.uint32, record_words, stream), status)
    finally:
        for ptr in (chars_dev, reference_dev, offsets, stats, records, scratch):
            device_free(ptr)


MAX_HAPLOTYPE_POSITIONS = 12         # SILO_GPU_MAX_HAPLOTYPE_POSITIONS: the positions of one silo_gpu_position_symbols / silo_gpu_haplotype_ids
HAPLOTYPE_POSITIONS_PER_COLUMN = 6    # SILO_GPU_HAPLOTYPE_POSITIONS_PER_COLUMN: 16^6 = 2^24, 25^6 < 2^28: an id column is a uint32
ALL_SYMBOLS_COMPLETE = 0xFFFFFFFF     # complete_symbols of silo_gpu_haplotype_ids: no row is left out


def haplotype_ids(symbols, sequence_count, n_symbols, complete_symbols=ALL_SYMBOLS_COMPLETE, filter_words=None, want_rows=True, fill=None,
                  guard_words=0, null=(), n_positions=None, row_words=None, stream=None):
    """silo_gpu_haplotype_ids (K16) over a host byte matrix uint8 [n_positions][row_words * 64] as silo_gpu_position_symbols leaves
    it; filter_words: uint64 [row_words], None = a null pointer (all rows).  Returns (ids uint32 [columns][row_words * 64 +
    guard_words], rows uint64 [row_words + guard_words] or None, status).  Every output is filled with the byte `fill` before the
    launch, so a test can see what is written and that nothing behind it is.  A status other than 0 is returned, not raised: the
    refusals leave the outputs as they were.  null: which of "symbols", "ids", "column" (the last id column) the call gets as
    NULL.  n_positions / row_words: what the call is told instead of the matrix's shape."""
    lib = load_library()
    symbols = np.ascontiguousarray(symbols, dtype=np.uint8)
    k, rows = symbols.shape
    words = rows // 64
    n_columns = (k + HAPLOTYPE_POSITIONS_PER_COLUMN - 1) // HAPLOTYPE_POSITIONS_PER_COLUMN
    column_words = rows + int(guard_words)
    symbols_dev = device_malloc(symbols.nbytes)
    columns = [device_malloc(column_words * 4, fill, stream) for _ in range(n_columns)]
    rows_dev = device_malloc((words + int(guard_words)) * 8, fill, stream) if want_rows else None
    filter_dev = None
    try:
        _check(lib.silo_gpu_memcpy_h2d(symbols_dev, _ptr(symbols), symbols.nbytes, stream))
        if filter_words is not None:
            filter_words = np.ascontiguousarray(filter_words, dtype=np.uint64)
            filter_dev = device_malloc(filter_words.nbytes)
            _check(lib.silo_gpu_memcpy_h2d(filter_dev, _ptr(filter_words), filter_words.nbytes, stream))
        pointers = (ctypes.c_void_p * max(1, n_columns))(*[c.value for c in columns])
        if "column" in null:
            pointers[n_columns - 1] = None
        status = lib.silo_gpu_haplotype_ids(
            None if "symbols" in null else symbols_dev, k if n_positions is None else n_positions, words if row_words is None else row_words,
            sequence_count, n_symbols, complete_symbols, filter_dev, None if "ids" in null else pointers, rows_dev, stream)
        _check(lib.silo_gpu_stream_synchronize(stream))
        ids = np.stack([device_read(c, np.uint32, column_words, stream) for c in columns])
        return ids, (device_read(rows_dev, np.uint64, words + int(guard_words), stream) if want_rows else None), status
    finally:
        for ptr in [symbols_dev, rows_dev, filter_dev, *columns]:
            if ptr is not None:
                device_free(ptr)


MAX_NEAREST_ROWS = 1024              # SILO_GPU_MAX_NEAREST_ROWS
NEAREST_ROWS_SCRATCH_BYTES = 32768   # SILO_GPU_NEAREST_ROWS_SCRATCH_BYTES
QUERY_DISTANCE_COUNTER_PLANES = 12   # SILO_GPU_QUERY_DISTANCE_COUNTER_PLANES: a vertical counter of K11 is unpacked after 2^12 - 1 adds
NO_ROW = 0xFFFFFFFF                  # exclude_row / max_distance of silo_gpu_nearest_rows: none


def query_distance_scratch_bytes(positions):
    """SILO_GPU_QUERY_DISTANCE_SCRATCH_BYTES: the scratch silo_gpu_query_distances needs."""
    return (positions // 256 + 1) * 256 + 2 * (((positions + 1) * 4) // 256 + 1) * 256


def nearest_rows_call(table_ptr, filter_ptr, sequence_count, exclude_row, max_distance, k, out_ptr, count_ptr, scratch_ptr, stream=None):
    """silo_gpu_nearest_rows (K11) on the caller's device buffers, waited for."""
    lib = load_library()
    _check(lib.silo_gpu_nearest_rows(table_ptr, filter_ptr, sequence_count, exclude_row, max_distance, k, out_ptr, count_ptr, scratch_ptr, stream))
    _check(lib.silo_gpu_stream_synchronize(stream))


def nearest_rows(table, filter_words, sequence_count, k, exclude_row=NO_ROW, max_distance=NO_ROW, fill=None, stream=None):
    """silo_gpu_nearest_rows (K11) over a host table uint32 [rows][2] (distance, compared) as silo_gpu_query_distances leaves it.
    filter_words: uint64 row bitset, None = all rows.  Returns (count, list): list uint32 [k][3] = row, distance, compared, of
    which the first `count` entries were written; the others hold the byte `fill` repeated (the list is filled with it before the
    launch), or whatever the allocation held."""
    lib = load_library()
    table = np.ascontiguousarray(table, dtype=np.uint32)
    k_cells = max(int(k), 1) * 3
    table_dev = device_malloc(table.nbytes)
    filter_dev = None
    out = device_malloc(k_cells * 4, fill, stream)
    count = device_malloc(4, fill, stream)
    scratch = device_malloc(NEAREST_ROWS_SCRATCH_BYTES, fill, stream)
    try:
        if table.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(table_dev, _ptr(table), table.nbytes, stream))
        if filter_words is not None:
            filter_words = np.ascontiguousarray(filter_words, dtype=np.uint64)
            filter_dev = device_malloc(filter_words.nbytes)
            _check(lib.silo_gpu_memcpy_h2d(filter_dev, _ptr(filter_words), filter_words.nbytes, stream))
        nearest_rows_call(table_dev, filter_dev, sequence_count, exclude_row, max_distance, k, out, count, scratch, stream)
        return int(device_read(count, np.uint32, 1, stream)[0]), device_read(out, np.uint32, k_cells, stream).reshape(-1, 3)
    finally:
        for ptr in (table_dev, filter_dev, out, count, scratch):
            if ptr is not None:
                device_free(ptr)


def bitset_from_distances_call(table_ptr, sequence_count, row_words, max_distance, min_compared, out_ptr, stream=None):
    """silo_gpu_bitset_from_distances (K11) on the caller's device buffers, waited for."""
    lib = load_library()
    _check(lib.silo_gpu_bitset_from_distances(table_ptr, sequence_count, row_words, max_distance, min_compared, out_ptr, stream))
    _check(lib.silo_gpu_stream_synchronize(stream))


def bitset_from_distances(table, sequence_count, row_words, max_distance=NO_ROW, min_compared=0, fill=None, stream=None, guard_words=0):
    """silo_gpu_bitset_from_distances (K11) over a host table uint32 [row_words * 64][2] (distance, compared) as
    silo_gpu_query_distances leaves it: bit r = r < sequence_count and distance <= max_distance and compared >= min_compared.
    Returns the row_words words the call writes, followed by `guard_words` words behind them that it must not touch: those hold
    the byte `fill` repeated (the whole allocation is filled with it before the launch), or whatever the allocation held."""
    lib = load_library()
    table = np.ascontiguousarray(table, dtype=np.uint32)
    words = int(row_words) + int(guard_words)
    table_dev = device_malloc(table.nbytes)
    out = device_malloc(words * 8, fill, stream)
    try:
        if table.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(table_dev, _ptr(table), table.nbytes, stream))
        bitset_from_distances_call(table_dev, sequence_count, row_words, max_distance, min_compared, out, stream)
        return device_read(out, np.uint64, words, stream)
    finally:
        device_free(table_dev)
        device_free(out)


MAX_SAMPLE_GROUPS = 1024   # SILO_GPU_MAX_SAMPLE_GROUPS
SAMPLE_LDS_GROUPS = 16     # SILO_GPU_SAMPLE_LDS_GROUPS: above, silo_gpu_sample_count adds to the table in global memory directly
SAMPLE_ROUNDS = 4          # SILO_GPU_SAMPLE_ROUNDS
NO_SAMPLE_GROUP = 0xFFFF   # a row of a group array that belongs to no group


def sample_state_bytes(n_groups):
    """SILO_GPU_SAMPLE_STATE_BYTES: the state of a selection over n_groups groups."""
    return 16 + int(n_groups) * (16 + 256 * 4)


def sample_key(seed, global_row):
    """silo_gpu_sample_key: the key of a row of the database under a seed (host function; the kernels compile the same code)."""
    return int(load_library().silo_gpu_sample_key(int(seed), int(global_row)))


def sample_state(words, n_groups):
    """The uint32 words of a K19 state as a dict: n_groups, size, k1, k2, and per group prefix, remaining, take_all (uint32
    [n_groups] each) and histogram uint32 [n_groups][256]."""
    words = np.asarray(words, dtype=np.uint32)
    groups = words[4:4 + 4 * n_groups].reshape(n_groups, 4)
    return {"n_groups": int(words[0]), "size": int(words[1]), "k1": int(words[2]), "k2": int(words[3]), "prefix": groups[:, 0].copy(),
            "remaining": groups[:, 1].copy(), "take_all": groups[:, 2].copy(),
            "histogram": words[4 + 4 * n_groups:4 + 4 * n_groups + 256 * n_groups].reshape(n_groups, 256).copy()}


def _upload(array, stream=None):
    """A device copy of a host array (free with device_free)."""
    ptr = device_malloc(array.nbytes)
    if array.nbytes:
        _check(load_library().silo_gpu_memcpy_h2d(ptr, _ptr(array), array.nbytes, stream))
    return ptr


def sample_groups(filter_words, dates, range_bounds, sequence_count, row_words, fill=None, guard_rows=0, stream=None):
    """silo_gpu_sample_groups (K19) over host arrays: filter_words uint64 [row_words], dates uint32 [>= sequence_count] (0 = NULL),
    range_bounds uint32 [n_ranges][2] = from, to (both inclusive).  Returns uint16 [row_words * 64 + guard_rows]: each row's range,
    0xFFFF for none, followed by `guard_rows` entries the call must not touch (they hold the byte `fill` repeated)."""
    lib = load_library()
    filter_words = np.ascontiguousarray(filter_words, dtype=np.uint64)
    dates = np.ascontiguousarray(dates, dtype=np.uint32)
    range_bounds = np.ascontiguousarray(range_bounds, dtype=np.uint32).reshape(-1, 2)
    rows = int(row_words) * 64 + int(guard_rows)
    filter_dev, dates_dev, out = _upload(filter_words, stream), _upload(dates, stream), device_malloc(rows * 2, fill, stream)
    try:
        _check(lib.silo_gpu_sample_groups(filter_dev, dates_dev, _ptr(range_bounds), len(range_bounds), sequence_count, row_words, out, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint16, rows, stream)
    finally:
        for ptr in (filter_dev, dates_dev, out):
            device_free(ptr)


def sample(partitions, size, seed=0, n_groups=1, fill=None, guard_words=0, stream=None):
    """A whole K19 selection over host arrays: silo_gpu_sample_begin, four rounds of silo_gpu_sample_count per partition and
    silo_gpu_sample_advance, silo_gpu_sample_select per partition.  partitions: a list of dicts {filter: uint64 [row_words], groups:
    uint16 [row_words * 64] or None (one group of every selected row), sequence_count, row_words, first_row}.  Returns (outputs,
    state): per partition the row_words words silo_gpu_sample_select writes followed by `guard_words` words behind them that it
    must not touch (every output is filled with the byte `fill` before the launches), and the state after round 3 as sample_state
    gives it."""
    lib = load_library()
    state = device_malloc(sample_state_bytes(n_groups), fill, stream)
    device = []
    try:
        for part in partitions:
            filter_words = np.ascontiguousarray(part["filter"], dtype=np.uint64)
            groups = None if part.get("groups") is None else np.ascontiguousarray(part["groups"], dtype=np.uint16)
            device.append({"filter": _upload(filter_words, stream), "groups": None if groups is None else _upload(groups, stream),
                           "out": device_malloc((int(part["row_words"]) + int(guard_words)) * 8, fill, stream)})
        _check(lib.silo_gpu_sample_begin(state, n_groups, size, seed, stream))
        for sample_round in range(SAMPLE_ROUNDS):
            for part, dev in zip(partitions, device):
                _check(lib.silo_gpu_sample_count(state, dev["filter"], dev["groups"], part["sequence_count"], part["row_words"], part["first_row"],
                                                 sample_round, stream))
            _check(lib.silo_gpu_sample_advance(state, sample_round, stream))
        for part, dev in zip(partitions, device):
            _check(lib.silo_gpu_sample_select(state, dev["filter"], dev["groups"], part["sequence_count"], part["row_words"], part["first_row"],
                                              dev["out"], stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        outputs = [device_read(dev["out"], np.uint64, int(part["row_words"]) + int(guard_words), stream) for part, dev in zip(partitions, device)]
        return outputs, sample_state(device_read(state, np.uint32, sample_state_bytes(n_groups) // 4, stream), n_groups)
    finally:
        device_free(state)
        for dev in device:
            for ptr in dev.values():
                if ptr is not None:
                    device_free(ptr)


CELL_COUNT_KINDS = 4           # SILO_GPU_CELL_COUNT_KINDS: substitutions, deletions, missing, ambiguous (K18's stats order)
CELL_COUNT_SUBSTITUTIONS, CELL_COUNT_DELETIONS, CELL_COUNT_MISSING, CELL_COUNT_AMBIGUOUS = 1, 2, 4, 8   # SILO_GPU_CELL_COUNT_*: bits of a kinds mask
MAX_CELL_COUNT_BINS = 4096     # SILO_GPU_MAX_CELL_COUNT_BINS


def row_cell_count_scratch_bytes(positions):
    """SILO_GPU_ROW_CELL_COUNT_SCRATCH_BYTES: the scratch silo_gpu_row_cell_counts needs."""
    return int(positions) * 17 + 1024


def bitset_from_cell_counts_call(table_ptr, row_words, sequence_count, kinds_mask, at_least, at_most, out_ptr, stream=None):
    """silo_gpu_bitset_from_cell_counts (K22) on the caller's device buffers, waited for."""
    lib = load_library()
    _check(lib.silo_gpu_bitset_from_cell_counts(table_ptr, row_words, sequence_count, kinds_mask, at_least, at_most, out_ptr, stream))
    _check(lib.silo_gpu_stream_synchronize(stream))


def bitset_from_cell_counts(table, row_words, sequence_count, kinds_mask, at_least=0, at_most=0xFFFFFFFF, fill=None, stream=None, guard_words=0):
    """silo_gpu_bitset_from_cell_counts (K22) over a host table uint32 [row_words * 64][4] as silo_gpu_row_cell_counts leaves it:
    bit r = r < sequence_count and at_least <= (the sum of the kinds of kinds_mask of row r) <= at_most.  Returns the row_words words
    the call writes, followed by `guard_words` words behind them that it must not touch: those hold the byte `fill` repeated (the
    whole allocation is filled with it before the launch), or whatever the allocation held."""
    table = np.ascontiguousarray(table, dtype=np.uint32)
    words = int(row_words) + int(guard_words)
    table_dev = _upload(table, stream)
    out = device_malloc(words * 8, fill, stream)
    try:
        bitset_from_cell_counts_call(table_dev, row_words, sequence_count, kinds_mask, at_least, at_most, out, stream)
        return device_read(out, np.uint64, words, stream)
    finally:
        device_free(table_dev)
        device_free(out)


def cell_count_histogram_call(table_ptr, row_words, sequence_count, filter_ptr, kinds_mask, bin_width, n_bins, bins_ptr, stream=None):
    """silo_gpu_cell_count_histogram (K22) on the caller's device buffers, waited for."""
    lib = load_library()
    _check(lib.silo_gpu_cell_count_histogram(table_ptr, row_words, sequence_count, filter_ptr, kinds_mask, bin_width, n_bins, bins_ptr, stream))
    _check(lib.silo_gpu_stream_synchronize(stream))


def cell_count_histogram(parts, kinds_mask, bin_width, n_bins, initial=None, guard_words=4, fill=0xA5, stream=None):
    """silo_gpu_cell_count_histogram (K22), one call per part into ONE array of bins.  parts: a list of dicts {table: uint32
    [row_words * 64][4], row_words, sequence_count, filter: uint64 [row_words] or None (every row)}.  initial: what the bins hold
    before the first call (uint64 [n_bins]; None = zeros).  Returns uint64 [n_bins + guard_words]: the bins, then `guard_words`
    words behind them that hold the byte `fill` repeated and that no call may touch."""
    lib = load_library()
    start = np.zeros(int(n_bins), dtype=np.uint64) if initial is None else np.ascontiguousarray(initial, dtype=np.uint64)
    bins = device_malloc((int(n_bins) + int(guard_words)) * 8, fill, stream)
    live = []
    try:
        if start.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(bins, _ptr(start), start.nbytes, stream))
        for part in parts:
            table_dev = _upload(np.ascontiguousarray(part["table"], dtype=np.uint32), stream)
            live.append(table_dev)
            filter_dev = None
            if part.get("filter") is not None:
                filter_dev = _upload(np.ascontiguousarray(part["filter"], dtype=np.uint64), stream)
                live.append(filter_dev)
            cell_count_histogram_call(table_dev, part["row_words"], part["sequence_count"], filter_dev, kinds_mask, bin_width, n_bins, bins, stream)
        return device_read(bins, np.uint64, int(n_bins) + int(guard_words), stream)
    finally:
        device_free(bins)
        for ptr in live:
            device_free(ptr)


MAX_REGIONS = 256              # SILO_GPU_MAX_REGIONS: the regions of one silo_gpu_region_cell_values, the columns of one silo_gpu_count_values


def region_value_scratch_bytes(positions):
    """SILO_GPU_REGION_VALUE_SCRATCH_BYTES: the scratch silo_gpu_region_cell_values needs."""
    return int(positions) * 7 + 8192


def bitset_from_values_call(values_ptr, row_words, sequence_count, at_least, at_most, out_ptr, stream=None):
    """silo_gpu_bitset_from_values (K23) on the caller's device buffers, waited for."""
    lib = load_library()
    _check(lib.silo_gpu_bitset_from_values(values_ptr, row_words, sequence_count, at_least, at_most, out_ptr, stream))
    _check(lib.silo_gpu_stream_synchronize(stream))


def bitset_from_values(values, row_words, sequence_count, at_least=0, at_most=0xFFFFFFFF, fill=None, stream=None, guard_words=0):
    """silo_gpu_bitset_from_values (K23) over ONE host column uint32 [row_words * 64] as silo_gpu_region_cell_values leaves it:
    bit r = r < sequence_count and at_least <= values[r] <= at_most.  Returns the row_words words the call writes, followed by
    `guard_words` words behind them that it must not touch: those hold the byte `fill` repeated (the whole allocation is filled
    with it before the launch), or whatever the allocation held."""
    values = np.ascontiguousarray(values, dtype=np.uint32)
    words = int(row_words) + int(guard_words)
    values_dev = _upload(values, stream)
    out = device_malloc(words * 8, fill, stream)
    try:
        bitset_from_values_call(values_dev, row_words, sequence_count, at_least, at_most, out, stream)
        return device_read(out, np.uint64, words, stream)
    finally:
        device_free(values_dev)
        device_free(out)


def count_values_call(values_ptr, n_columns, row_words, sequence_count, filter_ptr, bounds, counts_ptr, stream=None):
    """silo_gpu_count_values (K23) on the caller's device buffers, waited for.  bounds: host uint32 [n_columns][2], or None for NULL."""
    lib = load_library()
    if bounds is not None:
        bounds = np.ascontiguousarray(bounds, dtype=np.uint32)
    _check(lib.silo_gpu_count_values(values_ptr, n_columns, row_words, sequence_count, filter_ptr, None if bounds is None else _ptr(bounds), counts_ptr, stream))
    _check(lib.silo_gpu_stream_synchronize(stream))


def count_values(parts, bounds, initial=None, guard_words=4, fill=0xA5, stream=None):
    """silo_gpu_count_values (K23), one call per part into ONE array of counts.  parts: a list of dicts {values: uint32 [n_columns]
    [row_words * 64], row_words, sequence_count, filter: uint64 [row_words] or None (every row)}.  bounds: uint32 [n_columns][2] =
    at least, at most.  initial: what the counts hold before the first call (uint64 [n_columns]; None = zeros).  Returns uint64
    [n_columns + guard_words]: the counts, then `guard_words` words behind them that hold the byte `fill` repeated and that no call
    may touch."""
    lib = load_library()
    bounds = np.ascontiguousarray(bounds, dtype=np.uint32).reshape(-1, 2)
    n_columns = len(bounds)
    start = np.zeros(n_columns, dtype=np.uint64) if initial is None else np.ascontiguousarray(initial, dtype=np.uint64)
    counts = device_malloc((n_columns + int(guard_words)) * 8, fill, stream)
    live = []
    try:
        if start.nbytes:
            _check(lib.silo_gpu_memcpy_h2d(counts, _ptr(start), start.nbytes, stream))
        for part in parts:
            values_dev = _upload(np.ascontiguousarray(part["values"], dtype=np.uint32), stream)
            live.append(values_dev)
            filter_dev = None
            if part.get("filter") is not None:
                filter_dev = _upload(np.ascontiguousarray(part["filter"], dtype=np.uint64), stream)
                live.append(filter_dev)
            count_values_call(values_dev, n_columns, part["row_words"], part["sequence_count"], filter_dev, bounds, counts, stream)
        return device_read(counts, np.uint64, n_columns + int(guard_words), stream)
    finally:
        device_free(counts)
        for ptr in live:
            device_free(ptr)


ROW_HASH_NO_SYMBOL = 31        # SILO_GPU_ROW_HASH_NO_SYMBOL: a cell that nothing stored claims
DISTINCT_EMPTY = 0xFFFFFFFF    # SILO_GPU_DISTINCT_EMPTY: a slot of the owner table without an owner
DISTINCT_PART_DTYPE = np.dtype([("hashes_dev", np.uint64), ("first_row", np.uint32), ("sequence_count", np.uint32),
                                ("row_words", np.uint32), ("reserved", np.uint32)])   # silo_gpu_distinct_part


def row_hash_scratch_bytes(positions):
    """SILO_GPU_ROW_HASH_SCRATCH_BYTES: the scratch silo_gpu_row_hashes needs."""
    return int(positions) * 17 + 1024


def distinct_table_bytes(slots):
    """SILO_GPU_DISTINCT_TABLE_BYTES: `slots` owners and the overflow counter behind them."""
    return (int(slots) + 1) * 4


def distinct_slots(rows):
    """The smallest power of two >= 2 x rows (at least 2): the table size the engine takes for a database of `rows` rows."""
    slots = 2
    while slots < 2 * int(rows):
        slots *= 2
    return slots


def row_hash_term(position, symbol, lane):
    """silo_gpu_row_hash_term: H0 (lane 0) / H1 (lane 1) of a cell (host function; the kernels compile the same code)."""
    return int(load_library().silo_gpu_row_hash_term(int(position), int(symbol), int(lane)))


def distinct(parts, slots, fill=None, guard_words=0, calls=1, described=None, stream=None):
    """A whole K20 selection over host arrays: silo_gpu_distinct_begin, silo_gpu_distinct_insert per part, silo_gpu_distinct_select
    per part; the whole sequence `calls` times.  parts: a list of dicts {hashes: uint64 [row_words * 64][2], filter: uint64
    [row_words], first_row, sequence_count, row_words}, ordered by first_row.  Returns (outputs, owners, overflow): per part the
    row_words words silo_gpu_distinct_select writes followed by `guard_words` words behind them that it must not touch (every
    output is filled with the byte `fill` before the launches), the `slots` owners and the overflow counter."""
    lib = load_library()
    table = device_malloc(distinct_table_bytes(slots), fill, stream)
    device = []
    parts_dev = None
    try:
        records = np.zeros(len(parts), dtype=DISTINCT_PART_DTYPE)
        for k, part in enumerate(parts):
            hashes = np.ascontiguousarray(part["hashes"], dtype=np.uint64)
            device.append({"hashes": _upload(hashes, stream), "filter": _upload(np.ascontiguousarray(part["filter"], dtype=np.uint64), stream),
                           "out": device_malloc((int(part["row_words"]) + int(guard_words)) * 8, fill, stream)})
            records[k] = (device[k]["hashes"].value, part["first_row"], part["sequence_count"], part["row_words"], 0)
        parts_dev = _upload(records, stream)
        for _ in range(calls):
            _check(lib.silo_gpu_distinct_begin(table, slots, stream))
            for k, dev in enumerate(device):
                _check(lib.silo_gpu_distinct_insert(table, slots, parts_dev, len(parts), k, dev["filter"], stream))
            for k, dev in enumerate(device):
                _check(lib.silo_gpu_distinct_select(table, slots, parts_dev, len(parts), k, dev["filter"], dev["out"], stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        outputs = [device_read(dev["out"], np.uint64, int(part["row_words"]) + int(guard_words), stream) for part, dev in zip(parts, device)]
        words = device_read(table, np.uint32, int(slots) + 1, stream)
        return outputs, words[:-1].copy(), int(words[-1])
    finally:
        device_free(table)
        if parts_dev is not None:
            device_free(parts_dev)
        for dev in device:
            for ptr in dev.values():
                device_free(ptr)


MAX_DISTINCT_CLASSES = 16384          # SILO_GPU_MAX_DISTINCT_CLASSES: the most keys silo_gpu_smallest_keys selects
SMALLEST_KEYS_SCRATCH_BYTES = 1088    # SILO_GPU_SMALLEST_KEYS_SCRATCH_BYTES


def distinct_counts_bytes(slots):
    """SILO_GPU_DISTINCT_COUNTS_BYTES: one uint32 per slot of the owner table."""
    return int(slots) * 4


def distinct_class_key(count, global_row):
    """The key silo_gpu_distinct_classes appends for a class: ascending keys are descending counts, then ascending rows."""
    return ((0xFFFFFFFF - int(count)) << 32) | int(global_row)


def distinct_counts(parts, slots, min_count=1, capacity=1, fill=None, guard_words=0, calls=1, stream=None):
    """K20's table and K21's class counts over host arrays: silo_gpu_distinct_begin and silo_gpu_distinct_insert per part, then
    `calls` times { counts and the key counter cleared, silo_gpu_distinct_count per part, silo_gpu_distinct_classes per part }.
    parts as for distinct().  Returns a dict: owners uint32 [slots], overflow, counts uint32 [slots + guard_words], keys uint64
    [capacity + guard_words] and n_keys, what *n_keys_dev holds — the words behind `slots` counts and behind `capacity` keys are
    guards that no call may touch (counts apart, every array is filled with the byte `fill` before the launches)."""
    lib = load_library()
    table = device_malloc(distinct_table_bytes(slots), fill, stream)
    counts = device_malloc((int(slots) + int(guard_words)) * 4, fill, stream)
    keys = device_malloc((int(capacity) + int(guard_words)) * 8, fill, stream)
    n_keys = device_malloc(4, fill, stream)
    device = []
    parts_dev = None
    try:
        records = np.zeros(len(parts), dtype=DISTINCT_PART_DTYPE)
        for k, part in enumerate(parts):
            hashes = np.ascontiguousarray(part["hashes"], dtype=np.uint64)
            device.append({"hashes": _upload(hashes, stream), "filter": _upload(np.ascontiguousarray(part["filter"], dtype=np.uint64), stream)})
            records[k] = (device[k]["hashes"].value, part["first_row"], part["sequence_count"], part["row_words"], 0)
        parts_dev = _upload(records, stream)
        _check(lib.silo_gpu_distinct_begin(table, slots, stream))
        for k, dev in enumerate(device):
            _check(lib.silo_gpu_distinct_insert(table, slots, parts_dev, len(parts), k, dev["filter"], stream))
        for _ in range(calls):
            _check(lib.silo_gpu_memset_async(counts, 0, distinct_counts_bytes(slots), stream))
            _check(lib.silo_gpu_memset_async(n_keys, 0, 4, stream))
            for k, dev in enumerate(device):
                _check(lib.silo_gpu_distinct_count(table, slots, counts, parts_dev, len(parts), k, dev["filter"], stream))
            for k, dev in enumerate(device):
                _check(lib.silo_gpu_distinct_classes(table, slots, counts, parts_dev, len(parts), k, dev["filter"], min_count, keys, capacity,
                                                     n_keys, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        words = device_read(table, np.uint32, int(slots) + 1, stream)
        return {"owners": words[:-1].copy(), "overflow": int(words[-1]),
                "counts": device_read(counts, np.uint32, int(slots) + int(guard_words), stream),
                "keys": device_read(keys, np.uint64, int(capacity) + int(guard_words), stream),
                "n_keys": int(device_read(n_keys, np.uint32, 1, stream)[0])}
    finally:
        for ptr in (table, counts, keys, n_keys):
            device_free(ptr)
        if parts_dev is not None:
            device_free(parts_dev)
        for dev in device:
            for ptr in dev.values():
                device_free(ptr)


def smallest_keys(keys, n, k, fill=None, guard_words=0, calls=1, stream=None):
    """silo_gpu_smallest_keys over a host array: keys uint64 [capacity] of which the first `n` are the list (n reaches the device
    as *n_keys_dev only).  Returns (out, count): uint64 [k + guard_words], filled with the byte `fill` before the launches, and
    what *out_count_dev holds after `calls` calls."""
    lib = load_library()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    keys_dev, n_dev = _upload(keys, stream), _upload(np.array([n], dtype=np.uint32), stream)
    out = device_malloc((int(k) + int(guard_words)) * 8, fill, stream)
    out_count = device_malloc(4, fill, stream)
    scratch = device_malloc(SMALLEST_KEYS_SCRATCH_BYTES, fill, stream)
    try:
        for _ in range(calls):
            _check(lib.silo_gpu_smallest_keys(keys_dev, n_dev, len(keys), k, out, out_count, scratch, stream))
        _check(lib.silo_gpu_stream_synchronize(stream))
        return device_read(out, np.uint64, int(k) + int(guard_words), stream), int(device_read(out_count, np.uint32, 1, stream)[0])
    finally:
        for ptr in (keys_dev, n_dev, out, out_count, scratch):
            device_free(ptr)


class GpuStore:
    """One device shard: the dense restatement of a DatabasePartition's sequence stores."""

    def __init__(self, sequence_count, seqstores, device=0):
        """seqstores: list of dicts {name, alphabet ('nuc'|'aa'), reference (np.uint8 symbol ids)}."""
        self.lib = load_library()
        self.sequence_count = int(sequence_count)
        self.names = [s["name"] for s in seqstores]
        self.alphabets = [s["alphabet"] for s in seqstores]
        self.references = [np.ascontiguousarray(s["reference"], dtype=np.uint8) for s in seqstores]
        self._keep = []
        descs = (SeqStoreDesc * len(seqstores))()
        self.scan_symbols = []
        for k, s in enumerate(seqstores):
            alpha = alphabet.ALPHABETS[s["alphabet"]]
            scan = np.array(s.get("scan_symbols", alpha.valid_mutation_symbols), dtype=np.uint8)
            extra = np.array(s.get("extra_symbols", [alpha.missing]), dtype=np.uint8)
            self._keep += [scan, extra]
            self.scan_symbols.append(scan)
            descs[k].alphabet = alpha.abi_id
            descs[k].positions = len(self.references[k])
            descs[k].reference = self.references[k].ctypes.data_as(c_u8p)
            descs[k].n_scan_symbols = len(scan)
            descs[k].scan_symbols = scan.ctypes.data_as(c_u8p)
            descs[k].n_extra_symbols = len(extra)
            descs[k].extra_symbols = extra.ctypes.data_as(c_u8p)
        desc = StoreDesc(device, self.sequence_count, len(seqstores), descs)
        handle = ctypes.c_void_p()
        _check(self.lib.silo_gpu_store_create(ctypes.byref(desc), ctypes.byref(handle)))
        self.handle = handle
        self.row_words = self.lib.silo_gpu_store_row_words(handle)
        self._owned = []

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "handle", None):
            for ptr in self._owned:
                self.lib.silo_gpu_free(ptr)
            self._owned = []
            self.lib.silo_gpu_store_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def device_bytes(self):
        return self.lib.silo_gpu_store_device_bytes(self.handle)

    def seqstore_id(self, name):
        return self.names.index(name)

    def positions(self, seqstore_id):
        return len(self.references[seqstore_id])

    # -- build ----------------------------------------------------------------------------------
    def append_sequences(self, seqstore_id, first_sequence, sequences, is_null=None):
        """sequences: list of str/bytes (None = missing genome) or uint8 array [n][P] of characters."""
        positions = self.positions(seqstore_id)
        if isinstance(sequences, np.ndarray):
            chars = np.ascontiguousarray(sequences, dtype=np.uint8)
            n = chars.shape[0]
        else:
            n = len(sequences)
            chars = np.zeros((n, positions), dtype=np.uint8)
            if is_null is None:
                is_null = np.zeros(n, dtype=np.uint8)
            for i, seq in enumerate(sequences):
                if seq is None:
                    is_null[i] = 1
                    continue
                raw = seq.encode() if isinstance(seq, str) else bytes(seq)
                if len(raw) != positions:
                    raise ValueError(f"sequence {i} has length {len(raw)}, expected {positions}")
                chars[i] = np.frombuffer(raw, dtype=np.uint8)
        assert chars.shape == (n, positions)
        null_ptr = None
        if is_null is not None:
            is_null = np.ascontiguousarray(is_null, dtype=np.uint8)
            null_ptr = _ptr(is_null)
        _check(self.lib.silo_gpu_store_append_sequences(self.handle, seqstore_id, first_sequence, n, _ptr(chars), null_ptr))

    def generate_synthetic(self, seqstore_id, model):
        """model: silo_amd.synth.SynthModel for this sequence store."""
        arrays = dict(
            lineage=np.ascontiguousarray(model.lineage_of_sequence, dtype=np.uint16),
            lead=np.ascontiguousarray(model.lead_gap, dtype=np.uint32),
            trail=np.ascontiguousarray(model.trail_gap, dtype=np.uint32),
            mstart=np.ascontiguousarray(model.missing_start, dtype=np.uint32),
            mlen=np.ascontiguousarray(model.missing_len, dtype=np.uint32),
            table=np.ascontiguousarray(model.lineage_symbol, dtype=np.uint8),
        )
        assert len(arrays["lineage"]) == self.sequence_count
        assert arrays["table"].shape == (self.positions(seqstore_id), model.n_lineages)
        desc = SynthDesc(
            model.seed, model.n_lineages,
            arrays["lineage"].ctypes.data_as(c_u16p), arrays["lead"].ctypes.data_as(c_u32p),
            arrays["trail"].ctypes.data_as(c_u32p), arrays["mstart"].ctypes.data_as(c_u32p),
            arrays["mlen"].ctypes.data_as(c_u32p), arrays["table"].ctypes.data_as(c_u8p),
            model.private_threshold, model.ambiguous_threshold, 0, 0,
        )
        _check(self.lib.silo_gpu_store_generate_synthetic(self.handle, seqstore_id, ctypes.byref(desc)))

    def finalize(self):
        _check(self.lib.silo_gpu_store_finalize(self.handle))

    # -- device buffers -------------------------------------------------------------------------
    def bitset_alloc(self):
        ptr = ctypes.c_void_p()
        _check(self.lib.silo_gpu_bitset_alloc(self.handle, ctypes.byref(ptr)))
        self._owned.append(ptr)
        return ptr

    def malloc(self, nbytes):
        ptr = ctypes.c_void_p()
        _check(self.lib.silo_gpu_malloc(nbytes, ctypes.byref(ptr)))
        self._owned.append(ptr)
        return ptr

    def free(self, ptr):
        self._owned = [p for p in self._owned if p.value != ptr.value]
        self.lib.silo_gpu_free(ptr)

    def bitset_upload(self, ptr, words, stream=None):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        _check(self.lib.silo_gpu_bitset_upload(self.handle, ptr, _ptr(words), len(words), stream))

    def bitset_download(self, ptr, stream=None):
        out = np.empty(self.row_words, dtype=np.uint64)
        _check(self.lib.silo_gpu_bitset_download(self.handle, _ptr(out), ptr, self.row_words, stream))
        return out

    def bitset_from_lineages(self, ptr, membership, stream=None):
        membership = np.ascontiguousarray(membership, dtype=np.uint8)
        _check(self.lib.silo_gpu_bitset_from_lineages(self.handle, ptr, _ptr(membership), len(membership), stream))

    def plane(self, seqstore_id, position, symbol):
        """Device pointer (int) of a dense plane or None for a sparse symbol."""
        return self.lib.silo_gpu_store_plane(self.handle, seqstore_id, position, symbol)

    def plane_download(self, seqstore_id, position, symbol):
        ptr = self.plane(seqstore_id, position, symbol)
        if ptr is None:
            tmp = self.bitset_alloc()
            _check(self.lib.silo_gpu_store_sparse_plane(self.handle, seqstore_id, position, symbol, tmp, None))
            out = self.bitset_download(tmp)
            self.free(tmp)
            return out
        return self.bitset_download(ctypes.c_void_p(ptr))

    def sparse_plane(self, seqstore_id, position, symbol, dst, stream=None):
        _check(self.lib.silo_gpu_store_sparse_plane(self.handle, seqstore_id, position, symbol, dst, stream))

    def memset(self, ptr, value, nbytes, stream=None):
        _check(self.lib.silo_gpu_memset_async(ptr, value, nbytes, stream))

    def read(self, ptr, dtype, count, stream=None):
        out = np.empty(count, dtype=dtype)
        _check(self.lib.silo_gpu_memcpy_d2h(_ptr(out), ptr, out.nbytes, stream))
        return out

    def synchronize(self, stream=None):
        _check(self.lib.silo_gpu_stream_synchronize(stream))

    # -- kernels --------------------------------------------------------------------------------
    def filter_eval(self, code, leaves, n_slots, out_bitset=None, out_count=None, stream=None):
        """code: flat list of uint32 (2 per instruction); leaves: list of device pointers (int)."""
        code = np.ascontiguousarray(code, dtype=np.uint32)
        leaf_array = (ctypes.c_void_p * max(1, len(leaves)))(*[
            (l.value if isinstance(l, ctypes.c_void_p) else l) for l in leaves
        ])
        prog = BitProg(len(code) // 2, code.ctypes.data_as(c_u32p), len(leaves), leaf_array, n_slots)
        _check(self.lib.silo_gpu_filter_eval(self.handle, ctypes.byref(prog), out_bitset, out_count, stream))

    def filter_eval_batch(self, programs, out_bitsets=None, stream=None):
        """programs: list of (code, leaves, n_slots); returns the cardinalities (one launch for all of them)."""
        return filter_eval_batch(self.handle, programs, out_bitsets, stream)

    def filter_eval_count(self, code, leaves, n_slots, slot, out_bitset=None, stream=None):
        """silo_gpu_filter_eval_count: as filter_eval, the cardinality delivered into `slot` (a CountSlot; read it with
        slot.wait(stream)).  Only launches."""
        code = np.ascontiguousarray(code, dtype=np.uint32)
        leaf_array = (ctypes.c_void_p * max(1, len(leaves)))(*[
            (l.value if isinstance(l, ctypes.c_void_p) else l) for l in leaves
        ])
        prog = BitProg(len(code) // 2, code.ctypes.data_as(c_u32p), len(leaves), leaf_array, n_slots)
        _check(self.lib.silo_gpu_filter_eval_count(self.handle, ctypes.byref(prog), out_bitset, None if slot is None else slot.handle, stream))

    def count_buffer(self, stream=None):
        """Zeroed accumulator for cardinalities: COUNT_SHARDS uint64 (their sum is the count)."""
        counter = self.malloc(8 * COUNT_SHARDS)
        self.memset(counter, 0, 8 * COUNT_SHARDS, stream)
        return counter

    def read_count(self, counter, stream=None):
        return int(self.read(counter, np.uint64, COUNT_SHARDS, stream).sum())

    def popcount(self, bitset, stream=None):
        counter = self.count_buffer(stream)
        _check(self.lib.silo_gpu_popcount(self.handle, bitset, counter, stream))
        value = self.read_count(counter, stream)
        self.free(counter)
        return value

    def mutations_scan_async(self, seqstore_id, filter_ptr, pos_begin, pos_end, counts_ptr, stream=None):
        _check(self.lib.silo_gpu_mutations_scan(self.handle, seqstore_id, filter_ptr, pos_begin, pos_end, counts_ptr, stream))

    def mutations_scan(self, seqstore_id, filter_ptr=None, pos_begin=0, pos_end=None, stream=None):
        """Returns uint32 counts [pos_end - pos_begin][n_scan_symbols]."""
        if pos_end is None:
            pos_end = self.positions(seqstore_id)
        n_scan = len(self.scan_symbols[seqstore_id])
        n = (pos_end - pos_begin) * n_scan
        counts = self.malloc(max(4, 4 * n))
        self.memset(counts, 0, max(4, 4 * n), stream)
        self.mutations_scan_async(seqstore_id, filter_ptr, pos_begin, pos_end, counts, stream)
        out = self.read(counts, np.uint32, n, stream).reshape(pos_end - pos_begin, n_scan)
        self.free(counts)
        return out

    def mutations_scan_batch(self, seqstore_id, filter_ptrs, pos_begin=0, pos_end=None, stream=None):
        """One pass over the planes for several filters; returns a list of uint32 count tables."""
        if pos_end is None:
            pos_end = self.positions(seqstore_id)
        n_scan = len(self.scan_symbols[seqstore_id])
        n = (pos_end - pos_begin) * n_scan
        outs = []
        for _ in filter_ptrs:
            buf = self.malloc(max(4, 4 * n))
            self.memset(buf, 0, max(4, 4 * n), stream)
            outs.append(buf)
        filters = (ctypes.c_void_p * len(filter_ptrs))(*[(f.value if isinstance(f, ctypes.c_void_p) else f) for f in filter_ptrs])
        counts = (ctypes.c_void_p * len(outs))(*[o.value for o in outs])
        _check(self.lib.silo_gpu_mutations_scan_batch(self.handle, seqstore_id, filters, len(filter_ptrs), pos_begin, pos_end, counts, stream))
        tables = [self.read(o, np.uint32, n, stream).reshape(pos_end - pos_begin, n_scan) for o in outs]
        for o in outs:
            self.free(o)
        return tables

    def scan_planes(self, seqstore_id):
        """Code planes per position of the store's most common layout: 2 (or 3) after the re-encoding at finalize, else 3 / 5."""
        return self.lib.silo_gpu_store_scan_planes(self.handle, seqstore_id)

    def scan_rows(self, seqstore_id, pos_begin, pos_end):
        """Plane rows the Mutations scan reads for positions [pos_begin, pos_end)."""
        return int(self.lib.silo_gpu_store_scan_rows(self.handle, seqstore_id, pos_begin, pos_end))

    def finalize_seqstore(self, seqstore_id):
        _check(self.lib.silo_gpu_store_finalize_seqstore(self.handle, seqstore_id))

    def scan_runs(self, seqstore_id):
        """Runs of the missing symbol a scan of the store reads (0 unless the store derives the most numerous symbol of its positions)."""
        return int(self.lib.silo_gpu_store_scan_runs(self.handle, seqstore_id))

    def scan_escapes(self, seqstore_id):
        return self.lib.silo_gpu_store_scan_escapes(self.handle, seqstore_id)

    def scan_overflow_keys(self, seqstore_id):
        """Escape keys of the store that do not fit the packed form of their granule: a scan counts them in a launch of its own
        (0 for a store that is not finalized or has no slice-major keys)."""
        return int(self.lib.silo_gpu_store_scan_overflow_keys(self.handle, seqstore_id))

    def scan_prunable_granules(self, seqstore_id, cardinality, min_proportion):
        """(skippable, total) granules of the store's slice-major escape keys for one filter of `cardinality` rows."""
        skippable, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.lib.silo_gpu_store_scan_prunable_granules(self.handle, seqstore_id, int(cardinality), ctypes.c_double(min_proportion),
                                                              ctypes.byref(skippable), ctypes.byref(total)))
        return skippable.value, total.value

    def scan_end_runs(self, seqstore_id):
        """The end runs of the gap symbol a Mutations scan counts instead of reading rows: (covered one-hot rows, end events,
        residual keys) of a sequence store; all 0 where the store has none."""
        return (int(self.lib.silo_gpu_store_scan_covered_rows(self.handle, seqstore_id)), int(self.lib.silo_gpu_store_scan_end_events(self.handle, seqstore_id)),
                int(self.lib.silo_gpu_store_scan_residual_keys(self.handle, seqstore_id)))

    def scan_prunable_rows(self, seqstore_id, cardinality, min_proportion):
        """(skippable, total) one-hot plane rows of the store for one filter of `cardinality` rows."""
        skippable, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.lib.silo_gpu_store_scan_prunable_rows(self.handle, seqstore_id, int(cardinality), ctypes.c_double(min_proportion),
                                                          ctypes.byref(skippable), ctypes.byref(total)))
        return skippable.value, total.value

    def mutations_scan_ranges(self, ranges, filter_ptrs, stream=None, min_proportions=None):
        """Every filter over every (seqstore_id, pos_begin, pos_end) range in as few launches as the layouts allow;
        returns tables[range][filter].  min_proportions (one per filter): silo_gpu_mutations_scan_ranges_min_proportion."""
        flat = (ctypes.c_uint32 * (3 * len(ranges)))(*[int(v) for r in ranges for v in r])  # silo_gpu_scan_range[]
        outs = []
        for seqstore_id, pos_begin, pos_end in ranges:
            n = (pos_end - pos_begin) * len(self.scan_symbols[seqstore_id])
            for _ in filter_ptrs:
                buf = self.malloc(max(4, 4 * n))
                self.memset(buf, 0, max(4, 4 * n), stream)
                outs.append(buf)
        filters = (ctypes.c_void_p * len(filter_ptrs))(*[(f.value if isinstance(f, ctypes.c_void_p) else f) for f in filter_ptrs])
        counts = (ctypes.c_void_p * max(1, len(outs)))(*[o.value for o in outs])
        if min_proportions is None:
            _check(self.lib.silo_gpu_mutations_scan_ranges(self.handle, flat, len(ranges), filters, len(filter_ptrs), counts, stream))
        else:
            proportions = (ctypes.c_double * max(1, len(filter_ptrs)))(*[float(p) for p in min_proportions])
            _check(self.lib.silo_gpu_mutations_scan_ranges_min_proportion(self.handle, flat, len(ranges), filters, len(filter_ptrs), proportions, counts, stream))
        tables = []
        for r, (seqstore_id, pos_begin, pos_end) in enumerate(ranges):
            n_scan = len(self.scan_symbols[seqstore_id])
            tables.append([self.read(outs[r * len(filter_ptrs) + q], np.uint32, (pos_end - pos_begin) * n_scan, stream).reshape(pos_end - pos_begin, n_scan)
                           for q in range(len(filter_ptrs))])
        for o in outs:
            self.free(o)
        return tables

    def mutations_scan_select(self, ranges, filter_ptrs, min_proportions, tables, table_offsets, total_positions, reference_ptr, slots, stream=None):
        """silo_gpu_mutations_scan_select: every filter over every (seqstore_id, pos_begin, pos_end) range, range r counted at position
        table_offsets[r] of the filter's device table tables[q] ([total_positions][scan symbols], overwritten), the selected rows of filter
        q delivered into slots[q] (RowSlot.wait); reference_ptr: the device array of the table's reference symbol indexes."""
        n_symbols = len(self.scan_symbols[ranges[0][0]])
        flat = (ctypes.c_uint32 * (3 * len(ranges)))(*[int(v) for r in ranges for v in r])
        filters = (ctypes.c_void_p * len(filter_ptrs))(*[(f.value if isinstance(f, ctypes.c_void_p) else f) for f in filter_ptrs])
        counts = (ctypes.c_void_p * (len(ranges) * len(filter_ptrs)))(
            *[tables[q].value + 4 * n_symbols * int(table_offsets[r]) for r in range(len(ranges)) for q in range(len(filter_ptrs))])
        proportions = (ctypes.c_double * len(filter_ptrs))(*[float(p) for p in min_proportions])
        sinks = (SelectSink * len(filter_ptrs))(
            *[SelectSink(tables[q].value, total_positions, n_symbols, reference_ptr.value, slots[q].handle.value) for q in range(len(filter_ptrs))])
        _check(self.lib.silo_gpu_mutations_scan_select(self.handle, flat, len(ranges), filters, len(filter_ptrs), proportions, counts, sinks, stream))

    def _count_table_call(self, launch, shape, scratch_bytes, out_ptr, stream, scratch_ptr, return_groups=False):
        """What the three count-table entries (K7, K8, K9) share around launch(scratch, table) -> status: the call's own scratch or
        the caller's; the call's own zeroed uint32 table of `shape`, read back and returned, or the caller's out_ptr, which
        returns nothing; return_groups: also (or only, with out_ptr) the uint16 [row_words * 64] range ids at the start of the
        scratch.  Whatever the call allocated is freed, also when it raises."""
        cells = int(np.prod(shape, dtype=np.int64))
        own_scratch = scratch_ptr is _OWN_SCRATCH
        scratch = self.malloc(scratch_bytes) if own_scratch else scratch_ptr
        table = out_ptr
        try:
            if out_ptr is None:
                table = self.malloc(max(8, 4 * cells))
                self.memset(table, 0, max(8, 4 * cells), stream)
            if own_scratch and return_groups:
                self.memset(scratch, 0xFF, self.row_words * 128, stream)  # a call that launches nothing assigns no row
            _check(launch(scratch, table))
            self.synchronize(stream)
            result = None
            if out_ptr is None:
                result = (self.read(table, np.uint32, cells, stream) if cells else np.zeros(0, dtype=np.uint32)).reshape(shape)
            if return_groups:
                groups = self.read(scratch, np.uint16, self.row_words * 64, stream)
                return groups if out_ptr is not None else (result, groups)
            return result
        finally:
            if own_scratch:
                self.free(scratch)
            if out_ptr is None and table is not None:
                self.free(table)

    @staticmethod
    def _pointer_array(pointers):
        """(array of device pointers, its length) for a list of row bitsets (None = all rows); (None, 0) for no list at all."""
        if pointers is None:
            return None, 0
        return (ctypes.c_void_p * max(1, len(pointers)))(*[(f.value if isinstance(f, ctypes.c_void_p) else f) for f in pointers]), len(pointers)

    def mutations_grouped(self, seqstore_id, filter_ptr, dates_ptr, ranges, positions, symbols, out_ptr=None, stream=None, return_groups=False,
                          scratch_ptr=_OWN_SCRATCH):
        """silo_gpu_mutations_grouped (K7).  ranges: (from, to) uint32 pairs in request order; positions / symbols: the listed
        cells; dates_ptr: a device column of uint32 dates (upload_column).  Without out_ptr: a zeroed table for the call, returned
        as uint32 [M][G][2] (count, coverage).  With out_ptr: accumulates into the caller's device table and returns nothing.
        return_groups: also (or only, with out_ptr) the per-row range ids the call leaves at the start of its scratch, uint16
        [row_words * 64] (0xFFFF = none).  scratch_ptr: the caller's scratch instead of one allocated for the call."""
        bounds = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint32).reshape(-1, 2))
        positions = np.ascontiguousarray(positions, dtype=np.uint32)
        symbols = np.ascontiguousarray(symbols, dtype=np.uint32)
        if len(positions) != len(symbols):
            raise ValueError("one symbol per position")
        n_ranges, n_mutations = len(bounds), len(positions)

        def launch(scratch, table):
            return self.lib.silo_gpu_mutations_grouped(self.handle, seqstore_id, filter_ptr, dates_ptr, _ptr(bounds), n_ranges, _ptr(positions),
                                                       _ptr(symbols), n_mutations, scratch, table, stream)

        return self._count_table_call(launch, (n_mutations, n_ranges, 2), grouped_scratch_bytes(self.row_words, n_ranges, n_mutations),
                                      out_ptr, stream, scratch_ptr, return_groups)

    def filters_grouped(self, base_ptr, dates_ptr, ranges, filter_ptrs, out_ptr=None, stream=None, return_groups=False, scratch_ptr=_OWN_SCRATCH):
        """silo_gpu_filters_grouped (K8).  ranges: (from, to) uint32 pairs in request order; filter_ptrs: device row bitsets
        (None = all rows), None for the whole list = a null array; base_ptr: the bitset every filter is intersected with (None = all
        rows); dates_ptr: a device column of uint32 dates (upload_column).  Without out_ptr: a zeroed table for the call, returned
        as uint32 [F][G].  With out_ptr: accumulates into the caller's device table and returns nothing.  return_groups: also (or
        only, with out_ptr) the per-row range ids under the base filter that the call leaves at the start of its scratch, uint16
        [row_words * 64] (0xFFFF = none).  scratch_ptr: the caller's scratch instead of one allocated for the call."""
        bounds = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint32).reshape(-1, 2))
        n_ranges = len(bounds)
        filters, n_filters = self._pointer_array(filter_ptrs)

        def launch(scratch, table):
            return self.lib.silo_gpu_filters_grouped(self.handle, base_ptr, dates_ptr, _ptr(bounds), n_ranges, filters, n_filters, scratch, table, stream)

        return self._count_table_call(launch, (n_filters, n_ranges), filters_grouped_scratch_bytes(self.row_words, n_ranges, n_filters),
                                      out_ptr, stream, scratch_ptr, return_groups)

    def filters_cross(self, base_ptr, row_ptrs, col_ptrs, row_index=None, col_index=None, out_shape=None, out_ptr=None, stream=None,
                      scratch_ptr=_OWN_SCRATCH):
        """silo_gpu_filters_cross (K9).  row_ptrs / col_ptrs: device row bitsets (None = all rows), None for a whole list = a null
        array; base_ptr: the bitset every pair is intersected with (None = all rows); row_index / col_index: where filter i / j
        lands in the table (None = identity); out_shape: (out_rows, out_cols), by default (len(row_ptrs), len(col_ptrs)).  Without
        out_ptr: a zeroed table for the call, returned as uint32 [out_rows][out_cols].  With out_ptr: accumulates into the caller's
        device table and returns nothing.  scratch_ptr: the caller's scratch instead of one allocated for the call."""
        rows, n_rows = self._pointer_array(row_ptrs)
        cols, n_cols = self._pointer_array(col_ptrs)
        row_index = None if row_index is None else np.ascontiguousarray(row_index, dtype=np.uint32)
        col_index = None if col_index is None else np.ascontiguousarray(col_index, dtype=np.uint32)
        if (row_index is not None and len(row_index) != n_rows) or (col_index is not None and len(col_index) != n_cols):
            raise ValueError("one index per filter")
        out_rows, out_cols = (n_rows, n_cols) if out_shape is None else out_shape

        def launch(scratch, table):
            return self.lib.silo_gpu_filters_cross(self.handle, base_ptr, rows, None if row_index is None else _ptr(row_index), n_rows,
                                                   cols, None if col_index is None else _ptr(col_index), n_cols, scratch, table, out_rows, out_cols, stream)

        return self._count_table_call(launch, (out_rows, out_cols), filters_cross_scratch_bytes(n_rows, n_cols), out_ptr, stream, scratch_ptr)

    def query_distances(self, seqstore_id, query, fill=None, stream=None, out_ptr=None, scratch_ptr=_OWN_SCRATCH):
        """silo_gpu_query_distances (K11).  query: the aligned query as bytes / uint8 [P] (None = a null pointer).  Without out_ptr:
        a table for the call — filled with the byte `fill` before the launch, so a test can see that every cell is written —
        returned as uint32 [row_words * 64][2] (distance, compared).  With out_ptr: writes the caller's device table and returns
        nothing.  scratch_ptr: the caller's scratch instead of one allocated for the call."""
        if query is not None:
            query = np.ascontiguousarray(np.frombuffer(query, dtype=np.uint8) if isinstance(query, (bytes, bytearray)) else query, dtype=np.uint8)
        known = seqstore_id < len(self.references)
        positions = len(self.references[seqstore_id]) if known else 0
        if known and query is not None and len(query) != positions:
            raise ValueError("the query has to be as long as the sequence store's reference")
        cells = self.row_words * 64 * 2
        own_scratch = scratch_ptr is _OWN_SCRATCH
        scratch = self.malloc(query_distance_scratch_bytes(positions)) if own_scratch else scratch_ptr
        table = out_ptr
        try:
            if out_ptr is None:
                table = self.malloc(max(8, 4 * cells))
                if fill is not None:
                    self.memset(table, fill, max(8, 4 * cells), stream)
            _check(self.lib.silo_gpu_query_distances(self.handle, seqstore_id, None if query is None else _ptr(query), table, scratch, stream))
            self.synchronize(stream)
            return self.read(table, np.uint32, cells, stream).reshape(-1, 2) if out_ptr is None else None
        finally:
            if own_scratch:
                self.free(scratch)
            if out_ptr is None and table is not None:
                self.free(table)

    def row_hashes(self, seqstore_id, fill=None, guard_rows=0, stream=None):
        """silo_gpu_row_hashes (K20) into a table for the call, filled with the byte `fill` before the launches so that a test can
        see that every cell is written: returns uint64 [row_words * 64 + guard_rows][2], the last `guard_rows` rows untouched."""
        rows = self.row_words * 64 + int(guard_rows)
        scratch = self.malloc(row_hash_scratch_bytes(self.positions(seqstore_id)))
        table = self.malloc(max(16, 16 * rows))
        try:
            if fill is not None:
                self.memset(table, fill, max(16, 16 * rows), stream)
            _check(self.lib.silo_gpu_row_hashes(self.handle, seqstore_id, table, scratch, stream))
            self.synchronize(stream)
            return self.read(table, np.uint64, rows * 2, stream).reshape(-1, 2)
        finally:
            self.free(scratch)
            self.free(table)

    def kept_row_hashes(self, seqstore_id, stream=None):
        """silo_gpu_store_row_hashes (K20): the device address of the store's own table of row hashes (computed on the first call)."""
        out = ctypes.c_void_p()
        _check(self.lib.silo_gpu_store_row_hashes(self.handle, seqstore_id, ctypes.byref(out), stream))
        return out.value

    def row_cell_counts(self, seqstore_id, fill=None, guard_rows=0, stream=None):
        """silo_gpu_row_cell_counts (K22) into a table for the call, filled with the byte `fill` before the launches so that a test
        can see that every cell is written: returns uint32 [row_words * 64 + guard_rows][4] (substitutions, deletions, missing,
        ambiguous), the last `guard_rows` rows untouched."""
        rows = self.row_words * 64 + int(guard_rows)
        scratch = self.malloc(row_cell_count_scratch_bytes(self.positions(seqstore_id)))
        table = self.malloc(max(16, 16 * rows))
        try:
            if fill is not None:
                self.memset(table, fill, max(16, 16 * rows), stream)
            _check(self.lib.silo_gpu_row_cell_counts(self.handle, seqstore_id, table, scratch, stream))
            self.synchronize(stream)
            return self.read(table, np.uint32, rows * 4, stream).reshape(-1, 4)
        finally:
            self.free(scratch)
            self.free(table)

    def kept_row_cell_counts(self, seqstore_id, stream=None):
        """silo_gpu_store_row_cell_counts (K22): the device address of the store's own table of cell counts (computed on the first call)."""
        out = ctypes.c_void_p()
        _check(self.lib.silo_gpu_store_row_cell_counts(self.handle, seqstore_id, ctypes.byref(out), stream))
        return out.value

    def region_cell_values(self, seqstore_id, ranges, kinds_mask, fill=None, guard_rows=0, stream=None):
        """silo_gpu_region_cell_values (K23) into columns for the call, filled with the byte `fill` before the launches so that a
        test can see that every cell is written.  ranges: 0-based half-open [first, end), ascending and disjoint.  Returns uint32
        [len(ranges) * row_words * 64 + guard_rows]: the columns region-major (reshape the first part to [len(ranges)][row_words *
        64]), the last `guard_rows` cells untouched."""
        ranges = np.ascontiguousarray(ranges, dtype=np.uint32).reshape(-1, 2)
        cells = len(ranges) * self.row_words * 64 + int(guard_rows)
        scratch = self.malloc(region_value_scratch_bytes(self.positions(seqstore_id)))
        columns = self.malloc(max(4, 4 * cells))
        try:
            if fill is not None:
                self.memset(columns, fill, max(4, 4 * cells), stream)
            _check(self.lib.silo_gpu_region_cell_values(self.handle, seqstore_id, _ptr(ranges), len(ranges), kinds_mask, columns, scratch, stream))
            self.synchronize(stream)
            return self.read(columns, np.uint32, cells, stream)
        finally:
            self.free(scratch)
            self.free(columns)

    def position_symbols(self, seqstore_id, positions, fill=None, guard_bytes=0, calls=1, null=(), n_positions=None, stream=None):
        """silo_gpu_position_symbols (K16).  positions: 0-based, any order, repeats allowed.  Returns (symbols uint8
        [len(positions) * row_words * 64 + guard_bytes], unresolved uint32 [1 + guard_bytes / 4], the status of the last of `calls`
        calls).  Both outputs are filled with the byte `fill` before the first call, so a test can see that every byte is written,
        that nothing behind them is, and that a second call gives the same bytes.  A status other than 0 is returned, not raised:
        the refusals leave the outputs as they were.  null: which of "store", "positions", "symbols", "unresolved" the call gets
        as NULL.  n_positions: what the call is told instead of len(positions)."""
        positions = np.ascontiguousarray(positions, dtype=np.uint32)
        symbol_bytes = len(positions) * self.row_words * 64 + int(guard_bytes)
        unresolved_words = 1 + int(guard_bytes) // 4
        symbols = self.malloc(max(8, symbol_bytes))
        unresolved = self.malloc(unresolved_words * 4)
        try:
            if fill is not None:
                self.memset(symbols, fill, max(8, symbol_bytes), stream)
                self.memset(unresolved, fill, unresolved_words * 4, stream)
            status = 0
            for _ in range(calls):
                status = self.lib.silo_gpu_position_symbols(
                    None if "store" in null else self.handle, seqstore_id, None if "positions" in null else _ptr(positions),
                    len(positions) if n_positions is None else n_positions, None if "symbols" in null else symbols,
                    None if "unresolved" in null else unresolved, stream)
            self.synchronize(stream)
            return self.read(symbols, np.uint8, symbol_bytes, stream), self.read(unresolved, np.uint32, unresolved_words, stream), status
        finally:
            self.free(symbols)
            self.free(unresolved)

    def position_symbols_call(self, seqstore_id, positions, symbols_ptr, unresolved_ptr, stream=None):
        """silo_gpu_position_symbols (K16) on the caller's device buffers, not waited for."""
        positions = np.ascontiguousarray(positions, dtype=np.uint32)
        _check(self.lib.silo_gpu_position_symbols(self.handle, seqstore_id, _ptr(positions), len(positions), symbols_ptr, unresolved_ptr, stream))

    # ---- metadata columns (K5 / K6) and FastaAligned ---------------------------------------------
    VALUE_TYPES = {np.dtype(np.int32): 0, np.dtype(np.uint32): 1, np.dtype(np.float64): 2}
    COMPARATORS = {"==": 0, "!=": 1, "<": 2, ">=": 3, ">": 4, "<=": 5}

    def upload_column(self, values):
        """int32 / uint32 / float64 array with one value per row -> device pointer (free with self.free)."""
        values = np.ascontiguousarray(values)
        out = ctypes.c_void_p()
        _check(self.lib.silo_gpu_upload_column(values.ctypes.data_as(ctypes.c_void_p), len(values), self.VALUE_TYPES[values.dtype], ctypes.byref(out)))
        return out

    def bitset_from_compare(self, column_ptr, dtype, comparator, value, stream=None):
        """Row bitset (as downloaded words) of `column <comparator> value`."""
        dtype = np.dtype(dtype)
        scalar = np.array([value], dtype=dtype)
        out = self.bitset_alloc()
        _check(self.lib.silo_gpu_bitset_from_compare(
            self.handle, out, column_ptr, self.VALUE_TYPES[dtype], self.COMPARATORS[comparator], scalar.ctypes.data_as(ctypes.c_void_p), stream))
        words = self.bitset_download(out, stream)
        self.free(out)
        return words

    def group_count(self, filter_ptr, id_ptrs, cardinalities, stream=None):
        """Histogram of the mixed-radix tuple ids (first column most significant) of the filtered rows."""
        n_bins = int(np.prod(cardinalities, dtype=np.int64))
        counts = self.malloc(4 * n_bins)
        self.memset(counts, 0, 4 * n_bins, stream)
        ids = (ctypes.c_void_p * len(id_ptrs))(*[p.value for p in id_ptrs])
        cards = (ctypes.c_uint32 * len(cardinalities))(*cardinalities)
        _check(self.lib.silo_gpu_group_count(self.handle, filter_ptr, ids, cards, len(id_ptrs), counts, stream))
        out = self.read(counts, np.uint32, n_bins, stream)
        self.free(counts)
        return out

    def group_count_hashed(self, filter_ptr, id_ptrs, cardinalities, max_rows, stream=None):
        """(tuple ids, counts) of the filtered rows through the HBM hash table (K6b), sorted by tuple id."""
        ids = (ctypes.c_void_p * len(id_ptrs))(*[p.value for p in id_ptrs])
        cards = (ctypes.c_uint32 * len(cardinalities))(*cardinalities)
        keys, counts, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        _check(self.lib.silo_gpu_group_count_hashed(self.handle, filter_ptr, ids, cards, len(id_ptrs), max_rows, ctypes.byref(keys),
                                                    ctypes.byref(counts), ctypes.byref(n), stream))
        if n.value == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        tuple_ids = self.read(keys, np.uint64, n.value, stream)
        tuple_counts = self.read(counts, np.uint32, n.value, stream)
        self.free(keys)
        self.free(counts)
        order = np.argsort(tuple_ids)
        return tuple_ids[order], tuple_counts[order]

    def reconstruct_sequences(self, seqstore_id, rows, stream=None):
        """The stored characters of the given rows: uint8 array [len(rows)][positions]."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        positions = self.positions(seqstore_id)
        rows_dev = self.upload_column(rows)
        out = self.malloc(max(1, len(rows) * positions))
        _check(self.lib.silo_gpu_reconstruct_sequences(self.handle, seqstore_id, rows_dev, len(rows), out, stream))
        chars = self.read(out, np.uint8, len(rows) * positions, stream).reshape(len(rows), positions)
        self.free(out)
        self.free(rows_dev)
        return chars

    def mutations_select(self, counts, reference_index, min_proportion, capacity, stream=None):
        """K4 on a host-made count table [positions][symbols]: (n_selected, rows[min(n, capacity)] as (position, symbol, count, total))."""
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        positions, n_symbols = counts.shape
        counts_dev = self.upload_column(counts.reshape(-1))
        ref = np.ascontiguousarray(reference_index, dtype=np.uint8)
        ref_dev = ctypes.c_void_p()
        _check(self.lib.silo_gpu_upload_bytes(ref.ctypes.data_as(ctypes.c_void_p), ref.nbytes, ctypes.byref(ref_dev)))
        out = self.malloc(16 + 16 * max(capacity, 1))
        _check(self.lib.silo_gpu_mutations_select(counts_dev, ref_dev, positions, n_symbols, ctypes.c_double(min_proportion), capacity, out, stream))
        words = self.read(out, np.uint32, 4 + 4 * max(capacity, 1), stream)
        for pointer in (counts_dev, ref_dev, out):
            self.free(pointer)
        n = int(words[0])
        return n, words[4:4 + 4 * min(n, capacity)].reshape(-1, 4)

    def mutations_select_to_slot(self, counts, reference_index, min_proportion, slot, stream=None):
        """K4 delivered into a RowSlot: (n_selected, rows[min(n, slot.capacity)]) as mutations_select returns them."""
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        positions, n_symbols = counts.shape
        # (an empty table still gets a device address, so that it is the entry point that refuses it)
        counts_dev = self.upload_column(counts.reshape(-1) if counts.size else np.zeros(1, dtype=np.uint32))
        ref = np.ascontiguousarray(reference_index if len(reference_index) else [0], dtype=np.uint8)
        ref_dev = ctypes.c_void_p()
        try:
            _check(self.lib.silo_gpu_upload_bytes(ref.ctypes.data_as(ctypes.c_void_p), ref.nbytes, ctypes.byref(ref_dev)))
            _check(self.lib.silo_gpu_mutations_select_to_slot(counts_dev, ref_dev, positions, n_symbols, ctypes.c_double(min_proportion),
                                                              None if slot is None else slot.handle, stream))
            return slot.wait(stream)
        finally:
            for pointer in (counts_dev, ref_dev):
                if pointer:
                    self.lib.silo_gpu_free(pointer)

    def bitset_from_value_ids(self, ptr, value_ids_ptr, membership, n_values=None, stream=None):
        """bit i of the bitset at ptr = membership[value_ids[i]] (ids >= n_values select nothing); value_ids_ptr: a device
        column of uint32 ids (upload_column).  n_values defaults to len(membership)."""
        if membership is not None:
            membership = np.ascontiguousarray(membership, dtype=np.uint8)
            if n_values is None:
                n_values = len(membership)
        _check(self.lib.silo_gpu_bitset_from_value_ids(self.handle, ptr, value_ids_ptr, None if membership is None else _ptr(membership), n_values or 0, stream))

    def bitset_from_pairs(self, ptr, rows_ptr, ids_ptr, n_pairs, membership, stream=None):
        """The bitset at ptr = the rows of the (row, id) pairs with membership[id] != 0; rows_ptr / ids_ptr: device columns of uint32."""
        membership = np.ascontiguousarray(membership, dtype=np.uint8)
        _check(self.lib.silo_gpu_bitset_from_pairs(self.handle, ptr, rows_ptr, ids_ptr, n_pairs, _ptr(membership), len(membership), stream))

    def count_pairs(self, filter_ptr, rows_ptr, ids_ptr, n_pairs, counts_ptr, stream=None):
        """counts[id] += pairs of that id whose row is in the filter (None = all rows); counts_ptr: device uint32 table, accumulated into."""
        _check(self.lib.silo_gpu_count_pairs(self.handle, filter_ptr, rows_ptr, ids_ptr, n_pairs, counts_ptr, stream))

    def last_scan_kernel(self):
        return self.lib.silo_gpu_last_scan_kernel().decode()

    def tune(self, knob, value):
        return self.lib.silo_gpu_tune(knob, value)

    def build_pass(self, seqstore_id, which):
        """Two-pass build: 1 = the sequences that follow are only counted, 2 = they are written straight into the adaptive planes."""
        _check(self.lib.silo_gpu_store_build_pass(self.handle, seqstore_id, which))

    def build_mode(self, seqstore_id):
        return self.lib.silo_gpu_store_build_mode(self.handle, seqstore_id)
