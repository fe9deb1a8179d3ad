"""ctypes binding of include/dge.h (libdge.so).  No fallback: if the HIP library is missing the import fails."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdge.so")

DGE_OK, DGE_ERR_ARG, DGE_ERR_RANGE, DGE_ERR_TOPK, DGE_ERR_CAP, DGE_ERR_STATE, DGE_ERR_DEVICE, DGE_ERR_IO = range(8)


class DgeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libdge error %d: %s" % (code, msg))
        self.code = code


class TrainConfig(C.Structure):
    """struct dge_train_config (include/dge.h) — the Word2Vec.Builder contract of J/DeepWalk.java:73-76."""
    _fields_ = [
        ("dim", C.c_int32), ("window", C.c_int32), ("negative", C.c_int32), ("min_count", C.c_int32),
        ("epochs", C.c_int32), ("workers", C.c_int32), ("alpha", C.c_float), ("min_alpha", C.c_float),
        ("seed", C.c_uint64), ("table_size", C.c_int64), ("n_vertices", C.c_int32), ("update_policy", C.c_int32),
        ("use_hs", C.c_int32), ("reserved", C.c_int32),
    ]


class TrainStats(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("words", C.c_int64), ("kernel_ms", C.c_double),
                ("walk_kernel_ms", C.c_double), ("launches", C.c_int64)]


class EvalResult(C.Structure):
    """struct dge_eval_result (include/dge.h) — what dge_model_eval_links / dge_model_eval_sgns hand back."""
    _fields_ = [("pairs", C.c_int64), ("negatives", C.c_int64), ("skipped", C.c_int64), ("auc", C.c_double),
                ("loss", C.c_double), ("kernel_ms", C.c_double)]


class SeqInfo(C.Structure):
    """struct dge_seq_info (include/dge.h) — what dge_walks_from_seq_text / dge_walks_from_seq_files report."""
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("rows", C.c_int64), ("tokens", C.c_int64), ("unknown", C.c_int64),
                ("names_added", C.c_int64), ("max_len", C.c_int32), ("reserved", C.c_int32), ("read_ms", C.c_double),
                ("kernel_ms", C.c_double)]


class SeqOutInfo(C.Structure):
    """struct dge_seq_out_info (include/dge.h) — what dge_walks_to_seq_text / dge_walks_write_seq report."""
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("tokens", C.c_int64), ("empty_lines", C.c_int64), ("kernel_ms", C.c_double),
                ("write_ms", C.c_double)]


class VecInfo(C.Structure):
    """struct dge_vec_info (include/dge.h) — what dge_vectors_from_vec_text / dge_vectors_from_vec_files report."""
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("rows", C.c_int64), ("values", C.c_int64), ("dropped", C.c_int64), ("missing", C.c_int64),
                ("names_added", C.c_int64), ("host_values", C.c_int64), ("dim", C.c_int32), ("reserved", C.c_int32), ("read_ms", C.c_double),
                ("kernel_ms", C.c_double)]


class OdInfo(C.Structure):
    """struct dge_od_info (include/dge.h) — what dge_graph_add_od_files / dge_graph_add_od_texts report."""
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("flows", C.c_int64), ("edges", C.c_int64), ("dropped", C.c_int64), ("regions", C.c_int64),
                ("sources", C.c_int64), ("host_values", C.c_int64), ("slices", C.c_int32), ("reserved", C.c_int32), ("read_ms", C.c_double),
                ("kernel_ms", C.c_double)]


class RegionsInfo(C.Structure):
    """struct dge_regions_info (include/dge.h)."""
    _fields_ = [("regions", C.c_int64), ("rings", C.c_int64), ("segments", C.c_int64), ("max_cell_candidates", C.c_int64), ("grid", C.c_int32),
                ("tile_segments", C.c_int32), ("x0", C.c_double), ("y0", C.c_double), ("x1", C.c_double), ("y1", C.c_double)]


class LocateInfo(C.Structure):
    """struct dge_locate_info (include/dge.h) — what dge_regions_locate / dge_regions_locate_device report."""
    _fields_ = [("points", C.c_int64), ("located", C.c_int64), ("on_boundary", C.c_int64), ("multi", C.c_int64), ("outside", C.c_int64), ("exact", C.c_int64),
                ("kernel_ms", C.c_double)]


class FlowsInfo(C.Structure):
    """struct dge_flows_info (include/dge.h) — accumulated over the calls that added trips."""
    _fields_ = [("trips", C.c_int64), ("mapped", C.c_int64), ("bad", C.c_int64), ("no_start", C.c_int64), ("no_end", C.c_int64), ("entries", C.c_int64),
                ("located", C.c_int64), ("on_boundary", C.c_int64), ("multi", C.c_int64), ("outside", C.c_int64), ("exact", C.c_int64), ("kernel_ms", C.c_double)]


class TripTextOptions(C.Structure):
    """struct dge_trip_text_options (include/dge.h)."""
    _fields_ = [("format", C.c_int32), ("header", C.c_int32), ("slab_bytes", C.c_int64)]


class TripTextInfo(C.Structure):
    """struct dge_trip_text_info (include/dge.h) — what dge_trips_parse_texts / dge_flows_add_trip_texts / dge_flows_add_trip_files report."""
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("header_lines", C.c_int64), ("ok", C.c_int64), ("bad_fields", C.c_int64), ("bad_parse", C.c_int64),
                ("too_long", C.c_int64), ("host_values", C.c_int64), ("slabs", C.c_int64), ("read_ms", C.c_double), ("kernel_ms", C.c_double)]


class SpatialInfo(C.Structure):
    """struct dge_spatial_info (include/dge.h) — what dge_graph_add_spatial / dge_graph_add_spatial_points report."""
    _fields_ = [("regions", C.c_int64), ("edges", C.c_int64), ("weights", C.c_int64), ("zero_weights", C.c_int64), ("kernel_ms", C.c_double)]


class KmeansCfg(C.Structure):
    """struct dge_kmeans_cfg (include/dge.h)."""
    _fields_ = [("k", C.c_int32), ("n_init", C.c_int32), ("max_iter", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class KmeansInfo(C.Structure):
    """struct dge_kmeans_info (include/dge.h) — what dge_kmeans_vectors / dge_kmeans report."""
    _fields_ = [("rows", C.c_int64), ("best_restart", C.c_int32), ("iterations", C.c_int32), ("total_iterations", C.c_int64), ("scale_bits", C.c_int32),
                ("empty", C.c_int32), ("inertia", C.c_double), ("kernel_ms", C.c_double)]


class NmfCfg(C.Structure):
    """struct dge_nmf_cfg (include/dge.h)."""
    _fields_ = [("rank", C.c_int32), ("max_iter", C.c_int32), ("update", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class NmfInfo(C.Structure):
    """struct dge_nmf_info (include/dge.h) — what dge_nmf_coo / dge_nmf_flows report."""
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int64), ("entries", C.c_int64), ("zeros", C.c_int64), ("iterations", C.c_int32), ("reserved", C.c_int32),
                ("vmax", C.c_double), ("objective", C.c_double), ("kernel_ms", C.c_double)]


class LineCfg(C.Structure):
    """struct dge_line_cfg (include/dge.h)."""
    _fields_ = [("dim", C.c_int32), ("order", C.c_int32), ("negative", C.c_int32), ("batch", C.c_int32), ("samples", C.c_int64), ("rho0", C.c_double), ("seed", C.c_uint64)]


class LineInfo(C.Structure):
    """struct dge_line_info (include/dge.h) — what dge_line_coo / dge_line_flows report."""
    _fields_ = [("vertices", C.c_int64), ("entries", C.c_int64), ("zeros", C.c_int64), ("batches", C.c_int64), ("samples", C.c_int64), ("total_weight", C.c_int64),
                ("neg_total", C.c_int64), ("max_abs", C.c_double), ("kernel_ms", C.c_double)]


class TreeCfg(C.Structure):
    """struct dge_tree_cfg (include/dge.h)."""
    _fields_ = [("max_depth", C.c_int32), ("min_samples_split", C.c_int32), ("min_samples_leaf", C.c_int32), ("reserved", C.c_int32)]


class TreeInfo(C.Structure):
    """struct dge_tree_info (include/dge.h) — what dge_tree_fit* / dge_tree_cv* report."""
    _fields_ = [("rows", C.c_int64), ("n_nodes", C.c_int64), ("depth", C.c_int32), ("levels", C.c_int32), ("trees", C.c_int32), ("batches", C.c_int32),
                ("kernel_ms", C.c_double)]


class RidgeInfo(C.Structure):
    """struct dge_ridge_info (include/dge.h) — what dge_ridge_loo_vectors / dge_ridge_loo report."""
    _fields_ = [("rows", C.c_int64), ("blocks", C.c_int64), ("chunks", C.c_int64), ("min_pivot", C.c_double), ("max_leverage", C.c_double), ("kernel_ms", C.c_double)]


class SvmCfg(C.Structure):
    """struct dge_svm_cfg (include/dge.h)."""
    _fields_ = [("C", C.c_double), ("gamma", C.c_double), ("eps", C.c_double), ("max_iter", C.c_int64), ("state", C.c_int32), ("launch_iters", C.c_int32)]


class SvmInfo(C.Structure):
    """struct dge_svm_info (include/dge.h) — what dge_svm_fit* / dge_svm_cv* report."""
    _fields_ = [("rows", C.c_int64), ("problems", C.c_int64), ("iterations", C.c_int64), ("max_iterations", C.c_int64), ("not_converged", C.c_int64),
                ("support", C.c_int64), ("kernel_bytes", C.c_int64), ("launches", C.c_int64), ("kernel_ms", C.c_double)]


class PairwiseInfo(C.Structure):
    """struct dge_pairwise_info (include/dge.h) — what dge_pairwise_eval_vectors reports."""
    _fields_ = [("regions", C.c_int64), ("members", C.c_int64), ("tested", C.c_int64), ("threshold_keys", C.c_int64), ("knn_ms", C.c_double),
                ("ground_ms", C.c_double), ("score_ms", C.c_double)]


class HourWindow(C.Structure):
    """struct dge_hour_window (include/dge.h): the hours start, start + 1, .., start + hours - 1, each mod 24."""
    _fields_ = [("start", C.c_int32), ("hours", C.c_int32)]


class TripletRule(C.Structure):
    """struct dge_triplet_rule (include/dge.h): five windows, two minima and the ratio of the triplet search."""
    _fields_ = [("A", HourWindow), ("B", HourWindow), ("C", HourWindow), ("D", HourWindow), ("E", HourWindow), ("min_a", C.c_int64), ("min_b", C.c_int64),
                ("ratio", C.c_int32), ("reserved", C.c_int32)]


class TripletInfo(C.Structure):
    """struct dge_triplet_info (include/dge.h) — what dge_flows_triplets reports."""
    _fields_ = [("pairs_12", C.c_int64), ("pairs_23", C.c_int64), ("pairs_31", C.c_int64), ("candidates", C.c_int64), ("triplets", C.c_int64), ("kernel_ms", C.c_double)]


class FlowSlices(C.Structure):
    """struct dge_flow_slices (include/dge.h): K == 0 — the slots of (T, mode); K >= 1 — the windows win[0 .. K), T = mode = 0."""
    _fields_ = [("T", C.c_int32), ("mode", C.c_int32), ("K", C.c_int32), ("reserved", C.c_int32), ("win", C.POINTER(HourWindow))]


class FlowTextInfo(C.Structure):
    """struct dge_flow_text_info (include/dge.h) — what the flow table's text writers report."""
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("edges", C.c_int64), ("zeros", C.c_int64), ("slices", C.c_int32), ("reserved", C.c_int32),
                ("kernel_ms", C.c_double), ("write_ms", C.c_double)]


class MatrixReadOptions(C.Structure):
    """struct dge_matrix_read_options (include/dge.h): sep is the byte's code; slab_bytes 0 is the default."""
    _fields_ = [("sep", C.c_int32), ("reserved", C.c_int32), ("slab_bytes", C.c_int64)]


class MatrixReadInfo(C.Structure):
    """struct dge_matrix_read_info (include/dge.h) — what dge_flows_add_matrix_texts / dge_flows_add_matrix_files report."""
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("rows", C.c_int64), ("values", C.c_int64), ("entries", C.c_int64), ("zeros", C.c_int64),
                ("total", C.c_int64), ("pieces", C.c_int32), ("n", C.c_int32), ("tile_bytes", C.c_int32), ("slabs", C.c_int32), ("read_ms", C.c_double),
                ("kernel_ms", C.c_double)]


class CountsInfo(C.Structure):
    """struct dge_counts_info (include/dge.h)."""
    _fields_ = [("regions", C.c_int64), ("cols", C.c_int64), ("nonzero", C.c_int64), ("total", C.c_int64)]


class TableReadOptions(C.Structure):
    """struct dge_table_read_options (include/dge.h): sep is the byte's code; neg_col_offset -1 refuses a signed key; slab_bytes 0 is the default."""
    _fields_ = [("sep", C.c_int32), ("skip_lines", C.c_int32), ("key_field", C.c_int32), ("key_lo", C.c_int32), ("key_hi", C.c_int32), ("col_lo", C.c_int32),
                ("n_cols", C.c_int32), ("col_offset", C.c_int32), ("neg_col_offset", C.c_int32), ("reserved", C.c_int32), ("slab_bytes", C.c_int64),
                ("reserved2", C.c_int64)]


class TableReadInfo(C.Structure):
    """struct dge_table_read_info (include/dge.h) — what dge_counts_add_table_texts / dge_counts_add_table_files report."""
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("skipped", C.c_int64), ("empty", C.c_int64), ("rows", C.c_int64), ("foreign", C.c_int64),
                ("values", C.c_int64), ("total", C.c_int64), ("pieces", C.c_int32), ("slabs", C.c_int32), ("read_ms", C.c_double), ("kernel_ms", C.c_double)]


DGE_SLOTS_EVEN, DGE_SLOTS_AS_TRACTS = 0, 1
DGE_COUNTS_PRESENT_ALL, DGE_COUNTS_PRESENT_NONZERO = 0, 1
DGE_FLOW_TEXT_OD, DGE_FLOW_TEXT_OD_LAYERED, DGE_FLOW_TEXT_MATRIX = 0, 1, 2
DGE_NMF_DIVERGENCE, DGE_NMF_EUCLIDEAN = 0, 1
DGE_TRIPS_TYPE1, DGE_TRIPS_TYPE2, DGE_TRIPS_TYPE3 = 1, 2, 3

# every symbol include/dge.h declares: name -> (restype, argtypes)
_vp, _i32, _i64, _dbl, _int = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_int
_P = C.POINTER
SIGNATURES = {
    "dge_last_error": (C.c_char_p, []),
    "dge_version": (_int, []),
    "dge_build_stamp": (C.c_char_p, []),
    "dge_device_count": (_int, [_P(_int)]),
    "dge_graph_create": (_int, [_P(_vp), _int]),
    "dge_graph_free": (None, [_vp]),
    "dge_graph_set_stream": (_int, [_vp, _vp]),
    "dge_graph_add_edges": (_int, [_vp, _vp, _vp, _vp, _i64]),
    "dge_graph_add_edges_device": (_int, [_vp, _vp, _vp, _vp, _i64]),
    "dge_graph_set_sources": (_int, [_vp, _vp, _i64, _int]),
    "dge_graph_reserve_vertices": (_int, [_vp, _i32]),
    "dge_graph_set_out_degree": (_int, [_vp, _vp, _i32]),
    "dge_graph_set_source_weight_sum": (_int, [_vp, _dbl]),
    "dge_graph_get_csr": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64]),
    "dge_graph_keep_top_k": (_int, [_vp, _i32]),
    "dge_graph_build_alias": (_int, [_vp, _int]),
    "dge_graph_num_vertices": (_int, [_vp, _P(_i32)]),
    "dge_graph_num_edges": (_int, [_vp, _P(_i64)]),
    "dge_graph_get_alias": (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _P(_i32), _P(_dbl)]),
    "dge_graph_get_source_alias": (_int, [_vp, _vp, _vp, _vp, _i32, _P(_i32), _P(_dbl)]),
    "dge_graph_sample_next": (_int, [_vp, _i32, _dbl, _P(_i32)]),
    "dge_graph_add_od_files": (_int, [_vp, _vp, _i32, _vp, _P(OdInfo)]),
    "dge_graph_add_od_texts": (_int, [_vp, _vp, _vp, _i32, _vp, _P(OdInfo)]),
    "dge_graph_regions": (_int, [_vp, _vp, _i64, _P(_i64)]),
    "dge_regions_create": (_int, [_int, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _P(_vp)]),
    "dge_regions_info": (_int, [_vp, _P(RegionsInfo)]),
    "dge_regions_locate": (_int, [_vp, _vp, _i64, _vp, _P(LocateInfo)]),
    "dge_regions_locate_device": (_int, [_vp, _vp, _i64, _vp, _P(LocateInfo)]),
    "dge_regions_free": (None, [_vp]),
    "dge_flows_create": (_int, [_vp, _P(_vp)]),
    "dge_flows_add_trips": (_int, [_vp, _vp, _vp, _vp, _i64]),
    "dge_flows_add_trips_device": (_int, [_vp, _vp, _vp, _vp, _i64]),
    "dge_flows_info": (_int, [_vp, _P(FlowsInfo)]),
    "dge_flows_to_host": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _P(_i64)]),
    "dge_flows_slot_edges": (_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _P(_i64)]),
    "dge_flows_free": (None, [_vp]),
    "dge_graph_add_flows": (_int, [_vp, _vp, _i32, _i32, _vp, _P(OdInfo)]),
    "dge_flows_add_entries": (_int, [_vp, _vp, _vp, _vp, _vp, _i64]),
    "dge_flows_window_edges": (_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _P(_i64)]),
    "dge_graph_add_flow_windows": (_int, [_vp, _vp, _vp, _i32, _vp, _P(OdInfo)]),
    "dge_triplet_rule_default": (_int, [_P(TripletRule)]),
    "dge_triplet_rule_check": (_int, [_P(TripletRule), _vp, _P(_i32)]),
    "dge_flows_triplets": (_int, [_vp, _P(TripletRule), _vp, _vp, _vp, _i64, _P(_i64), _P(TripletInfo)]),
    "dge_flows_to_text": (_int, [_vp, _P(FlowSlices), _i32, _i32, _vp, _i32, _vp, _i64, _P(_i64), _P(FlowTextInfo)]),
    "dge_flows_write_text": (_int, [_vp, _P(FlowSlices), _i32, _vp, _i32, _vp, _i32, _P(FlowTextInfo)]),
    "dge_flows_time_series": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _P(_i64)]),
    "dge_flows_time_series_text": (_int, [_vp, _vp, _vp, _i64, _P(_i64), _P(FlowTextInfo)]),
    "dge_flows_write_time_series": (_int, [_vp, _vp, C.c_char_p, _P(FlowTextInfo)]),
    "dge_flows_add_matrix_texts": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _P(MatrixReadOptions), _P(MatrixReadInfo)]),
    "dge_flows_add_matrix_files": (_int, [_vp, _vp, _vp, _i32, _vp, _P(MatrixReadOptions), _P(MatrixReadInfo)]),
    "dge_counts_create": (_int, [_vp, _i32, _P(_vp)]),
    "dge_counts_destroy": (None, [_vp]),
    "dge_counts_info": (_int, [_vp, _P(CountsInfo)]),
    "dge_counts_to_host": (_int, [_vp, _vp]),
    "dge_counts_add_entries": (_int, [_vp, _vp, _vp, _vp, _i64]),
    "dge_counts_add_table_texts": (_int, [_vp, _vp, _vp, _i32, _P(TableReadOptions), _P(TableReadInfo)]),
    "dge_counts_add_table_files": (_int, [_vp, _vp, _i32, _P(TableReadOptions), _P(TableReadInfo)]),
    "dge_counts_add_points": (_int, [_vp, _vp, _vp, _i64, _P(_i64)]),
    "dge_counts_merge": (_int, [_vp, _vp, _vp, _P(_vp)]),
    "dge_counts_vectors": (_int, [_vp, _i32, _i32, _i32, _i32, _P(_vp)]),
    "dge_regions_centroids": (_int, [_vp, _vp, _i64, _P(_i64)]),
    "dge_graph_add_spatial": (_int, [_vp, _vp, _i32, _dbl, _vp, _P(SpatialInfo)]),
    "dge_graph_add_spatial_points": (_int, [_vp, _vp, _vp, _i64, _i32, _dbl, _vp, _P(SpatialInfo)]),
    "dge_trips_parse_texts": (_int, [_int, _vp, _vp, _i32, _P(TripTextOptions), _vp, _vp, _vp, _vp, _i64, _P(_i64), _P(TripTextInfo)]),
    "dge_flows_add_trip_texts": (_int, [_vp, _vp, _vp, _i32, _P(TripTextOptions), _P(TripTextInfo)]),
    "dge_flows_add_trip_files": (_int, [_vp, _vp, _i32, _P(TripTextOptions), _P(TripTextInfo)]),
    "dge_sample_walks": (_int, [_vp, _i64, _i32, _i64, _int, _i64, _vp, _P(_i64)]),
    "dge_sample_walks_device": (_int, [_vp, _i64, _i32, _i64, _int, _i64, _P(_vp), _P(_i64)]),
    "dge_sample_walks_into": (_int, [_vp, _vp, _i64, _i64, _i64, _i64]),
    "dge_walks_from_host": (_int, [_int, _vp, _i64, _i32, _P(_vp)]),
    "dge_names_create": (_int, [_P(_vp)]),
    "dge_names_add": (_int, [_vp, _vp, _i64]),
    "dge_names_count": (_int, [_vp, _P(_i64)]),
    "dge_names_cstrs": (_int, [_vp, _P(_vp)]),
    "dge_names_free": (None, [_vp]),
    "dge_walks_from_seq_text": (_int, [_int, _vp, _i64, _vp, _int, _P(_vp), _P(SeqInfo)]),
    "dge_walks_from_seq_files": (_int, [_int, _vp, _i32, _vp, _int, _P(_vp), _P(SeqInfo)]),
    "dge_walks_to_seq_text": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _i64, _P(_i64), _P(SeqOutInfo)]),
    "dge_walks_write_seq": (_int, [_vp, _i64, _i64, _vp, _int, C.c_char_p, _int, _P(SeqOutInfo)]),
    "dge_walks_to_host": (_int, [_vp, _vp, _i64]),
    "dge_walks_info": (_int, [_vp, _P(_i64), _P(_i32), _P(_vp)]),
    "dge_walks_add_position_prefix": (_int, [_vp, _i32]),
    "dge_walks_free": (None, [_vp]),
    "dge_count_tokens": (_int, [_vp, _i64, _i64, _i32, _vp]),
    "dge_model_create": (_int, [_int, _P(TrainConfig), _vp, _P(_vp)]),
    "dge_model_set_stream": (_int, [_vp, _vp]),
    "dge_model_train": (_int, [_vp, _vp, _i64, _i64, _i64, _i32, _i64, _dbl, _i64]),
    "dge_train_sgns": (_int, [_int, _vp, _i64, _i32, _P(TrainConfig), _P(_vp)]),
    "dge_train_sgns_device": (_int, [_vp, _P(TrainConfig), _P(_vp)]),
    "dge_model_walk_and_train": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _i64, _dbl, _i64]),
    "dge_model_vectors": (_int, [_vp, _P(_vp), _P(_vp), _P(_i64), _P(_i32)]),
    "dge_model_syn1neg": (_int, [_vp, _P(_vp)]),
    "dge_model_syn1": (_int, [_vp, _P(_vp), _P(_i64)]),
    "dge_model_huffman": (_int, [_vp, _P(_vp), _P(_vp), _P(_vp)]),
    "dge_model_counts": (_int, [_vp, _P(_vp)]),
    "dge_model_table": (_int, [_vp, _P(_vp), _P(_i64)]),
    "dge_model_stats": (_int, [_vp, _P(TrainStats)]),
    "dge_model_row_rates": (_int, [_vp, _P(C.c_double), _P(C.c_double), _P(C.c_double), _P(C.c_double)]),
    "dge_model_table_placement": (_int, [_vp, _i32, _vp, _vp, _vp]),
    "dge_model_table_runs": (_int, [_vp, _vp, _vp]),
    "dge_model_tune_placement": (_int, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    "dge_model_placement_search": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "dge_model_reset_stats": (_int, [_vp]),
    "dge_model_schedule": (_int, [_vp, _P(_i32), _P(_i64), _P(_i32)]),
    "dge_model_kernel": (_int, [_vp, C.c_char_p, _i32]),
    "dge_model_pair_loop": (_int, [_vp, _P(_i32), _P(_i32)]),
    "dge_model_lock_stats": (_int, [_vp, _P(_i64), _P(_i64), _P(_i64)]),
    "dge_model_score_pairs": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "dge_model_eval_links": (_int, [_vp, _vp, _i64, _i64, _i32, C.c_uint64, _P(EvalResult)]),
    "dge_model_eval_sgns": (_int, [_vp, _vp, _i64, _i64, C.c_uint64, _P(EvalResult)]),
    "dge_write_vec": (_int, [_vp, _vp, C.c_char_p, _int]),
    "dge_model_free": (None, [_vp]),
    "dge_model_set_partition": (_int, [_vp, _i32, _i32, _i32]),
    "dge_model_partition_floats": (_int, [_vp, _i32, _P(_i64)]),
    "dge_model_export_partition": (_int, [_vp, _int, _i32, _i32, _vp]),
    "dge_model_import_partition": (_int, [_vp, _int, _i32, _i32, _vp]),
    "dge_model_export_partition_async": (_int, [_vp, _int, _i32, _i32, _vp, _vp]),
    "dge_model_import_partition_async": (_int, [_vp, _int, _i32, _i32, _vp, _vp]),
    "dge_model_stream": (_int, [_vp, _P(_vp)]),
    "dge_host_sync_count": (_int, [_P(_i64)]),
    "dge_model_sync_size": (_int, [_vp, _P(_i64)]),
    "dge_model_snapshot": (_int, [_vp]),
    "dge_model_export_delta": (_int, [_vp, _vp]),
    "dge_model_import_delta": (_int, [_vp, _vp, C.c_float]),
    "dge_comm_unique_id": (_int, [_vp]),
    "dge_comm_create": (_int, [_P(_vp), _vp, _int, _int, _int]),
    "dge_comm_free": (None, [_vp]),
    "dge_model_allreduce_deltas": (_int, [_vp, _vp]),
    "dge_model_ring_pass": (_int, [_vp, _vp, _i32]),
    "dge_model_gather_table": (_int, [_vp, _vp, _int]),
    "dge_set_tuning": (_int, [_i32, _i64]),
    "dge_get_tuning": (_int, [_i32, _vp]),
    "dge_ndcg_at_k": (_int, [_int, _vp, _i32, _vp, _i32, _i32, _i32, _P(_dbl), _P(_dbl)]),
    "dge_knn_cosine": (_int, [_int, _vp, _i32, _i32, _i32, _vp, _vp, _P(_dbl)]),
    "dge_vectors_from_vec_text": (_int, [_int, _vp, _i64, _int, _vp, _int, _P(_vp), _P(VecInfo)]),
    "dge_vectors_from_vec_files": (_int, [_int, _vp, _i32, _int, _vp, _int, _P(_vp), _P(VecInfo)]),
    "dge_vectors_from_host": (_int, [_int, _vp, _i64, _i32, _vp, _P(_vp)]),
    "dge_vectors_info": (_int, [_vp, _P(_i64), _P(_i32), _P(_vp), _P(_vp)]),
    "dge_vectors_to_host": (_int, [_vp, _vp, _vp, _i64]),
    "dge_vectors_free": (None, [_vp]),
    "dge_model_load_vectors": (_int, [_vp, _vp, _P(_i64)]),
    "dge_knn_cosine_vectors": (_int, [_vp, _i32, _vp, _vp, _P(_dbl)]),
    "dge_ndcg_at_k_vectors": (_int, [_vp, _vp, _i32, _P(_dbl), _P(_dbl)]),
    "dge_kmeans_vectors": (_int, [_vp, _vp, _P(KmeansCfg), _vp, _vp, _vp, _P(KmeansInfo)]),
    "dge_kmeans": (_int, [_int, _vp, _i64, _i32, _vp, _P(KmeansCfg), _vp, _vp, _vp, _P(KmeansInfo)]),
    "dge_cluster_accuracy": (_int, [_vp, _vp, _i64, _i32, _vp, _vp, _P(_dbl)]),
    "dge_nmf_coo": (_int, [_int, _vp, _vp, _vp, _i64, _i64, _i64, _P(NmfCfg), _vp, _vp, _vp, _vp, _P(NmfInfo)]),
    "dge_nmf_flows": (_int, [_vp, _i32, _i32, _i32, _vp, _P(NmfCfg), _vp, _vp, _vp, _P(NmfInfo)]),
    "dge_line_coo": (_int, [_int, _vp, _vp, _vp, _i64, _i64, _P(LineCfg), _vp, _vp, _vp, _vp, _vp, _P(LineInfo)]),
    "dge_line_flows": (_int, [_vp, _i32, _i32, _i32, _vp, _P(LineCfg), _vp, _vp, _vp, _vp, _P(LineInfo)]),
    "dge_tree_fit_vectors": (_int, [_vp, _vp, _vp, _P(TreeCfg), _i64, _vp, _vp, _vp, _vp, _vp, _P(TreeInfo)]),
    "dge_tree_predict_vectors": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dge_tree_cv_vectors": (_int, [_vp, _vp, _vp, _i32, _P(TreeCfg), _vp, _vp, _vp, _vp, _P(TreeInfo)]),
    "dge_tree_fit": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _P(TreeCfg), _i64, _vp, _vp, _vp, _vp, _vp, _P(TreeInfo)]),
    "dge_tree_cv": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _i32, _P(TreeCfg), _vp, _vp, _vp, _vp, _P(TreeInfo)]),
    "dge_ridge_loo_vectors": (_int, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _P(RidgeInfo)]),
    "dge_ridge_loo": (_int, [_int, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _P(RidgeInfo)]),
    "dge_ridge_predict_vectors": (_int, [_vp, _vp, _i32, _vp]),
    "dge_svm_fit_vectors": (_int, [_vp, _vp, _i32, _vp, _P(SvmCfg), _vp, _vp, _vp, _vp, _P(SvmInfo)]),
    "dge_svm_decision_vectors": (_int, [_vp, _vp, _vp, _i32, C.c_double, _vp, _vp]),
    "dge_svm_cv_vectors": (_int, [_vp, _vp, _i32, _vp, _i32, _P(SvmCfg), _vp, _vp, _vp, _vp, _vp, _vp, _P(SvmInfo)]),
    "dge_svm_fit": (_int, [_int, _vp, _i64, _i32, _vp, _i32, _vp, _P(SvmCfg), _vp, _vp, _vp, _vp, _P(SvmInfo)]),
    "dge_svm_decision": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _i32, C.c_double, _vp, _i64, _vp]),
    "dge_svm_cv": (_int, [_int, _vp, _i64, _i32, _vp, _i32, _vp, _i32, _P(SvmCfg), _vp, _vp, _vp, _vp, _vp, _vp, _P(SvmInfo)]),
    "dge_pairwise_eval_vectors": (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(PairwiseInfo)]),
    "dge_pairwise_ground_vectors": (_int, [_vp, _i32, _vp, _vp]),
    "dge_selftest_locked_rows": (_int, [_int, _i32, _i64, _i32, C.c_uint64, _i32, _P(_i64), _P(_dbl)]),
    "dge_selftest_atomics_wave": (_int, [_int, _i32, _i32, _i32, _i32, _i32, C.c_uint64, _P(_i64), _P(_dbl)]),
    "dge_selftest_atomics_wave_block": (_int, [_int, _i32, _i32, _i32, _i32, _i32, _i32, C.c_uint64, _P(_i64), _P(_dbl)]),
    "dge_selftest_fmt_g9": (_int, [_i64, C.c_uint64, _P(_i64), _P(_i64)]),
    "dge_selftest_hot_add": (_int, [_int, _i32, _i64, _i32, _i32, C.c_uint64, _P(_i64), _P(_dbl)]),
    "dge_selftest_seq_intern": (_int, [_int, _vp, _i64, _i32, _i64, _vp, _i64, _P(_i64), _P(_i64)]),
}


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  The PyTorch-ROCm wheel ships its own libamdhip64.so (SONAME libamdhip64.so.7,
    loaded by file name), libdge.so needs libamdhip64.so.7: if both copies get loaded, the second one finds no
    device.  When torch is installed, load ITS runtime first so libdge.so binds to it by SONAME; torch tensors
    (torch.distributed / RCCL plumbing) and libdge then share streams and memory."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        p = os.path.join(libdir, name)
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "embedding_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    _preload_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (rt, at) in SIGNATURES.items():
        f = getattr(lib, name)      # AttributeError if the library does not export a declared symbol
        f.restype = rt
        f.argtypes = at
    return lib


lib = load()


def check(rc):
    if rc != 0:
        raise DgeError(rc, (lib.dge_last_error() or b"").decode("utf-8", "replace"))
