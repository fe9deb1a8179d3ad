"""Thin object view of the C ABI (include/dge.h).  All compute happens in libdge.so on the GPU."""
import ctypes as C
import os

import numpy as np

from ._native import DGE_COUNTS_PRESENT_ALL, DGE_COUNTS_PRESENT_NONZERO, DGE_ERR_CAP, DGE_FLOW_TEXT_MATRIX, DGE_FLOW_TEXT_OD, DGE_FLOW_TEXT_OD_LAYERED, DGE_SLOTS_AS_TRACTS, DGE_SLOTS_EVEN, CountsInfo, EvalResult, FlowSlices, FlowTextInfo, FlowsInfo, HourWindow, KmeansCfg, KmeansInfo, LocateInfo, MatrixReadInfo, MatrixReadOptions, OdInfo, RegionsInfo, RidgeInfo, SeqInfo, SeqOutInfo, SpatialInfo, SvmCfg, SvmInfo, TableReadInfo, TableReadOptions, TrainConfig, TrainStats, TreeCfg, TreeInfo, TripTextInfo, TripTextOptions, TripletInfo, TripletRule, VecInfo, check, lib
from .evaluate import _info_dict, _select_mask


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


_byref = C.byref             # for the methods that have a parameter named C (the SVM's, as scikit-learn spells it)


def _dev_ptr(t):
    """device pointer of a torch tensor (or a raw int)."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


class DeviceGraph:
    """Edge store + alias tables in HBM (replaces the LayeredGraph store, J/LayeredGraph.java:142-226)."""

    def __init__(self, device=0):
        h = C.c_void_p(0)
        check(lib.dge_graph_create(C.byref(h), int(device)))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib.dge_graph_free(self._h)
            self._h = None

    __del__ = close

    @classmethod
    def from_od(cls, paths_or_list_of_bytes, names=True, device=0):
        """.od flow text -> (graph, names, info): one "src dst w" line per flow, one piece per time slice, parsed and turned into the layered graph on the
        device (include/dge.h: dge_graph_add_od_files / dge_graph_add_od_texts) under the rule of io.read_od_slices; the edges never visit the host.
        paths_or_list_of_bytes: a path (one slice: the static graph), a sequence of paths, or a sequence of texts as bytes / bytearray / memoryview — slice h
        is entry h.  names=True: a new Names receives the T*R vertex names "<h>-<region id>" in vertex-id order; an empty Names of the caller's is filled
        instead; False / None: no names (None is returned in their place).  The graph has its edges, its reserved vertices and its sources: build_alias
        is next.  info: the fields of struct dge_od_info."""
        if names is True:
            names = Names()
        elif not names and not isinstance(names, Names):
            names = None
        g = cls(device)
        inf = OdInfo()
        nh = names._h if names is not None else None
        kind, _keep, ptrs, sizes, n = _piece_args(paths_or_list_of_bytes)
        if kind == "texts":
            check(lib.dge_graph_add_od_texts(g._h, ptrs, sizes, n, nh, C.byref(inf)))
        else:
            check(lib.dge_graph_add_od_files(g._h, ptrs, n, nh, C.byref(inf)))
        return g, names, _info_dict(inf, reserved=False)

    @classmethod
    def from_flows(cls, flows, T, mode=DGE_SLOTS_EVEN, names=True):
        """A Flows table -> (graph, names, info): the slot edges of (T, mode) become the layered graph on the device (include/dge.h: dge_graph_add_flows), exactly
        the graph from_od gives for flows.to_od_bytes(T, mode), with no text in between.  names as in from_od."""
        if names is True:
            names = Names()
        elif not names and not isinstance(names, Names):
            names = None
        g = cls(flows.regions.device)
        inf = OdInfo()
        check(lib.dge_graph_add_flows(g._h, flows._h, int(T), int(mode), names._h if names is not None else None, C.byref(inf)))
        return g, names, _info_dict(inf, reserved=False)

    @classmethod
    def from_flow_windows(cls, flows, windows, names=True):
        """A Flows table and K hour windows [(start, hours), ..] -> (graph, names, info): the window edges become the layered graph on the device (include/dge.h:
        dge_graph_add_flow_windows), exactly the graph from_od gives for the texts of flows.window_edges(windows), slice k = window k.
        from_flow_windows(f, Flows.windows_cross_time(T)) is CrossTimeGraph.constructGraph_tract with numLayer = T (J/CrossTimeGraph.java:25-52) — the graph
        DeepWalk trains on; from_flows(f, T, AS_TRACTS) keeps only the destinations seen in the window's first hour and is not.
        from_flow_windows(f, Flows.windows_from_intervals(iv)) is constructGraph_CA(iv) (:68-95).  names as in from_od."""
        if names is True:
            names = Names()
        elif not names and not isinstance(names, Names):
            names = None
        g = cls(flows.regions.device)
        inf = OdInfo()
        win = _windows(windows)
        check(lib.dge_graph_add_flow_windows(g._h, flows._h, win, len(win), names._h if names is not None else None, C.byref(inf)))
        return g, names, _info_dict(inf, reserved=False)

    @classmethod
    def from_spatial(cls, regions_or_ids_xy, k=10, scale=100.0, names=True, device=0):
        """Regions, or (ids, xy) host arrays of centroids -> (graph, names, info): the spatial graph of SpatialGraph.constructGraph_tract / _CA
        (J/SpatialGraph.java:37-88) built on the device (include/dge.h: dge_graph_add_spatial / dge_graph_add_spatial_points): vertex i is region i, its edges
        the first k candidates under (w descending, j ascending) with w = E(-d * scale) between centroids, all vertices sources.  No R x R matrix exists
        anywhere.  names as in from_od: the decimal region ids in vertex order.  build_alias is next.  info: the fields of struct dge_spatial_info."""
        if names is True:
            names = Names()
        elif not names and not isinstance(names, Names):
            names = None
        nh = names._h if names is not None else None
        inf = SpatialInfo()
        if isinstance(regions_or_ids_xy, Regions):
            g = cls(regions_or_ids_xy.device)
            check(lib.dge_graph_add_spatial(g._h, regions_or_ids_xy._h, int(k), float(scale), nh, C.byref(inf)))
        else:
            ids, xy = regions_or_ids_xy
            ids = np.ascontiguousarray(ids, np.int64); xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
            if len(ids) != len(xy):
                raise ValueError("ids has R entries, xy R x 2")
            g = cls(device)
            check(lib.dge_graph_add_spatial_points(g._h, _ptr(ids), _ptr(xy), len(ids), int(k), float(scale), nh, C.byref(inf)))
        return g, names, _info_dict(inf)

    def regions(self):
        """The R region ids of a graph made by from_od, ascending int64 (vertex h*R + i is region regions()[i] in slice h); empty for any other graph."""
        n = C.c_int64(0)
        rc = lib.dge_graph_regions(self._h, None, 0, C.byref(n))          # a size query: DGE_ERR_CAP with n set when there are regions
        if rc not in (0, DGE_ERR_CAP):
            check(rc)
        out = np.empty(n.value, np.int64)
        if n.value:
            check(lib.dge_graph_regions(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def set_stream(self, stream_ptr):
        check(lib.dge_graph_set_stream(self._h, C.c_void_p(int(stream_ptr))))

    def add_edges(self, src, dst, w):
        src = np.ascontiguousarray(src, np.int32); dst = np.ascontiguousarray(dst, np.int32)
        w = np.ascontiguousarray(w, np.float64)
        if not (len(src) == len(dst) == len(w)):
            raise ValueError("src/dst/w lengths differ")
        check(lib.dge_graph_add_edges(self._h, _ptr(src), _ptr(dst), _ptr(w), len(src)))

    def add_edges_device(self, src_t, dst_t, w_t):
        """src/dst int32, w float64 torch tensors on this device."""
        n = int(src_t.numel())
        check(lib.dge_graph_add_edges_device(self._h, _dev_ptr(src_t), _dev_ptr(dst_t), _dev_ptr(w_t), n))

    def set_sources(self, v, stream_sum=False):
        v = np.ascontiguousarray(v, np.int32)
        check(lib.dge_graph_set_sources(self._h, _ptr(v), len(v), int(bool(stream_sum))))

    def reserve_vertices(self, n):
        check(lib.dge_graph_reserve_vertices(self._h, int(n)))

    def set_out_degree(self, out_degree):
        """Vertex.outDegree values as the host holds them (a public field of the reference), one per vertex."""
        od = np.ascontiguousarray(out_degree, np.float64)
        check(lib.dge_graph_set_out_degree(self._h, _ptr(od), len(od)))

    def set_source_weight_sum(self, s):
        check(lib.dge_graph_set_source_weight_sum(self._h, float(s)))

    def get_csr(self, tables=True):
        """The whole store in CSR order: row_ptr, nbr, weight, out_degree (+ prob, alias when the tables are built)."""
        V, E = self.num_vertices, self.num_edges
        row_ptr = np.zeros(V + 1, np.int64); nbr = np.zeros(max(E, 1), np.int32); wt = np.zeros(max(E, 1), np.float64)
        od = np.zeros(max(V, 1), np.float64)
        prob = np.zeros(max(E, 1), np.float64) if tables else None; alias = np.zeros(max(E, 1), np.int32) if tables else None
        check(lib.dge_graph_get_csr(self._h, _ptr(row_ptr), _ptr(nbr), _ptr(wt), _ptr(prob), _ptr(alias), _ptr(od), V, max(E, 1)))
        E = int(row_ptr[V])
        out = dict(row_ptr=row_ptr, nbr=nbr[:E], weight=wt[:E], out_degree=od[:V])
        if tables:
            out.update(prob=prob[:E], alias=alias[:E])
        return out

    def keep_top_k(self, k):
        check(lib.dge_graph_keep_top_k(self._h, int(k)))

    def build_alias(self, exact=True):
        check(lib.dge_graph_build_alias(self._h, int(bool(exact))))

    @property
    def num_vertices(self):
        n = C.c_int32(0); check(lib.dge_graph_num_vertices(self._h, C.byref(n))); return n.value

    @property
    def num_edges(self):
        n = C.c_int64(0); check(lib.dge_graph_num_edges(self._h, C.byref(n))); return n.value

    def get_alias(self, v, tables=True):
        k = C.c_int32(0); od = C.c_double(0)
        check(lib.dge_graph_get_alias(self._h, int(v), None, None, None, None, 0, C.byref(k), C.byref(od)))
        n = max(k.value, 1)
        prob = np.zeros(n, np.float64); alias = np.zeros(n, np.int32); nbr = np.zeros(n, np.int32); wt = np.zeros(n, np.float64)
        check(lib.dge_graph_get_alias(self._h, int(v), _ptr(prob) if tables else None, _ptr(alias) if tables else None,
                                      _ptr(nbr), _ptr(wt), n, C.byref(k), C.byref(od)))
        kk = k.value
        return dict(prob=prob[:kk], alias=alias[:kk], nbr=nbr[:kk], weight=wt[:kk], out_degree=od.value)

    def get_source_alias(self):
        k = C.c_int32(0); ws = C.c_double(0)
        check(lib.dge_graph_get_source_alias(self._h, None, None, None, 0, C.byref(k), C.byref(ws)))
        n = max(k.value, 1)
        prob = np.zeros(n, np.float64); alias = np.zeros(n, np.int32); src = np.zeros(n, np.int32)
        check(lib.dge_graph_get_source_alias(self._h, _ptr(prob), _ptr(alias), _ptr(src), n, C.byref(k), C.byref(ws)))
        kk = k.value
        return dict(prob=prob[:kk], alias=alias[:kk], src=src[:kk], weight_sum=ws.value)

    def sample_next(self, v, x):
        nxt = C.c_int32(-1)
        check(lib.dge_graph_sample_next(self._h, int(v), float(x), C.byref(nxt)))
        return nxt.value

    def sample_walks(self, n_walks, max_len, seed, rng_mode=1, first_index=0, return_draws=False):
        out = np.empty((int(n_walks), int(max_len)), np.int32)
        draws = C.c_int64(0)
        check(lib.dge_sample_walks(self._h, int(n_walks), int(max_len), int(seed), int(rng_mode), int(first_index),
                                   _ptr(out), C.byref(draws)))
        return (out, draws.value) if return_draws else out

    def sample_walks_device(self, n_walks, max_len, seed, rng_mode=1, first_index=0):
        h = C.c_void_p(0); draws = C.c_int64(0)
        check(lib.dge_sample_walks_device(self._h, int(n_walks), int(max_len), int(seed), int(rng_mode), int(first_index),
                                          C.byref(h), C.byref(draws)))
        return WalkCorpus(h, self.device)

    def sample_walks_into(self, corpus, row0, n_walks, seed, first_index):
        check(lib.dge_sample_walks_into(self._h, corpus._h, int(row0), int(n_walks), int(seed), int(first_index)))


def _windows(windows):
    """[(start, hours), ..] -> a C array of struct dge_hour_window"""
    windows = [(int(a), int(b)) for a, b in windows]
    return (HourWindow * len(windows))(*[HourWindow(a, b) for a, b in windows])


_BYTES = (bytes, bytearray, memoryview)


def _text_args(texts):
    """bytes-like pieces -> (the arrays kept alive, pointer array, size array, count)"""
    if isinstance(texts, _BYTES):
        texts = [texts]
    views = [np.frombuffer(t, np.uint8) for t in texts]
    ptrs = (C.c_void_p * max(len(views), 1))(*[v.ctypes.data if v.size else None for v in views])
    sizes = (C.c_int64 * max(len(views), 1))(*[v.size for v in views])
    return views, ptrs, sizes, len(views)


def _piece_args(x, kind=None):
    """A path, a sequence of paths, a bytes-like or a sequence of bytes-likes -> (kind, the arrays kept alive, pointer array, size array, count), kind "texts"
    or "paths" (no size array then).  kind given: the caller's entry takes only that.  Otherwise texts are a bytes-like or a sequence of nothing but
    bytes-likes; an empty sequence is one of paths."""
    if isinstance(x, (str, os.PathLike)):
        x = [x]
    elif not isinstance(x, _BYTES):
        x = list(x)
    if kind is None:
        kind = "texts" if isinstance(x, _BYTES) or (x and all(isinstance(p, _BYTES) for p in x)) else "paths"
    if kind == "texts":
        return ("texts",) + _text_args(x)
    return "paths", None, (C.c_char_p * max(len(x), 1))(*[os.fsencode(p) for p in x]), None, len(x)


def parse_trips(texts, fmt, header=True, slab_bytes=0, device=0):
    """Taxi trip text -> a dict of arrays, one record per non-header line in text order (include/dge.h: dge_trips_parse_texts): status uint8 (0 ok, 1 wrong
    piece count, 2 a field did not parse, 3 too long), hour int32, start_xy and end_xy float64 [n, 2] (x, y), and info, the fields of struct
    dge_trip_text_info.  texts: one text or a sequence of texts as bytes / bytearray / memoryview, each a piece (a file's bytes); fmt: 1, 2 or 3."""
    views, ptrs, sizes, n = _text_args(texts)
    opt = TripTextOptions(int(fmt), 1 if header else 0, int(slab_bytes))
    inf = TripTextInfo()
    got = C.c_int64(0)
    rc = lib.dge_trips_parse_texts(int(device), ptrs, sizes, n, C.byref(opt), None, None, None, None, 0, C.byref(got), C.byref(inf))          # a size query
    if rc not in (0, DGE_ERR_CAP):
        check(rc)
    m = got.value
    status = np.zeros(m, np.uint8); hour = np.zeros(m, np.int32); s = np.zeros((m, 2), np.float64); e = np.zeros((m, 2), np.float64)
    if m:
        check(lib.dge_trips_parse_texts(int(device), ptrs, sizes, n, C.byref(opt), _ptr(status), _ptr(hour), _ptr(s), _ptr(e), m, C.byref(got), C.byref(inf)))
    return dict(status=status, hour=hour, start_xy=s, end_xy=e, info=_info_dict(inf))


class Regions:
    """Region rings with their cell index in HBM (struct dge_regions, include/dge.h): what Tracts / CommunityAreas hold as JTS MultiPolygons
    (J/Tracts.java:26-43).  Points are located by the exact ray-crossing rule of csrc/pip_exact.h."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = int(device)

    @classmethod
    def from_arrays(cls, ids, ring_first, vert_first, xy, grid=0, device=0):
        """ids int64 [R]; ring_first int64 [R + 1]; vert_first int64 [rings + 1]; xy float64 [verts, 2] (x = longitude, y = latitude).  grid: 0 = the library's
        rule, n > 0 = n x n cells; the result does not depend on it."""
        ids = np.ascontiguousarray(ids, np.int64); ring_first = np.ascontiguousarray(ring_first, np.int64)
        vert_first = np.ascontiguousarray(vert_first, np.int64); xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        if len(ring_first) != len(ids) + 1 or len(vert_first) < 1:
            raise ValueError("ring_first has R + 1 entries, vert_first rings + 1")
        h = C.c_void_p(0)
        check(lib.dge_regions_create(int(device), _ptr(ids), len(ids), _ptr(ring_first), _ptr(vert_first), _ptr(xy), len(vert_first) - 1, len(xy), int(grid), C.byref(h)))
        self = cls(h, device)
        self.ids = ids.copy()              # region index -> id (Flows.nmf names its rows with it)
        return self

    @classmethod
    def from_ids(cls, ids, device=0):
        """Regions that are ids and nothing else: no rings, so no point lies in any of them.  What a host that holds only the reference's sortedId and its
        .matrix or .od files needs to get a Flows (Flows.add_matrix, Flows.add_entries)."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        return cls.from_arrays(ids, np.zeros(len(ids) + 1, np.int64), np.zeros(1, np.int64), np.zeros((0, 2), np.float64), device=device)

    def close(self):
        if getattr(self, "_h", None):
            lib.dge_regions_free(self._h)
            self._h = None

    __del__ = close

    def info(self):
        inf = RegionsInfo()
        check(lib.dge_regions_info(self._h, C.byref(inf)))
        return _info_dict(inf)

    def centroids(self):
        """The regions' centroids, float64 [R, 2] (x, y): JTS's area-weighted centroid of the rings under the rule of include/dge.h, computed on the device on
        first use and kept with the handle (dge_regions_centroids).  A region whose rings have no area: DgeError (DGE_ERR_ARG) naming it."""
        n = C.c_int64(0)
        rc = lib.dge_regions_centroids(self._h, None, 0, C.byref(n))         # a size query: DGE_ERR_CAP with n set when there are regions
        if rc not in (0, DGE_ERR_CAP):
            check(rc)
        out = np.empty((n.value, 2), np.float64)
        if n.value:
            check(lib.dge_regions_centroids(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def locate(self, xy, return_info=False):
        """xy: numpy float64 [n, 2] -> numpy int32 [n]; or a torch float64 tensor on this device -> a torch int32 tensor there.  -1: in no region."""
        inf = LocateInfo()
        if isinstance(xy, np.ndarray) or not hasattr(xy, "data_ptr"):
            xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
            out = np.empty(len(xy), np.int32)
            check(lib.dge_regions_locate(self._h, _ptr(xy), len(xy), _ptr(out), C.byref(inf)))
        else:
            import torch
            xy = xy.contiguous()
            if xy.dtype != torch.float64 or not xy.is_cuda:
                raise ValueError("a device tensor of float64 is expected")
            out = torch.empty(xy.numel() // 2, dtype=torch.int32, device=xy.device)
            check(lib.dge_regions_locate_device(self._h, _dev_ptr(xy), xy.numel() // 2, _dev_ptr(out), C.byref(inf)))
        return (out, _info_dict(inf)) if return_info else out


class Flows:
    """The table (hour, s, e) -> count in HBM (struct dge_flows, include/dge.h): what Tract.taxiFlows holds after Tracts.mapTripsIntoTracts
    (J/Tracts.java:71-102)."""
    EVEN, AS_TRACTS = DGE_SLOTS_EVEN, DGE_SLOTS_AS_TRACTS

    def __init__(self, regions):
        h = C.c_void_p(0)
        check(lib.dge_flows_create(regions._h, C.byref(h)))
        self._h = h
        self.regions = regions

    def close(self):
        if getattr(self, "_h", None):
            lib.dge_flows_free(self._h)
            self._h = None

    __del__ = close

    def add_trips(self, start_xy, end_xy, hour):
        """numpy arrays (float64 [n, 2] twice, int32 [n]) or torch tensors of those types on the regions' device; may be called any number of times."""
        if hasattr(start_xy, "data_ptr") and not isinstance(start_xy, np.ndarray):
            import torch
            s, e, h = start_xy.contiguous(), end_xy.contiguous(), hour.contiguous()
            if s.dtype != torch.float64 or e.dtype != torch.float64 or h.dtype != torch.int32 or not (s.is_cuda and e.is_cuda and h.is_cuda):
                raise ValueError("device tensors of float64, float64 and int32 are expected")
            if not (s.numel() == e.numel() == 2 * h.numel()):
                raise ValueError("start / end / hour lengths differ")
            check(lib.dge_flows_add_trips_device(self._h, _dev_ptr(s), _dev_ptr(e), _dev_ptr(h), h.numel()))
            return
        s = np.ascontiguousarray(start_xy, np.float64).reshape(-1, 2); e = np.ascontiguousarray(end_xy, np.float64).reshape(-1, 2)
        h = np.ascontiguousarray(hour, np.int32)
        if not (len(s) == len(e) == len(h)):
            raise ValueError("start / end / hour lengths differ")
        check(lib.dge_flows_add_trips(self._h, _ptr(s), _ptr(e), _ptr(h), len(h)))

    def add_trip_text(self, texts, fmt, header=True, slab_bytes=0):
        """Taxi trip text (one text or a sequence of texts, bytes-like, each a piece) parsed and added on the device (include/dge.h: dge_flows_add_trip_texts):
        the table stands where add_trips leaves it on the status-0 records of the text.  -> the fields of struct dge_trip_text_info"""
        _, _keep, ptrs, sizes, n = _piece_args(texts, "texts")
        opt = TripTextOptions(int(fmt), 1 if header else 0, int(slab_bytes))
        inf = TripTextInfo()
        check(lib.dge_flows_add_trip_texts(self._h, ptrs, sizes, n, C.byref(opt), C.byref(inf)))
        return _info_dict(inf)

    def add_trip_files(self, paths, fmt, header=True, slab_bytes=0):
        """The same for trip files (one path or a sequence), streamed from disk: dge_flows_add_trip_files."""
        _, _keep, arr, _, n = _piece_args(paths, "paths")
        opt = TripTextOptions(int(fmt), 1 if header else 0, int(slab_bytes))
        inf = TripTextInfo()
        check(lib.dge_flows_add_trip_files(self._h, arr, n, C.byref(opt), C.byref(inf)))
        return _info_dict(inf)

    def info(self):
        inf = FlowsInfo()
        check(lib.dge_flows_info(self._h, C.byref(inf)))
        return _info_dict(inf)

    def to_host(self):
        """-> hour int32, src int32, dst int32 (region indices), count int64: ascending by (hour, src, dst)."""
        n = self.info()["entries"]
        hour = np.empty(n, np.int32); src = np.empty(n, np.int32); dst = np.empty(n, np.int32); count = np.empty(n, np.int64)
        got = C.c_int64(0)
        check(lib.dge_flows_to_host(self._h, _ptr(hour), _ptr(src), _ptr(dst), _ptr(count), n, C.byref(got)))
        return hour, src, dst, count

    def slot_edges(self, T, mode=DGE_SLOTS_EVEN):
        """-> slot int32, src id int64, dst id int64, w int64: ascending by (slot, src id, dst id)."""
        n = C.c_int64(0)
        rc = lib.dge_flows_slot_edges(self._h, int(T), int(mode), None, None, None, None, 0, C.byref(n))          # a size query
        if rc not in (0, DGE_ERR_CAP):
            check(rc)
        m = n.value
        slot = np.empty(m, np.int32); src = np.empty(m, np.int64); dst = np.empty(m, np.int64); w = np.empty(m, np.int64)
        if m:
            check(lib.dge_flows_slot_edges(self._h, int(T), int(mode), _ptr(slot), _ptr(src), _ptr(dst), _ptr(w), m, C.byref(n)))
        return slot, src, dst, w

    def add_entries(self, hour, src, dst, count):
        """Table entries back in (include/dge.h: dge_flows_add_entries; replaces Tracts.deserialzeTracts, J/Tracts.java:115-125): hour int32 in 0 .. 23, src /
        dst int32 region INDICES, count int64 >= 1 — what to_host() gave, in any order, with repeats, over any number of calls.  The table stands where
        add_trips leaves it on `count` trips per entry."""
        h = np.ascontiguousarray(hour, np.int32); s = np.ascontiguousarray(src, np.int32); d = np.ascontiguousarray(dst, np.int32); c = np.ascontiguousarray(count, np.int64)
        if not (h.shape == s.shape == d.shape == c.shape and h.ndim == 1):
            raise ValueError("hour / src / dst / count are four arrays of one length")
        check(lib.dge_flows_add_entries(self._h, _ptr(h), _ptr(s), _ptr(d), _ptr(c), len(h)))

    def add_matrix(self, paths_or_bytes, hours, sep=",", select=None, slab_bytes=0):
        """.matrix adjacency text read and added on the device (include/dge.h: dge_flows_add_matrix_texts / dge_flows_add_matrix_files): one piece — a path, or a
        bytes-like — or a sequence of pieces, and for each its hour (0 .. 23; an int for one piece).  A piece is n lines of n decimals joined by sep (",", " "
        or a tab) over all regions in ascending id or those select marks, as matrix_text writes them; value j of line i, when > 0, adds itself to the count
        of (hour, r_i, r_j).  The table stands where add_entries leaves it on those entries; on any error (DgeError naming kind, piece, offset, line and
        column of the first offence) it is as it was.  -> the fields of struct dge_matrix_read_info.

        What replaces matrixFactorization_tract.NMFfeatures (np.loadtxt of taxi-h%d.matrix, f[idx,:][:,idx], NMF) for a host that holds sortedId, the 24
        files and the mask of the tracts it keeps:
            flows = Flows(Regions.from_ids(sortedId))
            flows.add_matrix(["taxi-h%d.matrix" % h for h in range(24)], range(24))
            W, H, ids, info = flows.nmf(slot, T=24, select=mask)"""
        kind, _keep, ptrs, sizes, n = _piece_args(paths_or_bytes)
        hours = np.ascontiguousarray([hours] if np.isscalar(hours) else list(hours), np.int32)
        if len(hours) != n:
            raise ValueError("one hour per piece is needed")
        opt = MatrixReadOptions(ord(sep), 0, int(slab_bytes))
        select = self._select(select)
        inf = MatrixReadInfo()
        if kind == "texts":
            check(lib.dge_flows_add_matrix_texts(self._h, ptrs, sizes, _ptr(hours), n, _ptr(select), C.byref(opt), C.byref(inf)))
        else:
            check(lib.dge_flows_add_matrix_files(self._h, ptrs, _ptr(hours), n, _ptr(select), C.byref(opt), C.byref(inf)))
        return _info_dict(inf)

    @staticmethod
    def windows_cross_time(T):
        """The windows of CrossTimeGraph.constructGraph_tract with numLayer = T (J/CrossTimeGraph.java:31-36): window h starts at hour h and holds 24 // T hours."""
        T = int(T)
        if not 1 <= T <= 24:
            raise ValueError("1 <= T <= 24")
        return [(h, 24 // T) for h in range(T)]

    @staticmethod
    def windows_from_intervals(intervals):
        """constructGraph_CA(int[] timeIntervals) (J/CrossTimeGraph.java:68-95): window h is CommunityArea.getFlowTo(dst, iv[h], iv[h + 1]) — exclusive
        high, wrapping past midnight (J/CommunityAreas.java:240-245): (iv[h], (iv[h + 1] - iv[h]) mod 24).  iv[h] == iv[h + 1] is an empty window, as there."""
        iv = [int(v) for v in intervals]
        if len(iv) < 2 or not all(0 <= v <= 23 for v in iv):
            raise ValueError("two hours at least, each in 0 .. 23")
        return [(lo, (hi - lo) % 24) for lo, hi in zip(iv[:-1], iv[1:])]

    @staticmethod
    def windows_ca_default(num_layer):
        """The windows constructGraph_CA() gets from the interval array it builds, as written (J/CrossTimeGraph.java:54-61), quirks kept: only every
        (24 // numLayer)-th entry of the array is set, to (i * timeStep) % numLayer, the others stay 0.  numLayer = 24 gives the 24 one-hour windows."""
        n = int(num_layer)
        if not 1 <= n <= 24:
            raise ValueError("1 <= num_layer <= 24")
        step = 24 // n
        iv = [0] * (n + 1)
        for i in range(0, n + 1, step):
            iv[i] = (i * step) % n
        return Flows.windows_from_intervals(iv)

    def window_edges(self, windows):
        """K hour windows [(start, hours), ..] -> k int32, src id int64, dst id int64, w int64: the sums of the table over each window's hours where they are
        > 0, ascending by (k, src id, dst id) (include/dge.h: dge_flows_window_edges).  Windows may overlap, repeat and be empty."""
        win = _windows(windows)
        n = C.c_int64(0)
        rc = lib.dge_flows_window_edges(self._h, win, len(win), None, None, None, None, 0, C.byref(n))          # a size query
        if rc not in (0, DGE_ERR_CAP):
            check(rc)
        m = n.value
        k = np.empty(m, np.int32); src = np.empty(m, np.int64); dst = np.empty(m, np.int64); w = np.empty(m, np.int64)
        if m:
            check(lib.dge_flows_window_edges(self._h, win, len(win), _ptr(k), _ptr(src), _ptr(dst), _ptr(w), m, C.byref(n)))
        return k, src, dst, w

    @staticmethod
    def triplet_rule(**kw):
        """The default rule of the triplet search (the reference's constants) with the given fields replaced: A .. E as (start, hours), min_a, min_b, ratio."""
        r = TripletRule()
        check(lib.dge_triplet_rule_default(C.byref(r)))
        for name, v in kw.items():
            if name in "ABCDE" and len(name) == 1:
                setattr(r, name, HourWindow(int(v[0]), int(v[1])))
            elif name in ("min_a", "min_b", "ratio"):
                setattr(r, name, int(v))
            else:
                raise TypeError("triplet_rule has no field %r" % name)
        return r

    def triplets(self, rule=None, return_info=False):
        """The brute-force triplet search (include/dge.h: dge_flows_triplets; replaces Tracts.bruteForceSearchCase, J/Tracts.java:371-415) as a directed-triangle
        listing on the device: -> int64 [n, 3], the (residence, office, night life) region ids that pass the ten conditions, ascending.  rule: None (the
        reference's constants), a TripletRule, or a dict of the fields triplet_rule takes.  return_info: also the fields of struct dge_triplet_info."""
        if isinstance(rule, dict):
            rule = Flows.triplet_rule(**rule)
        rp = C.byref(rule) if rule is not None else None
        n = C.c_int64(0)
        inf = TripletInfo()
        rc = lib.dge_flows_triplets(self._h, rp, None, None, None, 0, C.byref(n), C.byref(inf))          # a size query
        if rc not in (0, DGE_ERR_CAP):
            check(rc)
        m = n.value
        a = np.empty(m, np.int64); b = np.empty(m, np.int64); c = np.empty(m, np.int64)
        if m:
            check(lib.dge_flows_triplets(self._h, rp, _ptr(a), _ptr(b), _ptr(c), m, C.byref(n), C.byref(inf)))
        out = np.stack([a, b, c], 1) if m else np.empty((0, 3), np.int64)
        return (out, _info_dict(inf)) if return_info else out

    def nmf(self, slot, T=8, mode=DGE_SLOTS_EVEN, select=None, **kw):
        """NMF of the flow matrix of one slot (dge_nmf_flows; the rule of include/dge.h): V[src][dst] = w over the edges slot_edges(T, mode) gives for `slot`,
        restricted to the regions select marks (one entry per region, by region index; None: all) and re-indexed in ascending region index — what the reference
        gets from outputAdjacencyMatrix, np.loadtxt and the idx sub-matrix (P/matrixFactorization_tract.py:32-38), built on the device from the resident table.
        kw: rank, max_iter, update, seed as evaluate.nmf_gpu takes them.  nmf(0, T=1) factors taxi-all.matrix.
        -> (W float64 [n x rank], H float64 [rank x n], region_ids int64 [n], info)"""
        from ._native import NmfInfo
        from .evaluate import nmf_config
        cfg = nmf_config(**kw)
        R = self.regions.info()["regions"]
        if select is not None:
            select = np.ascontiguousarray(np.asarray(select) != 0, np.uint8)
            if select.shape != (R,):
                raise ValueError("select must hold one entry per region")
        n = R if select is None else int(select.sum())
        rank = max(cfg.rank, 0)
        W = np.empty((n, rank), np.float64); H = np.empty((rank, n), np.float64); index = np.empty(n, np.int64); inf = NmfInfo()
        check(lib.dge_nmf_flows(self._h, int(T), int(mode), int(slot), _ptr(select), C.byref(cfg), _ptr(W), _ptr(H), _ptr(index), C.byref(inf)))
        ids = getattr(self.regions, "ids", None)
        info = _info_dict(inf, reserved=False)
        info["region_index"] = index
        return W, H, (ids[index] if ids is not None else index), info

    def line(self, slot, T=8, mode=DGE_SLOTS_EVEN, select=None, **kw):
        """LINE on the flow graph of one slot (dge_line_flows; the rule of include/dge.h): the edges slot_edges(T, mode) gives for `slot`, restricted to the
        regions select marks (one entry per region, by region index; None: all) and re-indexed in ascending region index, exactly as Flows.nmf takes them; the
        graph is built on the device from the resident table.  kw: dim, order, negative, samples, batch, rho0, seed as evaluate.line_gpu takes them.
        line(0, T=1) trains on taxi-all.od.
        -> (X float64 [n x dim], Y float64 [n x dim], touched bool [n], region_ids int64 [n], info)"""
        from ._native import LineInfo
        from .evaluate import line_config
        cfg = line_config(**kw)
        R = self.regions.info()["regions"]
        if select is not None:
            select = np.ascontiguousarray(np.asarray(select) != 0, np.uint8)
            if select.shape != (R,):
                raise ValueError("select must hold one entry per region")
        n = R if select is None else int(select.sum())
        dim = max(cfg.dim, 0)
        X = np.empty((n, dim), np.float64); Y = np.empty((n, dim), np.float64); touched = np.empty(n, np.uint8); index = np.empty(n, np.int64); inf = LineInfo()
        check(lib.dge_line_flows(self._h, int(T), int(mode), int(slot), _ptr(select), C.byref(cfg), _ptr(X), _ptr(Y), _ptr(touched), _ptr(index), C.byref(inf)))
        ids = getattr(self.regions, "ids", None)
        info = _info_dict(inf)
        info["region_index"] = index
        return X, Y, touched.astype(bool), (ids[index] if ids is not None else index), info

    # ---- the table out as text, sized and spelled on the device (include/dge.h: "flow table out as text")
    def _slices(self, T, mode, windows):
        """(T, mode) or windows -> (struct dge_flow_slices, what it points at, the number of slices)"""
        if windows is not None:
            if T is not None:
                raise ValueError("T or windows, not both")
            win = _windows(windows)
            return FlowSlices(0, 0, len(win), 0, C.cast(win, C.POINTER(HourWindow))), win, len(win)
        if T is None:
            raise ValueError("T or windows is needed")
        return FlowSlices(int(T), int(mode), 0, 0, None), None, int(T)

    def _select(self, select):
        if select is None:
            return None
        select = np.ascontiguousarray(np.asarray(select) != 0, np.uint8)
        if select.shape != (self.regions.info()["regions"],):
            raise ValueError("select must hold one entry per region")
        return select

    def _text(self, sl, kind, k, select, sep, return_info=False):
        need = C.c_int64(0); inf = FlowTextInfo()
        check(lib.dge_flows_to_text(self._h, C.byref(sl), kind, k, _ptr(select), sep, None, 0, C.byref(need), None))          # a size query
        buf = np.empty(max(need.value, 1), np.uint8)
        check(lib.dge_flows_to_text(self._h, C.byref(sl), kind, k, _ptr(select), sep, _ptr(buf), need.value, C.byref(need), C.byref(inf)))
        text = buf[:need.value].tobytes()
        return (text, _info_dict(inf)) if return_info else text

    def _write(self, paths, sl, kind, select, sep):
        if isinstance(paths, (str, os.PathLike)):
            paths = [paths]
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        inf = FlowTextInfo()
        check(lib.dge_flows_write_text(self._h, C.byref(sl), kind, _ptr(select), sep, arr, len(paths), C.byref(inf)))
        return _info_dict(inf)

    def od_text(self, T=None, mode=DGE_SLOTS_EVEN, windows=None, layered=False):
        """The .od texts of the slots (T, mode) or of the hour windows [(start, hours), ..] (dge_flows_to_text; J/Tracts.java:236-264): a list of bytes, one per
        slice, the lines "src dst w" ascending by (src id, dst id).  layered: ONE bytes for all slices, the lines "k-src (k+1)%S-dst w"
        (outputEdgeGraph_crossInterval, J/Tracts.java:314-330).  od_text(T=1) is [taxi-all.od].  Every text is a size query and a call, and each forms the
        edges: for many slices of a large table write_od, which forms them once, is the way."""
        sl, _keep, S = self._slices(T, mode, windows)
        if layered:
            return self._text(sl, DGE_FLOW_TEXT_OD_LAYERED, 0, None, 0)
        return [self._text(sl, DGE_FLOW_TEXT_OD, k, None, 0) for k in range(S)]

    def write_od(self, paths, T=None, mode=DGE_SLOTS_EVEN, windows=None, layered=False):
        """The same texts into files, one path per slice (one path when layered); the edges are formed once (dge_flows_write_text).  Files are created or
        truncated, in slice order.  -> the fields of struct dge_flow_text_info, summed over the files"""
        sl, _keep, _ = self._slices(T, mode, windows)
        return self._write(paths, sl, DGE_FLOW_TEXT_OD_LAYERED if layered else DGE_FLOW_TEXT_OD, None, 0)

    def matrix_text(self, slice, T=None, mode=DGE_SLOTS_EVEN, windows=None, sep=",", select=None):
        """The .matrix text of one slice (Tracts.outputAdjacencyMatrix, J/Tracts.java:269-301; CommunityAreas', J/CommunityAreas.java:148-166): n lines of n
        decimals, 0 for an absent pair, joined by sep (",", " " or a tab), over all regions in ascending id or those select marks (one entry per region, by
        region index).  Nothing of size n^2 is formed on the device."""
        sl, _keep, _ = self._slices(T, mode, windows)
        return self._text(sl, DGE_FLOW_TEXT_MATRIX, int(slice), self._select(select), ord(sep))

    def write_matrix(self, paths, T=None, mode=DGE_SLOTS_EVEN, windows=None, sep=",", select=None):
        """Every slice's .matrix into its own file -> the fields of struct dge_flow_text_info, summed over the files."""
        sl, _keep, _ = self._slices(T, mode, windows)
        return self._write(paths, sl, DGE_FLOW_TEXT_MATRIX, self._select(select), ord(sep))

    def time_series(self, select=None):
        """Tracts.timeSeries_traffic as numbers (dge_flows_time_series; J/Tracts.java:187-224) -> (ids int64 [n], in int64 [n, 24], out int64 [n, 24]) for the
        regions select marks (None: all), ascending by id.  out sums over ALL destinations, in over the SELECTED sources — the reference's asymmetry, kept.
        ids are region indices when the regions were not made by Regions.from_arrays."""
        select = self._select(select)
        n = C.c_int64(0)
        rc = lib.dge_flows_time_series(self._h, _ptr(select), None, None, None, 0, C.byref(n))          # a size query
        if rc not in (0, DGE_ERR_CAP):
            check(rc)
        m = n.value
        fin = np.zeros((m, 24), np.int64); fout = np.zeros((m, 24), np.int64); index = np.zeros(m, np.int64)
        if m:
            check(lib.dge_flows_time_series(self._h, _ptr(select), _ptr(fin), _ptr(fout), _ptr(index), m, C.byref(n)))
        ids = getattr(self.regions, "ids", None)
        return (ids[index] if ids is not None else index), fin, fout

    def time_series_text(self, select=None):
        """taxi-flow-time-series.txt (dge_flows_time_series_text): two lines per region, "id,in_0,..,in_23" and "-id,out_0,..,out_23"."""
        select = self._select(select)
        need = C.c_int64(0)
        check(lib.dge_flows_time_series_text(self._h, _ptr(select), None, 0, C.byref(need), None))          # a size query
        buf = np.empty(max(need.value, 1), np.uint8)
        check(lib.dge_flows_time_series_text(self._h, _ptr(select), _ptr(buf), need.value, C.byref(need), None))
        return buf[:need.value].tobytes()

    def write_time_series(self, path, select=None):
        """The same text into a file (created or truncated) -> the fields of struct dge_flow_text_info."""
        inf = FlowTextInfo()
        check(lib.dge_flows_write_time_series(self._h, _ptr(self._select(select)), os.fsencode(path), C.byref(inf)))
        return _info_dict(inf)

    def to_od_bytes(self, T, mode=DGE_SLOTS_EVEN):
        """The T .od texts (J/Tracts.java:236-260), formatted on the host from slot_edges: the tables are small."""
        slot, src, dst, w = self.slot_edges(T, mode)
        out = [[] for _ in range(int(T))]
        for k, s, d, x in zip(slot.tolist(), src.tolist(), dst.tolist(), w.tolist()):
            out[k].append(b"%d %d %d\n" % (s, d, x))
        return [b"".join(lines) for lines in out]


class Counts:
    """An int64 table [regions x n_cols] in HBM (struct dge_counts, include/dge.h): the per-tract rows the reference's label builders keep in a dict of numpy
    arrays (getLEHDfeatures_helper, P/embeddingEvaluation_tract.py:512-536, and its siblings).  Row i belongs to the region with the i-th least id.  Every
    call that fills the table stages and commits once: after a DgeError the table is as it was.

    What replaces generateLEHD_ac_clusteringLabel("both") and the KMeans behind it:
        counts = Counts(Regions.from_ids(sortedId), 40)
        counts.add_table("il_rac_S000_JT00_2013.csv", skip_lines=1, key=(5, 11), cols=(8, 20))
        counts.add_table("il_wac_S000_JT00_2013.csv", skip_lines=1, key=(5, 11), cols=(8, 20), col_offset=20)
        labels, centres, info = counts.vectors(present="nonzero").kmeans(k)"""
    ALL, NONZERO = DGE_COUNTS_PRESENT_ALL, DGE_COUNTS_PRESENT_NONZERO

    def __init__(self, regions, n_cols, _handle=None):
        h = _handle
        if h is None:
            h = C.c_void_p(0)
            check(lib.dge_counts_create(regions._h, int(n_cols), C.byref(h)))
        self._h = h
        self.regions = regions
        self.shape = (regions.info()["regions"], int(n_cols))       # (rows, columns): host numbers, no kernel behind them

    def close(self):
        if getattr(self, "_h", None):
            lib.dge_counts_destroy(self._h)
            self._h = None

    __del__ = close

    def info(self):
        inf = CountsInfo()
        check(lib.dge_counts_info(self._h, C.byref(inf)))
        return _info_dict(inf)

    def to_host(self):
        """-> int64 [regions, n_cols]"""
        out = np.zeros(self.shape, np.int64)
        check(lib.dge_counts_to_host(self._h, _ptr(out)))
        return out

    def add_entries(self, row, col, value):
        """row / col int32, value int64 in 0 .. 2^40 — in any order, with repeats: value adds itself to cell (row, col) (dge_counts_add_entries)."""
        r = np.ascontiguousarray(row, np.int32); c = np.ascontiguousarray(col, np.int32); v = np.ascontiguousarray(value, np.int64)
        if not (r.shape == c.shape == v.shape and r.ndim == 1):
            raise ValueError("row / col / value are three arrays of one length")
        check(lib.dge_counts_add_entries(self._h, _ptr(r), _ptr(c), _ptr(v), len(r)))

    def add_table(self, paths_or_bytes, sep=",", skip_lines=0, key_field=0, key=(0, 0), cols=(1, 1), col_offset=0, neg_col_offset=None, slab_bytes=0, return_info=False):
        """Delimited text read and added on the device (include/dge.h: dge_counts_add_table_texts / dge_counts_add_table_files): one piece — a path, or a
        bytes-like — or a sequence of pieces.  Of every line behind the skip_lines headers of its piece the key is characters [key[0], key[1]) of field
        key_field (key[1] == 0: to the field's end), the values are the cols[1] fields from field cols[0] on, and value j adds itself to column
        col_offset + j of the row whose region id is the key.  Lines whose key is no region's id are skipped (info["foreign"]).  neg_col_offset: the column
        the values of a line whose key starts with '-' land at (None: such a key is an offence).  A DgeError names kind, piece, offset, line and field of
        the first offence."""
        kind, _keep, ptrs, sizes, n = _piece_args(paths_or_bytes)
        opt = TableReadOptions(ord(sep), int(skip_lines), int(key_field), int(key[0]), int(key[1]), int(cols[0]), int(cols[1]), int(col_offset),
                               -1 if neg_col_offset is None else int(neg_col_offset), 0, int(slab_bytes), 0)
        inf = TableReadInfo()
        if kind == "texts":
            check(lib.dge_counts_add_table_texts(self._h, ptrs, sizes, n, C.byref(opt), C.byref(inf)))
        else:
            check(lib.dge_counts_add_table_files(self._h, ptrs, n, C.byref(opt), C.byref(inf)))
        return _info_dict(inf) if return_info else None

    def add_points(self, xy, col):
        """xy float64 [n, 2], col int32 [n]: every point located as Regions.locate does adds 1 to (its region's row, col) — Tweets.mapTweetsIntoTracts
        (J/Tweets.java:43-88) with col the hour.  -> the points in no region, which are dropped"""
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2); col = np.ascontiguousarray(col, np.int32)
        if col.shape != (len(xy),):
            raise ValueError("one column per point is needed")
        dropped = C.c_int64(0)
        check(lib.dge_counts_add_points(self._h, _ptr(xy), _ptr(col), len(col), C.byref(dropped)))
        return dropped.value

    def merge(self, groups, group_of):
        """-> a new Counts over the Regions `groups` whose row g is the sum of the rows i with group_of[i] == g; -1 drops a row
        (get_CAfeatures_from_tractFeatures, P/embeddingCaseStudy_CA.py:56-74)."""
        g = np.ascontiguousarray(group_of, np.int32)
        if g.shape != (self.shape[0],):
            raise ValueError("group_of must hold one entry per row")
        h = C.c_void_p(0)
        check(lib.dge_counts_merge(self._h, groups._h, _ptr(g), C.byref(h)))
        return Counts(groups, self.shape[1], _handle=h)

    def vectors(self, cols=None, normalise=True, present="all"):
        """Columns cols = (lo, n) (None: all) as a Vectors of float32 rows: row / row.sum() in float64, rounded once to float32, when normalise, else the
        counts themselves.  present="nonzero" marks only the rows whose sum is not 0, which the evaluators then leave out."""
        lo, n = (0, self.shape[1]) if cols is None else (int(cols[0]), int(cols[1]))
        mode = {"all": DGE_COUNTS_PRESENT_ALL, "nonzero": DGE_COUNTS_PRESENT_NONZERO}[present]
        h = C.c_void_p(0)
        check(lib.dge_counts_vectors(self._h, lo, n, 1 if normalise else 0, mode, C.byref(h)))
        return Vectors(h, self.regions.device)


class Names:
    """Interned token strings, id = position (struct dge_names, include/dge.h): what WalkCorpus.from_seq fills and SgnsModel.write_vec
    takes.  A host object: it needs no device.  Strings are bytes in the library; `list(names)` decodes them as UTF-8 (bytes that are
    not UTF-8 come back as surrogate escapes), `names.as_bytes()` hands them out as they are."""

    def __init__(self, initial=None):
        h = C.c_void_p(0)
        check(lib.dge_names_create(C.byref(h)))
        self._h = h
        if initial:
            self.add(initial)

    def close(self):
        if getattr(self, "_h", None):
            lib.dge_names_free(self._h)
            self._h = None

    __del__ = close

    def add(self, strs):
        """Seed names a host already owns ids for (a graph's vertex names): they take the next ids in the order given.  A duplicate, an
        empty name or one with a whitespace byte is refused (DgeError, code 1) and nothing is added."""
        enc = [s if isinstance(s, bytes) else str(s).encode("utf-8", "surrogateescape") for s in strs]
        arr = (C.c_char_p * len(enc))(*enc)
        check(lib.dge_names_add(self._h, arr, len(enc)))

    def __len__(self):
        n = C.c_int64(0); check(lib.dge_names_count(self._h, C.byref(n))); return n.value

    def _cstrs(self):
        """const char* const* of the library's own strings (borrowed until names are added)."""
        p = C.c_void_p(0); check(lib.dge_names_cstrs(self._h, C.byref(p))); return p

    def as_bytes(self):
        n = len(self)
        if n == 0:
            return []
        arr = C.cast(self._cstrs(), C.POINTER(C.c_char_p))
        return [arr[i] for i in range(n)]

    def __iter__(self):
        return iter([b.decode("utf-8", "surrogateescape") for b in self.as_bytes()])

    def __getitem__(self, i):
        n = len(self)
        if not -n <= i < n:
            raise IndexError(i)
        return C.cast(self._cstrs(), C.POINTER(C.c_char_p))[i % n].decode("utf-8", "surrogateescape")


class WalkCorpus:
    """Walk corpus int32 [n x L] in HBM (replaces the .seq text corpus between J/CrossTimeGraph.java:132-141
    and J/DeepWalk.java:49-56)."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device

    @classmethod
    def from_host(cls, walks, device=0):
        walks = np.ascontiguousarray(walks, np.int32)
        n, L = walks.shape
        h = C.c_void_p(0)
        check(lib.dge_walks_from_host(int(device), _ptr(walks), n, L, C.byref(h)))
        return cls(h, int(device))

    @classmethod
    def from_seq(cls, paths_or_bytes, names=None, intern=True, device=0):
        """.seq text -> (corpus, names, info): tokenised, interned and packed on the device (include/dge.h: dge_walks_from_seq_files /
        dge_walks_from_seq_text).  paths_or_bytes: a path, a sequence of paths (taken in order), or the text itself as bytes / bytearray /
        memoryview.  names: a Names whose entries keep their ids (default: a new, empty one); new names are appended to it in the order of
        their first appearance.  intern=False adds nothing: a token that is not in `names` becomes -1 in its place and is counted in
        info["unknown"].  info: the fields of struct dge_seq_info."""
        if names is None:
            names = Names()
        h = C.c_void_p(0); inf = SeqInfo()
        kind, _keep, ptrs, sizes, n = _piece_args(paths_or_bytes, "texts" if isinstance(paths_or_bytes, _BYTES) else "paths")      # the text comes alone
        if kind == "texts":
            check(lib.dge_walks_from_seq_text(int(device), ptrs[0], sizes[0], names._h, int(bool(intern)), C.byref(h), C.byref(inf)))
        else:
            check(lib.dge_walks_from_seq_files(int(device), ptrs, n, names._h, int(bool(intern)), C.byref(h), C.byref(inf)))
        return cls(h, int(device)), names, _info_dict(inf, reserved=False)

    def close(self):
        if getattr(self, "_h", None):
            lib.dge_walks_free(self._h)
            self._h = None

    __del__ = close

    @property
    def shape(self):
        n = C.c_int64(0); L = C.c_int32(0)
        check(lib.dge_walks_info(self._h, C.byref(n), C.byref(L), None))
        return n.value, L.value

    def to_host(self):
        n, L = self.shape
        out = np.empty((n, L), np.int32)
        check(lib.dge_walks_to_host(self._h, _ptr(out), n * L))
        return out

    def _seq_args(self, names, row0, n_rows):
        if n_rows is None:
            n_rows = self.shape[0] - int(row0)
        if names is not None and not isinstance(names, Names):
            names = Names(names)
        return names, int(row0), int(n_rows)

    def write_seq(self, path, names=None, position_prefix=False, row0=0, n_rows=None, append=False):
        """Rows [row0, row0 + n_rows) as .seq text into `path`, formatted on the device (include/dge.h: dge_walks_write_seq): one line per row, the
        names of its ids >= 0 joined by one blank; position_prefix writes the token of column j as "j-name".  names: a Names or a list (names[v] = the
        string of id v); None writes the decimal ids.  append=False creates or truncates the file.  -> the fields of struct dge_seq_out_info."""
        names, row0, n_rows = self._seq_args(names, row0, n_rows)
        inf = SeqOutInfo()
        check(lib.dge_walks_write_seq(self._h, row0, n_rows, names._h if names is not None else None, int(bool(position_prefix)), os.fsencode(path),
                                      int(bool(append)), C.byref(inf)))
        return _info_dict(inf)

    def to_seq_bytes(self, names=None, position_prefix=False, row0=0, n_rows=None):
        """The same text as write_seq's, into host memory (dge_walks_to_seq_text: a size query, then the text) -> (bytes, info)."""
        names, row0, n_rows = self._seq_args(names, row0, n_rows)
        nh = names._h if names is not None else None
        need = C.c_int64(0); inf = SeqOutInfo()
        check(lib.dge_walks_to_seq_text(self._h, row0, n_rows, nh, int(bool(position_prefix)), None, 0, C.byref(need), None))
        buf = np.empty(max(need.value, 1), np.uint8)
        check(lib.dge_walks_to_seq_text(self._h, row0, n_rows, nh, int(bool(position_prefix)), _ptr(buf), need.value, C.byref(need), C.byref(inf)))
        return buf[:need.value].tobytes(), _info_dict(inf)

    def add_position_prefix(self, region_count):
        check(lib.dge_walks_add_position_prefix(self._h, int(region_count)))

    def count_tokens(self, n_vertices, d_counts, row0=0, n_rows=None):
        """d_counts: torch int64 tensor [n_vertices] on this device (accumulated into)."""
        if n_rows is None:
            n_rows = self.shape[0] - row0
        check(lib.dge_count_tokens(self._h, int(row0), int(n_rows), int(n_vertices), _dev_ptr(d_counts)))


class Vectors:
    """float32 rows [rows x dim] in HBM with one present byte per row (struct dge_vectors, include/dge.h): what a .vec file holds, aligned by name."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device

    @classmethod
    def from_vec(cls, paths_or_bytes, header=False, names=None, intern=True, device=0):
        """.vec text -> (vectors, names, info): tokenised, interned and converted on the device (include/dge.h: dge_vectors_from_vec_files /
        dge_vectors_from_vec_text); every value is the float32 nearest its exact decimal.  paths_or_bytes: a path, a sequence of paths (taken in
        order), or the text itself as bytes / bytearray / memoryview.  header=True: every file opens with a "V D" line, which is checked.  names: a
        Names whose entries keep their ids (default: a new, empty one); row i of the result is the vector of names[i].  intern=True appends new
        names in the order of their first appearance; intern=False drops rows whose name is unknown (info["dropped"]).  info: the fields of struct
        dge_vec_info."""
        if names is None:
            names = Names()
        h = C.c_void_p(0); inf = VecInfo()
        kind, _keep, ptrs, sizes, n = _piece_args(paths_or_bytes, "texts" if isinstance(paths_or_bytes, _BYTES) else "paths")      # the text comes alone
        if kind == "texts":
            check(lib.dge_vectors_from_vec_text(int(device), ptrs[0], sizes[0], int(bool(header)), names._h, int(bool(intern)), C.byref(h), C.byref(inf)))
        else:
            check(lib.dge_vectors_from_vec_files(int(device), ptrs, n, int(bool(header)), names._h, int(bool(intern)), C.byref(h), C.byref(inf)))
        return cls(h, int(device)), names, _info_dict(inf, reserved=False)

    @classmethod
    def from_host(cls, rows, present=None, device=0):
        rows = np.ascontiguousarray(rows, np.float32)
        n, dim = rows.shape
        if present is not None:
            present = np.ascontiguousarray(present, np.uint8)
            if present.shape != (n,):
                raise ValueError("present must hold one entry per row")
        h = C.c_void_p(0)
        check(lib.dge_vectors_from_host(int(device), _ptr(rows), n, dim, _ptr(present), C.byref(h)))
        return cls(h, int(device))

    @classmethod
    def from_line(cls, X, touched, device=0):
        """The rows of a LINE result (evaluate.line_gpu, Flows.line) as resident float32 rows with present = touched: a vertex no kept edge names is left out
        of KNN, nDCG and k-means, as a region the reference's LINE output lacks is."""
        from .evaluate import line_features
        return cls.from_host(line_features(X, touched, np.float32), present=np.asarray(touched) != 0, device=device)

    def close(self):
        if getattr(self, "_h", None):
            lib.dge_vectors_free(self._h)
            self._h = None

    __del__ = close

    @property
    def shape(self):
        n = C.c_int64(0); d = C.c_int32(0)
        check(lib.dge_vectors_info(self._h, C.byref(n), C.byref(d), None, None))
        return n.value, d.value

    def to_host(self):
        n, d = self.shape
        out = np.empty((n, d), np.float32)
        check(lib.dge_vectors_to_host(self._h, _ptr(out), None, n * d))
        return out

    def present(self):
        pres = np.empty(self.shape[0], np.uint8)
        check(lib.dge_vectors_to_host(self._h, None, _ptr(pres), 0))
        return pres.astype(bool)

    def knn(self, k):
        """The k nearest other rows of every row in cosine distance (dge_knn_cosine_vectors) -> (idx int32 [n x k], dist float32 [n x k], kernel_ms)."""
        n = self.shape[0]
        idx = np.empty((n, int(k)), np.int32); dist = np.empty((n, int(k)), np.float32); ms = C.c_double(0)
        check(lib.dge_knn_cosine_vectors(self._h, int(k), _ptr(idx), _ptr(dist), C.byref(ms)))
        return idx, dist, ms.value

    def ndcg_against(self, gnd, k=10):
        """nDCG@k of these rows' neighbours under the ground features `gnd` (dge_ndcg_at_k_vectors) -> (nDCG, kernel ms)."""
        out = C.c_double(0); ms = C.c_double(0)
        check(lib.dge_ndcg_at_k_vectors(self._h, gnd._h, int(k), C.byref(out), C.byref(ms)))
        return out.value, ms.value

    def pairwise_eval(self, gnd, row_of, ks=(5, 10, 20, 30, 40, 50, 60, 70), rel_m=0, test=None, want_rows=False, want_lists=False):
        """The per-slice pairwise figure of these feature rows under the ground rows `gnd` (a Vectors, one row a region) as the rule of include/dge.h
        (dge_pairwise_eval_vectors); see evaluate.pairwise_eval for the arguments and the dict it returns."""
        from ._native import PairwiseInfo
        n = gnd.shape[0]
        row_of = np.ascontiguousarray(row_of, np.int64)
        if row_of.ndim == 1:
            row_of = row_of[None, :]
        if row_of.ndim != 2 or row_of.shape[1] != n:
            raise ValueError("row_of must be [n_sets x n] with n = %d ground rows, not %s" % (n, list(row_of.shape)))
        ks = np.ascontiguousarray(np.atleast_1d(ks), np.int32)
        if ks.ndim != 1 or len(ks) == 0:
            raise ValueError("ks must be a non-empty one-dimensional sequence")
        test = _select_mask(test, n)
        S, K, kmax, rel_m = row_of.shape[0], len(ks), int(ks[-1]), int(rel_m)
        ndcg = np.zeros((S, K)); precision = np.zeros((S, K)) if rel_m else None
        members = np.zeros(S, np.int64); tested = np.zeros(S, np.int64); inf = PairwiseInfo()
        ratio = np.empty((S, K, n)) if want_rows else None; hits = np.empty((S, K, n), np.int32) if want_rows else None
        ideal = np.empty((K, n)) if want_rows else None
        lists = np.empty((S, n, max(kmax, 0)), np.int32) if want_lists else None
        check(lib.dge_pairwise_eval_vectors(self._h, gnd._h, _ptr(row_of), S, _ptr(test), _ptr(ks), K, rel_m, _ptr(ndcg), _ptr(precision), _ptr(members),
                                            _ptr(tested), _ptr(ratio), _ptr(hits), _ptr(lists), _ptr(ideal), C.byref(inf)))
        out = dict(ndcg=ndcg, precision=precision, members=members, tested=tested, coverage=members / float(n), ks=ks, info=_info_dict(inf))
        if want_rows:
            out.update(ratio=ratio, hits=hits, ideal=ideal)
        if want_lists:
            out["lists"] = lists
        return out

    def pairwise_ground(self, m):
        """These rows as ground rows: the m <= 128 nearest other regions of every region by the keys of the pairwise rule (dge_pairwise_ground_vectors)
        -> (idx int32 [n x m], dist float64 [n x m])."""
        n, m = self.shape[0], int(m)
        idx = np.empty((n, max(m, 0)), np.int32); dist = np.empty((n, max(m, 0)), np.float64)
        check(lib.dge_pairwise_ground_vectors(self._h, m, _ptr(idx), _ptr(dist)))
        return idx, dist

    def kmeans(self, k, seed=1, n_init=10, max_iter=300, select=None, init=None):
        """k-means on these rows as the rule of include/dge.h (dge_kmeans_vectors): the same bits for the same rows, k, seed, n_init and max_iter.
        select: one entry per row, non-zero = take the row (default: every present row).  init: [k x dim] initial centres instead of k-means++ seeding
        (n_init is then 1).  -> (labels int32 [rows], -1 on rows not selected; centres float32 [k x dim]; info: the fields of struct dge_kmeans_info)."""
        n, dim = self.shape
        k = int(k)
        select = _select_mask(select, n)
        if init is not None:
            init = np.ascontiguousarray(init, np.float32)
            if init.shape != (k, dim):
                raise ValueError("init must be [k x dim] = [%d x %d], not %s" % (k, dim, list(init.shape)))
        cfg = KmeansCfg(k, int(n_init), int(max_iter), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)
        labels = np.empty(n, np.int32); centres = np.empty((max(k, 0), dim), np.float32); inf = KmeansInfo()
        check(lib.dge_kmeans_vectors(self._h, _ptr(select), C.byref(cfg), _ptr(init), _ptr(labels), _ptr(centres), C.byref(inf)))
        return labels, centres, _info_dict(inf)


    def _labels(self, y):
        y = np.asarray(y)
        if y.shape != (self.shape[0],):
            raise ValueError("y must hold one label per row")
        if y.dtype != np.uint8:
            y = np.where((y == 0) | (y == 1), y, 255).astype(np.uint8)      # anything but 0 and 1 is refused by the library where the row is used
        return np.ascontiguousarray(y)

    def tree_fit(self, y, select=None, max_depth=0, min_samples_split=2, min_samples_leaf=1):
        """A binary decision tree on these rows as the rule of include/dge.h (dge_tree_fit_vectors): the same bits for the same set of rows, labels and limits.
        y: one label, 0 or 1, per row.  select: one entry per row, non-zero = take the row (default: every present row).
        -> (tree: dict of feature int32, threshold float64, left int32, count int64, pos int64, one entry per node; info: the fields of struct dge_tree_info)."""
        n = self.shape[0]
        y = self._labels(y)
        select = _select_mask(select, n)
        cfg = TreeCfg(int(max_depth), int(min_samples_split), int(min_samples_leaf), 0)
        cap = max(2 * n - 1, 1)
        feature = np.empty(cap, np.int32); threshold = np.empty(cap, np.float64); left = np.empty(cap, np.int32)
        count = np.empty(cap, np.int64); pos = np.empty(cap, np.int64); inf = TreeInfo()
        check(lib.dge_tree_fit_vectors(self._h, _ptr(y), _ptr(select), C.byref(cfg), cap, _ptr(feature), _ptr(threshold), _ptr(left), _ptr(count), _ptr(pos), C.byref(inf)))
        m = inf.n_nodes
        tree = dict(feature=feature[:m].copy(), threshold=threshold[:m].copy(), left=left[:m].copy(), count=count[:m].copy(), pos=pos[:m].copy())
        return tree, _info_dict(inf)

    def tree_predict(self, tree):
        """The leaf vote of `tree` (the dict tree_fit gives) for every row (dge_tree_predict_vectors) -> uint8 [rows], 255 on an absent row."""
        feature = np.ascontiguousarray(tree["feature"], np.int32); threshold = np.ascontiguousarray(tree["threshold"], np.float64)
        left = np.ascontiguousarray(tree["left"], np.int32); count = np.ascontiguousarray(tree["count"], np.int64); pos = np.ascontiguousarray(tree["pos"], np.int64)
        m = len(feature)
        if not (feature.shape == threshold.shape == left.shape == count.shape == pos.shape == (m,)):
            raise ValueError("the five arrays of a tree must be one-dimensional and of one length")
        out = np.empty(self.shape[0], np.uint8)
        check(lib.dge_tree_predict_vectors(self._h, m, _ptr(feature), _ptr(threshold), _ptr(left), _ptr(count), _ptr(pos), _ptr(out)))
        return out

    def tree_cv(self, y, fold, n_folds, max_depth=0, min_samples_split=2, min_samples_leaf=1):
        """Cross-validated accuracy of the tree of tree_fit (dge_tree_cv_vectors): tree t trains on the present rows with fold != t and is tested on those with
        fold == t; fold -1 takes a row out.  -> dict(scores float64 [n_folds], NaN for a fold without test rows; mean over the others; correct, tested int64;
        n_nodes, depth int32; info: the fields of struct dge_tree_info)."""
        n = self.shape[0]
        y = self._labels(y)
        fold = np.ascontiguousarray(fold, np.int32)
        if fold.shape != (n,):
            raise ValueError("fold must hold one entry per row")
        F = int(n_folds)
        cfg = TreeCfg(int(max_depth), int(min_samples_split), int(min_samples_leaf), 0)
        correct = np.zeros(max(F, 0), np.int64); tested = np.zeros(max(F, 0), np.int64); nodes = np.zeros(max(F, 0), np.int32); depth = np.zeros(max(F, 0), np.int32)
        inf = TreeInfo()
        check(lib.dge_tree_cv_vectors(self._h, _ptr(y), _ptr(fold), F, C.byref(cfg), _ptr(correct), _ptr(tested), _ptr(nodes), _ptr(depth), C.byref(inf)))
        from .evaluate import cv_scores
        return dict(cv_scores(correct, tested), n_nodes=nodes, depth=depth, info=_info_dict(inf))

    def ridge_loo(self, y, lambdas, select=None, want_beta=True, want_pred=True):
        """Leave-one-out ridge regression on these rows as the rule of include/dge.h (dge_ridge_loo_vectors): the same bits for the same used rows in row order,
        targets and penalties.  y: [rows] or [rows x n_targets]; lambdas: the penalties, each >= 0; select: one entry per row, non-zero = take the row
        (default: every present row).  -> dict(mae, mre float64 [n_lambda x n_targets]; beta [n_lambda x n_targets x (dim + 1)], the intercept first;
        loo_pred [n_lambda x n_targets x rows], NaN on rows not used; info: the fields of struct dge_ridge_info)."""
        from .evaluate import _ridge_args
        n, dim = self.shape
        y, lam, select = _ridge_args(n, y, lambdas, select)
        T, L = y.shape[1], len(lam)
        mae = np.empty((L, T), np.float64); mre = np.empty((L, T), np.float64); inf = RidgeInfo()
        beta = np.empty((L, T, dim + 1), np.float64) if want_beta else None
        pred = np.empty((L, T, n), np.float64) if want_pred else None
        check(lib.dge_ridge_loo_vectors(self._h, _ptr(y), T, _ptr(select), _ptr(lam), L, _ptr(mae), _ptr(mre), _ptr(beta), _ptr(pred), C.byref(inf)))
        return dict(mae=mae, mre=mre, beta=beta, loo_pred=pred, info=_info_dict(inf))

    def ridge_predict(self, beta):
        """The predictions of the models beta [.. x (dim + 1)] (what ridge_loo gives, the intercept first) for every row (dge_ridge_predict_vectors)
        -> float64 [.. x rows], NaN on an absent row."""
        n, dim = self.shape
        beta = np.ascontiguousarray(beta, np.float64)
        if beta.ndim < 1 or beta.shape[-1] != dim + 1:
            raise ValueError("beta must be [.. x (dim + 1)] = [.. x %d], not %s" % (dim + 1, list(beta.shape)))
        m = int(np.prod(beta.shape[:-1], dtype=np.int64))
        out = np.empty(beta.shape[:-1] + (n,), np.float64)
        check(lib.dge_ridge_predict_vectors(self._h, _ptr(beta), m, _ptr(out)))
        return out

    def _label_columns(self, y):
        """y [rows] or [n_labels x rows] -> uint8 [n_labels x rows]; anything but 0 and 1 becomes 255, which the library refuses where the row is used"""
        y = np.asarray(y)
        if y.ndim == 1:
            y = y[None, :]
        if y.ndim != 2 or y.shape[1] != self.shape[0] or y.shape[0] < 1:
            raise ValueError("y must hold one label per row: [rows] or [n_labels x rows]")
        if y.dtype != np.uint8:
            y = np.where((y == 0) | (y == 1), y, 255).astype(np.uint8)
        return np.ascontiguousarray(y)

    def _svm_cfg(self, C, gamma, eps, max_iter, state, launch_iters):
        return SvmCfg(float(C), 1.0 / max(self.shape[1], 1) if gamma is None else float(gamma), float(eps), int(max_iter), int(state), int(launch_iters))

    def svm_fit(self, y, select=None, C=1.0, gamma=None, eps=1e-3, max_iter=10_000_000, state=0, launch_iters=0):
        """An RBF C-SVC per label column on these rows as the rule of include/dge.h (dge_svm_fit_vectors): the same bits for the same used rows in row order,
        labels and configuration.  y: [rows] or [n_labels x rows], 0 or 1; select: one entry per row, non-zero = take the row (default: every present row);
        gamma: default 1 / dim.  -> dict(coef float64 [n_labels x rows]: s * alpha, 0 on used rows that are not support, NaN on rows not used; bias float64
        [n_labels]; iterations int64, converged int32 [n_labels]; gamma; info: the fields of struct dge_svm_info)."""
        n = self.shape[0]
        y = self._label_columns(y)
        L = y.shape[0]
        select = _select_mask(select, n)
        cfg = self._svm_cfg(C, gamma, eps, max_iter, state, launch_iters)
        coef = np.empty((L, n), np.float64); bias = np.empty(L, np.float64); iters = np.zeros(L, np.int64); conv = np.zeros(L, np.int32); inf = SvmInfo()
        check(lib.dge_svm_fit_vectors(self._h, _ptr(y), L, _ptr(select), _byref(cfg), _ptr(coef), _ptr(bias), _ptr(iters), _ptr(conv), _byref(inf)))
        return dict(coef=coef, bias=bias, iterations=iters, converged=conv, gamma=cfg.gamma, info=_info_dict(inf))

    def svm_decision(self, coef, bias, gamma, x=None):
        """f(x) of the models (coef [.. x rows], bias [..]: what svm_fit gives for these rows) for every row of x, another Vectors of the same dim, or of these
        rows themselves (dge_svm_decision_vectors) -> float64 [n_models x rows(x)], NaN on an absent row."""
        coef = np.ascontiguousarray(np.atleast_2d(np.asarray(coef, np.float64)))
        bias = np.ascontiguousarray(np.atleast_1d(np.asarray(bias, np.float64)))
        if coef.ndim != 2 or coef.shape[1] != self.shape[0] or bias.shape != (coef.shape[0],):
            raise ValueError("coef must be [n_models x rows] and bias [n_models]")
        x = self if x is None else x
        out = np.empty((coef.shape[0], x.shape[0]), np.float64)
        check(lib.dge_svm_decision_vectors(self._h, _ptr(coef), _ptr(bias), coef.shape[0], float(gamma), x._h, _ptr(out)))
        return out

    def svm_cv(self, y, fold, n_folds, C=1.0, gamma=None, eps=1e-3, max_iter=10_000_000, state=0, launch_iters=0, want_decision=False):
        """Cross-validated accuracy of the SVM of svm_fit for every label column at once (dge_svm_cv_vectors): problem (l, f) trains column l on the present
        rows with fold != f and is tested on those with fold == f; fold -1 takes a row out.  -> dict(scores float64 [n_labels x n_folds], NaN for a fold
        without test rows; mean, std [n_labels] over the others (numpy's, what the reference prints); correct int64 [n_labels x n_folds]; tested int64
        [n_folds]; iterations, support int64, converged int32 [n_labels x n_folds]; decision [n_labels x rows] where asked for; info)."""
        n = self.shape[0]
        y = self._label_columns(y)
        L = y.shape[0]
        fold = np.ascontiguousarray(fold, np.int32)
        if fold.shape != (n,):
            raise ValueError("fold must hold one entry per row")
        F = int(n_folds)
        cfg = self._svm_cfg(C, gamma, eps, max_iter, state, launch_iters)
        shape = (L, max(F, 0))
        correct = np.zeros(shape, np.int64); tested = np.zeros(max(F, 0), np.int64); iters = np.zeros(shape, np.int64); support = np.zeros(shape, np.int64)
        conv = np.zeros(shape, np.int32); inf = SvmInfo()
        decision = np.empty((L, n), np.float64) if want_decision else None
        check(lib.dge_svm_cv_vectors(self._h, _ptr(y), L, _ptr(fold), F, _byref(cfg), _ptr(correct), _ptr(tested), _ptr(iters), _ptr(support), _ptr(conv), _ptr(decision),
                                     _byref(inf)))
        from .evaluate import svm_scores
        return dict(svm_scores(correct, tested), iterations=iters, support=support, converged=conv, decision=decision, gamma=cfg.gamma,
                    info=_info_dict(inf))


def make_config(dim, window, n_vertices, negative=5, min_count=2, epochs=1, workers=0, alpha=0.025, min_alpha=1e-4,
                seed=1, table_size=100_000_000, update_policy=0, use_hs=False):
    """struct dge_train_config, field by field (a ctypes view, not a mirror of DeepWalk: use_hs defaults to the plain
    negative-sampling path that BASELINE.json's metric and bench.py are about).  `deepwalk_config` is the reference's setting."""
    return TrainConfig(int(dim), int(window), int(negative), int(min_count), int(epochs), int(workers), float(alpha),
                       float(min_alpha), int(seed), int(table_size), int(n_vertices), int(update_policy), int(bool(use_hs)), 0)


def deepwalk_config(region_level, num_layer, n_vertices, use_hs=True, **kw):
    """What J/DeepWalk.java:62-76 builds: layerSize 20 ("tract") or 2 ("CA"), windowSize = LayeredGraph.numLayer, 5 negatives,
    minWordFrequency 2, one iteration, DL4J's learning rates — and the hierarchical-softmax term ON, because the builder never
    calls useHierarchicSoftmax(false) (java/embedding/DeepWalk.java and the C++ mirror default to the same)."""
    return make_config(2 if region_level == "CA" else 20, num_layer, n_vertices, negative=5, min_count=2, epochs=1, use_hs=use_hs, **kw)


class SgnsModel:
    """Vocabulary + syn0/syn1neg in HBM (replaces the DL4J Word2Vec object of J/DeepWalk.java:73-82)."""

    def __init__(self, handle, device, cfg):
        self._h = handle
        self.device = device
        self.cfg = cfg
        self.torch_device = "cuda:%d" % int(device)

    @classmethod
    def create(cls, cfg, d_counts, device=0):
        h = C.c_void_p(0)
        check(lib.dge_model_create(int(device), C.byref(cfg), _dev_ptr(d_counts), C.byref(h)))
        return cls(h, int(device), cfg)

    @classmethod
    def create_placed(cls, cfg, d_counts, device, probe, trials=3, first=None):
        """Start-up placement trials.  Where the driver puts a model's tables decides its training speed by up to 15 % (two models of one
        process differ reproducibly, a model freed and re-created in the same memory does not: profiles/r02_box_drift.txt), and no cheap probe
        of the memory predicts it — so: create `trials` models side by side (the earlier ones kept, or the next would get their memory
        back), time `probe(model) -> milliseconds` on each (one launch of the caller's own workload), keep the fastest, free the others.
        -> (model, [milliseconds of every trial])."""
        models = [first if first is not None else cls.create(cfg, d_counts, device)]
        ms = [float(probe(models[0]))]
        for _ in range(max(int(trials), 1) - 1):
            models.append(cls.create(cfg, d_counts, device)); ms.append(float(probe(models[-1])))
        best = min(range(len(ms)), key=ms.__getitem__)
        for i, m in enumerate(models):
            if i != best:
                m.close()
        return models[best], ms

    @classmethod
    def fit(cls, walks, cfg, device=0):
        """w2v.fit() one-shot: walks is a host int32 [n x L] array or a WalkCorpus."""
        h = C.c_void_p(0)
        if isinstance(walks, WalkCorpus):
            check(lib.dge_train_sgns_device(walks._h, C.byref(cfg), C.byref(h)))
            device = walks.device
        else:
            walks = np.ascontiguousarray(walks, np.int32)
            n, L = walks.shape
            check(lib.dge_train_sgns(int(device), _ptr(walks), n, L, C.byref(cfg), C.byref(h)))
        return cls(h, int(device), cfg)

    def close(self):
        if getattr(self, "_h", None):
            lib.dge_model_free(self._h)
            self._h = None

    __del__ = close

    def set_stream(self, stream_ptr):
        check(lib.dge_model_set_stream(self._h, C.c_void_p(int(stream_ptr))))

    def train(self, corpus, row0=0, n_rows=None, walk_index_base=0, epoch=0, words_before=0, words_scale=1.0, total_walks=0):
        if n_rows is None:
            n_rows = corpus.shape[0] - row0
        check(lib.dge_model_train(self._h, corpus._h, int(row0), int(n_rows), int(walk_index_base), int(epoch),
                                  int(words_before), float(words_scale), int(total_walks)))

    def walk_and_train(self, graph, corpus, row0, n_rows, walk_seed, walk_index_base, epoch=0, words_before=0,
                       words_scale=1.0, total_walks=0):
        check(lib.dge_model_walk_and_train(self._h, graph._h, corpus._h, int(row0), int(n_rows), int(walk_seed),
                                           int(walk_index_base), int(epoch), int(words_before), float(words_scale),
                                           int(total_walks)))

    def vectors(self):
        p = C.c_void_p(0); ids = C.c_void_p(0); V = C.c_int64(0); D = C.c_int32(0)
        check(lib.dge_model_vectors(self._h, C.byref(p), C.byref(ids), C.byref(V), C.byref(D)))
        if V.value == 0:
            return np.zeros((0, D.value), np.float32), np.zeros(0, np.int32)
        syn0 = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(V.value * D.value,)).copy().reshape(V.value, D.value)
        vid = np.ctypeslib.as_array(C.cast(ids, C.POINTER(C.c_int32)), shape=(V.value,)).copy()
        return syn0, vid

    def syn1neg(self):
        syn0, _ = self.vectors()
        p = C.c_void_p(0)
        check(lib.dge_model_syn1neg(self._h, C.byref(p)))
        if syn0.size == 0:
            return np.zeros_like(syn0)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(syn0.size,)).copy().reshape(syn0.shape)

    def syn1(self):
        """Inner-node table of the hierarchical softmax, [V-1 x dim] (models created with use_hs)."""
        p = C.c_void_p(0); rows = C.c_int64(0)
        check(lib.dge_model_syn1(self._h, C.byref(p), C.byref(rows)))
        n = rows.value * self.cfg.dim
        if n == 0:
            return np.zeros((0, self.cfg.dim), np.float32)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,)).copy().reshape(rows.value, self.cfg.dim)

    def huffman(self):
        """Huffman paths of the vocabulary rows: (offsets[V+1], points, codes) — bit d of codes[r] is the branch at
        points[offsets[r] + d] (word2vec.c CreateBinaryTree)."""
        _, vid = self.vectors()
        V = len(vid)
        po, pp, pc = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        check(lib.dge_model_huffman(self._h, C.byref(po), C.byref(pp), C.byref(pc)))
        if V == 0:
            return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint64)
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_int64)), shape=(V + 1,)).copy()
        n = int(off[-1])
        pts = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_int32)), shape=(max(n, 1),)).copy()[:n]
        codes = np.ctypeslib.as_array(C.cast(pc, C.POINTER(C.c_uint64)), shape=(V,)).copy()
        return off, pts, codes

    def counts(self):
        _, vid = self.vectors()
        p = C.c_void_p(0)
        check(lib.dge_model_counts(self._h, C.byref(p)))
        if len(vid) == 0:
            return np.zeros(0, np.int64)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int64)), shape=(len(vid),)).copy()

    def table(self):
        p = C.c_void_p(0); T = C.c_int64(0)
        check(lib.dge_model_table(self._h, C.byref(p), C.byref(T)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(T.value,)).copy()

    def row_rates(self):
        """(GB/s of random row reads, GB/s of random row read + write-back, lock-word exchanges per second, unigram-table look-ups per
        second) on this model's own memory (diagnostic: include/dge.h, dge_model_row_rates)."""
        v = [C.c_double(0) for _ in range(4)]
        check(lib.dge_model_row_rates(self._h, *[C.byref(x) for x in v])); return tuple(x.value for x in v)

    def table_runs(self):
        """(runs, exceptions) of the negative-sampling table's run form (include/dge.h, dge_model_table_runs); (0, 0): this model has none."""
        n, e = C.c_int32(0), C.c_int32(0)
        check(lib.dge_model_table_runs(self._h, C.byref(n), C.byref(e)))
        return n.value, e.value

    def table_placement(self):
        """What dge_model_create's probe-selected table allocation saw: [(candidates probed, best GB/s = the one kept, worst GB/s)] for syn0, syn1neg
        (and syn1 under hierarchical softmax)."""
        out = []
        for t in range(3 if self.cfg.use_hs else 2):
            n, a, b = C.c_int32(0), C.c_double(0), C.c_double(0)
            check(lib.dge_model_table_placement(self._h, t, C.byref(n), C.byref(a), C.byref(b)))
            out.append((n.value, round(a.value), round(b.value)))
        return out

    def tune_placement(self, corpus, row0=0, n_rows=None, candidates=3):
        """Placement search (include/dge.h: dge_model_tune_placement): -> (probe ms before, probe ms after, arrays moved).  The model's tables,
        counters and statistics are as before the call."""
        if n_rows is None:
            n_rows = corpus.shape[0] - row0
        a, b, n = C.c_double(0), C.c_double(0), C.c_int32(0)
        check(lib.dge_model_tune_placement(self._h, corpus._h, int(row0), int(n_rows), int(candidates), C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def placement_search(self):
        """{"runs", "probe_ms_before", "probe_ms_after", "arrays_moved"} of the placement search on this model (runs == 0: it never ran — the one-shot
        fit skips it where it cannot pay)."""
        n, a, b, mv = C.c_int32(0), C.c_double(0), C.c_double(0), C.c_int32(0)
        check(lib.dge_model_placement_search(self._h, C.byref(n), C.byref(a), C.byref(b), C.byref(mv)))
        return {"runs": n.value, "probe_ms_before": a.value, "probe_ms_after": b.value, "arrays_moved": mv.value}

    def stats(self):
        s = TrainStats()
        check(lib.dge_model_stats(self._h, C.byref(s)))
        return dict(pairs=s.pairs, words=s.words, kernel_ms=s.kernel_ms, walk_kernel_ms=s.walk_kernel_ms, launches=s.launches)

    def reset_stats(self):
        check(lib.dge_model_reset_stats(self._h))

    # ---- held-out evaluation (include/dge.h: dge_model_score_pairs / eval_links / eval_sgns); the model is only read
    def score_pairs(self, ctx_t, tgt_t):
        """syn0[row(ctx)] . syn1neg[row(tgt)] for vertex-id pairs (torch int32 tensors on the model's device) -> torch float32 tensor there;
        NaN where an id is outside the vocabulary."""
        import torch
        if ctx_t.dtype != torch.int32 or tgt_t.dtype != torch.int32 or ctx_t.numel() != tgt_t.numel():
            raise ValueError("score_pairs: two int32 tensors of one length")
        ctx_t = ctx_t.contiguous(); tgt_t = tgt_t.contiguous()
        out = torch.empty(ctx_t.numel(), dtype=torch.float32, device=ctx_t.device)
        check(lib.dge_model_score_pairs(self._h, _dev_ptr(ctx_t), _dev_ptr(tgt_t), ctx_t.numel(), _dev_ptr(out)))
        return out

    @staticmethod
    def _eval_dict(r):
        return dict(pairs=r.pairs, negatives=r.negatives, skipped=r.skipped, auc=r.auc, loss=r.loss, kernel_ms=r.kernel_ms)

    def eval_links(self, corpus, regions_per_slice, seed=3, row0=0, n_rows=None):
        """Link-prediction AUC and loss on the held-out walk steps of corpus rows [row0, row0 + n_rows)."""
        if n_rows is None:
            n_rows = corpus.shape[0] - row0
        r = EvalResult()
        check(lib.dge_model_eval_links(self._h, corpus._h, int(row0), int(n_rows), int(regions_per_slice), int(seed), C.byref(r)))
        return self._eval_dict(r)

    def eval_sgns(self, corpus, seed=3, row0=0, n_rows=None):
        """The negative-sampling objective (mean loss per pair) and AUC over the full-window pairs of corpus rows [row0, row0 + n_rows)."""
        if n_rows is None:
            n_rows = corpus.shape[0] - row0
        r = EvalResult()
        check(lib.dge_model_eval_sgns(self._h, corpus._h, int(row0), int(n_rows), int(seed), C.byref(r)))
        return self._eval_dict(r)

    def write_vec(self, path, names=None, header=False):
        """names: a list of str (names[v] = the string of vertex id v; None entries -> the decimal id), a Names, or None."""
        arr = None
        if isinstance(names, Names):
            arr = names._cstrs()
        elif names is not None:
            arr = (C.c_char_p * len(names))(*[n.encode() if n is not None else None for n in names])
        check(lib.dge_write_vec(self._h, arr, str(path).encode(), int(bool(header))))

    def load_vectors(self, v):
        """syn0 rows of the vocabulary words that `v` (a Vectors) holds := v's rows (dge_model_load_vectors) -> how many rows were set."""
        n = C.c_int64(0)
        check(lib.dge_model_load_vectors(self._h, v._h, C.byref(n)))
        return n.value

    # --- multi-GPU exchange (include/dge.h, last section)
    def schedule(self):
        """What the latest launch resolved update_policy 0 / workers 0 to."""
        pol, w, hot = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        check(lib.dge_model_schedule(self._h, C.byref(pol), C.byref(w), C.byref(hot)))
        return {"update_policy": pol.value, "workers": w.value, "hot_rows": hot.value}

    def lock_stats(self):
        """{"pairs_put_back", "rounds_short", "rounds"} of the block schedule's lock kernels since reset_stats (include/dge.h: dge_model_lock_stats)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib.dge_model_lock_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"pairs_put_back": a.value, "rounds_short": b.value, "rounds": c.value}

    def kernel(self):
        """Name and form of the trainer kernel the latest launch ran (include/dge.h: dge_model_kernel)."""
        buf = C.create_string_buffer(256)
        check(lib.dge_model_kernel(self._h, buf, 256))
        return buf.value.decode()

    def pair_loop(self):
        """{"loop", "slots"}: which pair loop the latest launch ran — 0 the per-pair syn0 lock, 1 the walk window (include/dge.h: dge_model_pair_loop)."""
        a, b = C.c_int32(0), C.c_int32(0)
        check(lib.dge_model_pair_loop(self._h, C.byref(a), C.byref(b)))
        return {"loop": a.value, "slots": b.value}

    # ---- multi-GPU block schedule (include/dge.h: dge_model_set_partition)
    def set_partition(self, n_parts, ctx_part=0, tgt_part=0):
        check(lib.dge_model_set_partition(self._h, int(n_parts), int(ctx_part), int(tgt_part)))

    def partition_floats(self, n_parts):
        n = C.c_int64(0); check(lib.dge_model_partition_floats(self._h, int(n_parts), C.byref(n))); return n.value

    def export_partition(self, table, n_parts, part, d_buf):
        check(lib.dge_model_export_partition(self._h, int(table), int(n_parts), int(part), _dev_ptr(d_buf)))

    def import_partition(self, table, n_parts, part, d_buf):
        check(lib.dge_model_import_partition(self._h, int(table), int(n_parts), int(part), _dev_ptr(d_buf)))

    def export_partition_async(self, table, n_parts, part, d_buf, consumer_stream=0):
        """Stream-ordered export (include/dge.h): the pack kernel runs on the model's stream and `consumer_stream` (a hipStream_t as an integer, 0 = the
        legacy default stream, e.g. torch.cuda.current_stream().cuda_stream) waits for it; the host does not."""
        check(lib.dge_model_export_partition_async(self._h, int(table), int(n_parts), int(part), _dev_ptr(d_buf), C.c_void_p(int(consumer_stream))))

    def import_partition_async(self, table, n_parts, part, d_buf, producer_stream=0):
        """Stream-ordered import: the model's stream waits for what `producer_stream` holds now, then unpacks; the host does not wait."""
        check(lib.dge_model_import_partition_async(self._h, int(table), int(n_parts), int(part), _dev_ptr(d_buf), C.c_void_p(int(producer_stream))))

    def stream(self):
        """The hipStream_t (as an integer) the model's launches are enqueued on."""
        p = C.c_void_p(0); check(lib.dge_model_stream(self._h, C.byref(p))); return p.value or 0

    def sync_size(self):
        n = C.c_int64(0); check(lib.dge_model_sync_size(self._h, C.byref(n))); return n.value

    def snapshot(self):
        check(lib.dge_model_snapshot(self._h))

    def export_delta(self, d_buf):
        check(lib.dge_model_export_delta(self._h, _dev_ptr(d_buf)))

    def import_delta(self, d_buf, scale):
        check(lib.dge_model_import_delta(self._h, _dev_ptr(d_buf), float(scale)))


def host_sync_count():
    """Blocking waits (stream / device / event synchronisations, blocking copies) the library has made in this process so far (include/dge.h:
    dge_host_sync_count): tests assert that an episode of the block schedule adds none."""
    n = C.c_int64(0); check(lib.dge_host_sync_count(C.byref(n))); return n.value


def build_stamp():
    """{"kernels": hash, "sorted": hash} of the trainer kernels' sources the loaded libdge.so was built from (include/dge.h: dge_build_stamp)."""
    return dict(kv.split("=") for kv in lib.dge_build_stamp().decode().split())


TUNING_KNOBS = {"hot_rows": 0, "hs_drain": 1, "force_segments": 2, "segment_shift": 3, "sorted_chunk": 4, "sorted_walks": 5, "workers": 6, "static_walks": 7, "hs_cold": 8, "hs_wave": 9, "acc_rows": 10, "acc_drain": 11, "table_runs": 12, "block_syn0_free": 13, "hs_centre": 14, "hs_hot_kb": 15, "allow_unsafe": 16, "watchdog_ms": 17, "hs_copies": 18, "small_rows": 19, "tree_batch": 20, "ridge_chunk": 21}      # include/dge.h: DGE_TUNE_*


class tuning:
    """Context manager around dge_set_tuning (ablation / test knobs of the trainer; process-wide):
    `with tuning(hot_rows=100): model.train(...)`.  Leaving the block puts the knobs back to what they were before it."""

    def __init__(self, **knobs):
        self.knobs = {TUNING_KNOBS[k]: int(v) for k, v in knobs.items()}
        self.before = {}

    def __enter__(self):
        for k, v in self.knobs.items():
            old = C.c_int64(-1)
            check(lib.dge_get_tuning(k, C.byref(old)))
            self.before[k] = old.value
            check(lib.dge_set_tuning(k, v))
        return self

    def __exit__(self, *exc):
        for k in self.knobs:
            check(lib.dge_set_tuning(k, self.before.get(k, -1)))
        return False
