"""`CPIndex` — drop-in for the reference's `cphnsw.CPIndex` (src/bindings.cpp:115-240) whose
query path runs on an MI355X through the C-ABI in include/cphnsw_mi355x.h.

Same constructor, methods, argument meaning, return shapes/dtypes and exception types as the
pybind11 class.  Returned ids are the reference's internal (post-reorder) node ids by default; an index that
has a row map (built here, or loaded from a native file that holds one) returns rows of the array given to
build() with `index.result_ids = "input"` (not in the reference).
"""
import ctypes as C

import numpy as np

from . import _lib

DEFAULT_K = 10  # constants::kDefaultK


def _as_f32(a):
    # py::array_t<float, c_style | forcecast>
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def pack_allowed_bits(mask):
    """Bool mask [n] -> uint32 words [ceil(n / 32)]: bit (i & 31) of word i >> 5 = mask[i] (the bitmap the filtered
    search reads; the same bits as np.packbits(mask, bitorder="little") read as little-endian words)."""
    m = np.asarray(mask, dtype=bool).ravel()
    nw = (m.size + 31) // 32
    padded = np.zeros(nw * 32, dtype=np.uint64)
    padded[:m.size] = m
    return (padded.reshape(nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


class IdFilter:
    """An allowed-id set on the index' device (CPIndex.make_filter).  The bitmap speaks of internal ids, or, with
    input_rows=True, of input rows: the device then converts it through the index' row map, once, into the internal-id
    bitmap the searches read.  Usable with any index of the same size on the same device; freeing it waits for the
    batches that may still read it.  A multi-device index' filter holds one bitmap per replica, each on that
    replica's device.  A partitioned index' filter speaks of global input rows and holds one bitmap per part, each the
    part's slice, behind one handle."""

    def __init__(self, index, words, n_bits, count, input_rows=False):
        self._h = C.c_void_p()
        self._hs = []                # one cph_filter per replica (a single-device index: one)
        self._pf = None              # partitioned index: the cph_parts_filter that owns the per-part filters
        self.size = int(n_bits)      # ids the filter covers (= the index size)
        self.count = int(count)      # allowed ids
        w = np.ascontiguousarray(words, np.uint32)
        if index._p is not None:
            pf = C.c_void_p()
            _lib.check(_lib.lib().cph_parts_filter_create_rows(index._p, w.ctypes.data if w.size else None, self.size,
                                                               C.byref(pf)))
            self._pf = pf
            self._parts = len(index._devices)
            return
        for rh in index._replicas():
            h = C.c_void_p()
            create = _lib.lib().cph_filter_create_rows if input_rows else _lib.lib().cph_filter_create
            _lib.check(create(rh, w.ctypes.data if w.size else None, self.size, C.byref(h)))
            self._hs.append(h)
        self._h = self._hs[0]

    @classmethod
    def _adopt(cls, size, count, hs=(), pf=None, parts=None):
        """An IdFilter around filters the library made itself (CPIndex.label_filters): one cph_filter per replica, or
        the cph_parts_filter of a partitioned index."""
        f = cls.__new__(cls)
        f._hs = list(hs)
        f._h = f._hs[0] if f._hs else C.c_void_p()
        f._pf = pf
        f._parts = parts
        f.size = int(size)
        f.count = int(count)
        return f

    def words(self):
        """The bitmap as it is resident on the device (replica 0's copy): uint32 [ceil(size / 32)], internal ids --
        what pack_allowed_bits gives for the allowed-id mask."""
        if getattr(self, "_pf", None) is not None:
            raise ValueError("words() is not defined for a partitioned index' filter (one bitmap per part, each in the "
                             "part's own internal ids)")
        if not self._h.value:
            raise ValueError("filter was closed")
        w = np.empty((self.size + 31) // 32, np.uint32)
        _lib.check(_lib.lib().cph_filter_export(self._h, w.ctypes.data if w.size else None, None))
        return w

    def close(self):
        pf = getattr(self, "_pf", None)
        if pf is not None:
            self._pf = None
            _lib.check(_lib.lib().cph_parts_filter_destroy(pf))
        hs = getattr(self, "_hs", [])
        self._hs = []
        self._h = C.c_void_p()
        for h in hs:
            if h.value:
                _lib.check(_lib.lib().cph_filter_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- filter algebra: a new IdFilter, made and counted on the device; the operands stay as they are.  Replica i is
    # combined with replica i, part p with part p.  A result is closed by its owner like any filter (the temporaries of
    # a chain such as (f & g) | h are freed when the expression drops them).
    def _binary(self, op, other):
        if not isinstance(other, IdFilter):
            return NotImplemented
        return combine_filters(op, [self], other)[0]

    def __and__(self, other):
        return self._binary("and", other)

    def __or__(self, other):
        return self._binary("or", other)

    def __sub__(self, other):
        """f - g: the ids of f that g does not allow (f AND NOT g)."""
        return self._binary("andnot", other)

    def __xor__(self, other):
        return self._binary("xor", other)

    def __invert__(self):
        """~f: every id below `size` that f does not allow (removed rows included: searches drop them anyway)."""
        return combine_filters("not", [self])[0]


FILTER_OPS = {"and": 0, "or": 1, "andnot": 2, "xor": 3, "not": 4}      # CPH_FILTER_*


def combine_filters(op, filters, other=None):
    """[IdFilter]: filters[j] OP other for every j, in one device pass per replica / part (cph_filters_combine).  op:
    "and", "or", "andnot" (a & ~b), "xor", or "not" (no `other`).  other: one IdFilter, combined with every filters[j], or
    a sequence of len(filters).  ValueError: a closed operand, operands of different size, device, replica count or part
    count, a partitioned filter mixed with a plain one, `other` of the wrong length."""
    if op not in FILTER_OPS:
        raise ValueError(f"op must be one of {sorted(FILTER_OPS)}")
    fs = list(filters)
    if op == "not":
        if other is not None:
            raise ValueError('"not" takes no second operand')
        gs = []
    elif isinstance(other, IdFilter):
        gs = [other]
    elif isinstance(other, (list, tuple)):
        gs = list(other)
        if len(gs) != len(fs):
            raise ValueError(f"the second operand must be one filter or a sequence of {len(fs)} filters (got {len(gs)})")
    else:
        raise ValueError(f'"{op}" needs a second operand: an IdFilter or a sequence of them')
    if not fs:
        return []
    for f in fs + gs:
        if not isinstance(f, IdFilter):
            raise ValueError("operands must be IdFilter objects")
        if getattr(f, "_pf", None) is None and not getattr(f, "_hs", []):
            raise ValueError("filter was closed")
    first = fs[0]
    parts = first._pf is not None
    for f in fs + gs:
        if (f._pf is not None) != parts:
            raise ValueError("a partitioned index' filter cannot be combined with a plain one")
        if f.size != first.size:
            raise ValueError(f"filters of different sizes cannot be combined ({f.size} and {first.size} ids)")
        if parts and f._parts != first._parts:
            raise ValueError("filters with different part counts cannot be combined")
        if not parts and len(f._hs) != len(first._hs):
            raise ValueError("filters with different replica counts cannot be combined")
    L, m, code = _lib.lib(), len(fs), FILTER_OPS[op]

    def table(xs):
        return (C.c_void_p * len(xs))(*[x.value for x in xs]) if xs else None

    if parts:
        out = (C.c_void_p * m)()
        _lib.check(L.cph_parts_filters_combine(code, table([f._pf for f in fs]), m, table([g._pf for g in gs]), len(gs), out))
        made = [IdFilter._adopt(first.size, 0, pf=C.c_void_p(out[j]), parts=first._parts) for j in range(m)]
        return CPIndex._with_counts(made, lambda f, c: L.cph_parts_filter_count(f._pf, c))
    per_rep = []
    try:
        for r in range(len(first._hs)):
            out = (C.c_void_p * m)()
            _lib.check(L.cph_filters_combine(code, table([f._hs[r] for f in fs]), m, table([g._hs[r] for g in gs]), len(gs), out))
            per_rep.append(out)
    except Exception:
        for out in per_rep:
            for j in range(m):
                L.cph_filter_destroy(C.c_void_p(out[j]))
        raise
    made = [IdFilter._adopt(first.size, 0, hs=[C.c_void_p(out[j]) for out in per_rep]) for j in range(m)]
    return CPIndex._with_counts(made, lambda f, c: L.cph_filter_export(f._h, None, c))


class GroupKeys:
    """A key column for grouped search on the index' device (CPIndex.make_group_keys): one int32 per row, for callers whose
    labels mean something else than their groups (labels = tenants, keys = documents).  It serves the index it was made
    for and covers `size` ids: after an add() it is refused with the size error a filter gets; load(), build() and
    compact() invalidate it.  A multi-device index' object holds one copy per replica.  close() waits for the batches
    that may still read it."""

    def __init__(self, index, keys, input_rows=False):
        self._hs = []                # one cph_group_keys per replica (a single-device index: one)
        self.size = int(keys.size)
        code = _lib.IDS_INPUT if input_rows else _lib.IDS_INTERNAL
        try:
            for rh in index._replicas():
                h = C.c_void_p()
                _lib.check(_lib.lib().cph_group_keys_create(rh, keys.ctypes.data if keys.size else None, self.size, code,
                                                            C.byref(h)))
                self._hs.append(h)
        except Exception:
            self.close()
            raise

    def close(self):
        hs = getattr(self, "_hs", [])
        self._hs = []
        for h in hs:
            if h.value:
                _lib.check(_lib.lib().cph_group_keys_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RescoreVectors:
    """Full-size rows for two-stage search on the index' device (CPIndex.make_rescore_vectors): one row of `dim`
    coordinates per id of the index, stored as `dtype` ("float16" or "float32") with one float32 squared norm per row, and
    the `metric` ("l2" or "ip") search_rescored scores them by.  It follows the rules of GroupKeys: it serves the index
    it was made for and covers `size` ids -- after an add() it is refused with the size error; load(), build() and
    compact() invalidate it; save_native does not carry it.  A multi-device index' object holds one copy per replica.
    close() waits for the batches that may still read it."""

    def __init__(self, index, rows, input_rows, dtype, metric):
        self._hs = []                # one cph_rescore_vectors per replica (a single-device index: one)
        self.size, self.dim = int(rows.shape[0]), int(rows.shape[1])
        self.dtype, self.metric = dtype, metric
        code = _lib.IDS_INPUT if input_rows else _lib.IDS_INTERNAL
        dt = _lib.RESCORE_FLOAT32 if dtype == "float32" else _lib.RESCORE_FLOAT16
        mt = _lib.RESCORE_IP if metric == "ip" else _lib.RESCORE_L2
        try:
            for rh in index._replicas():
                h = C.c_void_p()
                _lib.check(_lib.lib().cph_rescore_vectors_create(rh, rows.ctypes.data if rows.size else None, self.size, self.dim, code,
                                                                 dt, mt, C.byref(h)))
                self._hs.append(h)
        except Exception:
            self.close()
            raise

    def _info(self):
        if not self._hs:
            raise ValueError("rescore vectors were closed")
        size, dim, row_bytes, nbytes = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        dt, mt = C.c_int(), C.c_int()
        _lib.check(_lib.lib().cph_rescore_vectors_info(self._hs[0], C.byref(size), C.byref(dim), C.byref(dt), C.byref(mt),
                                                       C.byref(row_bytes), C.byref(nbytes)))
        return size.value, dim.value, dt.value, mt.value, row_bytes.value, nbytes.value

    @property
    def row_bytes(self):
        """Stored bytes of one row: dim coordinates of the dtype, padded to a multiple of 16."""
        return self._info()[4]

    @property
    def nbytes(self):
        """Device bytes of the rows and norms, summed over the replicas."""
        return self._info()[5] * len(self._hs)

    def stored(self, first=0, count=None, replica=0):
        """(rows uint8 [count, row_bytes], norms float32 [count]): the stored bytes in internal id order; waits for the
        device."""
        size, _, _, _, rb, _ = self._info()
        count = size - first if count is None else int(count)
        rows, norms = np.empty((count, rb), np.uint8), np.empty(count, np.float32)
        _lib.check(_lib.lib().cph_rescore_vectors_get(self._hs[replica], int(first), count, rows.ctypes.data if count else None,
                                                      norms.ctypes.data if count else None))
        return rows, norms

    def close(self):
        hs = getattr(self, "_hs", [])
        self._hs = []
        for h in hs:
            if h.value:
                _lib.check(_lib.lib().cph_rescore_vectors_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CPIndex:
    """`devices=[...]` (instead of `device`): the index is replicated on every listed HIP device (duplicates allowed:
    several replicas on one GPU) and search_batch splits its queries across the replicas in one call, with results
    byte-identical to a single-device index.  Hooks, get_vectors and internal_to_input_rows are served by replica 0.

    `devices=[...], partition=True`: the index is PARTITIONED instead (FAISS: IndexShards).  build() gives device p the
    contiguous rows dist.shard_bounds(n, P, p) as an ordinary single-device index, finalize() builds all parts at once,
    every search goes to all parts and row i of the answer is the first k entries of the stable merge of their rows
    (ascending distance, equal distances lower part first), made on devices[0].  One handle holds P times as much and
    the quadratic build does 1 / P of the work, on P devices; a query costs P searches.  Such an index speaks input
    rows only (result_ids is "input"), is saved and loaded with save_native / load_native (one file per part), and has
    no index-wide hooks: `parts` lists the (lo, hi) bounds and `part(i)` is part i as a single-device CPIndex.

    `metric="cosine"` (default "l2"): distances are 1 - cos(q, x) instead of squared L2.  build() and add() store every
    row as x / (sqrt(2) |x|), normalised on the device, and refuse (ValueError naming the first such row) a row without
    a direction: all zero, NaN or Inf in it, or a norm that overflows float32.  Every search normalises its queries the
    same way with one more kernel launch per batch, so the squared-L2 kernels report 1 - cos; a query without a
    direction is searched as the zero vector (every distance about 0.5) and is not refused.  The hooks (encode_query,
    entry_point, exact_l2, fastscan_block, calib_samples_debug) act on the vector as given.  The metric is fixed at
    construction; save_native / load_native carry it, save / load (the reference's format) do not and are refused.

    `metric="ip"`: maximum inner product search; every search returns score = -(q . x), ascending, so the best row has the
    most negative score.  The index stores [x, sqrt(M2 - |x|^2)], dim + 1 coordinates, for a bound M2 >= max |x|^2 and
    searches [q, 0]: the squared-L2 kernels then rank by inner product, one kernel in front of a batch augments its
    queries and one behind it turns distances into scores (two more launches per batch).  `max_norm` is sqrt(M2), a bound
    on the length of every row ever stored, add() included; None takes the longest row of the build() call.  build() and
    add() refuse (ValueError naming the first such row) a row with NaN or Inf, an overflowing norm, or a length above
    the bound; a query with NaN or Inf searches as the zero vector.  `dim` stays the caller's; the padded width is
    next_pow2(dim + 1), so dim = 128 pads to 256 (dim <= 2047).  get_vectors(stored=True) returns the stored rows,
    `ip_bound` is M2.  search() runs as a batch of one.  range_search, search_grouped, search_diverse, search_maxsim,
    partition=True and save / load are not available yet and raise; save_native / load_native carry the metric and M2."""

    _METRICS = {"l2": _lib.METRIC_L2, "cosine": _lib.METRIC_COSINE, "ip": _lib.METRIC_IP}

    def __init__(self, dim, bits=1, device=None, devices=None, partition=False, metric="l2", max_norm=None):
        self._h = C.c_void_p()
        self._m = None               # cph_multi handle of a multi-device index
        self._p = None               # cph_parts handle of a partitioned index
        self._owner = None           # a part(i) view: the partitioned index that owns the handle
        if dim < 0 or bits < 0:
            raise TypeError("CPIndex(): incompatible constructor arguments")  # size_t in pybind11
        self._dim = int(dim)
        self._bits = int(bits)
        self._result_ids = "internal"
        self._exact_threshold = 0
        self._columns = {}           # attribute columns (set_column): name -> slot on the handle
        self._tag_columns = {}       # tag columns (set_tags): name -> slot on the handle
        if metric not in self._METRICS:
            raise ValueError(f'metric must be "l2", "cosine" or "ip", not {metric!r}')
        self._metric = metric
        self._sdim = self._dim + (1 if metric == "ip" else 0)      # the width of the stored rows
        if metric == "ip" and partition:
            raise ValueError('partition=True does not take metric="ip" yet: the parts would need one global bound')
        if max_norm is not None and metric != "ip":
            raise ValueError('max_norm belongs to metric="ip"')
        if max_norm is not None and not (0 < float(max_norm) < float("inf")):
            raise ValueError("max_norm must be a positive finite length (None: the longest row of build())")
        # M2 as the float32 square of the float32 length (what the kernels compare squared norms with)
        bound = None if max_norm is None else float(np.float32(max_norm) * np.float32(max_norm))
        if bound is not None and not (0 < bound < float("inf")):
            raise ValueError("max_norm squared must be a positive finite float32")
        if partition and (devices is None or device is not None):
            raise ValueError("partition=True needs devices=[...] (one part per listed device), not device")
        if devices is not None:
            if device is not None:
                raise ValueError("pass either device or devices, not both")
            devs = [int(d) for d in devices]
            if not devs:
                raise ValueError("devices must list at least one device")
            if partition:
                p = C.c_void_p()
                _lib.check(_lib.lib().cph_parts_create(int(dim), int(bits), (C.c_int * len(devs))(*devs), len(devs),
                                                       C.byref(p)))
                self._p = p
                self._devices = devs
                self._device = devs[0]
                self._result_ids = "input"
                self._part_handles = []      # borrowed part handles (owned by the parts handle)
                for i in range(len(devs)):
                    h = C.c_void_p()
                    _lib.check(_lib.lib().cph_parts_part(p, i, C.byref(h)))
                    self._part_handles.append(h)
                if metric != "l2":
                    _lib.check(_lib.lib().cph_parts_set_metric(p, self._METRICS[metric]))
                return
            m = C.c_void_p()
            _lib.check(_lib.lib().cph_multi_create(int(dim), int(bits), (C.c_int * len(devs))(*devs), len(devs),
                                                   C.byref(m)))
            self._m = m
            self._devices = devs
            self._device = devs[0]
            self._reps = []          # borrowed replica handles (owned by the multi handle)
            for i in range(len(devs)):
                h = C.c_void_p()
                _lib.check(_lib.lib().cph_multi_replica(m, i, C.byref(h)))
                self._reps.append(h)
            self._h = self._reps[0]  # hooks, get_vectors, ...: replica 0
            self._next_dev = 0       # search_batch_device: alternates between the replicas on the queries' device
            if metric == "ip":
                _lib.check(_lib.lib().cph_multi_set_metric_ip(m))
            elif metric != "l2":
                _lib.check(_lib.lib().cph_multi_set_metric(m, self._METRICS[metric]))
            if bound is not None:
                _lib.check(_lib.lib().cph_multi_set_ip_bound(m, bound))
            return
        if device is None:
            device = _default_device()
        self._device = int(device)
        self._devices = [self._device]
        _lib.check(_lib.lib().cph_create(int(dim), int(bits), int(device), C.byref(self._h)))
        if metric == "ip":
            _lib.check(_lib.lib().cph_set_metric_ip(self._h))
        elif metric != "l2":
            _lib.check(_lib.lib().cph_set_metric(self._h, self._METRICS[metric]))
        if bound is not None:
            _lib.check(_lib.lib().cph_set_ip_bound(self._h, bound))

    @property
    def metric(self):
        """"l2", "cosine" or "ip": fixed at construction."""
        return self._metric

    @property
    def ip_bound(self):
        """metric="ip": M2, the squared-length bound of the rows the index holds (before build(): max_norm squared, 0.0
        when it comes from the data)."""
        if self._metric != "ip":
            raise ValueError('ip_bound belongs to metric="ip"')
        m2 = C.c_float(0.0)
        _lib.check(_lib.lib().cph_get_ip_bound(self._h, C.byref(m2)))
        return float(m2.value)

    def metric_stats(self):
        """(launches of the metric's kernels, bytes of the metric's query buffers), summed over the replicas / parts:
        both 0 on an "l2" index, which launches and allocates nothing for the metric.  "cosine": the normalisation
        kernel; "ip": the augmenting kernel, the max pass of build() and the score epilogue.  Counted on the host."""
        tot = [0, 0]
        for h in self._replicas():
            out = (C.c_uint64 * 2)()
            _lib.check(_lib.lib().cph_metric_stats(h, out))
            tot = [tot[0] + int(out[0]), tot[1] + int(out[1])]
        return tuple(tot)

    def __del__(self):
        if getattr(self, "_owner", None) is not None:      # a borrowed part: the partitioned index destroys it
            self._owner = None
            self._h = C.c_void_p()
            return
        p = getattr(self, "_p", None)
        if p is not None:
            self._p = None
            try:
                _lib.lib().cph_parts_destroy(p)
            except Exception:
                pass
            return
        m = getattr(self, "_m", None)
        if m is not None:
            self._m = None
            self._h = C.c_void_p()
            try:
                _lib.lib().cph_multi_destroy(m)
            except Exception:
                pass
            return
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib().cph_destroy(h)
            except Exception:
                pass
            self._h = C.c_void_p()

    def _replicas(self):
        if self._p is not None:
            return self._part_handles
        return self._reps if self._m is not None else [self._h]

    # -- partitioned index (not in the reference) -----------------------------------------------
    @property
    def partitioned(self):
        return self._p is not None

    @property
    def parts(self):
        """[(lo, hi)] input rows of every part of a partitioned index (zeros before build())."""
        self._need_parts("parts")
        b = np.zeros(len(self._devices) + 1, np.uint64)
        _lib.check(_lib.lib().cph_parts_bounds(self._p, b.ctypes.data))
        return [(int(b[i]), int(b[i + 1])) for i in range(len(self._devices))]

    def part(self, i):
        """Part i of a partitioned index as a single-device CPIndex over its slice: a borrowed view (the partitioned
        index owns it and must outlive it) that returns slice-local input rows; add parts[i][0] for global rows.  Its
        hooks, row_map() and get_vectors work as on any index; load, build and finalize on it are refused.  The view knows
        the names of the index' columns and tag columns (set before or after it was made): column(), column_filters,
        tag_filters, where and facet on it read the part's slice of them."""
        self._need_parts("part()")
        i = int(i)
        if not 0 <= i < len(self._devices):
            raise ValueError(f"part index must lie in [0, {len(self._devices)})")
        v = CPIndex.__new__(CPIndex)
        v._h = self._part_handles[i]
        v._m = None
        v._p = None
        v._owner = self
        v._dim, v._bits = self._dim, self._bits
        v._metric = self._metric
        v._sdim = self._sdim
        v._device = self._devices[i]
        v._devices = [self._devices[i]]
        v._result_ids = "input" if self.is_finalized else "internal"
        v._exact_threshold = self._exact_threshold
        v._columns = self._column_slots()                # shared with the index: a part holds its slice of every column in
        v._tag_columns = self._tag_slots()               # the same slot, so the view sees the names set before and after it was made
        return v

    def _need_parts(self, what):
        if self._p is None:
            raise ValueError(f"{what} needs a partitioned index (CPIndex(..., devices=[...], partition=True))")

    def _no_parts(self, what):
        if self._p is not None:
            raise ValueError(f"{what} is not defined on a partitioned index (every part has its own internal ids): "
                             f"use part(i).{what}")

    @property
    def devices(self):
        """HIP device of every replica (a single-device index: its one device)."""
        return list(self._devices)

    def set_min_shard(self, q):
        """Smallest shard of a search_batch worth a replica (default 1024 queries; a batch of fewer than 2 * q
        queries goes whole to one replica).  No effect on a single-device index."""
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_set_min_shard(self._m, int(q)))

    # -- construction (host side) -------------------------------------------
    def build(self, vectors):
        v = _as_f32(vectors)
        if v.ndim != 2 or v.shape[1] != self._dim:
            raise ValueError("vectors must be a (n, dim) float32 array")
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_build(self._p, v.ctypes.data, v.shape[0]))
            return
        self._result_ids = "internal"    # the old index and its row map are gone
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_build(self._m, v.ctypes.data, v.shape[0]))
            return
        _lib.check(_lib.lib().cph_build(self._h, v.ctypes.data, v.shape[0]))

    def finalize(self):
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_finalize(self._p))
            return
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_finalize(self._m))
            return
        _lib.check(_lib.lib().cph_finalize(self._h))

    # -- filtered search (not in the reference) ------------------------------------------------
    def make_filter(self, allowed, ids=None):
        """IdFilter from a bool mask of length `size` or an integer array of allowed ids.  `ids`: the space `allowed`
        speaks of, "internal" or "input" (rows of the array given to build(); needs a row map); default: the index'
        result_ids, so that a filter and the results it restricts use the same numbers."""
        space = self._result_ids if ids is None else ids
        if space not in ("internal", "input"):
            raise ValueError('ids must be "internal" or "input"')
        if self._p is not None and space != "input":
            raise ValueError('a partitioned index takes filters in input rows only (ids="input")')
        a = np.asarray(allowed)
        n = self.size
        if a.dtype == bool:
            if a.ndim != 1 or a.shape[0] != n:
                raise ValueError(f"filter mask must be a 1D bool array of length {n} (the index size)")
            mask = a
        elif a.size == 0 or np.issubdtype(a.dtype, np.integer):
            ids = a.astype(np.int64).ravel()
            if ids.size and (ids.min() < 0 or ids.max() >= n):
                raise ValueError(f"filter ids must lie in [0, {n})")
            mask = np.zeros(n, dtype=bool)
            mask[ids] = True
        else:
            raise ValueError("filter must be a bool mask or an integer array of ids")
        return IdFilter(self, pack_allowed_bits(mask), n, int(np.count_nonzero(mask)), input_rows=space == "input")

    def _filter(self, f):
        if isinstance(f, IdFilter):
            if self._p is not None:
                if f._pf is None:
                    raise ValueError("filter was closed, or was not made by a partitioned index")
                if f._parts != len(self._devices):
                    raise ValueError("filter was made for an index with another number of parts")
                return f
            if not f._h.value:
                raise ValueError("filter was closed")
            if len(f._hs) != len(self._replicas()):
                raise ValueError("filter was made for an index with another number of replicas")
            return f
        return self.make_filter(f)

    def _filter_list(self, filter, filter_of, n):
        """The arguments of a batch with per-query filters -> ([IdFilter], filter_of as int32 [n])."""
        if filter_of is None:
            # (a flat list of ids or of bools stays what it always was: ONE filter, the argument of make_filter)
            if isinstance(filter, (list, tuple)) and any(isinstance(f, (IdFilter, np.ndarray, list, tuple)) for f in filter):
                raise ValueError("a sequence of filters needs filter_of (the filter of every query)")
            return None, None
        if not isinstance(filter, (list, tuple)):
            raise ValueError("filter_of needs filter to be a sequence of filters")
        fo = np.asarray(filter_of)
        if fo.ndim != 1 or fo.shape[0] != n or not (fo.size == 0 or np.issubdtype(fo.dtype, np.integer)):
            raise ValueError(f"filter_of must be a 1D integer array of length {n} (one entry per query)")
        if fo.size and (fo.min() < -1 or fo.max() >= len(filter)):
            raise ValueError(f"filter_of values must lie in [-1, {len(filter)})")
        fs = []
        try:
            for f in filter:
                fs.append(self._filter(f))
        except Exception:
            for made, given in zip(fs, filter):     # the filters this call made are freed now, not by the collector
                if made is not given:
                    made.close()
            raise
        return fs, np.ascontiguousarray(fo, np.int32)

    @staticmethod
    def _filter_handles(fs, rep=None):
        """cph_filter* array of a filter list: [f] of replica `rep`, or (rep None) [f][replica]; of filters of a
        partitioned index: their cph_parts_filter*."""
        hs = [h.value for f in fs for h in ([f._pf] if f._pf is not None else f._hs if rep is None else [f._hs[rep]])]
        return (C.c_void_p * len(hs))(*hs) if hs else None

    def _filter_args(self, fs, fo, f, rep):
        """(filters, n_filters, filter_of) of a C entry that takes all three: the list `fs` with `fo`, or the one filter
        `f` (filter_of NULL), or none.  rep: as in _filter_handles."""
        if fs is not None:
            return self._filter_handles(fs, rep), len(fs), fo.ctypes.data
        if f is not None:
            return self._filter_handles([f], rep), 1, None
        return None, 0, None

    # (handle kind, call form) -> the C entry of a batch in host memory, in device memory (replicas: the replica's own)
    _BATCH_ENTRY = {
        ("single", "filtered"): ("cph_search_batch_filtered", "cph_search_batch_device_filtered"),
        ("single", "exact"): ("cph_search_batch_exact", "cph_search_batch_exact_device"),
        ("single", "filters"): ("cph_search_batch_filters", "cph_search_batch_filters_device"),
        ("multi", "filtered"): ("cph_multi_search_batch_filtered", "cph_search_batch_device_filtered"),
        ("multi", "exact"): ("cph_multi_search_batch_exact", "cph_search_batch_exact_device"),
        ("multi", "filters"): ("cph_multi_search_batch_filters", "cph_search_batch_filters_device"),
        ("parts", "filtered"): ("cph_parts_search_batch_filtered", "cph_parts_search_batch_device_filtered"),
        ("parts", "exact"): ("cph_parts_search_batch_exact", "cph_parts_search_batch_exact_device"),
        ("parts", "filters"): ("cph_parts_search_batch_filters", "cph_parts_search_batch_filters_device"),
    }

    def _batch_call(self, qp, n, k, filter, exact, filter_of, out, rep=None, stream=None):
        """One batch through its C entry.  qp, out = (ids, dist): addresses; rep None: the host form on the whole index,
        else the device form on replica `rep` (a partitioned index: 0), enqueued on `stream`."""
        fs, fo = self._filter_list(filter, filter_of, n)
        kind, whole = (("parts", self._p) if self._p is not None else ("multi", self._m) if self._m is not None
                       else ("single", self._h))
        if fs is not None:
            form, fa = "filters", self._filter_args(fs, fo, None, rep) + (int(bool(exact)),)
        else:
            # (f is held until the call returns: it may have been made here, and freeing it waits for the batch)
            f = None if filter is None else self._filter(filter)
            if f is None:
                fa = (None,)
            elif kind == "multi" and rep is None:               # one filter per replica
                fa = (self._filter_handles([f]),)
            else:
                fa = (f._pf if kind == "parts" else f._hs[rep or 0],)
            form = "exact" if exact else "filtered"
        host, dev = self._BATCH_ENTRY[kind, form]
        if rep is None:
            fn, h, tail = host, whole, ()
        else:
            fn, h, tail = dev, (whole if kind == "parts" else self._replicas()[rep]), (C.c_void_p(stream),)
        _lib.check(getattr(_lib.lib(), fn)(h, qp, n, k, *fa, *out, *tail))

    # -- labels (not in the reference) -----------------------------------------------------------
    @staticmethod
    def _as_labels(a, what):
        a = np.asarray(a)
        if a.dtype == bool or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{what} must be integers")
        if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) > 2 ** 31 - 1):
            raise ValueError(f"{what} must fit int32")
        return a.astype(np.int32, order="C")     # (a scalar stays 0-d)

    def set_labels(self, labels, ids=None):
        """One integer label per row (a tenant, a category, a day), kept on the device (4 B per row): an integer array
        [size] of any width whose values fit int32, indexed in the space `ids` ("internal" or "input"; default:
        result_ids, as for make_filter).  None removes the column.  label_filter / label_filters and the `label=`
        argument of the searches read it.  build(), load() and load_native() drop it (no file carries it: keep the array
        and call set_labels again after loading); remove() and set_row_map() leave it; compact() carries it over."""
        if labels is None:
            self._set_attribute("labels", None, 0)
            return
        space = self._id_space(ids)
        a = self._as_labels(labels, "labels")
        if a.ndim != 1 or a.shape[0] != self.size:
            raise ValueError(f"labels must be a 1D integer array of length {self.size} (the index size)")
        self._set_attribute("labels", a.ctypes.data, a.size, space=space)

    def _dispatch(self, single, multi, parts):
        """What the one handle this index has gives: parts(handle) of a partitioned index, multi(handle) of replicas,
        else single(handle)."""
        if self._p is not None:
            return parts(self._p)
        if self._m is not None:
            return multi(self._m)
        return single(self._h)

    def _set_attribute(self, what, *args, space="internal"):
        """cph_set_<what>(handle, *args, id space), or its cph_multi_ form; cph_parts_set_<what> takes the same without
        the id space (a partitioned index is always given input rows).  None in place of the values drops the column."""
        L = _lib.lib()
        code = _lib.IDS_INPUT if space == "input" else _lib.IDS_INTERNAL
        _lib.check(self._dispatch(lambda h: getattr(L, f"cph_set_{what}")(h, *args, code),
                                  lambda m: getattr(L, f"cph_multi_set_{what}")(m, *args, code),
                                  lambda p: getattr(L, f"cph_parts_set_{what}")(p, *args)))

    @property
    def has_labels(self):
        """The index holds a label column (set_labels)."""
        def has(h):
            f = C.c_int(0)
            _lib.check(_lib.lib().cph_has_labels(h, C.byref(f)))
            return bool(f.value)
        if self._p is not None:
            return all(has(h) for h in self._part_handles)
        return has(self._h)

    @staticmethod
    def _labels_of(h, n, by_row, slot=None):
        """The label column (slot None) or attribute column `slot` of handle h."""
        out = np.empty(n, np.int32)
        if n and slot is None:
            _lib.check(_lib.lib().cph_get_labels(h, 0, n, out.ctypes.data))
        elif n:
            _lib.check(_lib.lib().cph_get_column(h, slot, 0, n, out.ctypes.data))
        if not by_row:
            return out
        rows = np.empty(n, np.uint32)
        if n:
            _lib.check(_lib.lib().cph_get_row_map(h, 0, n, rows.ctypes.data))
        r = np.empty(n, np.int32)
        r[rows] = out
        return r

    def labels(self, ids=None):
        """int32[size] copy of the label column, indexed in the space `ids` (default: result_ids)."""
        return self._column_values(None, ids)

    def _column_values(self, slot, ids):
        by_row = self._id_space(ids) == "input"          # (a partitioned index: always; _id_space refuses "internal")
        if self._p is not None:
            return np.concatenate([self._labels_of(h, hi - lo, by_row, slot) for h, (lo, hi) in zip(self._part_handles, self.parts)])
        return self._labels_of(self._h, self.size, by_row, slot)

    def label_filters(self, lo, hi=None):
        """[IdFilter]: filter j allows the rows whose label x satisfies lo[j] <= x <= hi[j] (hi=None: x == lo[j];
        lo[j] > hi[j]: nothing).  All of them are made in ONE pass over the label column on the device, which also
        counts them (`count`); nothing is packed on the host.  They are ordinary filters: usable wherever filter=
        is, with removed rows, replicas and parts.  Their bitmaps share one device allocation, freed with the last."""
        return self._range_filters(None, lo, hi, "label bounds")

    def _range_filters(self, slot, lo, hi, what):
        """label_filters on the label column (slot None) or on attribute column `slot`."""
        lo = self._as_labels(lo, what).ravel()
        hi = lo if hi is None else self._as_labels(hi, what).ravel()
        if hi.shape != lo.shape:
            raise ValueError("lo and hi must have the same length")
        L = _lib.lib()
        col = () if slot is None else (slot,)
        return self._column_pass(L.cph_filters_from_labels if slot is None else L.cph_filters_from_column,
                                 L.cph_parts_filters_from_labels if slot is None else L.cph_parts_filters_from_column,
                                 (*col, lo.ctypes.data, hi.ctypes.data), lo.size)

    def _column_pass(self, make, make_parts, args, m):
        """[IdFilter] of one device pass over a column: make(handle, *args, m, out) on every replica, or make_parts on a
        partitioned index; the counts are filled in, and what was made before a failure is destroyed."""
        L, n = _lib.lib(), self.size
        if m == 0:
            return []
        if self._p is not None:
            out = (C.c_void_p * m)()
            _lib.check(make_parts(self._p, *args, m, out))
            fs = [IdFilter._adopt(n, 0, pf=C.c_void_p(out[j]), parts=len(self._devices)) for j in range(m)]
            return self._with_counts(fs, lambda f, c: L.cph_parts_filter_count(f._pf, c))
        per_rep = []
        try:
            for rh in self._replicas():
                out = (C.c_void_p * m)()
                _lib.check(make(rh, *args, m, out))
                per_rep.append(out)
        except Exception:
            for out in per_rep:
                for j in range(m):
                    L.cph_filter_destroy(C.c_void_p(out[j]))
            raise
        fs = [IdFilter._adopt(n, 0, hs=[C.c_void_p(out[j]) for out in per_rep]) for j in range(m)]
        return self._with_counts(fs, lambda f, c: L.cph_filter_export(f._h, None, c))

    @staticmethod
    def _with_counts(fs, ask):
        """Fills in `count` of filters the library just made; if that fails they are closed here, not by the collector."""
        try:
            for f in fs:
                c = C.c_uint64(0)
                _lib.check(ask(f, C.byref(c)))
                f.count = c.value
        except Exception:
            for f in fs:
                f.close()
            raise
        return fs

    def time_label_filters(self, on=True):
        """Debug hook of the measurement script: while on, every label pass is bracketed by HIP events
        (last_label_filters_us).  Off by default."""
        self._time_pass("cph_debug_time_label_filters", on)

    def last_label_filters_us(self):
        """Device time (HIP events, microseconds) of the last label_filters pass made under time_label_filters(): a
        multi-device or partitioned index reports the longest of its replicas' / parts' passes."""
        return max(self._last_pass_us("cph_debug_last_label_filters_us", r) for r in range(len(self._replicas())))

    def _time_pass(self, entry, on):
        """time_*: the debug hook `entry` (cph_debug_time_*) on every replica."""
        for h in self._replicas():
            _lib.check(getattr(_lib.lib(), entry)(h, int(bool(on))))

    def _last_pass_us(self, entry, replica):
        """last_*_us: what `entry` (cph_debug_last_*_us) reports on one replica."""
        us = C.c_double(0)
        _lib.check(getattr(_lib.lib(), entry)(self._replicas()[replica], C.byref(us)))
        return us.value

    def label_filter(self, lo, hi=None):
        """IdFilter of the rows whose label is `lo`, or lies in [lo, hi] (both ends inclusive)."""
        return self.label_filters([lo], None if hi is None else [hi])[0]

    # -- attribute columns and filter algebra (not in the reference) ----------------------------
    MAX_COLUMNS = 8                  # CPH_MAX_COLUMNS

    def _held_slots(self, slots, has_entry):
        """`slots` (name -> slot) without the names whose column a handle no longer holds (has_entry: cph_has_column or
        cph_has_tags): build(), load() and load_native() drop every column, and their names go with them here."""
        def has(h, slot):
            f = C.c_int(0)
            _lib.check(getattr(_lib.lib(), has_entry)(h, slot, C.byref(f)))
            return bool(f.value)
        hs = self._part_handles if self._p is not None else [self._h]
        for name, slot in list(slots.items()):
            if not all(has(h, slot) for h in hs):
                del slots[name]
        return slots

    @staticmethod
    def _slot_for(slots, name, maximum, full):
        """The slot `name` has in `slots`, or the first of the `maximum` that no name holds; none free: ValueError(full)."""
        if name in slots:
            return slots[name]
        free = [s for s in range(maximum) if s not in slots.values()]
        if not free:
            raise ValueError(full)
        return free[0]

    def _column_slots(self):
        """name -> slot of the attribute columns the handle still holds."""
        return self._held_slots(self._columns, "cph_has_column")

    def _slot(self, name):
        if name == "label":
            if not self.has_labels:
                raise ValueError('the index has no label column: call set_labels first')
            return None
        slots = self._column_slots()
        if name not in slots:
            raise ValueError(f"the index has no column {name!r}: call set_column first")
        return slots[name]

    def set_column(self, name, values, ids=None):
        """A named int32 attribute column next to the label column (a year, a price band, a stock flag): an integer array
        [size] whose values fit int32, indexed in the space `ids` (default: result_ids), kept on the device (4 B per
        row).  None drops the column and frees its name.  At most MAX_COLUMNS names; "label" is the label column's
        (set_labels).  column_filter(s) and where() read it.  Lifecycle as for labels: build(), load() and
        load_native() drop every column, remove() and set_row_map() leave them, compact() carries them; add() on an
        index that holds columns raises (drop them, add, set them again at the new size)."""
        if not isinstance(name, str) or not name:
            raise ValueError("a column name must be a non-empty string")
        if name == "label":
            raise ValueError('"label" names the label column: use set_labels')
        if name in self._tag_slots():
            raise ValueError(f"{name!r} names a tag column: columns and tag columns share one namespace")
        slots = self._column_slots()
        if values is None:
            if name in slots:
                self._set_attribute("column", slots[name], None, 0)
                del slots[name]
            return
        space = self._id_space(ids)
        a = self._as_labels(values, "column values")
        if a.ndim != 1 or a.shape[0] != self.size:
            raise ValueError(f"column values must be a 1D integer array of length {self.size} (the index size)")
        slot = self._slot_for(slots, name, self.MAX_COLUMNS,
                              f"an index holds at most {self.MAX_COLUMNS} columns: drop one first (set_column(name, None))")
        self._set_attribute("column", slot, a.ctypes.data, a.size, space=space)
        slots[name] = slot

    @property
    def columns(self):
        """Names of the attribute columns the index holds (set_column)."""
        return list(self._column_slots())

    def column(self, name, ids=None):
        """int32[size] copy of column `name` ("label": the label column), indexed in the space `ids` (default: result_ids)."""
        return self._column_values(self._slot(name), ids)

    def column_filters(self, name, lo, hi=None):
        """label_filters on column `name`: filter j allows the rows whose value x satisfies lo[j] <= x <= hi[j]
        (hi=None: x == lo[j]); one device pass, the same kernel."""
        return self._range_filters(self._slot(name), lo, hi, "column bounds")

    def column_filter(self, name, lo, hi=None):
        """IdFilter of the rows whose value in column `name` is `lo`, or lies in [lo, hi] (both ends inclusive)."""
        return self.column_filters(name, [lo], None if hi is None else [hi])[0]

    # -- tag columns: set-valued attributes (not in the reference) --------------------------------
    MAX_TAG_COLUMNS = 4              # CPH_MAX_TAG_COLUMNS
    MAX_TAGS_PER_ROW = 1024          # CPH_MAX_TAGS_PER_ROW
    MAX_TAG_TEST_VALUES = 64         # CPH_MAX_TAG_TEST_VALUES
    _TAG_MODES = {"any": 0, "all": 1, "none": 2}

    def _tag_slots(self):
        """name -> slot of the tag columns the handle still holds."""
        return self._held_slots(self._tag_columns, "cph_has_tags")

    def _tag_slot(self, name):
        slots = self._tag_slots()
        if name not in slots:
            raise ValueError(f"the index has no tag column {name!r}: call set_tags first")
        return slots[name]

    def set_tags(self, name, tags, lims=None, ids=None):
        """A named tag column: a SET of integer tags per row (the groups allowed to read a document, the topics of a
        chunk, the languages of a page), kept on the device as a CSR (4 B per row and 4 B per tag).  `tags` is a
        sequence of `size` integer sequences (a row may be empty); or, with `lims` given, the flat integer array of a
        CSR whose `lims` is [size + 1], starts at 0 and does not decrease.  Values must fit int32; the rows are indexed in
        the space `ids` (default: result_ids).  Duplicates and any order inside a row are accepted: the column is stored
        sorted and distinct (tags()).  At most MAX_TAGS_PER_ROW distinct tags per row and MAX_TAG_COLUMNS names, which
        share one namespace with the attribute columns.  None drops the column and frees its name.  tag_filter(s) and
        where() read it.  Lifecycle as for set_column: build(), load() and load_native() drop every tag column,
        remove() and set_row_map() leave them, compact() carries them; add() on an index that holds one raises."""
        if not isinstance(name, str) or not name:
            raise ValueError("a tag column name must be a non-empty string")
        if name == "label":
            raise ValueError('"label" names the label column: use set_labels')
        if name in self._column_slots():
            raise ValueError(f"{name!r} names an attribute column: columns and tag columns share one namespace")
        slots = self._tag_slots()
        if tags is None:
            if name in slots:
                self._set_attribute("tags", slots[name], None, None, 0)
                del slots[name]
            return
        space = self._id_space(ids)
        if lims is None:
            rows = [np.asarray(r).ravel() for r in tags]
            lims = np.zeros(len(rows) + 1, np.uint64)
            if rows:
                np.cumsum([r.size for r in rows], out=lims[1:])
            filled = [r for r in rows if r.size]
            flat = np.concatenate(filled) if filled else np.zeros(0, np.int32)
        else:
            la = np.asarray(lims)
            if la.ndim != 1 or la.size == 0 or not np.issubdtype(la.dtype, np.integer) or (la.size and int(la.min()) < 0):
                raise ValueError("lims must be a 1D array of non-negative integers")
            lims = la.astype(np.uint64, order="C")
            flat = np.asarray(tags).ravel()
            if int(lims[-1]) != flat.size:
                raise ValueError(f"lims ends at {int(lims[-1])}, tags holds {flat.size} values")
        flat = self._as_labels(flat, "tags")
        if lims.size != self.size + 1:
            raise ValueError(f"a tag column has one row per index row: {lims.size - 1} rows given, the index holds {self.size}")
        slot = self._slot_for(slots, name, self.MAX_TAG_COLUMNS,
                              f"an index holds at most {self.MAX_TAG_COLUMNS} tag columns: drop one first (set_tags(name, None))")
        self._set_attribute("tags", slot, lims.ctypes.data, flat.ctypes.data if flat.size else None, lims.size - 1, space=space)
        slots[name] = slot

    @property
    def tag_columns(self):
        """Names of the tag columns the index holds (set_tags)."""
        return list(self._tag_slots())

    @staticmethod
    def _tags_of(h, n, by_row, slot):
        """(lims int64[n + 1], tags int32) of tag column `slot` of handle h: in internal ids, or by input row."""
        L = _lib.lib()
        lims = np.zeros(n + 1, np.uint64)
        _lib.check(L.cph_get_tags(h, slot, 0, n, lims.ctypes.data, None))
        vals = np.empty(int(lims[-1]), np.int32)
        if vals.size:
            _lib.check(L.cph_get_tags(h, slot, 0, n, lims.ctypes.data, vals.ctypes.data))
        lims = lims.astype(np.int64)
        if not by_row or n == 0:
            return lims, vals
        rows = np.empty(n, np.uint32)
        _lib.check(L.cph_get_row_map(h, 0, n, rows.ctypes.data))
        id_of_row = np.empty(n, np.int64)
        id_of_row[rows] = np.arange(n)
        lens = np.diff(lims)[id_of_row]
        out = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=out[1:])
        src = np.repeat(lims[:-1][id_of_row] - out[:-1], lens) + np.arange(int(out[-1]))
        return out, vals[src]

    def tags(self, name, ids=None):
        """(lims int64[size + 1], tags int32[lims[-1]]): tag column `name` in its canonical form (every row ascending and
        distinct), the rows indexed in the space `ids` (default: result_ids)."""
        slot = self._tag_slot(name)
        by_row = self._id_space(ids) == "input"
        if self._p is None:
            return self._tags_of(self._h, self.size, by_row, slot)
        cut = [self._tags_of(h, hi - lo, by_row, slot) for h, (lo, hi) in zip(self._part_handles, self.parts)]
        lims, at = [np.zeros(1, np.int64)], 0
        for pl, _ in cut:
            lims.append(pl[1:] + at)
            at += int(pl[-1])
        return np.concatenate(lims), np.concatenate([v for _, v in cut])

    def tag_filters(self, name, tests, mode="any"):
        """[IdFilter]: one filter per test on tag column `name`.  A test is an int (the row has this tag) or a sequence
        of at most MAX_TAG_TEST_VALUES distinct ints V; `mode` -- one string, or one per test -- says how many of V a row
        must hold: "any" (at least one), "all" (every one) or "none".  An empty V allows nothing under "any" and every
        row under "all" and "none".  All filters are made in ONE pass over the column on the device, which also counts
        them; they are ordinary filters (filter=, filter_of=, & | ~, removed rows, replicas and parts).  Per-query
        permissions: fs = tag_filters("acl", groups_of_distinct_users); search_batch(q, k, filter=fs, filter_of=user)."""
        slot = self._tag_slot(name)
        tests = list(tests)
        m = len(tests)
        modes = [mode] * m if isinstance(mode, str) else list(mode)
        if len(modes) != m or any(not isinstance(x, str) or x not in self._TAG_MODES for x in modes):
            raise ValueError('mode must be "any", "all" or "none": one string, or one per test')
        vals = [self._as_labels(t, "tag test values").ravel() for t in tests]
        lims = np.zeros(m + 1, np.uint32)
        if m:
            np.cumsum([v.size for v in vals], out=lims[1:])
        flat = np.concatenate(vals) if m else np.zeros(0, np.int32)
        flat = np.ascontiguousarray(flat, np.int32)
        codes = np.array([self._TAG_MODES[x] for x in modes], np.uint8)
        L = _lib.lib()
        return self._column_pass(L.cph_filters_from_tags, L.cph_parts_filters_from_tags,
                                 (slot, lims.ctypes.data, flat.ctypes.data if flat.size else None, codes.ctypes.data), m)

    def tag_filter(self, name, test, mode="any"):
        """IdFilter of the rows that pass one test on tag column `name` (tag_filters)."""
        return self.tag_filters(name, [test], mode)[0]

    def time_tag_filters(self, on=True):
        """Debug hook of the measurement script: while on, every tag pass is bracketed by HIP events (last_tag_filters_us)."""
        self._time_pass("cph_debug_time_tag_filters", on)

    def last_tag_filters_us(self):
        """Device time (HIP events, microseconds) of the last tag_filters pass made under time_tag_filters(): the longest
        of the replicas' / parts' passes."""
        return max(self._last_pass_us("cph_debug_last_tag_filters_us", r) for r in range(len(self._replicas())))

    # -- facet counts: rows per column value under filters (not in the reference) --------------------
    MAX_FACET_TOP = 1024             # K of facet(top=K), at most
    _FACET_LABEL, _FACET_COLUMN, _FACET_TAGS = 0, 1, 2      # CPH_FACET_*

    def _facet_column(self, name):
        """(kind, slot) of the column `name` for the cph_facet_* calls: "label", an attribute column or a tag column."""
        if self._p is not None:
            raise ValueError("facet is not defined on a partitioned index (every part has its own dictionary and merging "
                             "them is not done here): use part(i).facet")
        if not isinstance(name, str):
            raise ValueError("a column name must be a string")
        if name == "label":
            self._slot(name)
            return self._FACET_LABEL, 0
        if name in self._tag_slots():
            return self._FACET_TAGS, self._tag_slot(name)
        if name not in self._column_slots():
            raise ValueError(f"the index has no column {name!r}: call set_column or set_tags first")
        return self._FACET_COLUMN, self._slot(name)

    def prepare_facets(self, name):
        """Builds the facet dictionary of column `name` now (its distinct values, and one code per row on the device:
        4 B per row, per tag for a tag column) instead of on the first facet() call."""
        kind, slot = self._facet_column(name)
        _lib.check(_lib.lib().cph_facet_prepare(self._h, kind, slot))

    def facet(self, name, filter=None, top=None):
        """Rows per distinct value of column `name` ("label": the label column; an attribute column; a tag column)
        among the rows a filter allows, counted on the device: (values int32 [U] ascending, counts int64 [U]).
        `values` are the distinct values of the whole column, removed rows included (the list does not change under
        remove(); their count goes to 0); for a tag column the distinct tags, and a row counts once per tag it holds.
        counts[u] = rows that the filter allows, that are not removed, and whose value is (whose set holds) values[u].
        filter: None (all live rows), one filter (an IdFilter or anything make_filter accepts), or a list of m of them:
        counts is then int64 [m, U], made in one device pass per 2^22 counters; an empty list gives [0, U].
        top=K (1 <= K <= MAX_FACET_TOP): (values int32 [m, K], counts int64 [m, K], found int32 [m]) instead -- per filter
        the K values with the largest non-zero counts, count descending and ties by value ascending, selected on the
        device; found[j] = min(K, values with a non-zero count), the slots behind it hold 0 (a single filter: [K], [K]
        and an int).  Not changed by result_ids or set_row_map: filters are internal-id bitmaps once made.  The call
        waits for its outputs.  A replicated index answers from its first replica; a partitioned one raises (use
        part(i).facet).  The dictionary is built on the first call for a column (prepare_facets) and kept until the
        column changes.  Like every call that reads a column, facet() must not run while another thread changes that
        column (set_labels, set_column, set_tags, add, compact, build, load): the outputs are sized from the dictionary
        the call saw first.  On an index with removed rows every filter is first narrowed to its live rows (one more
        device pass and wait per filter the first time it is used after a remove(); cached with the filter after that).
        ValueError: an unknown column, an index that is not finalized, a closed filter or one of another
        size, device or replica count, top outside [1, MAX_FACET_TOP]."""
        if top is not None and (isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= int(top) <= self.MAX_FACET_TOP):
            raise ValueError(f"top must be an integer in [1, {self.MAX_FACET_TOP}]")
        kind, slot = self._facet_column(name)
        L = _lib.lib()
        single = not isinstance(filter, list)
        given = [filter] if single else list(filter)
        fs = []
        try:
            for f in given:
                fs.append(None if f is None else self._filter(f))
            U = C.c_uint64(0)
            _lib.check(L.cph_facet_values(self._h, kind, slot, C.byref(U), None))
            values = np.empty(U.value, np.int32)
            _lib.check(L.cph_facet_values(self._h, kind, slot, C.byref(U), values.ctypes.data if values.size else None))
            m = len(fs)
            table = (C.c_void_p * m)(*[None if f is None else f._hs[0].value for f in fs]) if m else None
            if top is None:
                counts = np.zeros((m, U.value), np.uint64)
                if m:
                    _lib.check(L.cph_facet_counts(self._h, kind, slot, table, m, counts.ctypes.data if counts.size else None))
                counts = counts.view(np.int64)              # (counts stay below 2^32: the same bits)
                return (values, counts[0]) if single else (values, counts)
            K = int(top)
            tv, tc, found = np.zeros((m, K), np.int32), np.zeros((m, K), np.uint64), np.zeros(m, np.uint32)
            if m:
                _lib.check(L.cph_facet_top(self._h, kind, slot, table, m, K, tv.ctypes.data, tc.ctypes.data, found.ctypes.data))
            tc, found = tc.view(np.int64), found.view(np.int32)
            return (tv[0], tc[0], int(found[0])) if single else (tv, tc, found)
        finally:
            for made, g in zip(fs, given):          # the filters this call made are freed now, not by the collector
                if made is not None and made is not g:
                    made.close()

    def time_facets(self, on=True):
        """Debug hook of the measurement script: while on, the launches of every facet() call are bracketed by HIP events
        (last_facets_us).  Off by default."""
        _lib.check(_lib.lib().cph_debug_time_facets(self._h, int(bool(on))))

    def last_facets_us(self):
        """Device time (HIP events, microseconds) of the launches of the last facet() call made under time_facets()."""
        us = C.c_double(0)
        _lib.check(_lib.lib().cph_debug_last_facets_us(self._h, C.byref(us)))
        return us.value

    def combine_filters(self, op, filters, other=None):
        """[IdFilter]: filters[j] OP other, made and counted on the device in one pass (module function
        combine_filters): op "and" / "or" / "andnot" / "xor" with `other` one filter (combined with every filters[j]) or
        a sequence of len(filters); "not" without `other`.  The per-tenant case: combine_filters("and",
        label_filters(vals), in_stock) and search_batch(..., filter=that list, filter_of=...)."""
        return combine_filters(op, filters, other)

    def where(self, **tests):
        """IdFilter of the rows that pass every test: name=value (equality) or name=(lo, hi) (inclusive range) on the
        column `name`; "label" names the label column.  On a tag column (set_tags) name=7 means "has tag 7", and
        name={"any": [...]}, {"all": [...]} or {"none": [...]} (one key) is that test; a (lo, hi) pair is a ValueError
        there.  Each test is one column pass, the AND runs on the device; the intermediate filters are closed here."""
        if not tests:
            raise ValueError("where() needs at least one column test")
        made = []
        try:
            tag_names = self._tag_slots()
            for name, t in tests.items():
                if name in tag_names:
                    if isinstance(t, dict):
                        if len(t) != 1:
                            raise ValueError(f'a tag test is {{"any" | "all" | "none": values}} with one key, got {t!r} for {name!r}')
                        (mode, vals), = t.items()
                        made.append(self.tag_filter(name, vals, mode))
                    elif isinstance(t, (tuple, list)):
                        raise ValueError(f'tag column {name!r} has no range test: give a tag or {{"any": [...]}}, got {t!r}')
                    else:
                        made.append(self.tag_filter(name, t))
                    continue
                lo, hi = t if isinstance(t, (tuple, list)) and len(t) == 2 else (t, None)
                if isinstance(t, (tuple, list)) and len(t) != 2:
                    raise ValueError(f"a test is a value or a (lo, hi) pair, got {t!r} for {name!r}")
                made.append(self.column_filter(name, lo, hi))
            acc = made[0]
            for f in made[1:]:
                acc = acc & f
                made.append(acc)
            made.remove(acc)
            return acc
        finally:
            for f in made:
                f.close()

    def _from_label(self, label, filter, filter_of, n):
        """The `label=` argument of a search -> (filter, filter_of, [filters made here, closed by that call]).  A scalar:
        one filter for the batch; an integer array [n] (n None: not allowed here): one label per query -- a filter per
        distinct value, all made in one device pass, and the filter_of path."""
        if filter is not None or filter_of is not None:
            raise ValueError("label= and filter= exclude each other")
        if not self.has_labels:
            raise ValueError("label= needs a label column: call set_labels first")
        a = self._as_labels(label, "label")
        if a.ndim == 0:
            f = self.label_filter(int(a))
            return f, None, [f]
        if n is None:
            raise ValueError("this call takes one label (a label per query needs search_batch / search_batch_device)")
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"label must be one integer or a 1D integer array of length {n} (one entry per query)")
        vals, inv = np.unique(a, return_inverse=True)
        fs = self.label_filters(vals)
        return fs, np.ascontiguousarray(inv.ravel(), np.int32), fs

    def _with_label(self, label, filter, filter_of, n, call):
        """The `label=` prologue of every search entry: call(filter, filter_of) under the filters of `label`
        (_from_label), which live for that call only."""
        filter, filter_of, made = self._from_label(label, filter, filter_of, n)
        try:
            return call(filter, filter_of)
        finally:
            for f in made:
                f.close()

    def _device_replica(self, queries):
        """The replica that serves a batch in the device tensor `queries`: one on the tensor's device, alternating
        between several there.  A single-device index: 0; a partitioned one (in the calls that take one): 0, and the
        tensor lives on its first device."""
        dev = queries.device.index if queries.is_cuda else None
        if self._m is None:
            if dev != self._device:
                raise ValueError("queries must live on the first device of a partitioned index (the merge runs there)"
                                 if self._p is not None else "queries must live on this index' device")
            return 0
        on = [i for i, d in enumerate(self._devices) if d == dev]
        if not on:
            raise ValueError("queries must live on one of this index' devices")
        self._next_dev += 1
        return on[(self._next_dev - 1) % len(on)]

    @staticmethod
    def _search_stream(stream, queries, fresh):
        """The stream of a device-form call -> (its handle, its torch stream, or None where it is torch's current stream:
        the caller's allocations are in order already).  `fresh`: tensors the call has just allocated, on the current
        stream; another search stream has to run after them, and the caching allocator must not hand the blocks out
        again while the search still uses them."""
        import torch
        cur = torch.cuda.current_stream(queries.device)
        st = cur.cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
        if st == cur.cuda_stream:
            return st, None
        ext = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(st, device=queries.device)
        if fresh:
            ext.wait_stream(cur)
            for t in fresh:
                t.record_stream(ext)
        return st, ext

    # -- search -----------------------------------------------------------------------------
    def search(self, query, k=DEFAULT_K, filter=None, exact=False, label=None):
        """Single query, unpadded rows.  With `filter` (an IdFilter or anything make_filter accepts) only allowed ids
        are returned; that query runs as a batch of one through the filtered batch path.  `exact`: as in search_batch
        (a batch of one as well).  `label`: one label value, instead of filter=label_filter(label).
        metric="cosine": distances are 1 - cos(query, row)."""
        q = _as_f32(query)
        if q.ndim != 1 or q.shape[0] != self._dim:
            raise ValueError("query must be 1D and match index dimension")
        if label is not None:
            return self._with_label(label, filter, None, None, lambda f, _: self.search(q, k, filter=f, exact=exact))
        kk = max(int(k), 1)
        if self._p is not None and filter is None and not exact:
            ids = np.empty(kk, np.int64)
            dist = np.empty(kk, np.float32)
            m = C.c_uint64(0)
            _lib.check(_lib.lib().cph_parts_search(self._p, q.ctypes.data, int(k), ids.ctypes.data, dist.ctypes.data,
                                                   C.byref(m)))
            return ids[:m.value].copy(), dist[:m.value].copy()
        if filter is not None or exact:
            ids, dist = self.search_batch(q[None, :], kk, filter=filter, exact=exact)
            m = int(np.count_nonzero(ids[0] >= 0))
            return ids[0, :m].copy(), dist[0, :m].copy()
        ids = np.empty(kk, np.int64)
        dist = np.empty(kk, np.float32)
        m = C.c_uint64(0)
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_search(self._m, q.ctypes.data, int(k), ids.ctypes.data,
                                                   dist.ctypes.data, C.byref(m)))
            return ids[:m.value].copy(), dist[:m.value].copy()
        _lib.check(_lib.lib().cph_search(self._h, q.ctypes.data, int(k), ids.ctypes.data,
                                         dist.ctypes.data, C.byref(m)))
        return ids[:m.value].copy(), dist[:m.value].copy()

    def search_batch(self, queries, k=DEFAULT_K, filter=None, exact=False, filter_of=None, label=None):
        """Rows padded with -1 / FLT_MAX.  `filter`: restrict the results to allowed ids (see make_filter).
        `exact=True`: brute force instead of the graph search -- every row holds the k nearest allowed ids (without a
        filter: of the whole index), ascending by distance, equal distances by ascending internal id, no id twice;
        k <= 1024.  A distance has the same bytes the graph search returns for that id.  See also exact_threshold.
        Per-query filters: `filter` = a sequence of filters and `filter_of` = an integer array [n] (host data): query i
        is searched under filter[filter_of[i]], unfiltered where filter_of[i] == -1, and row i holds the bytes of the
        single-filter call for that query and that filter.  Every query is routed on its own (padding, exact scan or
        graph search, by the rules above); one call serves them all.
        `label` (needs set_labels; instead of filter=): one value = filter=label_filter(value); an integer array [n] =
        one label per query -- the filters of the distinct values are made in one device pass and the batch runs as
        with filter_of.  The filters live for this call only.
        metric="cosine": distances are 1 - cos(query, row); the queries are normalised on the device first."""
        q = _as_f32(queries)
        if q.ndim != 2 or q.shape[1] != self._dim:
            raise ValueError("queries must be a (n, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, q.shape[0],
                                    lambda f, fo: self.search_batch(q, k, filter=f, exact=exact, filter_of=fo))
        n, k = q.shape[0], int(k)
        ids = np.empty((n, k), np.int64)
        dist = np.empty((n, k), np.float32)
        self._batch_call(q.ctypes.data, n, k, filter, exact, filter_of, (ids.ctypes.data, dist.ctypes.data))
        return ids, dist

    def search_batch_device(self, queries, k=DEFAULT_K, out=None, stream=None, filter=None, exact=False, filter_of=None,
                            label=None):
        """Device-resident variant: `queries` is a float32 CUDA/HIP torch tensor (n, dim) on this
        index' device; returns (ids int64, dist float32) torch tensors on the same device.  The work
        is enqueued on `stream` (default: torch's current stream) and the call does not wait for it:
        the tensors are valid in stream order.  Two batches on two streams overlap.  `filter`: as in
        search_batch (an IdFilter made here from a mask or ids is freed on return, which waits for the batch).
        A multi-device index runs the whole batch on one replica that lives on the queries' device (alternating
        between several there); the batch is not split.  `exact`: as in search_batch.  `filter_of` (with a sequence
        of filters): per-query filters as in search_batch; it is host data here too, a numpy array or a list.
        `label`: as in search_batch (host data; its filters are freed on return, which waits for the batch).
        metric="cosine": distances are 1 - cos; the normalisation is one more launch on `stream`, still enqueue-only."""
        import torch
        if queries.dim() != 2 or queries.shape[1] != self._dim or queries.dtype != torch.float32:
            raise ValueError("queries must be a (n, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, queries.shape[0],
                                    lambda f, fo: self.search_batch_device(queries, k, out=out, stream=stream, filter=f,
                                                                           exact=exact, filter_of=fo))
        n, k = queries.shape[0], int(k)
        rep = self._device_replica(queries)
        fresh = []                       # tensors allocated here, on torch's current stream
        if not queries.is_contiguous():
            queries = queries.contiguous()
            fresh.append(queries)
        if out is None:
            ids = torch.empty((n, k), dtype=torch.int64, device=queries.device)
            dist = torch.empty((n, k), dtype=torch.float32, device=queries.device)
            fresh += [ids, dist]
        else:
            ids, dist = out
            for t, dt in ((ids, torch.int64), (dist, torch.float32)):
                if (tuple(t.shape) != (n, k) or t.dtype != dt or t.device != queries.device
                        or not t.is_contiguous()):
                    raise ValueError("out must be contiguous (n, k) int64 / float32 tensors on the queries' device")
        st, _ = self._search_stream(stream, queries, fresh)
        # (a partitioned index waits on the host for every part's search, then enqueues the merge on the stream)
        self._batch_call(queries.data_ptr(), n, k, filter, exact, filter_of, (ids.data_ptr(), dist.data_ptr()), rep, st)
        return ids, dist

    # -- range search (not in the reference) ---------------------------------------------------
    def _range_args(self, n, radius, filter, exact, max_results, filter_of):
        """Validation shared by both range entry points -> (radius float32 [n] on the host, IdFilter or None, K)."""
        if self._p is not None:
            raise ValueError("range_search is not defined on a partitioned index (every part has its own internal ids "
                             "and its own segments): use part(i).range_search")
        if filter_of is not None or (isinstance(filter, (list, tuple))
                                     and any(isinstance(f, (IdFilter, np.ndarray, list, tuple)) for f in filter)):
            raise ValueError("range_search takes one filter for the whole batch (per-query filters, filter_of, are not "
                             "supported)")
        if hasattr(radius, "detach"):                     # a torch tensor (copied to the host: the C-ABI takes host radii)
            radius = radius.detach().cpu().numpy()
        r = np.asarray(radius)
        if r.dtype == bool or not (np.issubdtype(r.dtype, np.floating) or np.issubdtype(r.dtype, np.integer)):
            raise ValueError("radius must be a number or a float array with one entry per query")
        if r.ndim == 0:
            r = np.full(n, r, np.float32)
        elif r.ndim != 1 or r.shape[0] != n:
            raise ValueError(f"radius must be a scalar or a 1D array of length {n} (one entry per query)")
        r = np.ascontiguousarray(r, np.float32)
        K = 0
        if not exact:
            if max_results is None:
                raise ValueError("range_search(exact=False) needs max_results (the k of the underlying search)")
            K = int(max_results)
            if K < 1:
                raise ValueError("max_results must be >= 1")
        return r, (None if filter is None else self._filter(filter)), K

    def range_search(self, queries, radius, filter=None, exact=True, max_results=None, filter_of=None, label=None):
        """Every allowed id closer than `radius`: (lims int64 [n + 1], ids int64 [lims[n]], dist float32 [lims[n]]);
        query i owns ids[lims[i]:lims[i + 1]] and dist[...] (the FAISS layout, ids first as everywhere here).  `radius`: a
        scalar or a float array [n], compared as float32 against the squared-L2 values the searches return; an id is a
        hit iff dist < radius (strict), so a radius <= 0 or NaN selects nothing and +inf every allowed id.
        exact=True (default): the candidates are the filter's ids, or the whole index, minus removed rows; EVERY hit is
        returned, each segment ascends by (distance, internal id), no id twice, and a distance has the bytes
        search_batch(..., exact=True) returns for the pair.  With result_ids = "input" the ids are input rows, in the
        same (internal-id) order.  exact=False needs max_results=K: segment i is row i of search_batch(queries, K,
        filter=filter) cut at the radius -- its entries with id >= 0 and dist < radius[i], in row order.
        A multi-device index shards the queries like search_batch(exact=True); the bytes are those of one device.
        Per-query filters (filter_of) and a partitioned index are refused (use part(i).range_search).
        `label`: one label value, instead of filter=label_filter(label).
        metric="cosine": `radius` and the distances are in 1 - cos (0 = same direction, 1 = orthogonal, 2 = opposite)."""
        q = _as_f32(queries)
        if q.ndim != 2 or q.shape[1] != self._dim:
            raise ValueError("queries must be a (n, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, None, lambda f, _: self.range_search(
                q, radius, filter=f, exact=exact, max_results=max_results))
        n = q.shape[0]
        r, f, K = self._range_args(n, radius, filter, exact, max_results, filter_of)
        L = _lib.lib()
        obj, total = C.c_void_p(), C.c_uint64(0)
        lims = np.zeros(n + 1, np.int64)
        qp, rp = (q.ctypes.data if n else None), (r.ctypes.data if n else None)
        if self._m is not None:
            fs = None if f is None else (C.c_void_p * len(f._hs))(*[h.value for h in f._hs])
            _lib.check(L.cph_multi_range_search_begin(self._m, qp, n, rp, fs, int(bool(exact)), K, C.byref(obj), C.byref(total)))
            finish, destroy = L.cph_multi_range_search_finish, L.cph_multi_range_destroy
            tail = ()
        else:
            _lib.check(L.cph_range_search_begin(self._h, qp, 0, n, rp, None if f is None else f._h, int(bool(exact)), K, None,
                                                C.byref(obj), C.byref(total)))
            finish, destroy = L.cph_range_search_finish, L.cph_range_destroy
            tail = (0,)
        try:
            ids = np.empty(total.value, np.int64)
            dist = np.empty(total.value, np.float32)
            _lib.check(finish(obj, lims.ctypes.data, ids.ctypes.data if total.value else None,
                              dist.ctypes.data if total.value else None, *tail))
        finally:
            destroy(obj)
        return lims, ids, dist

    def range_search_device(self, queries, radius, filter=None, exact=True, max_results=None, stream=None, filter_of=None,
                            label=None):
        """range_search on a float32 torch tensor (n, dim) on this index' device; returns (lims, ids, dist) with `lims`
        a CPU int64 tensor and ids / dist on the queries' device.  The kernels run on `stream` (default: torch's current
        stream), but unlike search_batch_device this call is NOT enqueue-only: the size of the output is data, so it
        waits once for the counts, allocates ids / dist, and waits for its own kernels before it returns -- the tensors
        are complete on return, and a filter may be closed right after the call.  `radius`: a scalar, an array, or a
        tensor (copied to the host).  A multi-device index runs the whole batch on one replica on the queries' device,
        alternating like search_batch_device.  `label`: as in range_search."""
        import torch
        if queries.dim() != 2 or queries.shape[1] != self._dim or queries.dtype != torch.float32:
            raise ValueError("queries must be a (n, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, None, lambda f, _: self.range_search_device(
                queries, radius, filter=f, exact=exact, max_results=max_results, stream=stream))
        n = queries.shape[0]
        r, f, K = self._range_args(n, radius, filter, exact, max_results, filter_of)
        rep = self._device_replica(queries)
        h = self._replicas()[rep]
        fresh = []
        if not queries.is_contiguous():
            queries = queries.contiguous()
            fresh.append(queries)                # (the copy belongs to the current stream)
        st, ext = self._search_stream(stream, queries, fresh)
        L = _lib.lib()
        obj, total = C.c_void_p(), C.c_uint64(0)
        _lib.check(L.cph_range_search_begin(h, queries.data_ptr() if n else None, 1, n, r.ctypes.data if n else None,
                                            None if f is None else f._hs[rep], int(bool(exact)), K, C.c_void_p(st), C.byref(obj),
                                            C.byref(total)))
        try:
            lims = torch.zeros(n + 1, dtype=torch.int64)
            ids = torch.empty(total.value, dtype=torch.int64, device=queries.device)
            dist = torch.empty(total.value, dtype=torch.float32, device=queries.device)
            if ext is not None:
                # The blocks belong to the current stream, whose earlier work may still use them: the fill runs after it.
                # (finish waits for its writes, so nothing has to be recorded for the allocator.)
                ext.wait_stream(torch.cuda.current_stream(queries.device))
            _lib.check(L.cph_range_search_finish(obj, lims.data_ptr(), ids.data_ptr() if total.value else None,
                                                 dist.data_ptr() if total.value else None, 1))
        finally:
            L.cph_range_destroy(obj)
        return lims, ids, dist

    # -- grouped search (not in the reference) --------------------------------------------------
    GROUP_MAX_CANDIDATES = 1024

    def make_group_keys(self, keys, ids=None):
        """GroupKeys from an integer array [size] whose values fit int32, indexed in the space `ids` ("internal" or
        "input"; default: result_ids, as for set_labels): the `keys=` argument of search_grouped, for grouping by
        something else than the label column."""
        self._no_parts("make_group_keys")
        space = self._id_space(ids)
        a = self._as_labels(keys, "keys")
        if a.ndim != 1 or a.shape[0] != self.size:
            raise ValueError(f"keys must be a 1D integer array of length {self.size} (the index size)")
        return GroupKeys(self, a, input_rows=space == "input")

    # -- what grouped, diverse and maxsim search share: one validation tail, one host call, one device call ----------
    def _group_keys_arg(self, keys, what):
        """The `keys=` of search_grouped / search_maxsim (`what`): an open GroupKeys of this index, or None and a label
        column."""
        if keys is not None:
            if not isinstance(keys, GroupKeys):
                raise ValueError("keys must be a GroupKeys object (make_group_keys)")
            if not keys._hs:
                raise ValueError("group keys were closed")
            if len(keys._hs) != len(self._replicas()):
                raise ValueError("group keys were made for an index with another number of replicas")
        elif not self.has_labels:
            raise ValueError(f"{what} needs keys: call set_labels first, or pass keys=make_group_keys(...)")
        return keys

    def _filters_arg(self, filter, filter_of, n):
        """-> ([IdFilter] or None, filter_of or None, IdFilter or None), as _filter_args takes them."""
        fs, fo = self._filter_list(filter, filter_of, n)
        return fs, fo, None if (fs is not None or filter is None) else self._filter(filter)

    def _rerank_host(self, name, q, lead, keys, filters, exact, table):
        """cph_search_<name>, or cph_multi_search_<name> on a multi-device index, over the float32 array q [n, ...] ->
        the outputs, allocated from `table` = ((shape, dtype name), ...).  `lead`: the scalars between n and the keys;
        `keys`: a GroupKeys, None (the label column), or False where the entry takes none; `filters`: _filters_arg."""
        n, multi = q.shape[0], self._m is not None
        out = tuple(np.empty(sh, dt) for sh, dt in table)
        fh, nf, fop = self._filter_args(*filters, None if multi else 0)
        if keys is False:
            kh = ()
        elif keys is None or not multi:
            kh = (None if keys is None else keys._hs[0],)
        else:
            kh = ((C.c_void_p * len(keys._hs))(*[h.value for h in keys._hs]),)
        fn = getattr(_lib.lib(), ("cph_multi_search_" if multi else "cph_search_") + name)
        _lib.check(fn(self._m if multi else self._h, q.ctypes.data if n else None, n, *lead, *kh, fh, nf, fop, int(bool(exact)),
                      *[o.ctypes.data if n else None for o in out]))
        return out

    def _rerank_device(self, name, queries, lead, keys, filters, exact, table, out, stream, out_what):
        """cph_search_<name>_device over the float32 torch tensor `queries` on the stream of _search_stream -> the list of
        outputs: `out` checked against `table` (a uint8 output may be bool; out_what = the two refusals), or allocated
        from it.  The other arguments are those of _rerank_host."""
        import torch
        n = queries.shape[0]
        rep = self._device_replica(queries)
        fresh = []                       # tensors allocated here, on torch's current stream
        if not queries.is_contiguous():
            queries = queries.contiguous()
            fresh.append(queries)
        table = [(sh, getattr(torch, dt)) for sh, dt in table]
        if out is None:
            res = [torch.empty(sh, dtype=dt, device=queries.device) for sh, dt in table]
            fresh += res
        else:
            res = list(out)
            if len(res) != len(table):
                raise ValueError(out_what[0])
            for t, (sh, dt) in zip(res, table):
                ok_dt = t.dtype == dt or (dt == torch.uint8 and t.dtype == torch.bool)
                if tuple(t.shape) != sh or not ok_dt or t.device != queries.device or not t.is_contiguous():
                    raise ValueError(out_what[1])
        st, _ = self._search_stream(stream, queries, fresh)
        fh, nf, fop = self._filter_args(*filters, rep)
        kh = () if keys is False else (None if keys is None else keys._hs[rep],)
        fn = getattr(_lib.lib(), f"cph_search_{name}_device")
        _lib.check(fn(self._replicas()[rep], queries.data_ptr() if n else None, n, *lead, *kh, fh, nf, fop, int(bool(exact)),
                      *[t.data_ptr() if n else None for t in res], C.c_void_p(st)))
        return res

    @staticmethod
    def _grouped_table(n, k, g):
        return (((n, k, g), "int64"), ((n, k, g), "float32"), ((n, k), "int32"), ((n, k), "int32"), ((n,), "uint8"))

    def _grouped_args(self, n, k, group_size, keys, candidates, filter, filter_of):
        """Validation shared by both grouped entry points -> (k, g, C or None, GroupKeys or None, [IdFilter] or None,
        filter_of or None, IdFilter or None)."""
        if self._p is not None:
            raise ValueError("search_grouped is not defined on a partitioned index (every part has its own internal ids and "
                             "its own slice of the labels): use part(i).search_grouped")
        k, g = int(k), int(group_size)
        cap = self.GROUP_MAX_CANDIDATES
        if k < 1 or g < 1:
            raise ValueError("search_grouped needs k >= 1 and group_size >= 1")
        if k * g > cap:
            raise ValueError(f"search_grouped needs k * group_size <= {cap} (the longest candidate row)")
        if candidates is not None:
            candidates = int(candidates)
            if not k * g <= candidates <= cap:
                raise ValueError(f"candidates must lie in [k * group_size, {cap}]")
        return (k, g, candidates, self._group_keys_arg(keys, "search_grouped")) + self._filters_arg(filter, filter_of, n)

    def _grouped_pass(self, q, k, g, C_, keys, fs, fo, f, exact):
        """One pass of the host form at C_ candidates over the float32 array q [n, dim] -> the five arrays."""
        return self._rerank_host("grouped", q, (k, g, C_), keys, (fs, fo, f), exact, self._grouped_table(q.shape[0], k, g))

    def search_grouped(self, queries, k=DEFAULT_K, group_size=1, keys=None, candidates=None, filter=None, exact=False,
                       filter_of=None, label=None):
        """The k best key groups of every query, up to group_size rows of each (group-by / collapse):
        (ids int64 [n, k, g], dist float32 [n, k, g], keys int32 [n, k], counts int32 [n, k], complete bool [n]).
        Rows that share a key answer as one group; the key of a row is its label (set_labels), or its entry in
        `keys` (make_group_keys).  A query's candidate row is row i of search_batch(queries, C, filter=..., exact=...,
        filter_of=...) -- same routing, removed rows, tail and refusals -- walked front to back: padding and repeated ids
        are skipped, a new key opens a group while fewer than k exist, an entry joins its key's group while that has fewer
        than g members, everything else is dropped.  Groups are ordered by their best member, members ascend, ties keep
        the order of the search; every int32 value is an ordinary key.  ids are padded with -1 (input rows under
        result_ids = "input"), dist with FLT_MAX, keys and counts with 0; counts[i, j] == 0 means no group j.
        complete[i]: k groups with g members each were found, or the candidate row held fewer than C ids (the search ran
        dry: a longer row would add nothing).  With exact=True and complete[i] the answer is the exact grouped top-k
        over the allowed ids.
        `candidates=C` (k * g <= C <= 1024) runs one pass at that C.  candidates=None is a policy, not a measured
        optimum: one pass at C0 = min(1024, max(64, 4 * k * g)), then the queries that came back incomplete are run
        again at min(4 * C, 1024) until they are complete or C is 1024; a query's answer is that of the last pass it
        took part in.  complete[i] can still be False at C = 1024: the 1,024 nearest candidates did not fill the groups
        (a few keys own most near rows); the groups returned are the best of those candidates.
        `label`: as in search_batch (it restricts the rows; the groups still come from the label column or `keys`).
        A multi-device index shards the queries like search_batch; the bytes are those of one device.  A partitioned
        index is refused (use part(i).search_grouped).
        metric="cosine": distances are 1 - cos(query, row)."""
        q = _as_f32(queries)
        if q.ndim != 2 or q.shape[1] != self._dim:
            raise ValueError("queries must be a (n, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, q.shape[0], lambda f, fo: self.search_grouped(
                q, k, group_size, keys=keys, candidates=candidates, filter=f, exact=exact, filter_of=fo))
        n = q.shape[0]
        k, g, C_, keys, fs, fo, f = self._grouped_args(n, k, group_size, keys, candidates, filter, filter_of)
        if C_ is not None:
            out = self._grouped_pass(q, k, g, C_, keys, fs, fo, f, exact)
            return out[:4] + (out[4].astype(bool),)
        cap = self.GROUP_MAX_CANDIDATES
        C_ = min(cap, max(64, 4 * k * g))
        out = self._grouped_pass(q, k, g, C_, keys, fs, fo, f, exact)
        todo = np.flatnonzero(out[4] == 0)
        while todo.size and C_ < cap:
            C_ = min(4 * C_, cap)
            sub = self._grouped_pass(np.ascontiguousarray(q[todo]), k, g, C_, keys, fs,
                                     None if fo is None else np.ascontiguousarray(fo[todo]), f, exact)
            for o, s_ in zip(out, sub):
                o[todo] = s_
            todo = todo[sub[4] == 0]
        return out[:4] + (out[4].astype(bool),)

    def search_grouped_device(self, queries, k=DEFAULT_K, group_size=1, keys=None, candidates=None, out=None, stream=None,
                              filter=None, exact=False, filter_of=None, label=None):
        """search_grouped on a float32 torch tensor (n, dim) on this index' device; returns the five outputs as torch
        tensors on the same device (complete: bool).  Like search_batch_device it only enqueues, on `stream` (default:
        torch's current stream), and never waits: the tensors are valid in stream order, two batches on two streams
        overlap.  ONE pass: at `candidates`, or (None) at the C0 of search_grouped -- re-running incomplete queries
        would need `complete` on the host.  `out`: the five tensors to write (contiguous, on the queries' device;
        complete as uint8 or bool).  filter / filter_of / label are host data as in search_batch_device; a filter or
        GroupKeys closed after the call waits for the batch.  A multi-device index runs the whole batch on one replica
        on the queries' device."""
        import torch
        if queries.dim() != 2 or queries.shape[1] != self._dim or queries.dtype != torch.float32:
            raise ValueError("queries must be a (n, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, queries.shape[0], lambda f, fo: self.search_grouped_device(
                queries, k, group_size, keys=keys, candidates=candidates, out=out, stream=stream, filter=f, exact=exact,
                filter_of=fo))
        n = queries.shape[0]
        k, g, C_, keys, fs, fo, f = self._grouped_args(n, k, group_size, keys, candidates, filter, filter_of)
        if C_ is None:
            C_ = min(self.GROUP_MAX_CANDIDATES, max(64, 4 * k * g))
        res = self._rerank_device("grouped", queries, (k, g, C_), keys, (fs, fo, f), exact, self._grouped_table(n, k, g), out, stream,
                                  ("out must be the five tensors (ids, dist, keys, counts, complete)",
                                   "out must be contiguous (n, k, g) int64 / float32, (n, k) int32 / int32 and (n,) uint8 tensors on the "
                                   "queries' device"))
        if res[4].dtype != torch.bool:
            res[4] = res[4].view(torch.bool)
        return tuple(res)

    def time_grouped(self, on=True):
        """Debug hook of the measurement script: while on, the group kernel of every grouped search is bracketed by HIP
        events (last_group_rows_us).  Off by default."""
        self._time_pass("cph_debug_time_grouped", on)

    def last_group_rows_us(self, replica=0):
        """Device time (HIP events, microseconds) of the group kernel of the last grouped search made under
        time_grouped() on the given replica; waits for that launch."""
        return self._last_pass_us("cph_debug_last_group_rows_us", replica)

    # -- diversified search (not in the reference) ----------------------------------------------
    DIVERSE_MAX_CANDIDATES = 1024

    def _diverse_args(self, n, k, lam, candidates, filter, filter_of):
        """Validation shared by both diverse entry points -> (k, lam, C, the filters as of _filters_arg)."""
        if self._p is not None:
            raise ValueError("search_diverse is not defined on a partitioned index (every part has its own internal ids): "
                             "use part(i).search_diverse")
        k, lam = int(k), float(lam)
        cap = self.DIVERSE_MAX_CANDIDATES
        if k < 1:
            raise ValueError("search_diverse needs k >= 1")
        if not 0.0 <= lam <= 1.0:                    # (NaN fails both comparisons)
            raise ValueError("search_diverse needs lam in [0, 1]")
        if candidates is None:
            if k > cap:
                raise ValueError(f"search_diverse needs k <= {cap} (the longest candidate row)")
            candidates = min(cap, max(64, 4 * k))    # a policy, not a measured optimum
        candidates = int(candidates)
        if not k <= candidates <= cap:
            raise ValueError(f"candidates must lie in [k, {cap}]")
        return k, lam, candidates, self._filters_arg(filter, filter_of, n)

    @staticmethod
    def _diverse_table(n, k):
        return (((n, k), "int64"), ((n, k), "float32"), ((n, k), "float32"))

    def search_diverse(self, queries, k=DEFAULT_K, lam=0.5, candidates=None, filter=None, exact=False, filter_of=None,
                       label=None):
        """k results per query that are close to the query and not copies of each other (maximal marginal relevance),
        re-ranked on the device: (ids int64 [n, k], dist float32 [n, k], gap float32 [n, k]), in PICK order, not ascending.
        A query's candidate row is row i of search_batch(queries, C, filter=..., exact=..., filter_of=...) -- same
        routing, removed rows, tail and refusals -- with padding and repeated ids skipped.  Pick 0 is the nearest
        candidate.  Every later pick minimises lam * dist_j - (1 - lam) * m_j over the unpicked candidates, m_j = the
        smallest distance from j to a row picked so far (float32, the arithmetic of exact_l2; equal scores go to the
        earlier candidate).  dist[i, t] is the pick's distance to the query, gap[i, t] its m when it was taken (FLT_MAX
        for pick 0).  Fewer than k candidates: ids padded with -1 (input rows under result_ids = "input"), dist and gap
        with FLT_MAX.  lam = 1 is the plain search with repeats dropped, lam = 0 a farthest-point walk.
        `candidates=C` (k <= C <= 1024) is the length of the candidate row; candidates=None takes
        C = min(1024, max(64, 4 * k)): a policy, not a measured optimum, in ONE pass (nothing is re-run at a larger C).
        last_search_stats() afterwards reports the underlying search only: the pair distances of the re-ranking are not
        added to exact_l2.  A multi-device index shards the queries like search_batch; the bytes are those of one
        device.  A partitioned index is refused (use part(i).search_diverse).
        metric="cosine": dist and gap are 1 - cos (to the query, and between stored rows); the formula is unchanged."""
        q = _as_f32(queries)
        if q.ndim != 2 or q.shape[1] != self._dim:
            raise ValueError("queries must be a (n, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, q.shape[0], lambda f, fo: self.search_diverse(
                q, k, lam, candidates=candidates, filter=f, exact=exact, filter_of=fo))
        k, lam, C_, filters = self._diverse_args(q.shape[0], k, lam, candidates, filter, filter_of)
        return self._rerank_host("diverse", q, (k, lam, C_), False, filters, exact, self._diverse_table(q.shape[0], k))

    def search_diverse_device(self, queries, k=DEFAULT_K, lam=0.5, candidates=None, out=None, stream=None, filter=None,
                              exact=False, filter_of=None, label=None):
        """search_diverse on a float32 torch tensor (n, dim) on this index' device; returns (ids, dist, gap) as torch
        tensors on the same device.  Like search_batch_device it only enqueues, on `stream` (default: torch's current
        stream), and never waits: the tensors are valid in stream order, two batches on two streams overlap.  `out`: the
        three tensors to write (contiguous, on the queries' device).  filter / filter_of / label are host data as in
        search_batch_device; a filter closed after the call waits for the batch.  A multi-device index runs the whole
        batch on one replica on the queries' device."""
        import torch
        if queries.dim() != 2 or queries.shape[1] != self._dim or queries.dtype != torch.float32:
            raise ValueError("queries must be a (n, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, queries.shape[0], lambda f, fo: self.search_diverse_device(
                queries, k, lam, candidates=candidates, out=out, stream=stream, filter=f, exact=exact, filter_of=fo))
        n = queries.shape[0]
        k, lam, C_, filters = self._diverse_args(n, k, lam, candidates, filter, filter_of)
        return tuple(self._rerank_device("diverse", queries, (k, lam, C_), False, filters, exact, self._diverse_table(n, k), out, stream,
                                         ("out must be the three tensors (ids, dist, gap)",
                                          "out must be contiguous (n, k) int64 / float32 / float32 tensors on the queries' device")))

    def time_diverse(self, on=True):
        """Debug hook of the measurement script: while on, the re-ranking kernel of every diverse search is bracketed by
        HIP events (last_diverse_rows_us).  Off by default."""
        self._time_pass("cph_debug_time_diverse", on)

    def last_diverse_rows_us(self, replica=0):
        """Device time (HIP events, microseconds) of the re-ranking kernel of the last diverse search made under
        time_diverse() on the given replica; waits for that launch."""
        return self._last_pass_us("cph_debug_last_diverse_rows_us", replica)

    # -- multi-vector search (not in the reference) ----------------------------------------------
    MAXSIM_MAX_TOKENS = 64
    MAXSIM_MAX_CANDIDATES = 1024
    MAXSIM_MAX_ENTRIES = 8192          # tokens * candidates: what the kernel sorts in LDS
    MAXSIM_MAX_K = 1024

    def _maxsim_args(self, n, T, k, n_tokens, candidates, keys, filter, filter_of):
        """Validation shared by both maxsim entry points -> (k, C, n_tokens as int32 [n] or None, GroupKeys or None, the
        filters as of _filters_arg)."""
        if self._p is not None:
            raise ValueError("search_maxsim is not defined on a partitioned index (every part has its own internal ids and "
                             "its own slice of the labels): use part(i).search_maxsim")
        k = int(k)
        if not 1 <= T <= self.MAXSIM_MAX_TOKENS:
            raise ValueError(f"search_maxsim needs 1 <= tokens <= {self.MAXSIM_MAX_TOKENS} (queries is [n, tokens, dim]), got {T}")
        if not 1 <= k <= self.MAXSIM_MAX_K:
            raise ValueError(f"search_maxsim needs 1 <= k <= {self.MAXSIM_MAX_K}")
        if candidates is None:                       # a policy, not a measured optimum
            candidates = min(self.MAXSIM_MAX_CANDIDATES, self.MAXSIM_MAX_ENTRIES // T, max(32, 4 * k))
        candidates = int(candidates)
        if not 1 <= candidates <= self.MAXSIM_MAX_CANDIDATES:
            raise ValueError(f"candidates must lie in [1, {self.MAXSIM_MAX_CANDIDATES}]")
        if T * candidates > self.MAXSIM_MAX_ENTRIES:
            raise ValueError(f"search_maxsim needs tokens * candidates <= {self.MAXSIM_MAX_ENTRIES} (got {T} * {candidates})")
        if n * T > 0x7FFFFFFF:
            raise ValueError("search_maxsim needs n * tokens <= 2147483647")
        if n_tokens is not None:
            nt = np.asarray(n_tokens)
            if nt.ndim != 1 or nt.shape[0] != n or not (nt.size == 0 or np.issubdtype(nt.dtype, np.integer)):
                raise ValueError(f"n_tokens must be a 1D integer array of length {n} (one entry per query)")
            if nt.size and (nt.min() < 1 or nt.max() > T):
                raise ValueError(f"n_tokens values must lie in [1, {T}]")
            n_tokens = np.ascontiguousarray(nt, np.int32)
        return k, candidates, n_tokens, self._group_keys_arg(keys, "search_maxsim"), self._filters_arg(filter, filter_of, n)

    @staticmethod
    def _maxsim_call(n, T, k, C_, nt):
        """-> (the scalars between n and the keys, the output table)."""
        return ((T, None if (nt is None or n == 0) else nt.ctypes.data, k, C_),
                (((n, k), "int32"), ((n, k), "float32"), ((n, k), "int32"), ((n, k, T), "int64"), ((n,), "int32")))

    MAXSIM_MAX_RESCORE = 1024

    def _maxsim_rescore_arg(self, rescore, k):
        """rescore=R of search_maxsim / search_maxsim_device -> R, checked against k <= R <= 1024."""
        if isinstance(rescore, bool) or not isinstance(rescore, (int, np.integer)):
            raise ValueError("rescore must be an integer (the number of keys to rescore) or None")
        R = int(rescore)
        if not int(k) <= R <= self.MAXSIM_MAX_RESCORE:
            raise ValueError(f"search_maxsim needs k <= rescore <= {self.MAXSIM_MAX_RESCORE} (got rescore={R} at k={int(k)})")
        return R

    @staticmethod
    def _maxsim_rescored_call(n, T, k, C_, nt, R):
        """-> (the scalars between n and the keys, the output table) of the rescored entries."""
        lead, table = CPIndex._maxsim_call(n, T, k, C_, nt)
        return lead + (R,), table + (((n,), "int32"),)

    def prepare_maxsim_rescore(self, keys=None):
        """Builds the inverted key column search_maxsim(..., rescore=R) walks -- of `keys` (a GroupKeys), or of the label
        column -- ahead of the first rescored call, which would otherwise build it and wait for the device.  It is made
        once per column: set_labels, add, compact, load and build drop the label column's; a GroupKeys keeps its own."""
        if self._p is not None:
            raise ValueError("search_maxsim is not defined on a partitioned index (every part has its own internal ids and "
                             "its own slice of the labels): use part(i).prepare_maxsim_rescore")
        keys = self._group_keys_arg(keys, "prepare_maxsim_rescore")
        for r, rh in enumerate(self._replicas()):
            _lib.check(_lib.lib().cph_prepare_maxsim_rescore(rh, None if keys is None else keys._hs[r]))

    def search_maxsim(self, queries, k=DEFAULT_K, n_tokens=None, candidates=None, keys=None, filter=None, exact=False,
                      filter_of=None, label=None, rescore=None):
        """Multi-vector (late-interaction, ColBERT / ColPali style) search: `queries` is float32 [n, T, dim], T token vectors
        per query of which the first n_tokens[i] (default: all T) are live; returns the k keys (documents) that minimise
        the sum, over the live tokens, of the token's best row of the key:
        (keys int32 [n, k], score float32 [n, k], hits int32 [n, k], rows int64 [n, k, T], found int32 [n]).
        The key of a row is its label (set_labels) or its entry in `keys` (make_group_keys); every int32 value is an
        ordinary key.  The statement, over the T candidate rows search_batch(queries.reshape(n * T, dim), C, filter=...,
        exact=..., ...) returns for a query -- same routing, removed rows, tail and refusals; `filter_of[i]` and `label[i]`
        serve all T tokens of query i -- in internal ids, an entry being valid when it is not padding:
          floor_t = the distance of the last valid entry of row t (+0.0 when there is none);
          pos_t(key) = the lowest position of row t whose entry has the key; term_t(key) = the distance there, else floor_t;
          score(key) = ((+0.0 + term_0) + term_1) + ... over t < n_tokens, in float32, in that order;
          hits(key) = the live tokens that have a pos_t(key);
        the min(k, distinct keys) keys with the smallest (score, key) are returned in that order, found[i] of them;
        rows[i, j, t] is the id at pos_t (input rows under result_ids = "input"), -1 where token t has no row of the key or
        t >= n_tokens[i].  Padding: key 0, score FLT_MAX, hits 0, rows -1.  The tokens t >= n_tokens[i] are searched with
        the batch and then ignored entirely.
        Lower bound: floor_t is the C-th distance of token t, and a row of the key that the search did not return for t is
        no closer.  With exact=True score is therefore a lower bound of the true sum_t min over the key's allowed rows of
        dist(q_t, row) -- in float32 too -- and equal to it where hits == n_tokens; with exact=True and C at least the
        number of allowed rows the answer is the exact MaxSim top-k.  hits is this call's counterpart of `complete` in
        search_grouped; nothing is re-run on low hits.
        cosine: MaxSim similarity = n_tokens - score.
        `candidates=C` (1 <= C <= 1024, T * C <= 8192) is the length of every token's candidate row; candidates=None takes
        C0 = min(1024, 8192 // T, max(32, 4 * k)): a policy, not a measured optimum, in ONE pass.  Limits: 1 <= T <= 64,
        1 <= k <= 1024, n * T <= 2^31 - 1.  A multi-device index shards the QUERIES like search_batch, never the tokens of
        one query; the bytes are those of one device.  A partitioned index is refused (use part(i).search_maxsim).
        `rescore=R` (k <= R <= 1024; None: everything above, five outputs) adds the second stage of a late-interaction
        retriever and returns SIX outputs, (keys, score, hits, rows, found, certified int32 [n]): the statement above at
        k = R gives the candidate keys and their lower bounds lb_j in (lb, key) order; every candidate is then scored against
        ALL its allowed rows -- the ids with that key in the query's effective filter (the caller's filter AND not removed,
        tail rows included) -- per live token the row with the smallest (distance, internal id), the distance having the
        bytes of exact_l2 for the token vector the search saw (cosine: normalised); score is the same sequential float32 sum
        over those distances, hits == n_tokens in every real slot, rows holds the argmin ids, and the min(k, found at R)
        candidates with the smallest (score, key) are returned.  certified[i] is the number of leading slots whose score is
        strictly below lb_{R-1} (found[i] when fewer than R keys were found): every key outside the candidates has a lower
        bound of at least lb_{R-1}, so with exact=True those leading slots are the true MaxSim top slots over the allowed
        rows, in the true order; with a graph-routed search the bound is relative to the candidate rows the search returned,
        not to the index.  The first rescored call on a key column builds its inverted form on the host and waits for the
        device (prepare_maxsim_rescore does it ahead of time)."""
        q = _as_f32(queries)
        if q.ndim != 3 or q.shape[2] != self._dim:
            raise ValueError("queries must be a (n, tokens, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, q.shape[0], lambda f, fo: self.search_maxsim(
                q, k, n_tokens=n_tokens, candidates=candidates, keys=keys, filter=f, exact=exact, filter_of=fo, rescore=rescore))
        n, T = q.shape[0], q.shape[1]
        k, C_, nt, keys, filters = self._maxsim_args(n, T, k, n_tokens, candidates, keys, filter, filter_of)
        if rescore is not None:
            lead, table = self._maxsim_rescored_call(n, T, k, C_, nt, self._maxsim_rescore_arg(rescore, k))
            return self._rerank_host("maxsim_rescored", q, lead, keys, filters, exact, table)
        lead, table = self._maxsim_call(n, T, k, C_, nt)
        return self._rerank_host("maxsim", q, lead, keys, filters, exact, table)

    def search_maxsim_device(self, queries, k=DEFAULT_K, n_tokens=None, candidates=None, keys=None, out=None, stream=None,
                             filter=None, exact=False, filter_of=None, label=None, rescore=None):
        """search_maxsim on a float32 torch tensor (n, T, dim) on this index' device; returns the five outputs as torch
        tensors on the same device.  Like search_batch_device it only enqueues, on `stream` (default: torch's current
        stream), and waits for no kernel: the tensors are valid in stream order, two batches on two streams overlap.
        ONE pass at `candidates`, or (None) at the C0 of search_maxsim.  `out`: the five tensors to write (contiguous, on
        the queries' device).  n_tokens / filter / filter_of / label are host data as in search_batch_device (n_tokens is
        copied to the device through a pinned buffer by a command on `stream`); a filter or GroupKeys closed after the
        call waits for the batch.  A multi-device index runs the whole batch on one replica on the queries' device.
        cosine: MaxSim similarity = n_tokens - score.
        `rescore=R`: the six outputs of search_maxsim(..., rescore=R) (`out`: six tensors, the last (n,) int32).  The first
        rescored call on a key column builds its inverted form and waits for the device -- the one exception to "only
        enqueues"; prepare_maxsim_rescore builds it ahead of time."""
        import torch
        if queries.dim() != 3 or queries.shape[2] != self._dim or queries.dtype != torch.float32:
            raise ValueError("queries must be a (n, tokens, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, queries.shape[0], lambda f, fo: self.search_maxsim_device(
                queries, k, n_tokens=n_tokens, candidates=candidates, keys=keys, out=out, stream=stream, filter=f, exact=exact,
                filter_of=fo, rescore=rescore))
        n, T = queries.shape[0], queries.shape[1]
        k, C_, nt, keys, filters = self._maxsim_args(n, T, k, n_tokens, candidates, keys, filter, filter_of)
        if rescore is not None:
            lead, table = self._maxsim_rescored_call(n, T, k, C_, nt, self._maxsim_rescore_arg(rescore, k))
            return tuple(self._rerank_device("maxsim_rescored", queries, lead, keys, filters, exact, table, out, stream,
                                             ("out must be the six tensors (keys, score, hits, rows, found, certified)",
                                              "out must be contiguous (n, k) int32 / float32 / int32, (n, k, tokens) int64, (n,) int32 "
                                              "and (n,) int32 tensors on the queries' device")))
        lead, table = self._maxsim_call(n, T, k, C_, nt)
        return tuple(self._rerank_device("maxsim", queries, lead, keys, filters, exact, table, out, stream,
                                         ("out must be the five tensors (keys, score, hits, rows, found)",
                                          "out must be contiguous (n, k) int32 / float32 / int32, (n, k, tokens) int64 and (n,) int32 "
                                          "tensors on the queries' device")))

    def time_maxsim(self, on=True):
        """Debug hook of the measurement script: while on, the maxsim kernel of every maxsim search is bracketed by HIP
        events (last_maxsim_rows_us).  Off by default."""
        self._time_pass("cph_debug_time_maxsim", on)

    def last_maxsim_rows_us(self, replica=0):
        """Device time (HIP events, microseconds) of the maxsim kernel of the last maxsim search made under time_maxsim()
        on the given replica; waits for that launch."""
        return self._last_pass_us("cph_debug_last_maxsim_rows_us", replica)

    def time_maxsim_rescore(self, on=True):
        """Debug hook of the measurement script: while on, the scan kernel of every rescored maxsim search (the exact terms;
        not the lower-bound kernel, the pad or the select) is bracketed by HIP events (last_maxsim_rescore_us)."""
        self._time_pass("cph_debug_time_maxsim_rescore", on)

    def last_maxsim_rescore_us(self, replica=0):
        """Device time (HIP events, microseconds) of the scan kernel of the last rescored maxsim search made under
        time_maxsim_rescore() on the given replica; waits for it."""
        return self._last_pass_us("cph_debug_last_maxsim_rescore_us", replica)

    # -- fused search: several query vectors per query (not in the reference) -------------------------
    FUSED_MAX_VECTORS = MAXSIM_MAX_TOKENS
    FUSED_MAX_CANDIDATES = MAXSIM_MAX_CANDIDATES
    FUSED_MAX_ENTRIES = MAXSIM_MAX_ENTRIES          # vectors * candidates: what the union kernel sorts in LDS
    FUSED_MAX_K = MAXSIM_MAX_K

    def _fused_args(self, n, T, k, weights, n_vectors, candidates, filter, filter_of):
        """Validation shared by both fused entry points -> (k, C, weights as float32 [n, T], n_vectors as int32 [n] or None,
        the filters as of _filters_arg)."""
        if self._p is not None:
            raise ValueError("search_fused is not defined on a partitioned index (every part has its own internal ids): "
                             "use part(i).search_fused")
        k = int(k)
        if not 1 <= T <= self.FUSED_MAX_VECTORS:
            raise ValueError(f"search_fused needs 1 <= vectors <= {self.FUSED_MAX_VECTORS} (queries is [n, vectors, dim]), got {T}")
        if not 1 <= k <= self.FUSED_MAX_K:
            raise ValueError(f"search_fused needs 1 <= k <= {self.FUSED_MAX_K}")
        if candidates is None:                       # a policy, not a measured optimum
            candidates = min(self.FUSED_MAX_CANDIDATES, self.FUSED_MAX_ENTRIES // T, max(32, 4 * k))
        candidates = int(candidates)
        if not 1 <= candidates <= self.FUSED_MAX_CANDIDATES:
            raise ValueError(f"search_fused needs candidates in [1, {self.FUSED_MAX_CANDIDATES}]")
        if T * candidates > self.FUSED_MAX_ENTRIES:
            raise ValueError(f"search_fused needs vectors * candidates <= {self.FUSED_MAX_ENTRIES} (got {T} * {candidates})")
        if k > T * candidates:
            raise ValueError(f"search_fused needs k <= vectors * candidates (got {k} > {T} * {candidates})")
        if n * T > 0x7FFFFFFF:
            raise ValueError("search_fused needs n * vectors <= 2147483647")
        if weights is None:
            w = np.ones((n, T), np.float32)
        else:
            w = np.asarray(weights, np.float32)
            if w.shape not in ((T,), (n, T)):
                raise ValueError(f"search_fused needs weights of shape ({T},) or ({n}, {T}) (one weight per query vector)")
            if not np.isfinite(w).all():
                raise ValueError("search_fused needs finite weights")
            w = np.ascontiguousarray(np.broadcast_to(w, (n, T)), np.float32)
        if n_vectors is not None:
            nv = np.asarray(n_vectors)
            if nv.ndim != 1 or nv.shape[0] != n or not (nv.size == 0 or np.issubdtype(nv.dtype, np.integer)):
                raise ValueError(f"search_fused needs n_vectors as a 1D integer array of length {n} (one entry per query)")
            if nv.size and (nv.min() < 1 or nv.max() > T):
                raise ValueError(f"search_fused needs n_vectors in [1, {T}]")
            n_vectors = np.ascontiguousarray(nv, np.int32)
        return k, candidates, w, n_vectors, self._filters_arg(filter, filter_of, n)

    @staticmethod
    def _fused_call(n, T, k, C_, w, nv):
        """-> (the scalars between n and the filters, the output table)."""
        return ((T, None if (nv is None or n == 0) else nv.ctypes.data, w.ctypes.data if n else None, k, C_),
                (((n, k), "int64"), ((n, k), "float32"), ((n, k), "int32")))

    def search_fused(self, queries, k=DEFAULT_K, weights=None, n_vectors=None, candidates=None, filter=None, exact=False,
                     filter_of=None, label=None):
        """Several query vectors per query, one ranked list of rows: `queries` is float32 [n, T, dim] -- rewrites of one
        question (query expansion), liked (weight > 0) and disliked (weight < 0) examples, an image and a text vector -- of
        which the first n_vectors[i] (default: all T) are live; `weights` is [T] (every query) or [n, T], float32, finite,
        any sign, default all ones.  Returns (ids int64 [n, k], score float32 [n, k], hits int32 [n, k]).
        The statement, over the T candidate rows search_batch(queries.reshape(n * T, dim), C, filter=..., exact=..., ...)
        returns for a query in internal ids -- same routing, removed and added rows and refusals; `filter_of[i]` and
        `label[i]` serve all T vectors of query i; the distances of that search are used for nothing else:
          the candidates are the DISTINCT ids in the rows of the live vectors; hits(x) = the live vectors whose row holds x;
          d_t(x) = exact_l2 of vector t (cosine: normalised, as the search saw it) and id x, for EVERY live t;
          score(x) = s = +0.0; for t < n_vectors: s = s + (w[t] * d_t(x)), float32, product and sum each rounded once;
          a candidate whose score is NaN (overflow under weights of both signs) is dropped;
        the k candidates with the smallest (score, internal id) are returned in that order, ids as input rows under
        result_ids = "input"; unused slots are -1 / FLT_MAX / 0.  No candidate has a missing term: a row that only one
        vector found is still scored against all of them.  With T = 1 and weight 1 the answer is the first k distinct ids of
        search_batch at k = C wherever that search's distance bytes are exact_l2's; scaling a query's weights by a power of
        two changes no id.  The tokens t >= n_vectors[i] are searched with the batch and then ignored entirely.
        `candidates=C` (1 <= C <= 1024, T * C <= 8192) is the length of every vector's candidate row; candidates=None takes
        min(1024, 8192 // T, max(32, 4 * k)): a policy, not a measured optimum, in ONE pass.  Limits: 1 <= T <= 64,
        1 <= k <= min(1024, T * C), n * T <= 2^31 - 1.  A multi-device index shards the QUERIES like search_batch, never the
        vectors of one query; the bytes are those of one device.  A partitioned index (use part(i).search_fused) and the
        inner-product metric are refused."""
        q = _as_f32(queries)
        if q.ndim != 3 or q.shape[2] != self._dim:
            raise ValueError("queries must be a (n, vectors, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, q.shape[0], lambda f, fo: self.search_fused(
                q, k, weights=weights, n_vectors=n_vectors, candidates=candidates, filter=f, exact=exact, filter_of=fo))
        n, T = q.shape[0], q.shape[1]
        k, C_, w, nv, filters = self._fused_args(n, T, k, weights, n_vectors, candidates, filter, filter_of)
        lead, table = self._fused_call(n, T, k, C_, w, nv)
        return self._rerank_host("fused", q, lead, False, filters, exact, table)

    def search_fused_device(self, queries, k=DEFAULT_K, weights=None, n_vectors=None, candidates=None, out=None, stream=None,
                            filter=None, exact=False, filter_of=None, label=None):
        """search_fused on a float32 torch tensor (n, T, dim) on this index' device; returns (ids, score, hits) as torch
        tensors on the same device.  Like search_batch_device it only enqueues, on `stream` (default: torch's current
        stream), and waits for no kernel: the tensors are valid in stream order, two batches on two streams overlap.  ONE
        pass at `candidates`, or (None) at the default of search_fused.  `out`: the three tensors to write (contiguous, on
        the queries' device).  weights / n_vectors / filter / filter_of / label are host data as in search_batch_device
        (weights and n_vectors are copied to the device through a pinned buffer by a command on `stream`); a filter closed
        after the call waits for the batch.  A multi-device index runs the whole batch on one replica on the queries'
        device."""
        import torch
        if queries.dim() != 3 or queries.shape[2] != self._dim or queries.dtype != torch.float32:
            raise ValueError("queries must be a (n, vectors, dim) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, queries.shape[0], lambda f, fo: self.search_fused_device(
                queries, k, weights=weights, n_vectors=n_vectors, candidates=candidates, out=out, stream=stream, filter=f,
                exact=exact, filter_of=fo))
        n, T = queries.shape[0], queries.shape[1]
        k, C_, w, nv, filters = self._fused_args(n, T, k, weights, n_vectors, candidates, filter, filter_of)
        lead, table = self._fused_call(n, T, k, C_, w, nv)
        return tuple(self._rerank_device("fused", queries, lead, False, filters, exact, table, out, stream,
                                         ("out must be the three tensors (ids, score, hits)",
                                          "out must be contiguous (n, k) int64 / float32 / int32 tensors on the queries' device")))

    def time_fused(self, on=True):
        """Debug hook of the measurement script: while on, the scan kernel of every fused search (the exact weighted sums;
        not the pad, the union or the select) is bracketed by HIP events (last_fused_us)."""
        self._time_pass("cph_debug_time_fused", on)

    def last_fused_us(self, replica=0):
        """Device time (HIP events, microseconds) of the scan kernel of the last fused search made under time_fused() on
        the given replica; waits for it."""
        return self._last_pass_us("cph_debug_last_fused_us", replica)

    # -- two-stage search: rescoring against full-size rows (not in the reference) -------------------
    RESCORE_MAX_CANDIDATES = 1024
    RESCORE_MAX_DIM = 8192

    def make_rescore_vectors(self, rows, ids=None, dtype="float16", metric="l2"):
        """RescoreVectors from a float32 or float16 array [size, dim_full] (1 <= dim_full <= 8192), one row per id of the
        index, indexed in the space `ids` ("internal" or "input"; default: result_ids, as for make_group_keys; the input
        form needs the row map): the `vectors` argument of search_rescored.  `dtype`: how the rows are stored on the
        device, "float16" (default; float32 input is rounded to nearest even) or "float32".  `metric`: "l2" or "ip"; it
        belongs to the object, not to the index -- for cosine, normalise the rows and the full queries yourself and use
        "ip".  ValueError names the lowest row that holds a NaN or an Inf, a value that overflows float16, or whose
        squared norm overflows, and how many there are; no object exists then."""
        self._no_parts("make_rescore_vectors")
        space = self._id_space(ids)
        if dtype not in ("float16", "float32"):
            raise ValueError('dtype must be "float16" or "float32"')
        if metric not in ("l2", "ip"):
            raise ValueError('metric must be "l2" or "ip" (cosine: normalise rows and full queries and use "ip")')
        a = np.asarray(rows)
        if a.dtype not in (np.float32, np.float16):
            raise ValueError("rows must be a float32 or float16 array")
        if a.ndim != 2 or a.shape[0] != self.size or not 1 <= a.shape[1] <= self.RESCORE_MAX_DIM:
            raise ValueError(f"rows must be a ({self.size}, dim_full) array (the index size), 1 <= dim_full <= {self.RESCORE_MAX_DIM}")
        return RescoreVectors(self, _as_f32(a), space == "input", dtype, metric)       # (float16 -> float32 is exact)

    def _rescored_args(self, n, k, vectors, candidates, filter, filter_of):
        """Validation shared by both rescored entry points -> (k, C, the filters as of _filters_arg)."""
        if self._p is not None:
            raise ValueError("search_rescored is not defined on a partitioned index (every part has its own internal ids): "
                             "use part(i).search_rescored")
        if not isinstance(vectors, RescoreVectors):
            raise ValueError("vectors must be a RescoreVectors object (make_rescore_vectors)")
        if not vectors._hs:
            raise ValueError("rescore vectors were closed")
        if len(vectors._hs) != len(self._replicas()):
            raise ValueError("rescore vectors were made for an index with another number of replicas")
        k = int(k)
        cap = self.RESCORE_MAX_CANDIDATES
        if k < 1:
            raise ValueError("search_rescored needs k >= 1")
        if candidates is None:
            if k > cap:
                raise ValueError(f"search_rescored needs k <= {cap} (the longest candidate row)")
            candidates = min(cap, max(64, 4 * k))    # a policy, not a measured optimum
        candidates = int(candidates)
        if not k <= candidates <= cap:
            raise ValueError(f"candidates must lie in [k, {cap}]")
        return k, candidates, self._filters_arg(filter, filter_of, n)

    @staticmethod
    def _rescored_table(n, k):
        return (((n, k), "int64"), ((n, k), "float32"), ((n, k), "float32"))

    def search_rescored(self, queries, k=DEFAULT_K, vectors=None, full_queries=None, candidates=None, filter=None, exact=False,
                        filter_of=None, label=None):
        """Two-stage search: (ids int64 [n, k], score float32 [n, k], first float32 [n, k]).  The index finds C candidates
        per query among its (narrow) rows, and the device rescores them against the full-size rows in `vectors`
        (make_rescore_vectors) with the full query; nothing but the k answers leaves the device.
        `queries` [n, dim] go to the graph and `full_queries` [n, dim_full] to the rescoring; with full_queries=None,
        `queries` is [n, dim_full] with dim_full >= dim and the graph searches its first dim coordinates (embeddings
        whose prefix is itself an embedding).  A query's candidate row is row i of search_batch(queries, C, filter=...,
        exact=..., filter_of=...) -- same routing, removed rows, tail and refusals -- with padding and repeated ids
        dropped.  Each candidate is scored in float32: "l2" max(0, (|q|^2 + |x|^2) - 2 q.x), "ip" -(q.x), x the STORED row
        (rounded to float16 under dtype="float16"); the k best by (score, internal id) ascending are returned, `first` is
        the candidate's first-stage distance; fewer than k candidates: ids padded with -1 (input rows under result_ids =
        "input"), score and first with FLT_MAX.  A query whose full vector has no finite squared norm gets padding.
        `candidates=C` (k <= C <= 1024); None takes C = min(1024, max(64, 4 * k)): a policy, not a measured optimum, in
        ONE pass.  A multi-device index shards the queries like search_batch; the bytes are those of one device.  A
        partitioned index is refused (use part(i).search_rescored), an inner-product index too: search a cosine or L2
        index and give the object metric="ip"."""
        q = _as_f32(queries)
        if full_queries is None:
            fq = q
            if q.ndim != 2 or q.shape[1] < self._dim:
                raise ValueError("queries must be a (n, dim_full) array with dim_full >= dim when full_queries is None")
            q = np.ascontiguousarray(q[:, :self._dim])
        else:
            fq = _as_f32(full_queries)
        if q.ndim != 2 or q.shape[1] != self._dim:
            raise ValueError("queries must be a (n, dim) array")
        if fq.ndim != 2 or fq.shape[0] != q.shape[0]:
            raise ValueError("full_queries must be a (n, dim_full) array")
        if label is not None:
            return self._with_label(label, filter, filter_of, q.shape[0], lambda f, fo: self.search_rescored(
                q, k, vectors, full_queries=fq, candidates=candidates, filter=f, exact=exact, filter_of=fo))
        n = q.shape[0]
        k, C_, filters = self._rescored_args(n, k, vectors, candidates, filter, filter_of)
        return self._rerank_host("rescored", q, (fq.ctypes.data if n else None, fq.shape[1], k, C_), vectors, filters, exact,
                                 self._rescored_table(n, k))

    def search_rescored_device(self, queries, k=DEFAULT_K, vectors=None, full_queries=None, candidates=None, out=None, stream=None,
                               filter=None, exact=False, filter_of=None, label=None):
        """search_rescored on float32 torch tensors on this index' device; returns (ids, score, first) as torch tensors on
        the same device.  Like search_batch_device it only enqueues, on `stream` (default: torch's current stream), and
        never waits.  With full_queries=None the contiguous prefix of `queries` is made on that stream.  `out`: the three
        tensors to write (contiguous, on the queries' device).  filter / filter_of / label are host data as in
        search_batch_device; a filter or RescoreVectors closed after the call waits for the batch.  A multi-device index
        runs the whole batch on one replica on the queries' device."""
        import torch
        if queries.dim() != 2 or queries.dtype != torch.float32:
            raise ValueError("queries must be a (n, dim) array")
        if full_queries is None:
            fq = queries
            if queries.shape[1] < self._dim:
                raise ValueError("queries must be a (n, dim_full) array with dim_full >= dim when full_queries is None")
            cur = torch.cuda.current_stream(queries.device)
            st = cur.cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
            on = cur if st == cur.cuda_stream else (stream if isinstance(stream, torch.cuda.Stream)
                                                    else torch.cuda.ExternalStream(st, device=queries.device))
            with torch.cuda.stream(on):
                queries = queries[:, :self._dim].contiguous()
        else:
            fq = full_queries
        if queries.shape[1] != self._dim:
            raise ValueError("queries must be a (n, dim) array")
        if (fq.dim() != 2 or fq.shape[0] != queries.shape[0] or fq.dtype != torch.float32 or fq.device != queries.device
                or not fq.is_contiguous()):
            raise ValueError("the full queries must be a contiguous float32 (n, dim_full) tensor on the queries' device")
        if label is not None:
            return self._with_label(label, filter, filter_of, queries.shape[0], lambda f, fo: self.search_rescored_device(
                queries, k, vectors, full_queries=fq, candidates=candidates, out=out, stream=stream, filter=f, exact=exact,
                filter_of=fo))
        n = queries.shape[0]
        k, C_, filters = self._rescored_args(n, k, vectors, candidates, filter, filter_of)
        return tuple(self._rerank_device("rescored", queries, (fq.data_ptr() if n else None, fq.shape[1], k, C_), vectors, filters, exact,
                                         self._rescored_table(n, k), out, stream,
                                         ("out must be the three tensors (ids, score, first)",
                                          "out must be contiguous (n, k) int64 / float32 / float32 tensors on the queries' device")))

    def time_rescored(self, on=True):
        """Debug hook of the measurement script: while on, the rescoring kernel of every rescored search is bracketed by
        HIP events (last_rescored_us).  Off by default."""
        self._time_pass("cph_debug_time_rescored", on)

    def last_rescored_us(self, replica=0):
        """Device time (HIP events, microseconds) of the rescoring kernel of the last rescored search made under
        time_rescored() on the given replica; waits for that launch."""
        return self._last_pass_us("cph_debug_last_rescored_us", replica)

    # -- removed rows (not in the reference) ---------------------------------------------------
    def _id_space(self, ids):
        space = self._result_ids if ids is None else ids
        if space not in ("internal", "input"):
            raise ValueError('ids must be "internal" or "input"')
        if self._p is not None and space != "input":
            raise ValueError('a partitioned index speaks input rows only (ids="input")')
        return space

    def remove(self, rows, ids=None):
        """Removes rows from the finalized index; returns how many were newly removed.  `rows`: an integer array of ids,
        in the space `ids` ("internal" or "input"; default: result_ids, as for make_filter).  An id outside [0, size)
        raises ValueError and changes nothing; duplicates and ids removed before are fine.  A removed row is a tombstone:
        it stays in the graph, `size` and every id keep their meaning, and every search from now on returns what the
        same call would return under the filter "caller's filter AND not removed" -- also filters made before the
        call.  Waits for the batches in flight.  The first removed row takes unfiltered batches off the probe-first
        kernel (they run the filtered one); compact() rebuilds the index without the removed rows."""
        space = self._id_space(ids)
        a = np.asarray(rows)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("remove takes an integer array of ids")
        r = np.ascontiguousarray(a.ravel(), np.int64)
        newly = C.c_uint64(0)
        ptr = r.ctypes.data if r.size else None
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_remove(self._p, ptr, r.size, C.byref(newly)))
            return newly.value
        code = _lib.IDS_INPUT if space == "input" else _lib.IDS_INTERNAL
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_remove(self._m, ptr, r.size, code, C.byref(newly)))
        else:
            _lib.check(_lib.lib().cph_remove(self._h, ptr, r.size, code, C.byref(newly)))
        return newly.value

    @property
    def live_count(self):
        """Rows that can still be returned: size minus the removed rows."""
        n = C.c_uint64(0)
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_live_count(self._p, C.byref(n)))
        elif self._m is not None:
            _lib.check(_lib.lib().cph_multi_live_count(self._m, C.byref(n)))
        else:
            _lib.check(_lib.lib().cph_live_count(self._h, C.byref(n)))
        return n.value

    def removed_mask(self, ids=None):
        """bool[size]: True where the id (in the space `ids`; default: result_ids) has been removed."""
        space = self._id_space(ids)
        n = self.size
        w = np.zeros((n + 31) // 32, np.uint32)
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_get_removed(self._p, w.ctypes.data))
        elif self._m is not None:
            _lib.check(_lib.lib().cph_multi_get_removed(self._m, w.ctypes.data))
        else:
            _lib.check(_lib.lib().cph_get_removed(self._h, w.ctypes.data))
        mask = np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)
        if space == "input" and self._p is None:
            by_row = np.zeros(n, bool)
            by_row[self.row_map()] = mask
            return by_row
        return mask

    def compact(self):
        """Rebuilds the index from the rows that are left (build + finalize of the live vectors in input-row order;
        internal-id order if the index has no row map).  Returns int64[old size]: the new input row of every old id, in
        the space remove() defaults to (result_ids), -1 for removed ids.  Afterwards size == live_count, nothing is
        removed, the index has a fresh row map and result_ids is kept.  A partitioned index is cut into parts again.
        Rows added with add() are folded into the new graph: they follow the base rows, in id order, and tail_size is 0
        afterwards."""
        out = np.empty(self.size, np.int64)
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_compact(self._p, out.ctypes.data))
        elif self._m is not None:
            _lib.check(_lib.lib().cph_multi_compact(self._m, out.ctypes.data))
        else:
            _lib.check(_lib.lib().cph_compact(self._h, out.ctypes.data))
        return out

    # -- added rows (not in the reference) -----------------------------------------------------
    def add(self, vectors, labels=None):
        """Appends rows to the finalized index without a rebuild; returns their ids as int64, arange(size before, size
        after): the same numbers in internal ids and in input rows.  `labels`: one int per row, required exactly when
        the index has a label column.  The rows form a tail behind the graph: every exact path sees them as more
        candidates, a graph-routed search scans them exactly and folds them into the graph's rows (ascending distance,
        the graph's entry first where two are equal), so they are always found and a search slows down as the tail
        grows -- compact() folds the tail into a new graph.  Filters made before the call no longer fit (size changed).
        While tail_size > 0: save, save_native and set_row_map raise (compact() first), graph-routed searches take
        k <= 1024, and per-query filters serve scanned queries only (NotImplementedError otherwise).  Waits for the
        batches in flight.  Not available on devices=[...] indexes, their replicas or parts.
        metric="cosine": the rows are normalised like those of build(); a row without a direction (zero, NaN, Inf)
        raises ValueError naming it and adds nothing."""
        if self._m is not None or self._p is not None or self._owner is not None:
            raise NotImplementedError("add is not available on a multi-device or partitioned index, its replicas or parts")
        v = _as_f32(vectors)
        if v.ndim != 2 or v.shape[1] != self._dim:
            raise ValueError("vectors must be a (m, dim) float32 array")
        lab = None
        if labels is not None:
            lab = self._as_labels(labels, "labels")
            if lab.ndim != 1 or lab.shape[0] != v.shape[0]:
                raise ValueError(f"labels must hold one entry per added row ({v.shape[0]})")
        first = C.c_int64(0)
        _lib.check(_lib.lib().cph_add(self._h, v.ctypes.data if v.size else None, v.shape[0],
                                      lab.ctypes.data if lab is not None and lab.size else None, C.byref(first)))
        return np.arange(first.value, first.value + v.shape[0], dtype=np.int64)

    @property
    def tail_size(self):
        """Rows added since the index was built, loaded or compacted (size counts them)."""
        if self._m is not None or self._p is not None:
            return 0
        t = C.c_uint64(0)
        _lib.check(_lib.lib().cph_tail_count(self._h, C.byref(t)))
        return t.value

    # -- persistence ------------------------------------------------------------------------
    def save(self, path):
        """Reference-format (v2) file.  metric="cosine": refused (ValueError) -- the format cannot carry the metric and a
        reader would search the rows as squared-L2 data; use save_native."""
        if self._p is not None:
            raise RuntimeError("a partitioned index has no reference-format file (that format holds one graph and no row "
                               "map): use save_native")
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_save(self._m, str(path).encode()))
            return
        _lib.check(_lib.lib().cph_save(self._h, str(path).encode()))

    def load(self, path):
        """Reference-format (v2) file: it holds no row map, so the index comes back with result_ids "internal".
        metric="cosine": refused (ValueError) -- nobody normalised the file's rows; use load_native."""
        if self._p is not None:
            raise RuntimeError("a partitioned index cannot load a reference-format file (that format holds one graph and "
                               "no row map): use load_native")
        try:
            if self._m is not None:
                _lib.check(_lib.lib().cph_multi_load(self._m, str(path).encode()))
                return
            _lib.check(_lib.lib().cph_load(self._h, str(path).encode()))
        finally:
            self._after_index_change()

    def calib_samples_debug(self, queries, start):
        """Construction hook: the calibration sampler on given queries / start vertices: (rec [ns, 32, 6], cnt, dqp)."""
        self._no_parts("calib_samples_debug")
        q = _as_f32(queries)
        st = np.ascontiguousarray(start, np.uint32)
        ns = q.shape[0]
        rec = np.zeros((ns, 32, 6), np.float32)
        cnt = np.zeros(ns, np.uint32)
        dqp = np.zeros(ns, np.float32)
        _lib.check(_lib.lib().cph_calib_hook(self._h, q.ctypes.data, st.ctypes.data, ns, rec.ctypes.data, cnt.ctypes.data,
                                             dqp.ctypes.data))
        return rec, cnt, dqp

    def save_native(self, path):
        """GPU-native file (device block layout; not readable by the reference): fast to load."""
        if self._p is not None:       # one file per part: path.p<i>of<P>
            _lib.check(_lib.lib().cph_parts_save_native(self._p, str(path).encode()))
            return
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_save_native(self._m, str(path).encode()))
            return
        _lib.check(_lib.lib().cph_save_native(self._h, str(path).encode()))

    def load_native(self, path):
        if self._p is not None:       # the files of save_native on a handle with as many parts; ValueError leaves it untouched
            _lib.check(_lib.lib().cph_parts_load_native(self._p, str(path).encode()))
            return
        try:
            if self._m is not None:
                _lib.check(_lib.lib().cph_multi_load_native(self._m, str(path).encode()))
                return
            _lib.check(_lib.lib().cph_load_native(self._h, str(path).encode()))
        finally:
            self._after_index_change()

    # -- ids in input rows (not in the reference) ------------------------------------------------
    def _after_index_change(self):
        # the handle returns internal ids again once it has lost its row map
        if self._result_ids == "input" and not self.has_row_map:
            self.result_ids = "internal"

    @property
    def has_row_map(self):
        """The index knows the input row of every internal id: it was built here, loaded from a native file saved
        from such an index, or given a map with set_row_map.  A reference-format file (save / load) cannot carry it."""
        f = C.c_int(0)
        if self._p is not None:
            return self.is_finalized        # (every part of a partitioned index keeps its row map)
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_has_row_map(self._m, C.byref(f)))
        else:
            _lib.check(_lib.lib().cph_has_row_map(self._h, C.byref(f)))
        return bool(f.value)

    def row_map(self):
        """int64[size] copy: row_map()[i] = row, in the array given to build(), of internal id i (a permutation; exact
        also where rows repeat, which internal_to_input_rows is not)."""
        self._no_parts("row_map")
        out = np.empty(self.size, np.uint32)
        _lib.check(_lib.lib().cph_get_row_map(self._h, 0, out.size, out.ctypes.data))
        return out.astype(np.int64)

    def set_row_map(self, rows):
        """Gives an index that has none (loaded from a reference-format file) its row map: a permutation of 0..size-1,
        else ValueError.  None removes the map and puts result_ids back to "internal"."""
        self._no_parts("set_row_map")
        if rows is None:
            if self._m is not None:
                _lib.check(_lib.lib().cph_multi_set_row_map(self._m, None, 0))
            else:
                _lib.check(_lib.lib().cph_set_row_map(self._h, None, 0))
            self._result_ids = "internal"
            return
        r = np.asarray(rows)
        if r.ndim != 1 or not np.issubdtype(r.dtype, np.integer):
            raise ValueError("row map must be a 1D integer array")
        if r.size and (r.min() < 0 or r.max() > 0xFFFFFFFF):
            raise ValueError("row map must be a permutation of 0..size-1")
        r = np.ascontiguousarray(r, np.uint32)
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_set_row_map(self._m, r.ctypes.data, r.size))
        else:
            _lib.check(_lib.lib().cph_set_row_map(self._h, r.ctypes.data, r.size))

    @property
    def result_ids(self):
        """"internal" (default: the reference's post-reorder ids) or "input": every search returns rows of the array
        given to build(), translated on the GPU where the results are written (padding stays -1; distances are the
        same bytes).  Also the default id space of make_filter and of the `filter=` arguments.  get_vectors, exact_l2,
        fastscan_block and entry_point stay in internal ids."""
        return self._result_ids

    @result_ids.setter
    def result_ids(self, space):
        if space not in ("internal", "input"):
            raise ValueError('result_ids must be "internal" or "input"')
        if self._p is not None:
            if space != "input":
                raise ValueError('a partitioned index speaks input rows only: result_ids stays "input" '
                                 "(every part has its own internal ids: part(i))")
            return
        code = _lib.IDS_INPUT if space == "input" else _lib.IDS_INTERNAL
        if self._m is not None:
            _lib.check(_lib.lib().cph_multi_set_result_ids(self._m, code))
        else:
            _lib.check(_lib.lib().cph_set_result_ids(self._h, code))
        self._result_ids = space

    @property
    def exact_threshold(self):
        """Cut-over of the filtered searches (search / search_batch / search_batch_device with `filter=`): a filter that
        allows at most this many ids is scanned exactly (as with exact=True) instead of walking the graph.  Default 0:
        never.  profiles/exact_scan.md: at 1M x 128, 10,000 queries, k = 10 the two paths meet at about 3,900 allowed ids."""
        return self._exact_threshold

    @exact_threshold.setter
    def exact_threshold(self, max_allowed):
        v = int(max_allowed)
        if v < 0:
            raise ValueError("exact_threshold must be >= 0")
        if self._p is not None:       # compared with every PART's allowed count
            _lib.check(_lib.lib().cph_parts_set_exact_threshold(self._p, v))
        elif self._m is not None:
            _lib.check(_lib.lib().cph_multi_set_exact_threshold(self._m, v))
        else:
            _lib.check(_lib.lib().cph_set_exact_threshold(self._h, v))
        self._exact_threshold = v

    # -- properties -------------------------------------------------------------------------
    @property
    def size(self):
        n = C.c_uint64(0)
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_size(self._p, C.byref(n)))
        elif self._m is not None:
            _lib.check(_lib.lib().cph_multi_size(self._m, C.byref(n)))
        else:
            _lib.check(_lib.lib().cph_size(self._h, C.byref(n)))
        return n.value

    @property
    def dim(self):
        return self._dim

    @property
    def is_finalized(self):
        f = C.c_int(0)
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_is_finalized(self._p, C.byref(f)))
        elif self._m is not None:
            _lib.check(_lib.lib().cph_multi_is_finalized(self._m, C.byref(f)))
        else:
            _lib.check(_lib.lib().cph_is_finalized(self._h, C.byref(f)))
        return bool(f.value)

    # -- extras (not in the reference) ------------------------------------------------------
    def set_batch_sets(self, n_sets):
        """Batch scratch sets in rotation (1..4, default 2): batches that can be in flight together on different streams.
        A multi-device index sets every replica."""
        for h in self._replicas():
            _lib.check(_lib.lib().cph_set_batch_sets(h, int(n_sets)))

    def set_search_params(self, slots=0, beam_capacity=0):
        for h in self._replicas():
            _lib.check(_lib.lib().cph_set_search_params(h, int(slots), int(beam_capacity)))

    def last_search_stats(self):
        """Work counters of the last batch; a multi-device index' last search_batch: summed over the replicas that
        took part, kernel_us and capacity their maximum.  A partitioned index: summed over the parts, kernel_us and
        capacity their maximum, plus merge_us, the device time of the merge kernel."""
        out = (C.c_uint64 * 13)()
        if self._p is not None:
            _lib.check(_lib.lib().cph_parts_last_search_stats(self._p, out))
        elif self._m is not None:
            _lib.check(_lib.lib().cph_multi_last_search_stats(self._m, out))
        else:
            _lib.check(_lib.lib().cph_last_search_stats(self._h, out))
        keys = ("expansions", "exact_l2", "new_neighbours", "beam_pushes", "stage2_skipped",
                "rerun_queries", "kernel_us", "expansions_nothing_new", "slots", "capacity",
                "stage2_reruns", "stage2_undecided") + (("merge_us",) if self._p is not None else ())
        return dict(zip(keys, [int(x) for x in out]))

    def synchronize(self):
        """Waits for every batch enqueued with search_batch_device."""
        for h in self._replicas():
            _lib.check(_lib.lib().cph_synchronize(h))

    def last_query_expansions(self, n):
        """Vertices expanded by each of the n queries of the last batch."""
        out = np.empty(int(n), np.uint32)
        if self._p is not None:       # summed over the parts
            _lib.check(_lib.lib().cph_parts_last_query_expansions(self._p, out.ctypes.data, int(n)))
        elif self._m is not None:
            _lib.check(_lib.lib().cph_multi_last_query_expansions(self._m, out.ctypes.data, int(n)))
        else:
            _lib.check(_lib.lib().cph_last_query_expansions(self._h, out.ctypes.data, int(n)))
        return out

    def order_queries(self, keys):
        """Launch order the search would use for these (non-negative) scheduling keys."""
        self._no_parts("order_queries")
        keys = np.ascontiguousarray(keys, np.float32)
        out = np.empty(len(keys), np.uint32)
        _lib.check(_lib.lib().cph_order_queries(self._h, keys.ctypes.data, len(keys), out.ctypes.data))
        return out

    def get_vectors(self, first=0, count=None, stored=False):
        """Stored vectors of internal ids [first, first+count) as float32 (count, dim) (internal ids also when
        result_ids is "input").  metric="cosine": the rows as stored, x / (sqrt(2) |x|), not the rows given to build().
        metric="ip": the first dim columns of the stored rows, which are the rows given to build() bit for bit;
        stored=True returns all dim + 1 columns, the last one sqrt(M2 - |x|^2)."""
        self._no_parts("get_vectors")
        if count is None:
            count = self.size - first
        out = np.empty((count, self._sdim), np.float32)
        _lib.check(_lib.lib().cph_get_vectors(self._h, int(first), int(count), out.ctypes.data))
        return out if stored or self._sdim == self._dim else np.ascontiguousarray(out[:, :self._dim])

    def internal_to_input_rows(self, base, chunk=1 << 18):
        """int64[size]: input row number of every internal id, by exact row matching.
        Rows that occur several times in `base` map to one of their equal copies.  (For an index without a row map;
        with one, row_map() is exact and needs neither `base` nor the download.)"""
        base = _as_f32(base)
        key = {}
        for i in range(base.shape[0] - 1, -1, -1):
            key[base[i].tobytes()] = i
        out = np.empty(self.size, np.int64)
        for lo in range(0, self.size, chunk):
            v = self.get_vectors(lo, min(chunk, self.size - lo))
            for j in range(v.shape[0]):
                out[lo + j] = key[v[j].tobytes()]
        return out

    # kernel-level hooks (parity tests)
    def encode_query(self, query):
        self._no_parts("encode_query")
        q = _as_f32(query)
        D = 1
        while D < self._sdim:
            D *= 2
        lut = np.zeros((D // 4, 16), np.uint8)
        co = np.zeros(3, np.float32)
        _lib.check(_lib.lib().cph_encode_query(self._h, q.ctypes.data, lut.ctypes.data, co.ctypes.data))
        return lut, co

    def entry_point(self, query):
        self._no_parts("entry_point")
        q = _as_f32(query)
        ep = C.c_uint32(0)
        _lib.check(_lib.lib().cph_entry_point(self._h, q.ctypes.data, C.byref(ep)))
        return ep.value

    def fastscan_block(self, lut, qparams, vertex, dist_qp_sq, worst=3.402823466e+38, nn_full=False):
        self._no_parts("fastscan_block")
        lut = np.ascontiguousarray(lut, np.uint8)
        qp = np.ascontiguousarray(qparams, np.float32)
        sums = np.zeros(32, np.uint32)
        msb = np.zeros(32, np.uint32)
        est = np.zeros(32, np.float32)
        lower = np.zeros(32, np.float32)
        lower1 = np.zeros(32, np.float32)
        _lib.check(_lib.lib().cph_fastscan_block(
            self._h, lut.ctypes.data, qp.ctypes.data, int(vertex), float(dist_qp_sq), float(worst),
            int(bool(nn_full)), sums.ctypes.data, msb.ctypes.data, est.ctypes.data, lower.ctypes.data,
            lower1.ctypes.data))
        return sums, msb, est, lower, lower1

    def exact_l2(self, query, ids):
        self._no_parts("exact_l2")
        q = _as_f32(query)
        ids = np.ascontiguousarray(ids, np.uint32)
        out = np.zeros(len(ids), np.float32)
        _lib.check(_lib.lib().cph_exact_l2(self._h, q.ctypes.data, ids.ctypes.data, len(ids),
                                           out.ctypes.data))
        return out


def knn_bruteforce(vectors, queries=None, device=None):
    """Exact 32 nearest neighbours on the GPU's matrix cores: ids uint32, squared distances float32.
    queries=None: every row of `vectors` against the others (self excluded), shape [n, 32];
    else `queries` against `vectors`, shape [nq, 32]."""
    v = _as_f32(vectors)
    n, dim = v.shape
    q = None if queries is None else _as_f32(queries)
    if q is not None and (q.ndim != 2 or q.shape[1] != dim):
        raise ValueError("queries must be a (nq, dim) array")
    rows = n if q is None else q.shape[0]
    ids = np.zeros((rows, 32), np.uint32)
    dist = np.zeros((rows, 32), np.float32)
    dev = _default_device() if device is None else int(device)
    _lib.check(_lib.lib().cph_knn_bruteforce(dev, v.ctypes.data, n, dim, None if q is None else q.ctypes.data,
                                             0 if q is None else q.shape[0], ids.ctypes.data, dist.ctypes.data))
    return ids, dist


def knn_debug(vectors, queries=None, q_ids=None, path=0, blocks_per_launch=0, device=None):
    """Test hook of the exact-kNN kernels: knn_bruteforce with the choices the production path makes from the size laid open.
    queries=None: the self-join; q_ids (with queries): row i never lists column q_ids[i]; path 0 = the two-pass kernel,
    1 = the symmetric join (self-join, 1024 <= n <= 4096, padded D >= 64); blocks_per_launch 0 = the production slicing, else
    128-row blocks per launch (two-pass) and workgroups per launch (join).  Returns (ids u32[rows, 32], dist f32[rows, 32],
    fallback rows of the join, launches made of the kernel `path` names)."""
    v = _as_f32(vectors)
    n, dim = v.shape
    q = None if queries is None else _as_f32(queries)
    if q is not None and (q.ndim != 2 or q.shape[1] != dim):
        raise ValueError("queries must be a (nq, dim) array")
    qi = None if q_ids is None else np.ascontiguousarray(q_ids, np.uint32)
    if qi is not None and (q is None or qi.shape != (q.shape[0],)):
        raise ValueError("q_ids must be a (nq,) array and goes with queries")
    rows = n if q is None else q.shape[0]
    ids = np.zeros((rows, 32), np.uint32)
    dist = np.zeros((rows, 32), np.float32)
    redo, made = C.c_uint32(0), C.c_uint32(0)
    dev = _default_device() if device is None else int(device)
    _lib.check(_lib.lib().cph_debug_knn(dev, v.ctypes.data, n, dim, None if q is None else q.ctypes.data, 0 if q is None else q.shape[0],
                                        None if qi is None else qi.ctypes.data, 0 if qi is None else 1, int(path), int(blocks_per_launch),
                                        ids.ctypes.data, dist.ctypes.data, C.byref(redo), C.byref(made)))
    return ids, dist, int(redo.value), int(made.value)


def encode_edges(parent, nbrs, bits, device=None):
    """GPU data-side encoder of one vertex' edges (construction hook): (values u8[cnt, D], aux f32[cnt, 3] =
    nop, ip_qo, ip_cp, pops u32[cnt, 2] = msb popcount, weighted popcount)."""
    p = _as_f32(parent)
    nb = _as_f32(nbrs)
    cnt, dim = nb.shape
    D = 16
    while D < dim:
        D *= 2
    vals = np.zeros((cnt, D), np.uint8)
    aux = np.zeros((cnt, 3), np.float32)
    pops = np.zeros((cnt, 2), np.uint32)
    dev = _default_device() if device is None else int(device)
    _lib.check(_lib.lib().cph_encode_edges(dev, dim, int(bits), p.ctypes.data, nb.ctypes.data, cnt, vals.ctypes.data,
                                           aux.ctypes.data, pops.ctypes.data))
    return vals, aux, pops


def select_neighbors_debug(x, vertex, fwd, rev, R, alpha, tau, alpha_max=0.0, err=None, device=None):
    """Construction hook: the GPU selection kernel on one vertex (x = [n, D] padded vectors, fwd = 32 candidate ids with
    0xFFFFFFFF for none, rev = up to 65,536 more: the reverse edges).  Beyond 96 reverse edges the vertex is a hub and the
    kernel keeps the nearest 64 unique candidates of both lists, whatever the order of rev.  Returns the selected ids."""
    x = _as_f32(x)
    n, D = x.shape
    fwd = np.ascontiguousarray(fwd, np.uint32)
    rev = np.ascontiguousarray(rev, np.uint32)
    assert fwd.shape == (32,)
    out = np.zeros(32, np.uint32)
    cnt = np.zeros(1, np.uint32)
    e = None if err is None else _as_f32(err)
    dev = _default_device() if device is None else int(device)
    _lib.check(_lib.lib().cph_select_hook(dev, x.ctypes.data, n, D, int(vertex), fwd.ctypes.data, rev.ctypes.data if len(rev) else None,
                                          len(rev), int(R), float(alpha), float(tau), float(alpha_max),
                                          None if e is None else e.ctypes.data, out.ctypes.data, cnt.ctypes.data))
    return out[:cnt[0]].copy()


def select_layer_debug(x, knn, R, alpha, tau, alpha_max=0.0, err=None, grid_cap=0, device=None):
    """Construction hook: layer-0 selection of a whole table as finalize() launches it (x = [n, D] padded vectors, knn =
    [n, 32] ids with 0xFFFFFFFF for none): the reverse CSR built from the table, then the selection kernel over all rows,
    on the production grid or on at most grid_cap workgroups.  Returns (ids u32[n, 32] padded with 0xFFFFFFFF, counts
    u32[n], rev_off u64[n + 1], rev u32[rev_off[n]]): the selected lists and the reverse CSR the kernel read."""
    x = _as_f32(x)
    n, D = x.shape
    knn = np.ascontiguousarray(knn, np.uint32)
    if knn.shape != (n, 32):
        raise ValueError("knn must be a (n, 32) array")
    ids = np.zeros((n, 32), np.uint32)
    cnt = np.zeros(n, np.uint32)
    off = np.zeros(n + 1, np.uint64)
    rev = np.zeros(n * 32, np.uint32)
    e = None if err is None else _as_f32(err)
    dev = _default_device() if device is None else int(device)
    _lib.check(_lib.lib().cph_select_layer_hook(dev, x.ctypes.data, n, D, knn.ctypes.data, int(R), float(alpha), float(tau),
                                                float(alpha_max), None if e is None else e.ctypes.data, int(grid_cap),
                                                ids.ctypes.data, cnt.ctypes.data, off.ctypes.data, rev.ctypes.data))
    return ids, cnt, off, rev[:int(off[n])].copy()


def heap_ops_debug(ops, keys, ids, device=None):
    """Self-test hook: runs a push (1) / pop (0) / pop-then-push (2: the way one expansion does it, with the leaf's
    ancestors fetched ahead of the pop) sequence through the beam's wave-parallel heap routines (first 255 entries in
    LDS, the rest in HBM) and returns the heap array (keys f32, ids u32)."""
    ops = np.ascontiguousarray(ops, np.uint8)
    keys = np.ascontiguousarray(keys, np.float32)
    ids = np.ascontiguousarray(ids, np.uint32)
    n_push = int((ops != 0).sum())
    assert len(keys) == n_push and len(ids) == n_push
    ok = np.zeros(max(1, n_push), np.float32)
    oi = np.zeros(max(1, n_push), np.uint32)
    sz = np.zeros(1, np.uint32)
    dev = _default_device() if device is None else int(device)
    _lib.check(_lib.lib().cph_debug_heap_ops(dev, ops.ctypes.data, len(ops), keys.ctypes.data, ids.ctypes.data, n_push,
                                             ok.ctypes.data, oi.ctypes.data, sz.ctypes.data))
    return ok[:sz[0]].copy(), oi[:sz[0]].copy()


def _default_device():
    """One process per GPU: LOCAL_RANK selects the device when launched by torch.distributed.run."""
    import os
    try:
        return int(os.environ.get("LOCAL_RANK", "0"))
    except ValueError:
        return 0


class FastScanStream:
    """Synthetic-block streaming FastScan benchmark (cph_fastscan_stream_*)."""

    def __init__(self, D, bits, n_blocks, seed=4, device=None):
        self._h = C.c_void_p()
        bb = C.c_uint64(0)
        self.D, self.bits, self.n_blocks = int(D), int(bits), int(n_blocks)
        dev = _default_device() if device is None else int(device)
        _lib.check(_lib.lib().cph_fastscan_stream_create(dev, self.D, self.bits, self.n_blocks, int(seed),
                                                         C.byref(self._h), C.byref(bb)))
        self.block_bytes = bb.value

    def run(self, reps=1):
        ms = C.c_double(0)
        ck = C.c_double(0)
        _lib.check(_lib.lib().cph_fastscan_stream_run(self._h, int(reps), C.byref(ms), C.byref(ck)))
        return ms.value, ck.value

    def export(self, first, count, ref_block_bytes):
        blocks = np.zeros(count * ref_block_bytes, np.uint8)
        lut = np.zeros((self.D // 4, 16), np.uint8)
        qp = np.zeros(7, np.float32)
        dqp = C.c_float(0)
        _lib.check(_lib.lib().cph_fastscan_stream_export(self._h, int(first), int(count), blocks.ctypes.data,
                                                         lut.ctypes.data, qp.ctypes.data, C.byref(dqp)))
        return blocks, lut, qp, dqp.value

    def eval(self, first, count):
        est = np.zeros((count, 32), np.float32)
        lower = np.zeros((count, 32), np.float32)
        _lib.check(_lib.lib().cph_fastscan_stream_eval(self._h, int(first), int(count), est.ctypes.data,
                                                       lower.ctypes.data))
        return est, lower

    def close(self):
        if self._h.value:
            _lib.lib().cph_fastscan_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
