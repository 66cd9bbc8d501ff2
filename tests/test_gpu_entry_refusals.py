"""What the batch entry points refuse, and that a refusal writes nothing, on every handle kind: one index, two replicas
(devices=[0, 0], min_shard 1: 9 queries make two uneven shards) and two parts -- through the C entries themselves, host
and device form (replicas have a host form only: their device form is a replica's own entry).  Every output row starts
as sentinels (-7 / -7.0); after a refused call every sentinel must still be there.

The single index and the replicas load the smallest golden index (g16, 1-bit, 300 rows); the partitioned index is built
from the vectors of test_gpu_partitioned.py's two40 (4,000 x 40, 1-bit, seed 12).  9 queries, k = 3."""
import ctypes as C

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

N, K = 9, 3
FILTER_OF = np.array([0, 1, -1, 1, 0, -1, -1, 0, 1], np.int32)     # (both shards of 5 + 4 hold -1, 0 and 1)

ENTRIES = {
    # (kind, where): the single-filter, exact and per-query entry
    ("single", "host"): ("cph_search_batch_filtered", "cph_search_batch_exact", "cph_search_batch_filters"),
    ("single", "device"): ("cph_search_batch_device_filtered", "cph_search_batch_exact_device", "cph_search_batch_filters_device"),
    ("multi", "host"): ("cph_multi_search_batch_filtered", "cph_multi_search_batch_exact", "cph_multi_search_batch_filters"),
    ("parts", "host"): ("cph_parts_search_batch_filtered", "cph_parts_search_batch_exact", "cph_parts_search_batch_filters"),
    ("parts", "device"): ("cph_parts_search_batch_device_filtered", "cph_parts_search_batch_exact_device",
                          "cph_parts_search_batch_filters_device"),
}


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


class Kind:
    """One handle kind: the index, its C handle, 9 queries, two filters and a filter made for an index of another size.
    one(f): the filter argument of the single-filter entries; many(fs): that of the per-query entries (None: a null
    entry, in the last place)."""

    def __init__(self, ix, handle, Q, alien_ix):
        n = ix.size
        self.ix, self.handle, self.alien_ix = ix, handle, alien_ix
        self.Q = np.ascontiguousarray(Q[:N], np.float32)
        self.fs = [ix.make_filter(np.arange(0, n, 2)), ix.make_filter(np.arange(5, 25))]
        self.alien = alien_ix.make_filter(np.arange(0, alien_ix.size, 3))
        assert alien_ix.size != n

    def one(self, f):
        if self.ix.partitioned:
            return f._pf
        return (C.c_void_p * len(f._hs))(*[h.value for h in f._hs]) if len(f._hs) > 1 else f._h

    def many(self, fs):
        if self.ix.partitioned:
            hs = [None if f is None else f._pf.value for f in fs]
        else:
            hs = []
            for f in fs:            # (replicas: the layout is [filter][replica], and the null entry is the last replica's)
                hs += [h.value for h in f._hs] if f is not None else [h.value for h in self.fs[0]._hs[:-1]] + [None]
        return (C.c_void_p * len(hs))(*hs)


@pytest.fixture(scope="module")
def kinds(cph, gold):
    dim = DATASETS["g16"]["dim"]
    single = cph.CPIndex(dim, 1, device=0)
    single.load(fixture_path("g16", 1))
    multi = cph.CPIndex(dim, 1, devices=[0, 0])
    multi.set_min_shard(1)
    multi.load(fixture_path("g16", 1))
    other = cph.CPIndex(DATASETS["g128"]["dim"], 1, devices=[0, 0])      # 400 rows: its filters fit neither of the two
    other.load(fixture_path("g128", 1))
    rng = np.random.default_rng(12)
    X = rng.standard_normal((4000, 40)).astype(np.float32)
    PQ = rng.standard_normal((200, 40)).astype(np.float32)
    parts = cph.CPIndex(40, 1, devices=[0, 0], partition=True)
    parts.build(X)
    parts.finalize()
    small = cph.CPIndex(40, 1, devices=[0, 0], partition=True)           # another size, the same number of parts
    small.build(X[:130])
    small.finalize()
    Q = gold["Q/g16"]
    out = {"single": Kind(single, single._h, Q, other), "multi": Kind(multi, multi._m, Q, other),
           "parts": Kind(parts, parts._p, PQ, small)}
    out["single"].alien_h = out["single"].alien._hs[0]                    # (replica 0's filter: an ordinary cph_filter)
    return out


def _call(kd, kind, where, form, k, fargs):
    """One call of the C entry `form` (0: single filter, 1: exact, 2: per-query) into rows of sentinels -> (the exception
    or None, ids, dist)."""
    from cphnsw_mi355x import _lib
    fn = getattr(_lib.lib(), ENTRIES[kind, where][form])
    err = None
    if where == "host":
        ids = np.full((N, k), -7, np.int64)
        dist = np.full((N, k), -7.0, np.float32)
        try:
            _lib.check(fn(kd.handle, kd.Q.ctypes.data, N, k, *fargs, ids.ctypes.data, dist.ctypes.data))
        except Exception as e:      # noqa: BLE001 (the caller asserts its type)
            err = e
        return err, ids, dist
    import torch
    q = torch.from_numpy(kd.Q).cuda()
    ids = torch.full((N, k), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((N, k), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    try:
        _lib.check(fn(kd.handle, q.data_ptr(), N, k, *fargs, ids.data_ptr(), dist.data_ptr(),
                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    except Exception as e:          # noqa: BLE001
        err = e
    torch.cuda.synchronize()
    return err, ids.cpu().numpy(), dist.cpu().numpy()


def _refusals(kd, kind):
    """name -> (form, k, the filter arguments, what the message must match or None)."""
    bad_of = FILTER_OF.copy()
    bad_of[-1] = 2
    alien = kd.alien_h if kind == "single" else kd.one(kd.alien)
    return {
        "filter_of_last_is_F": (2, K, (kd.many(kd.fs), 2, bad_of.ctypes.data, 0), r"outside \[-1, 2\)", bad_of),
        "null_filter_in_list": (2, K, (kd.many([kd.fs[0], None]), 2, FILTER_OF.ctypes.data, 0), None, None),
        "exact_k_1025": (1, 1025, (None,), r"exact search supports k <= 1024", None),
        "exact_k_1025_per_query": (2, 1025, (kd.many(kd.fs), 2, FILTER_OF.ctypes.data, 1), r"exact search supports k <= 1024", None),
        "filter_of_another_size": (0, K, (alien,), r"filter covers \d+ (ids|rows), the index holds \d+", None),
    }


CASES = ["filter_of_last_is_F", "null_filter_in_list", "exact_k_1025", "exact_k_1025_per_query", "filter_of_another_size"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind,where", list(ENTRIES))
def test_refusal_writes_nothing(kinds, kind, where, case):
    kd = kinds[kind]
    form, k, fargs, match, _keep = _refusals(kd, kind)[case]
    err, ids, dist = _call(kd, kind, where, form, k, fargs)
    assert isinstance(err, ValueError), (kind, where, case, err)
    if match:
        import re
        assert re.search(match, str(err)), (kind, where, case, str(err))
    assert (ids == -7).all() and (dist == -7.0).all(), (kind, where, case)


@pytest.mark.parametrize("kind", ["single", "multi", "parts"])
def test_per_query_filters_host_and_device_entries_agree(kinds, kind):
    """filter_of mixing -1, 0 and 1: the host entry (replicas: two shards) and the device entry (replicas: replica 0's own)
    return the same bytes, and every row was written."""
    kd = kinds[kind]
    fargs = (kd.many(kd.fs), 2, FILTER_OF.ctypes.data, 0)
    err, hi, hd = _call(kd, kind, "host", 2, K, fargs)
    assert err is None, err
    dev = kd
    if kind == "multi":                          # replica 0 as an ordinary handle, with replica 0's filters
        dev = Kind.__new__(Kind)
        dev.handle, dev.Q = kd.ix._reps[0], kd.Q
        fargs = ((C.c_void_p * 2)(*[f._hs[0].value for f in kd.fs]),) + fargs[1:]
    err, di, dd = _call(dev, "single" if kind == "multi" else kind, "device", 2, K, fargs)
    assert err is None, err
    assert not (hi == -7).any() and not (hd == -7.0).any()
    assert hi.tobytes() == di.tobytes() and hd.tobytes() == dd.tobytes(), kind
    assert (hi[FILTER_OF == 1] >= 5).all() and (hi[FILTER_OF == 1] < 25).all()      # (20 allowed ids, k = 3: no padding)
    assert (hi[FILTER_OF == 0] % 2 == 0).all()
