"""CPU tier of the facet counts (cph_facet_values, cph_facet_counts, cph_facet_top): the host statements of the device passes.

tests/facet_host/facet_host.cpp includes csrc/host_index.h and is built with plain g++ and -fsanitize=address,undefined,
the way tests/test_tags_host.py builds its driver (a stand-alone program; nothing loaded into Python runs under a
sanitizer).  `eval` runs facet_dictionary_host, facet_counts_host and facet_top_host on data written by this test, every
bitmap in an exact-size buffer, and every value, code, count and top entry is compared with the numpy model
(tests/facet_model.py); `self` compares them with a bit-by-bit loop; `refuse` must refuse.  cph_host_facet_counts and
cph_host_facet_top (the library's host-only entries, no HIP call) are compared with the model on the same cases.
Everything is integers: every comparison is exact equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import facet_model as fm
import tags_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "facet_host", "facet_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]

SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4100]
FILTER_COUNTS = [1, 3, 70]
VOCAB16 = np.array([fm.I32_MIN, -1, 0, fm.I32_MAX] + list(range(3, 15)), np.int64)
COLUMN_KINDS = ["one_value", "all_distinct", "vocab16", "tags"]
TOP_K = 5


def _column(n, kind):
    """(column, lims or None).  "tags": a CSR as a caller gives it (unsorted, duplicates), a third of the rows empty, and
    (n permitting) the first and the last row with exactly 1,024 distinct tags."""
    rng = np.random.default_rng(9000 + n)
    if kind == "one_value":
        return np.full(n, -7, np.int64), None
    if kind == "all_distinct":
        return rng.permutation(n).astype(np.int64) * 3 - 100, None
    if kind == "vocab16":
        return VOCAB16[rng.integers(0, 16, n)], None
    rows = []
    for i in range(n):
        if rng.random() < 0.33:
            rows.append(np.zeros(0, np.int64))
            continue
        r = VOCAB16[rng.integers(0, 16, rng.integers(1, 10))]
        rows.append(np.concatenate([r, r[:rng.integers(0, 3)]]))
    if n:
        long_row = np.concatenate([np.arange(20000, 21024), [20000, 20500, 21023]])      # 1,024 distinct, 1,027 given
        rows[0] = rng.permutation(long_row)
        rows[-1] = rng.permutation(long_row + 1)
    lims, tags = tm.to_csr(rows)
    return np.asarray(tags, np.int64), np.asarray(lims, np.int64)


def _filters(n, m, seed):
    """m entries: None ("every row", no bitmap) or uint32 words [(n + 31) / 32] whose bits behind n may be dirty.  Kinds in
    rotation: none, all ones, empty, single bits on word borders, random, random with dirty bits behind n."""
    rng = np.random.default_rng(seed)
    nw = (n + 31) // 32
    out = []
    for j in range(m):
        kind = (j + seed) % 6
        if kind == 0:
            out.append(None)
            continue
        mask = np.zeros(nw * 32, bool)
        if kind == 1:
            mask[:] = True                                   # all ones, the bits behind n too
        elif kind == 3:
            for b in (0, 31, 32, 63, 64, n - 1):
                if 0 <= b < n:
                    mask[b] = True
        elif kind >= 4:
            mask[:n] = rng.random(n) < 0.4
            if kind == 5:
                mask[n:] = True                              # dirty bits behind n in the last word
        out.append(fm.pack(mask) if nw else np.zeros(0, np.uint32))
    return out


def _case(n, m, kind):
    column, lims = _column(n, kind)
    filters = _filters(n, m, n + m)
    removed = np.random.default_rng(n + 3).random(n) < 0.2 if n % 2 else None
    return column, lims, filters, removed


def _expect(column, lims, filters, removed, n):
    if lims is not None:
        lims, column = tm.canonical(lims, column)
    masks = [None if f is None else fm.unpack(f, n) for f in filters]
    values, counts = fm.counts(column, masks, removed, lims)
    return values, fm.dictionary(column)[1], counts


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("facet_host")), "facet_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(cmd, timeout=600):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    return r


def test_model_by_hand():
    fm.check_by_hand()


def test_facet_statements_against_a_loop_under_asan_ubsan(asan_exe):
    assert "self: ok" in _run([asan_exe, "self"]).stdout


def test_facet_statements_refuse_under_asan_ubsan(asan_exe):
    out = _run([asan_exe, "refuse"]).stdout
    assert "refuse: ok" in out and out.count("refused:") == 5


@pytest.mark.parametrize("kind", COLUMN_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_facet_statements_against_the_model_under_asan_ubsan(asan_exe, tmp_path, n, kind):
    for m in FILTER_COUNTS:
        column, lims, filters, removed = _case(n, m, kind)
        nw = (n + 31) // 32
        fin, fout = str(tmp_path / f"in{m}.bin"), str(tmp_path / f"out{m}.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, m, len(column), lims is not None, removed is not None, TOP_K], np.uint64).tobytes())
            if lims is not None:
                f.write(lims.astype(np.uint64).tobytes())
            f.write(column.astype(np.int32).tobytes())
            f.write(np.array([w is not None for w in filters], np.uint8).tobytes())
            for w in filters:
                f.write((np.zeros(nw, np.uint32) if w is None else w).tobytes())
            if removed is not None:
                f.write(fm.pack(removed).tobytes())
        assert "eval: ok" in _run([asan_exe, "eval", fin, fout]).stdout
        values, codes, counts = _expect(column, lims, filters, removed, n)
        U, E = len(values), len(codes)
        raw = open(fout, "rb").read()
        assert np.frombuffer(raw, np.uint64, 2).tolist() == [U, E]
        assert len(raw) == 16 + U * 4 + E * 4 + m * U * 8 + m * TOP_K * 12 + m * 4
        at = 16
        assert np.array_equal(np.frombuffer(raw, np.int32, U, at), values)
        at += U * 4
        assert np.array_equal(np.frombuffer(raw, np.uint32, E, at), codes)
        at += E * 4
        assert np.array_equal(np.frombuffer(raw, np.uint64, m * U, at).reshape(m, U).astype(np.int64), counts)
        at += m * U * 8
        tv, tc, found = fm.top(values, counts, TOP_K)
        assert np.array_equal(np.frombuffer(raw, np.int32, m * TOP_K, at).reshape(m, TOP_K), tv)
        at += m * TOP_K * 4
        assert np.array_equal(np.frombuffer(raw, np.uint64, m * TOP_K, at).reshape(m, TOP_K).astype(np.int64), tc)
        at += m * TOP_K * 8
        assert np.array_equal(np.frombuffer(raw, np.uint32, m, at).astype(np.int32), found)
        if kind == "tags" and n:
            assert np.diff(tm.canonical(lims, column)[0]).max() == 1024      # the long rows are exactly at the limit


def _lib_host(column, lims, filters, removed, n, K):
    """cph_host_facet_values / _counts / _top on the case; a case with a "no bitmap" filter gives it as all ones."""
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    col = np.ascontiguousarray(column, np.int32)
    l64 = None if lims is None else np.ascontiguousarray(lims, np.uint64)
    nw, m = (n + 31) // 32, len(filters)
    words = np.stack([np.full(nw, 0xFFFFFFFF, np.uint32) if w is None else w for w in filters]) if m else np.zeros((0, nw), np.uint32)
    words = np.ascontiguousarray(words, np.uint32)
    rem = None if removed is None else fm.pack(removed)
    args = (col.ctypes.data if col.size else None, col.size, None if l64 is None else l64.ctypes.data, n)
    masks = (words.ctypes.data if words.size else None, None if rem is None or not rem.size else rem.ctypes.data, m)
    U = np.zeros(1, np.uint64)
    _lib.check(L.cph_host_facet_values(*args, U.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64)), None))
    values = np.full(int(U[0]), 77, np.int32)
    _lib.check(L.cph_host_facet_values(*args, U.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64)), values.ctypes.data if values.size else None))
    counts = np.full((m, int(U[0])), 12345, np.uint64)
    _lib.check(L.cph_host_facet_counts(*args, *masks, counts.ctypes.data if counts.size else None))
    tv, tc, found = np.full((m, K), 77, np.int32), np.full((m, K), 77, np.uint64), np.full(m, 77, np.uint32)
    _lib.check(L.cph_host_facet_top(*args, *masks, K, tv.ctypes.data, tc.ctypes.data, found.ctypes.data))
    return values, counts.astype(np.int64), tv, tc.astype(np.int64), found.astype(np.int32)


@pytest.mark.parametrize("kind", COLUMN_KINDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", FILTER_COUNTS)
def test_library_host_entries_match_the_model(n, m, kind):
    column, lims, filters, removed = _case(n, m, kind)
    ev, _, ec = _expect(column, lims, filters, removed, n)
    values, counts, tv, tc, found = _lib_host(column, lims, filters, removed, n, TOP_K)
    assert np.array_equal(values, ev) and np.array_equal(counts, ec)
    etv, etc, efound = fm.top(ev, ec, TOP_K)
    assert np.array_equal(tv, etv) and np.array_equal(tc, etc) and np.array_equal(found, efound)


def test_library_host_entries_refuse_and_write_nothing():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    col = np.arange(5, dtype=np.int32)
    tv, tc, found = np.full(4, 77, np.int32), np.full(4, 77, np.uint64), np.full(1, 77, np.uint32)
    for K in (0, 1025):
        with pytest.raises(ValueError):
            _lib.check(L.cph_host_facet_top(col.ctypes.data, 5, None, 5, None, None, 1, K, tv.ctypes.data, tc.ctypes.data, found.ctypes.data))
    counts = np.full(5, 77, np.uint64)
    with pytest.raises(ValueError):          # a dense column has one entry per row
        _lib.check(L.cph_host_facet_counts(col.ctypes.data, 5, None, 4, None, None, 1, counts.ctypes.data))
    lims = np.array([0, 3, 2], np.uint64)
    with pytest.raises(ValueError):          # decreasing limits
        _lib.check(L.cph_host_facet_counts(col.ctypes.data, 2, lims.ctypes.data, 2, None, None, 1, counts.ctypes.data))
    assert (tv == 77).all() and (tc == 77).all() and (found == 77).all() and (counts == 77).all()
    assert L.cph_version() >= 118
    assert 1 <= L.cph_facet_onchip_limit() and L.cph_facet_slab_counters() >= L.cph_facet_onchip_limit()
