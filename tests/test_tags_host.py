"""CPU tier of the tag columns (cph_set_tags, cph_filters_from_tags): the host statements of the device pass.

tests/tags_host/tags_host.cpp includes csrc/host_index.h and is built with plain g++ and -fsanitize=address,undefined,
the way tests/test_labels_host.py builds its driver (a stand-alone program; nothing loaded into Python runs under a
sanitizer).  `eval` runs the canonicalisation, the gather to internal order and tag_filters_host on data written by this
test, on exact-size buffers, and every word and count is compared with the numpy model (tests/tags_model.py); `self`
compares them with a bit-by-bit loop; `refuse` must refuse.  cph_host_tag_filters (the library's host-only hook, no HIP
call) is compared with the model on the same cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tags_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "tags_host", "tags_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]

SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4100]
FILTER_COUNTS = [1, 3, 70]
VOCAB = np.array([tm.I32_MIN, -1, 0, tm.I32_MAX] + list(range(3, 15)), np.int64)
COLUMN_KINDS = ["mixed", "all_empty"]


def _column(n, kind):
    """rows as given by a caller: unsorted, with duplicates; a third empty; up to two rows of exactly 1,024 distinct
    tags (n permitting: the first and the last row); kind "all_empty": no tag at all (the column goes in with a NULL
    tags pointer)."""
    rng = np.random.default_rng(7000 + n)
    rows = []
    for i in range(n):
        if kind == "all_empty" or rng.random() < 0.33:
            rows.append(np.zeros(0, np.int64))
            continue
        r = VOCAB[rng.integers(0, len(VOCAB), rng.integers(1, 10))]
        rows.append(np.concatenate([r, r[:rng.integers(0, 3)]]))          # duplicates, any order
    if kind == "mixed" and n:
        long_row = np.concatenate([np.arange(20000, 21024), [20000, 20500, 21023]])      # 1,024 distinct, 1,027 given
        rows[0] = rng.permutation(long_row)
        rows[-1] = rng.permutation(long_row + 1)
    return rows


def _tests(m, seed):
    present = list(VOCAB) + [20000, 21024]
    off = seed % 24                                       # (every kind and mode shows up across the sizes even at m = 1)
    ts = [tm.test_kinds(present, j + off) for j in range(m)]
    return [t for t, _ in ts], [mode for _, mode in ts]


def _case(n, m, kind):
    rows = _column(n, kind)
    lims, tags = tm.to_csr(rows)
    tests, modes = _tests(m, n + m)
    order = np.random.default_rng(n + 7).permutation(n)
    return lims, tags, tests, modes, order


def _flat_tests(tests, modes):
    tl, tv = tm.to_csr(tests)
    return tl.astype(np.uint32), tv.astype(np.int32), np.array([tm.MODES[x] for x in modes], np.uint8)


def _write(path, lims, tags, order, tests, modes, has_tags=None, nnz=None):
    tl, tv, codes = _flat_tests(tests, modes)
    n, m = len(lims) - 1, len(tests)
    nnz = len(tags) if nnz is None else nnz
    has = (len(tags) != 0) if has_tags is None else has_tags
    with open(path, "wb") as f:
        f.write(np.array([n, m, nnz, len(tv), int(has)], np.uint64).tobytes() + np.asarray(lims, np.uint64).tobytes() +
                np.asarray(tags, np.int32).tobytes() + np.asarray(order, np.uint32).tobytes() + tl.tobytes() + tv.tobytes() +
                codes.tobytes())


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("tags_host")), "tags_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(cmd, timeout=600, ok=True):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    if ok:
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    return r


def test_tag_statements_against_a_loop_under_asan_ubsan(asan_exe):
    assert "self: ok" in _run([asan_exe, "self"]).stdout


@pytest.mark.parametrize("kind", COLUMN_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_tag_statements_against_the_model_under_asan_ubsan(asan_exe, tmp_path, n, kind):
    """Canonicalisation, gather to internal order and tag_filters_host (every m): every word and count, the tail bits
    of the last word included."""
    for m in FILTER_COUNTS:
        lims, tags, tests, modes, order = _case(n, m, kind)
        fin, fout = str(tmp_path / f"in{m}.bin"), str(tmp_path / f"out{m}.bin")
        _write(fin, lims, tags, order, tests, modes)
        assert "eval: ok" in _run([asan_exe, "eval", fin, fout]).stdout
        raw = open(fout, "rb").read()
        clims, ctags = tm.canonical(lims, tags, order)
        nw, nnz = (n + 31) // 32, len(ctags)
        assert int(np.frombuffer(raw, np.uint64, 1)[0]) == nnz
        assert len(raw) == 8 + (n + 1) * 4 + nnz * 4 + m * nw * 4 + m * 8
        got_lims = np.frombuffer(raw, np.uint32, n + 1, 8)
        got_tags = np.frombuffer(raw, np.int32, nnz, 8 + (n + 1) * 4)
        words = np.frombuffer(raw, np.uint32, m * nw, 8 + (n + 1 + nnz) * 4).reshape(m, nw)
        counts = np.frombuffer(raw, np.uint64, m, 8 + (n + 1 + nnz + m * nw) * 4)
        assert np.array_equal(got_lims, clims) and np.array_equal(got_tags, ctags)
        if kind == "mixed" and n:
            assert np.diff(clims).max() == 1024                  # the long rows are exactly at the limit after dedup
        ew, ec = tm.expect(clims, ctags, tests, modes)
        assert np.array_equal(words, ew)                     # every word written, tail bits of the last word clear
        assert np.array_equal(counts, ec)


def _hook(lims, tags, tests, modes):
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    tl, tv, codes = _flat_tests(tests, modes)
    n, m = len(lims) - 1, len(tests)
    nw = (n + 31) // 32
    words = np.full((m, nw), 0xDEADBEEF, np.uint32)
    counts = np.full(m, 12345, np.uint64)
    l32, t32 = np.asarray(lims, np.uint32), np.asarray(tags, np.int32)
    _lib.check(L.cph_host_tag_filters(l32.ctypes.data, t32.ctypes.data if t32.size else None, n, tl.ctypes.data,
                                      tv.ctypes.data if tv.size else None, codes.ctypes.data, m, words.ctypes.data if n else None,
                                      counts.ctypes.data))
    return words, counts


@pytest.mark.parametrize("kind", COLUMN_KINDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", FILTER_COUNTS)
def test_host_tag_filters_hook_matches_the_model(n, m, kind):
    lims, tags, tests, modes, _ = _case(n, m, kind)
    words, counts = _hook(lims, tags, tests, modes)
    clims, ctags = tm.canonical(lims, tags)
    ew, ec = tm.expect(clims, ctags, tests, modes)
    assert np.array_equal(words, ew)
    assert np.array_equal(counts, ec)


def test_model_semantics_by_hand():
    """The model itself on a column small enough to read: rows {}, {1}, {1, 2}, {2, 3}, {INT32_MIN, INT32_MAX}."""
    lims, tags = tm.canonical(*tm.to_csr([[], [1, 1], [2, 1], [3, 2, 3], [tm.I32_MAX, tm.I32_MIN]]))
    assert list(lims) == [0, 0, 1, 3, 5, 7] and list(tags) == [1, 1, 2, 2, 3, tm.I32_MIN, tm.I32_MAX]
    f = lambda v, mode: list(tm.allowed(lims, tags, v, mode).astype(int))
    assert f([1], "any") == [0, 1, 1, 0, 0] and f([1, 2], "all") == [0, 0, 1, 0, 0] and f([1, 2], "none") == [1, 0, 0, 0, 1]
    assert f([], "any") == [0] * 5 and f([], "all") == [1] * 5 and f([], "none") == [1] * 5
    assert f([2, 2, 1], "all") == [0, 0, 1, 0, 0] and f([tm.I32_MIN, tm.I32_MAX], "all") == [0, 0, 0, 0, 1]
    assert f([tm.NOBODY], "none") == [1] * 5 and f([tm.NOBODY, 3], "any") == [0, 0, 0, 1, 0]


REFUSALS = {
    "1025 distinct tags in a row": dict(rows=[[1], list(range(1025))], tests=[[1]], modes=[0]),
    "65 distinct test values": dict(rows=[[1], [2]], tests=[list(range(65))], modes=[0]),
    "a decreasing lims": dict(lims=[0, 2, 1], tags=[1, 2], tests=[[1]], modes=[0]),
    "lims[0] != 0": dict(lims=[1, 2, 2], tags=[1, 2], tests=[[1]], modes=[0]),
    "a mode of 3": dict(rows=[[1], [2]], tests=[[1]], modes=[3]),
}


def _refusal(spec):
    if "rows" in spec:
        lims, tags = tm.to_csr(spec["rows"])
    else:
        lims, tags = np.array(spec["lims"], np.int64), np.array(spec["tags"], np.int64)
    tl, tv = tm.to_csr(spec["tests"])
    return lims, tags, tl.astype(np.uint32), tv.astype(np.int32), np.array(spec["modes"], np.uint8)


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(asan_exe, tmp_path, what):
    """The driver's canonicalisation and the library hook refuse the same inputs; 1,024 tags and 64 values pass."""
    from cphnsw_mi355x import _lib
    lims, tags, tl, tv, codes = _refusal(REFUSALS[what])
    n, m = len(lims) - 1, len(tl) - 1
    fin = str(tmp_path / "bad.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, m, len(tags), len(tv), 1], np.uint64).tobytes() + lims.astype(np.uint64).tobytes() +
                tags.astype(np.int32).tobytes() + np.arange(n, dtype=np.uint32).tobytes() + tl.tobytes() + tv.tobytes() + codes.tobytes())
    r = _run([asan_exe, "refuse", fin], ok=False)
    assert r.returncode == 0 and "refused:" in r.stdout, (what, r.stdout[-500:], r.stderr[-3000:])
    words, counts = np.zeros((m, 1), np.uint32), np.zeros(m, np.uint64)
    l32, t32 = lims.astype(np.uint32), tags.astype(np.int32)
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().cph_host_tag_filters(l32.ctypes.data, t32.ctypes.data, n, tl.ctypes.data, tv.ctypes.data, codes.ctypes.data,
                                                    m, words.ctypes.data, counts.ctypes.data))


def test_limits_themselves_pass():
    from cphnsw_mi355x import _lib
    rows = [list(range(1024)) + [0, 5], []]
    tests, modes = [list(range(64)) + [3], list(range(960, 1024))], ["all", "any"]
    words, counts = _hook(*tm.to_csr(rows), tests, modes)
    assert list(counts) == [1, 1] and list(words[:, 0]) == [1, 1]
    assert _lib.lib().cph_version() >= 116
