"""CPU tier of grouped search (search_grouped): the host statement of the grouping pass.

cph_host_group_rows (csrc/host_group.h behind the library's host-only hook, no HIP call) is compared, byte for byte in all
five outputs, with tests/group_model.py on synthetic candidate rows: every C in {1, 63, 64, 65, 70, 128, 1000, 1024} with
every (k, g) of {(1,1), (3,2), (10,3), (64,1), (1,64), (32,32)} that fits (k * g <= C), each with and without a row map.
tests/group_host/group_host.cpp includes csrc/host_group.h, is built with plain g++ and -fsanitize=address,undefined and
runs the same cases as a child process on buffers of exactly the stated sizes, the way tests/test_add_host.py runs its
driver.  No sanitizer touches code loaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from group_model import (FMAX, I32_MAX, I32_MIN, N_IDS, ROW_KINDS, group_model, group_model_batch, host_group_rows, same_bytes,
                         shapes, synth_batch)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "group_host", "group_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]


def _rows_of(kinds, kind):
    return [i for i, x in enumerate(kinds) if x == kind]


def _check_batch_promises(Cn, k, g, ids, dist, key_of, kinds, want):
    """The batch holds what the case list promises (so that a generator that quietly stopped producing a case fails here)."""
    w_ids, w_dist, w_keys, w_counts, w_complete = want
    at = {kind: _rows_of(kinds, kind)[0] for kind in ROW_KINDS}
    valid = (ids >= 0).sum(axis=1)
    assert len(set(key_of[ids[at["one_key"]]])) == 1
    assert len(set(key_of[ids[at["distinct_keys"]]])) == Cn
    assert set(key_of[ids[at["special_keys"]]]) <= {I32_MIN, -1, 0, 1, I32_MAX}
    if Cn >= 5:
        assert set(key_of[ids[at["special_keys"]]]) == {I32_MIN, -1, 0, 1, I32_MAX} or Cn < 40
    if Cn >= 6:
        _, c = np.unique(ids[at["repeated_ids"]], return_counts=True)
        assert 2 in c and 3 in c
    assert valid[at["all_padding"]] == 0 and (Cn < 3 or 0 < valid[at["partly_padding"]] < Cn)
    d = dist[at["equal_distances"]]
    if Cn >= 63:
        zeros = d[d == 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()       # +0.0 and -0.0 side by side
        assert (np.diff(d) >= 0).all() and (np.diff(d) == 0).sum() > Cn // 2
    if k > 3 and Cn >= 3:
        assert 0 < (w_counts[at["few_keys"]] > 0).sum() < k
    # exactly full at the last entry / one entry before the end: the entry that completes the answer sits there
    for kind, pos in (("full_at_last", Cn - 1), ("full_before_last", max(Cn - 2, k * g - 1))):
        r = at[kind]
        assert (w_counts[r] == g).all() and w_complete[r] == 1
        cut = ids[r].copy()
        cut[pos:] = -1
        assert not (group_model(cut, dist[r], key_of, k, g)[3] == g).all(), (kind, "is full before", pos)
    # complete and incomplete rows, and complete for each of the two reasons alone
    full = (w_counts == g).all(axis=1)
    assert (full & (valid == Cn)).any(), "no row is complete because its groups are full"
    assert (~full & (valid < Cn) & (w_complete == 1)).any(), "no row is complete because the search ran dry"
    if k * g > 1:
        assert (w_complete == 0).any(), "no incomplete row"
        assert ((w_complete == 0) == (~full & (valid == Cn))).all()
    # padding: every slot behind a group's members, every group behind the last
    for q in range(ids.shape[0]):
        for j in range(k):
            c = w_counts[q, j]
            assert (w_ids[q, j, c:] == -1).all() and (w_dist[q, j, c:] == FMAX).all() and (w_ids[q, j, :c] >= 0).all()
            assert c > 0 or w_keys[q, j] == 0


@pytest.mark.parametrize("Cn,k,g", shapes())
def test_host_group_rows_matches_the_model(Cn, k, g):
    ids, dist, key_of, rows, kinds = synth_batch(Cn, k, g, seed=1)
    assert ids.shape == (len(ROW_KINDS), Cn) and key_of.shape == (N_IDS,) and sorted(rows.tolist()) == list(range(N_IDS))
    want = group_model_batch(ids, dist, key_of, k, g)
    _check_batch_promises(Cn, k, g, ids, dist, key_of, kinds, want)
    assert same_bytes(host_group_rows(ids, dist, key_of, k, g), want)
    want_rows = group_model_batch(ids, dist, key_of, k, g, rows)
    assert same_bytes(host_group_rows(ids, dist, key_of, k, g, rows), want_rows)
    # the row map only renames members
    assert want_rows[1].tobytes() == want[1].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(want_rows[2:], want[2:]))
    m = want[0] >= 0
    assert np.array_equal(want_rows[0][m], rows[want[0][m]]) and (want_rows[0][~m] == -1).all()


def test_model_on_a_row_worked_by_hand():
    key_of = np.array([5, 5, -1, 5, I32_MIN, -1, 0, I32_MAX], np.int32)
    ids = np.array([3, 2, 3, 0, -1, 4, 1, 5, 7, 6], np.int64)            # 3 twice; padding in between
    dist = np.array([-0.0, 0.0, 0.0, 1.0, FMAX, 1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    w = group_model(ids, dist, key_of, 3, 2)
    assert w[0].tolist() == [[3, 0], [2, 5], [4, -1]]                      # 1 (key 5) is dropped: its group is full
    assert w[1].tobytes() == np.array([[-0.0, 1.0], [0.0, 3.0], [1.0, FMAX]], np.float32).tobytes()
    assert w[2].tolist() == [5, -1, I32_MIN] and w[3].tolist() == [2, 2, 1]
    assert w[4]                                                             # one entry is padding: the search ran dry
    ids[4] = 6
    assert not group_model(ids, dist, key_of, 3, 2)[4]
    got = host_group_rows(ids[None], dist[None], key_of, 3, 2)
    assert same_bytes(got, group_model_batch(ids[None], dist[None], key_of, 3, 2))


def test_host_group_rows_refuses_bad_arguments():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    ids, dist, key_of, rows, _ = synth_batch(70, 3, 2, seed=3)
    n = ids.shape[0]
    o = (np.empty((n, 64, 64), np.int64), np.empty((n, 64, 64), np.float32), np.empty((n, 1024), np.int32), np.empty((n, 1024), np.int32),
         np.empty(n, np.uint8))
    po = [x.ctypes.data for x in o]

    def call(i=ids, d=dist, nn=n, Cn=70, ko=key_of, nk=N_IDS, k=3, g=2, out=po):
        return L.cph_host_group_rows(None if i is None else i.ctypes.data, None if d is None else d.ctypes.data, nn, Cn,
                                     None if ko is None else ko.ctypes.data, nk, None, k, g, *out)
    assert call() == _lib.OK
    for bad in (dict(i=None), dict(d=None), dict(ko=None), dict(k=0), dict(g=0), dict(k=36, g=2), dict(k=71, g=1), dict(k=1, g=71),
                dict(Cn=0), dict(nn=0), dict(nk=0), dict(nk=int(ids.max())), dict(out=[None] + po[1:]), dict(out=po[:4] + [None])):
        assert call(**bad) == _lib.INVALID_ARGUMENT, bad
        assert L.cph_last_error()
    big = np.zeros((1, 1025), np.int64)
    assert call(i=big, d=np.zeros((1, 1025), np.float32), nn=1, Cn=1025, k=1, g=1) == _lib.INVALID_ARGUMENT
    assert b"1024" in L.cph_last_error()
    # the other new entry points answer before they touch a device
    assert L.cph_search_grouped(None, None, 0, 1, 1, 64, None, None, 0, None, 0, None, None, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_search_grouped_device(None, None, 0, 1, 1, 64, None, None, 0, None, 0, None, None, None, None, None,
                                       None) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_search_grouped(None, None, 0, 1, 1, 64, None, None, 0, None, 0, None, None, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_group_keys_create(None, None, 0, 0, None) == _lib.INVALID_ARGUMENT
    assert L.cph_group_keys_destroy(None) == _lib.OK
    assert L.cph_group_rows_hook(0, None, None, 1, 64, None, 1, None, 1, 1, None, None, None, None, None) == _lib.INVALID_ARGUMENT


def test_new_symbols_are_declared_with_the_issue_s_signatures():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    call = ("uint64_t n, uint64_t k, uint64_t group_size, uint64_t candidates, const cph_group_keys* keys, const cph_filter* const* "
            "filters, uint32_t n_filters, const int32_t* filter_of, int exact, ")
    rows_args = ("const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const int32_t* key_of, uint64_t n_keys, "
                 "const uint32_t* rows, uint64_t k, uint64_t group_size, int64_t* out_ids, float* out_dist, int32_t* out_keys, "
                 "int32_t* out_counts, uint8_t* out_complete);")
    for decl in ("typedef struct cph_group_keys cph_group_keys;",
                 "int cph_group_keys_create(cph_index* h, const int32_t* keys, uint64_t size, int space, cph_group_keys** out);",
                 "int cph_group_keys_destroy(cph_group_keys* keys);",
                 "int cph_search_grouped(cph_index* h, const float* queries, " + call +
                 "int64_t* ids, float* dist, int32_t* group_keys, int32_t* counts, uint8_t* complete);",
                 "int cph_search_grouped_device(cph_index* h, const float* d_queries, " + call +
                 "int64_t* d_ids, float* d_dist, int32_t* d_group_keys, int32_t* d_counts, uint8_t* d_complete, void* stream);",
                 "int cph_multi_search_grouped(cph_multi* m, const float* queries, " + call.replace("cph_group_keys* keys", "cph_group_keys* const* keys") +
                 "int64_t* ids, float* dist, int32_t* group_keys, int32_t* counts, uint8_t* complete);",
                 "int cph_group_rows_hook(int device, " + rows_args,
                 "int cph_host_group_rows(" + rows_args):
        assert decl in flat, decl
    p, u64 = C.c_void_p, C.c_uint64
    grouped = [p, p, u64, u64, u64, u64, p, p, C.c_uint32, p, C.c_int, p, p, p, p, p]
    rows_sig = [p, p, u64, u64, p, u64, p, u64, u64, p, p, p, p, p]
    want = {"cph_group_keys_create": [p, p, u64, C.c_int, C.POINTER(p)], "cph_group_keys_destroy": [p],
            "cph_search_grouped": grouped, "cph_search_grouped_device": grouped + [p], "cph_multi_search_grouped": grouped,
            "cph_group_rows_hook": [C.c_int] + rows_sig, "cph_host_group_rows": rows_sig}
    for name, args in want.items():
        assert hasattr(L, name) and _lib.SYMBOLS[name] == (C.c_int, args), name
    assert L.cph_version() >= 107


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("group_host")), "group_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_group_rows_host_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases as above, through the stand-alone program: exact-size buffers, every output byte compared there."""
    path = os.path.join(str(tmp_path), "cases.bin")
    n_cases = 0
    with open(path, "wb") as f:
        f.write(np.uint64(0).tobytes())
        for (Cn, k, g) in shapes():
            ids, dist, key_of, rows, _ = synth_batch(Cn, k, g, seed=1)
            for rm in (None, rows):
                want = group_model_batch(ids, dist, key_of, k, g, rm)
                f.write(np.array([ids.shape[0], Cn, k, g, key_of.size, int(rm is not None)], np.uint64).tobytes())
                for a in (ids, dist, key_of) + (() if rm is None else (rm,)) + want:
                    f.write(np.ascontiguousarray(a).tobytes())
                n_cases += 1
        f.seek(0)
        f.write(np.uint64(n_cases).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"group: ok ({n_cases} cases)" in r.stdout and n_cases == 2 * len(shapes())
