"""CPU tier of the exact-kNN kernels (device_knn.h, device_knn_sym.h): their host statement and the census of the cases.

cph_host_knn (csrc/host_knn.h behind the library's host-only hook, no HIP call) is judged by the float64 reference and the
derived bound of tests/knn_model.py on every row of every case the GPU tier runs (tests/test_gpu_knn.py compares the kernels
with it byte for byte).  The census: every case asserts here, on the CPU, what it promises -- the descending columns are
nearer than all earlier ones by more than both tolerances, the plain join cases keep the fallback at or below 25 % of the
rows, the dups and outlier cases have fallback rows of both kinds.  tests/knn_host/knn_host.cpp includes the header, is built
with plain g++ and -fsanitize=address,undefined -ffp-contract=off and runs the same cases as a child process on buffers of
exactly the stated sizes.  No sanitizer touches code loaded into Python."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import knn_model as km

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "knn_host", "knn_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("name", km.CASE_NAMES)
def test_host_model_against_float64(name):
    ids, dist, redo, cand = km.model(name)
    km.check_case(name, ids, dist)
    assert (cand is None) == (km.case(name).path == 0) and (redo == 0 or cand is not None)


def test_rows_worked_by_hand():
    """dim = 1, integers: every product and sum is exact.  x = 0, 1, 1, 3."""
    X = np.array([[0], [1], [1], [3]], np.float32)
    ids, dist, redo, cand = km.host_knn(X)
    assert ids[:, :3].tolist() == [[1, 2, 3], [2, 0, 3], [1, 0, 3], [1, 2, 0]] and (ids[:, 3:] == km.PAD).all()
    assert dist[:, :3].tolist() == [[1, 1, 9], [0, 1, 4], [0, 1, 4], [4, 4, 9]] and (dist[:, 3:] == km.FMAX).all() and redo == 0
    Q = np.array([[2], [-1]], np.float32)
    ids, dist, _, _ = km.host_knn(X, Q)
    assert ids[:, :4].tolist() == [[1, 2, 3, 0], [0, 1, 2, 3]] and dist[:, :4].tolist() == [[1, 1, 1, 4], [1, 4, 4, 16]]
    ids, dist, _, _ = km.host_knn(X, Q, q_ids=np.array([2, 0], np.uint32))          # row 0 is "row 2", row 1 is "row 0"
    assert ids[:, :3].tolist() == [[1, 3, 0], [1, 2, 3]] and (ids[:, 3:] == km.PAD).all()


def test_chain_order_is_the_kernels():
    """The order inside every group of eight coordinates is 0, 4, 1, 5, 2, 6, 3, 7.  The chains are re-done here in numpy (a
    float32 product is exact in float64, and with operands this close in size so is its sum with a float32: one rounding, an
    fmaf) in that order, in index order and with the second and third of the four MFMAs swapped; the model's distances have
    the bytes of the first and of neither of the others."""
    def chain(a, b, init, order):
        acc = np.full(len(b), init, np.float32)
        for k in order:
            acc = (a[..., k].astype(np.float64) * b[:, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        return acc
    rng = np.random.default_rng(5)
    X = rng.standard_normal((64, 16)).astype(np.float32)
    q = rng.standard_normal((1, 16)).astype(np.float32)
    ids, dist, _, _ = km.host_knn(X, q)
    bn = chain(X, X, 0, range(16))
    qn = chain(q, q, 0, range(16))
    got = np.zeros(64, np.float32)
    got[ids[0]] = dist[0]                                    # the 32 nearest; the others stay 0 and are not compared
    differ = {}
    for label, in8 in (("kernel", (0, 4, 1, 5, 2, 6, 3, 7)), ("index", range(8)), ("yz", (0, 4, 2, 6, 1, 5, 3, 7))):
        s = chain(q[0], X, np.float32(-0.5) * bn, [8 * g + e for g in range(2) for e in in8])
        d = np.maximum(qn - np.float32(2) * s, np.float32(0)).astype(np.float32)
        differ[label] = int((d[ids[0]].view(np.uint32) != got[ids[0]].view(np.uint32)).sum())
    assert differ["kernel"] == 0 and differ["index"] > 0 and differ["yz"] > 0, differ


def test_census_descending_columns_pass_any_stale_threshold():
    """Every column nearer than all earlier ones by more than tol_i + tol_j (so whatever the float32 keys are, each beats every
    threshold a list can hold when it arrives, and a row of nb columns compacts at least (nb - 64) / 32 times); the ascending
    case the other way round."""
    for name in ("descending_d32", "descending_d128", "ascending_d32"):
        c = km.case(name)
        d64, tol = km.reference(c.X, c.Q)
        if c.promise["order"] == "ascending":
            d64, tol = d64[:, ::-1], tol[:, ::-1]
        assert d64.shape == (40, 400) and km.padded_dim(c.X.shape[1]) == int(name.split("_d")[1])
        worst_before = np.minimum.accumulate(d64 - tol, axis=1)[:, :-1]             # the nearest any earlier column can look
        assert (d64[:, 1:] + tol[:, 1:] < worst_before).all(), name
        assert (400 - 64) // 32 >= 10


def test_census_join_fallback_counts():
    seen_n, seen_D = set(), set()
    for name in km.CASE_NAMES:
        c = km.case(name)
        if c.path != 1:
            continue
        ids, dist, redo, cand = km.model(name)
        n = len(c.X)
        assert redo == int(((cand < 32) | (cand > 256)).sum())
        if c.promise.get("plain"):
            assert redo <= n // 4, (name, redo)                  # the join, not its fallback, is the code under test
            seen_n.add(n)
            seen_D.add(km.padded_dim(c.X.shape[1]))
        if c.promise.get("overflow"):
            assert redo > 0 and (cand > 256).any() and (cand < 32).any(), name
    assert seen_n >= {1024, 1025, 1151, 1152, 1153, 1409} and seen_D >= {64, 128, 256, 2048}
    dups = km.model("join_dups")[3]
    assert dups.max() >= 299                                     # 299 copies at distance zero: past the cap of 256


def test_census_shapes():
    names = set(km.CASE_NAMES)
    assert {f"self_nb{nb}" for nb in km.NB_EDGES} | {f"q{nq}_nb{nb}" for nq in km.NQ_EDGES for nb in km.NB_EDGES} <= names
    assert {km.padded_dim(d) for d in km.DIMS} == {32, 64, 128, 256} and km.padded_dim(1536) == 2048
    c = km.case("q_ids")
    assert len(c.Q) == 130 and len(c.X) == 300 and c.Q.tobytes() == c.X[c.q_ids].tobytes()
    c = km.case("large_norms")
    d64, _ = km.reference(c.X)
    np.fill_diagonal(d64, np.inf)
    assert (c.X ** 2).sum(1).min() > 1e5 * d64.min(1)[c.promise["near"]].max() and (c.X == np.round(c.X)).all()
    c = km.case("three_copies")
    assert len(c.X) == 257 and len(c.X) % 128 == 1
    c = km.case("scattered_copies")
    assert len(set(c.promise["copies"] // 128)) == 4 and len(c.promise["copies"]) == 40


def test_refusals():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    X = np.zeros((1100, 40), np.float32)
    ids, dist = np.full((1100, 32), 7, np.uint32), np.full((1100, 32), 7, np.float32)
    qi = np.zeros(4, np.uint32)
    bad_qi = np.array([0, 1100, 0, 0], np.uint32)

    def call(fn, x=X, n=1100, dim=40, q=None, nq=0, q_ids=None, ex=0, path=0):
        p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        if fn == "host":
            return L.cph_host_knn(p(x), n, dim, p(q), nq, p(q_ids), ex, path, ids.ctypes.data, dist.ctypes.data, None, None)
        return L.cph_debug_knn(0, p(x), n, dim, p(q), nq, p(q_ids), ex, path, 0, ids.ctypes.data, dist.ctypes.data, None, None)
    for fn in ("host", "debug"):                                 # both answer before they touch a device
        for bad, msg in ((dict(x=None), b"bad arguments"), (dict(n=0), b"bad arguments"), (dict(dim=0), b"bad arguments"),
                         (dict(dim=4096), b"out of range"), (dict(path=2), b"path is 0"), (dict(ex=2), b"exclude_self is 0 or 1"),
                         (dict(q_ids=qi), b"go with queries"), (dict(q=X, nq=4, q_ids=qi), b"needs q_ids"), (dict(q=X, nq=4, ex=1), b"needs q_ids"),
                         (dict(q=X, nq=4, q_ids=bad_qi, ex=1), b"out of range"), (dict(q=X, nq=4, path=1), b"the join needs"),
                         (dict(n=1023, path=1), b"the join needs"), (dict(dim=32, path=1), b"the join needs"), (dict(dim=20, path=1), b"the join needs"),
                         (dict(n=4097, path=1), b"at most 4096")):
            assert call(fn, **bad) == _lib.INVALID_ARGUMENT, (fn, bad)
            assert msg in L.cph_last_error(), (fn, bad, L.cph_last_error())
            assert (ids == 7).all() and (dist == 7).all()
    assert call("host", dim=33, path=1) == _lib.OK               # padded D = 64


def test_new_symbols_are_declared():
    from cphnsw_mi355x import _lib
    import cphnsw_mi355x
    import inspect
    L = _lib.lib()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    for name in ("cph_debug_knn", "cph_host_knn"):
        assert f"int {name}(" in flat and hasattr(L, name) and name in _lib.SYMBOLS, name
    assert L.cph_version() >= 117
    assert list(inspect.signature(cphnsw_mi355x.knn_debug).parameters) == ["vectors", "queries", "q_ids", "path", "blocks_per_launch", "device"]
    builder = open(os.path.join(ROOT, "rabitq-ann-search_amd", "csrc", "builder.h")).read()
    assert "CPH_KNN_SYM" in builder and "32768" in builder       # the production switch stays where it was


# ---- the stand-alone program under sanitizers ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("knn_host")), "knn_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_host_model_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases through the stand-alone program: exact-size buffers, every output byte compared there."""
    path = os.path.join(str(tmp_path), "cases.bin")
    with open(path, "wb") as f:
        f.write(np.uint64(len(km.CASE_NAMES)).tobytes())
        for name in km.CASE_NAMES:
            c = km.case(name)
            ids, dist, redo, _ = km.model(name)
            n, dim = c.X.shape
            nq = 0 if c.Q is None else len(c.Q)
            f.write(np.array([n, dim, nq, int(c.q_ids is not None), c.path, redo], np.uint64).tobytes())
            for a in (c.X,) + (() if c.Q is None else (c.Q,)) + (() if c.q_ids is None else (c.q_ids,)) + (ids, dist):
                f.write(np.ascontiguousarray(a).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"knn: ok ({len(km.CASE_NAMES)} cases)" in r.stdout
