"""CPU tier of the cosine metric: the host statement of the row normalisation.

tests/cosine_model.py is the statement in numpy.  cph_host_normalize_rows (csrc/host_normalize.h behind the library's
host-only hook, no HIP call) is compared with the model byte for byte: dims on both sides of the 64-lane stride and in the
multi-pass loop, 1, 3 and 130 rows, per-row scales 2^-20 .. 2^20; scale invariance under powers of two; the norm bound;
the four kinds of bad row at the first, a middle and the last row; in place.  tests/cosine_host/cosine_host.cpp includes
csrc/host_normalize.h, is built with plain g++, -fsanitize=address,undefined and -ffp-contract=off and runs the same cases
as a child process on buffers of exactly the stated sizes, the way tests/test_diverse_host.py runs its driver.  No
sanitizer touches code loaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cosine_model import BAD_KINDS, DIMS, NO_BAD_ROW, NS, bad_cases, case_rows, cases, normalize_model

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cosine_host", "cosine_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]


def host_normalize_rows(x, in_place=False):
    from cphnsw_mi355x import _lib
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    out = x.copy() if in_place else np.full(x.shape, np.float32(np.frombuffer(b"\xa5" * 4, np.float32)[0]), np.float32)
    src = out if in_place else x
    bad, first = C.c_uint64(77), C.c_uint64(77)
    _lib.check(_lib.lib().cph_host_normalize_rows(src.ctypes.data, n, dim, out.ctypes.data, C.byref(bad), C.byref(first)))
    return out, int(bad.value), int(first.value)


def test_case_list_covers_what_the_issue_names():
    assert set(DIMS) == {1, 3, 63, 64, 65, 127, 128, 130, 960} and set(NS) == {1, 3, 130}
    assert len(cases()) == len(DIMS) * len(NS) and set(BAD_KINDS) == {"zero", "nan", "inf", "overflow"}
    x = case_rows(130, 64)
    norms = np.linalg.norm(x.astype(np.float64), axis=1)
    assert norms.max() / norms.min() > 2.0 ** 38            # scales from 2^-20 to 2^20 are really there


@pytest.mark.parametrize("n,dim", cases())
def test_host_twin_has_the_model_s_bytes(n, dim):
    x = case_rows(n, dim)
    want, wbad, wfirst = normalize_model(x)
    assert wbad == 0 and wfirst == NO_BAD_ROW
    got, bad, first = host_normalize_rows(x)
    assert got.tobytes() == want.tobytes() and (bad, first) == (0, NO_BAD_ROW)
    # in place == out of place
    got2, bad2, first2 = host_normalize_rows(x, in_place=True)
    assert got2.tobytes() == want.tobytes() and (bad2, first2) == (0, NO_BAD_ROW)


@pytest.mark.parametrize("dim", DIMS)
def test_scaling_a_row_by_a_power_of_two_changes_no_byte(dim):
    # plain Gaussian rows: every square stays a normal float32 under the exponents below, so no rounding moves
    x = np.random.default_rng(dim).standard_normal((3, dim)).astype(np.float32)
    assert np.abs(x[x != 0]).min() > 2.0 ** -20
    want = normalize_model(x)[0]
    for e in (-40, -7, 1, 13, 40):
        y = (x * np.float32(2.0 ** e)).astype(np.float32)
        assert np.isfinite(y).all() and (y != 0).sum() == (x != 0).sum()
        assert normalize_model(y)[0].tobytes() == want.tobytes(), e
        assert host_normalize_rows(y)[0].tobytes() == want.tobytes(), e


@pytest.mark.parametrize("n,dim", cases())
def test_squared_norm_is_one_half_within_the_rounding_bound(n, dim):
    """Products, sums and the division each round below one ulp of a value of at most 1/2: (dim + 8) * 2^-24 in all."""
    out = host_normalize_rows(case_rows(n, dim))[0].astype(np.float64)
    err = np.abs((out * out).sum(axis=1) - 0.5)
    assert err.max() <= (dim + 8) * 2.0 ** -24, err.max()


@pytest.mark.parametrize("dim", (1, 3, 64, 65, 130))
def test_bad_rows_are_zeroed_counted_and_leave_their_neighbours_alone(dim):
    for kind, pos, x in bad_cases(dim):
        clean = x.copy()
        clean[pos] = 1.0
        ref = normalize_model(clean)[0]
        want, wbad, wfirst = normalize_model(x)
        assert (wbad, wfirst) == (1, pos)
        for in_place in (False, True):
            got, bad, first = host_normalize_rows(x, in_place=in_place)
            assert (bad, first) == (1, pos), (kind, pos)
            assert got.tobytes() == want.tobytes(), (kind, pos)
            assert got[pos].tobytes() == np.zeros(dim, np.float32).tobytes()            # +0.0, every slot
            others = np.arange(len(x)) != pos
            assert got[others].tobytes() == ref[others].tobytes()                       # the neighbours are untouched
    # several bad rows: all counted, the lowest reported
    x = case_rows(9, dim)
    x[[2, 5, 8]] = 0.0
    assert host_normalize_rows(x)[1:] == (3, 2) == normalize_model(x)[1:]


def test_host_hook_validates_its_arguments():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    x = np.ones((2, 4), np.float32)
    o = np.zeros_like(x)
    assert L.cph_host_normalize_rows(None, 2, 4, o.ctypes.data, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_host_normalize_rows(x.ctypes.data, 2, 4, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_host_normalize_rows(x.ctypes.data, 2, 0, o.ctypes.data, None, None) == _lib.INVALID_ARGUMENT
    assert (o == 0).all()
    assert L.cph_host_normalize_rows(x.ctypes.data, 2, 4, o.ctypes.data, None, None) == _lib.OK      # null counters are allowed
    assert o.tobytes() == normalize_model(x)[0].tobytes()
    # the other new entry points answer before they touch a device
    assert L.cph_set_metric(None, 1) == _lib.INVALID_ARGUMENT
    assert L.cph_get_metric(None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_set_metric(None, 1) == _lib.INVALID_ARGUMENT
    assert L.cph_parts_set_metric(None, 1) == _lib.INVALID_ARGUMENT
    assert L.cph_metric_stats(None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_normalize_rows_hook(0, None, 1, 4, None, None, None) == _lib.INVALID_ARGUMENT


def test_new_symbols_are_declared_with_the_issue_s_signatures():
    from cphnsw_mi355x import _lib
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    for decl in ("enum { CPH_METRIC_L2 = 0, CPH_METRIC_COSINE = 1 };",
                 "int cph_set_metric(cph_index* h, int metric);", "int cph_get_metric(cph_index* h, int* metric);",
                 "int cph_multi_set_metric(cph_multi* m, int metric);", "int cph_parts_set_metric(cph_parts* m, int metric);",
                 "int cph_normalize_rows_hook(int device, const float* x, uint64_t n, uint64_t dim, float* out, uint64_t* bad_count, "
                 "uint64_t* first_bad);",
                 "int cph_host_normalize_rows(const float* x, uint64_t n, uint64_t dim, float* out, uint64_t* bad_count, "
                 "uint64_t* first_bad);"):
        assert decl in flat, decl
    assert (_lib.METRIC_L2, _lib.METRIC_COSINE) == (0, 1)
    assert _lib.lib().cph_version() >= 110


def test_python_metric_argument_is_checked_before_any_device_is_touched():
    import cphnsw_mi355x
    with pytest.raises(ValueError, match="metric"):
        cphnsw_mi355x.CPIndex(24, 4, metric="dot")
    with pytest.raises(ValueError, match="metric"):
        cphnsw_mi355x.CPIndex(24, 4, devices=[0, 0], partition=True, metric="ip")


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("cosine_host")), "cosine_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_normalize_rows_host_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases as above, through the stand-alone program: exact-size buffers, every output byte compared there."""
    path = os.path.join(str(tmp_path), "cases.bin")
    todo = [case_rows(n, dim) for n, dim in cases()]
    todo += [x for dim in (1, 3, 64, 65, 130) for _, _, x in bad_cases(dim)]
    with open(path, "wb") as f:
        f.write(np.uint64(len(todo)).tobytes())
        for x in todo:
            want, bad, first = normalize_model(x)
            f.write(np.array([x.shape[0], x.shape[1], bad, first], np.uint64).tobytes())
            f.write(x.tobytes())
            f.write(want.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"cosine: ok ({len(todo)} cases)" in r.stdout


@pytest.fixture(scope="module")
def files_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("cosine_files")), "cosine_files_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "cosine_host", "cosine_files.cpp"), "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_native_file_metric_record_under_asan_ubsan(files_exe, tmp_path):
    """Format 4: an L2 index keeps the bytes of the older writer (also against a file an older library wrote: the g16
    1-bit fixture with the row map (7 i + 3) mod n); a cosine index adds a record that older readers refuse, reads back
    with its metric, and is refused by a caller that holds L2 rows."""
    import gzip
    from golden_util import fixture_path
    parent = tmp_path / "parent_native_f2.cphn"
    with gzip.open(os.path.join(HERE, "golden", "remove_g16_b1_parent_native_f2.cphn.gz"), "rb") as f:
        parent.write_bytes(f.read())
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([files_exe, fixture_path("g16", 1), str(parent), str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "cosine files: ok" in r.stdout
