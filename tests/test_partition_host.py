"""The host-only half of the partitioned index (CPU build only).

cph_host_part_bounds must cut like dist.shard_bounds, which is how the Python side and the documents state the partition.

tests/partitioned_host/part_host.cpp includes csrc/partitioned.h (the part bounds, the cut of a global allowed-row bitmap
into one bitmap per part, and the fan-out that runs one callable on every part at once on the replica worker pool) and
drives it with a stand-in part: every part runs exactly once on its own worker, a part that fails and a part that throws
reach the caller with the status and message of the lowest-numbered one only after every part has finished, several
callers share the workers, and the mask cut is compared bit by bit at bounds that are not multiples of 32 on an input
vector with no spare word behind it.  The copy between two devices without peer access must synchronise the part's
stream before its blocking copy reads the source (a stand-in stream that is still writing: a race report otherwise), and
a thread started inside a builder's share of the host threads -- by run_threads, or a bare std::thread that adopts the
share as builder_pipeline.h does -- sees the divided count.  It is built twice with plain g++, under -fsanitize=address,undefined and under
-fsanitize=thread, and the binaries are run directly; a sanitizer report makes them exit non-zero."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "partitioned_host", "part_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"]
SANITIZERS = {
    "tsan": ["-fsanitize=thread"],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("P", [1, 3, 16])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 6001])
def test_part_bounds_equal_shard_bounds(n, P):
    from cphnsw_mi355x import _lib, dist
    out = np.full(P + 1, 2**63, np.uint64)
    _lib.check(_lib.lib().cph_host_part_bounds(n, P, out.ctypes.data))
    for p in range(P):
        assert (int(out[p]), int(out[p + 1])) == dist.shard_bounds(n, P, p), (n, P, p)


def test_part_bounds_refuses_bad_part_counts():
    from cphnsw_mi355x import _lib
    out = np.zeros(32, np.uint64)
    for P in (0, 17):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().cph_host_part_bounds(100, P, out.ctypes.data))
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().cph_host_part_bounds(100, 2, None))


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_partition_policy_under_sanitizer(tmp_path, san):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/partitioned_host/part_host.cpp"
    exe = str(tmp_path / f"part_host_{san}")
    r = subprocess.run([cxx] + COMMON + SANITIZERS[san] + [SRC, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    for part in ("bounds", "mask_cut", "fan_out", "errors", "concurrent", "copy_order", "thread_share", "part_host"):
        assert f"{part}: ok" in r.stdout, r.stdout


def test_partition_needs_devices():
    """Argument checks that need no GPU: they fire before any handle is created."""
    import cphnsw_mi355x
    with pytest.raises(ValueError, match="partition=True needs devices"):
        cphnsw_mi355x.CPIndex(128, 4, partition=True)
    with pytest.raises(ValueError, match="partition=True needs devices"):
        cphnsw_mi355x.CPIndex(128, 4, device=0, partition=True)
    with pytest.raises(ValueError):
        cphnsw_mi355x.CPIndex(128, 4, device=0, devices=[0, 0], partition=True)
    out = C.c_void_p()
    from cphnsw_mi355x import _lib
    with pytest.raises(ValueError, match="n_dev must be 1..16"):
        _lib.check(_lib.lib().cph_parts_create(128, 4, (C.c_int * 17)(*([0] * 17)), 17, C.byref(out)))
    assert not out.value
