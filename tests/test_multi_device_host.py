"""The host-only half of the multi-device index under sanitizers (CPU build only).

tests/multi_device_host/multi_host.cpp includes csrc/multi_device.h (the query split and the replica worker pool of
cph_multi_search_batch) and drives it with a stand-in launch that sleeps for random times and writes rows.  It is built
twice with plain g++, under -fsanitize=thread and under -fsanitize=address,undefined, and checks: the shard bounds
(ragged, fewer queries than replicas, min_shard), every row written exactly once by the replica of its shard, an error
of one worker reaching the caller with its message only after every worker has finished (lowest-numbered failing
replica wins), no write after return, 8 callers at once, and destroy joining the workers.  A sanitizer report makes the
binary exit non-zero."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "multi_device_host", "multi_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"]
SANITIZERS = {
    "tsan": ["-fsanitize=thread"],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_multi_device_pool_under_sanitizer(tmp_path, san):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / f"multi_host_{san}")
    r = subprocess.run([cxx] + COMMON + SANITIZERS[san] + [SRC, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    for part in ("plans", "rows", "errors", "concurrent", "destroy", "multi_host"):
        assert f"{part}: ok" in r.stdout, r.stdout
