"""ctypes front-end of the filtered-search model (TEST INFRASTRUCTURE).

tests/filtered_model/filtered_search.cpp includes oracle/cph_oracle.cpp and restates its search with the result-heap
push gated by an allowed-id bitmap.  It is compiled here, once per process, with exactly the oracle's flags
(oracle/Makefile), into a temporary directory: nothing is written into the tree.
"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "filtered_model", "filtered_search.cpp")
# oracle/Makefile: CXXFLAGS (without the warnings) + the oracle rule's -ffp-contract=off -shared
FLAGS = ["-O3", "-std=c++17", "-march=x86-64-v3", "-mavx2", "-mfma", "-fopenmp", "-fPIC", "-ffp-contract=off", "-shared"]

_LIB = None


def compiler():
    return os.environ.get("CXX") or shutil.which("g++")


def build_model():
    """Path of the compiled model (built on first use)."""
    cxx = compiler()
    if cxx is None:
        raise RuntimeError("g++ not available: the filtered-search model cannot be built")
    out = os.path.join(tempfile.mkdtemp(prefix="cph_filtered_model_"), "libcph_filtered_model.so")
    r = subprocess.run([cxx] + FLAGS + [SRC, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building the filtered-search model failed:\n" + r.stderr[-4000:])
    return out


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(build_model())
        L.orc_load.restype = C.c_void_p
        L.orc_load.argtypes = [C.c_char_p]
        L.orc_free.argtypes = [C.c_void_p]
        L.orc_last_error.restype = C.c_char_p
        L.orc_search_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int]
        L.flt_search_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int]
        _LIB = L
    return _LIB


def pack_words(mask):
    """Bool mask -> uint32 words, bit (i & 31) of word i >> 5 (numpy's own little-endian bit packing)."""
    m = np.asarray(mask, dtype=bool)
    b = np.packbits(m, bitorder="little")
    b = np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)])
    return b.view("<u4").astype(np.uint32)


class ModelIndex:
    """An index file loaded into the model library (its own copy of the oracle's reader)."""

    def __init__(self, path):
        self.L = lib()
        h = self.L.orc_load(str(path).encode())
        if not h:
            raise RuntimeError(self.L.orc_last_error().decode())
        self.h = C.c_void_p(h)
        info = (C.c_long * 8)()
        self.L.orc_info.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        self.L.orc_info(self.h, info)
        self.n, self.dim = int(info[0]), int(info[1])

    def __del__(self):
        try:
            self.L.orc_free(self.h)
        except Exception:
            pass

    def _run(self, fn, queries, k, words, nthreads):
        q = np.ascontiguousarray(queries, np.float32)
        n = q.shape[0]
        ids = np.zeros((n, k), np.int64)
        d = np.zeros((n, k), np.float32)
        cnt = np.zeros(n, np.int32)
        ctr = np.zeros((n, 9), np.uint64)
        args = [self.h, q.ctypes.data, n, k]
        if words is not False:
            args.append(None if words is None else words.ctypes.data)
        rc = fn(*args, ids.ctypes.data, d.ctypes.data, cnt.ctypes.data, ctr.ctypes.data, nthreads)
        if rc != 0:
            raise RuntimeError("Search failed: invalid entry point after finalize.")
        return ids, d, cnt, ctr

    def search_batch(self, queries, k, mask=None, nthreads=0):
        """The filtered model: (ids, dist, counts, counters [n, 9]); mask None = every id allowed."""
        words = None
        if mask is not None:
            mask = np.asarray(mask, dtype=bool)
            assert mask.shape == (self.n,)
            words = np.ascontiguousarray(pack_words(mask))
        return self._run(self.L.flt_search_batch, queries, k, words, nthreads)

    def search_batch_unfiltered(self, queries, k, nthreads=0):
        """The oracle's own orc_search_batch, compiled into the same library."""
        return self._run(self.L.orc_search_batch, queries, k, False, nthreads)
