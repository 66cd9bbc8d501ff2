"""Needs an MI355X.  Facet counts against the host loop they replace, in one process on one GPU: n = 1M rows (16 dimensions,
1 bit: facets never look at the vectors), a dense column of U in {8, 1,000, 100,000} distinct values drawn uniformly and
with a Zipf skew, m in {1, 16, 256, 1,024} random filters at selectivities 1 %, 50 % and 100 %, and a tag column at about
7 tags per row.
    (a) the loop a caller writes today, per filter: f.words(), unpack, np.bincount over the masked codes of a host copy
        of the column (timed on the first min(m, 16) filters and scaled to m: `host_loop_filters` says how many ran)
    (b) index.facet(name, filter=fs)                                             (one call)
Wall clock, the median of --reps runs after a warm-up.  `kernel_us` is the device time of the call's launches (HIP events
through time_facets: the memset of the counters and the counting kernel) against the bytes no implementation of this
design can avoid, m n / 8 + 4 n ceil(m / 16) (every bitmap once, the codes once per chunk of 16 filters), at the copy rate
measured in this process (a device-to-device copy of 1 GiB: read + write bytes over its HIP-event time).  (b) is checked
against (a) before anything is timed.  A second table runs the production launcher on the same columns through
cph_facet_hook with the on-chip and the global counting path forced (m = 16, 50 %): which path wins at each U.
`--paths-only` times only the launcher, through the hook on synthetic codes, with both paths forced at U = 2,000, 4,000
and just below and at the on-chip limit (m = 16 and 256), and prints one JSON line per shape; run against diagnostic builds
(CPH_LIB_PATH, -DCPH_FACET_MIN_BLOCKS=...) it is the run-length table of profiles/facets.md.
    python scripts/facet_sweep.py [--n 1000000] [--reps 5] [--out profiles/facets.md] [--paths-only]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))

CHUNK = 16             # device_facets.h: kFacetFilterChunk


def copy_rate():
    """bytes / s of a device-to-device copy of 1 GiB (read + write), the best of five."""
    import torch
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    best = 0.0
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        best = max(best, 2 * a.numel() / (e0.elapsed_time(e1) * 1e-3))
    del a, b
    torch.cuda.empty_cache()
    return best


def draw(rng, n, U, skew):
    if not skew:
        col = rng.integers(0, U, n)
    else:
        p = 1.0 / np.arange(1, U + 1)
        col = rng.choice(U, n, p=p / p.sum())
    col[:U] = np.arange(U)                                  # every value occurs
    return (col * 3 - 7).astype(np.int32)


def unpack(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "facets.md"))
    ap.add_argument("--paths-only", action="store_true",
                    help="only time both counting paths through cph_facet_hook at U near the on-chip limit (m = 16 and 256, 50 %%)")
    args = ap.parse_args()
    rate = 0.0 if args.paths_only else copy_rate()
    print(f"copy rate {rate / 1e12:.2f} TB/s", flush=True)
    import cphnsw_mi355x
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    n, dim = args.n, 16
    rng = np.random.default_rng(6)
    if args.paths_only:                                     # the launcher alone, near the on-chip limit: no index is needed
        lim = L.cph_facet_onchip_limit()
        nw = (n + 31) // 32
        for m in (16, 256):
            words = rng.integers(0, 2 ** 32, (m, nw), dtype=np.uint64).astype(np.uint32)     # 50 % of the rows each
            for U in (2000, 4000, lim - 192, lim):
                for skew in (False, True):
                    c32 = np.unique(draw(rng, n, U, skew), return_inverse=True)[1].reshape(-1).astype(np.uint32)
                    out = np.zeros(m * U + 64, np.uint64)
                    rec = dict(lib=os.path.basename(os.environ.get("CPH_LIB_PATH", "product")), column="zipf" if skew else "uniform", U=U, m=m)
                    for label, path in (("onchip_us", 1), ("global_us", 2)):
                        us, best = C.c_double(0), []
                        for _ in range(args.reps + 1):
                            _lib.check(L.cph_facet_hook(0, c32.ctypes.data, n, None, n, U, words.ctypes.data, m, path, out.ctypes.data, C.byref(us)))
                            best.append(us.value)
                        rec[label] = round(float(np.median(best[1:])), 1)
                    print(json.dumps(rec), flush=True)
        return
    ix = cphnsw_mi355x.CPIndex(dim, 1, device=0)
    t0 = time.perf_counter()
    ix.build(rng.standard_normal((n, dim)).astype(np.float32))
    ix.finalize()
    print(f"built {n} x {dim} in {time.perf_counter() - t0:.1f} s", flush=True)
    ix.time_facets(True)
    filters = {}
    for sel in (0.01, 0.5, 1.0):
        filters[sel] = [ix.make_filter(rng.random(n) < sel if sel < 1.0 else np.ones(n, bool), ids="internal") for _ in range(CHUNK)]

    def fs_of(sel, m):                                      # m filters: the 16 distinct bitmaps of a selectivity, repeated
        return [filters[sel][j % CHUNK] for j in range(m)]

    def host_loop(codes, U, fs, lims=None):
        out = np.zeros((len(fs), U), np.int64)
        for j, f in enumerate(fs):
            mask = unpack(f.words(), n)
            if lims is not None:
                mask = np.repeat(mask, np.diff(lims))
            out[j] = np.bincount(codes[mask], minlength=U)
        return out

    def measure(name, codes, U, sel, m, lims=None):
        fs = fs_of(sel, m)
        k = min(m, CHUNK)
        want = host_loop(codes, U, fs[:k], lims)
        values, counts = ix.facet(name, filter=fs)          # (also the warm-up)
        assert len(values) == U and np.array_equal(counts[:k], want) and np.array_equal(counts[k:], want[np.arange(k, m) % CHUNK])
        told = []
        for _ in range(3 if m > 1 else args.reps):
            t = time.perf_counter()
            host_loop(codes, U, fs[:k], lims)
            told.append((time.perf_counter() - t) * m / k)
        tnew, kus = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            ix.facet(name, filter=fs)
            tnew.append(time.perf_counter() - t)
            kus.append(ix.last_facets_us())
        floor_bytes = m * n // 8 + 4 * n * ((m + CHUNK - 1) // CHUNK)
        k_us = float(np.median(kus))
        return dict(host_loop_ms=round(float(np.median(told)) * 1e3, 3), host_loop_filters=k, facet_ms=round(float(np.median(tnew)) * 1e3, 3),
                    speedup=round(float(np.median(told)) / float(np.median(tnew)), 1), kernel_us=round(k_us, 1),
                    floor_us=round(floor_bytes / rate * 1e6, 2), share_of_floor=round(floor_bytes / rate * 1e6 / k_us, 3))

    rows, paths = [], []
    lim = L.cph_facet_onchip_limit()
    for U in (8, 1000, 100000):
        for skew in (False, True):
            col = draw(rng, n, U, skew)
            ix.set_column("c", col, ids="internal")
            codes = np.unique(col, return_inverse=True)[1].reshape(-1)
            for m in (1, 16, 256, 1024):
                for sel in (0.01, 0.5, 1.0):
                    if m * U > 30_000_000 and sel != 0.5:   # (the m x U copy back dominates there: one selectivity is enough)
                        continue
                    row = dict(column="zipf" if skew else "uniform", U=U, m=m, selectivity=sel, **measure("c", codes, U, sel, m))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            words = np.stack([f.words() for f in filters[0.5]])
            c32 = np.ascontiguousarray(codes, np.uint32)
            out = np.zeros(CHUNK * U + 64, np.uint64)
            rec = dict(column="zipf" if skew else "uniform", U=U)
            for label, path in (("onchip_us", 1), ("global_us", 2)):
                if path == 1 and U > lim:
                    rec[label] = None
                    continue
                us, best = C.c_double(0), []
                for _ in range(args.reps + 1):
                    _lib.check(L.cph_facet_hook(0, c32.ctypes.data, n, None, n, U, words.ctypes.data, CHUNK, path, out.ctypes.data, C.byref(us)))
                    best.append(us.value)
                rec[label] = round(float(np.median(best[1:])), 1)
            print(json.dumps(rec), flush=True)
            paths.append(rec)
    ix.set_column("c", None)
    lens = rng.binomial(28, 0.25, n)
    lims = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=lims[1:])
    p = 1.0 / np.arange(1, 1025)
    ix.set_tags("t", rng.choice(1024, int(lims[-1]), p=p / p.sum()).astype(np.int32), lims=lims, ids="internal")
    tl, tv = ix.tags("t", ids="internal")
    tvals, tcodes = np.unique(tv, return_inverse=True)
    for m in (1, 16, 256):
        row = dict(column=f"tags ({len(tv) / n:.2f} per row)", U=len(tvals), m=m, selectivity=0.5,
                   **measure("t", tcodes.reshape(-1), len(tvals), 0.5, m, lims=tl))
        print(json.dumps(row), flush=True)
        rows.append(row)

    def table(recs):
        cols = list(recs[0])
        lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
        for r in recs:
            lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
        return "\n".join(lines)

    with open(args.out, "w") as fh:
        fh.write(f"# Facet counts: n = {n:,} rows, one MI355X\n\n"
                 "`host loop`: per filter `words()`, unpack, `np.bincount` over the masked codes (timed on `host loop filters` "
                 "filters, scaled to m).  `facet`: `index.facet(name, filter=fs)`, one call, wall clock, median of "
                 f"{args.reps} after a warm-up.  `kernel us`: HIP events around the call's launches.  `floor us`: "
                 f"m n / 8 + 4 n ceil(m / 16) bytes at the copy rate measured here, {rate / 1e12:.2f} TB/s.\n\n"
                 + table(rows) + f"\n\n## Counting paths (cph_facet_hook, m = 16, 50 %; on-chip limit {lim:,} values)\n\n" + table(paths)
                 + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows + paths) + "\n```\n")
    print(table(rows))
    print(table(paths))


if __name__ == "__main__":
    main()
