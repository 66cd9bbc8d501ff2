"""Filter algebra against the host loop it replaces, in one process on one GPU: n = 1M rows (16 dimensions, 1 bit: the
filters never look at the vectors), labels uniform over 1,024 values, one common mask that allows half the rows,
m in {1, 16, 256, 1024} tenant filters from index.label_filters(values).
    (a) the loop users wrote so far:  [index.make_filter(unpack(f.words()) & mask) for f in tenant_filters]   (one D2H, a
        numpy AND, pack and count on the host and one H2D per filter)
    (b) index.combine_filters("and", tenant_filters, mask_filter)                                           (one device pass)
Both start from the same tenant filters, made outside the timed window; the label pass that makes them is timed beside
them (HIP events, last_label_filters_us), so the table shows what the extra streaming pass costs as a fraction of it.
Wall clock with synchronize() on both sides, the median of --reps runs after a warm-up; every filter made is closed
outside the timed window.  The kernel figure is the device time of the pass from the HIP events of
cph_filter_combine_hook (the memset of the counts and the kernel; median of --reps after a warm-up) on random words, for
the broadcast and for the per-filter second operand, against the bytes the pass must move, 2 m nw 4 + nw 4 and 3 m nw 4,
at the 8 TB/s HBM peak.  (b) is checked against (a) bit for bit before anything is timed.
    python scripts/filter_algebra_sweep.py [--n 1000000] [--reps 7] [--out profiles/filter_algebra.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))

HBM_PEAK = 8.0e12      # bytes / s (MI355X specification)
N_VALUES = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_algebra.md"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    import ctypes as C

    import cphnsw_mi355x
    from cphnsw_mi355x import _lib
    n, dim = args.n, 16
    nw = (n + 31) // 32
    rng = np.random.default_rng(5)
    ix = cphnsw_mi355x.CPIndex(dim, 1, device=0)
    t0 = time.perf_counter()
    ix.build(rng.standard_normal((n, dim)).astype(np.float32))
    ix.finalize()
    print(f"built {n} x {dim} in {time.perf_counter() - t0:.1f} s", flush=True)
    labels = rng.integers(0, N_VALUES, n).astype(np.int32)
    mask = rng.random(n) < 0.5
    ix.set_labels(labels, ids="internal")
    ix.time_label_filters(True)
    mask_filter = ix.make_filter(mask, ids="internal")

    def unpack(words):
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)

    def old_path(tenant):
        return [ix.make_filter(unpack(f.words()) & mask, ids="internal") for f in tenant]

    def new_path(tenant):
        return ix.combine_filters("and", tenant, mask_filter)

    def timed(make, tenant):
        ix.synchronize()
        t = time.perf_counter()
        fs = make(tenant)
        ix.synchronize()
        dt = time.perf_counter() - t
        for f in fs:
            f.close()
        return dt

    def kernel_us(m, broadcast):
        a = rng.integers(0, 2 ** 32, (m, nw), dtype=np.uint64).astype(np.uint32)
        b = a[:1].copy() if broadcast else a[::-1].copy()
        words, counts, us = np.empty((m, nw), np.uint32), np.empty(m, np.uint64), C.c_double(0)
        out = []
        for _ in range(args.reps + 1):                       # (the first run is the warm-up)
            _lib.check(_lib.lib().cph_filter_combine_hook(0, 0, a.ctypes.data, b.ctypes.data, int(broadcast), n, m, words.ctypes.data,
                                                          counts.ctypes.data, C.byref(us)))
            out.append(us.value)
        assert np.array_equal(words[m - 1], a[m - 1] & b[0 if broadcast else m - 1])
        return float(np.median(out[1:]))

    rows = []
    for m in (1, 16, 256, 1024):
        values = rng.permutation(N_VALUES)[:m].astype(np.int32)
        tenant = ix.label_filters(values)
        label_us = ix.last_label_filters_us()
        a, b = old_path(tenant[:4]), new_path(tenant[:4])      # the same bits before anything is timed
        for fa, fb in zip(a, b):
            assert np.array_equal(fa.words(), fb.words()) and fa.count == fb.count
        for f in a + b:
            f.close()
        old_reps = args.reps if m <= 256 else 5                 # (the host loop at m = 1024 takes seconds per run)
        timed(old_path, tenant[:min(m, 16)])
        timed(new_path, tenant)
        told = [timed(old_path, tenant) for _ in range(old_reps)]
        tnew = [timed(new_path, tenant) for _ in range(args.reps)]
        for f in tenant:
            f.close()
        k_bc, k_per = kernel_us(m, True), kernel_us(m, False)
        floor_bc, floor_per = 2 * m * nw * 4 + nw * 4, 3 * m * nw * 4
        row = dict(m=m, host_loop_ms=round(float(np.median(told)) * 1e3, 3), loop_min_ms=round(min(told) * 1e3, 3),
                   loop_max_ms=round(max(told) * 1e3, 3), combine_filters_ms=round(float(np.median(tnew)) * 1e3, 3),
                   new_min_ms=round(min(tnew) * 1e3, 3), new_max_ms=round(max(tnew) * 1e3, 3),
                   speedup=round(float(np.median(told)) / float(np.median(tnew)), 1),
                   kernel_us_broadcast=round(k_bc, 1), floor_bytes_broadcast=floor_bc,
                   floor_us_broadcast=round(floor_bc / HBM_PEAK * 1e6, 2), share_of_hbm_peak_broadcast=round(floor_bc / HBM_PEAK * 1e6 / k_bc, 3),
                   kernel_us_per_filter=round(k_per, 1), floor_bytes_per_filter=floor_per,
                   floor_us_per_filter=round(floor_per / HBM_PEAK * 1e6, 2), share_of_hbm_peak_per_filter=round(floor_per / HBM_PEAK * 1e6 / k_per, 3),
                   label_pass_kernel_us=round(label_us, 1), combine_as_fraction_of_label_pass=round(k_bc / label_us, 3))
        print(json.dumps(row), flush=True)
        rows.append(row)

    cols = list(rows[0])
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    with open(args.out, "w") as fh:
        fh.write(f"# Filter algebra: n = {n:,} rows, labels uniform over {N_VALUES:,} values, a mask that allows half the rows, one MI355X\n\n"
                 "`host loop`: `[index.make_filter(unpack(f.words()) & mask) for f in tenant_filters]`, the path before the "
                 "filter algebra (one download, a numpy AND, pack and count on the host, one upload per filter).  `combine "
                 "filters`: `index.combine_filters(\"and\", tenant_filters, mask_filter)`, one device pass.  Both start from "
                 "the same `index.label_filters(values)`.  Wall clock, synchronize() on both sides, median of "
                 f"{args.reps} runs (the loop at m = 1,024: 5) after a warm-up, min and max beside it.  `kernel us`: device time "
                 "of the pass (the memset of the counts and the kernel) from the HIP events of `cph_filter_combine_hook` on "
                 "random words (median), `broadcast`: one second operand for all m, `per filter`: m of them; `floor`: "
                 "2 m nw 4 + nw 4 and 3 m nw 4 bytes, at the 8 TB/s HBM peak.  `label pass kernel us`: the device time of the "
                 "`label_filters` pass that made the m tenant filters.\n\n"
                 + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
