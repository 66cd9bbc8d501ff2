"""Label filters against the path that existed before them, in one process on one GPU: n = 1M rows (16 dimensions,
1 bit: the filters never look at the vectors), labels uniform over 1,024 values, m in {1, 16, 256, 1024} filters.
    (a) the loop users wrote so far:  [index.make_filter(labels == v) for v in values]   (mask, pack and count on the
        host, one upload per filter)
    (b) index.label_filters(values)                                                      (one device pass)
Wall clock with synchronize() on both sides, the median of --reps runs after a warm-up; every filter is closed outside
the timed window.  The kernel figure is the device time of the pass (HIP events on the handle's stream,
last_label_filters_us) against the traffic no implementation can avoid, 4 n + m n / 8 bytes, at the 8 TB/s HBM peak.
(b) is checked against (a) bit for bit before anything is timed.
    python scripts/label_filter_sweep.py [--n 1000000] [--reps 7] [--out profiles/label_filters.md]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_filters.md"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    import cphnsw_mi355x
    n, dim = args.n, 16
    rng = np.random.default_rng(5)
    ix = cphnsw_mi355x.CPIndex(dim, 1, device=0)
    t0 = time.perf_counter()
    ix.build(rng.standard_normal((n, dim)).astype(np.float32))
    ix.finalize()
    print(f"built {n} x {dim} in {time.perf_counter() - t0:.1f} s", flush=True)
    labels = rng.integers(0, N_VALUES, n).astype(np.int32)
    ix.set_labels(labels, ids="internal")
    ix.time_label_filters(True)

    def old_path(values):
        return [ix.make_filter(labels == v, ids="internal") for v in values]

    def new_path(values):
        return ix.label_filters(values)

    def timed(make, values):
        ix.synchronize()
        t = time.perf_counter()
        fs = make(values)
        ix.synchronize()
        dt = time.perf_counter() - t
        us = ix.last_label_filters_us() if make is new_path else None
        for f in fs:
            f.close()
        return dt, us

    rows = []
    for m in (1, 16, 256, 1024):
        values = rng.permutation(N_VALUES)[:m].astype(np.int32)
        a, b = old_path(values[:4]), new_path(values[:4])      # the same bits before anything is timed
        for fa, fb in zip(a, b):
            assert np.array_equal(fa.words(), fb.words()) and fa.count == fb.count
        for f in a + b:
            f.close()
        old_reps = args.reps if m <= 256 else 5                 # (the host loop at m = 1024 takes seconds per run)
        timed(old_path, values[:min(m, 16)])
        timed(new_path, values)
        told = [timed(old_path, values)[0] for _ in range(old_reps)]
        new = [timed(new_path, values) for _ in range(args.reps)]
        tnew = [x[0] for x in new]
        kus = float(np.median([x[1] for x in new]))
        floor_bytes = 4 * n + m * n // 8
        row = dict(m=m, make_filter_loop_ms=round(float(np.median(told)) * 1e3, 3), loop_min_ms=round(min(told) * 1e3, 3),
                   loop_max_ms=round(max(told) * 1e3, 3), label_filters_ms=round(float(np.median(tnew)) * 1e3, 3),
                   new_min_ms=round(min(tnew) * 1e3, 3), new_max_ms=round(max(tnew) * 1e3, 3),
                   speedup=round(float(np.median(told)) / float(np.median(tnew)), 1), kernel_us=round(kus, 1),
                   floor_bytes=floor_bytes, floor_us_at_hbm_peak=round(floor_bytes / HBM_PEAK * 1e6, 2),
                   kernel_share_of_hbm_peak=round(floor_bytes / HBM_PEAK * 1e6 / kus, 3))
        print(json.dumps(row), flush=True)
        rows.append(row)

    cols = list(rows[0])
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    with open(args.out, "w") as fh:
        fh.write(f"# Label filters: n = {n:,} rows, labels uniform over {N_VALUES:,} values, one MI355X\n\n"
                 "`make filter loop`: `[index.make_filter(labels == v) for v in values]`, the path before label filters "
                 "(numpy mask, pack and count on the host, one upload per filter).  `label filters`: "
                 "`index.label_filters(values)`, one device pass.  Wall clock, synchronize() on both sides, median of "
                 f"{args.reps} runs (the loop at m = 1,024: 5) after a warm-up, min and max beside it.  `kernel us`: device "
                 "time of the pass from HIP events (median); `floor`: 4 n + m n / 8 bytes, at the 8 TB/s HBM peak.\n\n"
                 + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
