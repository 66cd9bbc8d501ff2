"""Tag filters against the host loop they replace and against the label pass, in one process on one GPU: n = 1M rows (16
dimensions, 1 bit: the filters never look at the vectors), 0 to 32 tags per row (8 on average) drawn with a skew from a
1,024-tag vocabulary, m in {1, 16, 256, 1024} `any` tests of one value and of 16 values.
    (a) the loop a caller with tags_of_row writes today: per test np.isin over the CSR, np.logical_or.reduceat, make_filter
        (mask, pack and count on the host, one upload per filter)
    (b) index.tag_filters(name, tests)                                          (one device pass)
    (c) index.label_filters(values) at the same n and m: the yardstick for the instruction stream
Wall clock with synchronize() on both sides, the median of --reps runs after a warm-up (the host loop: fewer runs at
m >= 256, where one run takes many seconds; the count is in the table); every filter is closed outside the timed window.
`kernel us` is the device time of the pass (HIP events on the handle's stream, the median of --reps) against the traffic no
implementation can avoid, 4 (n + 1) + 4 nnz + m n / 8 bytes, at the 8 TB/s HBM peak.  (b) is checked against (a) bit for
bit before anything is timed.
    python scripts/tag_filter_sweep.py [--n 1000000] [--reps 7] [--out profiles/tag_filters.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))

HBM_PEAK = 8.0e12      # bytes / s (MI355X specification)
VOCAB = 1024


def make_column(n, rng):
    """A caller's column: row lengths 0..32 (binomial, mean 8) and a Zipf-like draw over the vocabulary, duplicates and
    all -- set_tags makes it canonical (the mean drops a little where a row drew a frequent tag twice)."""
    lens = rng.binomial(32, 0.25, n)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    lims = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=lims[1:])
    return lims, rng.choice(VOCAB, int(lims[-1]), p=p).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tag_filters.md"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    import cphnsw_mi355x
    n, dim = args.n, 16
    rng = np.random.default_rng(6)
    ix = cphnsw_mi355x.CPIndex(dim, 1, device=0)
    t0 = time.perf_counter()
    ix.build(rng.standard_normal((n, dim)).astype(np.float32))
    ix.finalize()
    print(f"built {n} x {dim} in {time.perf_counter() - t0:.1f} s", flush=True)
    ix.set_tags("t", *make_column(n, rng)[::-1], ids="internal")
    lims, tags = ix.tags("t", ids="internal")             # the canonical column: what both sides evaluate
    nnz = int(lims[-1])
    labels = rng.integers(0, VOCAB, n).astype(np.int32)
    ix.set_labels(labels, ids="internal")
    ix.time_tag_filters(True)
    ix.time_label_filters(True)
    full = np.diff(lims) > 0
    starts = lims[:-1][full]
    print(f"column: nnz = {nnz}, mean {nnz / n:.2f} tags per row, longest {int(np.diff(lims).max())}", flush=True)

    def host_loop(tests):
        out = []
        for v in tests:
            mask = np.zeros(n, bool)
            mask[full] = np.logical_or.reduceat(np.isin(tags, v), starts)
            out.append(ix.make_filter(mask, ids="internal"))
        return out

    def device(tests):
        return ix.tag_filters("t", tests)

    def label_pass(tests):
        return ix.label_filters(np.array([t[0] for t in tests], np.int32))

    def timed(make, tests):
        ix.synchronize()
        t = time.perf_counter()
        fs = make(tests)
        ix.synchronize()
        dt = time.perf_counter() - t
        us = ix.last_tag_filters_us() if make is device else ix.last_label_filters_us() if make is label_pass else None
        for f in fs:
            f.close()
        return dt, us

    rows = []
    for width in (1, 16):
        for m in (1, 16, 256, 1024):
            tests = [rng.choice(VOCAB, width, replace=False).astype(np.int32) for _ in range(m)]
            a, b = host_loop(tests[:4]), device(tests[:4])      # the same bits before anything is timed
            for fa, fb in zip(a, b):
                assert np.array_equal(fa.words(), fb.words()) and fa.count == fb.count
            for f in a + b:
                f.close()
            loop_reps = args.reps if m <= 16 else 3 if m <= 256 else 1
            timed(device, tests)
            timed(label_pass, tests)
            told = [timed(host_loop, tests)[0] for _ in range(loop_reps)]
            new = [timed(device, tests) for _ in range(args.reps)]
            lab = [timed(label_pass, tests) for _ in range(args.reps)]
            tnew = [x[0] for x in new]
            kus, lus = float(np.median([x[1] for x in new])), float(np.median([x[1] for x in lab]))
            floor_bytes = 4 * (n + 1) + 4 * nnz + m * n // 8
            row = dict(values_per_test=width, m=m, host_loop_ms=round(float(np.median(told)) * 1e3, 3), host_loop_runs=loop_reps,
                       tag_filters_ms=round(float(np.median(tnew)) * 1e3, 3), new_min_ms=round(min(tnew) * 1e3, 3),
                       new_max_ms=round(max(tnew) * 1e3, 3), speedup=round(float(np.median(told)) / float(np.median(tnew)), 1),
                       kernel_us=round(kus, 1), label_kernel_us=round(lus, 1), kernel_over_label=round(kus / lus, 2),
                       floor_bytes=floor_bytes, floor_us_at_hbm_peak=round(floor_bytes / HBM_PEAK * 1e6, 2),
                       kernel_share_of_hbm_peak=round(floor_bytes / HBM_PEAK * 1e6 / kus, 3),
                       ns_per_row_tag_and_test=round(kus * 1e3 / (nnz * m), 6))
            print(json.dumps(row), flush=True)
            rows.append(row)

    cols = list(rows[0])
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    with open(args.out, "w") as fh:
        fh.write(f"# Tag filters: n = {n:,} rows, {nnz:,} tags (0 to 32 per row, a skewed draw from {VOCAB:,}), one MI355X\n\n"
                 "`host loop`: per test `np.isin` over the CSR, `np.logical_or.reduceat`, `make_filter` -- the path before tag "
                 "columns.  `tag filters`: `index.tag_filters(name, tests)` with `any` tests of `values per test` values, one "
                 "device pass.  Wall clock, synchronize() on both sides, median after a warm-up "
                 f"({args.reps} runs; the host loop: `host loop runs`), min and max beside it.  `kernel us`: device time of the "
                 "pass from HIP events (median); `label kernel us`: the label pass at the same n and m; `floor`: "
                 "4 (n + 1) + 4 nnz + m n / 8 bytes, at the 8 TB/s HBM peak.\n\n"
                 + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
