"""Range search against the exact top-k call at the C2 shape (1M x 128, 4-bit, 10,000-query device batches), in one
process: range_search_device next to search_batch_device(exact=True, k=64) on the same index, queries and filter,
alternating, warm; median and spread of --reps runs each, host clock around calls that end in a device synchronise.
Radii: one scalar per target, the quantile of a query sample's exact distances at which the MEAN number of hits is about
10, 100 and 1,000; the measured mean / max hits are reported.  Filters: none, and a random 1 % mask.
The exact call does the same FMA work once, the range search twice (count pass, fill pass), so the expectation at few hits
is a ratio near 2.
    python scripts/range_sweep.py [--reps 7] [--nq 10000] [--out profiles/range_search.md]
    python scripts/range_sweep.py --only "none/1000" --reps 3 --no-write      # one case, for a kernel trace of its own
Reuses bench.py's data generators (config c2); the index is built in the process.  The report is the table and the JSON
lines; whatever the output file holds from the line KEEP on (the hand-written reading of the numbers and of the kernel
traces) is carried over to the new file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))

import bench  # noqa: E402

TARGETS = (10, 100, 1000)
K_REF = 64
KEEP = "<!-- below this line: written by hand, kept by scripts/range_sweep.py -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--n", type=int, default=0, help="override the index size (rehearsals)")
    ap.add_argument("--only", default="", help="filter/target of the one case to run, e.g. none/1000")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_search.md"))
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n, dim, nq = args.n or cfg["n"], cfg["dim"], args.nq

    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("range_sweep.py measures on the GPU: no HIP device here")
    X = bench.make_base(cfg, n)
    Q = bench.make_queries(cfg, n, nq)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    t0 = time.time()
    ix.build(X)
    ix.finalize()
    print(f"built n={n} in {time.time() - t0:.1f} s", flush=True)
    del X
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    masks = [("none", None), ("random 1 %", np.random.default_rng(7).random(n) < 0.01)]

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ix.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    rows = []
    for fname, mask in masks:
        f = None if mask is None else ix.make_filter(mask)
        m = n if mask is None else int(mask.sum())
        # radii from a sample: pooled exact distances of 512 queries, the quantile that gives the target mean
        ns = min(512, nq)
        kk = min(1024, m)
        _, sd = ix.search_batch_device(Qd[:ns], kk, filter=f, exact=True)
        ix.synchronize()
        pooled = np.sort(sd.cpu().numpy().ravel())
        for target in TARGETS:
            if args.only and args.only != f"{fname.split()[0]}/{target}":
                continue
            radius = float(pooled[min(len(pooled) - 1, target * ns)])
            run_range = lambda: ix.range_search_device(Qd, radius, filter=f)                         # noqa: E731
            run_exact = lambda: ix.search_batch_device(Qd, K_REF, filter=f, exact=True)              # noqa: E731
            for _ in range(2):                                                                       # warm, both
                timed(run_range)
                timed(run_exact)
            tr, tx = [], []
            for _ in range(args.reps):                                                               # alternating
                dt, (lims, ids, d) = timed(run_range)
                tr.append(dt)
                dt, _ = timed(run_exact)
                tx.append(dt)
            hits = np.diff(lims.numpy())
            row = dict(filter=fname, candidates=m, queries=nq, target_mean_hits=target, radius=round(radius, 3),
                       mean_hits=round(float(hits.mean()), 1), max_hits=int(hits.max()), total_hits=int(hits.sum()),
                       range_ms_median=round(float(np.median(tr)) * 1e3, 2), range_ms_min=round(min(tr) * 1e3, 2),
                       range_ms_max=round(max(tr) * 1e3, 2), exact_k64_ms_median=round(float(np.median(tx)) * 1e3, 2),
                       exact_k64_ms_min=round(min(tx) * 1e3, 2), exact_k64_ms_max=round(max(tx) * 1e3, 2), reps=args.reps)
            row["ratio_of_medians"] = round(row["range_ms_median"] / row["exact_k64_ms_median"], 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del f
    if not args.no_write:
        write_report(rows, cfg, n, dim, nq, args.reps, args.out)


def write_report(rows, cfg, n, dim, nq, reps, out):
    cols = ["filter", "candidates", "queries", "target_mean_hits", "radius", "mean_hits", "max_hits", "range_ms_median",
            "range_ms_min", "range_ms_max", "exact_k64_ms_median", "exact_k64_ms_min", "exact_k64_ms_max", "ratio_of_medians"]
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    head = (f"# Range search: range_search_device against search_batch_device(exact=True, k={K_REF})\n\n"
            f"{cfg['label']}: {n:,} x {dim}, {cfg['bits']}-bit, batches of {nq:,} queries on the device, one process, the two "
            f"calls alternating, warm; median / min / max of {reps} runs each (host clock around calls that end in a "
            "device synchronise; the range call includes its two host waits, the allocation of the result tensors and the "
            "copy of lims).  scripts/range_sweep.py.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    old = open(out).read() if os.path.exists(out) else ""
    kept = old[old.index(KEEP):] if KEEP in old else KEEP + "\n"
    with open(out, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
