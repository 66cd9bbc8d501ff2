"""Fused search against what a caller pays today before the host merge: 1M x 128, 4-bit, L2, device batches of
n * T = 32,000 vectors, T in {1, 4, 16} vectors per query (rewrites of one question: a query row plus noise), C in {32, 64, 128},
k = 10, weights all one, in one process.  Per (T, C): search_fused_device(k, candidates=C) next to
search_batch_device(k=C) over the same n * T rows on the same handle -- alternating, warm; median and spread of --reps runs
each, host clock around calls that end in a device synchronise -- and fused_scan_kernel alone between two HIP events
(CPIndex.time_fused / last_fused_us) against its packed-fp32 VALU floor (2 U L D flop per query at the measured union size U) and
against the bytes it gathers (U D 4 per query).
No target is fixed in advance.
    python scripts/fused_sweep.py [--reps 7] [--rows 32000] [--out profiles/fused_search.md]
Reuses bench.py's data generators (config c2); the index is built in the process.  Whatever the output file holds from the
line KEEP on (resource usage, the bench.py comparison, a hand-written reading of the numbers) is carried over."""
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

VECTORS = (1, 4, 16)
CANDIDATES = (32, 64, 128)
PEAK_VALU_FP32_TFLOPS = 157.3                              # MI355X vector fp32 (FMA), the floor's denominator
PEAK_HBM_TBS = 8.0                                         # MI355X HBM3E, the gather floor's denominator
KEEP = "<!-- below this line: written by hand, kept by scripts/fused_sweep.py -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=32_000, help="n * T, the vectors of a batch")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n", type=int, default=0, help="override the index size (rehearsals)")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_search.md"))
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n, dim, rows_, k = args.n or cfg["n"], cfg["dim"], args.rows, args.k

    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("fused_sweep.py measures on the GPU: no HIP device here")
    X = bench.make_base(cfg, n)
    Q = bench.make_queries(cfg, n, rows_)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    t0 = time.time()
    ix.build(X)
    ix.finalize()
    print(f"built n={n} in {time.time() - t0:.1f} s", flush=True)
    del X
    dev = torch.device("cuda", 0)
    ix.time_fused(True)
    rng = np.random.default_rng(1)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ix.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    rows = []
    for T in VECTORS:
        nq = rows_ // T
        base = Q[:nq][:, None, :]
        V = base if T == 1 else (base + np.float32(0.1) * np.abs(base).mean() * rng.standard_normal((nq, T, dim))).astype(np.float32)
        V = np.ascontiguousarray(V, np.float32)
        Vd = torch.from_numpy(V).to(dev)
        flat = Vd.view(nq * T, dim)
        for C_ in CANDIDATES:
            out_f = [torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                     torch.empty((nq, k), dtype=torch.int32, device=dev)]
            out_b = [torch.empty((nq * T, C_), dtype=torch.int64, device=dev), torch.empty((nq * T, C_), dtype=torch.float32, device=dev)]
            run_fused = lambda: ix.search_fused_device(Vd, k, candidates=C_, out=out_f)               # noqa: E731
            run_plain = lambda: ix.search_batch_device(flat, C_, out=out_b)                          # noqa: E731
            for _ in range(2):                                                                        # warm, both
                timed(run_fused)
                timed(run_plain)
            tf, tp, ts = [], [], []
            for _ in range(args.reps):                                                                # alternating
                dt, _ = timed(run_fused)
                tf.append(dt)
                ts.append(ix.last_fused_us())
                dt, plain = timed(run_plain)
                tp.append(dt)
            ids = plain[0].cpu().numpy().reshape(nq, T * C_)                                          # the union size, for the floors
            s = np.sort(ids, axis=1)
            U = float((((s[:, 1:] != s[:, :-1]) & (s[:, 1:] >= 0)).sum(axis=1) + (s[:, 0] >= 0)).mean())
            scan = float(np.median(ts))
            valu_us = 2.0 * U * T * dim * nq / (PEAK_VALU_FP32_TFLOPS * 1e12) * 1e6
            bytes_us = U * dim * 4 * nq / (PEAK_HBM_TBS * 1e12) * 1e6
            row = dict(vectors=T, candidates=C_, k=k, queries=nq,
                       fused_ms_median=round(float(np.median(tf)) * 1e3, 3), fused_ms_min=round(min(tf) * 1e3, 3),
                       fused_ms_max=round(max(tf) * 1e3, 3), search_ms_median=round(float(np.median(tp)) * 1e3, 3),
                       search_ms_min=round(min(tp) * 1e3, 3), search_ms_max=round(max(tp) * 1e3, 3),
                       scan_us_median=round(scan, 1), scan_us_min=round(min(ts), 1), scan_us_max=round(max(ts), 1),
                       mean_union=round(U, 1), valu_floor_us=round(valu_us, 1), gather_floor_us=round(bytes_us, 1),
                       scan_over_valu_floor=round(scan / max(valu_us, 1e-9), 2), scan_over_gather_floor=round(scan / max(bytes_us, 1e-9), 2),
                       reps=args.reps)
            row["ratio_of_medians"] = round(row["fused_ms_median"] / row["search_ms_median"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    ix.time_fused(False)
    if not args.no_write:
        write_report(rows, cfg, n, dim, rows_, k, args.reps, args.out)


def write_report(rows, cfg, n, dim, rows_, k, reps, out):
    cols = ["vectors", "candidates", "queries", "fused_ms_median", "fused_ms_min", "fused_ms_max", "search_ms_median", "search_ms_min",
            "search_ms_max", "ratio_of_medians", "scan_us_median", "scan_us_min", "scan_us_max", "mean_union", "valu_floor_us",
            "gather_floor_us", "scan_over_valu_floor", "scan_over_gather_floor"]
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    head = ("# Fused search: search_fused_device(k, candidates=C) against search_batch_device(k=C) over the same n * T rows\n\n"
            f"{cfg['label']}: {n:,} x {dim}, {cfg['bits']}-bit, metric L2, k = {k}, weights all one, every vector live, batches of "
            f"n * T = {rows_:,} vectors on the device (a query's T vectors: one query row plus noise), one process, the two calls "
            f"alternating, warm, both into preallocated outputs; median / min / max of {reps} runs each (host clock around calls that "
            "end in a device synchronise).  `search` is what the caller pays today before the host merge, and what the fused call "
            "contains.  `scan us` is fused_scan_kernel alone between two HIP events; `mean union` = U, the distinct candidates of a "
            f"query; `valu floor us` = 2 U T D flop per query at {PEAK_VALU_FP32_TFLOPS} Tflop/s, `gather floor us` = U D 4 bytes per "
            f"query at {PEAK_HBM_TBS} TB/s.  scripts/fused_sweep.py.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    old = open(out).read() if os.path.exists(out) else ""
    kept = old[old.index(KEEP):] if KEEP in old else KEEP + "\n"
    with open(out, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
