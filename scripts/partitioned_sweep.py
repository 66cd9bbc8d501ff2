"""Partitioned index sweep: Gaussian 1M x 128, 4-bit, P in {1, 2, 4, 8} parts on as many GPUs as the box has (part p on
device p % gpus), one process.  Per P: build time (build + finalize), QPS of 10,000-query numpy batches at k = 10,
deduplicated recall@10 against exact=True of the same index (the exact global top-k), and the merge kernel's share of
the call (merge_us of last_search_stats against the wall time of the call).
    python scripts/partitioned_sweep.py [--n 1000000] [--nq 10000] [--parts 1,2,4,8] [--reps 3] [--out profiles/partitioned.md]
P = 1 is a partitioned index of one part: the same path (search on the device, merge, one copy out), so the lines compare
like with like."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))


def recall_dedup(ids, truth):
    """Mean over the queries of |unique returned ids that are in the truth row| / k (duplicate slots count once)."""
    hit = 0
    for r, t in zip(ids, truth):
        hit += len(set(r[r >= 0].tolist()) & set(t[t >= 0].tolist()))
    return hit / truth.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--parts", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partitioned.md"))
    args = ap.parse_args()

    import torch
    import cphnsw_mi355x
    gpus = max(1, torch.cuda.device_count())
    rng = np.random.default_rng(1)
    X = rng.standard_normal((args.n, args.dim)).astype(np.float32)
    Q = rng.standard_normal((args.nq, args.dim)).astype(np.float32)
    rows = []
    for P in [int(p) for p in args.parts.split(",")]:
        devices = [p % gpus for p in range(P)]
        ix = cphnsw_mi355x.CPIndex(args.dim, args.bits, devices=devices, partition=True)
        t0 = time.perf_counter()
        ix.build(X)
        ix.finalize()
        build_s = time.perf_counter() - t0
        ix.search_batch(Q, args.k)                                  # warm-up: scratch, adaptive capacity
        best, merge_us = float("inf"), 0
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ids, _ = ix.search_batch(Q, args.k)
            dt = time.perf_counter() - t0
            if dt < best:
                best, merge_us = dt, ix.last_search_stats()["merge_us"]
        truth, _ = ix.search_batch(Q, args.k, exact=True)
        row = {"parts": P, "devices": devices, "build_s": round(build_s, 2), "qps": round(args.nq / best),
               "recall_at_k_dedup": round(recall_dedup(ids, truth), 4), "merge_us": int(merge_us),
               "merge_share": round(merge_us / (best * 1e6), 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ix
    with open(args.out, "w") as f:
        f.write("# Partitioned index: %d x %d Gaussian, %d-bit, %d queries, k = %d, %d GPU(s)\n\n" %
                (args.n, args.dim, args.bits, args.nq, args.k, gpus))
        f.write("Written by scripts/partitioned_sweep.py.  QPS: best of %d numpy batches (host arrays in, host arrays out).  "
                "Recall: deduplicated, against exact=True of the same index.  Merge share: merge kernel device time / wall "
                "time of the call.\n\n" % args.reps)
        f.write("| parts | devices | build s | QPS | recall@%d | merge us | merge share |\n|---|---|---|---|---|---|---|\n" % args.k)
        for r in rows:
            f.write("| %d | %s | %.2f | %d | %.4f | %d | %.2f %% |\n" %
                    (r["parts"], ",".join(map(str, r["devices"])), r["build_s"], r["qps"], r["recall_at_k_dedup"], r["merge_us"],
                     100 * r["merge_share"]))


if __name__ == "__main__":
    main()
