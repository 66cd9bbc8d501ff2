"""Filtered search at the C2 shape (1M x 128, 4-bit, 10k queries, k = 10): throughput, work, re-runs, recall and parity
per filter -- unfiltered, all ones, random at 0.5 / 0.1 / 0.01, and a clustered 10 % filter (a contiguous internal-id
range).  Reuses bench.py's data generators and its cached index file (same --workdir).
    python scripts/filtered_sweep.py [--workdir DIR] [--reps 5] [--parity-queries 100] [--out profiles/filtered_sweep.md]
Recall@10 is measured against the filtered ground truth (exact k-NN over the allowed rows, bench.recall_at_10: by
distance, tie-safe); parity = ids and distance bytes equal to the model of the filtered search
(tests/filtered_model/filtered_search.cpp) on the first --parity-queries queries."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=os.environ.get("CPH_BENCH_DIR", "/tmp/cph_bench"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parity-queries", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_sweep.md"))
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, nq, k = cfg["n"], cfg["nq"], cfg["k"]

    import torch
    import cphnsw_mi355x
    from filtered_model_lib import ModelIndex
    path, info, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    Q = bench.make_queries(cfg, n, nq)
    ix = cphnsw_mi355x.CPIndex(cfg["dim"], cfg["bits"], device=0)
    if os.path.exists(path + ".native"):
        ix.load_native(path + ".native")
    else:
        ix.load(path)
    Xi = ix.get_vectors()                           # internal order: the filters and the ground truth speak internal ids
    rng = np.random.default_rng(7)
    filters = [("unfiltered", None), ("all ones", np.ones(n, bool))]
    for p in (0.5, 0.1, 0.01):
        filters.append((f"random {p}", rng.random(n) < p))
    clustered = np.zeros(n, bool)
    clustered[int(0.45 * n):int(0.55 * n)] = True
    filters.append(("clustered 10 % (ids 450k-550k)", clustered))

    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    mi = ModelIndex(path)
    gt_all = bench.ground_truth(Xi, Q, 0)
    rows = []
    for name, mask in filters:
        f = None if mask is None else ix.make_filter(mask)
        # host batch: median of reps
        ix.search_batch(Q, k, filter=f)
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ids, d = ix.search_batch(Q, k, filter=f)
            t.append(time.perf_counter() - t0)
        st = ix.last_search_stats()
        qps_host = nq / float(np.median(t))
        # device batches, alternately on two streams, as bench.py's steps
        torch.cuda.synchronize()
        for i in range(2):
            ix.search_batch_device(Qd, k, stream=streams[i & 1], filter=f)
        ix.synchronize()
        t0 = time.perf_counter()
        for i in range(args.reps * 2):
            streams[i & 1].wait_stream(torch.cuda.current_stream(dev))
            ix.search_batch_device(Qd, k, stream=streams[i & 1], filter=f)
        ix.synchronize()
        qps_dev = nq * args.reps * 2 / (time.perf_counter() - t0)
        # recall@10 against the exact neighbours among the allowed rows
        if mask is None:
            gt_d = gt_all
        else:
            gt_d = bench.ground_truth(Xi[mask], Q, 0)
        rec = bench.recall_at_10(ids, d, gt_d, dedup=False)
        # parity with the model on a bounded sample
        m = args.parity_queries
        mids, md, _, _ = mi.search_batch(Q[:m], k, mask, nthreads=16)
        parity = bool(np.array_equal(ids[:m], mids) and d[:m].tobytes() == md.tobytes())
        row = dict(filter=name, allowed=int(n if mask is None else mask.sum()), qps_search_batch=round(qps_host),
                   qps_search_batch_device=round(qps_dev), expansions_per_query=round(st["expansions"] / nq, 1),
                   rerun_queries=st["rerun_queries"], kernel_us=st["kernel_us"], recall_at_10=round(rec, 4),
                   parity_queries=m, parity=parity)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del f
    hdr = ("| filter | allowed ids | QPS search_batch | QPS search_batch_device | expansions / query | re-run queries | "
           "kernel us (last batch) | recall@10 (filtered GT) | parity (first %d queries) |" % args.parity_queries)
    lines = [hdr, "|" + "---|" * 9]
    for r in rows:
        lines.append(f"| {r['filter']} | {r['allowed']:,} | {r['qps_search_batch']:,} | {r['qps_search_batch_device']:,} | "
                     f"{r['expansions_per_query']} | {r['rerun_queries']} | {r['kernel_us']:,} | {r['recall_at_10']} | "
                     f"{'equal' if r['parity'] else 'DIFFERENT'} |")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
