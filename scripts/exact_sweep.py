"""Exact scan against the graph path at the C2 shape (1M x 128, 4-bit, 10k queries, k = 10), per filter, in one process:
the six filters of filtered_sweep.py plus random 0.001.  Per filter: QPS of the graph path (search_batch and
search_batch_device), QPS of the exact path (both), kernel microseconds of the exact launches, the achieved FMA rate
(nq x candidates x D / kernel time) against the fp32 VALU peak, and recall@10 by distance of both paths against
knn_bruteforce(X[allowed], Q).  From the random-filter lines: the crossover popcount, where the exact path's device
QPS equals the graph path's (log-log interpolation between the two lines that bracket it).  Reuses bench.py's data
generators and its cached index file (same --workdir).
    python scripts/exact_sweep.py [--workdir DIR] [--reps 3] [--out profiles/exact_scan.md] [--max-exact-candidates N]
Peak used: "Peak FP32 (vector) 157.3 TFLOPS (spec)" of the MI355X microarchitecture guide (its section-1 table) -- the
PACKED rate (v_pk_fma_f32: two FMAs per lane and instruction) = 78.65 T FMA/s.  The scan issues plain v_fma_f32 with a
scalar query operand, one FMA per lane and instruction: its own ceiling is half of that, 39.3 T FMA/s; both fractions
are reported."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402

PEAK_FMA = 157.3e12 / 2          # packed fp32 vector peak, in FMAs
PEAK_FMA_PLAIN = PEAK_FMA / 2    # one v_fma_f32 per lane and cycle slot: what this kernel's instruction mix can reach


def crossover(rows):
    """Popcount at which exact device QPS = graph device QPS, from the random-filter lines (None: no sign change)."""
    pts = sorted((r["allowed"], math.log(r["exact_qps_device"] / r["graph_qps_device"])) for r in rows
                 if r["filter"].startswith(("random", "all ones")) and "exact_qps_device" in r)
    for (m0, g0), (m1, g1) in zip(pts, pts[1:]):
        if g0 >= 0 > g1:
            return int(round(math.exp(math.log(m0) + (math.log(m1) - math.log(m0)) * g0 / (g0 - g1))))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=os.environ.get("CPH_BENCH_DIR", "/tmp/cph_bench"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_scan.md"))
    ap.add_argument("--max-exact-candidates", type=int, default=0, help="skip the exact path above this many allowed ids (0: never)")
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, nq, k, dim = cfg["n"], cfg["nq"], cfg["k"], cfg["dim"]

    import torch
    import cphnsw_mi355x
    path, info, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    Q = bench.make_queries(cfg, n, nq)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    if os.path.exists(path + ".native"):
        ix.load_native(path + ".native")
    else:
        ix.load(path)
    Xi = ix.get_vectors()
    rng = np.random.default_rng(7)
    filters = [("unfiltered", None), ("all ones", np.ones(n, bool))]
    for p in (0.5, 0.1, 0.01):
        filters.append((f"random {p}", rng.random(n) < p))
    clustered = np.zeros(n, bool)
    clustered[int(0.45 * n):int(0.55 * n)] = True
    filters.append(("clustered 10 % (ids 450k-550k)", clustered))
    filters.append(("random 0.001", np.random.default_rng(8).random(n) < 0.001))

    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]

    def host_qps(f, exact):
        ix.search_batch(Q, k, filter=f, exact=exact)
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ids, d = ix.search_batch(Q, k, filter=f, exact=exact)
            t.append(time.perf_counter() - t0)
        return nq / float(np.median(t)), ids, d, ix.last_search_stats()

    def dev_qps(f, exact):
        torch.cuda.synchronize()
        for i in range(2):
            ix.search_batch_device(Qd, k, stream=streams[i & 1], filter=f, exact=exact)
        ix.synchronize()
        t0 = time.perf_counter()
        for i in range(args.reps * 2):
            streams[i & 1].wait_stream(torch.cuda.current_stream(dev))
            ix.search_batch_device(Qd, k, stream=streams[i & 1], filter=f, exact=exact)
        ix.synchronize()
        return nq * args.reps * 2 / (time.perf_counter() - t0)

    rows = []
    for name, mask in filters:
        f = None if mask is None else ix.make_filter(mask)
        m = int(n if mask is None else mask.sum())
        gt_d = bench.ground_truth(Xi if mask is None else Xi[mask], Q, 0)
        g_host, g_ids, g_d, g_st = host_qps(f, False)
        g_dev = dev_qps(f, False)
        row = dict(filter=name, allowed=m, graph_qps_search_batch=round(g_host), graph_qps_device=round(g_dev),
                   graph_expansions_per_query=round(g_st["expansions"] / nq, 1),
                   graph_recall_at_10=round(bench.recall_at_10(g_ids, g_d, gt_d, dedup=False), 4))
        if not args.max_exact_candidates or m <= args.max_exact_candidates:
            x_host, x_ids, x_d, x_st = host_qps(f, True)
            x_dev = dev_qps(f, True)
            us = max(1, x_st["kernel_us"])
            fma = nq * m * dim / (us * 1e-6)
            row.update(exact_qps_search_batch=round(x_host), exact_qps_device=round(x_dev), exact_kernel_us=us,
                       exact_tfma_per_s=round(fma / 1e12, 2), exact_fraction_of_valu_peak=round(fma / PEAK_FMA, 3),
                       exact_fraction_of_plain_fma_peak=round(fma / PEAK_FMA_PLAIN, 3),
                       exact_recall_at_10=round(bench.recall_at_10(x_ids, x_d, gt_d, dedup=False), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del f
    cols = ["filter", "allowed", "graph_qps_search_batch", "graph_qps_device", "graph_expansions_per_query", "graph_recall_at_10",
            "exact_qps_search_batch", "exact_qps_device", "exact_kernel_us", "exact_tfma_per_s", "exact_fraction_of_valu_peak",
            "exact_fraction_of_plain_fma_peak", "exact_recall_at_10"]
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r.get(c), int) else str(r.get(c, "-")) for c in cols) + " |")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    x = crossover(rows)
    cross = dict(crossover_popcount=x, basis="exact_qps_device = graph_qps_device, log-log between the bracketing random-filter lines",
                 valu_peak_tfma_per_s=PEAK_FMA / 1e12, plain_fma_peak_tfma_per_s=PEAK_FMA_PLAIN / 1e12)
    print(json.dumps(cross), flush=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows + [cross]) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
