"""Removed rows at the C2 shape (1M x 128, 4-bit, k = 10, 10,000-query search_batch_device batches), in one process:
unfiltered QPS and recall@10 (against exact=True over the live rows) with 0, 1 row, 1 %, 10 % and 50 % of the rows
removed at random -- the 1-row line is the price of leaving the probe-first kernel --, the latency of remove() for 1,
1,000 and 100,000 ids, and compact() against build + finalize of the same live rows.  Every share starts from a fresh
load of bench.py's cached index file (same --workdir).  The comparison of a clean handle with the parent commit is the
`python bench.py` headline at both commits in one session; it is not run from here.
    python scripts/remove_sweep.py [--workdir DIR] [--reps 5] [--out profiles/remove.md]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove.md"))
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, nq, k, dim = cfg["n"], cfg["nq"], cfg["k"], cfg["dim"]

    import torch
    import cphnsw_mi355x
    path, info, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    Q = bench.make_queries(cfg, n, nq)
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]

    def load():
        ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
        if os.path.exists(path + ".native"):
            ix.load_native(path + ".native")
        else:
            ix.load(path)
        return ix

    def dev_qps(ix):
        torch.cuda.synchronize()
        for i in range(4):                                   # warm-up: scratch, the adaptive knobs
            ix.search_batch_device(Qd, k, stream=streams[i & 1])
        ix.synchronize()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for i in range(4):
                ix.search_batch_device(Qd, k, stream=streams[i & 1])
            ix.synchronize()
            t.append(nq * 4 / (time.perf_counter() - t0))
        return float(np.median(t)), float(min(t)), float(max(t))

    rows = []
    rng = np.random.default_rng(11)
    for name, m in (("none", 0), ("1 row", 1), ("1 %", n // 100), ("10 %", n // 10), ("50 %", n // 2)):
        ix = load()
        if m:
            ix.remove(rng.choice(n, m, replace=False))
        qps, lo, hi = dev_qps(ix)
        ids, d = ix.search_batch(Q, k)
        st = ix.last_search_stats()
        xi, xd = ix.search_batch(Q, k, exact=True)
        hits = sum(len(np.intersect1d(ids[i][ids[i] >= 0], xi[i][xi[i] >= 0])) for i in range(nq))
        row = dict(removed=name, removed_rows=m, live=ix.live_count, qps_device=round(qps), qps_min=round(lo), qps_max=round(hi),
                   expansions_per_query=round(st["expansions"] / nq, 1), stage2_reruns=st["stage2_reruns"],
                   recall_at_10_vs_exact_live=round(hits / float((xi >= 0).sum()), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ix
    lat = []
    for m in (1, 1000, 100000):
        ix = load()
        ix.search_batch(Q[:64], k)
        ids = rng.choice(n, m, replace=False)
        t0 = time.perf_counter()
        ix.remove(ids)
        first = time.perf_counter() - t0
        more = rng.choice(n, m, replace=False)
        t0 = time.perf_counter()
        ix.remove(more)
        lat.append(dict(ids=m, first_remove_ms=round(first * 1e3, 3), second_remove_ms=round((time.perf_counter() - t0) * 1e3, 3)))
        print(json.dumps(lat[-1]), flush=True)
        del ix
    ix = load()
    ix.remove(rng.choice(n, n // 10, replace=False))
    live = ix.get_vectors()[~ix.removed_mask(ids="internal")]
    t0 = time.perf_counter()
    ix.compact()
    t_compact = time.perf_counter() - t0
    fresh = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    t0 = time.perf_counter()
    fresh.build(live)
    fresh.finalize()
    comp = dict(live_rows=int(live.shape[0]), compact_s=round(t_compact, 3), build_finalize_s=round(time.perf_counter() - t0, 3))
    print(json.dumps(comp), flush=True)

    cols = list(rows[0])
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    with open(args.out, "w") as fh:
        fh.write("# Removed rows: 1M x 128, 4-bit, k = 10, 10,000-query search_batch_device batches\n\n" + "\n".join(lines) +
                 "\n\n```\n" + "\n".join(json.dumps(r) for r in rows + lat + [comp]) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
