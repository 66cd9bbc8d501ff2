"""Per-query filters against the loop they replace, at the C2 shape (1M x 128, 4-bit, 10,000 queries, k = 10), in one
process: T tenants with equal-sized allowed sets, the queries assigned to them uniformly at random.  Per (route, T):
the wall time of ONE search_batch(Q, k, filter=[...], filter_of=...) and of the only way there was before -- a loop of
T single-filter search_batch(Q[sel], k, filter=f) calls over the same queries -- medians over --reps repetitions after
warm-up, their min-max spread, the ratio, and a byte comparison of the two results.  The two are timed interleaved, once
each per repetition in alternating order; at T = 1 the single-filter call on the whole batch is timed twice in the same
rounds, and the distance between those two medians is the noise the grouped call is held against.  Two set sizes, one on each side of
exact_threshold = 4000: 900 ids (every query is scanned) and 8,000 ids (every query takes the graph search).  The sets
are disjoint wherever T x size fits into the index; 8,000-id sets for T >= 256 cannot be (stated in the table), they are
drawn at random and overlap.  Two MIXED rows at T = 64 show what a graph-route query costs a scanned batch (the call then
encodes and descends every row): 64 tenants of 900 ids plus ONE query under an 8,000-id filter, and 32 tenants of each
size.  Reuses bench.py's data generators and its cached index file (same --workdir).
    python scripts/per_query_filter_sweep.py [--workdir DIR] [--reps 10] [--tenants 1,4,16,64,256,1024] [--out profiles/per_query_filters.md]"""
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

THRESHOLD = 4000
SIZES = (("scan", 900), ("graph", 8000))


def timed(fns, reps, warm=2):
    """Every function once per repetition, interleaved (A B C, then C B A, ...), so that a drift of clocks or temperature
    falls on all of them alike; per function (median, min, max) in ms and its last result."""
    outs = [None] * len(fns)
    t = [[] for _ in fns]
    for r in range(warm + reps):
        order = range(len(fns)) if r % 2 == 0 else range(len(fns) - 1, -1, -1)
        for i in order:
            t0 = time.perf_counter()
            outs[i] = fns[i]()
            if r >= warm:
                t[i].append((time.perf_counter() - t0) * 1e3)
    return [(float(np.median(x)), float(min(x)), float(max(x)), o) for x, o in zip(t, outs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=os.environ.get("CPH_BENCH_DIR", "/tmp/cph_bench"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tenants", default="1,4,16,64,256,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_query_filters.md"))
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, nq, k, dim = cfg["n"], cfg["nq"], cfg["k"], cfg["dim"]

    import cphnsw_mi355x
    path, _, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    Q = bench.make_queries(cfg, n, nq)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    if os.path.exists(path + ".native"):
        ix.load_native(path + ".native")
    else:
        ix.load(path)
    ix.exact_threshold = THRESHOLD
    rows = []
    tenants = [int(x) for x in args.tenants.split(",")]
    cases = [(route, [size] * T, False) for route, size in SIZES for T in tenants]
    # mixed routes in one call: a scanned batch with ONE graph-route query, and half the tenants on each side
    cases += [("scan+1graph", [SIZES[0][1]] * 64 + [SIZES[1][1]], True), ("half+half", [SIZES[0][1]] * 32 + [SIZES[1][1]] * 32, False)]
    for route, sizes, lone_last in cases:
        T, size = len(sizes), sizes[0]
        rng = np.random.default_rng(1000 * size + T)
        disjoint = sum(sizes) <= n
        if disjoint:
            perm = rng.permutation(n)
            cut = np.concatenate([[0], np.cumsum(sizes)])
            sets = [perm[cut[t]:cut[t + 1]] for t in range(T)]
        else:
            sets = [rng.choice(n, sz, replace=False) for sz in sizes]
        filters = [ix.make_filter(s) for s in sets]
        if lone_last:      # the last filter on exactly one query
            which = rng.integers(0, T - 1, nq)
            which[nq // 2] = T - 1
        else:
            which = rng.integers(0, T, nq)
        sels = [np.flatnonzero(which == t) for t in range(T)]
        subs = [np.ascontiguousarray(Q[s]) for s in sels]

        def grouped():
            return ix.search_batch(Q, k, filter=filters, filter_of=which)

        def loop():
            ids = np.empty((nq, k), np.int64)
            dist = np.empty((nq, k), np.float32)
            for t in range(T):
                if len(sels[t]):
                    ids[sels[t]], dist[sels[t]] = ix.search_batch(subs[t], k, filter=filters[t])
            return ids, dist

        fns = [grouped, loop]
        if T == 1:
            # the single-filter call on the whole batch, timed twice in the same rounds: the second against the first
            # is the noise floor the grouped call is held against
            fns += [lambda: ix.search_batch(Q, k, filter=filters[0])] * 2
        res = timed(fns, args.reps)
        (g_med, g_min, g_max, g_out), (l_med, l_min, l_max, l_out) = res[0], res[1]
        grouped()
        st = ix.last_search_stats()
        same = bool(np.array_equal(g_out[0], l_out[0]) and g_out[1].tobytes() == l_out[1].tobytes())
        row = dict(route=route, allowed_per_tenant="/".join(str(x) for x in sorted(set(sizes))), tenants=T, disjoint=disjoint,
                   grouped_ms=round(g_med, 3),
                   grouped_min_ms=round(g_min, 3), grouped_max_ms=round(g_max, 3), loop_ms=round(l_med, 3),
                   loop_min_ms=round(l_min, 3), loop_max_ms=round(l_max, 3), loop_over_grouped=round(l_med / g_med, 2),
                   grouped_kernel_us=st["kernel_us"], same_bytes=same)
        if T == 1:
            (s_med, s_min, s_max, _), (s2_med, s2_min, s2_max, _) = res[2], res[3]
            row.update(single_ms=round(s_med, 3), single_min_ms=round(s_min, 3), single_max_ms=round(s_max, 3),
                       single_again_ms=round(s2_med, 3), single_again_min_ms=round(s2_min, 3), single_again_max_ms=round(s2_max, 3))
        print(json.dumps(row), flush=True)
        rows.append(row)
        for f in filters:
            f.close()
    cols = ["route", "allowed_per_tenant", "tenants", "disjoint", "grouped_ms", "grouped_min_ms", "grouped_max_ms", "loop_ms",
            "loop_min_ms", "loop_max_ms", "loop_over_grouped", "grouped_kernel_us", "same_bytes"]
    lines = [f"C2 shape, {nq:,} queries, k = {k}, exact_threshold = {THRESHOLD}, medians of {args.reps} repetitions after 2 warm-up "
             "rounds (grouped and loop interleaved inside every round, order alternating), wall time of search_batch (host "
             "arrays in, host arrays out).  loop = T single-filter calls.  grouped kernel us = `kernel_us` of the grouped call: "
             "its clock starts BEFORE the query encode and the upper-layer descent of a call with graph-route queries, while "
             "the single-filter graph call starts it behind them, so on the graph rows it is not the single-filter call's quantity.", "",
             "| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(str(r.get(c, "-")) for c in cols) + " |")
    lines += ["", "What the rows say (loop over grouped above 1: the one call is faster):", ""]
    for r in rows:
        if r["tenants"] == 1:
            floor = abs(r["single_again_ms"] / r["single_ms"] - 1.0) * 100
            spread = (r["single_max_ms"] - r["single_min_ms"]) / r["single_ms"] * 100
            diff = (r["grouped_ms"] / r["single_ms"] - 1.0) * 100
            lines.append(f"- {r['route']}, T = 1: grouped {r['grouped_ms']} ms against the single-filter call {r['single_ms']} ms "
                         f"({diff:+.1f} %); the same single-filter call timed a second time in the same rounds: {r['single_again_ms']} ms "
                         f"(medians {floor:.1f} % apart), min-max spread of its repetitions {spread:.1f} % of the median.")
        else:
            verdict = "grouped faster" if r["loop_over_grouped"] > 1.0 else "LOOP FASTER OR EQUAL"
            lines.append(f"- {r['route']}, T = {r['tenants']}: loop / grouped = {r['loop_over_grouped']} ({verdict}); grouped min-max "
                         f"{r['grouped_min_ms']}-{r['grouped_max_ms']} ms, loop min-max {r['loop_min_ms']}-{r['loop_max_ms']} ms.")
    pure = [r for r in rows if r["route"] == "scan" and r["tenants"] == 64]
    lone = [r for r in rows if r["route"] == "scan+1graph"]
    if pure and lone:
        lines += ["", f"One graph-route query in a scanned batch (the call then encodes and descends all {nq:,} rows and adds a graph launch "
                  f"pair): {lone[0]['grouped_ms']} ms against {pure[0]['grouped_ms']} ms for the all-scanned batch of 64 tenants, "
                  f"{lone[0]['grouped_ms'] - pure[0]['grouped_ms']:+.3f} ms; device time {lone[0]['grouped_kernel_us']} against "
                  f"{pure[0]['grouped_kernel_us']} us."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
