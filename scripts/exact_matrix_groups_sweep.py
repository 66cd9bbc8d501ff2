"""Per-query filters under both engines of the exact scan (index.exact_engine "vector" / "matrix",
device_exact_mfma_groups.h): the C2 index (1M x 128, 4-bit), device batches of 10,000 queries, k = 10.
  1. The batch spread evenly over F = 1, 8, 64, 512 filters of 100,000 and of 10,000 allowed ids: segments of 10,000 down
     to about 20 queries.  The F = 1 line also against the single-filter matrix call over the same filter.
  2. Segments of 8, 16, 32, 64 and 128 queries over filters of 10,000 ids, on a handle made with CPH_MATRIX_GROUP_MIN=1
     (every scanned segment takes the matrix kernels): kMxGroupMinQueries is the smallest size from which the matrix route
     is not slower than the vector route by more than the run-to-run spread.
Both engines ALTERNATE in one process (vector, matrix, vector, ... per repetition; repetition 0 warms up and is dropped);
per line the median wall-clock time of a device call with its synchronize, min and max, kernel_us, and a byte comparison.
    python scripts/exact_matrix_groups_sweep.py [--workdir DIR] [--reps 7] [--out profiles/exact_matrix_groups.md]"""
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

K = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=os.environ.get("CPH_BENCH_DIR", "/tmp/cph_bench"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_matrix_groups.md"))
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, nq, dim = cfg["n"], cfg["nq"], cfg["dim"]

    import torch
    import cphnsw_mi355x
    path, _, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    Qd = torch.from_numpy(bench.make_queries(cfg, n, nq)).to(torch.device("cuda", 0))

    def handle(group_min=None):
        if group_min is not None:
            os.environ["CPH_MATRIX_GROUP_MIN"] = str(group_min)
        ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
        os.environ.pop("CPH_MATRIX_GROUP_MIN", None)
        ix.load_native(path + ".native") if os.path.exists(path + ".native") else ix.load(path)
        return ix

    def timed(ix, engine, **kw):
        ix.exact_engine = engine
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, d = ix.search_batch_device(Qd, K, exact=True, **kw)
        ix.synchronize()
        return time.perf_counter() - t0, ids, d, ix.last_search_stats()

    def line(ix, what, calls):
        """calls: name -> (engine, kwargs), run in turn per repetition; a dict of medians and spreads, bytes compared with the first."""
        t = {c: [] for c in calls}
        us = {c: [] for c in calls}
        out = {}
        for rep in range(args.reps + 1):
            for c, (engine, kw) in calls.items():
                dt, ids, d, st = timed(ix, engine, **kw)
                out[c] = (ids, d, st)
                if rep:
                    t[c].append(dt * 1e3)
                    us[c].append(st["kernel_us"])
        first = next(iter(calls))
        row = dict(what)
        for c in calls:
            row[f"{c}_ms"] = round(float(np.median(t[c])), 3)
            row[f"{c}_ms_min_max"] = [round(min(t[c]), 3), round(max(t[c]), 3)]
            row[f"{c}_kernel_us"] = round(float(np.median(us[c])))
            if c != first:
                row[f"{first}_over_{c}"] = round(float(np.median(t[first]) / np.median(t[c])), 3)
                row[f"{c}_same_bytes"] = bool(torch.equal(out[first][0], out[c][0]) and
                                              torch.equal(out[first][1].view(torch.int32), out[c][1].view(torch.int32)))
        st = out["matrix"][2]
        row.update(matrix_parts=st.get("matrix_parts", 0), survivors_per_query=round(st.get("matrix_survivors", 0) / nq, 2),
                   matrix_redo=st.get("matrix_redo", 0))
        print(json.dumps(row), flush=True)
        return row

    def filters_of(ix, F, m, seed):
        rng = np.random.default_rng(seed)
        return [ix.make_filter(np.sort(rng.choice(n, m, replace=False)), ids="internal") for _ in range(F)]

    tables = []
    ix = handle()
    rows = []
    for m in (100_000, 10_000):
        for F in (1, 8, 64, 512):
            fs = filters_of(ix, F, m, 100 + F)
            fo = np.arange(nq) % F
            calls = {"vector": ("vector", dict(filter=fs, filter_of=fo)), "matrix": ("matrix", dict(filter=fs, filter_of=fo))}
            if F == 1:
                calls["single_filter_matrix"] = ("matrix", dict(filter=fs[0]))
            rows.append(line(ix, dict(allowed=m, filters=F, queries_per_segment=nq // F), calls))
            del fs
    tables.append(("Segments of 10,000 down to about 20 queries (default handle)", rows))
    del ix
    ix = handle(group_min=1)
    rows = []
    for size in (8, 16, 32, 64, 128):
        F = nq // size
        fs = filters_of(ix, F, 10_000, 200 + size)
        fo = np.arange(nq) % F
        rows.append(line(ix, dict(allowed=10_000, filters=F, queries_per_segment=size),
                         {"vector": ("vector", dict(filter=fs, filter_of=fo)), "matrix": ("matrix", dict(filter=fs, filter_of=fo))}))
        del fs
    tables.append(("Segment sizes at 10,000 allowed ids, every segment on the matrix kernels (CPH_MATRIX_GROUP_MIN=1)", rows))
    with open(args.out, "w") as fh:
        for title, rows in tables:
            cols = list(dict.fromkeys(c for r in rows for c in r))
            fh.write(f"## {title}\n\n| " + " | ".join(c.replace("_", " ") for c in cols) + " |\n|" + "---|" * len(cols) + "\n")
            fh.write("\n".join("| " + " | ".join(str(r.get(c, "")) for c in cols) + " |" for r in rows) + "\n\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
