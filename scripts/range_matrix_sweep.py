"""The two engines of the exact range search (index.exact_engine "vector" / "matrix") on the C2 index (1M x 128, 4-bit):
radii that give about 1, 10, 100 and 1,000 hits per query (the median k-th exact distance of the batch), unfiltered and
under a random 10 % filter, at 10,000, 128 and 16 queries.  Both engines ALTERNATE in one process, medians of --reps; a
line's ratio never compares two sessions, and losses are reported like gains.  Per line: wall-clock QPS of both engines
(range_search_device, begin + finish), matrix / vector, survivors per hit, whether the bytes are equal, and a LOWER bound on
the FMA rate of range_mfma_kernel: 2 passes x nq x candidates x D over the whole call's time, against the rate
knn_mfma_kernel reaches in the same process (wall clock, host copies inside).  The time per stage comes from a kernel
trace of this script (`rocprofv3 --kernel-trace --stats -- python scripts/range_matrix_sweep.py --reps 1`); it is pasted
under the table by hand.  Appends the table to --out.
    python scripts/range_matrix_sweep.py [--workdir DIR] [--reps 3] [--out profiles/range_matrix.md]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=os.environ.get("CPH_BENCH_DIR", "/tmp/cph_bench"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_matrix.md"))
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, nq, dim = cfg["n"], cfg["nq"], cfg["dim"]

    import torch
    import cphnsw_mi355x
    path, _, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    Q = bench.make_queries(cfg, n, nq)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    ix.load_native(path + ".native") if os.path.exists(path + ".native") else ix.load(path)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))

    Xk = np.ascontiguousarray(ix.get_vectors(0, 262144))
    cphnsw_mi355x.knn_bruteforce(Xk[:4096])
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        cphnsw_mi355x.knn_bruteforce(Xk)
        ts.append(time.perf_counter() - t0)
    knn_rate = len(Xk) ** 2 * dim / float(np.median(ts)) / 1e12

    def one(engine, f, radius, bq):
        ix.exact_engine = engine
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ix.range_search_device(Qd[:bq], radius[:bq], filter=f)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, ix.last_search_stats()

    rows = []
    for name, mask in (("unfiltered", None), ("random 0.1", np.random.default_rng(7).random(n) < 0.1)):
        f = None if mask is None else ix.make_filter(mask)
        m = int(n if mask is None else mask.sum())
        ix.exact_engine = "matrix"
        _, d = ix.search_batch(Q, 1000, filter=f, exact=True)
        for hits in (1, 10, 100, 1000):
            radius = np.full(nq, np.nextafter(np.float32(np.median(d[:, hits - 1])), np.float32(np.inf)), np.float32)
            for bq in (nq, 128, 16):
                t = {"vector": [], "matrix": []}
                out = {}
                for rep in range(args.reps + 1):                # (repetition 0 warms both up and is dropped)
                    for engine in ("vector", "matrix"):
                        dt, res, st = one(engine, f, radius, bq)
                        out[engine] = (res, st)
                        if rep:
                            t[engine].append(dt)
                (lv, iv, dv), (lm, im, dm) = out["vector"][0], out["matrix"][0]
                same = bool(torch.equal(lv, lm) and torch.equal(iv, im) and torch.equal(dv.view(torch.int32), dm.view(torch.int32)))
                st = out["matrix"][1]
                tm, tv = float(np.median(t["matrix"])), float(np.median(t["vector"]))
                total = int(lm[-1])
                row = dict(filter=name, allowed=m, queries=bq, hits_per_query=round(total / bq, 1), vector_qps=round(bq / tv),
                           matrix_qps=round(bq / tm), matrix_over_vector=round(tv / tm, 3),
                           survivors_per_hit=round(st.get("matrix_survivors", 0) / max(total, 1), 3),
                           matrix_parts=st.get("matrix_parts", 0),
                           count_kernel_tfma_lower_bound=round(2 * bq * m * dim / tm / 1e12, 2), same_bytes=same)
                rows.append(row)
                print(json.dumps(row), flush=True)
    keys = list(rows[0])
    with open(args.out, "a") as fh:
        fh.write(f"\n## Sweep ({time.strftime('%Y-%m-%d')}, medians of {args.reps}, engines alternating in one process)\n\n")
        fh.write(f"`knn_mfma_kernel` in the same process: {knn_rate:.1f} T FMA/s (wall clock, a lower bound).\n\n")
        fh.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
        for row in rows:
            fh.write("| " + " | ".join(str(row[k]) for k in keys) + " |\n")


if __name__ == "__main__":
    main()
