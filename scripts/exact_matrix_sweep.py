"""The two engines of the exact scan (index.exact_engine "vector" / "matrix") on the lines of profiles/exact_scan.md: the
C2 index (1M x 128, 4-bit), 10k queries, the filters of exact_sweep.py, k = 10, plus k = 100 and k = 1024 on the unfiltered
and the random 10 % lines.  Both engines ALTERNATE in one process (vector, matrix, vector, ... per repetition), so a line's
ratio never compares two sessions.  Per line: device QPS and kernel_us of both, matrix / vector, the prefilter's FMA rate
(nq x candidates x D / kernel time: an upper bound on its share, the certify kernel is inside) against --mfma-tfma, the
f32 MFMA rate knn_mfma_kernel reaches in the same session (knn_bruteforce of the index' first 262,144 rows against
themselves, wall clock: the host copies of 134 MB are inside, so the rate is a lower bound and the share an upper one),
survivors per query and matrix_redo; the rows of both engines are compared by bytes.  Then the small batches: 16, 128 and
1,024 queries on the unfiltered, 10 % and 0.1 % lines at k = 10 -- where the 128-query tile wastes work.
    python scripts/exact_matrix_sweep.py [--workdir DIR] [--reps 5] [--mfma-tfma X] [--out profiles/exact_matrix.md]"""
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
    ap.add_argument("--mfma-tfma", type=float, default=0.0, help="T FMA/s of knn_mfma_kernel measured in this session (0: not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_matrix.md"))
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
    rng = np.random.default_rng(7)
    lines = [("unfiltered", None, (10, 100, 1024)), ("all ones", np.ones(n, bool), (10,))]
    for p in (0.5, 0.1, 0.01):
        lines.append((f"random {p}", rng.random(n) < p, (10, 100, 1024) if p == 0.1 else (10,)))
    clustered = np.zeros(n, bool)
    clustered[int(0.45 * n):int(0.55 * n)] = True
    lines.append(("clustered 10 % (ids 450k-550k)", clustered, (10,)))
    lines.append(("random 0.001", np.random.default_rng(8).random(n) < 0.001, (10,)))
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)

    if not args.mfma_tfma:
        Xk = np.ascontiguousarray(ix.get_vectors(0, 262144))
        cphnsw_mi355x.knn_bruteforce(Xk[:4096])
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            cphnsw_mi355x.knn_bruteforce(Xk)
            ts.append(time.perf_counter() - t0)
        args.mfma_tfma = len(Xk) ** 2 * dim / float(np.median(ts)) / 1e12
        print(json.dumps(dict(knn_mfma_tfma_per_s_wall_clock=round(args.mfma_tfma, 2), rows=len(Xk))), flush=True)

    def one(engine, f, k, bq):
        ix.exact_engine = engine
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, d = ix.search_batch_device(Qd[:bq], k, filter=f, exact=True)
        ix.synchronize()
        return time.perf_counter() - t0, ids, d, ix.last_search_stats()

    rows = []
    full = nq
    small = [(name, mask, (10,), bq) for name, mask, _ in lines if name in ("unfiltered", "random 0.1", "random 0.001")
             for bq in (16, 128, 1024)]
    for name, mask, ks, nq in [(a, b, c, full) for a, b, c in lines] + small:
        f = None if mask is None else ix.make_filter(mask)
        m = int(n if mask is None else mask.sum())
        for k in ks:
            t = {"vector": [], "matrix": []}
            us = {"vector": [], "matrix": []}
            out = {}
            for rep in range(args.reps + 1):                    # (repetition 0 warms both up and is dropped)
                for engine in ("vector", "matrix"):
                    dt, ids, d, st = one(engine, f, k, nq)
                    out[engine] = (ids, d, st)
                    if rep:
                        t[engine].append(dt)
                        us[engine].append(st["kernel_us"])
            same = bool(torch.equal(out["vector"][0], out["matrix"][0]) and
                        torch.equal(out["vector"][1].view(torch.int32), out["matrix"][1].view(torch.int32)))
            st = out["matrix"][2]
            mus = float(np.median(us["matrix"]))
            row = dict(filter=name, allowed=m, queries=nq, k=k, vector_qps=round(nq / float(np.median(t["vector"]))),
                       matrix_qps=round(nq / float(np.median(t["matrix"]))), vector_kernel_us=round(float(np.median(us["vector"]))),
                       matrix_kernel_us=round(mus), matrix_over_vector=round(float(np.median(t["vector"]) / np.median(t["matrix"])), 3),
                       matrix_tfma_per_s=round(nq * m * dim / (max(mus, 1.0) * 1e-6) / 1e12, 2),
                       share_of_knn_mfma_rate=round(nq * m * dim / (max(mus, 1.0) * 1e-6) / 1e12 / args.mfma_tfma, 3) if args.mfma_tfma else "-",
                       survivors_per_query=round(st["matrix_survivors"] / nq, 2), matrix_redo=st["matrix_redo"],
                       matrix_parts=st["matrix_parts"], same_bytes=same,
                       qps_min_max=[round(nq / max(t[e])) for e in t] + [round(nq / min(t[e])) for e in t])
            print(json.dumps(row), flush=True)
            rows.append(row)
        del f
    cols = [c for c in rows[0] if c != "qps_min_max"]
    md = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    md += ["| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) and not isinstance(r[c], bool) else str(r[c]) for c in cols) + " |" for r in rows]
    with open(args.out, "w") as fh:
        fh.write(f"knn_mfma_kernel in this session: {args.mfma_tfma:.2f} T FMA/s\n\n")
        fh.write("\n".join(md) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
