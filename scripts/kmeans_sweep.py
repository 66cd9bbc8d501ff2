"""index.kmeans on the C2 index (1M x 128, 4-bit) at k = 256, 1024, 4096, 16384, next to what a caller writes today on the
same device and the same rows: torch.cdist + argmin + index_add_ per iteration.  Both ALTERNATE in one process (kmeans,
torch, kmeans, ... per repetition; repetition 0 warms both up and is dropped); medians, with the spread next to them.
Per k:
  assign_us / assign_tfma_per_s   the matrix kernel of the last assignment pass between two HIP events (time_kmeans):
                                  n x k x D FMA over that time, next to knn_mfma_kernel's rate re-measured in this session
                                  (knn_bruteforce of the first 262,144 rows, wall clock: a lower bound, host copies inside)
  resolve_share                   rows the matrix kernels left to the vector kernel / (rows x passes)
  update_us / update_floor_us     (a call of `iters` iterations - a call of 0 iterations) / iters - assign pass time,
                                  against 4 n D bytes at --hbm-tb-s: the update reads every live row once
  kmeans_ms / torch_ms            the whole call of --iters iterations, host clock around work that ends in a synchronise
The init of both is the same k live rows; the torch loop divides sums by counts and keeps empty clusters, like kmeans.
    python scripts/kmeans_sweep.py [--workdir DIR] [--reps 5] [--iters 5] [--hbm-tb-s 8.0] [--out profiles/kmeans.md]"""
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ks", type=int, nargs="*", default=[256, 1024, 4096, 16384])
    ap.add_argument("--hbm-tb-s", type=float, default=8.0, help="HBM bandwidth the update's byte floor is taken at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.md"))
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, dim = cfg["n"], cfg["dim"]

    import torch
    import cphnsw_mi355x
    path, _, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    ix.load_native(path + ".native") if os.path.exists(path + ".native") else ix.load(path)
    X = np.ascontiguousarray(ix.get_vectors(stored=True))
    dev = torch.device("cuda", 0)
    Xd = torch.from_numpy(X).to(dev)

    cphnsw_mi355x.knn_bruteforce(X[:4096])
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        cphnsw_mi355x.knn_bruteforce(X[:262144])
        ts.append(time.perf_counter() - t0)
    knn_tfma = 262144 ** 2 * dim / float(np.median(ts)) / 1e12
    print(json.dumps(dict(knn_mfma_tfma_per_s_wall_clock=round(knn_tfma, 2))), flush=True)

    def ours(k, iters, C0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = ix.kmeans_device(k, iters=iters, init=C0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, outs

    def theirs(k, iters, C0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        C = C0.clone()
        for it in range(iters + 1):
            a = torch.cat([torch.cdist(Xd[i:i + 65536], C).argmin(1) for i in range(0, n, 65536)])     # (n x k floats do not fit at once)
            if it == iters:
                break
            sums = torch.zeros_like(C).index_add_(0, a, Xd)
            cnt = torch.bincount(a, minlength=k).to(torch.float32)
            C = torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1)[:, None], C)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, a

    ix.time_kmeans(True)
    rows = []
    for k in args.ks:
        C0 = Xd[torch.from_numpy(np.random.default_rng(k).choice(n, k, replace=False)).to(dev)].contiguous()
        t = {"kmeans": [], "kmeans0": [], "torch": []}
        assign_us, unc = [], []
        for rep in range(args.reps + 1):
            dt, outs = ours(k, args.iters, C0)
            us, (passes, u) = ix.last_kmeans_us(), ix.kmeans_stats()
            dt0, _ = ours(k, 0, C0)
            dtt, a = theirs(k, args.iters, C0)
            if rep:
                t["kmeans"].append(dt), t["kmeans0"].append(dt0), t["torch"].append(dtt)
                assign_us.append(us), unc.append(u / (n * passes))
        agree = float((outs[1].to(torch.int64) == a).float().mean())
        med = {e: float(np.median(v)) for e, v in t.items()}
        aus = float(np.median(assign_us))
        row = dict(k=k, iters=args.iters, assign_us=round(aus), assign_tfma_per_s=round(n * k * dim / (aus * 1e-6) / 1e12, 2),
                   share_of_knn_mfma_rate=round(n * k * dim / (aus * 1e-6) / 1e12 / knn_tfma, 3),
                   resolve_share=round(float(np.median(unc)), 5),
                   update_us=round((med["kmeans"] - med["kmeans0"]) / args.iters * 1e6 - med["kmeans0"] * 1e6),
                   update_floor_us=round(4.0 * n * dim / (args.hbm_tb_s * 1e12) * 1e6, 1),
                   kmeans_ms=round(med["kmeans"] * 1e3, 2), torch_ms=round(med["torch"] * 1e3, 2),
                   torch_over_kmeans=round(med["torch"] / med["kmeans"], 2), same_assignment_share=round(agree, 5),
                   ms_min_max=[round(min(t[e]) * 1e3, 2) for e in ("kmeans", "torch")] + [round(max(t[e]) * 1e3, 2) for e in ("kmeans", "torch")])
        print(json.dumps(row), flush=True)
        rows.append(row)
    cols = [c for c in rows[0] if c != "ms_min_max"]
    md = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    md += ["| " + " | ".join(str(r[c]) for c in cols) + " |" for r in rows]
    with open(args.out, "w") as fh:
        fh.write(f"knn_mfma_kernel in this session: {knn_tfma:.2f} T FMA/s (wall clock)\n\n")
        fh.write("\n".join(md) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
