"""Measures search_maxsim_device(candidates="all", rescore=R) against search_maxsim_device(exact=True, candidates=C0,
rescore=R) on the same handle and prints a markdown table (profiles/maxsim_all.md keeps it).

Per line (rows-per-document, batch, R): the two calls alternate in one process, median of 3, each timed by a host clock
around a call that ends in a stream synchronise; the bounds kernel of the new call alone between two HIP events
(time_maxsim_all), its rate (n * T * rows * D multiply-adds over that time) and that rate as a share of what
knn_mfma_kernel reaches in the same process (knn_bruteforce of the first 262,144 rows, wall clock with the host copies
inside: a lower bound of the kernel's rate, so the share is an upper bound); how many queries each call certifies in all k
slots; recall@k of the old call against the new call's answer where that is fully certified.  Needs a GPU: no fallback.

    python scripts/maxsim_all_sweep.py --rows 1000000 --dim 128 --tokens 32 --batches 16 128 1000 --docs 32 256 --rescore 64 1024
"""
import argparse
import statistics
import time

import numpy as np
import torch

import cphnsw_mi355x as cph


def timed(fn, stream):
    stream.synchronize()
    t0 = time.perf_counter()
    out = fn()
    stream.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--docs", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 128, 1000])
    ap.add_argument("--rescore", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    X = rng.standard_normal((a.rows, a.dim)).astype(np.float32)
    ix = cph.CPIndex(a.dim, 4, metric="cosine")
    t0 = time.perf_counter()
    ix.build(X)
    ix.finalize()
    print(f"build of {a.rows} x {a.dim}: {time.perf_counter() - t0:.1f} s")
    Xk = np.ascontiguousarray(ix.get_vectors(0, min(a.rows, 262144)))
    cph.knn_bruteforce(Xk[:4096])
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        cph.knn_bruteforce(Xk)
        ts.append(time.perf_counter() - t0)
    knn = len(Xk) ** 2 * a.dim / statistics.median(ts) / 1e12
    print(f"knn_mfma_kernel in this process: {knn:.1f} T FMA/s (wall clock, a lower bound)")
    stream = torch.cuda.Stream()
    T, k = a.tokens, a.k
    print("| rows/doc | batch | R | all ms | old ms | bounds ms | T FMA/s | share of kNN | certified == k: all | old | recall@k of old |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for per in a.docs:
        ix.set_labels(np.arange(a.rows) // per, ids="internal")
        ix.prepare_maxsim_rescore()
        for n in a.batches:
            src = rng.integers(0, a.rows, (n, T))
            Q = torch.from_numpy((X[src] + np.float32(0.3) * rng.standard_normal((n, T, a.dim))).astype(np.float32)).cuda()
            for R in a.rescore:
                new = lambda: ix.search_maxsim_device(Q, k, candidates="all", rescore=R, stream=stream)                # noqa: E731
                old = lambda: ix.search_maxsim_device(Q, k, exact=True, rescore=R, stream=stream)                      # noqa: E731
                new(), old()                                                                                           # warm-up
                ix.time_maxsim_all(True)
                tn, to, tk = [], [], []
                for _ in range(a.reps):
                    ms, rn = timed(new, stream)
                    tn.append(ms)
                    tk.append(ix.last_maxsim_all_us() / 1e3)
                    ms, ro = timed(old, stream)
                    to.append(ms)
                ix.time_maxsim_all(False)
                kern = statistics.median(tk)
                rate = n * T * a.rows * a.dim / (kern * 1e-3) / 1e12
                cn, co = rn[5].cpu().numpy(), ro[5].cpu().numpy()
                kn, ko = rn[0].cpu().numpy(), ro[0].cpu().numpy()
                full = cn >= k
                rec = np.mean([len(set(kn[i]) & set(ko[i])) / k for i in np.flatnonzero(full)]) if full.any() else float("nan")
                print(f"| {per} | {n} | {R} | {statistics.median(tn):.2f} | {statistics.median(to):.2f} | {kern:.2f} | {rate:.2f} | {rate / knn:.2f} | "
                      f"{int(full.sum())}/{n} | {int((co >= k).sum())}/{n} | {rec:.3f} |", flush=True)


if __name__ == "__main__":
    main()
