"""Two-stage search against the plain call it is built on: 1M x 128, 4-bit, 10,000-query device batches, k = 10, one process.

Data: synthetic prefix-trained rows -- 1,024 coordinates whose standard deviation decays with the coordinate
(1 / (1 + j / 32)), 1,000 clusters -- indexed on their first 128 coordinates; the objects hold the first 256 or all 1,024.
  (a) search_rescored_device(k, candidates=C) next to search_batch_device(k=C) on the same handle and queries, alternating,
      warm; median / min / max of --reps runs each, host clock around calls that end in a device synchronise.
  (b) the rescoring kernel alone (CPIndex.time_rescored / last_rescored_us), median over the same runs, against its byte
      floor: queries x C x stored row bytes / 6.29 TB/s (the measured copy rate of the part).
  (c) recall@10 against a float64 brute force at full width over --recall-queries queries: the plain search on the prefix,
      and the rescored search at each C (float16 rows of 1,024).
No target is fixed in advance.
    python scripts/rescore_sweep.py [--reps 5] [--nq 10000] [--out profiles/rescored_search.md]
    python scripts/rescore_sweep.py --n 100000 --no-write        # a rehearsal
Whatever the output file holds from the line KEEP on (a hand-written reading of the numbers) is carried over."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))

CS = (64, 128, 256)
OBJECTS = ((256, "float16", CS), (1024, "float16", CS), (1024, "float32", (128,)))       # (dim_full, dtype, the C it runs at)
COPY_TB_S = 6.29
KEEP = "<!-- below this line: written by hand, kept by scripts/rescore_sweep.py -->"
DIM, DIM_FULL, BITS, K = 128, 1024, 4, 10


def make_data(torch, n, nq, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(20260)
    sigma = 1.0 / (1.0 + torch.arange(DIM_FULL, device=dev, dtype=torch.float32) / 32.0)
    centers = torch.randn((1000, DIM_FULL), generator=g, device=dev) * sigma

    def rows(m):
        c = torch.randint(0, 1000, (m,), generator=g, device=dev)
        return (centers[c] + 0.5 * torch.randn((m, DIM_FULL), generator=g, device=dev) * sigma).contiguous()
    return rows(n), rows(nq)


def brute_force(torch, Xd, Qd, k):
    """float64 top-k of |q - x|^2 at full width -> int64 [nq, k] on the host."""
    q = Qd.double()
    best_d = torch.full((q.shape[0], k), float("inf"), dtype=torch.float64, device=q.device)
    best_i = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=q.device)
    for lo in range(0, Xd.shape[0], 100_000):
        x = Xd[lo:lo + 100_000].double()
        d = (x * x).sum(1)[None, :] - 2.0 * (q @ x.T)
        dd, ii = torch.topk(d, k, dim=1, largest=False)
        alld, alli = torch.cat([best_d, dd], 1), torch.cat([best_i, ii + lo], 1)
        best_d, sel = torch.topk(alld, k, dim=1, largest=False)
        best_i = torch.gather(alli, 1, sel)
    return best_i.cpu().numpy()


def recall(ids, truth):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / truth.shape[1] for a, b in zip(ids, truth)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--n", type=int, default=1_000_000, help="override the index size (rehearsals)")
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescored_search.md"))
    args = ap.parse_args()
    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("rescore_sweep.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda", 0)
    n, nq, nr = args.n, args.nq, min(args.recall_queries, args.nq)
    Xd, FQd = make_data(torch, n, nq, dev)
    truth = brute_force(torch, Xd, FQd[:nr], K)
    X = Xd.cpu().numpy()
    del Xd
    torch.cuda.empty_cache()
    ix = cphnsw_mi355x.CPIndex(DIM, BITS, device=0)
    t0 = time.time()
    ix.build(np.ascontiguousarray(X[:, :DIM]))
    ix.finalize()
    ix.result_ids = "input"
    print(f"built n={n} in {time.time() - t0:.1f} s", flush=True)
    Qd = FQd[:, :DIM].contiguous()
    ix.time_rescored(True)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ix.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    rows, rec = [], {}
    plain = ix.search_batch_device(Qd[:nr], K)[0]
    torch.cuda.synchronize()
    rec["plain search on the 128-coordinate prefix, k = 10"] = round(recall(plain.cpu().numpy(), truth), 4)
    for (dim_full, dtype, cs) in OBJECTS:
        rv = ix.make_rescore_vectors(np.ascontiguousarray(X[:, :dim_full]), ids="input", dtype=dtype, metric="l2")
        fq = FQd[:, :dim_full].contiguous()
        for C_ in cs:
            out_r = (torch.empty((nq, K), dtype=torch.int64, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev),
                     torch.empty((nq, K), dtype=torch.float32, device=dev))
            out_s = (torch.empty((nq, C_), dtype=torch.int64, device=dev), torch.empty((nq, C_), dtype=torch.float32, device=dev))
            run_r = lambda: ix.search_rescored_device(Qd, K, rv, full_queries=fq, candidates=C_, out=out_r)      # noqa: E731
            run_s = lambda: ix.search_batch_device(Qd, C_, out=out_s)                                            # noqa: E731
            for _ in range(2):
                timed(run_r)
                timed(run_s)
            tr, ts, tk = [], [], []
            for _ in range(args.reps):
                dt, res = timed(run_r)
                tr.append(dt)
                tk.append(ix.last_rescored_us())
                dt, _ = timed(run_s)
                ts.append(dt)
            kern, gb = float(np.median(tk)), nq * C_ * rv.row_bytes / 1e9
            floor_us = gb / COPY_TB_S * 1e3
            row = dict(dim_full=dim_full, dtype=dtype, candidates=C_, queries=nq, rescored_ms_median=round(float(np.median(tr)) * 1e3, 3),
                       rescored_ms_min=round(min(tr) * 1e3, 3), rescored_ms_max=round(max(tr) * 1e3, 3),
                       plain_ms_median=round(float(np.median(ts)) * 1e3, 3), plain_ms_min=round(min(ts) * 1e3, 3),
                       plain_ms_max=round(max(ts) * 1e3, 3), kernel_us_median=round(kern, 1), kernel_us_max=round(max(tk), 1),
                       row_bytes=rv.row_bytes, gathered_gb=round(gb, 3), floor_us=round(floor_us, 1),
                       kernel_over_floor=round(kern / floor_us, 2), gathered_tb_s=round(gb / kern * 1e3, 3), reps=args.reps)
            row["ratio_of_medians"] = round(row["rescored_ms_median"] / row["plain_ms_median"], 3)
            row["kernel_over_plain_call"] = round(kern / 1e3 / row["plain_ms_median"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
            if dim_full == DIM_FULL and dtype == "float16":
                rec[f"rescored at C = {C_}, float16 rows of {DIM_FULL}"] = round(recall(res[0][:nr].cpu().numpy(), truth), 4)
        rv.close()
    ix.time_rescored(False)
    print(json.dumps(rec), flush=True)
    if not args.no_write:
        write_report(rows, rec, n, nq, nr, args.reps, args.out)


def write_report(rows, rec, n, nq, nr, reps, out):
    cols = ["dim_full", "dtype", "candidates", "rescored_ms_median", "rescored_ms_min", "rescored_ms_max", "plain_ms_median",
            "plain_ms_min", "plain_ms_max", "ratio_of_medians", "kernel_us_median", "kernel_us_max", "row_bytes", "gathered_gb",
            "floor_us", "kernel_over_floor", "gathered_tb_s", "kernel_over_plain_call"]
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(str(r[c]) for c in cols) + " |")
    lines += ["", "| recall@10 against float64 brute force at 1,024 coordinates | |", "|---|---|"]
    lines += [f"| {what} | {v} |" for what, v in rec.items()] or ["| Not measured | |"]
    head = ("# Two-stage search: search_rescored_device(k = 10, candidates=C) against search_batch_device(k=C)\n\n"
            f"{n:,} x {DIM}, {BITS}-bit, over synthetic prefix-trained rows of {DIM_FULL} coordinates (standard deviation 1 / (1 + j / 32), "
            f"1,000 clusters) indexed on their first {DIM}; batches of {nq:,} queries on the device, one process, the two calls "
            f"alternating, warm, both into preallocated outputs; median / min / max of {reps} runs each (host clock around calls that "
            "end in a device synchronise).  `plain` is the search at the same C, which the rescored call contains; `kernel us` is "
            "rescore_rows_kernel alone between two HIP events; `floor us` = queries x C x stored row bytes / 6.29 TB/s; `kernel "
            f"over plain call` = the kernel's time over the plain call's.  Recall over the first {nr:,} queries.  "
            "scripts/rescore_sweep.py.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    old = open(out).read() if os.path.exists(out) else ""
    kept = old[old.index(KEEP):] if KEEP in old else KEEP + "\n"
    with open(out, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n" + json.dumps(rec) + "\n```\n\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
