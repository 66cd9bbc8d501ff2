"""Multi-vector (MaxSim) search against the plain call it is built on: 1M x 128, 4-bit, cosine, T = 32 tokens per query,
device batches of 1,000 queries, k = 10, C in {32, 64, 128, 256}, in one process: search_maxsim_device(k, candidates=C)
next to search_batch_device(k=C) over the same 32,000 token rows on the same handle -- the call a user would otherwise make
before joining n * T * C results by document on the host -- alternating, warm; median and spread of --reps runs each, host
clock around calls that end in a device synchronise.  maxsim_rows_kernel alone is timed with HIP events
(CPIndex.time_maxsim / last_maxsim_rows_us), median over the same runs.
No target is fixed in advance: the numbers to report are the ratio to the plain call at the same C and the kernel's own
time and share.  The key of a row is its input row // --doc-rows (documents of 32 consecutive input rows).
    python scripts/maxsim_sweep.py [--reps 7] [--nq 1000] [--tokens 32] [--out profiles/maxsim.md]
Reuses bench.py's data generators (config c2); the index is built in the process.  The report is the table and the JSON
lines; whatever the output file holds from the line KEEP on (resource usage, the bench.py comparison, a hand-written
reading of the numbers) is carried over."""
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

CANDIDATES = (32, 64, 128, 256)
KEEP = "<!-- below this line: written by hand, kept by scripts/maxsim_sweep.py -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nq", type=int, default=1_000)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--doc-rows", type=int, default=32)
    ap.add_argument("--n", type=int, default=0, help="override the index size (rehearsals)")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim.md"))
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n, dim, nq, T, k = args.n or cfg["n"], cfg["dim"], args.nq, args.tokens, args.k

    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("maxsim_sweep.py measures on the GPU: no HIP device here")
    X = bench.make_base(cfg, n)
    Q = bench.make_queries(cfg, n, nq * T)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0, metric="cosine")
    t0 = time.time()
    ix.build(X)
    ix.finalize()
    print(f"built n={n} in {time.time() - t0:.1f} s", flush=True)
    del X
    ix.set_labels(np.arange(n) // args.doc_rows, ids="input")
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)                      # [nq * T, dim]: the plain call's batch
    Td = Qd.view(nq, T, dim)
    ix.time_maxsim(True)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ix.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    rows = []
    for C_ in CANDIDATES:
        out_m = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                 torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k, T), dtype=torch.int64, device=dev),
                 torch.empty((nq,), dtype=torch.int32, device=dev))
        out_s = (torch.empty((nq * T, C_), dtype=torch.int64, device=dev), torch.empty((nq * T, C_), dtype=torch.float32, device=dev))
        run_maxsim = lambda: ix.search_maxsim_device(Td, k, candidates=C_, out=out_m)          # noqa: E731
        run_plain = lambda: ix.search_batch_device(Qd, C_, out=out_s)                          # noqa: E731
        for _ in range(2):                                                                     # warm, both
            timed(run_maxsim)
            timed(run_plain)
        tm, tp, tk = [], [], []
        for _ in range(args.reps):                                                             # alternating
            dt, res = timed(run_maxsim)
            tm.append(dt)
            tk.append(ix.last_maxsim_rows_us())
            dt, plain = timed(run_plain)
            tp.append(dt)
        hits = res[2].cpu().numpy()
        found = res[4].cpu().numpy()
        ids = plain[0].cpu().numpy()
        kern = float(np.median(tk))
        row = dict(tokens=T, candidates=C_, k=k, queries=nq, token_rows=nq * T,
                   maxsim_ms_median=round(float(np.median(tm)) * 1e3, 3), maxsim_ms_min=round(min(tm) * 1e3, 3),
                   maxsim_ms_max=round(max(tm) * 1e3, 3), plain_ms_median=round(float(np.median(tp)) * 1e3, 3),
                   plain_ms_min=round(min(tp) * 1e3, 3), plain_ms_max=round(max(tp) * 1e3, 3),
                   kernel_us_median=round(kern, 1), kernel_us_min=round(min(tk), 1), kernel_us_max=round(max(tk), 1),
                   kernel_us_per_query=round(kern / nq, 3), mean_found=round(float(found.mean()), 2),
                   mean_hits_of_tokens=round(float(hits[:, 0].mean()) / T, 3), valid_entries=round(float((ids >= 0).mean()), 4),
                   host_download_mb_avoided=round(nq * T * C_ * 12 / 1e6, 1), reps=args.reps)
        row["ratio_of_medians"] = round(row["maxsim_ms_median"] / row["plain_ms_median"], 3)
        row["kernel_share_of_maxsim"] = round(kern / 1e3 / row["maxsim_ms_median"], 4)
        row["kernel_over_plain"] = round(kern / 1e3 / row["plain_ms_median"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    ix.time_maxsim(False)
    if not args.no_write:
        write_report(rows, cfg, n, dim, nq, T, k, args.doc_rows, args.reps, args.out)


def write_report(rows, cfg, n, dim, nq, T, k, doc_rows, reps, out):
    cols = ["candidates", "maxsim_ms_median", "maxsim_ms_min", "maxsim_ms_max", "plain_ms_median", "plain_ms_min", "plain_ms_max",
            "ratio_of_medians", "kernel_us_median", "kernel_us_min", "kernel_us_max", "kernel_us_per_query", "kernel_share_of_maxsim",
            "kernel_over_plain", "mean_found", "mean_hits_of_tokens", "valid_entries", "host_download_mb_avoided"]
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    head = ("# Multi-vector search: search_maxsim_device(k, candidates=C) against search_batch_device(k=C) of the same token rows\n\n"
            f"{cfg['label']}: {n:,} x {dim}, {cfg['bits']}-bit, metric cosine, T = {T} tokens per query (all live), k = {k}, batches of "
            f"{nq:,} queries = {nq * T:,} token rows on the device, documents of {doc_rows} consecutive input rows, one process, the two "
            f"calls alternating, warm, both into preallocated outputs; median / min / max of {reps} runs each (host clock around calls "
            "that end in a device synchronise).  `plain` is the search of the token rows at k = C, which the maxsim call contains; "
            "`kernel us` is maxsim_rows_kernel alone between two HIP events, `kernel over plain` its time over the plain call's.  "
            "`mean hits of tokens`: hits / T of the best key; `valid entries`: the share of the plain call's slots that are not "
            "padding; `host download mb avoided`: the ids and distances a caller would otherwise copy to the host per batch.  "
            "scripts/maxsim_sweep.py.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    old = open(out).read() if os.path.exists(out) else ""
    kept = old[old.index(KEEP):] if KEEP in old else KEEP + "\n"
    with open(out, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
