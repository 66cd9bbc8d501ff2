"""Grouped search against the ungrouped call it is built on, at the C2 shape (1M x 128, 4-bit, 10,000-query device
batches), in one process: search_grouped_device(k, g, candidates=C) next to search_batch_device(k=C) on the same handle
and queries -- the call a user would otherwise make before grouping on the host -- alternating, warm; median and spread of
--reps runs each, host clock around calls that end in a device synchronise.  The group kernel alone is timed with HIP
events (CPIndex.time_grouped / last_group_rows_us), median over the same runs.  Keys: every row belongs to one of
n / 8 documents, drawn at random, so a document has about eight rows anywhere in the index.
No target is fixed in advance: the numbers to report are the ratio to the ungrouped call at the same C and the kernel's
share of the grouped call.
    python scripts/grouped_sweep.py [--reps 7] [--nq 10000] [--out profiles/grouped_search.md]
    python scripts/grouped_sweep.py --only 10/3/128 --reps 3 --no-write       # one case, for a kernel trace of its own
Reuses bench.py's data generators (config c2); the index is built in the process.  The report is the table and the JSON
lines; whatever the output file holds from the line KEEP on (a hand-written reading of the numbers) is carried over."""
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

CASES = ((10, 1, 64), (10, 3, 128), (10, 3, 1024), (100, 4, 1024))       # (k, g, C)
ROWS_PER_KEY = 8
KEEP = "<!-- below this line: written by hand, kept by scripts/grouped_sweep.py -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--n", type=int, default=0, help="override the index size (rehearsals)")
    ap.add_argument("--only", default="", help="k/g/C of the one case to run, e.g. 10/3/128")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_search.md"))
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n, dim, nq = args.n or cfg["n"], cfg["dim"], args.nq

    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("grouped_sweep.py measures on the GPU: no HIP device here")
    X = bench.make_base(cfg, n)
    Q = bench.make_queries(cfg, n, nq)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    t0 = time.time()
    ix.build(X)
    ix.finalize()
    print(f"built n={n} in {time.time() - t0:.1f} s", flush=True)
    del X
    ix.set_labels(np.random.default_rng(11).integers(0, max(1, n // ROWS_PER_KEY), n), ids="internal")
    ix.time_grouped(True)
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ix.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    rows = []
    for (k, g, C_) in CASES:
        if args.only and args.only != f"{k}/{g}/{C_}":
            continue
        out_g = tuple(torch.empty(s, dtype=dt, device=dev) for s, dt in (((nq, k, g), torch.int64), ((nq, k, g), torch.float32),
                                                                         ((nq, k), torch.int32), ((nq, k), torch.int32),
                                                                         ((nq,), torch.uint8)))
        out_s = (torch.empty((nq, C_), dtype=torch.int64, device=dev), torch.empty((nq, C_), dtype=torch.float32, device=dev))
        run_grouped = lambda: ix.search_grouped_device(Qd, k, g, candidates=C_, out=out_g)      # noqa: E731
        run_plain = lambda: ix.search_batch_device(Qd, C_, out=out_s)                           # noqa: E731
        for _ in range(2):                                                                      # warm, both
            timed(run_grouped)
            timed(run_plain)
        tg, tp, tk = [], [], []
        for _ in range(args.reps):                                                              # alternating
            dt, res = timed(run_grouped)
            tg.append(dt)
            tk.append(ix.last_group_rows_us())
            dt, _ = timed(run_plain)
            tp.append(dt)
        complete = res[4].cpu().numpy()
        counts = res[3].cpu().numpy()
        row = dict(k=k, g=g, candidates=C_, queries=nq, complete_share=round(float(complete.mean()), 4),
                   mean_groups=round(float((counts > 0).sum(axis=1).mean()), 2),
                   mean_members=round(float(counts.sum(axis=1).mean()), 2),
                   grouped_ms_median=round(float(np.median(tg)) * 1e3, 3), grouped_ms_min=round(min(tg) * 1e3, 3),
                   grouped_ms_max=round(max(tg) * 1e3, 3), plain_ms_median=round(float(np.median(tp)) * 1e3, 3),
                   plain_ms_min=round(min(tp) * 1e3, 3), plain_ms_max=round(max(tp) * 1e3, 3),
                   group_kernel_us_median=round(float(np.median(tk)), 1), group_kernel_us_max=round(max(tk), 1), reps=args.reps)
        row["ratio_of_medians"] = round(row["grouped_ms_median"] / row["plain_ms_median"], 3)
        row["kernel_share_of_grouped"] = round(row["group_kernel_us_median"] / 1e3 / row["grouped_ms_median"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if not args.no_write:
        write_report(rows, cfg, n, dim, nq, args.reps, args.out)


def write_report(rows, cfg, n, dim, nq, reps, out):
    cols = ["k", "g", "candidates", "complete_share", "mean_groups", "mean_members", "grouped_ms_median", "grouped_ms_min",
            "grouped_ms_max", "plain_ms_median", "plain_ms_min", "plain_ms_max", "ratio_of_medians", "group_kernel_us_median",
            "group_kernel_us_max", "kernel_share_of_grouped"]
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    head = ("# Grouped search: search_grouped_device(k, g, candidates=C) against search_batch_device(k=C)\n\n"
            f"{cfg['label']}: {n:,} x {dim}, {cfg['bits']}-bit, batches of {nq:,} queries on the device, one process, the two "
            f"calls alternating, warm, both into preallocated outputs; median / min / max of {reps} runs each (host clock around "
            "calls that end in a device synchronise).  `plain` is the ungrouped call at the same C, which the grouped call "
            "contains; `group kernel us` is group_rows_kernel alone between two HIP events.  Keys: n / "
            f"{ROWS_PER_KEY} documents, each row in a random one.  scripts/grouped_sweep.py.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    old = open(out).read() if os.path.exists(out) else ""
    kept = old[old.index(KEEP):] if KEEP in old else KEEP + "\n"
    with open(out, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
