"""Diversified search against the plain call it is built on, at the C2 shape (1M x 128, 4-bit, 10,000-query device
batches), in one process: search_diverse_device(k, lam, candidates=C) next to search_batch_device(k=C) on the same handle
and queries -- the call a user would otherwise make before re-ranking on the host -- alternating, warm; median and spread
of --reps runs each, host clock around calls that end in a device synchronise.  The re-ranking kernel alone is timed with
HIP events (CPIndex.time_diverse / last_diverse_rows_us), median over the same runs, and held against its byte model:
C x D x 4 bytes per query from HBM once, (k - 1) x C x D x 4 of re-reads.
No target is fixed in advance: the numbers to report are the ratio to the plain call at the same C, the kernel's time
against the two terms of the byte model, and which of them bounds it.
    python scripts/diverse_sweep.py [--reps 7] [--nq 10000] [--lam 0.5] [--out profiles/diverse_search.md]
    python scripts/diverse_sweep.py --only 10/64 --reps 3 --no-write       # one case, for a kernel trace of its own
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

CASES = ((10, 64), (10, 128), (10, 1024), (100, 1024))       # (k, C)
KEEP = "<!-- below this line: written by hand, kept by scripts/diverse_sweep.py -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--n", type=int, default=0, help="override the index size (rehearsals)")
    ap.add_argument("--only", default="", help="k/C of the one case to run, e.g. 10/64")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_search.md"))
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n, dim, nq, lam = args.n or cfg["n"], cfg["dim"], args.nq, args.lam

    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("diverse_sweep.py measures on the GPU: no HIP device here")
    X = bench.make_base(cfg, n)
    Q = bench.make_queries(cfg, n, nq)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
    t0 = time.time()
    ix.build(X)
    ix.finalize()
    print(f"built n={n} in {time.time() - t0:.1f} s", flush=True)
    del X
    D = 1 << (dim - 1).bit_length()
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    ix.time_diverse(True)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ix.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    rows = []
    for (k, C_) in CASES:
        if args.only and args.only != f"{k}/{C_}":
            continue
        out_d = (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                 torch.empty((nq, k), dtype=torch.float32, device=dev))
        out_s = (torch.empty((nq, C_), dtype=torch.int64, device=dev), torch.empty((nq, C_), dtype=torch.float32, device=dev))
        run_diverse = lambda: ix.search_diverse_device(Qd, k, lam, candidates=C_, out=out_d)      # noqa: E731
        run_plain = lambda: ix.search_batch_device(Qd, C_, out=out_s)                             # noqa: E731
        for _ in range(2):                                                                        # warm, both
            timed(run_diverse)
            timed(run_plain)
        td, tp, tk = [], [], []
        for _ in range(args.reps):                                                                # alternating
            dt, res = timed(run_diverse)
            td.append(dt)
            tk.append(ix.last_diverse_rows_us())
            dt, plain = timed(run_plain)
            tp.append(dt)
        picks = res[0].cpu().numpy()
        first_k = plain[0][:, :k].cpu().numpy()
        once, again = nq * C_ * D * 4, nq * (k - 1) * C_ * D * 4
        kern = float(np.median(tk))
        row = dict(k=k, candidates=C_, lam=lam, queries=nq,
                   picks_outside_first_k=round(float((picks[:, :, None] != first_k[:, None, :]).all(axis=2).mean()), 4),
                   diverse_ms_median=round(float(np.median(td)) * 1e3, 3), diverse_ms_min=round(min(td) * 1e3, 3),
                   diverse_ms_max=round(max(td) * 1e3, 3), plain_ms_median=round(float(np.median(tp)) * 1e3, 3),
                   plain_ms_min=round(min(tp) * 1e3, 3), plain_ms_max=round(max(tp) * 1e3, 3),
                   kernel_us_median=round(kern, 1), kernel_us_max=round(max(tk), 1),
                   first_read_gb=round(once / 1e9, 3), reread_gb=round(again / 1e9, 3),
                   first_read_tb_s=round(once / kern / 1e6, 3), all_reads_tb_s=round((once + again) / kern / 1e6, 3), reps=args.reps)
        row["ratio_of_medians"] = round(row["diverse_ms_median"] / row["plain_ms_median"], 3)
        row["kernel_share_of_diverse"] = round(kern / 1e3 / row["diverse_ms_median"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    ix.time_diverse(False)
    if not args.no_write:
        write_report(rows, cfg, n, dim, nq, lam, args.reps, args.out)


def write_report(rows, cfg, n, dim, nq, lam, reps, out):
    cols = ["k", "candidates", "picks_outside_first_k", "diverse_ms_median", "diverse_ms_min", "diverse_ms_max",
            "plain_ms_median", "plain_ms_min", "plain_ms_max", "ratio_of_medians", "kernel_us_median", "kernel_us_max",
            "kernel_share_of_diverse", "first_read_gb", "reread_gb", "first_read_tb_s", "all_reads_tb_s"]
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    head = ("# Diversified search: search_diverse_device(k, lam, candidates=C) against search_batch_device(k=C)\n\n"
            f"{cfg['label']}: {n:,} x {dim}, {cfg['bits']}-bit, lam = {lam}, batches of {nq:,} queries on the device, one process, the "
            f"two calls alternating, warm, both into preallocated outputs; median / min / max of {reps} runs each (host clock "
            "around calls that end in a device synchronise).  `plain` is the search at the same C, which the diverse call "
            "contains; `kernel us` is diverse_rows_kernel alone between two HIP events.  Byte model of the kernel for the whole batch: "
            "`first read` = queries x C x D x 4 (every candidate row once), `reread` = queries x (k - 1) x C x D x 4 (every later "
            "pass); `first read tb s` and `all reads tb s` are those bytes over the kernel's median time.  `picks outside first "
            "k`: the share of picks that the plain search at k would not have returned.  scripts/diverse_sweep.py.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    old = open(out).read() if os.path.exists(out) else ""
    kept = old[old.index(KEEP):] if KEEP in old else KEEP + "\n"
    with open(out, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
