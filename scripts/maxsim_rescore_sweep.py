"""Exact rescoring of multi-vector (MaxSim) search against the lower-bound call it follows: 1M x 128, 4-bit, cosine, T = 32
tokens per query, device batches of 1,000 queries, k = 10, in one process.  Two key columns over the same index: documents of
32 consecutive input rows (those of scripts/maxsim_sweep.py) and of 256.  Per column and R in {32, 128, 1024}:
search_maxsim_device(k, candidates=C, rescore=R) next to search_maxsim_device(k, candidates=C) on the same handle --
alternating, warm; median and spread of --reps runs each, host clock around calls that end in a device synchronise -- and
maxsim_rescore_scan_kernel alone between two HIP events (CPIndex.time_maxsim_rescore / last_maxsim_rescore_us) against its
VALU floor of 2 D flop per (token, allowed row) pair.  Also: the host build of the inverted key column
(prepare_maxsim_rescore, wall clock), the share of queries whose top-k keys differ from the lower-bound order, the mean of
certified, and the mean rise of the best key's score over its bound.
No target is fixed in advance.
    python scripts/maxsim_rescore_sweep.py [--reps 7] [--nq 1000] [--tokens 32] [--candidates 64] [--out profiles/maxsim_rescore.md]
Reuses bench.py's data generators (config c2); the index is built in the process.  Whatever the output file holds from the
line KEEP on (resource usage, the bench.py comparison, a hand-written reading of the numbers) is carried over."""
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

RESCORES = (32, 128, 1024)
DOC_ROWS = (32, 256)
PEAK_VALU_FP32_TFLOPS = 157.3                              # MI355X vector fp32 (FMA), the floor's denominator
KEEP = "<!-- below this line: written by hand, kept by scripts/maxsim_rescore_sweep.py -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nq", type=int, default=1_000)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--n", type=int, default=0, help="override the index size (rehearsals)")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim_rescore.md"))
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n, dim, nq, T, k, C_ = args.n or cfg["n"], cfg["dim"], args.nq, args.tokens, args.k, args.candidates

    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("maxsim_rescore_sweep.py measures on the GPU: no HIP device here")
    X = bench.make_base(cfg, n)
    Q = bench.make_queries(cfg, n, nq * T)
    ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0, metric="cosine")
    t0 = time.time()
    ix.build(X)
    ix.finalize()
    print(f"built n={n} in {time.time() - t0:.1f} s", flush=True)
    del X
    dev = torch.device("cuda", 0)
    Td = torch.from_numpy(Q).to(dev).view(nq, T, dim)
    ix.time_maxsim_rescore(True)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ix.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def outs(six):
        o = [torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
             torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k, T), dtype=torch.int64, device=dev),
             torch.empty((nq,), dtype=torch.int32, device=dev)]
        return o + [torch.empty((nq,), dtype=torch.int32, device=dev)] if six else o

    rows = []
    for doc_rows in DOC_ROWS:
        ix.set_labels(np.arange(n) // doc_rows, ids="input")
        ix.synchronize()
        t0 = time.perf_counter()
        ix.prepare_maxsim_rescore()
        build_ms = (time.perf_counter() - t0) * 1e3
        out_p = outs(False)
        run_plain = lambda: ix.search_maxsim_device(Td, k, candidates=C_, out=out_p)                  # noqa: E731
        for R in RESCORES:
            out_r = outs(True)
            run_resc = lambda: ix.search_maxsim_device(Td, k, candidates=C_, rescore=R, out=out_r)    # noqa: E731
            for _ in range(2):                                                                        # warm, both
                timed(run_resc)
                timed(run_plain)
            tr, tp, ts = [], [], []
            for _ in range(args.reps):                                                                # alternating
                dt, res = timed(run_resc)
                tr.append(dt)
                ts.append(ix.last_maxsim_rescore_us())
                dt, plain = timed(run_plain)
                tp.append(dt)
            res = [t.cpu().numpy() for t in res]
            plain = [t.cpu().numpy() for t in plain]
            low = [t.cpu().numpy() for t in ix.search_maxsim_device(Td, R, candidates=C_)]            # the candidates, for the floor
            pairs = float(low[4].sum()) * doc_rows * T                                                # (every row allowed, every token live)
            scan = float(np.median(ts))
            floor_us = 2.0 * dim * pairs / (PEAK_VALU_FP32_TFLOPS * 1e12) * 1e6
            differs = float(np.mean([not np.array_equal(res[0][q], plain[0][q]) for q in range(nq)]))
            lb_best = {q: dict(zip(low[0][q, :low[4][q]].tolist(), low[1][q, :low[4][q]])) for q in range(nq)}
            rise = float(np.mean([res[1][q, 0] - lb_best[q][int(res[0][q, 0])] for q in range(nq) if res[4][q]]))
            row = dict(doc_rows=doc_rows, rescore=R, tokens=T, candidates=C_, k=k, queries=nq,
                       rescored_ms_median=round(float(np.median(tr)) * 1e3, 3), rescored_ms_min=round(min(tr) * 1e3, 3),
                       rescored_ms_max=round(max(tr) * 1e3, 3), plain_ms_median=round(float(np.median(tp)) * 1e3, 3),
                       plain_ms_min=round(min(tp) * 1e3, 3), plain_ms_max=round(max(tp) * 1e3, 3),
                       scan_us_median=round(scan, 1), scan_us_min=round(min(ts), 1), scan_us_max=round(max(ts), 1),
                       pairs=int(pairs), valu_floor_us=round(floor_us, 1), scan_over_floor=round(scan / max(floor_us, 1e-9), 2),
                       mean_found_at_R=round(float(low[4].mean()), 2), top_k_differs=round(differs, 4),
                       mean_certified=round(float(res[5].mean()), 2), mean_rise_of_best=round(rise, 5),
                       key_rows_build_ms=round(build_ms, 1), reps=args.reps)
            row["ratio_of_medians"] = round(row["rescored_ms_median"] / row["plain_ms_median"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    ix.time_maxsim_rescore(False)
    if not args.no_write:
        write_report(rows, cfg, n, dim, nq, T, k, C_, args.reps, args.out)


def write_report(rows, cfg, n, dim, nq, T, k, C_, reps, out):
    cols = ["doc_rows", "rescore", "rescored_ms_median", "rescored_ms_min", "rescored_ms_max", "plain_ms_median", "plain_ms_min",
            "plain_ms_max", "ratio_of_medians", "scan_us_median", "scan_us_min", "scan_us_max", "pairs", "valu_floor_us", "scan_over_floor",
            "mean_found_at_R", "top_k_differs", "mean_certified", "mean_rise_of_best", "key_rows_build_ms"]
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    head = ("# Rescored multi-vector search: search_maxsim_device(k, candidates=C, rescore=R) against search_maxsim_device(k, candidates=C)\n\n"
            f"{cfg['label']}: {n:,} x {dim}, {cfg['bits']}-bit, metric cosine, T = {T} tokens per query (all live), k = {k}, C = {C_}, "
            f"batches of {nq:,} queries on the device, documents of `doc rows` consecutive input rows, one process, the two calls "
            f"alternating, warm, both into preallocated outputs; median / min / max of {reps} runs each (host clock around calls that "
            "end in a device synchronise).  `plain` is the lower-bound call the rescored one contains (at k, not at R).  `scan us` is "
            "maxsim_rescore_scan_kernel alone between two HIP events; `pairs` = (candidate keys found at R) x doc rows x T, "
            f"`valu floor us` = 2 D x pairs flop at {PEAK_VALU_FP32_TFLOPS} Tflop/s.  `top k differs`: the share of queries whose k "
            "keys are not the lower-bound call's k keys in the same order; `mean rise of best`: exact score minus lower bound of the "
            "best key; `key rows build ms`: prepare_maxsim_rescore on the host (download, sort, upload), once per column.  "
            "scripts/maxsim_rescore_sweep.py.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    old = open(out).read() if os.path.exists(out) else ""
    kept = old[old.index(KEEP):] if KEEP in old else KEEP + "\n"
    with open(out, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
