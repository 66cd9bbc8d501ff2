"""What the inner-product metric costs, against a plain L2 index at the C2 shape (1M x 128, 4-bit), in one process:
    (a) CPIndex(127, metric="ip") over the first 127 columns: stored width 128, D = 128, the L2 index's own widths -- what
        is left is the cost of the two extra launches per batch (augmented queries in front, scores behind);
    (b) CPIndex(128, metric="ip") over all 128 columns: stored width 129, D = 256 -- the cost of the doubled padding on
        top of the launches.
Both against CPIndex(128) over the same rows, which answers another question (squared L2) with the same kernels, and
against the L2 twin: CPIndex(dim + 1) over the rows augmented on the host (cph_host_ip_augment: the same bits), asked
with [q, 0] made before the clock started -- the same graph walk, so IP / twin is the cost of the two launches alone:
    build() + finalize()                             once each (no spread is taken)
    search_batch_device, 10,000-query batches        the IP index and the L2 index alternating, warm, --reps runs each
    search_batch of 16 queries (the pinned route)    alternating, --small-reps runs of --small-calls calls each
Host clock around calls that end in a device synchronise; median and spread (min .. max) of the runs.  No target is fixed
in advance: the number to report is the ratio IP / L2 of each row.  The three indexes hold different graphs (other
widths, another metric), so the ratios compare workloads of the same shape, not the same graph walk; the expansions per
query of each are printed next to them.
    python scripts/ip_sweep.py [--reps 9] [--n 0] [--out profiles/inner_product.md]
    python scripts/ip_sweep.py --bench-parent parent.jsonl --bench-this this.jsonl     # records bench.py lines too
Reuses bench.py's data generators (config c2).  The report is the table and the JSON lines; whatever the output file holds
from the line KEEP on (a hand-written reading of the numbers) is carried over."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))

import bench  # noqa: E402

KEEP = "<!-- below this line: written by hand, kept by scripts/ip_sweep.py -->"


def host_augment(x, mode, m2=0.0):
    import ctypes as C
    from cphnsw_mi355x import _lib
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty((x.shape[0], x.shape[1] + 1), np.float32)
    c = np.empty(x.shape[0], np.float32)
    used = C.c_float(0.0)
    cnt = (C.c_uint64 * 3)()
    _lib.check(_lib.lib().cph_host_ip_augment(x.ctypes.data, x.shape[0], x.shape[1], mode, float(m2), out.ctypes.data, c.ctypes.data,
                                              C.byref(used), cnt))
    if cnt[0] or cnt[1]:
        raise SystemExit("bad rows in the generated data")
    return out, float(used.value)


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=len(v))


def bench_lines(path):
    if not path:
        return []
    return [ln.strip() for ln in open(path) if ln.strip().startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--small-reps", type=int, default=9)
    ap.add_argument("--small-calls", type=int, default=200)
    ap.add_argument("--n", type=int, default=0, help="override the index size (rehearsals)")
    ap.add_argument("--bench-parent", default="", help="file of bench.py result lines of the parent commit's library")
    ap.add_argument("--bench-this", default="", help="... and of this tree's, taken in the same visit, alternating")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inner_product.md"))
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n, dim, nq, k = args.n or cfg["n"], cfg["dim"], args.nq, cfg["k"]

    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("ip_sweep.py measures on the GPU: no HIP device here")
    X = bench.make_base(cfg, n)
    Q = bench.make_queries(cfg, n, nq)
    dev = torch.device("cuda", 0)

    def build(rows, **kw):
        ix = cphnsw_mi355x.CPIndex(rows.shape[1], cfg["bits"], device=0, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.build(rows)
        ix.finalize()
        ix.synchronize()
        return ix, time.perf_counter() - t0

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    l2, t_l2 = build(X)
    Qd = torch.from_numpy(Q).to(dev)
    out_l2 = (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
    run_l2 = lambda: l2.search_batch_device(Qd, k, out=out_l2)       # noqa: E731
    res, rows_md, twin_md = {}, [], []
    for name, d_ip in (("a", dim - 1), ("b", dim)):
        Xi, Qi = np.ascontiguousarray(X[:, :d_ip]), np.ascontiguousarray(Q[:, :d_ip])
        ip, t_ip = build(Xi, metric="ip")
        print(f"case ({name}) built n={n}: ip dim {d_ip} {t_ip:.1f} s, l2 dim {dim} {t_l2:.1f} s", flush=True)
        Qid = torch.from_numpy(Qi).to(dev)
        out_ip = (torch.empty_like(out_l2[0]), torch.empty_like(out_l2[1]))
        run_ip = lambda: ip.search_batch_device(Qid, k, out=out_ip)  # noqa: E731
        Xa, m2 = host_augment(Xi, 1)
        Qa, _ = host_augment(Qi, 2, m2)
        tw, t_tw = build(Xa)
        del Xa
        Qad = torch.from_numpy(Qa).to(dev)
        out_tw = (torch.empty_like(out_l2[0]), torch.empty_like(out_l2[1]))
        run_tw = lambda: tw.search_batch_device(Qad, k, out=out_tw)  # noqa: E731
        for _ in range(3):                                           # warm, all
            timed(run_ip)
            timed(run_tw)
            timed(run_l2)
        same_ids = float((out_ip[0] == out_tw[0]).all(dim=1).float().mean())
        exp_ip = ip.last_search_stats()["expansions"] / nq
        timed(run_l2)
        exp_l2 = l2.last_search_stats()["expansions"] / nq
        # what the scores are: -(q.x) of the returned rows, against float64 on a sample
        ip.result_ids = "input"
        ei, ed = ip.search_batch(Qi[:200], k, exact=True)
        ip.result_ids = "internal"
        t64 = -np.einsum("qd,qkd->qk", Qi[:200].astype(np.float64), Xi[ei].astype(np.float64))
        score_err = float(np.abs(ed - t64).max())
        ti, tl, tt = [], [], []
        for _ in range(args.reps):
            ti.append(timed(run_ip) * 1e3)
            tt.append(timed(run_tw) * 1e3)
            tl.append(timed(run_l2) * 1e3)
        q16, qi16 = Q[:16].copy(), Qi[:16].copy()

        def small(ix, q):
            t = time.perf_counter()
            for _ in range(args.small_calls):
                ix.search_batch(q, k)                                # (the call waits for its results)
            return (time.perf_counter() - t) / args.small_calls * 1e6
        qa16 = Qa[:16].copy()
        small(ip, qi16), small(tw, qa16), small(l2, q16)
        si, sl, st = [], [], []
        for _ in range(args.small_reps):
            si.append(small(ip, qi16))
            st.append(small(tw, qa16))
            sl.append(small(l2, q16))
        r = dict(dim=d_ip, stored=d_ip + 1, build_s=dict(ip=t_ip, l2=t_l2), batch_device_ms=dict(ip=spread(ti), twin=spread(tt), l2=spread(tl)),
                 batch16_us=dict(ip=spread(si), twin=spread(st), l2=spread(sl)), twin_build_s=t_tw, graph_rows_with_the_twin_s_ids=same_ids, expansions_per_query=dict(ip=exp_ip, l2=exp_l2),
                 exact_score_max_abs_err=score_err, ip_bound=ip.ip_bound, metric_stats=list(ip.metric_stats()),
                 l2_metric_stats=list(l2.metric_stats()))
        res[name] = r
        b, s = r["batch_device_ms"], r["batch16_us"]
        D = 1
        while D < d_ip + 1:
            D *= 2
        rows_md += [
            f"| ({name}) dim {d_ip}, stored {d_ip + 1}, D {D}: build() + finalize(), s (one run each) | {t_ip:.2f} | {t_l2:.2f} | {t_ip / t_l2:.3f} |",
            f"| ({name}) search_batch_device, {nq:,} queries, ms ({b['ip']['runs']} runs) | {b['ip']['median']:.3f} ({b['ip']['min']:.3f} .. "
            f"{b['ip']['max']:.3f}) | {b['l2']['median']:.3f} ({b['l2']['min']:.3f} .. {b['l2']['max']:.3f}) | "
            f"{b['ip']['median'] / b['l2']['median']:.4f} |",
            f"| ({name}) search_batch, 16 queries, us per call ({s['ip']['runs']} runs of {args.small_calls}) | {s['ip']['median']:.1f} "
            f"({s['ip']['min']:.1f} .. {s['ip']['max']:.1f}) | {s['l2']['median']:.1f} ({s['l2']['min']:.1f} .. {s['l2']['max']:.1f}) | "
            f"{s['ip']['median'] / s['l2']['median']:.4f} |",
            f"| ({name}) expansions per query of the 10,000-query batch | {exp_ip:.1f} | {exp_l2:.1f} | {exp_ip / exp_l2:.3f} |",
        ]
        twin_md += [
            f"| ({name}) search_batch_device, {nq:,} queries, ms | {b['ip']['median']:.3f} ({b['ip']['min']:.3f} .. {b['ip']['max']:.3f}) | "
            f"{b['twin']['median']:.3f} ({b['twin']['min']:.3f} .. {b['twin']['max']:.3f}) | {b['ip']['median'] / b['twin']['median']:.4f} |",
            f"| ({name}) search_batch, 16 queries, us per call | {s['ip']['median']:.1f} ({s['ip']['min']:.1f} .. {s['ip']['max']:.1f}) | "
            f"{s['twin']['median']:.1f} ({s['twin']['min']:.1f} .. {s['twin']['max']:.1f}) | {s['ip']['median'] / s['twin']['median']:.4f} |",
            f"| ({name}) rows of the 10,000-query batch with the twin's ids | {same_ids:.4f} | | |",
        ]
        del ip, tw, Qid, Qad, out_ip, out_tw

    lines = [
        "# Inner-product metric against a plain L2 index of the same shape",
        "",
        f"`scripts/ip_sweep.py`: n = {n:,} x {dim} (case a: its first {dim - 1} columns), {cfg['bits']}-bit, k = {k}; one process on one "
        "MI355X; host clock around calls that end in a device synchronise; median (min .. max) of the runs; the IP index and the L2 "
        "index alternate.  The L2 column is CPIndex(128) over the same rows in both cases.",
        "",
        "| what | IP | L2, dim 128 | IP / L2 |",
        "|---|---|---|---|",
    ] + rows_md + [
        "",
        "Against the L2 twin (CPIndex(dim + 1) over the host-augmented rows, asked with [q, 0]): the same walk, so the ratio is the "
        "cost of the two extra launches.",
        "",
        "| what | IP | L2 twin | IP / twin |",
        "|---|---|---|---|",
    ] + twin_md + ["", "```json", json.dumps(res), "```"]
    parent, this = bench_lines(args.bench_parent), bench_lines(args.bench_this)
    if parent or this:
        lines += ["", "## `python bench.py` on the L2 headline: the parent commit's library and this tree's, one visit, alternating", ""]

        def value(ln):
            j = json.loads(ln)
            return j.get("value"), j.get("ms_per_step")
        for name, ls in (("parent", parent), ("this tree", this)):
            vals = [value(ln) for ln in ls]
            if vals:
                lines.append(f"- {name}: value " + ", ".join(f"{v:,.0f}" for v, _ in vals) + f" (median {statistics.median(v for v, _ in vals):,.0f}, "
                             f"spread {max(v for v, _ in vals) - min(v for v, _ in vals):,.0f}); ms per step " +
                             ", ".join(f"{m:.4f}" for _, m in vals))
        lines += ["", "The last line of each:", "", "```json"] + parent[-1:] + this[-1:] + ["```"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.no_write:
        return
    kept = ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if KEEP in old:
            kept = old[old.index(KEEP):]
    with open(args.out, "w") as f:
        f.write(text + "\n" + (kept or KEEP + "\n"))


if __name__ == "__main__":
    main()
