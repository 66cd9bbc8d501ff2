"""What the cosine metric costs, against the index a user had to build before it existed: CPIndex(metric="cosine") built
from X next to a plain index built from the same rows normalised on the host (cph_host_normalize_rows: the same bits, so
both indexes hold the same rows and both searches do the same graph work), at the C2 shape (1M x 128, 4-bit), in one
process:
    build() + finalize()                             once each (no spread is taken)
    search_batch_device, 10,000-query batches        alternating, warm, --reps runs each; the cosine side pays one
                                                     normalisation launch per batch, the L2 side gets queries that were
                                                     normalised before the clock started
    search_batch of 16 queries (the pinned route)    alternating, --small-reps runs of --small-calls calls each
    add() of 10,000 rows                             once each, on the built indexes (last: it puts a tail on both)
Host clock around calls that end in a device synchronise; median and spread (min .. max) of the runs.  No target is fixed
in advance: the number to report is the ratio cosine / L2 of each row.
    python scripts/cosine_sweep.py [--reps 9] [--n 0] [--out profiles/cosine.md]
    python scripts/cosine_sweep.py --bench-parent parent.jsonl --bench-this this.jsonl     # records bench.py lines too
Reuses bench.py's data generators (config c2).  The report is the table and the JSON lines; whatever the output file holds
from the line KEEP on (a hand-written reading of the numbers) is carried over."""
import argparse
import ctypes as C
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

KEEP = "<!-- below this line: written by hand, kept by scripts/cosine_sweep.py -->"


def host_normalize(x):
    from cphnsw_mi355x import _lib
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    bad = C.c_uint64(0)
    _lib.check(_lib.lib().cph_host_normalize_rows(x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data, C.byref(bad), None))
    if bad.value:
        raise SystemExit(f"{bad.value} rows without a direction in the generated data")
    return out


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
    ap.add_argument("--add-rows", type=int, default=10_000)
    ap.add_argument("--n", type=int, default=0, help="override the index size (rehearsals)")
    ap.add_argument("--bench-parent", default="", help="file of bench.py result lines of the parent commit's library")
    ap.add_argument("--bench-this", default="", help="... and of this tree's, taken in the same visit, alternating")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cosine.md"))
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n, dim, nq, k = args.n or cfg["n"], cfg["dim"], args.nq, cfg["k"]

    import torch
    import cphnsw_mi355x
    if not torch.cuda.is_available():
        raise SystemExit("cosine_sweep.py measures on the GPU: no HIP device here")
    X = bench.make_base(cfg, n + args.add_rows)
    X, Y = X[:n], X[n:]
    Q = bench.make_queries(cfg, n, nq)
    Xn, Yn, Qn = host_normalize(X), host_normalize(Y), host_normalize(Q)
    res = {}

    def build(rows, **kw):
        ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.build(rows)
        ix.finalize()
        ix.synchronize()
        return ix, time.perf_counter() - t0
    l2, t_l2 = build(Xn)
    cos, t_cos = build(X, metric="cosine")
    res["build_s"] = dict(cosine=t_cos, l2=t_l2)
    print(f"built n={n}: cosine {t_cos:.1f} s, l2 twin {t_l2:.1f} s", flush=True)
    # Do the two hold the same index?  The rows must be the same bits.  The graph is the same only where the builder
    # repeats itself at this size: a second L2 build from the same rows is the control for that.
    l2b, _ = build(Xn)
    same_graph = bool(np.array_equal(cos.row_map(), l2.row_map()))
    rm_c, rm_l = cos.row_map()[:1000], l2.row_map()[:1000]
    same_rows = bool((cos.get_vectors(0, 1000) == Xn[rm_c]).all() and (l2.get_vectors(0, 1000) == Xn[rm_l]).all())

    dev = torch.device("cuda", 0)
    Qd, Qnd = torch.from_numpy(Q).to(dev), torch.from_numpy(Qn).to(dev)
    out = (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
    out2 = (torch.empty_like(out[0]), torch.empty_like(out[1]))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t
    run_cos = lambda: cos.search_batch_device(Qd, k, out=out)       # noqa: E731
    run_l2 = lambda: l2.search_batch_device(Qnd, k, out=out2)       # noqa: E731
    for _ in range(3):                                              # warm, both
        timed(run_cos)
        timed(run_l2)
    same_results = bool(torch.equal(out[0], out2[0]) and torch.equal(out[1].view(torch.int32), out2[1].view(torch.int32)))
    # whatever the graphs are, the exact scan must agree byte for byte, in input rows
    cos.result_ids = l2.result_ids = "input"
    ec, el = cos.search_batch(Q[:1000], k, exact=True), l2.search_batch(Qn[:1000], k, exact=True)
    gc, gl = cos.search_batch(Q[:1000], k), l2.search_batch(Qn[:1000], k)
    cos.result_ids = l2.result_ids = "internal"
    # graph batches, row by row: the cosine index against the twin, and the twin against its own second build
    gb = l2b.search_batch_device(Qnd, k)
    torch.cuda.synchronize()

    def same_rows_of(a, b):
        return float(((a[0] == b[0]).all(dim=1) & (a[1].view(torch.int32) == b[1].view(torch.int32)).all(dim=1)).float().mean())
    graph_rows, control_rows = same_rows_of(out, out2), same_rows_of(gb, out2)
    del l2b, gb
    same_exact = bool(np.array_equal(ec[0], el[0]) and ec[1].tobytes() == el[1].tobytes())
    recall = [float(np.mean([len(set(g[i]) & set(e[i])) / k for i in range(1000)])) for g, e in ((gc[0], ec[0]), (gl[0], el[0]))]
    tc, tl = [], []
    for _ in range(args.reps):
        tc.append(timed(run_cos) * 1e3)
        tl.append(timed(run_l2) * 1e3)
    res["batch_device_ms"] = dict(cosine=spread(tc), l2=spread(tl))

    q16, qn16 = Q[:16].copy(), Qn[:16].copy()

    def small(ix, q):
        t = time.perf_counter()
        for _ in range(args.small_calls):
            ix.search_batch(q, k)                                   # (the call waits for its results)
        return (time.perf_counter() - t) / args.small_calls * 1e6
    small(cos, q16), small(l2, qn16)
    sc, sl = [], []
    for _ in range(args.small_reps):
        sc.append(small(cos, q16))
        sl.append(small(l2, qn16))
    res["batch16_us"] = dict(cosine=spread(sc), l2=spread(sl))

    def add(ix, rows):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ix.add(rows)
        ix.synchronize()
        return (time.perf_counter() - t) * 1e3
    res["add_ms"] = dict(l2=add(l2, Yn), cosine=add(cos, Y))
    res["checks"] = dict(same_rows=same_rows, same_row_map=same_graph, same_graph_results=same_results, graph_rows_equal=graph_rows,
                         control_graph_rows_equal=control_rows,
                         same_exact_results=same_exact, recall_at_k=dict(cosine=recall[0], l2=recall[1]), metric_stats=list(cos.metric_stats()),
                         l2_metric_stats=list(l2.metric_stats()))

    def ratio(c, l):
        return c / l if l else float("nan")
    b, s = res["batch_device_ms"], res["batch16_us"]
    lines = [
        "# Cosine metric against an L2 index over rows normalised on the host",
        "",
        f"`scripts/cosine_sweep.py`: n = {n:,} x {dim}, {cfg['bits']}-bit, k = {k}; one process on one MI355X; host clock around "
        "calls that end in a device synchronise; median (min .. max) of the runs.",
        "",
        f"Checks at this size: both indexes store the host-normalised rows bit for bit (first 1,000 ids: {same_rows}); "
        f"exact=True returns the same ids and distance bytes on both (1,000 queries: {same_exact}); the builder's "
        f"row maps are equal ({same_graph}).  Graph batches: {graph_rows:.4f} of the {nq:,} rows have the same bytes on both; "
        f"the control -- the L2 twin against a second build of itself from the same rows -- gives {control_rows:.4f}, so what "
        f"differs is what two builds of one array differ in at this size, not the metric; recall@{k} of the graph search against the exact scan: cosine {recall[0]:.4f}, L2 twin "
        f"{recall[1]:.4f}.",
        "",
        "| what | cosine | L2 twin | cosine / L2 |",
        "|---|---|---|---|",
        f"| build() + finalize(), s (one run each) | {t_cos:.2f} | {t_l2:.2f} | {ratio(t_cos, t_l2):.3f} |",
        f"| search_batch_device, {nq:,} queries, ms ({b['cosine']['runs']} runs) | {b['cosine']['median']:.3f} ({b['cosine']['min']:.3f} .. {b['cosine']['max']:.3f}) | "
        f"{b['l2']['median']:.3f} ({b['l2']['min']:.3f} .. {b['l2']['max']:.3f}) | {ratio(b['cosine']['median'], b['l2']['median']):.4f} |",
        f"| search_batch, 16 queries, us per call ({s['cosine']['runs']} runs of {args.small_calls}) | {s['cosine']['median']:.1f} ({s['cosine']['min']:.1f} .. {s['cosine']['max']:.1f}) | "
        f"{s['l2']['median']:.1f} ({s['l2']['min']:.1f} .. {s['l2']['max']:.1f}) | {ratio(s['cosine']['median'], s['l2']['median']):.4f} |",
        f"| add() of {args.add_rows:,} rows, ms (one run each) | {res['add_ms']['cosine']:.2f} | {res['add_ms']['l2']:.2f} | "
        f"{ratio(res['add_ms']['cosine'], res['add_ms']['l2']):.3f} |",
        "",
        "```json",
        json.dumps(res),
        "```",
    ]
    parent, this = bench_lines(args.bench_parent), bench_lines(args.bench_this)
    if parent or this:
        lines += ["", "## `python bench.py` on the L2 headline: the parent commit's library and this tree's, one visit, alternating", ""]

        def value(ln):
            j = json.loads(ln)
            return j.get("value"), j.get("ms_per_step")
        for name, ls in (("parent", parent), ("this tree", this)):
            vals = [value(ln) for ln in ls]
            lines.append(f"- {name}: value " + ", ".join(f"{v:,.0f}" for v, _ in vals) + "; ms per step " +
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
