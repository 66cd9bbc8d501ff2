"""Added rows at the C2 shape (1M x 128, 4-bit, k = 10, 10,000-query search_batch_device batches): QPS with a tail of 0,
1k, 10k, 100k and 1M rows, the device time of a batch (kernel_us: all launches) and, from a kernel trace, of the tail's
scan and fold kernels apart; the wall time of add() for 1, 1,000 and 100,000 rows (the first add reallocates the resident
arrays, the second does not); compact() with a 100k tail against build + finalize of the same rows; and the tail size at
which a batch takes twice the time of t = 0 (interpolated between the measured sizes).

t = 0 against the parent commit: `--parent-lib PATH` names a library built from the parent's sources.  The t = 0 line is
then measured in fresh child processes, alternating this tree's library and the parent's (`--parent-reps` each), by this
same script -- it calls add() only when t > 0, so it runs on the parent's library unchanged.  The spread of the repeated
parent runs is recorded next to the figure; no percentage is assumed.

    python scripts/add_sweep.py [--workdir DIR] [--reps 5] [--parent-lib PATH] [--kernel-stats CSV] [--resource-usage TXT]
                                [--out profiles/add.md]
    rocprofv3 --kernel-trace --stats -d DIR -o add -- python scripts/add_sweep.py --trace 100000      # -> the CSV above

Every figure that could not be taken is written as "not measured"."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402

NM = "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=os.environ.get("CPH_BENCH_DIR", "/tmp/cph_bench"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "add.md"))
    ap.add_argument("--tails", default="0,1000,10000,100000,1000000")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-reps", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None, help="kernel stats CSV of a --trace run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--resource-usage", default=None,
                    help="text file with the scripts/resource_usage.py lines of the exact_scan / tail_ kernels, parent and this tree")
    ap.add_argument("--t0-child", action="store_true", help="measure t = 0 only and print one JSON line")
    ap.add_argument("--trace", type=int, default=None, help="run a few batches with this tail and exit (for a kernel trace)")
    ap.add_argument("--skip-lifecycle", action="store_true", help="leave out the add() / compact() timings")
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, nq, k, dim = cfg["n"], cfg["nq"], cfg["k"], cfg["dim"]

    import torch
    import cphnsw_mi355x
    path, info, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    Q = bench.make_queries(cfg, n, nq)
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    rng = np.random.default_rng(12)

    def load():
        ix = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
        if os.path.exists(path + ".native"):
            ix.load_native(path + ".native")
        else:
            ix.load(path)
        return ix

    def tail_rows(m):
        # rows like the base: the queries' distribution, so that tail rows do enter results
        return (Q[rng.integers(0, nq, m)] + rng.standard_normal((m, dim)).astype(np.float32) * np.float32(0.1)).astype(np.float32)

    def dev_qps(ix):
        torch.cuda.synchronize()
        for i in range(4):                                   # warm-up: scratch, the adaptive knobs
            ix.search_batch_device(Qd, k, stream=streams[i & 1])
        ix.synchronize()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for i in range(4):
                ix.search_batch_device(Qd, k, stream=streams[i & 1])
            ix.synchronize()
            t.append(nq * 4 / (time.perf_counter() - t0))
        ix.search_batch_device(Qd, k, stream=streams[0])     # one batch alone: its device time over all launches
        ix.synchronize()
        return float(np.median(t)), float(min(t)), float(max(t)), ix.last_search_stats()["kernel_us"]

    if args.t0_child:
        qps, lo, hi, us = dev_qps(load())
        print(json.dumps(dict(t0_child=True, lib="parent" if os.environ.get("CPH_LIB_PATH") else "this tree", qps_device=round(qps), qps_min=round(lo),
                              qps_max=round(hi), batch_kernel_us=us)), flush=True)
        return
    if args.trace is not None:
        ix = load()
        if args.trace:
            ix.add(tail_rows(args.trace))
        for i in range(6):
            ix.search_batch_device(Qd, k, stream=streams[i & 1])
        ix.synchronize()
        return

    rows = []
    for t in [int(x) for x in args.tails.split(",")]:
        ix = load()
        if t:
            ix.add(tail_rows(t))
        qps, lo, hi, us = dev_qps(ix)
        row = dict(tail_rows=t, qps_device=round(qps), qps_min=round(lo), qps_max=round(hi), batch_kernel_us=us,
                   batch_wall_ms=round(nq / qps * 1e3, 3))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ix
    # the tail size at which a batch takes twice the time of t = 0: linear between the two measured sizes around it
    twice = NM
    base_ms = rows[0]["batch_wall_ms"] if rows and rows[0]["tail_rows"] == 0 else None
    if base_ms:
        for a, b in zip(rows, rows[1:]):
            if a["batch_wall_ms"] < 2 * base_ms <= b["batch_wall_ms"]:
                f = (2 * base_ms - a["batch_wall_ms"]) / (b["batch_wall_ms"] - a["batch_wall_ms"])
                twice = int(round(a["tail_rows"] + f * (b["tail_rows"] - a["tail_rows"]), -3))
    print(json.dumps(dict(tail_rows_at_twice_the_batch_time=twice)), flush=True)

    life = []
    if not args.skip_lifecycle:
        ix = load()
        ix.search_batch(Q[:64], k)
        for m, what in ((1, "first add: the resident arrays are reallocated"), (1, "second add: they have room"), (1000, ""), (100000, "")):
            v = tail_rows(m)
            t0 = time.perf_counter()
            ix.add(v)
            life.append(dict(add_rows=m, add_ms=round((time.perf_counter() - t0) * 1e3, 3), note=what))
            print(json.dumps(life[-1]), flush=True)
        every = ix.get_vectors()
        t0 = time.perf_counter()
        ix.compact()
        t_compact = time.perf_counter() - t0
        del ix
        fresh = cphnsw_mi355x.CPIndex(dim, cfg["bits"], device=0)
        t0 = time.perf_counter()
        fresh.build(every)
        fresh.finalize()
        life.append(dict(rows=int(every.shape[0]), tail_rows=101002, compact_s=round(t_compact, 3),
                         build_finalize_s=round(time.perf_counter() - t0, 3)))
        print(json.dumps(life[-1]), flush=True)
        del fresh

    parent = []
    if args.parent_lib:
        for r in range(args.parent_reps):
            for lib in (None, args.parent_lib):
                env = dict(os.environ)
                env.pop("CPH_LIB_PATH", None)
                if lib:
                    env["CPH_LIB_PATH"] = lib
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--t0-child", "--workdir", args.workdir, "--reps", str(args.reps)],
                                     env=env, capture_output=True, text=True, timeout=600)
                line = [x for x in out.stdout.splitlines() if x.startswith('{"t0_child"')]
                if out.returncode != 0 or not line:
                    print(out.stderr[-2000:], file=sys.stderr)
                    continue
                parent.append(json.loads(line[-1]))
                print(json.dumps(parent[-1]), flush=True)

    kern = {}
    if args.kernel_stats and os.path.exists(args.kernel_stats):
        with open(args.kernel_stats) as fh:
            for r in csv.DictReader(fh):
                name = r.get("Name") or r.get("KernelName") or ""
                avg = r.get("AverageNs") or r.get("Average") or r.get("AverageNs ") or ""
                for key in ("tail_scan_kernel", "tail_fold_kernel", "exact_pad_kernel", "search_kernel"):
                    if key in name and avg:
                        kern.setdefault(key, []).append(dict(calls=r.get("Calls"), average_us=round(float(avg) / 1e3, 1)))

    cols = list(rows[0])
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(f"{r[c]:,}" if isinstance(r[c], int) else str(r[c]) for c in cols) + " |")
    ours = [p["qps_device"] for p in parent if p["lib"] == "this tree"]
    theirs = [p["qps_device"] for p in parent if p["lib"] != "this tree"]
    with open(args.out, "w") as fh:
        fh.write("# Added rows: 1M x 128, 4-bit, k = 10, 10,000-query search_batch_device batches\n\n")
        fh.write("Written by `scripts/add_sweep.py`.  QPS: median (min, max) of %d repetitions of four batches on two streams; "
                 "batch kernel us: the device time of ONE batch over all its launches (`last_search_stats`).\n\n" % args.reps)
        fh.write("\n".join(lines) + "\n\n")
        fh.write(f"Tail size at which a batch takes twice the time of t = 0 (linear between the measured sizes): {twice}\n\n")
        fh.write("## t = 0 against the parent commit\n\n")
        if ours and theirs:
            fh.write(f"Fresh processes, alternating, same session.  This tree: {sorted(ours)} QPS; parent: {sorted(theirs)} QPS "
                     f"(spread of the parent runs: {min(theirs):,} .. {max(theirs):,}).\n\n")
        else:
            fh.write(NM + "\n\n")
        fh.write("## Device time of the tail's kernels (kernel trace of `--trace`)\n\n")
        fh.write(("```\n" + json.dumps(kern, indent=1) + "\n```\n\n") if kern else NM + "\n\n")
        fh.write("## add() and compact()\n\n")
        fh.write(("```\n" + "\n".join(json.dumps(r) for r in life) + "\n```\n\n") if life else NM + "\n\n")
        fh.write("## Resource usage of the scan instantiations\n\nThe tail scan is the candidate loop of the exact scan "
                 "(`exact_scan_candidates`, `device_exact.h`) with a candidate source of its own "
                 "(`hipcc -Rpass-analysis=kernel-resource-usage`, `scripts/resource_usage.py`).\n\n")
        if args.resource_usage and os.path.exists(args.resource_usage):
            fh.write("```\n" + open(args.resource_usage).read().rstrip() + "\n```\n\n")
        else:
            fh.write(NM + "\n\n")
        fh.write("## Raw lines\n\n```\n" + "\n".join(json.dumps(r) for r in rows + parent) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
