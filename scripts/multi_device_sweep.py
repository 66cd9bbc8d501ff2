"""In-process multi-device search at the C2 shape (1M x 128, 4-bit, k = 10, a 10k-query numpy search_batch): the
single-device handle against CPIndex(devices=[...]) -- devices=[0] (the wrapper's overhead), devices=[0, 0] (two
replicas on one GPU: one shard's copies can overlap the other's kernels) and, where the box shows more than one GPU,
devices = 0..G-1 for G = 1, 2, 4, 8.  The legs run alternately, `--runs` runs each, every run `--batches` back-to-back
batches; the median run's QPS is reported.  Every leg's results are checked byte for byte against the single-device
handle.  Reuses bench.py's data generators and its cached index file (same --workdir).
    python scripts/multi_device_sweep.py [--workdir DIR] [--runs 7] [--batches 10] [--out profiles/multi_device.md]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=os.environ.get("CPH_BENCH_DIR", "/tmp/cph_bench"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_device.md"))
    args = ap.parse_args()
    args.config = "c2"
    os.makedirs(args.workdir, exist_ok=True)
    cfg = bench.CONFIGS["c2"]
    n, nq, k = cfg["n"], cfg["nq"], cfg["k"]

    import torch
    import cphnsw_mi355x
    path, _, _ = bench.get_index_file(args, cfg, n, 0, 0, need_base=False)
    Q = bench.make_queries(cfg, n, nq)
    G = torch.cuda.device_count()
    legs = [("single device", None), ("devices=[0]", [0]), ("devices=[0, 0]", [0, 0])]
    if G > 1:
        legs += [(f"devices=0..{g - 1}", list(range(g))) for g in (2, 4, 8) if g <= G]

    def load(devs):
        ix = cphnsw_mi355x.CPIndex(cfg["dim"], cfg["bits"], device=0 if devs is None else None, devices=devs)
        t0 = time.perf_counter()
        if os.path.exists(path + ".native"):
            ix.load_native(path + ".native")
        else:
            ix.load(path)
        return ix, time.perf_counter() - t0

    idx, load_s, identical = {}, {}, {}
    ref = None
    for name, devs in legs:
        idx[name], load_s[name] = load(devs)
        ids, d = idx[name].search_batch(Q, k)          # warm-up; also the parity batch
        if ref is None:
            ref = (ids, d)
        identical[name] = bool(np.array_equal(ids, ref[0]) and d.tobytes() == ref[1].tobytes())
        print(f"[sweep] {name}: loaded in {load_s[name]:.1f} s, identical={identical[name]}", flush=True)

    qps = {name: [] for name, _ in legs}
    for r in range(args.runs):
        for name, _ in legs:                            # alternate the legs within every run
            ix = idx[name]
            t0 = time.perf_counter()
            for _ in range(args.batches):
                ix.search_batch(Q, k)
            qps[name].append(nq * args.batches / (time.perf_counter() - t0))
    single = float(np.median(qps["single device"]))
    rows = []
    for name, devs in legs:
        med = float(np.median(qps[name]))
        row = dict(leg=name, devices=devs, median_qps=round(med), min_qps=round(min(qps[name])),
                   max_qps=round(max(qps[name])), vs_single=round(med / single, 4), load_s=round(load_s[name], 1),
                   identical_to_single=identical[name])
        print(json.dumps(row), flush=True)
        rows.append(row)
    meta = dict(config="c2", n=n, nq=nq, k=k, bits=cfg["bits"], runs=args.runs, batches_per_run=args.batches,
                device_count=G, device_name=torch.cuda.get_device_name(0))
    lines = [f"device_count = {G} ({meta['device_name']}); C2 shape, {nq:,}-query numpy search_batch, k = {k}; "
             f"{args.runs} runs per leg (alternating), {args.batches} batches per run.", "",
             "| leg | median QPS | min | max | vs single | load s | byte-identical to single |", "|" + "---|" * 7]
    for r in rows:
        lines.append(f"| {r['leg']} | {r['median_qps']:,} | {r['min_qps']:,} | {r['max_qps']:,} | {r['vs_single']:.3f} | "
                     f"{r['load_s']} | {'yes' if r['identical_to_single'] else 'NO'} |")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n\n```\n" + json.dumps(meta) + "\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
