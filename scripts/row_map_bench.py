"""Cost of results in input rows and of the row-space filter on the C2 workload (profiles/row_map.md).

    python scripts/row_map_bench.py [--rounds 7] [--steps 40] [--workdir /tmp/cph_row_map]

Builds the C2 index of bench.py (same generators; cached as a native file WITH its row map in --workdir), then
  * alternates `result_ids = "internal"` and `"input"` on one handle, `rounds` times: 10,000-query
    search_batch_device batches rotating over four streams, the step bench.py times; prints q/s of every run, the
    median and the min-max range of both modes;
  * times cph_filter_create against cph_filter_create_rows (upload + conversion kernel + wait) on a 50 % mask;
  * checks that both modes returned the same rows (ids mapped through row_map(), distances byte-identical).
One JSON line at the end."""
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


def main():
    import torch
    import bench
    import cphnsw_mi355x
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-index", type=int, default=0)
    ap.add_argument("--workdir", default="/tmp/cph_row_map")
    args = ap.parse_args()
    cfg = bench.CONFIGS["c2"]
    n = args.n_index or cfg["n"]
    os.makedirs(args.workdir, exist_ok=True)
    path = os.path.join(args.workdir, f"c2_{n}.native")
    ix = cphnsw_mi355x.CPIndex(cfg["dim"], cfg["bits"], device=0)
    if os.path.exists(path):
        ix.load_native(path)
    else:
        t0 = time.time()
        ix.build(bench.make_base(cfg, n))
        ix.finalize()
        print(f"built n={n} in {time.time() - t0:.1f} s", file=sys.stderr)
        ix.save_native(path)
    assert ix.has_row_map
    rm = ix.row_map()
    nq, k = cfg["nq"], cfg["k"]
    dev = torch.device("cuda:0")
    q = torch.from_numpy(bench.make_queries(cfg, n, nq)).to(dev)
    streams = [torch.cuda.Stream(dev) for _ in range(4)]
    outs = [(torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
            for _ in streams]
    ix.set_batch_sets(len(streams))

    def run(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            s = i % len(streams)
            ix.search_batch_device(q, k, out=outs[s], stream=streams[s])
        torch.cuda.synchronize()
        return nq * steps / (time.perf_counter() - t0)

    rates = {"internal": [], "input": []}
    last = {}
    for r in range(args.rounds):
        for mode in ("internal", "input"):
            ix.result_ids = mode
            run(args.warmup)
            rates[mode].append(run(args.steps))
            last[mode] = (outs[(args.steps - 1) % len(streams)][0].cpu().numpy(), outs[(args.steps - 1) % len(streams)][1].cpu().numpy())
            print(f"round {r} {mode:8s} {rates[mode][-1]:12.0f} q/s", file=sys.stderr)
    ii, di = last["internal"]
    ir, dr = last["input"]
    same = bool(np.array_equal(ir, np.where(ii >= 0, rm[np.maximum(ii, 0)], -1)) and di.tobytes() == dr.tobytes())

    # filter creation: internal bitmap (upload) against input-row bitmap (upload + conversion through the row map)
    mask = np.random.default_rng(0).random(n) < 0.5
    t_create = {"internal": [], "input": []}
    for _ in range(args.rounds + 1):
        for space in ("internal", "input"):
            t0 = time.perf_counter()
            f = ix.make_filter(mask, ids=space)
            t_create[space].append(time.perf_counter() - t0)
            f.close()
    words = cphnsw_mi355x.index.pack_allowed_bits(mask)
    import ctypes as C
    from cphnsw_mi355x import _lib
    t_abi = {}
    for name in ("cph_filter_create", "cph_filter_create_rows"):      # the C call alone, without numpy's bit packing
        ts = []
        for _ in range(args.rounds + 1):
            h = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(getattr(_lib.lib(), name)(ix._h, words.ctypes.data, n, C.byref(h)))
            ts.append(time.perf_counter() - t0)
            _lib.check(_lib.lib().cph_filter_destroy(h))
        t_abi[name] = ts[1:]

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": [round(x, 1) for x in v]}
    print(json.dumps({"n": n, "nq": nq, "k": k, "steps": args.steps, "rounds": args.rounds,
                      "qps": {m: summary(v) for m, v in rates.items()},
                      "input_equals_mapped_internal": same,
                      "filter_create_ms": {s: 1e3 * statistics.median(v[1:]) for s, v in t_create.items()},
                      "filter_create_abi_ms": {s: {"median": 1e3 * statistics.median(v), "min": 1e3 * min(v), "max": 1e3 * max(v)}
                                               for s, v in t_abi.items()}}))
    assert same


if __name__ == "__main__":
    main()
