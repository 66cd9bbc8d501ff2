"""Exhaustive int8 rescoring (search_rescored(..., candidates="all")) against the two-stage call: 1M rows, dim_full 256 and
1,024, device batches of 16, 128 and 1,000 queries, k = 10, one process, the calls alternating, warm.

Data: the prefix-trained rows of scripts/rescore_sweep.py, indexed on their first 128 coordinates (4-bit).
  (a) the scan kernel alone (CPIndex.time_rescored_all / last_rescored_all_us), median of --reps, against its two floors:
      bytes  ceil(n / 128) x object bytes / 6.29 TB/s (every query tile streams the object once)
      MACs   2 x n_pad x size x K_pad int8 MACs at the rate of a bare v_mfma_i32_32x32x32_i8 loop measured in this process
             (cph_debug_mfma_i8_rate)
  (b) the call next to search_rescored_device(candidates=64 / 256 / 1024) on the same handle and queries
  (c) recall@10 of both against float64 brute force at full width (dim_full 1,024)
No target is fixed in advance.
    python scripts/rescore_all_sweep.py [--reps 5] [--out profiles/rescored_all.md]
    python scripts/rescore_all_sweep.py --n 100000 --no-write        # a rehearsal"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from rescore_sweep import COPY_TB_S, DIM, DIM_FULL, BITS, K, brute_force, make_data, recall      # noqa: E402

BATCHES = (16, 128, 1000)
CS = (64, 256, 1024)
KEEP = "<!-- below this line: written by hand, kept by scripts/rescore_all_sweep.py -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescored_all.md"))
    args = ap.parse_args()
    import torch
    import cphnsw_mi355x
    from cphnsw_mi355x import _lib
    if not torch.cuda.is_available():
        raise SystemExit("rescore_all_sweep.py measures on the GPU: no HIP device here")
    dev, n, nq = torch.device("cuda", 0), args.n, max(BATCHES)
    Xd, FQd = make_data(torch, n, nq, dev)
    truth = brute_force(torch, Xd, FQd, K)
    X = Xd.cpu().numpy()
    del Xd
    torch.cuda.empty_cache()
    ix = cphnsw_mi355x.CPIndex(DIM, BITS, device=0)
    t0 = time.time()
    ix.build(np.ascontiguousarray(X[:, :DIM]))
    ix.finalize()
    ix.result_ids = "input"
    print(f"built n={n} in {time.time() - t0:.1f} s", flush=True)
    rate = C.c_double()
    _lib.check(_lib.lib().cph_debug_mfma_i8_rate(ix._h, 20000, C.byref(rate)))
    print(json.dumps(dict(mfma_i8_macs_per_s=rate.value)), flush=True)
    ix.time_rescored_all(True)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ix.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    rows = []
    for dim_full in (256, DIM_FULL):
        rv = ix.make_rescore_vectors(np.ascontiguousarray(X[:, :dim_full]), ids="input", dtype="int8", metric="l2")
        kpad = -(-rv.row_bytes // 32) * 32
        kpad = kpad if kpad <= 256 else -(-kpad // 128) * 128
        for b in BATCHES:
            fq, q = FQd[:b, :dim_full].contiguous(), FQd[:b, :DIM].contiguous()
            runs = {"all": lambda: ix.search_rescored_device(q, K, rv, full_queries=fq, candidates="all")}
            for c in CS:
                runs[c] = lambda c=c: ix.search_rescored_device(q, K, rv, full_queries=fq, candidates=c)
            t, kern, res = {name: [] for name in runs}, [], {}
            for rep in range(args.reps + 2):                       # two warm rounds, then the calls in turn
                for name, fn in runs.items():
                    dt, res[name] = timed(fn)
                    if rep >= 2:
                        t[name].append(dt)
                        if name == "all":
                            kern.append(ix.last_rescored_all_us())
            tiles = -(-b // 128)
            floor_b = tiles * n * rv.row_bytes / (COPY_TB_S * 1e12) * 1e6
            floor_m = 2.0 * tiles * 128 * n * kpad / rate.value * 1e6
            row = dict(dim_full=dim_full, queries=b, scan_us_median=round(float(np.median(kern)), 1), scan_us_max=round(max(kern), 1),
                       byte_floor_us=round(floor_b, 1), mac_floor_us=round(floor_m, 1),
                       scan_over_byte_floor=round(float(np.median(kern)) / floor_b, 2),
                       scan_over_mac_floor=round(float(np.median(kern)) / floor_m, 2), reps=args.reps)
            for name in runs:
                row[f"call_ms_{name}"] = round(float(np.median(t[name])) * 1e3, 3)
                if dim_full == DIM_FULL:
                    row[f"recall_{name}"] = round(recall(res[name][0].cpu().numpy(), truth[:b]), 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
        rv.close()
    ix.time_rescored_all(False)
    if not args.no_write:
        write_report(rows, rate.value, n, args.reps, args.out)


def write_report(rows, rate, n, reps, out):
    cols = sorted({c for r in rows for c in r}, key=lambda c: [c not in ("dim_full", "queries"), c])
    lines = ["| " + " | ".join(c.replace("_", " ") for c in cols) + " |", "|" + "---|" * len(cols)]
    lines += ["| " + " | ".join(str(r.get(c, "")) for c in cols) + " |" for r in rows]
    head = ('# Exhaustive int8 rescoring: search_rescored_device(k = 10, candidates="all") against the two-stage call\n\n'
            f"{n:,} x {DIM}, {BITS}-bit, over the prefix-trained rows of scripts/rescore_sweep.py; int8 objects of 256 and {DIM_FULL} "
            f"coordinates; device batches, one process, the calls alternating, warm; medians of {reps} runs (host clock around calls "
            "that end in a device synchronise).  `scan us` is rescore_i8_all_scan_kernel alone between two HIP events; `byte floor` = "
            "ceil(queries / 128) x object bytes / 6.29 TB/s; `mac floor` = 2 x padded queries x rows x K_pad MACs at "
            f"{rate / 1e12:.1f} T int8 MAC/s, the rate of a bare v_mfma_i32_32x32x32_i8 loop in the same process.  Recall@10 against "
            "float64 brute force at 1,024 coordinates.  scripts/rescore_all_sweep.py.\n\n")
    old = open(out).read() if os.path.exists(out) else ""
    kept = old[old.index(KEEP):] if KEEP in old else KEEP + "\n"
    with open(out, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
