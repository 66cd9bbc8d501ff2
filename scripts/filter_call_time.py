"""Host-side call time of label_filters / tag_filters at m = 1 and m = 16, where the call overhead is most of the cost:
the set-up and the timing method of scripts/label_filter_sweep.py and scripts/tag_filter_sweep.py (n = 1M rows, 16
dimensions, 1 bit; labels uniform over 1,024 values; 0..32 tags per row with a skew; wall clock with synchronize() on both
sides, every filter closed outside the timed window), the device paths only.  --tree names the checkout whose package and
library are measured, so two builds can be compared process by process; --tag is copied into every output line.
    python scripts/filter_call_time.py --tree . --tag new [--n 1000000] [--reps 41]
One JSON line per point: median, minimum and quartiles of the wall clock, the median device time of the pass."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", required=True)
ap.add_argument("--tag", required=True)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=41)
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path.insert(0, os.path.join(tree, "rabitq-ann-search_amd"))
sys.path.insert(0, os.path.join(tree, "scripts"))
import cphnsw_mi355x                              # noqa: E402
from tag_filter_sweep import VOCAB, make_column   # noqa: E402

assert os.path.dirname(os.path.dirname(cphnsw_mi355x.__file__)) == os.path.join(tree, "rabitq-ann-search_amd")
n, dim = args.n, 16
rng = np.random.default_rng(6)
ix = cphnsw_mi355x.CPIndex(dim, 1, device=0)
t0 = time.perf_counter()
ix.build(rng.standard_normal((n, dim)).astype(np.float32))
ix.finalize()
print(f"built {n} x {dim} in {time.perf_counter() - t0:.1f} s", flush=True)
ix.set_tags("t", *make_column(n, rng)[::-1], ids="internal")
labels = rng.integers(0, VOCAB, n).astype(np.int32)
ix.set_labels(labels, ids="internal")
ix.time_tag_filters(True)
ix.time_label_filters(True)


def timed(make, arg, last_us):
    ix.synchronize()
    t = time.perf_counter()
    fs = make(arg)
    ix.synchronize()
    dt = time.perf_counter() - t
    us = last_us()
    for f in fs:
        f.close()
    return dt, us


def point(what, m, make, arg, last_us):
    for _ in range(5):
        timed(make, arg, last_us)
    runs = [timed(make, arg, last_us) for _ in range(args.reps)]
    t = np.array([r[0] for r in runs]) * 1e6
    row = dict(tree=args.tag, call=what, m=m, median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1),
               p25_us=round(float(np.percentile(t, 25)), 1), p75_us=round(float(np.percentile(t, 75)), 1),
               kernel_us=round(float(np.median([r[1] for r in runs])), 1), reps=args.reps)
    print(json.dumps(row), flush=True)


for m in (1, 16):
    values = rng.permutation(VOCAB)[:m].astype(np.int32)
    point("label_filters", m, ix.label_filters, values, ix.last_label_filters_us)
for width in (1, 16):
    for m in (1, 16):
        tests = [rng.choice(VOCAB, width, replace=False).astype(np.int32) for _ in range(m)]
        point(f"tag_filters w{width}", m, lambda t: ix.tag_filters("t", t), tests, ix.last_tag_filters_us)
