#!/usr/bin/env python3
"""Graph-quality goldens (authoring container only; needs oracle/_ref).

    python tests/golden/make_golden_quality.py   ->   tests/golden/ref_graph_quality.json

The compiled reference builds and finalizes an index over each seeded dataset of the graph-quality tests
(tests/test_gpu_builder.py: quality_data_20k, quality_data_100k) and searches it with the tests' protocol; the
dedup recall@10 it reaches is what the tests hold this repo's GPU builder against.  The reference's build is not
reproducible across thread counts, so each build runs at every thread count of THREADS in a child
process and the highest recall is kept: the tests' margin is then measured from the reference's best.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
THREADS = (4, 8)
CASES = {"q20k_b4": ("quality_data_20k", (20,)), "q100k_b4": ("quality_data_100k", (20, 100))}


def measure(name):
    """One reference build + search in this process (OpenMP thread count from the environment)."""
    import tempfile
    import numpy as np  # noqa: F401
    import test_gpu_builder as t
    from oracle_lib import ref_module
    data, ks = CASES[name]
    X, Q = getattr(t, data)()
    gt = t.brute_topk(X, Q, 10)
    ref = ref_module().CPIndex(X.shape[1], 4)
    ref.build(X)
    ref.finalize()
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "ref.idx")
        ref.save(p)
        rows = t.input_rows(p, X)
    return {f"k{k}": t.dedup_recall(ref.search_batch(Q, k)[0], rows, gt, X) for k in ks}


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        print(json.dumps(measure(sys.argv[2])))
        return
    out = {}
    for name in CASES:
        runs = {}
        for th in THREADS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name], check=True, capture_output=True,
                               text=True, env=dict(os.environ, OMP_NUM_THREADS=str(th)))
            runs[th] = json.loads(r.stdout.strip().splitlines()[-1])
            print(name, th, "threads:", runs[th], flush=True)
        out[name] = {k: max(v[k] for v in runs.values()) for k in runs[THREADS[0]]}
        out[name]["runs"] = {str(th): v for th, v in runs.items()}
    with open(os.path.join(HERE, "ref_graph_quality.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
