"""Census of the arms of the steady loop's push tail (csrc/device_search_expansion.inc) on the batches of
tests/test_gpu_steady_tail.py, with a diagnostic build (-DCPH_TAIL_CENSUS: eight counters in the spare statistic words,
steady copy only; the shipped kernel has none).  Build here or on the box, then run on the GPU box from the repo root:
    python scripts/tail_census.py --build build/libcph_census.so
    python scripts/tail_census.py --lib build/libcph_census.so 2>&1 | tee census.txt
Each batch prints its name, then the library prints one `[tail census]` line for it on stderr (profiles/steady_tail.md)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rabitq-ann-search_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    if args.build:
        from cphnsw_mi355x import build as b
        os.makedirs(os.path.dirname(os.path.abspath(args.build)), exist_ok=True)
        subprocess.check_call([b._hipcc()] + b.FLAGS + ["-DCPH_TAIL_CENSUS", os.path.join(b.CSRC, "cphnsw_mi355x.hip"),
                                                         "-o", args.build, "-lpthread"])
        return
    os.environ["CPH_LIB_PATH"] = os.path.abspath(args.lib)
    import pathlib
    import tempfile
    import cphnsw_mi355x as cph
    import test_gpu_steady_tail as t
    from oracle_lib import Oracle
    tmp = pathlib.Path(tempfile.mkdtemp())
    for name, cap, k in t.CENSUS_BATCHES:
        b = t.built_for(cph, Oracle(), tmp, name)
        ix = t._index(cph, b, cap if cap else b.n + 1)
        ix.search_batch(b.queries(name), k)
        sys.stderr.flush()
        print(f"batch {name} k={k} capacity={cap if cap else b.n + 1}:", flush=True)
        st = ix.last_search_stats()          # (the library prints the census line here)
        sys.stderr.flush()
        print("   ", st, flush=True)


if __name__ == "__main__":
    main()
