#!/usr/bin/env python3
"""Reference goldens at the padded dimensions that only the generic search instantiation serves:
D = 32, 64, 256, 512 and 2048 (authoring container only; needs oracle/_ref, ``make -C oracle ref``).

    python tests/golden/make_golden_dims.py            # re-uses the committed idx_*.idx.gz files
    python tests/golden/make_golden_dims.py --rebuild  # builds new ones with the reference

Outputs (tests/golden/), all data, each file under 1 MiB:
    idx_<name>_b<bits>.idx.gz   reference-built v2 index files of the datasets marked
                                golden="golden_dims.npz" in golden_util.DATASETS
    golden_dims.npz             their Q/, S/, S1/ keys (same scheme as golden.npz), and
        X/<D>/{a,b,dot,l2}                    exact arithmetic vectors, D in DIMS
        ENC/<dim>/<D>/b<bits>/{values,aux,pops}   data-side edge encoder at ENC_SHAPES; the inputs
        ENC/<dim>/<D>/{parent,nbrs}           are shared by the three bit widths (16 edges at D = 2048)
    golden_dims_fastscan.npz
        F/<D>/b<bits>/...                     FastScan block vectors, D in DIMS (4 blocks at D >= 512)

golden.npz is not touched: make_golden.py draws its F/ and X/ inputs from one RNG stream, so the
dimensions here have their own seeds and their own files.  golden_util.golden() serves all of
them as one key space.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from golden_util import DATASETS  # noqa: E402
from make_golden import exact_goldens, fastscan_goldens, search_goldens  # noqa: E402
from oracle_lib import RefHooks, ref_module  # noqa: E402

OUT = "golden_dims.npz"
OUT_F = "golden_dims_fastscan.npz"
DIMS = (32, 64, 256, 512, 2048)
ENC_SHAPES = ((24, 32), (200, 256), (1536, 2048))


def enc_inputs(dim, seed, cnt=32):
    """Like make_golden_build.enc_inputs (Gaussian at a random scale / SIFT-like integers with an exact duplicate),
    seeded independently of the bit width so that one input set serves b1, b2 and b4."""
    rng = np.random.default_rng([17, dim, seed])
    if seed % 2 == 0:
        sc = 10.0 ** rng.uniform(-2, 2)
        p = (sc * rng.standard_normal(dim)).astype(np.float32)
        nb = (p + sc * rng.uniform(0.05, 1.5) * rng.standard_normal((cnt, dim))).astype(np.float32)
    else:
        p = np.round(rng.gamma(2, 15, dim)).astype(np.float32)
        nb = np.clip(np.round(p + rng.normal(0, 12, (cnt, dim))), 0, 218).astype(np.float32)
        nb[5] = p
    return p, nb


def main():
    m = ref_module()
    r = RefHooks()
    out = {}
    tmp = "/tmp/golden_build_dims"
    os.makedirs(tmp, exist_ok=True)

    for name, spec in DATASETS.items():
        if spec.get("golden") == OUT:
            search_goldens(m, name, spec, out, tmp)

    rng = np.random.default_rng(20480)
    for D in DIMS:
        fastscan_goldens(r, rng, D, out, nblk=4 if D >= 512 else 8)
    for D in DIMS:
        exact_goldens(r, rng, D, out, rows=4 if D == 2048 else 8 if D == 512 else 16)

    for dim, D in ENC_SHAPES:
        P, N = zip(*(enc_inputs(dim, seed, 16 if D == 2048 else 32) for seed in range(2)))
        out[f"ENC/{dim}/{D}/parent"], out[f"ENC/{dim}/{D}/nbrs"] = np.stack(P), np.stack(N)
        for bits in (1, 2, 4):
            V, A, S = zip(*(r.encode_edges(p, nb, D, bits) for p, nb in zip(P, N)))
            key = f"ENC/{dim}/{D}/b{bits}"
            out[f"{key}/values"], out[f"{key}/aux"], out[f"{key}/pops"] = np.stack(V), np.stack(A), np.stack(S)

    for name, keep in ((OUT, lambda k: not k.startswith("F/")), (OUT_F, lambda k: k.startswith("F/"))):
        part = {k: v for k, v in out.items() if keep(k)}
        np.savez_compressed(os.path.join(HERE, name), **part)
        print("wrote", name, "with", len(part), "arrays")


if __name__ == "__main__":
    main()
