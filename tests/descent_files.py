"""Hand-made upper layers for the golden index files: data plumbing, no reference code.

A golden fixture's bytes with the upper-layer section replaced by layers written here reach, in milliseconds, the hop
routines of the encoder's descent that no index built by this repository reaches (csrc/device_encode.h: degrees above
32, the unmapped fallback, every D, the 16 / 17 node switch, ties at chosen list positions, 24 layers).  The library,
the oracle and the compiled reference all load the same file; nothing here computes an expected result.

  split_v2 / parse_upper / with_upper_layers / with_equal_rows   the byte surgery
  census                                                         a float64 walk of the greedy rule that only COUNTS
                                                                 which hop classes the queries reach
  make_shape                                                     the seeded shapes (SHAPES) of tests/test_gpu_descent_shapes.py
"""
import gzip
import os
import struct
from collections import Counter

import numpy as np

from golden_util import DATASETS, GOLDEN_DIR, vertex_layout

MAX_LEVEL_OFF, ENTRY_OFF = 36, 40      # header fields of the v2 file
MAPPED_MAX_DEGREE = 62                 # a layer of more than 16 nodes gets a vertex -> row map up to this degree
SMALL_LAYER = 16                       # layers of this many nodes or fewer are searched by binary search
DEGREES = (0, 1, 2, 7, 8, 9, 31, 32, 33, 40, 61, 62)
SMALL_DEGREES = (0, 1, 7, 8, 9, 15)
# list positions of an equal pair, one per level of the two reductions: a lane pair's partner / the next group of eight
# lanes, a quad, row_ror:4, row_ror:8 / the next chunk of eight, the next row of 16, and the pass boundary 31 | 32
TIE_LOW = ((0, 1), (1, 2), (3, 4), (7, 8), (15, 16))
TIE_HIGH = ((31, 32), (32, 33), (47, 48), (60, 61))

SHAPES = ("wide", "fallback", "stray", "stray_entry", "ties", "extra", "extra_level0", "deep24")
FIXTURES = [(name, spec["bits"][-1]) for name, spec in DATASETS.items()]


def fixture_bytes(name, bits):
    with gzip.open(os.path.join(GOLDEN_DIR, f"idx_{name}_b{bits}.idx.gz"), "rb") as g:
        return g.read()


def split_v2(data, spec, bits):
    """Header fields and the (begin, end) byte ranges of the sections of a v2 index file."""
    n, dim, D = spec["n"], spec["dim"], spec["D"]
    assert struct.unpack_from("<I", data, 12)[0] == D and struct.unpack_from("<I", data, 24)[0] == dim
    assert struct.unpack_from("<Q", data, 28)[0] == n and struct.unpack_from("<I", data, 20)[0] == bits
    o = 68 + 248 + 72 + dim * 4
    out = dict(n=n, dim=dim, D=D, bits=bits, max_level=struct.unpack_from("<i", data, MAX_LEVEL_OFF)[0],
               entry=struct.unpack_from("<I", data, ENTRY_OFF)[0])
    for key, size in (("levels", n * 4), ("norm_sq", n * 4), ("raw", n * D * 4), ("vertex", n * vertex_layout(D, bits)[0])):
        out[key] = (o, o + size)
        o += size
    out["upper"] = (o, len(data))
    return out


def parse_upper(data, off):
    """The upper-layer section at `off` as [[(node, [neighbour ids])]], bottom layer first; it must end the file."""
    (nl,) = struct.unpack_from("<I", data, off)
    off += 4
    layers = []
    for _ in range(nl):
        (sz,) = struct.unpack_from("<I", data, off)
        off += 4
        layer = []
        for _ in range(sz):
            node, cnt = struct.unpack_from("<II", data, off)
            layer.append((node, list(struct.unpack_from(f"<{cnt}I", data, off + 8))))
            off += 8 + 4 * cnt
        layers.append(layer)
    assert off == len(data), (off, len(data))
    return layers


def with_upper_layers(data, spec, bits, layers, entry, max_level=None):
    """The file's bytes with the upper section replaced by `layers` ([(node, [neighbour ids])] per layer, bottom layer
    first, sorted by node and unique), levels[] rewritten (a node's level is the highest layer that lists it) and the
    header's entry and max_level patched (max_level defaults to the number of layers).  Every other byte stays."""
    s = split_v2(data, spec, bits)
    n = s["n"]
    levels = np.zeros(n, np.int32)
    sec = [struct.pack("<I", len(layers))]
    for l, layer in enumerate(layers):
        nodes = [node for node, _ in layer]
        assert nodes == sorted(set(nodes)) and all(0 <= v < n for v in nodes), ("layer", l + 1)
        sec.append(struct.pack("<I", len(layer)))
        for node, nbrs in layer:
            levels[node] = l + 1
            sec.append(struct.pack(f"<II{len(nbrs)}I", node, len(nbrs), *nbrs))
    b = bytearray(data[:s["upper"][0]])
    b[s["levels"][0]:s["levels"][1]] = levels.tobytes()
    struct.pack_into("<i", b, MAX_LEVEL_OFF, len(layers) if max_level is None else max_level)
    struct.pack_into("<I", b, ENTRY_OFF, entry)
    return bytes(b) + b"".join(sec)


def with_equal_rows(data, spec, pairs):
    """Raw row and norm_sq of `src` copied over those of `dst`, for every {dst: src}: ties in the exact bits at any
    precision.  (The layer-0 codes of `dst` go stale, which is harmless: every reader gets the same file.)"""
    n, dim, D = spec["n"], spec["dim"], spec["D"]
    o_norm = 68 + 248 + 72 + dim * 4 + n * 4
    o_raw = o_norm + n * 4
    b = bytearray(data)
    for dst, src in pairs.items():
        assert dst != src and src not in pairs, (dst, src)
        b[o_raw + dst * D * 4:o_raw + (dst + 1) * D * 4] = data[o_raw + src * D * 4:o_raw + (src + 1) * D * 4]
        b[o_norm + dst * 4:o_norm + dst * 4 + 4] = data[o_norm + src * 4:o_norm + src * 4 + 4]
    return bytes(b)


def raw_rows(data, spec, bits):
    s = split_v2(data, spec, bits)
    return np.frombuffer(data, np.float32, s["n"] * s["D"], s["raw"][0]).reshape(s["n"], s["D"])


def layer_kind(layer):
    """How the library serves a layer: "small" (binary search, 16 nodes or fewer), "mapped", or "unmapped" (a larger
    layer with a degree above 62: binary search again)."""
    if len(layer) <= SMALL_LAYER:
        return "small"
    return "mapped" if all(len(nb) <= MAPPED_MAX_DEGREE for _, nb in layer) else "unmapped"


def degree_class(deg):
    return "0" if deg == 0 else "1..32" if deg <= 32 else "33..62" if deg <= 62 else "63+"


def census(X, layers, entry, max_level, Q):
    """A float64 walk of the greedy rule (move to the first stored neighbour at the smallest distance while that is
    smaller than the best) that counts what the queries reach; it asserts reach only, never results.  Returns
      hops        Counter[(kind, degree class)]  lists expanded
      absent      Counter[kind]                  arrivals at a vertex that is no node of the layer (the walk stops)
      layer_hops  [lists expanded] per layer
      max_moves   [most moves any query makes] per layer
      ties        Counter[(kind, degree class, first position, second position)]  moves whose minimum two list entries
                  with identical raw rows share: the first stored position decides which id the walk goes to
      equal_best  lists whose minimum equals the best so far (no move)"""
    X32 = np.ascontiguousarray(X, np.float32)
    X = X32.astype(np.float64)
    Qp = np.zeros((len(Q), X.shape[1]))
    Qp[:, :Q.shape[1]] = Q
    assert max_level <= len(layers), "the reference indexes upper_layers_[max_level - 1]"
    maps = [dict(layer) for layer in layers]
    kinds = [layer_kind(layer) for layer in layers]
    out = dict(hops=Counter(), absent=Counter(), layer_hops=[0] * len(layers), max_moves=[0] * len(layers),
               ties=Counter(), equal_best=0)
    for q in Qp:
        cur = entry
        best = ((X[cur] - q) ** 2).sum()
        for level in range(max_level, 0, -1):
            kind, moves = kinds[level - 1], 0
            while True:
                nb = maps[level - 1].get(cur)
                if nb is None:
                    out["absent"][kind] += 1
                    break
                out["hops"][(kind, degree_class(len(nb)))] += 1
                out["layer_hops"][level - 1] += 1
                if not nb:
                    break
                d = ((X[nb] - q) ** 2).sum(1)
                m = d.min()
                at = np.flatnonzero(d == m)
                if m == best:
                    out["equal_best"] += 1
                if not m < best:
                    break
                if len(at) > 1 and nb[at[0]] != nb[at[1]] and np.array_equal(X32[nb[at[0]]], X32[nb[at[1]]]):
                    out["ties"][(kind, degree_class(len(nb)), int(at[0]), int(at[1]))] += 1
                best, cur, moves = m, nb[at[0]], moves + 1
            out["max_moves"][level - 1] = max(out["max_moves"][level - 1], moves)
    return out


# ---- the shapes ------------------------------------------------------------------------------------------------------

def _lists(rng, order, pool, degrees, shift=0):
    """{node: neighbours} for the nodes of `order`: degree degrees[(i + shift) % len] for the i-th, drawn from pool."""
    out = {}
    for i, v in enumerate(order):
        cand = [int(x) for x in pool if x != v]
        deg = min(degrees[(i + shift) % len(degrees)], len(cand))
        out[int(v)] = [int(x) for x in rng.choice(cand, deg, replace=False)] if deg else []
    return out


def _layer(lists):
    return sorted(lists.items())


def _wide(rng, n, perm, n1, stray=False, complete=False):
    """Layer 1: the first n1 vertices of perm, degrees cycling through DEGREES (the 17 nodes of layer 2 come first, so
    they hold every degree).  Layer 2: 17 nodes with lists of 3, 8, 9 or 16 -- or, with `complete`, each listing the 16
    others, so that a walk leaves it at the layer-2 node nearest to the query.  Layer 3: 16 nodes, short lists.
    Layer 4: the entry alone.  With `stray`, lists draw from every vertex, not only from their layer's nodes."""
    everyone = np.arange(n)
    l1 = _lists(rng, perm[:n1], everyone if stray else perm[:n1], DEGREES)
    if not complete:
        l2 = _lists(rng, perm[:17], everyone if stray else perm[:17], (3, 8, 9, 16))
    else:
        l2 = {int(v): [int(x) for x in rng.permutation([y for y in perm[:17] if y != v])] for v in perm[:17]}
    l3 = _lists(rng, perm[:16], everyone if stray else perm[:16], SMALL_DEGREES, shift=4)
    return [l1, l2, l3, {int(perm[0]): []}]


def _chain(rng, L, X, perm):
    """Three moves in layer 1 for one query, by construction: the query copies row r; the walk arrives from layer 2 at
    A; the lists of A, c1 and c2 are redrawn (same degrees) so that their nearest entries to the query are c1, c2 and r.
    Returns r, whose row the caller adds to the queries."""
    X = X.astype(np.float64)
    n, entry = len(X), int(perm[0])
    for r in (int(v) for v in perm[17:]):
        d = ((X - X[r]) ** 2).sum(1)
        cur, best = entry, d[entry]
        for l in (2, 1):                                       # layers 3 and 2 (layer 4 holds the entry alone)
            while L[l].get(cur):
                m = min(L[l][cur], key=lambda v: d[v])         # (no equal rows here: the minimum is unique)
                if not d[m] < best:
                    break
                cur, best = m, d[m]
        near = [int(v) for v in np.argsort(d) if v not in (r, cur) and len(L[0][int(v)]) >= 1][:2]
        if len(L[0][cur]) == 0 or not d[near[1]] < best:
            continue
        for node, nxt in ((cur, near[1]), (near[1], near[0]), (near[0], r)):
            far = [int(v) for v in rng.permutation(n) if d[v] > d[nxt] and v != node]
            deg = len(L[0][node])
            assert len(far) >= deg - 1
            nb = far[:deg - 1]
            nb.insert(int(rng.integers(0, deg)), nxt)
            L[0][node] = nb
        return r
    raise AssertionError("no row gives a chain")


def _nearest(X, rows, among):
    d = ((X[rows][:, None, :].astype(np.float64) - X[among][None, :, :].astype(np.float64)) ** 2).sum(2)
    return np.asarray(among)[d.argmin(1)]


def _ties(rng, n, perm, X):
    """`wide`, with the lists of some layer-2 nodes ("hosts") rebuilt to hold an equal pair at given positions.  A query
    that copies the pair's row leaves layer 2 at the layer-2 node nearest to that row, so the host of a pair is the
    layer-2 node nearest to its source row: the walk enters layer 1 there and finds the pair, distance 0 twice, in the
    host's list.  Degree 32 takes the paired hop where D % 128 == 0, degree 62 the eight-lane hop everywhere."""
    L = _wide(rng, n, perm, n, complete=True)
    hosts = [int(v) for v in perm[:17]]
    others = [int(v) for v in perm[17:]]
    home = _nearest(X, others, hosts)
    groups = {t: [x for x, h in zip(others, home) if h == t] for t in hosts}
    jobs = [(a, b, 32) for a, b in TIE_LOW] + [(a, b, 62) for a, b in TIE_LOW] + [(a, b, 62) for a, b in TIE_HIGH]
    degree, taken, placed = {}, {t: {} for t in hosts}, []
    for a, b, deg in jobs:
        ok = [t for t in hosts if groups[t] and degree.get(t, deg) == deg and a not in taken[t] and b not in taken[t]]
        assert ok, ("no host left for", a, b, deg)
        t = max(ok, key=lambda t: (t in degree, len(groups[t])))     # fill a started host before opening another
        degree[t] = deg
        src = groups[t].pop()
        taken[t][a] = taken[t][b] = src                              # (b gets its own id below)
        placed.append([t, a, b, src, None])
    free = [x for t in hosts for x in groups[t]]
    for p in placed:
        p[4] = free.pop()
        taken[p[0]][p[2]] = p[4]
    # one list also holds a copy of its own node's row: the minimum equals the best, and the walk stays
    stay = placed[0][0]
    copy = free.pop()
    taken[stay][min(set(range(degree[stay])) - set(taken[stay]))] = copy
    reserved = {x for t in hosts for x in taken[t].values()}
    for t in degree:
        fill = [int(x) for x in rng.permutation([x for x in range(n) if x != t and x not in taken[t].values()])]
        # (the other hosts' pairs may fall into this list at any position: they tie there as well, which is welcome)
        nb = [taken[t][p] if p in taken[t] else fill.pop() for p in range(degree[t])]
        assert len(set(nb)) == len(nb)
        L[0][t] = nb
    equal = {dst: src for _, _, _, src, dst in placed}
    equal[copy] = stay
    assert len(reserved) == 2 * len(placed) + 1
    expect = [("32" if degree[t] == 32 else "62", a, b) for t, a, b, _, _ in placed]
    exact = [src for _, _, _, src, _ in placed] + [stay]
    return L, equal, expect, exact


def _deep(rng, n, depth):
    """`depth` nested layers that narrow: every vertex, 40, 30, 24, 20, 18, 17, then 16, 15, ... nodes, the top ones the
    entry alone (depth 24) or the entry and one more (depth 25)."""
    perm = rng.permutation(n)
    sizes = [n, 40, 30, 24, 20, 18, 17] + [max(1 if depth <= 24 else 2, 24 - l) for l in range(8, depth + 1)]
    L = []
    for l, sz in enumerate(sizes):
        L.append(_lists(rng, perm[:sz], perm[:sz], DEGREES if sz > SMALL_LAYER else SMALL_DEGREES, shift=l + 3))
    return perm, L


def make_queries(X, dim, Qgold, rng, first, exact=()):
    """The golden queries, 40 noisy copies of rows (`first` ones, then random ones; four of them exact copies), and an
    exact copy of every row of `exact`."""
    n = len(X)
    rows = list(first)[:40]
    rows += [int(x) for x in rng.choice(n, 40 - len(rows), replace=False)]
    noise = 0.3 * float(X[:, :dim].std()) * rng.standard_normal((40, dim))
    noise[::10] = 0.0
    parts = [np.asarray(Qgold, np.float32), (X[rows, :dim] + noise).astype(np.float32)]
    if len(exact):
        parts.append(X[list(exact), :dim])
    return np.ascontiguousarray(np.concatenate(parts), np.float32)


_MADE = {}


def make_shape(name, bits, shape, Qgold):
    """One (fixture, shape): dict(data, layers, entry, max_level, Q, X, census, expect_ties).  Seeded; cached."""
    key = (name, bits, shape)
    if key in _MADE:
        return _MADE[key]
    spec = DATASETS[name]
    n, dim = spec["n"], spec["dim"]
    data = fixture_bytes(name, bits)
    rng = np.random.default_rng(spec["seed"] * 100 + SHAPES_ALL.index(shape))
    X0 = raw_rows(data, spec, bits)
    expect_ties, exact, max_level = [], (), None
    if shape in ("deep24", "deep25"):
        perm, L = _deep(rng, n, int(shape[4:]))
    else:
        perm = rng.permutation(n)
        if shape == "ties":
            L, equal, expect_ties, exact = _ties(rng, n, perm, X0)
            data = with_equal_rows(data, spec, equal)
        else:
            stray = shape.startswith("stray")
            L = _wide(rng, n, perm, max(64, 3 * n // 4) if stray else n, stray=stray, complete=shape == "fallback")
        if shape == "wide":
            exact = (_chain(rng, L, X0, perm),)
        if shape == "fallback":
            for v, deg in zip(perm[1:4], (63, 64, min(n - 1, 100))):
                L[0][int(v)] = [int(x) for x in rng.permutation([y for y in range(n) if y != v])[:deg]]
        if shape == "stray_entry":
            L[3] = {int(perm[1]): []}                 # the entry is no node of the top layer
        if shape == "extra":
            max_level = 2                             # four layers stored, two used
        if shape == "extra_level0":
            max_level = 0
    entry = int(perm[0])
    layers = [_layer(l) for l in L]
    data = with_upper_layers(data, spec, bits, layers, entry, max_level)
    if max_level is None:
        max_level = len(layers)
    X = raw_rows(data, spec, bits)
    Q = make_queries(X, dim, Qgold, rng, perm[:17], exact)
    made = dict(data=data, layers=layers, entry=entry, max_level=max_level, Q=Q, X=X, expect_ties=expect_ties,
                census=census(X, layers, entry, max_level, Q))
    _MADE[key] = made
    return made


SHAPES_ALL = SHAPES + ("deep25",)


def check_reach(name, shape, made):
    """What a shape is for is reached by at least one query (a condition on the inputs: seeds and noise are picked so
    that it holds).  Returns the census for printing."""
    c, D = made["census"], DATASETS[name]["D"]
    hops, where = c["hops"], (name, shape, dict(c["hops"]), dict(c["absent"]))
    need = []
    if shape in ("wide", "ties", "extra"):
        need = [("mapped", k) for k in (("0",) if shape != "ties" else ()) + ("1..32", "33..62")]
        need += [("small", "1..32")] if shape != "extra" else []          # (`extra` stops above the small layers)
    if shape == "wide":
        assert c["max_moves"][0] >= 3, where + (c["max_moves"],)
        assert [layer_kind(l) for l in made["layers"]] == ["mapped", "mapped", "small", "small"]
        assert [len(l) for l in made["layers"][1:]] == [17, 16, 1]
    if shape == "fallback":
        need = [("unmapped", k) for k in ("0", "1..32", "33..62", "63+")] + [("mapped", "1..32"), ("small", "1..32")]
    if shape.startswith("stray"):
        need = [("mapped", "1..32"), ("mapped", "33..62"), ("small", "1..32")]
        assert c["absent"]["mapped"] and c["absent"]["small"], where
        assert shape != "stray_entry" or c["absent"]["small"] >= len(made["Q"]), where
    if shape == "extra":
        assert made["max_level"] == 2 and len(made["layers"]) == 4
    if shape == "extra_level0":
        assert not hops and len(made["layers"]) == 4, where
    if shape == "deep24":
        need = [("mapped", k) for k in ("1..32", "33..62")] + [("small", "1..32")]
        assert len(made["layers"]) == 24 and all(c["layer_hops"]), where + (c["layer_hops"],)
        assert sum(m > 0 for m in c["max_moves"]) >= 12, c["max_moves"]
    for k in need:
        assert hops[k] > 0, ("not reached", k) + where
    if shape == "ties":
        assert c["equal_best"] > 0, where
        for deg, a, b in made["expect_ties"]:
            kind = "1..32" if deg == "32" else "33..62"
            assert c["ties"][("mapped", kind, a, b)] > 0, ("equal pair decides no hop", deg, a, b, dict(c["ties"]))
    return c
