"""GPU tests that pin layer-0 construction to the oracle (tests/layer_model.py states what is compared):

  1-2  select_kernel's hub branch (more than 96 reverse edges) on one vertex, and its independence of the reverse
       list's order;
  3    reverse_csr (count, prefix sum, fill) on whole tables;
  4-5  select_layer as finalize() launches it -- row == vertex, grid-stride loop, LDS carried from row to row -- on one
       and seven workgroups and on the production grid with more rows than workgroups;
  6    every edge stored by build() + finalize() is the encoder's output for that edge, on grids smaller than n;
  7    the invariants of the hub + BFS renumbering.

Every comparison is exact (ids in order, floats by their bytes) except the stored norms of test 7."""
import numpy as np
import pytest

import block_layout
import layer_model
from layer_model import INVALID

pytestmark = pytest.mark.gpu

PARAMS = ((1.2, 0.5, 0.0), (1.05, 2.0, 1.6))          # (alpha, tau, alpha_max) of the single-vertex test in test_gpu_builder.py


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


@pytest.fixture(scope="module")
def num_cus():
    """The CU count the library sizes its grids by (hipGetDeviceProperties: multiProcessorCount)."""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def clustered(rng, n, D, rounded, ncl=6):
    """The generator of test_select_kernel_matches_the_rule_on_fixed_candidates: clusters (occlusions happen); rounded
    rows give equal distances."""
    cent = rng.normal(0, 4, (ncl, D))
    x = (cent[rng.integers(0, ncl, n)] + rng.normal(0, 1, (n, D))).astype(np.float32)
    return np.round(x) if rounded else x


# ---- 1, 2: the hub branch on one vertex ---------------------------------------------------------------------------
N_REV = (97, 128, 129, 160, 161, 223, 224, 500, 1500)
HUB_CASES = [(D, 2000, n_rev, R) for D in (16, 64, 128) for R in (32, 18, 8) for n_rev in N_REV] + [(1024, 300, 200, 32)]


def hub_trial(rng, x, n_rev, trial):
    """One vertex' inputs.  Every trial: exactly 3 empty forward slots and the vertex itself in the forward list.
    trial 0, 2, 3, 5: every valid forward id again in rev, half of them at its front (first chunk), half at its end (last
    chunk); trial 1, 2, 4, 5: 20 rows spread over rev are byte copies of the vertex' row (distance 0, ordered by id
    across chunks); every trial but 2: the vertex itself in rev; odd trials: error margins; trials 3-5: the second
    parameter set."""
    n = len(x)
    v = int(rng.integers(0, n))
    fwd = rng.choice(n, 32, replace=False).astype(np.uint32)
    fwd[rng.choice(np.setdiff1d(np.arange(32), [5]), 3, replace=False)] = INVALID
    fwd[5] = v
    rev = rng.choice(n, n_rev, replace=False).astype(np.uint32)
    valid = fwd[(fwd != INVALID) & (fwd != v)]
    h = len(valid) // 2
    if trial in (0, 2, 3, 5):
        rev[:h] = valid[:h]
        rev[n_rev - (len(valid) - h):] = valid[h:]
    if trial != 2:
        rev[n_rev // 2] = v
    if trial in (1, 2, 4, 5):
        pos = np.linspace(h, n_rev - 1 - h, 20).astype(np.int64)
        pos[pos == n_rev // 2] += 1
        assert len(set(pos.tolist())) == 20
        x = x.copy()
        x[rev[pos]] = x[v]
    err = None if trial % 2 == 0 else np.abs(rng.normal(0, 0.3, n)).astype(np.float32)
    return x, v, fwd, rev, err, PARAMS[0 if trial < 3 else 1]


@pytest.mark.parametrize("D,n,n_rev,R", HUB_CASES)
def test_hub_path_matches_the_rule_on_the_hub_cut(cph, oracle, D, n, n_rev, R):
    """select_kernel on one vertex with more than 96 reverse edges against the oracle's rule on layer_model.candidates:
    the hub cut (the 64 nearest unique candidates by (distance, id)) is what the kernel's chunk loop must amount to --
    a deliberate property of the kernel, stated by the model.  n_rev puts 1 to 64 entries into the last chunk; the list
    of selected ids must be identical, order included."""
    seed = 1000 * D + 10 * n_rev + R
    rng = np.random.default_rng(seed)
    x0 = clustered(rng, n, D, seed % 4 < 2)
    for trial in range(6):
        x, v, fwd, rev, err, (alpha, tau, amax) = hub_trial(rng, x0, n_rev, trial)
        got = cph.select_neighbors_debug(x, v, fwd, rev, R, alpha, tau, amax, err)
        cand = layer_model.candidates(oracle, x, v, fwd, rev)
        assert len(cand) == layer_model.HUB_KEEP                  # the cut is taken: more unique candidates than it keeps
        want = oracle.select_neighbors(x, v, cand, R, alpha, tau, amax, err)
        assert np.array_equal(got, want), (D, n_rev, R, trial, got, want)
        assert len(got) == R and v not in got and len(set(got.tolist())) == len(got)


@pytest.mark.parametrize("D,n,n_rev,R", [(16, 2000, 97, 32), (64, 2000, 224, 18), (128, 2000, 1500, 8)])
def test_hub_path_does_not_depend_on_the_order_of_the_reverse_list(cph, D, n, n_rev, R):
    """The order of a reverse list comes from the atomics of reverse_fill_kernel and differs from run to run; the hub
    branch claims its result does not depend on it.  rev as given, reversed and under 4 seeded permutations: six equal
    outputs (on rounded rows: with equal distances at the cut)."""
    rng = np.random.default_rng(D + n_rev)
    x0 = clustered(rng, n, D, True)
    for trial in (1, 3, 5):
        x, v, fwd, rev, err, (alpha, tau, amax) = hub_trial(rng, x0, n_rev, trial)
        orders = [rev, rev[::-1].copy()] + [rng.permutation(rev) for _ in range(4)]
        outs = [cph.select_neighbors_debug(x, v, fwd, r, R, alpha, tau, amax, err) for r in orders]
        for o in outs[1:]:
            assert np.array_equal(o, outs[0]), (D, n_rev, trial, o, outs[0])


# ---- 3: the reverse CSR ----------------------------------------------------------------------------------------------
def random_table(rng, n, pool=None, keep=32):
    """[n][32]: per row up to `keep` distinct ids of `pool` (default: all vertices) other than the row itself, padded."""
    knn = np.full((n, 32), INVALID, np.uint32)
    pool = np.arange(n) if pool is None else np.asarray(pool)
    for u in range(n):
        p = pool[pool != u]
        m = min(keep, len(p))
        knn[u, :m] = rng.choice(p, m, replace=False)
    return knn


@pytest.mark.parametrize("n", [1, 33, 255, 256, 257, 1000])
@pytest.mark.parametrize("kind", ["random", "all_list_0", "unlisted"])
def test_reverse_csr_is_the_transpose_of_the_table(cph, n, kind):
    """reverse_count_kernel, the host prefix sum and reverse_fill_kernel through the production select_layer: offsets
    are the running in-degrees, and every segment holds, in some order, exactly the rows that list the vertex."""
    rng = np.random.default_rng(n)
    if kind == "random":
        knn = random_table(rng, n)
    elif kind == "all_list_0":
        knn = random_table(rng, n, keep=31)
        for u in range(1, n):
            if 0 not in knn[u]:
                knn[u, 31 if n > 32 else n - 2] = 0
        assert n == 1 or (knn[1:] == 0).sum() == n - 1
    else:
        knn = random_table(rng, n, pool=np.arange((n + 1) // 2))      # nobody lists the upper half
    x = rng.standard_normal((n, 16)).astype(np.float32)
    _, _, off, rev = cph.select_layer_debug(x, knn, 32, 1.2, 0.5)
    valid = knn[knn != INVALID]
    want_off = np.concatenate([[0], np.cumsum(np.bincount(valid, minlength=n))]).astype(np.uint64)
    assert np.array_equal(off, want_off)
    assert len(rev) == len(valid)
    lists = layer_model.reverse_lists(knn, n)
    for v in range(n):
        assert np.array_equal(np.sort(rev[int(off[v]):int(off[v + 1])]), lists[v]), (n, kind, v)
    if kind == "all_list_0":
        assert len(lists[0]) == n - 1
    if kind == "unlisted" and n > 1:
        assert all(len(lists[v]) == 0 for v in range((n + 1) // 2, n))


# ---- 4, 5: whole layers ----------------------------------------------------------------------------------------------
def check_lists(ids, cnt, n):
    """No self, no duplicates, kInvalidNode exactly from cnt[v] on."""
    slot = np.arange(32)[None, :]
    assert np.array_equal(ids != INVALID, slot < cnt[:, None])
    assert (ids != np.arange(n, dtype=np.uint32)[:, None]).all()
    assert ((ids < n) | (ids == INVALID)).all()
    s = np.sort(ids, axis=1)
    assert ((s[:, 1:] != s[:, :-1]) | (s[:, 1:] == INVALID)).all()


def branchy_table(rng, n, R):
    """A table whose consecutive rows take different branches of select_kernel.  Vertices 0..3 are hubs of in-degree
    97, 130, 300 and n - 1 (listed by the first rows: rows 0..97 list all four).  Of the rows from 4 on, by v % 4:
      0, 1  listed by others with a skewed probability: 1..96 reverse edges for most, a few more hubs, a few with none;
      2     listed by nobody, full forward list;
      3     listed by nobody, a forward list of at most 11 ids: at most R candidates, the kernel's early `continue`."""
    assert n >= 400 and R >= 12
    targets = {0: 97, 1: 130, 2: 300, 3: n - 1}
    pool = np.array([v for v in range(4, n) if v % 4 < 2])
    w = (np.arange(len(pool)) + 1.0) ** 2
    knn = np.full((n, 32), INVALID, np.uint32)
    for u in range(n):
        row = [h for h, t in targets.items() if h != u and (u < t if u < h else u <= t)]
        length = int(rng.integers(len(row), 12)) if (u >= 4 and u % 4 == 3) else 32
        p = w * (pool != u)
        more = rng.choice(pool, length - len(row), replace=False, p=p / p.sum())
        row = np.array(row + more.tolist(), np.uint32)
        knn[u, :length] = row[rng.permutation(length)]
    return knn


@pytest.fixture(scope="module")
def branchy():
    """(x, err, knn, model output) per (D, R), computed once: the grid caps share the reference."""
    cache = {}

    def get(oracle, D, R):
        if (D, R) not in cache:
            rng = np.random.default_rng(D + R)
            n = 600
            x = clustered(rng, n, D, R == 18)
            err = np.abs(rng.normal(0, 0.3, n)).astype(np.float32)
            knn = branchy_table(rng, n, R)
            alpha, tau, amax = PARAMS[0 if R == 32 else 1]
            want = layer_model.select_layer(oracle, x, knn, R, alpha, tau, amax, err)
            for a in (x, err, knn) + want:
                a.setflags(write=False)
            cache[(D, R)] = (x, err, knn, want)
        return cache[(D, R)]
    yield get
    cache.clear()


@pytest.mark.parametrize("grid_cap", [1, 7])
@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("R", [32, 18])
def test_whole_layer_on_few_workgroups_matches_the_model(cph, oracle, branchy, grid_cap, D, R):
    """600 rows on one workgroup and on seven: each workgroup walks rows of every kind one after the other -- hubs,
    1..96 reverse edges, none, and rows with at most R candidates (the early `continue`) -- carrying cvec, cid / cd and
    sel / selerr in LDS from one row to the next.  Ids (in order) and counts equal the model's on every row."""
    x, err, knn, (want_ids, want_cnt) = branchy(oracle, D, R)
    n = len(x)
    alpha, tau, amax = PARAMS[0 if R == 32 else 1]
    ids, cnt, off, _ = cph.select_layer_debug(x, knn, R, alpha, tau, amax, err, grid_cap=grid_cap)
    # the table does what it was built for
    indeg = np.diff(off.astype(np.int64))
    assert indeg[:4].tolist() == [97, 130, 300, n - 1]
    uniq = np.array([len(set(knn[v][knn[v] != INVALID].tolist()) - {v}) for v in range(n)])
    kinds = np.where(indeg > 96, 0, np.where(indeg > 0, 1, np.where(uniq == 32, 2, 3)))      # hub, 1..96, none, short
    assert all((kinds == k).sum() >= 20 for k in (1, 2, 3)) and (kinds == 0).sum() >= 4
    assert (np.abs(np.diff(kinds[::grid_cap])) > 0).mean() > 0.5          # a workgroup's consecutive rows change branch
    assert (uniq[kinds == 3] <= 11).all() and (want_cnt[kinds == 3] == uniq[kinds == 3]).all()    # the early `continue`
    bad = np.nonzero((ids != want_ids).any(axis=1) | (cnt != want_cnt))[0]
    assert len(bad) == 0, (grid_cap, D, R, bad[:8], ids[bad[:1]], want_ids[bad[:1]])
    check_lists(ids, cnt, n)


def test_whole_layer_on_the_production_grid_matches_the_model(cph, oracle, num_cus):
    """select_layer exactly as build_graph calls it (grid_cap = 0) on a true 32-NN table of 9,000 clustered rows with 3 %
    duplicated rows at D = 16: more rows than the num_cus * 32 workgroups of the launch, so the rows from `grid` on are
    second trips of the grid-stride loop.  Compared with the model on ALL rows (the oracle side takes about a second
    at D = 16)."""
    n, D, R = 9000, 16, 32
    grid = num_cus * 32
    assert n > grid, (n, grid)
    rng = np.random.default_rng(77)
    x = clustered(rng, n, D, False, ncl=40)
    dup = rng.choice(n, n * 3 // 100, replace=False)
    x[dup] = x[rng.choice(np.setdiff1d(np.arange(n), dup), len(dup))]
    err = np.abs(rng.normal(0, 0.3, n)).astype(np.float32)
    knn, _ = cph.knn_bruteforce(x)
    assert (knn < n).all()
    alpha, tau, amax = PARAMS[0]
    ids, cnt, off, _ = cph.select_layer_debug(x, knn, R, alpha, tau, amax, err)
    want_ids, want_cnt = layer_model.select_layer(oracle, x, knn, R, alpha, tau, amax, err)
    indeg = np.diff(off.astype(np.int64))
    print(f"production grid {grid} < n {n}: {(indeg > 96).sum()} hub rows, max in-degree {indeg.max()}")
    bad = np.nonzero((ids != want_ids).any(axis=1) | (cnt != want_cnt))[0]
    assert len(bad) == 0, (len(bad), bad[:8], ids[bad[:1]], want_ids[bad[:1]])
    assert (cnt == R).all()
    check_lists(ids, cnt, n)


# ---- 6, 7: a built index ---------------------------------------------------------------------------------------------
def padded_dim(dim):
    D = 16
    while D < dim:
        D *= 2
    return D


def encode_grid(D, num_cus):
    """The workgroups run_encode (builder_pipeline.h) launches for the edge codes of more than that many vertices."""
    def lds(epb):
        return (3 * D + 16 + 32) * 4 + epb * (D + 1) * 4 + epb * (D + 4)
    epb = 32
    while epb > 8 and lds(epb) > 72 * 1024:
        epb //= 2
    if epb < 32:                                        # rows in the HBM scratch (the G = true instantiation)
        per_cu = max(1, min(12, (150 * 1024) // ((3 * D + 16 + 32) * 4)))
    else:
        per_cu = max(1, min(16, (150 * 1024) // lds(32)))
    return num_cus * per_cu, epb < 32


def gauss_with_copies(n, dim, seed):
    """Gaussian rows, 5 % of them exact copies of other rows (edges of length zero: nop = 0 inside real launches).  The
    four rows nearest the centroid are neither copied nor copies, so that the hub of the renumbering is unique."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    c = X.astype(np.float64).mean(0)
    central = np.argsort(((X - c) ** 2).sum(1))[:4]
    rest = np.setdiff1d(np.arange(n), central)
    dup = rng.choice(rest, n // 20, replace=False)
    X[dup] = X[rng.choice(np.setdiff1d(rest, dup), len(dup))]
    return X


@pytest.fixture(scope="module")
def built(cph):
    """Indices built by the production build() + finalize(), with their exported storage-layout blocks: one per case."""
    from cphnsw_mi355x import _lib
    cache = {}

    def get(bits, dim, n):
        key = (bits, dim, n)
        if key not in cache:
            X = gauss_with_copies(n, dim, 100 * bits + dim)
            ix = cph.CPIndex(dim, bits)
            ix.build(X)
            ix.finalize()
            D = padded_dim(dim)
            blocks = np.zeros((n, block_layout._layout(D, bits)[5]), np.uint8)
            _lib.check(_lib.lib().cph_export_blocks(ix._h, 0, n, 0, blocks.ctypes.data))
            cache[key] = dict(ix=ix, X=X, D=D, blocks=blocks, raw=ix.get_vectors(), rows=ix.row_map())
        return cache[key]
    yield get
    cache.clear()


def all_ids(blocks, D, bits):
    o = block_layout.codes_bytes(D, bits) + 512
    ids = np.ascontiguousarray(blocks[:, o:o + 128]).view(np.uint32)
    cnt = np.ascontiguousarray(blocks[:, o + 128:o + 132]).view(np.uint32)[:, 0]
    return ids, cnt


@pytest.mark.parametrize("bits,dim,n", [(4, 96, 6000), (2, 10, 6000), (1, 300, 5000), (4, 300, 5000)])
def test_every_stored_edge_is_the_encoders_output(cph, oracle, built, num_cus, bits, dim, n):
    """The blocks finalize() leaves (encode_edges_kernel on its production grid, smaller than n: every workgroup encodes
    several vertices, reusing nops[] and -- at dim 300, D = 512 -- its rows in the HBM scratch) against the oracle's encoder
    on the stored vectors of the stored ids: code values from the plane dwords, nop / ip_qo / ip_cp by their bytes, both
    popcounts; edges to exact copies (nop = 0: all-zero code and aux) compared like every other edge.  Checked: 200 seeded
    vertices among the first `grid`, 200 from `grid` on, and every vertex with a copy of its own row among its
    neighbours.  For ALL vertices: 32 distinct neighbours, none the vertex, all < n."""
    b = built(bits, dim, n)
    D, blocks, raw = b["D"], b["blocks"], b["raw"]
    grid, scratch_rows = encode_grid(D, num_cus)
    assert n > grid, (n, grid)
    assert scratch_rows == (D > 256)
    ids, cnt = all_ids(blocks, D, bits)
    assert (cnt == 32).all() and (ids < n).all()
    assert (ids != np.arange(n, dtype=np.uint32)[:, None]).all()
    s = np.sort(ids, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all()
    # (count == 32 everywhere: there are no slots beyond the count that would have to hold kInvalidNode)
    grp = np.unique(raw, axis=0, return_inverse=True)[1].reshape(-1)
    with_copy = np.nonzero((grp[ids] == grp[:, None]).any(axis=1))[0]
    assert len(with_copy) >= n // 20
    rng = np.random.default_rng(bits + dim)
    pick = np.unique(np.concatenate([rng.choice(grid, 200, replace=False), grid + rng.choice(n - grid, 200, replace=False),
                                     with_copy]))
    zero_edges = 0
    for v in pick:
        bi, bc = block_layout.block_ids(blocks[v], D, bits)
        assert bc == 32 and np.array_equal(bi, ids[v])
        vals = block_layout.block_codes(blocks[v], D, bits)
        aux, pops = block_layout.block_aux(blocks[v], D, bits)
        ov, oa, op = oracle.encode_edges(raw[v], raw[bi], D, bits)
        assert np.array_equal(vals, ov), (bits, dim, v, int((vals != ov).sum()))
        assert aux.tobytes() == oa.tobytes(), (bits, dim, v)
        assert np.array_equal(pops, op), (bits, dim, v)
        zero_edges += int((aux[:, 0] == 0).sum())
    assert zero_edges >= len(with_copy)                 # degenerate edges were among the compared ones


def test_renumbering_invariants(built, tmp_path):
    """Hub choice, BFS walk, gather_rows_kernel / gather_u32_kernel / permute_lists_kernel and the row map of a built
    index (bits 4, dim 96, n 6,000: the index of the test above)."""
    bits, dim, n = 4, 96, 6000
    b = built(bits, dim, n)
    ix, X, D, blocks, raw, rows = b["ix"], b["X"], b["D"], b["blocks"], b["raw"], b["rows"]
    rows = np.asarray(rows).astype(np.int64)
    assert np.array_equal(np.sort(rows), np.arange(n))                     # a permutation
    assert raw.shape == (n, dim) and raw.tobytes() == X[rows].tobytes()    # vertex i holds input row rows[i]
    # the padded rows and the norms as the index stores them: from its file (header 68 B, calibration 248 B, profile
    # 72 B, centroid, levels, norms, vectors)
    p = str(tmp_path / "built.idx")
    ix.save(p)
    off = 68 + 248 + 72 + dim * 4 + n * 4
    norms = np.fromfile(p, dtype=np.float32, count=n, offset=off)
    padded = np.fromfile(p, dtype=np.float32, count=n * D, offset=off + n * 4).reshape(n, D)
    assert padded[:, :dim].tobytes() == raw.tobytes() and not padded[:, dim:].any()
    # row_norms_kernel adds dim non-negative products in float32, one fused multiply-add each: every step rounds a partial
    # sum that is at most the final one by at most 2^-24 of it, so the result is within dim * 2^-24 of the exact sum
    # (relative, to first order; the float64 reference's own error is 2^-29 of that).  No slack beyond the bound.
    exact = (X[rows].astype(np.float64) ** 2).sum(1)
    assert (np.abs(norms.astype(np.float64) - exact) <= dim * 2.0 ** -24 * exact).all()
    # vertex 0: all counts are 32, so the hub rule (most edges among the sqrt(n) rows nearest the centroid, the nearest
    # on ties) picks the input row nearest the centroid
    d = ((X.astype(np.float64) - X.astype(np.float64).mean(0)) ** 2).sum(1)
    first, second = np.argsort(d)[:2]
    assert d[second] - d[first] > 1e-9 * d[first]                          # the generator keeps the hub unique
    assert rows[0] == first
    # a BFS from vertex 0 over the stored lists, slots in order, discovers the vertices in the order 0, 1, 2, ...; when
    # the queue runs dry the walk restarts at the smallest input row not yet numbered
    ids, cnt = all_ids(blocks, D, bits)
    assert (cnt == 32).all()
    seen = np.zeros(n, bool)
    row_done = np.zeros(n, bool)
    nxt, restarts = 0, 0
    for v in range(n):
        if v == nxt:                                                       # the queue is empty: v starts a new walk
            if v > 0:
                restarts += 1
                assert rows[v] == np.flatnonzero(~row_done)[0], v
            seen[v] = True
            nxt += 1
        assert seen[v]
        row_done[rows[v]] = True
        for w in ids[v]:
            if not seen[w]:
                assert w == nxt, (v, int(w), nxt)
                seen[w] = True
                nxt += 1
    assert nxt == n
    print("BFS restarts:", restarts)
