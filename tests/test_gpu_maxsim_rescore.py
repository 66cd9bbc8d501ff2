"""Exact rescoring of multi-vector (MaxSim) search on the GPU (CPIndex.search_maxsim(..., rescore=R), search_maxsim_device,
cph_maxsim_rescore_hook).

The yardstick is tests/maxsim_rescore_model.py.  The kernel hook is compared with it and with the host twin on given
candidates against indexes of D = 16, 128 and 2048 whose added rows carry the synthetic key column of the CPU tier (segments
of 1, 63, 64, 65, 200 and more than 2,000 rows, a duplicated vector, twin keys).  An end-to-end call is compared with the
model applied to (search_maxsim at k = R on the same handle, exact_l2 bytes) under every option the underlying search takes.
Every comparison is a byte comparison."""
import functools

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path
from maxsim_model import maxsim_model_batch
from maxsim_rescore_model import (FMAX, I32_MIN, KEY_BIG, KEY_DUP, KEY_HALF, SEG_KEYS, hook_maxsim_rescore, host_maxsim_rescore,
                                  rescore_model_batch, same_bytes, synth_candidates, synth_index)
from test_gpu_maxsim import _keys_for, _open, _tokens, built  # noqa: F401  (built: the 8,230 x 16 fixture)

pytestmark = pytest.mark.gpu

KEY_BASE = 77                                               # the key of every row of the loaded fixture
MUST = tuple(SEG_KEYS.values()) + (KEY_DUP, -5, 900, KEY_HALF, KEY_BASE, I32_MIN, 2 ** 31 - 1, -1)


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


class Dists:
    """dist_rows(q, t) of the model from the handle: exact_l2 of the token (cosine: normalised as the search does) against
    every id, computed once per token."""

    def __init__(self, ix, tok, cosine=False):
        from cosine_model import model
        self.ix, self.rows = ix, {}
        self.tok = model(tok.reshape(-1, tok.shape[2])).reshape(tok.shape) if cosine else tok
        self.all = np.arange(ix.size, dtype=np.uint32)

    def __call__(self, q, t):
        if (q, t) not in self.rows:
            self.rows[q, t] = self.ix.exact_l2(self.tok[q, t], self.all)
        return self.rows[q, t]


def _stored(ix):
    """(raw [size, D] zero-padded, norm_sq [size]) of the handle for the host twin: exact_l2 of the zero vector is
    (+0 + norm) - 2 * 0 = the stored norm, bit for bit."""
    D = 16
    while D < ix.dim:
        D *= 2
    raw = np.zeros((ix.size, D), np.float32)
    raw[:, :ix.dim] = ix.get_vectors(0, ix.size)
    return raw, ix.exact_l2(np.zeros(ix.dim, np.float32), np.arange(ix.size, dtype=np.uint32))


# ---- the kernels against the host twin and the model ---------------------------------------------------------------------------
# name of the fixture: (big, labels instead of a keys object, cases); a case: (T, n_tokens, R, k, found per query, allow kind, ids)
HOOK = {
    "g16": (2100, False, (
        (9, (1, 7, 8, 9, 9, 9), 48, 10, (48, 48, 30, 5, 48, 1), None, "internal"),
        (9, (9, 8, 1), 48, 10, (48, 40, 48), "one", "internal"),
        (9, (9, 7, 9, 1), 32, 32, (32, 32, 20, 32), "each", "input"),
        (3, (3, 2), 1024, 10, (54, 9), None, "internal"),
        (2, (2,), 1024, 1024, (54,), "each", "internal"),
        (64, (64, 33), 1, 1, (1, 1), None, "internal"))),
    "g128": (0, True, (
        (64, (64, 33), 1, 1, (1, 1), None, "internal"),
        (64, (64, 1), 7, 7, (7, 3), "one", "input"),
        (9, (1, 7, 8, 9), 48, 10, (48, 48, 48, 48), None, "internal"))),
    "g2048": (0, False, (
        (3, (3, 1), 16, 4, (16, 2), None, "internal"),
        (9, (9, 8, 7, 1), 48, 10, (48, 48, 48, 20), "each", "input"))),
}


def _allow(kind, key_of, n, seed):
    if kind is None:
        return None
    rng = np.random.default_rng(seed)

    def one():
        a = rng.random(len(key_of)) < 0.5
        for key in np.unique(key_of):
            members = np.flatnonzero(key_of == key)
            if key == SEG_KEYS[64]:
                a[members] = False                            # this key keeps ONE allowed row
            if not a[members].any():
                a[rng.choice(members)] = True
        return a
    return one() if kind == "one" else np.stack([one() for _ in range(n)])


@pytest.mark.parametrize("name", sorted(HOOK))
def test_hook_matches_host_twin_and_model(cph, name):
    big, use_labels, cases = HOOK[name]
    spec = DATASETS[name]
    bits = spec["bits"][0]
    ix = cph.CPIndex(spec["dim"], bits)
    ix.load(fixture_path(name, bits))
    n0 = ix.size
    ix.set_row_map(np.random.default_rng(5).permutation(n0))
    syn = synth_index(spec["D"], spec["dim"], big)
    key_of = np.concatenate([np.full(n0, KEY_BASE, np.int32), syn["key_of"]])
    if use_labels:
        ix.set_labels(key_of[:n0], ids="internal")
        ix.add(syn["raw"][:, :spec["dim"]], labels=syn["key_of"])
        keys = None
    else:
        ix.add(syn["raw"][:, :spec["dim"]])
        keys = ix.make_group_keys(key_of, ids="internal")
    size = ix.size
    assert size == n0 + len(syn["key_of"]) and (big == 0 or (key_of == KEY_BIG).sum() >= 2000)
    raw, norm = _stored(ix)
    lo, hi = n0 + syn["dup"][0], n0 + syn["dup"][1]
    assert raw[lo].tobytes() == raw[hi].tobytes() and norm[lo].tobytes() == norm[hi].tobytes()
    rng = np.random.default_rng(len(name))
    for c, (T, n_tokens, R, k, founds, akind, space) in enumerate(cases):
        n = len(n_tokens)
        nt = np.array(n_tokens, np.int32)
        tok = (raw[rng.integers(0, size, (n, T)), :ix.dim] + np.float32(0.3) * rng.standard_normal((n, T, ix.dim))).astype(np.float32)
        tok[:, 0] = raw[lo, :ix.dim]                          # token 0 IS the duplicated vector: the lower id wins the tie
        for q, L in enumerate(n_tokens):
            tok[q, L:] = np.float32(1e30)                     # garbage in the ignored rows
        must = MUST + ((KEY_BIG,) if big else ())
        ck, lb, cf = synth_candidates(key_of, n, R, founds, seed=c, must=must)
        allow = _allow(akind, key_of, n, seed=R + T)
        ix.result_ids = space
        rows = ix.row_map().astype(np.uint32) if space == "input" else None
        want = rescore_model_batch(ck, lb, cf, nt, T, key_of, Dists(ix, tok), allow, k, rows)
        assert same_bytes(host_maxsim_rescore(ck, lb, cf, tok, nt, raw, norm, key_of, allow, k, rows), want), (name, c, "host twin")
        assert same_bytes(hook_maxsim_rescore(ix, ck, lb, cf, tok, nt, keys, allow, k), want), (name, c, "kernels")
        if np.all(nt == T):
            assert same_bytes(hook_maxsim_rescore(ix, ck, lb, cf, tok, None, keys, allow, k), want), (name, c, "no n_tokens")
    ix.result_ids = "internal"
    if keys is not None:
        keys.close()


def test_hook_special_keys_are_answered_in_key_order(cph):
    """R = k over every distinct key of the column: the duplicated vector reports its lower id, the twin keys tie on the
    score and the smaller key comes first; found < R."""
    spec = DATASETS["g16"]
    ix = cph.CPIndex(spec["dim"], 1)
    ix.load(fixture_path("g16", 1))
    n0 = ix.size
    syn = synth_index(spec["D"], spec["dim"], 0)
    key_of = np.concatenate([np.full(n0, KEY_BASE, np.int32), syn["key_of"]])
    ix.add(syn["raw"][:, :spec["dim"]])
    keys = ix.make_group_keys(key_of, ids="internal")
    U = len(np.unique(key_of))
    R = k = 64
    assert U < R
    ck, lb, cf = synth_candidates(key_of, 2, R, (U, U), seed=1, must=MUST)
    tok = np.repeat(syn["raw"][None, syn["dup"][0]:syn["dup"][0] + 1, :spec["dim"]], 2, axis=0).copy()
    tok = np.concatenate([tok, tok + np.float32(0.5)], axis=1)
    got = hook_maxsim_rescore(ix, ck, lb, cf, tok, None, keys, None, k)
    assert same_bytes(got, rescore_model_batch(ck, lb, cf, None, 2, key_of, Dists(ix, tok), None, k))
    for q in range(2):
        slots = {int(key): j for j, key in enumerate(got[0][q, :got[4][q]])}
        assert got[4][q] == U == got[5][q] and got[3][q, slots[KEY_DUP], 0] == n0 + syn["dup"][0]
        assert slots[900] == slots[-5] + 1 and got[1][q, slots[900]].tobytes() == got[1][q, slots[-5]].tobytes()
        assert (got[0][q, U:] == 0).all() and (got[1][q, U:] == FMAX).all() and (got[3][q, U:] == -1).all()
    keys.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _expect(ix, tok, n_tokens, k, R, C_, key_of, allow, cosine=False, **kw):
    """The statement: the model applied to the lower-bound call at k = R on the same handle and exact_l2 bytes."""
    low = ix.search_maxsim(tok, R, n_tokens=n_tokens, candidates=C_, **kw)
    rows = ix.row_map() if ix.result_ids == "input" else None
    return rescore_model_batch(low[0], low[1], low[4], n_tokens, tok.shape[1], np.asarray(key_of, np.int32), Dists(ix, tok, cosine), allow,
                               k, rows)


STATES = ("plain", "input", "removed", "added")
FIXTURES = [("g1024", 2), ("g2048", 1), ("built", 1)]


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name,bits", FIXTURES)
def test_end_to_end_options(cph, gold, built, name, bits, state):  # noqa: F811
    ix, Q = _open(cph, gold, built, name, bits)
    n0 = ix.size
    rng = np.random.default_rng(n0 + len(state))
    key_of = _keys_for(n0, n0)
    if name == "built":
        key_of[:2000] = 5000 + np.arange(2000) // 40          # the clustered rows: documents of forty
    ix.set_labels(key_of, ids="internal")
    live = np.ones(n0, bool)
    if state == "input":
        ix.result_ids = "input"
    if state in ("removed", "added"):
        gone = rng.choice(n0, n0 // 5, replace=False)
        assert ix.remove(gone, ids="internal") == len(gone)
        live[gone] = False
    if state == "added":
        twin = ix.get_vectors(5, 1)
        extra = np.concatenate([twin, twin + np.float32(0.25), rng.standard_normal((6, ix.dim)).astype(np.float32)])
        extra_keys = np.array([777777, int(key_of[5]), 0, 0, 1, 424242, I32_MIN, -1], np.int64)
        ix.add(extra, labels=extra_keys)
        key_of = np.concatenate([key_of, extra_keys])
        live = np.concatenate([live, np.ones(len(extra_keys), bool)])
    n = ix.size
    mask = rng.random(n) < 0.4
    small = rng.random(n) < 0.08
    f = ix.make_filter(mask, ids="internal")
    f2 = ix.make_filter(small, ids="internal")
    empty = ix.make_filter(np.zeros(n, bool), ids="internal")
    nq = 4
    fo = np.array([-1, 0, 1, 2])
    lab = key_of[rng.integers(0, n, nq)]
    per_query = np.stack([live, mask & live, small & live, np.zeros(n, bool)])
    by_label = np.stack([(key_of == x) & live for x in lab])
    variants = [(dict(), live), (dict(exact=True), live), (dict(filter=f), mask & live), (dict(filter=f, exact=True), mask & live),
                (dict(filter=empty), np.zeros(n, bool)), (dict(label=lab, exact=True), by_label),
                (dict(filter=[f, f2, empty], filter_of=fo, exact=True), per_query)]
    if state != "added":        # (inherited: per-query filters would walk the graph of an index with a tail)
        variants += [(dict(label=lab), by_label), (dict(filter=[f, f2, empty], filter_of=fo), per_query)]
    other = (key_of * 7 + 3) % 11                             # a second column: other keys
    gk_other = ix.make_group_keys(other, ids="internal")
    for (T, C_, k, R) in ((1, 70, 3, 3), (9, 40, 3, 24)):
        tok, n_tokens = _tokens(Q, nq, T, n0 + T)
        for kw, allow in variants:
            got = ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=C_, rescore=R, **kw)
            assert [g.shape for g in got] == [(nq, k), (nq, k), (nq, k), (nq, k, T), (nq,), (nq,)]
            assert same_bytes(got, _expect(ix, tok, n_tokens, k, R, C_, key_of, allow, **kw)), (name, state, T, R, sorted(kw))
            real = np.arange(k)[None, :] < got[4][:, None]
            assert (got[2][real] == np.broadcast_to(n_tokens[:, None], (nq, k))[real]).all() and (got[5] <= got[4]).all()
    got_o = ix.search_maxsim(tok, 3, n_tokens=n_tokens, candidates=C_, keys=gk_other, filter=f, rescore=11)
    assert same_bytes(got_o, _expect(ix, tok, n_tokens, 3, 11, C_, other, mask & live, keys=gk_other, filter=f))
    assert got_o[4].max() == 3
    for x in (f, f2, empty, gk_other):
        x.close()


def test_cosine_metric(cph):
    rng = np.random.default_rng(11)
    n, dim = 2500, 24
    X = (rng.standard_normal((n, dim)) * rng.uniform(0.2, 5.0, (n, 1))).astype(np.float32)
    ix = cph.CPIndex(dim, 4, metric="cosine")
    ix.build(X)
    ix.finalize()
    key_of = np.arange(n) // 5 - 7                            # documents of five chunks
    ix.set_labels(key_of, ids="internal")
    Q = rng.standard_normal((8, dim)).astype(np.float32)
    tok, n_tokens = _tokens(Q, 4, 9, 9)
    tok[:-1] *= np.float32(3.0)                               # (the length of a query vector does not matter)
    for kw in (dict(), dict(exact=True)):
        got = ix.search_maxsim(tok, 10, n_tokens=n_tokens, candidates=40, rescore=32, **kw)
        assert same_bytes(got, _expect(ix, tok, n_tokens, 10, 32, 40, key_of, None, cosine=True, **kw)), sorted(kw)
        assert (got[4] == 10).all() and (got[1][:, :10] <= n_tokens[:, None] + 1e-3).all()


# ---- the claims ------------------------------------------------------------------------------------------------------------------
def test_certified_slots_are_the_true_top_slots(cph, gold):
    """exact=True at C = 16 over 41 documents of seven or eight rows: the scores rise over their lower bounds, and the
    certified leading slots are the brute-force MaxSim top slots over all rows, in order; R = all documents certifies all."""
    ix, Q = _open(cph, gold, None, "g16", 1)
    size = ix.size
    key_of = (np.arange(size) * 7 % 41 - 3).astype(np.int32)
    ix.set_labels(key_of, ids="internal")
    T, k = 8, 10
    tok, n_tokens = _tokens(Q, 6, T, 3)
    ukeys = np.unique(key_of)
    dists = Dists(ix, tok)
    true_keys, true_score = [], []
    for q in range(len(tok)):
        score = np.zeros(len(ukeys), np.float32)
        for t in range(int(n_tokens[q])):
            best = np.full(len(ukeys), np.inf, np.float32)
            np.minimum.at(best, np.searchsorted(ukeys, key_of), dists(q, t))
            score = (score + best).astype(np.float32)
        o = np.lexsort((ukeys, score))
        true_keys.append(ukeys[o])
        true_score.append(score[o])
    rose = certified = 0
    for R in (10, 16, 41):
        low = ix.search_maxsim(tok, R, n_tokens=n_tokens, candidates=16, exact=True)
        got = ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=16, exact=True, rescore=R)
        for q in range(len(tok)):
            lb_of = dict(zip(low[0][q, :low[4][q]].tolist(), low[1][q, :low[4][q]]))
            for o in range(got[4][q]):
                assert got[1][q, o] >= lb_of[int(got[0][q, o])]
                rose += int(got[1][q, o] > lb_of[int(got[0][q, o])])
            c = got[5][q]
            assert np.array_equal(got[0][q, :c], true_keys[q][:c]) and got[1][q, :c].tobytes() == true_score[q][:c].tobytes(), (R, q)
            certified += c
            if low[4][q] < R:                                 # the candidates are ALL keys any token saw
                assert c == got[4][q]
    assert rose > 0 and certified > 0


def test_rescore_none_is_the_plain_call(cph, gold):
    ix, Q = _open(cph, gold, None, "g16", 1)
    key_of = _keys_for(ix.size, 3)
    ix.set_labels(key_of, ids="internal")
    tok, n_tokens = _tokens(Q, 5, 4, 2)
    was, ix.result_ids = ix.result_ids, "internal"
    ids, dist = ix.search_batch(tok.reshape(20, -1), 30)
    ix.result_ids = was
    want = maxsim_model_batch(ids.reshape(5, 4, 30), dist.reshape(5, 4, 30), n_tokens, key_of.astype(np.int32), ix.size, 6)
    before = ix.search_maxsim(tok, 6, n_tokens=n_tokens, candidates=30)
    ix.search_maxsim(tok, 6, n_tokens=n_tokens, candidates=30, rescore=12)
    for got in (before, ix.search_maxsim(tok, 6, n_tokens=n_tokens, candidates=30, rescore=None),
                ix.search_maxsim(tok, 6, n_tokens=n_tokens, candidates=30)):
        assert len(got) == 5 and same_bytes(got, want)


# ---- the inverted key column's cache ---------------------------------------------------------------------------------------------
def test_key_rows_follow_the_column(cph, gold):
    ix, Q = _open(cph, gold, None, "g16", 1)
    n0 = ix.size
    key_of = (np.arange(n0) % 37).astype(np.int64)
    ix.set_labels(key_of, ids="internal")
    ix.prepare_maxsim_rescore()
    tok, n_tokens = _tokens(Q, 4, 3, 1)
    kw = dict(n_tokens=n_tokens, candidates=30, exact=True, rescore=20)
    assert same_bytes(ix.search_maxsim(tok, 5, **kw), _expect(ix, tok, n_tokens, 5, 20, 30, key_of, None, exact=True))
    gk = ix.make_group_keys(key_of[::-1].copy(), ids="internal")
    ix.prepare_maxsim_rescore(gk)
    assert same_bytes(ix.search_maxsim(tok, 5, keys=gk, **kw), _expect(ix, tok, n_tokens, 5, 20, 30, key_of[::-1], None, exact=True, keys=gk))
    # set_labels: the next call walks the new column
    key2 = (np.arange(n0) % 11 - 5).astype(np.int64)
    ix.set_labels(key2, ids="internal")
    assert same_bytes(ix.search_maxsim(tok, 5, **kw), _expect(ix, tok, n_tokens, 5, 20, 30, key2, None, exact=True))
    # add: a row that IS token 0 of query 0, under key 3: the rebuilt column holds it and it is that token's best row
    first = ix.add(tok[0, :1], labels=[3])
    key3 = np.concatenate([key2, [3]])
    got = ix.search_maxsim(tok, 11, **kw)                      # (k = the eleven keys of the column: key 3 is answered)
    assert same_bytes(got, _expect(ix, tok, n_tokens, 11, 20, 30, key3, None, exact=True))
    slot = got[0][0, :got[4][0]].tolist().index(3)
    assert got[3][0, slot, 0] == first[0] == n0
    with pytest.raises(ValueError, match=f"cover {n0} ids, the index holds {n0 + 1}"):
        ix.search_maxsim(tok, 5, keys=gk, **kw)
    gk.close()


# ---- the device variant, replicas -------------------------------------------------------------------------------------------------
def test_device_variant(cph, gold):
    import torch
    ix, Q = _open(cph, gold, None, "g16", 1)
    n = ix.size
    key_of = _keys_for(n, 3)
    ix.set_labels(key_of, ids="internal")
    dev = torch.device("cuda", 0)
    T, k, C_, R = 5, 6, 40, 17
    tok, n_tokens = _tokens(Q, 7, T, 9)
    nq = len(tok)
    Td = torch.from_numpy(tok).to(dev)
    f = ix.make_filter(np.arange(n) % 3 != 0, ids="internal")
    fo = np.arange(nq) % 2 - 1
    st1 = torch.cuda.Stream(dev)
    st1.wait_stream(torch.cuda.current_stream(dev))
    for kw in (dict(), dict(n_tokens=n_tokens), dict(n_tokens=n_tokens, exact=True), dict(n_tokens=n_tokens, filter=f),
               dict(n_tokens=n_tokens, filter=[f], filter_of=fo), dict(n_tokens=n_tokens, label=0)):
        want = ix.search_maxsim(tok, k, candidates=C_, rescore=R, **kw)
        got = ix.search_maxsim_device(Td, k, candidates=C_, rescore=R, **kw)
        torch.cuda.synchronize()
        assert len(got) == 6 and same_bytes([t.cpu().numpy() for t in got], want), sorted(kw)
        out = [torch.full(w.shape, -9, dtype=getattr(torch, w.dtype.name), device=dev) for w in want]
        st1.wait_stream(torch.cuda.current_stream(dev))
        res = ix.search_maxsim_device(Td, k, candidates=C_, rescore=R, out=out, stream=st1, **kw)
        with torch.cuda.stream(st1):
            copies = [t.clone() for t in res]
        st1.synchronize()
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
        assert same_bytes([t.cpu().numpy() for t in copies], want), sorted(kw)
    with pytest.raises(ValueError, match="six tensors"):
        ix.search_maxsim_device(Td, k, candidates=C_, rescore=R, out=out[:5])
    # more calls than the handle has scratch sets, at growing shapes, plain calls in between
    for R2 in (6, 40, 200, 12, 1024):
        want = ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=C_, rescore=R2)
        ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=C_)
        got = ix.search_maxsim_device(Td, k, n_tokens=n_tokens, candidates=C_, rescore=R2)
        torch.cuda.synchronize()
        assert same_bytes([t.cpu().numpy() for t in got], want), R2
    ix.time_maxsim_rescore(True)
    ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=C_, rescore=R)
    assert ix.last_maxsim_rescore_us() > 0
    ix.time_maxsim_rescore(False)
    ix.synchronize()
    f.close()


def test_replicas_equal_one_device(cph, gold):
    name, bits = "g16", 1
    one, _ = _open(cph, gold, None, name, bits)
    Q = gold[f"Q/{name}"]
    m = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0])
    m.set_min_shard(1)
    m.load(fixture_path(name, bits))
    m.set_row_map(one.row_map())
    n = one.size
    key_of = _keys_for(n, 9)
    other = (key_of * 5 + 1) % 13
    mask = np.arange(n) % 4 != 1
    tok, n_tokens = _tokens(Q, 9, 4, 2)                        # nine queries over two replicas: shards of five and four
    fo = np.arange(len(tok)) % 3 - 1
    for ix in (one, m):
        ix.set_labels(key_of, ids="internal")
    m.prepare_maxsim_rescore()
    for ids in ("internal", "input"):
        one.result_ids = m.result_ids = ids
        gk1, gkm = one.make_group_keys(other, ids="internal"), m.make_group_keys(other, ids="internal")
        f1, fm = one.make_filter(mask, ids="internal"), m.make_filter(mask, ids="internal")
        e1, em = one.make_filter(~mask, ids="internal"), m.make_filter(~mask, ids="internal")
        for kw1, kwm in ((dict(), dict()), (dict(exact=True), dict(exact=True)), (dict(filter=f1), dict(filter=fm)),
                         (dict(keys=gk1, filter=f1, exact=True), dict(keys=gkm, filter=fm, exact=True)),
                         (dict(filter=[f1, e1], filter_of=fo), dict(filter=[fm, em], filter_of=fo)), (dict(label=0), dict(label=0))):
            assert same_bytes(m.search_maxsim(tok, 6, n_tokens=n_tokens, candidates=40, rescore=20, **kwm),
                              one.search_maxsim(tok, 6, n_tokens=n_tokens, candidates=40, rescore=20, **kw1)), (ids, sorted(kw1))
        for x in (gk1, gkm, f1, fm, e1, em):
            x.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(cph, gold):
    import torch
    ix, Q = _open(cph, gold, None, "g16", 1)
    ix.set_labels(np.arange(ix.size) % 7, ids="internal")
    tok, n_tokens = _tokens(Q, 4, 3, 1)
    for bad in (2, 1025, 0, -1):
        with pytest.raises(ValueError, match="k <= rescore <= 1024"):
            ix.search_maxsim(tok, 3, candidates=20, rescore=bad)
    with pytest.raises(ValueError, match="integer"):
        ix.search_maxsim(tok, 3, candidates=20, rescore=True)
    with pytest.raises(ValueError, match="k <= rescore <= 1024"):
        ix.search_maxsim_device(torch.from_numpy(tok).to("cuda:0"), 3, candidates=20, rescore=2)
    # the library's own refusals name the limit too (the Python checks are in front of them)
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    o = (np.empty((4, 3), np.int32), np.empty((4, 3), np.float32), np.empty((4, 3), np.int32), np.empty((4, 3, 3), np.int64),
         np.empty(4, np.int32), np.empty(4, np.int32))
    po = [x.ctypes.data for x in o]
    for R, what in ((2, b"k <= rescore <= 1024"), (1025, b"k <= rescore <= 1024")):
        assert L.cph_search_maxsim_rescored(ix._h, tok.ctypes.data, 4, 3, None, 3, 20, R, None, None, 0, None, 0, *po) == _lib.INVALID_ARGUMENT
        assert what in L.cph_last_error()
    assert ix.search_maxsim(np.zeros((0, 3, ix.dim), np.float32), 3, candidates=20, rescore=5)[5].shape == (0,)   # an empty batch is no error
    with pytest.raises(ValueError, match="no timed rescored maxsim search"):
        ix.last_maxsim_rescore_us()
    ip = cph.CPIndex(ix.dim, 1, metric="ip")
    ip.build(np.random.default_rng(1).standard_normal((300, ix.dim)).astype(np.float32))
    ip.finalize()
    ip.set_labels(np.arange(300) % 7, ids="internal")
    with pytest.raises(ValueError, match=r"inner-product \(ip\) metric"):
        ip.search_maxsim(tok, 3, candidates=20, rescore=5)
    with pytest.raises(ValueError, match=r"inner-product \(ip\) metric"):
        ip.prepare_maxsim_rescore()
    p = cph.CPIndex(DATASETS["g16"]["dim"], 1, devices=[0, 0], partition=True)
    with pytest.raises(ValueError, match="partitioned"):
        p.search_maxsim(tok, 3, rescore=5)
    with pytest.raises(ValueError, match="partitioned"):
        p.search_maxsim_device(torch.from_numpy(tok).to("cuda:0"), 3, rescore=5)
    with pytest.raises(ValueError, match="partitioned"):
        p.prepare_maxsim_rescore()
