"""The scratch sets and the staged host table of the re-rankers, shared by maxsim, rescored maxsim, fused and two-stage
rescored search on ONE handle (what test_rerankers_share_scratch_at_growing_shapes does for grouped, maxsim and diverse).

Every step runs five times -- one more than the handle has scratch sets, so every set's table and buffers are reused -- and
the steps are ordered so that the table grows (lengths; then pointers, filter_of and lengths; then weights and lengths), is
skipped, shrinks and is sent in the first layout again, while the staged full queries and the candidate buffers grow in
between.  Every answer is the model's, byte for byte, computed the way each feature's own end-to-end test does."""
import numpy as np
import pytest

from maxsim_model import same_bytes
from test_gpu_fused import _expect as _expect_fused
from test_gpu_fused import _queries
from test_gpu_maxsim import _expect as _expect_maxsim
from test_gpu_maxsim import _keys_for, _open, _tokens
from test_gpu_maxsim_rescore import _expect as _expect_maxsim_rescored
from test_gpu_rescore import _expect as _expect_rescored
from test_gpu_rescore import _object_over, _prefix_data

pytestmark = pytest.mark.gpu

C_ = 64
REPS = 5                                                    # kMaxBatchSets + 1


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def test_newer_rerankers_share_scratch_and_the_staged_table(cph, gold):
    import torch
    ix, Q = _open(cph, gold, None, "g16", 1)
    n = ix.size
    key_of = _keys_for(n, 2)
    ix.set_labels(key_of, ids="internal")
    rng = np.random.default_rng(3)
    masks = [rng.random(n) < 0.4, rng.random(n) < 0.1]
    f0, f1 = (ix.make_filter(m, ids="internal") for m in masks)
    T = 4
    tok2, nt2 = _tokens(Q, 2, T, 1)
    tok6, nt6 = _tokens(Q, 6, T, 2)
    tok3, _ = _tokens(Q, 3, T, 3)
    tok3[-1, 1:] = tok3[0, :T - 1]                          # (every token is live: no n_tokens)
    fo6 = np.array([-1, 0, 1, 1, 0, -1])
    allow6 = np.stack([np.ones(n, bool) if f < 0 else masks[f] for f in fo6])
    fq6, fq2 = _queries(Q, 6, T, 4), _queries(Q, 2, T, 5)
    w6 = rng.uniform(-1.0, 2.0, (6, T)).astype(np.float32)
    nv6 = np.array([T, 1, 2, T, 3, 1], np.int32)
    full, FQ = _prefix_data(ix, 24, 6, 6)
    Qr = np.ascontiguousarray(FQ[:, :ix.dim])
    obj = _object_over(ix, full, "float16", "l2")

    # (name of the search, its positional arguments, its keyword arguments, the model's answer)
    steps = [
        ("maxsim", (tok2, 4), dict(n_tokens=nt2), _expect_maxsim(ix, tok2, nt2, 4, C_, key_of)),
        ("maxsim", (tok6, 4), dict(n_tokens=nt6, rescore=8, filter=[f0, f1], filter_of=fo6),
         _expect_maxsim_rescored(ix, tok6, nt6, 4, 8, C_, key_of, allow6, filter=[f0, f1], filter_of=fo6)),
        ("fused", (fq6, 8), dict(weights=w6, n_vectors=nv6), _expect_fused(ix, fq6, 8, C_, w6, nv6)[0]),
        ("rescored", (Qr, 5, obj[0]), dict(full_queries=FQ), _expect_rescored(ix, obj, Qr, FQ, 5, C_)),
        ("maxsim", (tok3, 3), dict(rescore=6, filter=f0), _expect_maxsim_rescored(ix, tok3, None, 3, 6, C_, key_of, masks[0], filter=f0)),
        ("fused", (fq2, 8), dict(weights=None), _expect_fused(ix, fq2, 8, C_, None, None)[0]),
        ("maxsim", (tok6, 4), dict(n_tokens=nt6), _expect_maxsim(ix, tok6, nt6, 4, C_, key_of)),
    ]
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)

    def on_device(x):
        return torch.from_numpy(x).to(dev) if isinstance(x, np.ndarray) and x.dtype == np.float32 else x
    for device_form in (False, True):
        for step, (name, args, kw, want) in enumerate(steps):
            want = [np.asarray(w) for w in want]
            for rep in range(REPS):
                if device_form:
                    d_args = tuple(on_device(a) for a in args)
                    d_kw = {key: on_device(v) if key == "full_queries" else v for key, v in kw.items()}
                    out = [torch.full(w.shape, 9, dtype=getattr(torch, w.dtype.name), device=dev) for w in want]
                    st.wait_stream(torch.cuda.current_stream(dev))
                    got = getattr(ix, f"search_{name}_device")(*d_args, candidates=C_, out=out, stream=st, **d_kw)
                    st.synchronize()
                    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
                    got = [t.cpu().numpy() for t in got]
                else:
                    got = [np.asarray(g) for g in getattr(ix, f"search_{name}")(*args, candidates=C_, **kw)]
                assert len(got) == len(want) and same_bytes(got, want), (device_form, step, name, rep)
    ix.synchronize()
    for x in (f0, f1, obj[0]):
        x.close()
