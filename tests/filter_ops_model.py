"""numpy statement of the filter algebra (cph_filters_combine), shared by tests/test_filter_ops_host.py and
tests/test_gpu_filter_ops.py: the expected words and counts never come from the code under test."""
import numpy as np

OPS = {"and": 0, "or": 1, "andnot": 2, "xor": 3, "not": 4}


def nwords(n_bits):
    return (n_bits + 31) // 32


def clean(words, n_bits):
    """words [..., nw] with the bits at or above n_bits cleared."""
    w = np.array(words, np.uint32, copy=True)
    if n_bits & 31 and w.shape[-1]:
        w[..., -1] &= np.uint32((1 << (n_bits & 31)) - 1)
    return w


def popcounts(words):
    w = np.ascontiguousarray(words, np.uint32)
    if w.shape[-1] == 0:
        return np.zeros(w.shape[0], np.uint64)
    return np.unpackbits(w.view(np.uint8), axis=-1).sum(axis=-1).astype(np.uint64)


def expect(op, a, b, n_bits):
    """a [m][nw], b [m][nw] or [1][nw] (broadcast) or None -> (words [m][nw], counts [m])."""
    a = np.asarray(a, np.uint32)
    if op == "not":
        w = ~a
    else:
        bb = np.broadcast_to(np.asarray(b, np.uint32), a.shape)
        w = {"and": a & bb, "or": a | bb, "andnot": a & ~bb, "xor": a ^ bb}[op]
    w = clean(w, n_bits)
    return w, popcounts(w)


def operands(n_bits, m, seed):
    """Random words with dirty bits behind n_bits; with three filters or more, a[1] all ones, a[2] all zeros against an
    all-ones b[2], so the all-zero and the all-ones operand meet every op."""
    rng = np.random.default_rng(seed)
    nw = nwords(n_bits)
    a = rng.integers(0, 2 ** 32, (m, nw), dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 2 ** 32, (m, nw), dtype=np.uint64).astype(np.uint32)
    if m > 2:
        a[1] = 0xFFFFFFFF
        a[2] = 0
        b[2] = 0xFFFFFFFF
    return a, b


def cases():
    """(op, broadcast) of every form of a call."""
    return [(op, bc) for op in OPS for bc in (False, True) if not (op == "not" and bc)]
