"""The cosine metric's row normalisation in numpy (csrc/host_normalize.h and csrc/device_normalize.h state the same):
out = x / sqrt(2 |x|^2), float32 throughout, in the operation order of the kernel's wave.

    p_l = +0;  for j = l, l + 64, ... < dim:  p_l = p_l + (x[j] * x[j])      l = 0..63   (product and sum rounded apart)
    s   = xor butterfly over the 64 p_l, distances 32, 16, 8, 4, 2, 1:  p_l = p_l + p_(l ^ d)
    t   = sqrt(s + s);  out[j] = x[j] / t                                     (np.sqrt and / are correctly rounded)

A row is bad when not (0 < t < inf): its outputs are +0.0, it is counted, the lowest bad row is reported (NO_BAD_ROW when
there is none).  Padding a row with +0.0 up to a multiple of 64 changes no bit: p + (+0 * +0) == p for every p this sum
can hold (it starts at +0 and never becomes -0), so the model sums whole chunks of 64."""
import numpy as np

NO_BAD_ROW = 2 ** 64 - 1
DIMS = (1, 3, 63, 64, 65, 127, 128, 130, 960)      # both sides of the 64-lane stride, and the multi-pass loop
NS = (1, 3, 130)                                   # 130 rows: more than one workgroup of four waves
BAD_KINDS = ("zero", "nan", "inf", "overflow")


def normalize_model(x):
    """x [n, dim] float32 -> (out [n, dim] float32, bad_count, first_bad)."""
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    chunks = (dim + 63) // 64
    with np.errstate(all="ignore"):
        sq = np.zeros((n, chunks * 64), np.float32)
        sq[:, :dim] = x * x
        p = np.zeros((n, 64), np.float32)
        for c in range(chunks):
            p = p + sq[:, c * 64:(c + 1) * 64]
        lanes = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            p = p + p[:, lanes ^ d]
        assert (p.view(np.uint32) == p[:, :1].view(np.uint32)).all() or np.isnan(p).any()      # every lane ends with s
        s = p[:, 0]
        t = np.sqrt(s + s)
        good = (t > 0) & (t < np.inf)
        out = np.zeros_like(x)
        out[good] = x[good] / t[good, None]
    assert out.dtype == np.float32
    bad = np.flatnonzero(~good)
    return out, int(bad.size), int(bad[0]) if bad.size else NO_BAD_ROW


def model(x):
    """The rows as a cosine index stores them (no bad row allowed)."""
    out, bad, _ = normalize_model(x)
    assert bad == 0
    return out


def case_rows(n, dim, seed=0):
    """Gaussian rows times per-row scales 2^-20 .. 2^20 (both ends present when n >= 2)."""
    rng = np.random.default_rng(1000 * dim + n + seed)
    e = rng.integers(-20, 21, n)
    e[0] = 20
    e[-1] = -20 if n > 1 else e[-1]
    return (rng.standard_normal((n, dim)) * np.exp2(e)[:, None]).astype(np.float32)


def bad_row(kind, dim, rng):
    r = rng.standard_normal(dim).astype(np.float32)
    if kind == "zero":
        r[:] = 0.0
        r[::2] = -0.0                    # (negative zeros too: the outputs must be +0.0 all the same)
    elif kind == "nan":
        r[rng.integers(0, dim)] = np.nan
    elif kind == "inf":
        r[rng.integers(0, dim)] = -np.inf if dim % 2 else np.inf
    elif kind == "overflow":
        r[:] = 3e38
    else:
        raise ValueError(kind)
    return r


def bad_cases(dim, n=7, seed=0):
    """[(kind, position, x)]: each kind of bad row at row 0, in the middle and last of n Gaussian rows."""
    out = []
    for ki, kind in enumerate(BAD_KINDS):
        for pos in (0, n // 2, n - 1):
            rng = np.random.default_rng(seed + 10 * ki + pos + 100 * dim)
            x = case_rows(n, dim, seed=ki + 1)
            x[pos] = bad_row(kind, dim, rng)
            out.append((kind, pos, x))
    return out


def cases():
    return [(n, dim) for dim in DIMS for n in NS]
