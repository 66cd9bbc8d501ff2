"""The slack of the matrix prefilter (cph_host_exact_matrix_slack, csrc/host_exact_mfma.h) against float64: both float32
paths of a distance -- the eight-chain path of the vector scan and the one-chain path of the matrix cores -- emulated in
numpy, must lie within the slack of each other and of the real number they round."""
import ctypes as C

import numpy as np
import pytest

from cphnsw_mi355x import _lib

f32, f64 = np.float32, np.float64


def _fma(a, b, c):
    # float32 rounding of the float64 a * b + c.  The product of two float32 is exact in float64; the sum is rounded to
    # float64 and then to float32 -- a DOUBLE rounding, which differs from a true fmaf only on a float64 result within
    # 2^-53 relative of a float32 midpoint, and by one float32 ulp there: both are roundings the bound allows for.
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _dot8(x, y):
    c = np.zeros((x.shape[0], 8), f32)
    for i in range(0, x.shape[1], 8):
        c = _fma(x[:, i:i + 8], y[:, i:i + 8], c)
    return ((c[:, 0] + c[:, 4]) + (c[:, 1] + c[:, 5])) + ((c[:, 2] + c[:, 6]) + (c[:, 3] + c[:, 7]))


def _pairs(D, rng):
    n = 96
    q = rng.standard_normal((4 * n, D)).astype(f32)
    b = rng.standard_normal((4 * n, D)).astype(f32)
    b[n:2 * n] = q[n:2 * n]                                    # q = b: everything cancels
    b[2 * n:3 * n] = -q[2 * n:3 * n]                           # q = -b: nothing does
    q[3 * n:] *= (10.0 ** rng.uniform(-3, 3, (n, 1))).astype(f32)      # norm ratios up to 1e6, either way
    q[::7, D // 2:] = 0                                        # zero padding, as a dim < D leaves it
    return q, b


@pytest.mark.parametrize("D", (16, 128, 2048))
def test_slack_bounds_both_paths(D):
    q, b = _pairs(D, np.random.default_rng(D))
    qn, bn = _dot8(q, q), _dot8(b, b)
    d_vec = np.maximum((qn + bn) - f32(2) * _dot8(q, b), f32(0))
    # the matrix path twice: every product fused into the sum (one rounding), and rounded before it is added (two) -- the
    # bound budgets the second and so holds for either way the instruction may work
    s = t = -bn / f32(2)
    for i in range(D):
        s = _fma(q[:, i], b[:, i], s)
        t = (q[:, i] * b[:, i]) + t
    d_mat = np.maximum(_fma(np.full_like(s, -2), s, qn), f32(0))
    d_unfused = np.maximum(_fma(np.full_like(t, -2), t, qn), f32(0))
    real = np.maximum(qn.astype(f64) + bn.astype(f64) - 2 * (q.astype(f64) * b.astype(f64)).sum(1), 0)
    eps = np.empty(len(q), f32)
    out = C.c_float()
    for i in range(len(q)):
        _lib.check(_lib.lib().cph_host_exact_matrix_slack(float(qn[i]), float(bn[i]), D, C.byref(out)))
        eps[i] = out.value
    gap = np.abs(d_mat.astype(f64) - d_vec.astype(f64))
    print(D, "largest gap / slack:", float((gap / eps).max()))
    assert (gap <= eps).all() and (np.abs(d_unfused.astype(f64) - d_vec.astype(f64)) <= eps).all()
    assert (np.abs(d_mat - real) <= eps).all() and (np.abs(d_vec - real) <= eps).all()
    # and it is no blank cheque: the (4.125 D + 24) u (qn + bn) of the derivation, its outward rounding and no more
    assert (eps <= (4.125 * D + 24) * 2.0 ** -24 * 1.001 * (qn + bn).astype(f64) + 1e-30).all()


def test_slack_of_what_is_not_finite():
    out = C.c_float()
    for qn, bn in ((np.inf, 1.0), (1.0, np.nan), (3e38, 3e38)):
        _lib.check(_lib.lib().cph_host_exact_matrix_slack(qn, bn, 128, C.byref(out)))
        assert not np.isfinite(out.value)
