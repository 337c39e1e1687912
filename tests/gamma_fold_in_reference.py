"""The recursion `pmf_gamma_fold_in` is defined by (include/pmf_hip.h), literally, in NumPy: per row, ratings in the given
order, the other side's factors frozen.  float64 is the reference; `dtype=np.float32` runs the same statements in single
precision (what a float32 context may be expected to reach).  Also the CSR batch the CPU and the GPU tests share."""
import numpy as np

RATE_FLOOR = 1e-10

# every LPR batch edge up to LPR = 64, the four-in-flight edge, many passes
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 255, 256, 257, 700)

# tests/test_gamma_gpu.py:TOL -- relative, on every element, by the number of updates
TOL = {"f64": {1: 1e-12, 3: 1e-11, 20: 1e-9}, "f32": {1: 2e-5, 3: 5e-5, 20: 5e-4}}


def batch(seed, n_other, lengths=LENGTHS):
    """CSR batch: ids on the opposite side drawn with repeats, ratings from {0 .. 5}."""
    rng = np.random.default_rng(seed)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return row_ptr, rng.integers(0, n_other, row_ptr[-1]).astype(np.int32), rng.integers(0, 6, row_ptr[-1]).astype(np.float64)


def fold_in_reference(E_other, row_ptr, other_ids, ratings, shape_prior, rate_prior=0.0, hierarchical=False, hyper_shape=0.0,
                      hyper_rate_prior=0.0, n_iter=10, init_factor=None, init_prior_rate=None, dtype=np.float64):
    """(factor, shape, rate, prior_rate, hyper_rate); the last two are None unless `hierarchical`."""
    f = dtype
    E_other = np.asarray(E_other, dtype=f)
    K, n_rows = E_other.shape[1], len(row_ptr) - 1
    a, b0, a_h, b_h = f(shape_prior), f(rate_prior), f(hyper_shape), f(hyper_rate_prior)
    factor, shape, rate = (np.zeros((n_rows, K), dtype=f) for _ in range(3))
    prior_rate, hyper_rate = (np.zeros(n_rows, dtype=f) for _ in range(2))
    for r in range(n_rows):
        sel = slice(row_ptr[r], row_ptr[r + 1])
        beta = E_other[np.asarray(other_ids[sel], dtype=np.int64)]          # (n, K); n may be 0
        x = np.asarray(ratings[sel], dtype=f)
        if hierarchical:
            rho = f(init_prior_rate[r]) if init_prior_rate is not None else a_h / b_h
        else:
            rho = b0
        theta = np.asarray(init_factor[r], dtype=f) if init_factor is not None else np.full(K, a / rho, dtype=f)
        B = np.sum(beta, axis=0, dtype=f)
        s = rt = theta
        h = f(0)
        for _ in range(n_iter):
            lam = beta @ theta
            lam[lam < f(RATE_FLOOR)] = f(RATE_FLOOR)
            s = a + np.sum((x[:, None] / lam[:, None]) * beta * theta[None, :], axis=0, dtype=f)
            rt = rho + B
            theta = s / rt
            if hierarchical:
                h = b_h + np.sum(theta, dtype=f)
                rho = a_h / h
        factor[r], shape[r], rate[r], prior_rate[r], hyper_rate[r] = theta, s, rt, rho, h
    if not hierarchical:
        return factor, shape, rate, None, None
    return factor, shape, rate, prior_rate, hyper_rate
