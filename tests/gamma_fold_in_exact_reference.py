"""The recursion `pmf_gamma_fold_in_exact` is defined by (include/pmf_hip.h) in NumPy, built on
`gamma_elbo_reference.expectations` and scipy's digamma / logsumexp: vectorised per row, ratings in the given order, the
opposite side frozen as q = Gamma(a_other, b_other).  float64 is the reference.  `dtype=np.float32` is what a float32
context may be expected to reach: s, r, l, the (E log, E) table, the weights and every sum are rounded to float32, psi
and log of the row's own s and r are evaluated in double.

A pass states its sums the way `factor_half_sweep(exact=True)` of tests/gamma_elbo_reference.py does -- the weights are
exp(s - logsumexp(s)), the shape sum grows from the prior and the rate sum from rho, one rating after the other in input
order -- so one pass from a state's own (a, b, rho) on its own ratings IS that half-sweep followed by
`hyper_half_sweep`, bit for bit.  The rate sum is therefore re-added from rho in every pass: the header's
r = rho + B with B formed once, up to the order of the additions.

Also the share a single row has of `elbo_poisson` / `elbo_hpf`, with the distance an evaluation of it may have from
the exact value."""
import numpy as np
from scipy.special import digamma, gammaln, logsumexp

import gamma_elbo_reference as ref

DOUBLE_TOL = 1e-11          # tests/test_gamma_exact_gpu.py: relative bound of the bound's double terms


FROZEN = 29                 # rows of the frozen side in the tests' batch
KAPPA_PRIORS = (0.3, 0.4, 1.5)   # (s, s', r') of the hierarchical calls: hyper_shape = s' + K s, hyper_rate_prior = r'
FLAT_PRIORS = (0.3, 0.7)         # (a0, b0) of the others


def call_prior(K, hierarchical):
    """(shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior) as the C call takes them"""
    s, s1, r1 = KAPPA_PRIORS
    return (s, 0.0, True, s1 + K * s, r1) if hierarchical else (FLAT_PRIORS[0], FLAT_PRIORS[1], False, 0.0, 0.0)


def exact_batch(seed):
    """The batch of tests/gamma_fold_in_reference.py (rows of 0 .. 700 ratings from {0 .. 5}) plus a row of 769 and one of
    1500 ratings -- the block variant under the default threshold -- against FROZEN rows."""
    from gamma_fold_in_reference import LENGTHS, batch
    return batch(seed, FROZEN, LENGTHS + (769, 1500))


def frozen_state(K, small, row_ptr, other_ids):
    """The two frozen states of tests/test_gamma_exact_gpu.py:_draw_state (`small`: shapes down to 0.01, and the most
    gathered frozen row all 0.01 over 1e3, E log = -107.5) for FROZEN rows on both sides, and warm-start values for the
    rows of the batch drawn the same way (`small`: the longest row starts all 0.01 over 1e3 as well): a dict with
    a_theta, b_theta, a_beta, b_beta (either pair serves as the opposite side) and init_a, init_b, init_h [n_rows]."""
    from test_gamma_exact_gpu import _draw_state
    ids = np.asarray(other_ids, dtype=np.int64)
    st = _draw_state(K, FROZEN, FROZEN, K, small, ids, ids)
    n_rows = len(row_ptr) - 1
    rows = np.repeat(np.arange(n_rows), np.diff(row_ptr))
    own = _draw_state(1000 + K, n_rows, 1, K, small, rows, np.zeros(len(rows), dtype=np.int64))
    st["init_a"], st["init_b"], st["init_h"] = own["a_theta"], own["b_theta"], own["h_xi"]
    return st


def _running(start, addends, f):
    """start + addends[0] + addends[1] + ..., one after the other in dtype f ([n, K] -> [K]): a reduction over the
    outer axis of a C-ordered array adds row after row (tests/test_gamma_fold_in_exact_cpu.py holds it to np.add.at's bits)"""
    return np.add.reduce(np.ascontiguousarray(np.vstack([np.asarray(start, dtype=f)[None, :], addends.astype(f, copy=False)])), axis=0, dtype=f)


def fold_in_exact_reference(a_other, b_other, row_ptr, other_ids, ratings, shape_prior, rate_prior=0.0, hierarchical=False,
                            hyper_shape=0.0, hyper_rate_prior=0.0, n_iter=10, init_shape=None, init_rate=None, init_prior_rate=None,
                            dtype=np.float64, colsum=None, trace=None):
    """(factor, shape, rate, prior_rate, hyper_rate); the last two are None unless `hierarchical`.  `colsum` [K]: the
    zero mode's B of every row.  `trace`: a list that receives (shape, rate, hyper_rate) copies after every pass."""
    f = dtype
    E_o, L_o = ref.expectations(np.asarray(a_other, dtype=np.float64), np.asarray(b_other, dtype=np.float64))
    E_o, L_o = E_o.astype(f), L_o.astype(f)                                    # the table, rounded once
    K, n_rows = E_o.shape[1], len(row_ptr) - 1
    a, b0, a_h, b_h = f(shape_prior), f(rate_prior), f(hyper_shape), f(hyper_rate_prior)
    assert (init_shape is None) == (init_rate is None)
    shape, rate = (np.zeros((n_rows, K), dtype=f) for _ in range(2))
    prior_rate, hyper_rate = (np.zeros(n_rows, dtype=f) for _ in range(2))
    per_pass = [[np.zeros((n_rows, K), dtype=f), np.zeros((n_rows, K), dtype=f), np.zeros(n_rows, dtype=f)] for _ in range(n_iter)]
    for r in range(n_rows):
        sel = slice(row_ptr[r], row_ptr[r + 1])
        ids = np.asarray(other_ids[sel], dtype=np.int64)
        Lj, Ej = L_o[ids], E_o[ids]                                            # (n, K); n may be 0
        x = np.asarray(ratings[sel], dtype=f)
        if hierarchical:
            rho = f(init_prior_rate[r]) if init_prior_rate is not None else a_h / b_h
        else:
            rho = b0
        s = np.asarray(init_shape[r], dtype=f) if init_shape is not None else np.full(K, a, dtype=f)
        rt = np.asarray(init_rate[r], dtype=f) if init_rate is not None else np.full(K, rho, dtype=f)
        h = f(0)
        for t in range(n_iter):
            ell = ref.expectations(s.astype(np.float64), rt.astype(np.float64))[1].astype(f)     # psi and log in double
            sj = ell[None, :] + Lj
            w = np.exp(sj - logsumexp(sj, axis=1)[:, None]) if len(x) else sj
            assert w.dtype == f
            s = _running(np.full(K, a, dtype=f), x[:, None] * w, f)
            rt = rho + np.asarray(colsum, dtype=f) if colsum is not None else _running(np.full(K, rho, dtype=f), Ej, f)
            if hierarchical:
                h = b_h + (s / rt)[None, :].sum(axis=1, dtype=f)[0]
                rho = a_h / h
            per_pass[t][0][r], per_pass[t][1][r], per_pass[t][2][r] = s, rt, h
        shape[r], rate[r], prior_rate[r], hyper_rate[r] = s, rt, rho, h
    if trace is not None:
        trace.extend(tuple(p) for p in per_pass)
    if not hierarchical:
        return shape / rate, shape, rate, None, None
    return shape / rate, shape, rate, prior_rate, hyper_rate


def reverse_rows(row_ptr, other_ids, ratings):
    """The same batch with the ratings of every row in reverse order: another summation order of the same sums."""
    ids, x = np.array(other_ids), np.array(ratings)
    for r in range(len(row_ptr) - 1):
        sel = slice(row_ptr[r], row_ptr[r + 1])
        ids[sel], x[sel] = ids[sel][::-1], x[sel][::-1]
    return ids, x


def row_bound(a_other, b_other, row_ptr, other_ids, ratings, shape, rate, hyper_rate, prior, hierarchical, eps=2.0 ** -53):
    """(L [n_rows], allowed [n_rows]): row r's share of `elbo_poisson` (prior = (a0, b0)) or `elbo_hpf` (prior =
    (s, s', r'), `hyper_rate` = h of the rows) at q(row) = Gamma(shape, rate), the opposite side at Gamma(a_other,
    b_other) -- the data term of the row's ratings, the row's prior terms, its entropy terms and, for HPF, its xi terms --
    and the distance an evaluation may have from it, as tests/test_gamma_exact_gpu.py:_elbo_allowed defines it: the sum
    over the terms of |coefficient| x (1e-11 magnitude for the row terms, eps (n_r + K + 16) magnitude for DATA)."""
    shape, rate = np.asarray(shape, dtype=np.float64), np.asarray(rate, dtype=np.float64)
    a_other, b_other = np.asarray(a_other, dtype=np.float64), np.asarray(b_other, dtype=np.float64)
    n_rows, K = shape.shape
    rows = np.repeat(np.arange(n_rows), np.diff(row_ptr))
    x = np.asarray(ratings, dtype=np.float64)
    data, logfact, mag_data, mag_lf, count = ref.data_by_rows(shape, rate, a_other, b_other, rows, np.asarray(other_ids, dtype=np.int64), x)
    E, L = ref.expectations(shape, rate)
    entropy = (shape - np.log(rate) + gammaln(shape) + (1.0 - shape) * digamma(shape)).sum(axis=1)
    _, mags = ref.row_terms(shape, rate, np.asarray(hyper_rate, dtype=np.float64) if hierarchical else None)
    coef = np.zeros(ref.TERMS)
    coef[[ref.ENTROPY, ref.LOGFACT]] = 1.0
    if hierarchical:
        s, s1, r1 = prior
        h = np.asarray(hyper_rate, dtype=np.float64)
        kappa = s1 + K * s
        E_h, L_h = kappa / h, digamma(kappa) - np.log(h)
        value = (data - logfact
                 + np.sum(s * L_h[:, None] - gammaln(s) + (s - 1.0) * L - E_h[:, None] * E, axis=1)          # E log p(theta | xi)
                 + (s1 * np.log(r1) - gammaln(s1) + (s1 - 1.0) * L_h - r1 * E_h)                             # E log p(xi)
                 + entropy
                 + (kappa - np.log(h) + gammaln(kappa) + (1.0 - kappa) * digamma(kappa)))                    # entropy of q(xi)
        coef[ref.SUM_ELOG], coef[ref.FACTOR_OVER_HYPER], coef[ref.INV_HYPER] = abs(s - 1.0), kappa, r1 * kappa
        coef[ref.LOG_HYPER] = abs(K * s + (s1 - 1.0) + 1.0)
    else:
        a0, b0 = prior
        value = data - logfact + np.sum(a0 * np.log(b0) - gammaln(a0) + (a0 - 1.0) * L - b0 * E, axis=1) + entropy
        coef[ref.SUM_ELOG], coef[ref.SUM_FACTOR] = abs(a0 - 1.0), b0
    mags[:, ref.LOGFACT] = mag_lf
    allowed = DOUBLE_TOL * (mags @ coef) + eps * (count + K + 16) * mag_data
    return value, allowed
