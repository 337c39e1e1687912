"""Dense float64 NumPy restatement of the Poisson MF / HPF calls with every unlisted (user, item) cell counted as a
rating of 0 (PMF_ZEROS_OBSERVED, include/pmf_hip.h), written from the formulae there with tests/gamma_elbo_reference.py
as building blocks.  It shares no code with the kernels or with src/models.

A zero adds nothing to a shape sum and its row of the other side's expected factors to the rate sum, for every row
alike: the rate sum of every row is C_k = sum over ALL rows o of the other side of E_other[o, k], and the bound's
-E theta . E beta term over all cells is -(sum_u E theta_u) . (sum_i E beta_i).  States are the dicts of
gamma_elbo_reference; `u, i, x` list each cell at most once."""
import numpy as np
from scipy.special import gammaln, logsumexp

import gamma_elbo_reference as ref

RATE_FLOOR = 1e-10


def problem_p(seed=5, U=90, I=70, N=4000):
    """The sparse problem P the tests share: `skewed_problem(seed, U, I, N)` with duplicate pairs dropped (first
    occurrence kept, input order otherwise) and every eleventh rating set to 0."""
    from helpers import skewed_problem
    u, i, x = skewed_problem(seed, U, I, N)
    _, first = np.unique(u.astype(np.int64) * I + i, return_index=True)
    keep = np.sort(first)
    u, i, x = u[keep], i[keep], x[keep].astype(np.float64).copy()
    x[::11] = 0.0
    return u, i, x


def dense_completion(u, i, x, U, I):
    """D: the same ratings, then an explicit 0 for every cell of the U x I matrix that is not listed (row-major)."""
    listed = np.zeros((U, I), dtype=bool)
    listed[u, i] = True
    mu, mi = np.nonzero(~listed)
    return (np.concatenate([u, mu]).astype(u.dtype), np.concatenate([i, mi]).astype(i.dtype),
            np.concatenate([x, np.zeros(len(mu))]))


def column_sums(st, side):
    """C [K] of `side`: the sum of E = a / b over all its rows"""
    name = "theta" if side == 0 else "beta"
    return (st["a_" + name] / st["b_" + name]).sum(axis=0)


def factor_half_sweep(st, side, u, i, x, shape_prior, rate_prior, exact):
    """New (a, b) of every row of `side`: the shape sums of gamma_elbo_reference.factor_half_sweep over the listed
    ratings (a zero adds nothing), the rate `rate_prior_r + C` with C of the other side.  A row without ratings gets
    (shape_prior, rate_prior_r + C)."""
    a, _ = ref.factor_half_sweep(st, side, u, i, x, shape_prior, 0.0, exact)
    b = np.zeros_like(a) + np.reshape(rate_prior, (-1, 1)) + column_sums(st, 1 - side)[None, :]
    return a, b


def half_steps(st, u, i, x, priors, hierarchical, exact):
    """gamma_elbo_reference.half_steps with the zero-mode factor half-sweep."""
    st = dict(st)
    K = st["a_theta"].shape[1]
    for side, name, hyper in ((0, "theta", "h_xi"), (1, "beta", "h_eta")):
        prior = priors[side]
        rate = (prior[1] + K * prior[0]) / st[hyper] if hierarchical else prior[1]
        st["a_" + name], st["b_" + name] = factor_half_sweep(st, side, u, i, x, prior[0], rate, exact)
        yield dict(st)
        if hierarchical:
            st[hyper] = ref.hyper_half_sweep(st, side, prior[2])
            yield dict(st)


def data_by_rows(st, side, u, i, x):
    """Per row of `side`: (DATA [R], LOGFACT [R], magnitude of the x lse part [R], E_r . C [R], ratings per row [R]).
    DATA_r = sum_j x_j lse_j - E_r . C; the magnitude is sum_j x_j (max_k |Elog_rk| + max_k |Elog_ok| + |lse_j|)."""
    names = ("theta", "beta") if side == 0 else ("beta", "theta")
    rows, others = (u, i) if side == 0 else (i, u)
    Es, Ls = ref.expectations(st["a_" + names[0]], st["b_" + names[0]])
    _, Lo = ref.expectations(st["a_" + names[1]], st["b_" + names[1]])
    R = len(Es)
    lse = logsumexp(Ls[rows] + Lo[others], axis=1)
    xl = np.bincount(rows, weights=x * lse, minlength=R)
    mag = np.bincount(rows, weights=x * (np.abs(Ls).max(axis=1)[rows] + np.abs(Lo).max(axis=1)[others] + np.abs(lse)), minlength=R)
    logfact = np.bincount(rows, weights=gammaln(x + 1.0), minlength=R)
    dot = Es @ column_sums(st, 1 - side)
    return xl - dot, logfact, mag, dot, np.bincount(rows, minlength=R).astype(np.float64)


def data_block(st, u, i, x):
    """E_q log p(x | theta, beta) over ALL cells, the auxiliary multinomials at their optimum."""
    Et, Lt = ref.expectations(st["a_theta"], st["b_theta"])
    Eb, Lb = ref.expectations(st["a_beta"], st["b_beta"])
    lse = logsumexp(Lt[u] + Lb[i], axis=1)
    return float(np.sum(x * lse) - Et.sum(axis=0) @ Eb.sum(axis=0) - np.sum(gammaln(x + 1.0)))


def _listed_data_block(st, u, i, x):
    return ref.data_block(st, u, i, x)


def elbo_poisson(st, u, i, x, a0, b0):
    """gamma_elbo_reference.elbo_poisson with the data block over all cells"""
    return ref.elbo_poisson(st, u, i, x, a0, b0) - _listed_data_block(st, u, i, x) + data_block(st, u, i, x)


def elbo_hpf(st, u, i, x, user_prior, item_prior):
    return ref.elbo_hpf(st, u, i, x, user_prior, item_prior) - _listed_data_block(st, u, i, x) + data_block(st, u, i, x)


def fold_in(E_other, row_ptr, other_ids, ratings, shape_prior, rate_prior=0.0, hierarchical=False, hyper_shape=0.0,
            hyper_rate_prior=0.0, n_iter=10, init_factor=None, init_prior_rate=None):
    """The recursion of pmf_gamma_fold_in (gamma_fold_in_reference.fold_in_reference, float64) with B = the column sum of
    `E_other` for every row: (factor, shape, rate, prior_rate, hyper_rate); the last two None unless `hierarchical`."""
    E_other = np.asarray(E_other, dtype=np.float64)
    K, n_rows = E_other.shape[1], len(row_ptr) - 1
    B = E_other.sum(axis=0)
    factor, shape, rate = (np.zeros((n_rows, K)) for _ in range(3))
    prior_rate, hyper_rate = np.zeros(n_rows), np.zeros(n_rows)
    for r in range(n_rows):
        sel = slice(row_ptr[r], row_ptr[r + 1])
        beta = E_other[np.asarray(other_ids[sel], dtype=np.int64)]
        x = np.asarray(ratings[sel], dtype=np.float64)
        if hierarchical:
            rho = float(init_prior_rate[r]) if init_prior_rate is not None else hyper_shape / hyper_rate_prior
        else:
            rho = rate_prior
        theta = np.asarray(init_factor[r], dtype=np.float64) if init_factor is not None else np.full(K, shape_prior / rho)
        s = rt = theta
        h = 0.0
        for _ in range(n_iter):
            lam = np.maximum(beta @ theta, RATE_FLOOR)
            s = shape_prior + np.sum((x[:, None] / lam[:, None]) * beta * theta[None, :], axis=0)
            rt = rho + B
            theta = s / rt
            if hierarchical:
                h = hyper_rate_prior + np.sum(theta)
                rho = hyper_shape / h
        factor[r], shape[r], rate[r], prior_rate[r], hyper_rate[r] = theta, s, rt, rho, h
    if not hierarchical:
        return factor, shape, rate, None, None
    return factor, shape, rate, prior_rate, hyper_rate
