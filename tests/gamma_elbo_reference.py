"""Dense float64 NumPy / scipy restatement of the Poisson MF / HPF evidence lower bound: what `pmf_gamma_elbo_terms` and
`elbo_from_gamma_terms` are tested against.  It shares no code with the kernels or with src/models/_gamma_elbo.py.

q(theta_uk) = Gamma(a, b) (shape, rate), q(beta_ik) alike and, for HPF, q(xi_u) = Gamma(kappa, h_u) with
kappa = a' + K a (items: q(eta_i) = Gamma(c' + K c, h_i)).  A state is a dict with a_theta, b_theta, a_beta, b_beta and,
for HPF, h_xi, h_eta.  The auxiliary multinomial of a rating sits at its optimum phi_k ~ exp(Elog theta_uk + Elog beta_ik)
unless a phi is passed."""
import numpy as np
from scipy.special import digamma, gammaln, logsumexp

SUM_FACTOR, SUM_ELOG, ENTROPY, LOG_HYPER, INV_HYPER, FACTOR_OVER_HYPER, DATA, LOGFACT, TERMS = range(9)   # include/pmf_hip.h


def expectations(a, b):
    """E and E log of Gamma(a, b)"""
    return a / b, digamma(a) - np.log(b)


# ---- per-row terms and their magnitudes ------------------------------------------------------------------------------
def row_terms(a, b, h=None):
    """(terms, mags), both [rows, TERMS] with the DATA and LOGFACT columns zero: the per-row sums of one side and, for
    each, the sum of the absolute values of every product that enters it."""
    R = len(a)
    psi, lb, lg = digamma(a), np.log(b), gammaln(a)
    terms, mags = np.zeros((R, TERMS)), np.zeros((R, TERMS))
    terms[:, SUM_FACTOR] = mags[:, SUM_FACTOR] = (a / b).sum(axis=1)
    terms[:, SUM_ELOG] = (psi - lb).sum(axis=1)
    mags[:, SUM_ELOG] = (np.abs(psi) + np.abs(lb)).sum(axis=1)
    terms[:, ENTROPY] = (a - lb + lg + (1.0 - a) * psi).sum(axis=1)
    mags[:, ENTROPY] = (a + np.abs(lb) + np.abs(lg) + np.abs((1.0 - a) * psi)).sum(axis=1)
    if h is not None:
        terms[:, LOG_HYPER] = np.log(h)
        mags[:, LOG_HYPER] = np.abs(np.log(h))
        terms[:, INV_HYPER] = mags[:, INV_HYPER] = 1.0 / h
        terms[:, FACTOR_OVER_HYPER] = mags[:, FACTOR_OVER_HYPER] = (a / b).sum(axis=1) / h
    return terms, mags


# ---- the data term, three ways ---------------------------------------------------------------------------------------
def data_per_rating(st, u, i, x):
    """[N]: x lse - E theta . E beta of every rating, vectorised over the ratings (max-subtracted by hand)."""
    Et, Lt = expectations(st["a_theta"], st["b_theta"])
    Eb, Lb = expectations(st["a_beta"], st["b_beta"])
    s = Lt[u] + Lb[i]
    m = s.max(axis=1)
    lse = m + np.log(np.exp(s - m[:, None]).sum(axis=1))
    return x * lse - np.einsum("nk,nk->n", Et[u], Eb[i])


def data_by_rows(a_self, b_self, a_other, b_other, rows, others, x):
    """Row by row of one side (ratings of a row in input order): (data [R], logfact [R], data magnitude [R], logfact
    magnitude [R], ratings per row [R]).  The data magnitude of a row is
    sum_j [ x_j (max_k |Elog_rk| + max_k |Elog_ok| + |lse_j|) + sum_k E_rk E_ok ]."""
    R = len(a_self)
    Es, Ls = expectations(a_self, b_self)
    Eo, Lo = expectations(a_other, b_other)
    data, logfact, mag, mag_lf, count = (np.zeros(R) for _ in range(5))
    order = np.argsort(rows, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=R))])
    for r in range(R):
        at = order[ptr[r]:ptr[r + 1]]
        if len(at) == 0:
            continue
        o, xr = others[at], x[at]
        lse = logsumexp(Ls[r][None, :] + Lo[o], axis=1)
        dots = Eo[o] @ Es[r]
        data[r] = np.sum(xr * lse - dots)
        logfact[r] = np.sum(gammaln(xr + 1.0))
        mag[r] = np.sum(xr * (np.abs(Ls[r]).max() + np.abs(Lo[o]).max(axis=1) + np.abs(lse)) + dots)
        mag_lf[r] = np.sum(np.abs(gammaln(xr + 1.0)))
        count[r] = len(at)
    return data, logfact, mag, mag_lf, count


def side_terms(st, side, u, i, x, hierarchical, with_data=True):
    """What pmf_gamma_elbo_terms(side, with_data, hierarchical) returns per row, and the magnitudes: (terms, mags,
    ratings per row)."""
    names = ("theta", "beta") if side == 0 else ("beta", "theta")
    a_s, b_s, a_o, b_o = st["a_" + names[0]], st["b_" + names[0]], st["a_" + names[1]], st["b_" + names[1]]
    h = st["h_xi" if side == 0 else "h_eta"] if hierarchical else None
    terms, mags = row_terms(a_s, b_s, h)
    count = np.zeros(len(a_s))
    if with_data:
        rows, others = (u, i) if side == 0 else (i, u)
        terms[:, DATA], terms[:, LOGFACT], mags[:, DATA], mags[:, LOGFACT], count = data_by_rows(a_s, b_s, a_o, b_o, rows, others, x)
    return terms, mags, count


# ---- the whole bound, block by block ---------------------------------------------------------------------------------
def _gamma_entropy(a, b):
    return np.sum(a - np.log(b) + gammaln(a) + (1.0 - a) * digamma(a))


def data_block(st, u, i, x, phi=None):
    """E_q log p(x | theta, beta) with the auxiliary multinomials at their optimum, or at `phi` [N, K]."""
    Et, Lt = expectations(st["a_theta"], st["b_theta"])
    Eb, Lb = expectations(st["a_beta"], st["b_beta"])
    s = Lt[u] + Lb[i]
    if phi is None:
        bound = logsumexp(s, axis=1)
    else:
        bound = np.sum(phi * (s - np.log(phi)), axis=1)
    return float(np.sum(x * bound) - np.sum(Et[u] * Eb[i]) - np.sum(gammaln(x + 1.0)))


def elbo_poisson(st, u, i, x, a0, b0, phi=None):
    total = data_block(st, u, i, x, phi)
    for name in ("theta", "beta"):
        a, b = st["a_" + name], st["b_" + name]
        E, L = expectations(a, b)
        total += np.sum(a0 * np.log(b0) - gammaln(a0) + (a0 - 1.0) * L - b0 * E)     # E log p(theta)
        total += _gamma_entropy(a, b)
    return float(total)


def elbo_hpf(st, u, i, x, user_prior, item_prior, phi=None):
    """`user_prior` = (a, a', b'), `item_prior` = (c, c', d')"""
    total = data_block(st, u, i, x, phi)
    for name, hyper, (s, s1, r1) in (("theta", "h_xi", user_prior), ("beta", "h_eta", item_prior)):
        a, b, h = st["a_" + name], st["b_" + name], st[hyper]
        K = a.shape[1]
        kappa = s1 + K * s
        E, L = expectations(a, b)
        E_h, L_h = kappa / h, digamma(kappa) - np.log(h)
        total += np.sum(s * L_h[:, None] - gammaln(s) + (s - 1.0) * L - E_h[:, None] * E)        # E log p(theta | xi)
        total += np.sum(s1 * np.log(r1) - gammaln(s1) + (s1 - 1.0) * L_h - r1 * E_h)             # E log p(xi)
        total += _gamma_entropy(a, b)
        total += _gamma_entropy(np.full(len(h), kappa), h)
    return float(total)


# ---- half-sweeps -----------------------------------------------------------------------------------------------------
def factor_half_sweep(st, side, u, i, x, shape_prior, rate_prior, exact):
    """New (a, b) of every row of `side` with the other side fixed.  `rate_prior`: a scalar (Poisson MF) or the per-row
    E xi / E eta (HPF).  `exact`: the weights of a rating are exp(Elog + Elog) normalised (coordinate ascent on the
    bound); else E E normalised (the reference's update: poisson_mf_cavi.py:135-167, hpf_cavi.py:126-153)."""
    names = ("theta", "beta") if side == 0 else ("beta", "theta")
    rows, others = (u, i) if side == 0 else (i, u)
    Es, Ls = expectations(st["a_" + names[0]], st["b_" + names[0]])
    Eo, Lo = expectations(st["a_" + names[1]], st["b_" + names[1]])
    if exact:
        s = Ls[rows] + Lo[others]
        w = np.exp(s - logsumexp(s, axis=1)[:, None])
    else:
        w = Es[rows] * Eo[others]
        w /= w.sum(axis=1)[:, None]
    a = np.full_like(Es, float(shape_prior))
    b = np.zeros_like(Es) + np.reshape(rate_prior, (-1, 1))
    np.add.at(a, rows, x[:, None] * w)
    np.add.at(b, rows, Eo[others])
    return a, b


def hyper_half_sweep(st, side, hyper_rate_prior):
    """h of every row of `side` (hpf_cavi.py:155-159 / :189-193): b' + sum_k E theta_uk"""
    name = "theta" if side == 0 else "beta"
    return hyper_rate_prior + (st["a_" + name] / st["b_" + name]).sum(axis=1)


def half_steps(st, u, i, x, priors, hierarchical, exact):
    """Generator over the states after every half-step of one iteration: theta, (xi,) beta, (eta).  Poisson MF:
    `priors` = ((a0, b0), (a0, b0)); HPF: ((a, a', b'), (c, c', d'))."""
    st = dict(st)
    K = st["a_theta"].shape[1]
    for side, name, hyper in ((0, "theta", "h_xi"), (1, "beta", "h_eta")):
        prior = priors[side]
        rate = (prior[1] + K * prior[0]) / st[hyper] if hierarchical else prior[1]
        st["a_" + name], st["b_" + name] = factor_half_sweep(st, side, u, i, x, prior[0], rate, exact)
        yield dict(st)
        if hierarchical:
            st[hyper] = hyper_half_sweep(st, side, prior[2])
            yield dict(st)


def initial_state(seed, U, I, K, priors, hierarchical):
    """Priors plus gamma noise, as the model classes draw it."""
    rng = np.random.default_rng(seed)
    st = {"a_theta": priors[0][0] + rng.gamma(1.0, 0.1, size=(U, K)), "b_theta": 1.0 + rng.gamma(1.0, 0.1, size=(U, K)),
          "a_beta": priors[1][0] + rng.gamma(1.0, 0.1, size=(I, K)), "b_beta": 1.0 + rng.gamma(1.0, 0.1, size=(I, K))}
    if hierarchical:
        st["h_xi"] = priors[0][2] + rng.gamma(1.0, 0.1, size=U)
        st["h_eta"] = priors[1][2] + rng.gamma(1.0, 0.1, size=I)
    return st
