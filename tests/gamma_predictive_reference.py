"""Float64 NumPy / scipy / mpmath restatement of the posterior predictive of the Poisson MF and HPF models: what
`pmf_gamma_predictive` and the model classes' `predict_variance` / `log_predictive_density` are tested against.  It
shares no code with the kernels or with src/models/_gamma_predictive.py.

q(theta_uk) = Gamma(a, b) (shape, rate), q(beta_ik) = Gamma(c, d), independent.  For pair (u, i) with rating x:

    E_k    = (a_k / b_k)(c_k / d_k)
    mean   mu = sum_k E_k
    var    v  = sum_k E_k^2 (1/a_k + 1/c_k + 1/(a_k c_k))
    PLUGIN x log max(mu, 1e-10) - max(mu, 1e-10) - lgamma(x + 1)
    BOUND  x lse_k(psi(a_k) - log b_k + psi(c_k) - log d_k) - mu - lgamma(x + 1)
    NEGBIN lgamma(x + r) - lgamma(r) - lgamma(x + 1) + r log(r / (r + mu)) + x log(mu / (r + mu)),   r = mu^2 / v

NEGBIN is the LITERAL formula evaluated with mpmath at 50 digits (the literal formula in double loses every digit once r
passes 1e8), so it shares nothing with the library's stable rewrite.  Where v == 0 or r is not a finite double it is the
unclamped Poisson term x log mu - mu - lgamma(x + 1), with x log mu = 0 at x = 0."""
import mpmath
import numpy as np
from scipy.special import digamma, gammaln, logsumexp

PLUGIN, BOUND, NEGBIN, KINDS = 0, 1, 2, 3      # include/pmf_hip.h
RATE_FLOOR = 1e-10
mpmath.mp.dps = 50


def moments(a, b, c, d):
    """(mu, v, mag_mu, mag_v) of pairs whose rows are given [n, K]: the sums and the sums of the absolute values of their
    terms (every term is positive for positive shapes and rates, so the magnitudes are the sums themselves)."""
    E = (a / b) * (c / d)
    terms = E * E * (1.0 / a + 1.0 / c + 1.0 / (a * c))
    return E.sum(axis=1), terms.sum(axis=1), np.abs(E).sum(axis=1), np.abs(terms).sum(axis=1)


def elog(a, b):
    return digamma(a) - np.log(b)


def lse(a, b, c, d):
    """(lse, max_k |Elog theta| + max_k |Elog beta|) of pairs whose rows are given [n, K]"""
    lt, lb = elog(a, b), elog(c, d)
    return logsumexp(lt + lb, axis=1), np.abs(lt).max(axis=1) + np.abs(lb).max(axis=1)


def _xlog(x, mu):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 0.0, x * np.log(mu))


def poisson(x, mu):
    """(value, sum of |terms|) of the unclamped Poisson log density, x log mu = 0 at x = 0"""
    xl, lf = _xlog(x, mu), gammaln(x + 1.0)
    return xl - mu - lf, np.abs(xl) + np.abs(mu) + np.abs(lf)


def plugin(x, mu):
    """(value, sum of |terms|) of the Poisson log density at max(mu, 1e-10): metrics.PoissonLogPredictiveLikelihood's term"""
    lam = np.maximum(mu, RATE_FLOOR)
    xl, lf = x * np.log(lam), gammaln(x + 1.0)
    return xl - lam - lf, np.abs(xl) + lam + np.abs(lf)


def bound(x, lse_value, mu):
    xl, lf = x * lse_value, gammaln(x + 1.0)
    return xl - mu - lf, np.abs(xl) + np.abs(mu) + np.abs(lf)


def negbin_one(x, mu, v):
    """The literal negative binomial log density of one pair at 50 digits -> (float, sum of |terms| of the STABLE grouping).
    The magnitude is that of the terms a careful double evaluation works with -- x log mu, lgamma(x + 1),
    (r + x) log1p(mu / r), and D = lgamma(x + r) - lgamma(r) - x log r as (x + r - 1/2) log1p(x / r) and x (r >= 10) or as its
    three terms (r < 10) -- not of the literal terms, which are of size r log r and would make any bound vacuous."""
    x, mu, v = float(x), float(mu), float(v)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = np.float64(mu) * np.float64(mu) / np.float64(v)
    if v == 0.0 or not np.isfinite(r):
        val, mag = poisson(np.float64(x), np.float64(mu))
        return float(val), float(mag)
    X, M, R = mpmath.mpf(x), mpmath.mpf(mu), mpmath.mpf(mu) ** 2 / mpmath.mpf(v)
    lg = mpmath.loggamma
    val = lg(X + R) - lg(R) - lg(X + 1) + R * mpmath.log(R / (R + M)) + X * mpmath.log(M / (R + M))
    mag = abs(X * mpmath.log(M)) + abs(lg(X + 1)) + abs((R + X) * mpmath.log1p(M / R))
    if R >= 10:
        mag += abs((X + R - mpmath.mpf(1) / 2) * mpmath.log1p(X / R)) + abs(X)
    else:
        mag += abs(lg(X + R)) + abs(lg(R)) + abs(X * mpmath.log(R))
    return float(val), float(mag)


def negbin(x, mu, v):
    """(values [n], magnitudes [n])"""
    out = [negbin_one(*t) for t in zip(np.asarray(x, dtype=np.float64), np.asarray(mu, dtype=np.float64), np.asarray(v, dtype=np.float64))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def negbin_literal_double(x, mu, v):
    """The literal formula in plain float64: what a naive implementation computes (used to show that it fails)."""
    r = mu * mu / v
    return gammaln(x + r) - gammaln(r) - gammaln(x + 1.0) + r * np.log(r / (r + mu)) + x * np.log(mu / (r + mu))


def predictive(st, u, i, x=None):
    """Everything for pairs of a state dict (a_theta, b_theta, a_beta, b_beta): dict with mu, v, mag_mu, mag_v and, with
    ratings, logp [n, KINDS], mag [n, KINDS], lse, elog_max."""
    a, b, c, d = st["a_theta"][u], st["b_theta"][u], st["a_beta"][i], st["b_beta"][i]
    mu, v, mag_mu, mag_v = moments(a, b, c, d)
    out = {"mu": mu, "v": v, "mag_mu": mag_mu, "mag_v": mag_v}
    if x is None:
        return out
    x = np.asarray(x, dtype=np.float64)
    ls, lmax = lse(a, b, c, d)
    logp, mag = np.zeros((len(u), KINDS)), np.zeros((len(u), KINDS))
    logp[:, PLUGIN], mag[:, PLUGIN] = plugin(x, mu)
    logp[:, BOUND], mag[:, BOUND] = bound(x, ls, mu)
    logp[:, NEGBIN], mag[:, NEGBIN] = negbin(x, mu, v)
    out.update(logp=logp, mag=mag, lse=ls, elog_max=lmax)
    return out
