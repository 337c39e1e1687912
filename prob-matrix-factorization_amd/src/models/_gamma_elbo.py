"""Evidence lower bound of the Poisson MF and HPF classes (extension: the reference never evaluates its objective).
The sums over rows and ratings are formed on the device (`pmf_gamma_elbo_terms`, include/pmf_hip.h has the definition);
this module adds the handful of scalar terms that carry the hyperparameters, and holds what `fit(track_elbo=)` and
`elbo()` of the two classes share."""
import numpy as np
from scipy.special import digamma, gammaln

from pmf_hip import (GAMMA_ELBO_DATA, GAMMA_ELBO_ENTROPY, GAMMA_ELBO_FACTOR_OVER_HYPER, GAMMA_ELBO_INV_HYPER, GAMMA_ELBO_LOG_HYPER,
                     GAMMA_ELBO_LOGFACT, GAMMA_ELBO_SUM_ELOG, GAMMA_ELBO_SUM_FACTOR, ITEM, USER)


def elbo_from_gamma_terms(user_terms, item_terms, n_users, n_items, n_factors, user_prior, item_prior, hierarchical=False,
                          data_side=USER):
    """The evidence lower bound of a Poisson MF or HPF model from the sums `pmf_gamma_elbo_terms` returns:
    `user_terms` / `item_terms` are the two sides' total vectors (columns `pmf_hip.GAMMA_ELBO_*`), `data_side` the one
    whose DATA and LOGFACT columns are filled.  Poisson MF: `user_prior` = `item_prior` = (a0, b0).  HPF
    (`hierarchical`): `user_prior` = (a, a', b'), `item_prior` = (c, c', d'); the DEVICE terms must then come from
    hierarchical calls.  Returns (value, parts): `parts` names the data term and, per side, the expected log prior of the
    factors (given xi / eta for HPF), their entropy and -- HPF -- the expected log prior and the entropy of xi / eta."""
    K = int(n_factors)
    terms = {USER: np.asarray(user_terms, dtype=np.float64), ITEM: np.asarray(item_terms, dtype=np.float64)}
    parts = {"data": float(terms[data_side][GAMMA_ELBO_DATA]) - float(terms[data_side][GAMMA_ELBO_LOGFACT])}
    for side, name, hyper, R, prior in ((USER, "theta", "xi", int(n_users), user_prior), (ITEM, "beta", "eta", int(n_items), item_prior)):
        t = terms[side]
        sum_e, sum_elog = float(t[GAMMA_ELBO_SUM_FACTOR]), float(t[GAMMA_ELBO_SUM_ELOG])
        parts["entropy_" + name] = float(t[GAMMA_ELBO_ENTROPY])
        if not hierarchical:
            a0, b0 = (float(v) for v in prior)
            parts["prior_" + name] = R * K * (a0 * np.log(b0) - gammaln(a0)) + (a0 - 1.0) * sum_elog - b0 * sum_e
            continue
        s, s1, r1 = (float(v) for v in prior)
        kappa = s1 + K * s
        log_h, inv_h, e_over_h = float(t[GAMMA_ELBO_LOG_HYPER]), float(t[GAMMA_ELBO_INV_HYPER]), float(t[GAMMA_ELBO_FACTOR_OVER_HYPER])
        sum_elog_hyper = R * digamma(kappa) - log_h           # sum_r E log xi_r
        parts["prior_" + name] = K * s * sum_elog_hyper - R * K * gammaln(s) + (s - 1.0) * sum_elog - kappa * e_over_h
        parts["prior_" + hyper] = R * (s1 * np.log(r1) - gammaln(s1)) + (s1 - 1.0) * sum_elog_hyper - r1 * kappa * inv_h
        parts["entropy_" + hyper] = R * (kappa + gammaln(kappa) + (1.0 - kappa) * digamma(kappa)) - log_h
    parts = {k: float(v) for k, v in parts.items()}
    return float(sum(parts.values())), parts


# ---- what the two model classes share --------------------------------------------------------------------------------
def check_tracking(model, track_elbo, elbo_tol, train_df):
    """`fit`'s two ELBO arguments -> whether the fit tracks the bound; refuses what is not covered, before any device call.
    The frame is looked at only when the fit tracks: a default fit does what it did."""
    track = bool(track_elbo) or elbo_tol is not None
    if track:
        if model._comm is not None:
            raise NotImplementedError("track_elbo under a communicator: the ELBO of a sharded fit is not implemented")
        ratings = train_df["rating"].to_numpy(dtype=float)
        if len(ratings) and float(np.min(ratings)) < 0:
            raise ValueError("track_elbo: a training rating is negative; the Poisson likelihood is not defined for it")
    return track


def check_update(update, train_df):
    """`fit`'s `update` argument -> whether the fit runs the exact coordinate-ascent row update; refuses an unknown mode
    and, for the exact update, a negative rating (its weights multiply the rating: the Poisson likelihood is not defined
    for one), before any device call.  The frame is looked at only under "exact"."""
    if update not in ("reference", "exact"):
        raise ValueError(f"update must be 'reference' or 'exact', not {update!r}")
    if update == "exact":
        ratings = train_df["rating"].to_numpy(dtype=float)
        if len(ratings) and float(np.min(ratings)) < 0:
            raise ValueError("update='exact': a training rating is negative; the Poisson likelihood is not defined for it")
    return update == "exact"


def check_unobserved(model, unobserved, train_df):
    """`fit`'s `unobserved` argument -> whether unlisted cells count as zeros; refuses an unknown value and, for "zero",
    what the mode does not cover, before any device call.  The frame is looked at only under "zero"."""
    if unobserved not in ("missing", "zero"):
        raise ValueError(f"unobserved must be 'missing' or 'zero', not {unobserved!r}")
    if unobserved == "missing":
        return False
    if model._comm is not None:
        raise ValueError("unobserved='zero' with comm=: counting unobserved cells as zeros is not available on several ranks")
    ratings = train_df["rating"].to_numpy(dtype=float)
    if len(ratings) and float(np.min(ratings)) < 0:
        raise ValueError("unobserved='zero': a training rating is negative; the Poisson likelihood is not defined for it")
    if train_df.duplicated(subset=["u", "i"]).any():
        raise ValueError("unobserved='zero': train_df lists a (u, i) pair more than once; a cell has one count")
    return True


def model_elbo(model, ctx):
    """(value, parts) for the state `ctx` holds: the data term from the user side, whose gathers hit the smaller item
    table, and the item side without data."""
    user_prior, item_prior, hierarchical = model._elbo_priors()
    user = ctx.gamma_elbo_terms(USER, with_data=True, hierarchical=hierarchical)
    item = ctx.gamma_elbo_terms(ITEM, with_data=False, hierarchical=hierarchical)
    return elbo_from_gamma_terms(user, item, model.n_users, model.n_items, model.config.n_factors, user_prior, item_prior,
                                 hierarchical)


def record_elbo(model, ctx, it, elbo_tol):
    """After iteration `it` of a tracking fit: append the bound to `history_["elbo"]`, print it when verbose, and say
    whether `elbo_tol` stops the fit."""
    trace = model.history_["elbo"]
    trace.append(model_elbo(model, ctx)[0])
    if model.config.verbose:
        print(f"ELBO: {trace[-1]:.4f}")
    if elbo_tol is None or it < 2:
        return False
    before, now = trace[-2:]
    return (now - before) / abs(before) < elbo_tol


def fitted_elbo(model, parts):
    """`elbo()` of the two classes."""
    ctx = model._need_ctx()
    if model._shard_ctx is not None or model._comm is not None:
        raise NotImplementedError("elbo after a sharded fit: the ELBO of a sharded fit is not implemented")
    if model.history_["iterations"] == 0:
        raise RuntimeError(f"{type(model).__name__} has run no iteration: SHAPE and RATE were never written, q is not defined")
    value, named = model_elbo(model, ctx)
    return (value, named) if parts else value
