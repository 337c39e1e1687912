"""Posterior predictive of the Poisson MF and HPF classes (extension: the reference's `predict` returns the mean and its
PoissonLogPredictiveLikelihood plugs the factor means in, on the host).  Mean, variance and the three log densities of
a count are formed on the device from the fitted shapes and rates (`pmf_gamma_predictive`, include/pmf_hip.h has the
definitions); this module holds what `predict_variance`, `log_predictive_density` and `fit(track_loglik=)` of the two
classes share."""
import numpy as np

from pmf_hip import GAMMA_PRED_BOUND, GAMMA_PRED_NEGBIN, GAMMA_PRED_PLUGIN

KINDS = {"plugin": GAMMA_PRED_PLUGIN, "bound": GAMMA_PRED_BOUND, "negbin": GAMMA_PRED_NEGBIN}


def check_kind(kind, what="kind"):
    if kind not in KINDS:
        raise ValueError(f"{what} must be one of {sorted(KINDS)}, not {kind!r}")
    return kind


def check_ratings(ratings, what):
    """The Poisson densities are not defined for a negative count."""
    if len(ratings) and float(np.min(ratings)) < 0:
        raise ValueError(f"{what}: a rating is negative; the Poisson likelihood is not defined for it")


def check_tracking(model, track_loglik, loglik_tol, loglik_kind, val_df):
    """`fit`'s three log-likelihood arguments -> whether the fit tracks the validation log-likelihood; refuses what is not
    covered, before any device call.  The frame is looked at only when the fit tracks: a default fit does what it did."""
    track = bool(track_loglik) or loglik_tol is not None
    if track:
        check_kind(loglik_kind, "loglik_kind")
        if val_df is None:
            raise ValueError("track_loglik needs val_df: the log-likelihood is that of the validation ratings")
        if model._comm is not None:
            raise NotImplementedError("track_loglik under a communicator: the predictive of a sharded fit is not implemented")
        check_ratings(val_df["rating"].to_numpy(dtype=float), "track_loglik")
    return track


def _fitted_ctx(model, what):
    """The context whose SHAPE and RATE define q, or the reason there is none."""
    ctx = model._need_ctx()
    if model._shard_ctx is not None or model._comm is not None:
        raise NotImplementedError(f"{what} after a sharded fit: the full-size context holds FACTOR only, the predictive of a "
                                  "sharded fit is not implemented")
    if model.history_["iterations"] == 0:
        raise RuntimeError(f"{type(model).__name__} has run no iteration: SHAPE and RATE were never written, q is not defined")
    return ctx


def _seen(model, u, i):
    return (u >= 0) & (u < model.n_users) & (i >= 0) & (i < model.n_items)


def predict_variance(model, user_ids, item_ids, include_noise=True):
    """`predict_variance` of the two classes."""
    ctx = _fitted_ctx(model, "predict_variance")
    u, i = np.asarray(user_ids, dtype=int).reshape(-1), np.asarray(item_ids, dtype=int).reshape(-1)
    if len(u) != len(i):
        raise ValueError("user_ids and item_ids must have the same length")
    seen = _seen(model, u, i)
    out = np.zeros(len(u), dtype=np.float64)
    if seen.any():      # the call never sees an id the fit has not: it would refuse it
        res = ctx.gamma_predictive(u[seen], i[seen], with_bound=False)
        out[seen] = res.var + res.mean if include_noise else res.var
    return out


def validation_pairs(model, df, what):
    """(u, i, rating) of the frame's rows with seen ids; a negative rating among them is refused."""
    u, i = df["u"].to_numpy(dtype=int), df["i"].to_numpy(dtype=int)
    x = df["rating"].to_numpy(dtype=float)
    check_ratings(x, what)
    seen = _seen(model, u, i)
    return u[seen], i[seen], x[seen]


def total_log_density(ctx, u, i, x, kind):
    """The TOTAL of one log density over the pairs, on the device; nan with the reference's warning when there is none."""
    if len(u) == 0:
        print("Warning: No valid (u,i) pairs.")
        return float("nan")
    res = ctx.gamma_predictive(u, i, x, with_bound=kind == "bound", per_pair=False)
    return float(res.totals[1 + KINDS[kind]])


def log_predictive_density(model, df, kind="negbin", per_row=False):
    """`log_predictive_density` of the two classes."""
    check_kind(kind)
    check_ratings(df["rating"].to_numpy(dtype=float), "log_predictive_density")
    ctx = _fitted_ctx(model, "log_predictive_density")
    u, i, x = validation_pairs(model, df, "log_predictive_density")
    if not per_row:
        return total_log_density(ctx, u, i, x, kind)
    if len(u) == 0:
        print("Warning: No valid (u,i) pairs.")
        return float("nan"), np.zeros(0)
    res = ctx.gamma_predictive(u, i, x, with_bound=kind == "bound")
    return float(res.totals[1 + KINDS[kind]]), res.logp[:, KINDS[kind]].copy()


def monitor_setup(model, ctx, val_df, kind):
    """The validation pairs of a tracking fit, filtered once; returns the callable that gives the total for the state the
    context holds then."""
    u, i, x = validation_pairs(model, val_df, "track_loglik")
    return lambda: total_log_density(ctx, u, i, x, kind)


def record_loglik(model, monitor, it, loglik_tol):
    """After iteration `it` of a tracking fit: append the validation total to `history_["val_loglik"]`, print it when
    verbose, and say whether `loglik_tol` stops the fit (the HPF paper's rule: relative change of the held-out
    log-likelihood; it fires on a decrease too)."""
    trace = model.history_["val_loglik"]
    trace.append(monitor())
    if model.config.verbose:
        print(f"Validation log-likelihood: {trace[-1]:.4f}")
    if loglik_tol is None or it < 2:
        return False
    before, now = trace[-2:]
    return (now - before) / abs(before) < loglik_tol
