"""Logistic matrix factorisation for binary feedback (click / no click, like / dislike) -- MI355X engine.

Extension: the reference has no binary likelihood.  x_ij in {0, 1}, p(x_ij = 1) = sigmoid(theta_i . beta_j), bias-free,
N(0, eta2 I) priors and a mean-field Gaussian q with full covariances: what `GaussianMFCAVI` holds.  Under the
Jaakkola-Jordan bound with one variational parameter xi per rating the likelihood is Gaussian with precision 2 lambda(xi)
and pseudo-target (x - 1/2) / (2 lambda(xi)), so the factor half-sweep is the weighted Gaussian sweep
(`pmf_gauss_factor_sweep` on a context loaded through `pmf_ctx_set_ratings_weighted`) and the xi update is one device
pass over a side's ratings (`pmf_gauss_logit_refresh`).  DESIGN.md section 4.21 has the derivation.

Out of scope: biases, fold-in of new rows, several ranks (`comm=`), unobserved cells as zeros, user-supplied weights."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from src.models._device_model import ITEM, USER, frame_arrays
from src.models._gaussian_host import GaussianHost
from pmf_hip import ARR_FACTOR, ELBO_LOGDET, ELBO_SQNORM

LAMBDA_SERIES_BELOW = 1e-3     # below it lambda(xi) is its series (csrc/pmf_logit.hip has the same switch)


def jj_lambda(xi):
    """lambda(xi) = tanh(xi / 2) / (4 xi) of the Jaakkola-Jordan bound, float64, lambda(0) = 1/8; below
    LAMBDA_SERIES_BELOW the series 1/8 - xi^2/96 + xi^4/960, whose next term is under 1e-22 there."""
    xi = np.abs(np.asarray(xi, dtype=np.float64))
    x2 = xi * xi
    series = 0.125 - x2 * (1.0 / 96.0) + x2 * x2 * (1.0 / 960.0)
    big = np.where(xi < LAMBDA_SERIES_BELOW, 1.0, xi)
    return np.where(xi < LAMBDA_SERIES_BELOW, series, np.tanh(0.5 * big) / (4.0 * big))


def _sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(z, dtype=np.float64)))


def neg_kl(terms, rows, n_factors, eta2):
    """-KL(q || prior) of one side from `pmf_gauss_elbo_terms`' totals: q = N(m_r, V_r) per row, prior N(0, eta2 I)."""
    rk = rows * n_factors
    return 0.5 * float(terms[ELBO_LOGDET]) - float(terms[ELBO_SQNORM]) / (2.0 * eta2) - 0.5 * rk * np.log(eta2) + 0.5 * rk


@dataclass
class LogisticMFCAVIConfig:
    n_factors: int = 10
    eta2: float = 1.0
    max_iter: int = 20
    tol: Optional[float] = 1e-4
    seed: int = 42
    dtype: Optional[str] = None      # "f32" / "f64"; None: $PMF_HIP_DTYPE, else f32
    xi_init: float = 1.0
    verbose: bool = True


class LogisticMFCAVI(GaussianHost):
    """x_ij ~ Bernoulli(sigmoid(theta_i . beta_j))."""
    _uses_bias = False
    _gaussian = True

    def __init__(self, config: LogisticMFCAVIConfig, device=None, comm=None):
        if comm is not None:
            raise NotImplementedError("LogisticMFCAVI with comm=: the logistic model runs on one rank (the per-rating "
                                      "variational parameters live in one context's rating streams)")
        super().__init__(config, config.dtype, device, None, False)

    def _initialize_variational_params(self):
        """`GaussianMFCAVI`'s draw: user means, item means, 0.1 N(0, 1); identity covariances (`_prepare`)."""
        K = self.config.n_factors
        rng = np.random.default_rng(self.config.seed)
        self.m_theta = 0.1 * rng.standard_normal((self.n_users, K))
        self.m_beta = 0.1 * rng.standard_normal((self.n_items, K))
        self._V_theta = self._V_beta = None

    def _neg_kl(self, ctx, side):
        cfg = self.config
        return neg_kl(ctx.gauss_elbo_terms(side, with_data=False), ctx.rows(side), cfg.n_factors, cfg.eta2)

    def fit(self, train_df, *, unobserved="missing", weights=None):
        """`train_df`: columns u, i, rating with every rating 0 or 1.  One iteration: refresh xi on the user side's rating
        stream -> user factor sweep -> refresh xi on the item side's stream -> item factor sweep, each a coordinate ascent
        step on the bound.  `history_["elbo"]` holds the bound of every iteration at its item-side refresh (the data term
        of that refresh minus the two KL terms of the q it saw); the fit stops when its relative increase falls below
        `config.tol` (None: never)."""
        cfg = self.config
        if unobserved != "missing":
            raise NotImplementedError(f"LogisticMFCAVI with unobserved={unobserved!r}: unobserved cells as zeros are not "
                                      "available for the logistic model; list the negatives as ratings of 0")
        if weights is not None:
            raise NotImplementedError("LogisticMFCAVI with weights=: the per-rating weights carry the variational "
                                      "parameters of the bound, user-supplied weights are not available")
        u, i, x = frame_arrays(train_df)
        bad = np.flatnonzero((x != 0.0) & (x != 1.0))
        if len(bad):
            raise ValueError(f"LogisticMFCAVI: ratings must be 0 or 1, got {x[bad[0]]!r} at position {int(bad[0])}")
        self._infer_dimensions(train_df)
        self._initialize_variational_params()
        c0 = 2.0 * float(jj_lambda(cfg.xi_init))
        ctx = self._open_context(u, i, (x - 0.5) / c0, np.full(len(x), c0))
        self.history_["weighted"] = True
        self.history_["elbo"] = []
        self._elbo_counts = None
        ctx.set_array(USER, ARR_FACTOR, self.m_theta)
        ctx.set_array(ITEM, ARR_FACTOR, self.m_beta)
        self._prepare(ctx)
        kl_item = self._neg_kl(ctx, ITEM)
        for it in range(1, cfg.max_iter + 1):
            if cfg.verbose:
                print(f"\nCAVI iteration {it}/{cfg.max_iter}")
            ctx.gauss_logit_refresh(USER, want_data_term=False)
            ctx.gauss_factor_sweep(USER, 1.0, cfg.eta2)
            data = ctx.gauss_logit_refresh(ITEM)
            self.history_["elbo"].append(data + self._neg_kl(ctx, USER) + kl_item)
            ctx.gauss_factor_sweep(ITEM, 1.0, cfg.eta2)
            kl_item = self._neg_kl(ctx, ITEM)
            self._tick(it)
            if cfg.verbose:
                print(f"ELBO: {self.history_['elbo'][-1]:.4f}")
            if cfg.tol is not None and it > 1:
                before, now = self.history_["elbo"][-2:]
                if (now - before) / abs(before) < cfg.tol:
                    if cfg.verbose:
                        print("Early stopping: small increase of the ELBO.")
                    self.history_["stopped_early"] = True
                    break
        if self.history_["iterations"] > 0:
            self._pull_state()
        return self

    def elbo(self):
        """The Jaakkola-Jordan lower bound on the evidence of the training ratings at the fitted q, with every xi at its
        optimum for that q (float64): the data term of a refresh of the user side's stream (`pmf_gauss_logit_refresh`,
        which leaves that stream as the next iteration's first step would) minus the KL terms of both sides."""
        ctx = self._cov_ctx("elbo")
        return ctx.gauss_logit_refresh(USER) + self._neg_kl(ctx, USER) + self._neg_kl(ctx, ITEM)

    def decision_function(self, user_ids, item_ids):
        """The posterior mean score m_u . m_i (0 for ids outside the trained dimensions)."""
        return self._need_ctx().predict(np.asarray(user_ids, dtype=int), np.asarray(item_ids, dtype=int), use_bias=False, offset=0.0)

    def predict_variance(self, user_ids, item_ids):
        """Var[theta_u . beta_i] under the fitted q (`pmf_predict_var`); the Bernoulli likelihood has no noise term."""
        return self._cov_ctx("predict_variance").predict_var(np.asarray(user_ids, dtype=int), np.asarray(item_ids, dtype=int))

    def predict_proba(self, user_ids, item_ids, moderated=True):
        """p(x = 1): sigmoid(mu / sqrt(1 + pi v / 8)) with the score's posterior mean mu and variance v (MacKay's
        moderated output, the probit approximation of E_q[sigmoid(s)]); `moderated=False`: sigmoid(mu)."""
        mu = self.decision_function(user_ids, item_ids)
        if moderated:
            mu = mu / np.sqrt(1.0 + np.pi * self.predict_variance(user_ids, item_ids) / 8.0)
        return _sigmoid(mu)

    def predict(self, user_ids, item_ids, global_mean=0.0):
        return self.predict_proba(user_ids, item_ids)

    def log_loss(self, df, moderated=True):
        """Mean negative log-likelihood of the frame's 0 / 1 ratings under `predict_proba` (ids the fit has not seen
        predict 1/2); probabilities are clipped to [1e-15, 1 - 1e-15]."""
        u, i, x = frame_arrays(df)
        p = np.clip(self.predict_proba(u, i, moderated), 1e-15, 1.0 - 1e-15)
        return float(-np.mean(np.where(x > 0.5, np.log(p), np.log1p(-p))))

    def _refused(self, what):
        raise NotImplementedError(f"LogisticMFCAVI.{what}: not available for the logistic model")

    def fold_in_users(self, *a, **k):
        self._refused("fold_in_users")

    def fold_in_items(self, *a, **k):
        self._refused("fold_in_items")

    def log_predictive_density(self, *a, **k):
        self._refused("log_predictive_density")
