"""Host logic shared by the two Gaussian CAVI classes (with / without biases).

Iteration order, early-stop rule and verbose lines follow the reference
(`gaussian_mf_cavi_bias.py:91-286`, bias-free twin `gaussian_mf_cavi.py:81-200`);
each half-sweep is one C-ABI call (`pmf_gauss_factor_sweep`,
`pmf_gauss_bias_sweep`)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from src.evaluation.metrics import macro_mae, rmse
from src.models._device_model import ITEM, USER, DeviceModel, fold_in_batch, frame_arrays, frame_weights
from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ELBO_BIAS_SQ, ELBO_ESS, ELBO_LOGDET, ELBO_SQNORM, dist as pdist


def elbo_from_terms(user_terms, item_terms, user_counts, item_counts, n_ratings, n_factors, sigma2, eta_theta2, eta_beta2,
                    eta_bias2=None, data_side=USER, zero_weight=None, *, user_weight_sums=None, item_weight_sums=None,
                    log_weight_sum=None):
    """The evidence lower bound of a Gaussian CAVI model from the sums `pmf_gauss_elbo_terms` returns (include/pmf_hip.h
    has the definition): `user_terms` / `item_terms` are the two sides' total vectors (columns `pmf_hip.ELBO_*`),
    `user_counts` / `item_counts` the ratings per row of each side (their lengths are the row counts), `eta_bias2=None`
    the bias-free model.  The data term takes the ESS entry of `data_side`; either side's gives the same sum.  Pure
    host arithmetic in float64.  `zero_weight` (bias-free model only): the terms come from a context that counts unlisted
    cells as zeros of variance sigma2 / zero_weight (`pmf_ctx_set_gauss_zeros`), so the data constant also has the
    U I - N unlisted cells, U and I being the lengths of the two count vectors.  `user_weight_sums` / `item_weight_sums`
    / `log_weight_sum` (all three or none; the terms come from a context with rating weights, `pmf_ctx_set_ratings_weighted`):
    C_r = the sum of the weights of every row's ratings, which takes the place of the row's count in the bias variances
    and in the ESS, and sum_j log c_j, of which the data constant gains a half.  Returns (L, parts): parts names the data term and, per block of q, the expected log
    prior and the entropy; the parts add up to L."""
    terms = (np.asarray(user_terms, dtype=np.float64), np.asarray(item_terms, dtype=np.float64))
    counts = (np.asarray(user_counts, dtype=np.float64), np.asarray(item_counts, dtype=np.float64))
    K, two_pi = int(n_factors), 2.0 * np.pi
    ess = float(terms[data_side][ELBO_ESS])
    parts = {}
    given = [a is not None for a in (user_weight_sums, item_weight_sums, log_weight_sum)]
    if any(given) and not all(given):
        raise ValueError("user_weight_sums, item_weight_sums and log_weight_sum go together")
    mass = counts if not any(given) else (np.asarray(user_weight_sums, dtype=np.float64), np.asarray(item_weight_sums, dtype=np.float64))
    if eta_bias2 is not None:
        var = [1.0 / (1.0 / eta_bias2 + n / sigma2) for n in mass]       # gaussian_mf_cavi_bias.py:222 / :253
        ess += sum(float(np.sum(n * v)) for n, v in zip(mass, var))
    parts["data"] = -0.5 * n_ratings * np.log(two_pi * sigma2) - ess / (2.0 * sigma2)
    if any(given):
        parts["data"] += 0.5 * float(log_weight_sum)
    if zero_weight is not None:
        if eta_bias2 is not None:
            raise ValueError("zero_weight: unlisted cells as weighted zeros are defined for the bias-free model only")
        n_unlisted = float(len(counts[0])) * float(len(counts[1])) - n_ratings
        parts["data"] -= 0.5 * n_unlisted * np.log(two_pi * sigma2 / zero_weight)
    for name, t, n, eta2 in (("theta", terms[0], counts[0], eta_theta2), ("beta", terms[1], counts[1], eta_beta2)):
        rk = len(n) * K
        parts["prior_" + name] = -0.5 * rk * np.log(two_pi * eta2) - float(t[ELBO_SQNORM]) / (2.0 * eta2)
        parts["entropy_" + name] = 0.5 * rk * (1.0 + np.log(two_pi)) + 0.5 * float(t[ELBO_LOGDET])
    if eta_bias2 is not None:
        for name, t, v in (("user_bias", terms[0], var[0]), ("item_bias", terms[1], var[1])):
            parts["prior_" + name] = (-0.5 * len(v) * np.log(two_pi * eta_bias2)
                                      - (float(t[ELBO_BIAS_SQ]) + float(np.sum(v))) / (2.0 * eta_bias2))
            parts["entropy_" + name] = 0.5 * float(np.sum(1.0 + np.log(two_pi * v)))
    parts = {k: float(v) for k, v in parts.items()}
    return float(sum(parts.values())), parts


@dataclass
class FoldIn:
    """Posterior of folded-in rows (`fold_in_users` / `fold_in_items`): row r belongs to label `ids[r]`."""
    ids: np.ndarray            # the new side's labels, sorted
    mean: np.ndarray           # (n, K)
    cov: Optional[np.ndarray]  # (n, K, K), or None unless asked for
    bias: np.ndarray           # (n,), zeros for the bias-free model
    m_other: np.ndarray        # the fitted opposite side's means (and biases, or None)
    b_other: Optional[np.ndarray]
    side: int = USER                          # the side the rows belong to
    seen_ptr: Optional[np.ndarray] = None     # the batch `fold_in_batch` built: row r's own ratings are of the ids
    seen_ids: Optional[np.ndarray] = None     # seen_ids[seen_ptr[r]:seen_ptr[r + 1]] on the opposite side

    def predict(self, rows, other_ids, global_mean=0.0):
        """mean[rows] . m_other[other_ids] + bias[rows] + b_other[other_ids] + global_mean, on the host."""
        rows, other_ids = np.asarray(rows, dtype=int), np.asarray(other_ids, dtype=int)
        out = np.einsum("nk,nk->n", self.mean[rows], self.m_other[other_ids]) + self.bias[rows] + global_mean
        return out if self.b_other is None else out + self.b_other[other_ids]


class GaussianHost(DeviceModel):
    _has_covariances = True      # False for the MAP / gradient subclass: no posterior, no predictive variance

    def __init__(self, config, dtype=None, device=None, comm=None, presharded=False):
        super().__init__(config, dtype, device, comm, presharded)
        self.m_theta = self.m_beta = None
        self._V_theta = self._V_beta = None
        self._elbo_counts = None     # (ratings per user, per item) of the last single-process fit
        self._log_weight_sum = None  # sum_j log c_j of the last fit with weights
        self.global_mean = 0.0
        if self._uses_bias:
            self.m_user_bias = self.m_item_bias = None

    # The covariance stacks are rows x K x K float64 on the host (32 GB at
    # 1M x 64 x 64): they stay packed on the device and are materialised only
    # when the attribute is read.
    def _train_ctx(self):
        return getattr(self, "_shard_ctx", None) or self._ctx

    @property
    def V_theta(self):
        """(n_users, K, K) float64.  After a SHARDED fit this is only THIS RANK's user range
        (rows `user_range`): an attribute read must not hide a collective (a rank-0-only read
        would deadlock the job, and the full stack is U x K x K x 8 bytes on every rank).  All ranks
        together call `gather_V_theta()` for the full stack."""
        if self._V_theta is None and self._ctx is not None:
            self._V_theta = self._train_ctx().get_array(USER, ARR_COV)
        return self._V_theta

    @property
    def user_range(self):
        """[lo, hi) of the users this rank trained (all users when not sharded)."""
        if self._comm is None or self._bounds is None:
            return 0, self.n_users
        return int(self._bounds[self._comm.rank]), int(self._bounds[self._comm.rank + 1])

    def gather_V_theta(self):
        """Collective after a sharded fit: every rank gets the full (n_users, K, K) covariance stack
        (broadcast in 64 MB row blocks).  Equals `V_theta` when not sharded."""
        if self._comm is None:
            return self.V_theta
        return self._user_array(ARR_COV, self._train_ctx())

    @V_theta.setter
    def V_theta(self, value):
        self._V_theta = value

    def V_theta_rows(self, user_ids):
        """`V_theta[user_ids]` (len x K x K float64) read straight from the device's packed storage
        (`pmf_get_array_rows`) -- what the reference's row indexing does (gaussian_mf_cavi_bias.py:157-162)
        without materialising the whole stack.  After a sharded fit the ids must lie in `user_range`."""
        ids = np.asarray(user_ids, dtype=np.int64).reshape(-1)
        if self._V_theta is not None:
            return np.asarray(self._V_theta)[ids - self.user_range[0]]
        lo, hi = self.user_range
        if len(ids) and (ids.min() < lo or ids.max() >= hi):
            raise IndexError(f"V_theta_rows: user ids outside this rank's range [{lo}, {hi})")
        return self._train_ctx().get_array_rows(USER, ARR_COV, ids - lo)

    def V_beta_rows(self, item_ids):
        """`V_beta[item_ids]` (len x K x K float64), same idea."""
        ids = np.asarray(item_ids, dtype=np.int64).reshape(-1)
        if self._V_beta is not None:
            return np.asarray(self._V_beta)[ids]
        return self._train_ctx().get_array_rows(ITEM, ARR_COV, ids)

    @property
    def V_beta(self):
        if self._V_beta is None and self._ctx is not None:
            self._V_beta = self._train_ctx().get_array(ITEM, ARR_COV)
        return self._V_beta

    @V_beta.setter
    def V_beta(self, value):
        self._V_beta = value

    def _initialize_variational_params(self):
        """Reference draw order (gaussian_mf_cavi_bias.py:52-67): user means, item means."""
        K = self.config.n_factors
        rng = np.random.default_rng(self.config.random_state)
        self.m_theta = 0.1 * self._user_rows(lambda n: rng.standard_normal((n, K)))
        self.m_beta = 0.1 * rng.standard_normal((self.n_items, K))
        if self._uses_bias:
            self.m_user_bias = np.zeros(len(self.m_theta))
            self.m_item_bias = np.zeros(self.n_items)
        self._V_theta = self._V_beta = None

    def _pull_state(self):
        ctx, g = self._ctx, self._user_array
        self.m_theta, self.m_beta = g(ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
        arrays = [(USER, ARR_FACTOR, self.m_theta), (ITEM, ARR_FACTOR, self.m_beta)]
        if self._uses_bias:
            self.m_user_bias, self.m_item_bias = g(ARR_BIAS), ctx.get_array(ITEM, ARR_BIAS)
            arrays += [(USER, ARR_BIAS, self.m_user_bias), (ITEM, ARR_BIAS, self.m_item_bias)]
        self._V_theta = self._V_beta = None
        if self._comm is not None:
            self._finish_sharded(arrays)

    # ---- what one iteration is (the MAP / gradient subclass overrides these two) ----
    _iteration_label = "CAVI iteration"

    def _prepare(self, ctx):
        ctx.set_cov_identity(USER, 1.0)
        ctx.set_cov_identity(ITEM, 1.0)

    @staticmethod
    def _should_stop(improvement, tol):
        return improvement >= 0 and improvement < tol   # gaussian_mf_cavi_bias.py:279

    def _iterate(self, ctx):
        cfg = self.config
        pdist.gaussian_iteration(ctx, self._comm, None, None, cfg.sigma2, cfg.eta_theta2,
                                 cfg.eta_beta2, cfg.eta_bias2 if self._uses_bias else None)

    def _check_unobserved(self, unobserved, zero_weight, train_df):
        """`fit`'s `unobserved` / `zero_weight` -> whether unlisted cells count as weighted zeros; every refusal is made
        here, before any device call."""
        if unobserved not in ("missing", "zero"):
            raise ValueError(f"unobserved must be 'missing' or 'zero', not {unobserved!r}")
        if unobserved == "missing":
            return False
        if self._uses_bias or not self._has_covariances:
            raise NotImplementedError(f"unobserved='zero' is not available for {type(self).__module__.split('.')[-1]}."
                                      f"{type(self).__name__}: the bias-free gaussian_mf_cavi.GaussianMFCAVI supports it")
        if self._comm is not None:
            raise ValueError("unobserved='zero' with comm=: counting unobserved cells as zeros is not available on several ranks")
        if not (np.isfinite(zero_weight) and 0.0 < zero_weight <= 1.0):
            raise ValueError(f"zero_weight must lie in (0, 1], not {zero_weight!r}")
        if train_df.duplicated(subset=["u", "i"]).any():
            raise ValueError("unobserved='zero': train_df lists a (u, i) pair more than once; a cell has one rating")
        return True

    def fit(self, train_df, val_df=None, global_mean=0.0, *, track_elbo=False, elbo_tol=None, unobserved="missing",
            zero_weight=1.0, weights=None):
        """`track_elbo`: evaluate the evidence lower bound after every iteration (`history_["elbo"]`; about 1.3
        accumulates of the user side more per iteration).  `elbo_tol` (implies `track_elbo`): stop when the relative increase
        (L_t - L_{t-1}) / |L_{t-1}| falls below it -- an early stop that needs no `val_df`.
        `unobserved`: "missing" (default) -- the rating list is the whole data set, as in the reference; "zero"
        (`gaussian_mf_cavi.GaussianMFCAVI` only) -- every (user, item) cell without a rating is an observation of 0, in
        this call's rating convention, with variance sigma2 / `zero_weight`, `zero_weight` in (0, 1]: the model clicks,
        purchases and plays need, "implicit ALS" with full posterior covariances (`pmf_ctx_set_gauss_zeros`: the row
        statistics are blended with the other side's Gram matrix).  `zero_weight=1` equals the
        default fit of the frame with every missing cell listed as 0; 1 / (1 + alpha) is the usual confidence ratio.
        Recorded in `history_["unobserved"]` / `history_["zero_weight"]` and kept on the fit's context: `elbo()`,
        `track_elbo`, `fold_in_users` and `fold_in_items` run in the same mode.  "zero" refuses duplicate (u, i) pairs
        and `comm=`; negative ratings are fine.
        `weights`: None, the name of a column of `train_df`, or an array of len(train_df): a confidence weight c_j per
        rating, finite and > 0, which gives rating j the precision c_j / sigma2 (`pmf_ctx_set_ratings_weighted`,
        DESIGN.md section 4.18) -- `sample_weight` for explicit ratings (recency decay, de-duplicated counts,
        inverse-propensity weights) and, with `unobserved="zero"`, `zero_weight=1`, ratings of 1 and c = 1 + alpha r, the
        implicit-feedback model of Hu, Koren & Volinsky.  Recorded in `history_["weighted"]`; `elbo()`, `track_elbo` and
        `elbo_tol` follow the weights.  Refused with `comm=` and by the gradient class."""
        cfg = self.config
        zeros = self._check_unobserved(unobserved, zero_weight, train_df)
        weights = frame_weights(train_df, weights)
        if weights is not None:
            if not self._has_covariances:
                raise NotImplementedError(f"{type(self).__name__}: rating weights are not available in the gradient mode")
            if self._comm is not None:
                raise ValueError("weights with comm=: rating weights are not available on several ranks")
        track_elbo = bool(track_elbo) or elbo_tol is not None
        if track_elbo:
            if not self._has_covariances:
                raise NotImplementedError(f"{type(self).__name__} keeps point estimates, no covariances: the ELBO is not defined")
            if self._comm is not None:
                raise NotImplementedError("track_elbo under a communicator: the ELBO of a sharded fit is not implemented")
        self.global_mean = global_mean
        self._infer_dimensions(train_df)
        self._initialize_variational_params()
        u, i, x = frame_arrays(train_df)
        ctx = self._open_context(u, i, x, weights)
        self.history_["weighted"] = weights is not None
        self._log_weight_sum = None if weights is None else float(np.sum(np.log(weights)))
        if zeros:
            ctx.set_gauss_zeros(True, zero_weight)
        self.history_["unobserved"], self.history_["zero_weight"] = unobserved, float(zero_weight)
        self.history_.pop("elbo", None)
        self._elbo_counts = None
        if self._comm is None:      # rating counts per row: what `elbo` needs besides the device's sums
            self._elbo_counts = (np.bincount(u, minlength=self.n_users), np.bincount(i, minlength=self.n_items))
        if track_elbo:
            self.history_["elbo"] = []
        ctx.set_array(USER, ARR_FACTOR, self._mine(self.m_theta))
        ctx.set_array(ITEM, ARR_FACTOR, self.m_beta)
        if self._uses_bias:
            ctx.set_array(USER, ARR_BIAS, self._mine(self.m_user_bias))
            ctx.set_array(ITEM, ARR_BIAS, self.m_item_bias)
        self._prepare(ctx)
        monitor = self._monitor_setup(val_df, offset=global_mean, drop_unseen=True)
        previous = None
        for it in range(1, cfg.max_iter + 1):
            if cfg.verbose:
                print(f"\n{self._iteration_label} {it}/{cfg.max_iter}")
            self._run_iteration(lambda: self._iterate(ctx))
            self._tick(it)
            elbo_stop = False
            if track_elbo:
                self.history_["elbo"].append(self._elbo_of(ctx)[0])
                if cfg.verbose:
                    print(f"ELBO: {self.history_['elbo'][-1]:.4f}")
                if elbo_tol is not None and it > 1:
                    before, now = self.history_["elbo"][-2:]
                    elbo_stop = (now - before) / abs(before) < elbo_tol
            if monitor is not None:    # (before the ELBO stop: every iteration that ran has its validation entries)
                val_rmse, val_macro_mae = monitor()
                self._record(val_rmse, val_macro_mae)
                if cfg.verbose:
                    if self._uses_bias:
                        print(f"Validation RMSE: {val_rmse:.4f} | MacroMAE: {val_macro_mae:.4f}")
                    else:
                        print(f"Validation RMSE: {val_rmse:.4f}")
            if elbo_stop:
                if cfg.verbose:
                    print("Early stopping: small increase of the ELBO.")
                self.history_["stopped_early"] = True
                break
            if monitor is None:
                continue
            if previous is not None:
                improvement = previous - val_rmse
                if cfg.verbose:
                    print(f"Improvement: {improvement:.6f}")
                if self._should_stop(improvement, cfg.tol):
                    if cfg.verbose:
                        print("Early stopping: small improvement on validation.")
                    self.history_["stopped_early"] = True
                    break
            previous = val_rmse
        if self.history_["iterations"] > 0:
            self._pull_state()
        return self

    def predict(self, user_ids, item_ids, global_mean=0.0):
        return self._need_ctx().predict(np.asarray(user_ids, dtype=int), np.asarray(item_ids, dtype=int),
                                        use_bias=self._uses_bias, offset=global_mean)

    # ---- posterior predictive variance / density (extension: no reference counterpart) ----
    def _cov_ctx(self, what):
        """The context that holds FACTOR and COV of both sides for all users, or the reason there is none."""
        if not self._has_covariances:
            raise NotImplementedError(f"{type(self).__name__} keeps point estimates, no covariances: {what} is not defined")
        ctx = self._need_ctx()
        if self._shard_ctx is not None:
            raise NotImplementedError(f"{what} after a sharded fit: the full-size context holds no covariances "
                                      "(they stay on the ranks' shard contexts)")
        return ctx

    def _sample_ctx(self, what):
        """Posterior draws read FACTOR and COV of all rows of both sides: a single-process fit of a CAVI class."""
        if self._comm is not None:
            raise NotImplementedError(f"{what} with comm=: the user covariances stay sharded over the ranks")
        return self._cov_ctx(what)

    def predict_variance(self, user_ids, item_ids, include_noise=True):
        """Var[theta_u . beta_i] = m_u' V_i m_u + m_i' V_u m_i + tr(V_u V_i) under the fitted q (float64; the biases
        are point values; 0 for ids outside the trained dimensions, which `predict` treats as the point 0), plus
        `config.sigma2` when `include_noise`: the variance of the rating itself.  One pass over the packed covariance
        rows on the device (`pmf_predict_var`); nothing K x K reaches the host."""
        var = self._cov_ctx("predict_variance").predict_var(np.asarray(user_ids, dtype=int), np.asarray(item_ids, dtype=int))
        return var + self.config.sigma2 if include_noise else var

    def log_predictive_density(self, df, global_mean=0.0):
        """TOTAL over the rows of `df` with seen ids (as the reference's GaussianLogPredictiveLikelihood returns a
        total) of log N(rating + global_mean; predict, sigma2 + Var[f]).  Row filter and target as in
        `evaluate_rmse`; nan (with its warning) when no row is left.  Fused on the device (`pmf_eval_run_var`); the
        stored validation set of the context is replaced."""
        ctx = self._cov_ctx("log_predictive_density")
        df = self._seen(df)
        if df.empty:
            print("Warning: No valid (u,i) pairs.")
            return np.nan
        u, i = df["u"].to_numpy(dtype=int), df["i"].to_numpy(dtype=int)
        y = df["rating"].to_numpy(dtype=float) + global_mean
        sigma2 = self.config.sigma2
        if ctx.eval_set(u, i, y):
            return ctx.eval_var_sums(self._uses_bias, global_mean, sigma2)[2]
        # more distinct ratings than the stored set's label table takes: device predict / predict_var, host sum
        d = sigma2 + ctx.predict_var(u, i)
        e = y - ctx.predict(u, i, use_bias=self._uses_bias, offset=global_mean)
        return float(np.sum(-0.5 * np.log(2.0 * np.pi * d) - e * e / (2.0 * d)))

    # ---- evidence lower bound (extension: the reference never evaluates its objective) ----
    def _elbo_of(self, ctx):
        cfg = self.config
        user = ctx.gauss_elbo_terms(USER, with_data=True)      # the data term from the user side: its gathers hit the smaller item table
        item = ctx.gauss_elbo_terms(ITEM, with_data=False)
        if self._elbo_counts is None:
            raise NotImplementedError("elbo after a fit under a communicator: the ELBO of a sharded fit is not implemented")
        nu, ni = self._elbo_counts
        observed, weight = ctx.gauss_zeros
        weighted = {}
        if self.history_.get("weighted"):
            weighted = dict(user_weight_sums=ctx.rating_weight_sums(USER), item_weight_sums=ctx.rating_weight_sums(ITEM),
                            log_weight_sum=self._log_weight_sum)
        return elbo_from_terms(user, item, nu, ni, int(nu.sum()), cfg.n_factors, cfg.sigma2, cfg.eta_theta2, cfg.eta_beta2,
                               cfg.eta_bias2 if self._uses_bias else None, zero_weight=weight if observed else None, **weighted)

    def elbo(self, parts=False):
        """The evidence lower bound of the fitted q on the training ratings, for the config's sigma2 / eta2 (float64):
        E_q[log p(ratings | theta, beta, biases)] + E_q[log prior] + entropy of q, where q is Gaussian per row with the
        fitted means and covariances (and, in the bias model, the bias variances the updates imply).  The sums over
        rows and ratings are formed on the device (`pmf_gauss_elbo_terms`: 1.3 times an accumulate of the user side);
        `parts=True` also returns the dict of `elbo_from_terms`."""
        value, named = self._elbo_of(self._cov_ctx("elbo"))
        return (value, named) if parts else value

    # ---- fold-in of unseen users / items (extension: no reference counterpart as an operation) ----
    def _fold_in(self, what, side, df, n_iter, return_cov, weights=None):
        weights = frame_weights(df, weights)
        ctx = self._cov_ctx(what)
        ids, row_ptr, other, x, *w = fold_in_batch(df, side, self.n_items if side == USER else self.n_users, weights)
        cfg = self.config
        mean, cov, bias = ctx.gauss_fold_in(side, row_ptr, other, x, cfg.sigma2,
                                            cfg.eta_theta2 if side == USER else cfg.eta_beta2,
                                            cfg.eta_bias2 if self._uses_bias else 1.0, n_iter, want_cov=return_cov,
                                            **({"weights": w[0]} if w else {}))
        m_other = self.m_beta if side == USER else self.m_theta
        b_other = (self.m_item_bias if side == USER else self.m_user_bias) if self._uses_bias else None
        return FoldIn(ids, mean, cov, bias, m_other, b_other, side, row_ptr, other)

    def fold_in_users(self, df, n_iter=10, return_cov=False, weights=None):
        """Posterior of users the fit has not seen, from their ratings of fitted items: `df` has columns u, i, rating
        in `fit`'s rating convention; `u` holds arbitrary labels.  The item side stays frozen; each user gets the
        factor update and (bias model) `n_iter` factor / bias alternations from a zero bias -- the reference's own
        row updates, on the device (`pmf_gauss_fold_in`), without a refit.  Rows with an item id the fit has not seen
        are dropped; a user left without ratings gets the prior (after `fit(unobserved="zero")`: the posterior of a row of
        zeros, as every other row's unlisted cells are zeros too).  `weights`: as in `fit`, one confidence weight per row
        of `df` (`pmf_gauss_fold_in_weighted`).  Returns a `FoldIn`, one row per label in sorted order."""
        return self._fold_in("fold_in_users", USER, df, n_iter, return_cov, weights)

    def fold_in_items(self, df, n_iter=10, return_cov=False, weights=None):
        """The same for new items (labels in column `i`) against the fitted users."""
        return self._fold_in("fold_in_items", ITEM, df, n_iter, return_cov, weights)

    def _seen(self, df):
        keep = (df["u"] < self.n_users) & (df["i"] < self.n_items)
        return df[keep]

    def evaluate_rmse(self, df, global_mean):
        df = self._seen(df)
        if df.empty:
            print("Warning: No valid (u,i) pairs.")
            return np.nan
        y_true = df["rating"].to_numpy(dtype=float) + global_mean
        return rmse(y_true, self.predict(df["u"].to_numpy(), df["i"].to_numpy(), global_mean))

    def evaluate_macro_mae(self, df, global_mean):
        df = self._seen(df)
        if df.empty:
            return np.nan
        y_true = df["rating"].to_numpy(dtype=float) + global_mean
        return macro_mae(y_true, self.predict(df["u"].to_numpy(), df["i"].to_numpy(), global_mean))
