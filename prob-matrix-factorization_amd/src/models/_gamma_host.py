"""Host logic shared by the two gamma CAVI classes (Poisson MF and HPF).

Iteration order, early-stop rule and verbose lines follow the reference (`poisson_mf_cavi.py:118-222`,
`hpf_cavi.py:112-216`); each half-sweep is one C-ABI call (`pmf_gamma_sweep` / `pmf_gamma_exact_sweep`).  A subclass
supplies `_iteration_label`, `_draw_start` (its reference-named initialiser), `_upload_start`, `_priors`,
`_pull_state` and `_elbo_priors`."""
import numpy as np

from src.evaluation.metrics import macro_mae, rmse
from src.models._device_model import ITEM, USER, DeviceModel, frame_arrays
from src.models import _gamma_elbo, _gamma_predictive
from src.models._gamma_fold_in import gamma_fold_in
from pmf_hip import dist as pdist


class GammaModel(DeviceModel):
    def fit(self, train_df, val_df=None, *, track_elbo=False, elbo_tol=None, update="reference", track_loglik=False, loglik_tol=None,
            loglik_kind="plugin", unobserved="missing"):
        """`track_elbo`: evaluate the evidence lower bound after every iteration (`history_["elbo"]`, an `ELBO:` line
        when verbose; measured at K = 64 fp32, 1M users, 50M ratings: the user call's two kernels take 3.00 times a user
        half-sweep (the data pass 2.34 times the sweep's gather ceiling); an `elbo()` takes 5.27 times a whole iteration by wall
        clock, 1.30 times in kernel time -- the rest is the download and the host's sum of the per-row terms).  `elbo_tol` (implies `track_elbo`): stop when (L_t - L_{t-1}) / |L_{t-1}| falls below
        it -- an early stop that needs no `val_df`.  The rule also fires on a DECREASE, which can happen here: the
        reference's row update weights the factors with E[theta] E[beta] / (E[theta] . E[beta]) where exact CAVI uses
        exp(E log theta + E log beta), so an iteration is not exact coordinate ascent on this bound.
        `update`: "reference" (default) runs the reference's row update, which weights a rating's factors with
        E[theta] E[beta] / (E[theta] . E[beta]); "exact" runs coordinate ascent on the bound (`pmf_gamma_exact_sweep`: weights
        exp(E log theta + E log beta), normalised, formed from the shapes and rates), under which the bound cannot fall from
        one half-sweep to the next, except by rounding.  `history_["update"]` records the mode.  A negative training rating
        is refused under "exact".  Cost of an exact half-sweep: DESIGN.md section 4.12.
        `track_loglik` (needs `val_df`): after every iteration the total held-out log-likelihood of the validation rows
        with seen ids goes to `history_["val_loglik"]` (a `Validation log-likelihood:` line when verbose), formed on the
        device from the shapes and rates (`pmf_gamma_predictive`), for any number of distinct ratings.  `loglik_kind`:
        "plugin" (default: the reference's PoissonLogPredictiveLikelihood at the factor means), "bound" or "negbin", as
        for `log_predictive_density`.  `loglik_tol` (implies `track_loglik`): stop when (L_t - L_{t-1}) / |L_{t-1}| falls
        below it -- the stopping rule of the HPF paper; it fires on a decrease too.  It is independent of, and checked after,
        the RMSE rule and `elbo_tol`.  Cost: DESIGN.md section 4.13.
        `unobserved`: "missing" (default) -- the rating list is the whole data set, as in the reference; "zero" -- every
        (user, item) cell without a rating is a count of 0, the model of the HPF paper and the one click, purchase or play
        counts need (`pmf_ctx_set_gamma_zeros`: the rate sums come from the other side's column sums, the cost does not
        depend on the number of cells).  The fit equals a "missing" fit of the frame with every
        missing cell listed as an explicit 0.  Works with both `update`s; recorded in `history_["unobserved"]` and kept
        with the model: `elbo()`, `track_elbo`, `fold_in_users` and `fold_in_items` of the fitted model run in the same
        mode (a new row's unlisted cells are zeros too).  "zero" refuses a negative rating, duplicate (u, i) pairs (a cell
        has one count) and `comm=` (not available on several ranks)."""
        cfg = self.config
        zeros = _gamma_elbo.check_unobserved(self, unobserved, train_df)
        exact = _gamma_elbo.check_update(update, train_df)
        track_elbo = _gamma_elbo.check_tracking(self, track_elbo, elbo_tol, train_df)
        track_loglik = _gamma_predictive.check_tracking(self, track_loglik, loglik_tol, loglik_kind, val_df)
        self._infer_dimensions(train_df)
        self._draw_start()
        u, i, x = frame_arrays(train_df)
        ctx = self._open_context(u, i, x)
        if zeros:                      # (a new context starts in "missing": a default fit makes the calls it made)
            ctx.set_gamma_zeros(True)
        self.unobserved_ = unobserved
        self.history_["unobserved"] = unobserved
        self.history_.pop("elbo", None)
        if track_elbo:
            self.history_["elbo"] = []
        self.history_.pop("val_loglik", None)
        if track_loglik:
            self.history_["val_loglik"] = []
        self.history_["update"] = update
        self._upload_start(ctx, exact)
        user_prior, item_prior = self._priors()
        monitor = self._monitor_setup(val_df)
        loglik = _gamma_predictive.monitor_setup(self, ctx, val_df, loglik_kind) if track_loglik else None
        previous = None
        for it in range(1, cfg.max_iter + 1):
            if cfg.verbose:
                print(f"\n{self._iteration_label} {it}/{cfg.max_iter}")
            # users then items (poisson_mf_cavi.py:135-200; hpf_cavi.py:126-193, xi and eta with their sides); with a
            # Comm the library runs the item half-sweep as accumulate -> all-reduce -> finalize
            self._run_iteration(lambda: pdist.gamma_iteration(ctx, self._comm, None, user_prior, item_prior, exact=exact))
            self._tick(it)
            elbo_stop = track_elbo and _gamma_elbo.record_elbo(self, ctx, it, elbo_tol)
            loglik_stop = track_loglik and _gamma_predictive.record_loglik(self, loglik, it, loglik_tol)
            if monitor is not None:    # (before the ELBO stop: every iteration that ran has its validation entries)
                val_rmse, val_macro_mae = monitor()
                self._record(val_rmse, val_macro_mae)
                if cfg.verbose:
                    print(f"Validation RMSE: {val_rmse:.4f} | MacroMAE: {val_macro_mae:.4f}")
            if elbo_stop:
                if cfg.verbose:
                    print("Early stopping: ELBO change below elbo_tol.")
                self.history_["stopped_early"] = True
                break
            if monitor is None:
                continue
            if previous is not None:
                improvement = previous - val_rmse
                if cfg.verbose:
                    print(f"Improvement: {improvement:.6f}")
                if cfg.tol is not None and improvement < cfg.tol:  # poisson_mf_cavi.py:213, hpf_cavi.py:207
                    if cfg.verbose:
                        print("Early stopping.")
                    self.history_["stopped_early"] = True
                    break
            previous = val_rmse
            if loglik_stop:    # (after the other two rules: every iteration that ran has all its entries)
                if cfg.verbose:
                    print("Early stopping: validation log-likelihood change below loglik_tol.")
                self.history_["stopped_early"] = True
                break
        if self.history_["iterations"] > 0:
            self._pull_state()
        return self

    def fold_in_users(self, df, n_iter=10, update="reference"):
        """Variational parameters of users the fit has not seen, from their ratings of fitted items: `df` has columns
        u, i, rating; `u` holds arbitrary labels.  The item side stays frozen; each user gets `n_iter` row updates
        (poisson_mf_cavi.py:135-167; theta then xi, hpf_cavi.py:126-159) from the prior mean, on the device
        (`pmf_gamma_fold_in`), without a refit.  Rows with an item id the fit has not seen are dropped; a user left
        without ratings runs the same updates on empty sums.
        `update`: "reference" (default, whatever `update` the fit ran) runs the reference's row update against the fitted
        items' expected factors; "exact" runs coordinate ascent on the bound (`pmf_gamma_fold_in_exact`: the weights of
        `fit(update="exact")`, formed from the fitted items' shapes and rates and the row's own, which are re-formed
        between the passes), under which a folded row's bound cannot fall from pass to pass, except by rounding -- the
        update to serve a model fitted with `update="exact"` with.  Any other value is a ValueError.  "exact" needs a
        fit that ran at least one iteration, and after a sharded fit (`comm=`) it raises NotImplementedError: the
        full-size serving context holds the expected factors only, not the shapes and rates.  The record's `update` names
        the one that ran.
        After `fit(unobserved="zero")` a new user's unlisted items are zeros too: the rate is the prior rate plus the
        column sum of the fitted items' factors.  Returns a `GammaFoldIn`, one row per label in sorted order."""
        return gamma_fold_in(self, USER, df, n_iter, self._priors()[USER], update)

    def fold_in_items(self, df, n_iter=10, update="reference"):
        """The same for new items (labels in column `i`) against the fitted users (poisson_mf_cavi.py:173-197,
        hpf_cavi.py:162-193); `update` as for `fold_in_users`."""
        return gamma_fold_in(self, ITEM, df, n_iter, self._priors()[ITEM], update)

    def elbo(self, parts=False):
        """The evidence lower bound of the fitted q on the training ratings, for the config's priors (float64):
        E_q[log p(ratings | theta, beta)] + E_q[log prior] + entropy of q, where q(theta_uk) = Gamma(shape, rate) with the
        fitted shapes and rates, under HPF q(xi_u) = Gamma(a' + K a, gamma_b_xi) (items alike), and the auxiliary multinomials are at their optimum.  The sums over rows and ratings are
        formed on the device (`pmf_gamma_elbo_terms`; measured at K = 64 fp32, 1M users, 50M ratings: the user call's two kernels take 3.00 times a user
        half-sweep (the data pass 2.34 times the sweep's gather ceiling); an `elbo()` takes 5.27 times a whole iteration by wall
        clock, 1.30 times in kernel time -- the rest is the download and the host's sum of the per-row terms); `parts=True` also returns the dict of
        `elbo_from_gamma_terms`."""
        return _gamma_elbo.fitted_elbo(self, parts)

    def predict_variance(self, user_ids, item_ids, include_noise=True):
        """Var[theta_u . beta_i] under the fitted q(theta_uk) = Gamma(shape, rate) (items alike; the factors are
        independent): sum_k E_k^2 (1/a_k + 1/c_k + 1/(a_k c_k)) with E_k the product of the two means and a, c the two
        shapes (float64), plus the mean itself when `include_noise`: a count's own variance is E[rate] + Var[rate].  0 for
        ids the fit has not seen, which `predict` treats as the point 0.  Formed on the device (`pmf_gamma_predictive`)."""
        return _gamma_predictive.predict_variance(self, user_ids, item_ids, include_noise)

    def log_predictive_density(self, df, kind="negbin", per_row=False):
        """TOTAL over the rows of `df` with seen ids (as the reference's PoissonLogPredictiveLikelihood returns a total) of
        the log density of the rating under the fitted q; rows with an unseen id are skipped, nan (with the warning) when
        none is left, a negative rating is a ValueError.  `kind`: "plugin" -- Poisson at the factor means,
        max(mean, 1e-10), the reference's metric; "bound" -- the ELBO's data term on the held-out pair, a lower bound on
        the log density of the exact predictive; "negbin" (default) -- the negative binomial whose rate is the Gamma with the mean and
        variance of theta_u . beta_i under q, which is as wide as q is unsure.  `per_row=True` also returns the terms of the kept rows,
        in frame order.  Formed on the device (`pmf_gamma_predictive`: the densities in double from the mean and variance
        it returns); the context is only read."""
        return _gamma_predictive.log_predictive_density(self, df, kind, per_row)

    def predict(self, user_ids, item_ids):
        return self._need_ctx().predict(np.asarray(user_ids, dtype=int), np.asarray(item_ids, dtype=int))

    def evaluate_rmse(self, df):
        return rmse(df["rating"].to_numpy(), self.predict(df["u"].to_numpy(), df["i"].to_numpy()))

    def evaluate_macro_mae(self, df):
        return macro_mae(df["rating"].to_numpy(), self.predict(df["u"].to_numpy(), df["i"].to_numpy()))
