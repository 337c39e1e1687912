"""The posterior predictive of the count models without a GPU: the reference of tests/gamma_predictive_reference.py against
brute force and against the project's host metric, and the argument checks of the model classes that are made before any
device call."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
from scipy.special import gammaln

import gamma_predictive_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against brute force -------------------------------------------------------------------------------
def test_variance_is_the_closed_second_moment_on_a_hand_worked_example():
    """3 users x 2 items x K = 2.  Var[theta . beta] = sum_k ( E[theta_k^2] E[beta_k^2] - E_k^2 ) for independent factors
    (the cross terms k != l cancel against mu^2), with E[theta^2] = a (a + 1) / b^2 for Gamma(a, b).  Pair (0, 0) by hand:
    a = (2, 1/2), b = (1, 4), c = (3, 1), d = (2, 1/2): E = (3, 1/4), mu = 13/4; k = 1: 2 3 3 4 / (1 4) - 9 = 9;
    k = 2: (1/2)(3/2)(1)(2) / (16 / 4) - 1/16 = 5/16; v = 149/16."""
    st = {"a_theta": np.array([[2.0, 0.5], [0.3, 7.0], [40.0, 1.0]]), "b_theta": np.array([[1.0, 4.0], [2.0, 0.25], [8.0, 3.0]]),
          "a_beta": np.array([[3.0, 1.0], [0.05, 12.0]]), "b_beta": np.array([[2.0, 0.5], [50.0, 1.5]])}
    u, i = np.repeat(np.arange(3), 2), np.tile(np.arange(2), 3)
    got = ref.predictive(st, u, i)
    assert got["mu"][0] == 3.25 and abs(got["v"][0] - 149.0 / 16.0) <= 4 * 2.0 ** -52 * 149.0 / 16.0     # (1/3 is rounded)
    a, b, c, d = st["a_theta"][u], st["b_theta"][u], st["a_beta"][i], st["b_beta"][i]
    second = (a * (a + 1.0) / b ** 2) * (c * (c + 1.0) / d ** 2)
    first = (a / b) * (c / d)
    np.testing.assert_allclose(got["v"], (second - first ** 2).sum(axis=1), rtol=1e-13)
    np.testing.assert_allclose(got["mu"], first.sum(axis=1), rtol=1e-15)
    # the count's own variance is mu + v: E[Var[x | rate]] + Var[E[x | rate]]
    assert (got["v"] > 0).all()


def test_moments_agree_with_draws_from_q():
    """400 000 seeded draws of one pair's factors: mean and variance of theta . beta within 5 standard errors (the fourth
    moment of the draws gives the standard error of the variance)."""
    rng = np.random.default_rng(11)
    a, b, c, d = np.array([[2.0, 0.7, 5.0]]), np.array([[1.5, 2.0, 4.0]]), np.array([[3.0, 1.2, 0.9]]), np.array([[2.0, 0.8, 1.1]])
    mu, v, _, _ = ref.moments(a, b, c, d)
    n = 400_000
    f = (rng.gamma(a, 1.0 / b, size=(n, 3)) * rng.gamma(c, 1.0 / d, size=(n, 3))).sum(axis=1)
    assert abs(f.mean() - mu[0]) < 5.0 * math.sqrt(v[0] / n)
    dev = (f - f.mean()) ** 2
    assert abs(dev.mean() - v[0]) < 5.0 * dev.std() / math.sqrt(n)


def test_bound_is_below_plugin_on_random_states():
    """Jensen: E log theta_k + E log beta_k <= log E_k, so lse <= log mu and BOUND <= PLUGIN for x >= 0 (where the clamp
    is inactive)."""
    rng = np.random.default_rng(3)
    for K in (1, 2, 7, 40):
        lu = lambda lo, hi, size: np.exp(rng.uniform(np.log(lo), np.log(hi), size=size))
        st = {"a_theta": lu(0.05, 1e4, (30, K)), "b_theta": lu(0.1, 1e3, (30, K)),
              "a_beta": lu(0.05, 1e4, (20, K)), "b_beta": lu(0.1, 1e3, (20, K))}
        u, i = rng.integers(0, 30, 500), rng.integers(0, 20, 500)
        x = rng.choice([0.0, 1.0, 2.0, 3.5, 7.0, 40.0], 500)
        out = ref.predictive(st, u, i, x)
        assert (out["mu"] > ref.RATE_FLOOR).all()
        slack = 1e-12 * out["mag"][:, ref.PLUGIN]
        assert (out["logp"][:, ref.BOUND] <= out["logp"][:, ref.PLUGIN] + slack).all()
        assert (out["logp"][x > 0, ref.BOUND] < out["logp"][x > 0, ref.PLUGIN]).all()
        assert (out["lse"] <= np.log(out["mu"]) + 1e-12).all()


def test_negbin_tends_to_poisson_as_the_shapes_grow():
    """Shapes s with rates s / e (the means stay e): v ~ 1/s, so NEGBIN - Poisson ~ 1/s.  Monotonically closer at
    s = 1e3, 1e6, 1e9; and the literal formula in double is useless at the last (the reason for the stable form)."""
    rng = np.random.default_rng(5)
    K, n = 4, 60
    et, eb = rng.uniform(0.3, 2.0, (n, K)), rng.uniform(0.3, 2.0, (n, K))
    x = rng.choice([0.0, 1.0, 2.0, 3.5, 7.0, 40.0], n)
    gaps = []
    for s in (1e3, 1e6, 1e9):
        a, c = np.full((n, K), s), np.full((n, K), s)
        mu, v, _, _ = ref.moments(a, a / et, c, c / eb)
        nb, _ = ref.negbin(x, mu, v)
        po, _ = ref.poisson(x, mu)
        assert np.isfinite(nb).all()
        gaps.append(np.abs(nb - po))
    assert (gaps[1] < gaps[0]).all() and (gaps[2] < gaps[1]).all()
    assert gaps[2].max() < 1e-6 and gaps[0].max() > 1e-4
    naive = ref.negbin_literal_double(x, mu, v)
    # r ~ 3e8: the literal terms are of size r log r ~ 6e9, one ulp of which is 1e-6 -- more than the whole difference from
    # the Poisson term that the formula is there to compute
    assert np.abs(naive - nb).max() > gaps[2].max()
    # the figure quoted in the header's rationale: x = 3, mu = 2.5, r = 1e14
    lit = float(ref.negbin_literal_double(np.float64(3.0), np.float64(2.5), np.float64(6.25e-14)))
    val, _ = ref.negbin_one(3.0, 2.5, 6.25e-14)
    assert abs(val - (-1.54289)) < 1e-5 and abs(lit - val) > 0.05


def test_negbin_is_a_distribution_and_has_the_matched_moments():
    """Summed over the counts 0 .. 400 the reference's NEGBIN density is 1, its mean mu and its variance mu + v."""
    for mu, v in ((2.5, 1.7), (0.4, 0.01), (6.0, 30.0)):
        xs = np.arange(0.0, 400.0)
        lp, _ = ref.negbin(xs, np.full_like(xs, mu), np.full_like(xs, v))
        p = np.exp(lp)
        assert abs(p.sum() - 1.0) < 1e-9
        m = (p * xs).sum()
        assert abs(m - mu) < 1e-8 and abs((p * (xs - m) ** 2).sum() - (mu + v)) < 1e-6


def test_reference_plugin_is_the_host_metric_on_a_frame():
    """The reference's PLUGIN column summed = metrics.PoissonLogPredictiveLikelihood at E theta, E beta (clamp included:
    one item's factors are tiny enough for mu < 1e-10)."""
    from src.evaluation.metrics import PoissonLogPredictiveLikelihood
    rng = np.random.default_rng(9)
    K, nu, ni, n = 5, 12, 9, 200
    st = {"a_theta": rng.uniform(0.2, 5.0, (nu, K)), "b_theta": rng.uniform(0.5, 3.0, (nu, K)),
          "a_beta": rng.uniform(0.2, 5.0, (ni, K)), "b_beta": rng.uniform(0.5, 3.0, (ni, K))}
    st["b_beta"][4] = 1e12
    df = pd.DataFrame({"u": rng.integers(0, nu, n), "i": rng.integers(0, ni, n), "rating": rng.poisson(2.0, n).astype(float)})
    out = ref.predictive(st, df["u"].to_numpy(), df["i"].to_numpy(), df["rating"].to_numpy())
    assert (out["mu"] < ref.RATE_FLOOR).any()
    want = PoissonLogPredictiveLikelihood(df, st["a_theta"] / st["b_theta"], st["a_beta"] / st["b_beta"])
    got = math.fsum(out["logp"][:, ref.PLUGIN])
    assert abs(got - want) <= 1e-12 * math.fsum(out["mag"][:, ref.PLUGIN])
    # and the clamp is PLUGIN's alone
    tiny = out["mu"] < ref.RATE_FLOOR
    x = df["rating"].to_numpy()
    assert np.allclose(out["logp"][tiny, ref.PLUGIN], x[tiny] * np.log(1e-10) - 1e-10 - gammaln(x[tiny] + 1.0), rtol=1e-15)


# ---- binding ---------------------------------------------------------------------------------------------------------
def test_binding_constants_are_the_headers():
    import pmf_hip
    text = open(os.path.join(ROOT, "include", "pmf_hip.h")).read()
    defs = dict(re.findall(r"#define PMF_(GAMMA_PRED_[A-Z]+)\s+(\d+)", text))
    assert set(defs) == {"GAMMA_PRED_PLUGIN", "GAMMA_PRED_BOUND", "GAMMA_PRED_NEGBIN", "GAMMA_PRED_KINDS", "GAMMA_PRED_TOTALS"}
    for name, value in defs.items():
        assert getattr(pmf_hip, name) == int(value), name
    assert (ref.PLUGIN, ref.BOUND, ref.NEGBIN, ref.KINDS) == (pmf_hip.GAMMA_PRED_PLUGIN, pmf_hip.GAMMA_PRED_BOUND,
                                                             pmf_hip.GAMMA_PRED_NEGBIN, pmf_hip.GAMMA_PRED_KINDS)
    assert re.search(r"#define PMF_ABI_VERSION 3\b", text) and re.search(r"#define PMF_KERNEL_COUNT 13\b", text)
    assert pmf_hip.engine.GammaPredictive._fields == ("mean", "var", "logp", "totals")


# ---- the model classes' argument checks that need no device ----------------------------------------------------------
def _models():
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    return [HPF_CAVI(HPF_CAVI_Config(n_factors=3, max_iter=1, verbose=False)),
            PoissonMFCAVI(PoissonMFCAVIConfig(n_factors=3, max_iter=1, verbose=False))]


def _frame(ratings=(1.0, 2.0, 0.0)):
    return pd.DataFrame({"u": [0, 1, 2], "i": [0, 1, 1], "rating": list(ratings)})


@pytest.mark.parametrize("which", [0, 1])
def test_fit_refuses_bad_loglik_arguments_before_any_device_call(which):
    """No context is opened: the model is still unfitted afterwards (and the checks run on a machine without a GPU)."""
    model = _models()[which]
    train = _frame()
    with pytest.raises(ValueError, match="val_df"):
        model.fit(train, track_loglik=True)
    with pytest.raises(ValueError, match="val_df"):
        model.fit(train, loglik_tol=1e-3)
    with pytest.raises(ValueError, match="loglik_kind"):
        model.fit(train, _frame(), track_loglik=True, loglik_kind="poisson")
    with pytest.raises(ValueError, match="negative"):
        model.fit(train, _frame((1.0, -1.0, 2.0)), track_loglik=True)
    assert model._ctx is None and model.n_users is None


@pytest.mark.parametrize("which", [0, 1])
def test_log_predictive_density_checks_its_arguments_first(which):
    model = _models()[which]
    with pytest.raises(ValueError, match="kind"):
        model.log_predictive_density(_frame(), kind="gaussian")
    with pytest.raises(ValueError, match="negative"):
        model.log_predictive_density(_frame((1.0, 2.0, -0.5)))
    with pytest.raises(RuntimeError, match="not been fitted"):
        model.log_predictive_density(_frame())
    with pytest.raises(RuntimeError, match="not been fitted"):
        model.predict_variance([0], [0])


def test_the_extended_model_has_none_of_it():
    from src.models.poisson_mf_extended_cavi import PoissonMFExtendedCAVI
    assert not hasattr(PoissonMFExtendedCAVI, "predict_variance") and not hasattr(PoissonMFExtendedCAVI, "log_predictive_density")
