"""Unlisted cells as weighted zeros in the bias-free Gaussian model (PMF_ZEROS_OBSERVED of pmf_ctx_set_gauss_zeros,
`fit(unobserved="zero", zero_weight=)`), without a device: the identities the feature rests on, shown with the dense
float64 reference (tests/gauss_implicit_reference.py), `elbo_from_terms(..., zero_weight=)` against the bound written
cell by cell, and the argument checks of `fit` that need no GPU.

Tolerances: both sides of every identity are the same real numbers summed in a different order in float64, through
K x K inverses whose condition numbers stay below a few hundred on this problem: 1e-12 on the arrays (absolute, entries
are O(1)) and 1e-12 relative on the bound, a sum of 6300 cells and 160 row terms."""
import numpy as np
import pandas as pd
import pytest

import gauss_implicit_reference as zref
from helpers import max_abs

U, I, N, K = 90, 70, 4000, 6
SIGMA2, ETA_T, ETA_B = 1.0, 1.0, 1.0
WEIGHTS = (1.0, 0.1, 0.025)


@pytest.fixture(scope="module")
def problems():
    P = zref.problem_p(5, U, I, N)
    return P, zref.dense_completion(*P, U, I)


def test_problem_has_long_rows_empty_rows_and_negative_ratings(problems):
    (u, i, x), (du, di, dx) = problems
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    assert len(u) == 1984 and len(np.unique(u * I + i)) == 1984
    assert nu.max() == 67 and ni.max() == 87 and (nu == 0).sum() == 3 and (ni == 0).sum() == 2
    assert (x < 0).any() and (x == 0).any() and (x > 0).any()
    assert len(du) == U * I and len(np.unique(du * I + di)) == U * I
    assert np.array_equal(du[:1984], u) and np.array_equal(dx[:1984], x) and (dx[1984:] == 0).all()


def test_zero_mode_with_weight_one_is_the_default_update_on_the_dense_list(problems):
    """Four iterations, every array after every half-sweep, and the bound after every iteration: the zero-mode bound of
    P (from rows) against the default bound of D, which is tests/elbo_reference.py's."""
    import elbo_reference as dref
    P, D = problems
    st_p = st_d = zref.initial_state(3, U, I, K)
    for it in range(4):
        for st_p, st_d in zip(zref.half_steps(st_p, *P, SIGMA2, ETA_T, ETA_B, 1.0), zref.half_steps(st_d, *D, SIGMA2, ETA_T, ETA_B, None)):
            for key in st_p:
                assert max_abs(st_p[key], st_d[key]) <= 1e-12, (it, key)
        got = zref.elbo_rows(st_p, *P, SIGMA2, ETA_T, ETA_B, 1.0)
        want = dref.elbo(st_d, *D, SIGMA2, ETA_T, ETA_B, data="ratings")
        assert abs(got - want) <= 1e-12 * abs(want), (it, got, want)


@pytest.mark.parametrize("w0", WEIGHTS)
def test_bound_from_rows_of_either_side_is_the_bound_from_cells(problems, w0):
    P, _ = problems
    st = zref.initial_state(4, U, I, K)
    for st in zref.half_steps(st, *P, 0.3, 0.5, 0.7, w0):
        pass
    want = zref.elbo_cells(st, *P, 0.3, 0.5, 0.7, w0)
    for side in (0, 1):
        got = zref.elbo_rows(st, *P, 0.3, 0.5, 0.7, w0, side=side)
        assert abs(got - want) <= 1e-12 * abs(want), (side, got, want)


@pytest.mark.parametrize("w0", WEIGHTS)
def test_bound_never_falls_over_8_iterations(problems, w0):
    """The updates are exact coordinate ascent on the bound: it rises at every half-sweep (rounding aside)."""
    P, _ = problems
    st = zref.initial_state(6, U, I, K)
    trace = [zref.elbo_rows(st, *P, SIGMA2, ETA_T, ETA_B, w0)]
    for _ in range(8):
        for st in zref.half_steps(st, *P, SIGMA2, ETA_T, ETA_B, w0):
            trace.append(zref.elbo_rows(st, *P, SIGMA2, ETA_T, ETA_B, w0))
    steps = np.diff(trace)
    assert (steps >= -1e-12 * np.abs(trace[:-1])).all(), steps.min()
    assert trace[-1] > trace[0]


def test_rows_without_ratings_get_mean_zero_and_the_gram_covariance(problems):
    (u, i, x), _ = problems
    st = zref.initial_state(8, U, I, K)
    m, V = zref.half_sweep(st["m_beta"], st["V_beta"], u, i, x, U, 0.3, 0.5, 0.25)
    G, _ = zref.gram(st["m_beta"], st["V_beta"])
    empty = np.flatnonzero(np.bincount(u, minlength=U) == 0)
    assert len(empty) == 3
    for r in empty:
        assert (m[r] == 0.0).all()
        assert max_abs(V[r], np.linalg.inv(np.eye(K) / 0.5 + 0.25 * G / 0.3)) <= 1e-12


@pytest.mark.parametrize("w0", WEIGHTS)
def test_elbo_from_terms_with_zero_weight_against_the_cell_by_cell_bound(problems, w0):
    from src.models._gaussian_host import elbo_from_terms
    (u, i, x), _ = problems
    st = zref.initial_state(9, U, I, K)
    for st in zref.half_steps(st, u, i, x, 0.3, 0.5, 0.7, w0):
        pass
    user, _ = zref.side_terms(st["m_theta"], st["V_theta"], st["m_beta"], st["V_beta"], u, i, x, w0)
    item, _ = zref.side_terms(st["m_beta"], st["V_beta"], st["m_theta"], st["V_theta"], i, u, x, w0)
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    want = zref.elbo_cells(st, u, i, x, 0.3, 0.5, 0.7, w0)
    for data_side in (0, 1):
        got, parts = elbo_from_terms(user.sum(axis=0), item.sum(axis=0), nu, ni, len(x), K, 0.3, 0.5, 0.7, data_side=data_side,
                                     zero_weight=w0)
        assert abs(got - want) <= 1e-12 * abs(want), (data_side, got, want)
        assert abs(sum(parts.values()) - got) <= 1e-12 * abs(got)
    # without the keyword the constant is the listed ratings' alone
    plain = elbo_from_terms(user.sum(axis=0), item.sum(axis=0), nu, ni, len(x), K, 0.3, 0.5, 0.7)[0]
    assert abs((plain - got) - 0.5 * (U * I - len(x)) * np.log(2 * np.pi * 0.3 / w0)) <= 1e-9
    with pytest.raises(ValueError, match="bias-free"):
        elbo_from_terms(user.sum(axis=0), item.sum(axis=0), nu, ni, len(x), K, 0.3, 0.5, 0.7, eta_bias2=1.0, zero_weight=w0)


# ---- fit(unobserved=, zero_weight=): what is refused before any device call -----------------------------------------
def _model(**kw):
    from src.models.gaussian_mf_cavi import GaussianMFCAVI, GaussianMFCAVIConfig
    return GaussianMFCAVI(GaussianMFCAVIConfig(n_factors=4, max_iter=1, verbose=False), **kw)


def _frame(ratings=(1.0, -2.0, 0.0), pairs=((0, 0), (1, 2), (2, 1))):
    return pd.DataFrame({"u": [p[0] for p in pairs], "i": [p[1] for p in pairs], "rating": list(ratings)})


def test_fit_refuses_an_unknown_value():
    with pytest.raises(ValueError, match="unobserved must be 'missing' or 'zero'"):
        _model().fit(_frame(), unobserved="zeros")


@pytest.mark.parametrize("weight", [0.0, -0.5, 1.5, float("nan"), float("inf")])
def test_zero_mode_refuses_a_weight_outside_the_unit_interval(weight):
    with pytest.raises(ValueError, match="zero_weight must lie in"):
        _model().fit(_frame(), unobserved="zero", zero_weight=weight)


def test_zero_mode_refuses_duplicate_pairs():
    with pytest.raises(ValueError, match="unobserved='zero'.*more than once"):
        _model().fit(_frame(pairs=((0, 0), (1, 2), (0, 0))), unobserved="zero")


def test_zero_mode_refuses_a_communicator():
    class TwoRanks:
        world, rank = 2, 0

    with pytest.raises(ValueError, match="unobserved='zero'.*several ranks"):
        _model(comm=TwoRanks()).fit(_frame(), unobserved="zero")


def test_the_bias_model_and_the_gradient_mode_say_which_class_supports_it():
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI as WithBias, GaussianMFCAVIConfig as BiasConfig
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    for model in (WithBias(BiasConfig(n_factors=4, max_iter=1, verbose=False)),
                  GaussianMFSGD(GaussianMFSGDConfig(n_factors=4, verbose=False))):
        with pytest.raises(NotImplementedError, match=r"gaussian_mf_cavi\.GaussianMFCAVI"):
            model.fit(_frame(), unobserved="zero")
        with pytest.raises(ValueError, match="unobserved must be"):
            model.fit(_frame(), unobserved="nothing")
