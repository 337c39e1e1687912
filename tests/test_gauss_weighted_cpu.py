"""Per-rating confidence weights of the Gaussian CAVI models (`pmf_ctx_set_ratings_weighted`, `fit(weights=)`), without a
device: the identities the feature rests on, shown with the dense float64 reference (tests/gauss_weighted_reference.py),
`elbo_from_terms` with and without the new keywords, and the refusals of the model classes that need no GPU.

Tolerances.  An integer weight c is c copies of the rating: the weighted reference and the oracle on the replicated
frame are the same real numbers summed in another order in float64 -- the project's f64 bar, 1e-10 (absolute on means
and biases, which are O(1); relative to the row's largest entry on covariances).  The two routes to the bound differ by
summation order over 4000 ratings and 160 rows: 1e-12 relative.  Exact coordinate ascent never lowers the bound; a step
may fall by rounding, at most 1e-9 |L| (the bar tests/test_gauss_implicit_gpu.py uses for the device's trace).

What touches project code.  Only the `elbo_from_terms` tests and the `fit(weights=)` / `fold_in_users(weights=)` refusal
tests call the project; they fail without the feature.  The other tests validate the reference itself (against the
oracle on replicated ratings, against its own second route to the bound, and by the ascent of the bound), so that the
device tests of tests/test_gauss_weighted_gpu.py compare against something that has been checked; they say nothing
about the feature and pass without it."""
import numpy as np
import pandas as pd
import pytest

import gauss_weighted_reference as wref
from helpers import max_abs
from oracle import cavi_oracle as orc

U, I, N, K = 90, 70, 4000, 6
SIGMA2, ETA_T, ETA_B, ETA_BIAS = 0.3, 0.5, 0.7, 1.0


@pytest.fixture(scope="module")
def problem():
    return wref.problem(11, U, I, N)


def _oracle_state(st, bias):
    out = {k: st[k].copy() for k in ("m_theta", "V_theta", "m_beta", "V_beta")}
    if bias:
        out["m_user_bias"], out["m_item_bias"] = st["b_user"].copy(), st["b_item"].copy()
    return out


@pytest.mark.parametrize("bias", [False, True])
def test_integer_weights_equal_the_oracle_on_the_replicated_frame(problem, bias):
    u, i, x, _ = problem
    c = np.random.default_rng(2).integers(1, 5, len(u)).astype(np.float64)
    rep = c.astype(np.int64)
    ru, ri, rx = np.repeat(u, rep), np.repeat(i, rep), np.repeat(x, rep)
    idx = (orc.group_positions(ru, U), orc.group_positions(ri, I))
    st = wref.initial_state(3, U, I, K, bias)
    ost = _oracle_state(st, bias)
    eb = ETA_BIAS if bias else None
    for it in range(2):
        st = wref.iterate(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, eb)
        ost = orc.gaussian_iteration(ost, idx, ru, ri, rx, SIGMA2, ETA_T, ETA_B, eb)
        for key in ("m_theta", "m_beta"):
            assert max_abs(st[key], ost[key]) <= 1e-10, (it, key)
        for key in ("V_theta", "V_beta"):
            scale = np.abs(ost[key]).max(axis=(1, 2), keepdims=True)
            assert np.max(np.abs(st[key] - ost[key]) / scale) <= 1e-10, (it, key)
        if bias:
            assert max_abs(st["b_user"], ost["m_user_bias"]) <= 1e-10 and max_abs(st["b_item"], ost["m_item_bias"]) <= 1e-10
    assert np.array_equal(wref.weight_sums(u, c, U), np.bincount(ru, minlength=U))


@pytest.mark.parametrize("bias", [False, True])
def test_the_two_routes_to_the_bound_agree(problem, bias):
    u, i, x, c = problem
    eb = ETA_BIAS if bias else None
    st = wref.iterate(wref.initial_state(4, U, I, K, bias), u, i, x, c, SIGMA2, ETA_T, ETA_B, eb)
    want = wref.elbo_ratings(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, eb)
    for side in (0, 1):
        got = wref.elbo_rows(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, eb, side=side)
        assert abs(got - want) <= 1e-12 * abs(want), (side, got, want)


def test_the_two_routes_agree_in_zero_mode():
    u, i, x, c = wref.problem(12, 40, 30, 500, unique=True)
    st = wref.iterate(wref.initial_state(4, 40, 30, K), u, i, x, c, SIGMA2, ETA_T, ETA_B, None, w0=0.2)
    want = wref.elbo_ratings(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, None, w0=0.2)
    got = wref.elbo_rows(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, None, w0=0.2)
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_zero_mode_with_weight_one_is_the_default_weighted_fit_of_the_dense_completion():
    Uz, Iz = 40, 30
    u, i, x, c = wref.problem(12, Uz, Iz, 500, unique=True)
    D = wref.dense_completion(u, i, x, c, Uz, Iz)
    st_p = st_d = wref.initial_state(5, Uz, Iz, K)
    for it in range(2):
        for st_p, st_d in zip(wref.half_steps(st_p, u, i, x, c, SIGMA2, ETA_T, ETA_B, None, w0=1.0),
                              wref.half_steps(st_d, *D, SIGMA2, ETA_T, ETA_B, None)):
            for key in st_p:
                assert max_abs(st_p[key], st_d[key]) <= 1e-12, (it, key)


@pytest.mark.parametrize("bias,w0", [(False, None), (True, None), (False, 0.25)])
def test_bound_never_falls_over_alternating_weighted_half_sweeps(bias, w0):
    """A wrong weight anywhere in an update or in the bound breaks the ascent."""
    Uz, Iz = 40, 30
    u, i, x, c = wref.problem(13, Uz, Iz, 500, unique=True)
    eb = ETA_BIAS if bias else None
    st = wref.initial_state(6, Uz, Iz, K)   # (biases from 0, as the models start)
    trace = [wref.elbo_rows(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, eb, w0)]
    for _ in range(4):
        for st in wref.half_steps(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, eb, w0):
            trace.append(wref.elbo_rows(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, eb, w0))
    steps = np.diff(trace)
    assert (steps >= -1e-9 * np.abs(trace[:-1])).all(), steps.min()
    assert trace[-1] > trace[0]
    # the same updates scored with the unweighted bound are no ascent: the test can fail
    flat = [wref.elbo_rows(s, u, i, x, np.ones_like(c), SIGMA2, ETA_T, ETA_B, eb, w0)
            for s in wref.half_steps(st, u, i, x, 4.0 * c, SIGMA2, ETA_T, ETA_B, eb, w0)]
    assert flat[0] < wref.elbo_rows(st, u, i, x, np.ones_like(c), SIGMA2, ETA_T, ETA_B, eb, w0)


def test_fold_in_recursion_is_the_half_sweeps_of_a_new_row(problem):
    """one fold-in iteration of a user = that user's factor then bias update from a zero bias against the frozen items"""
    u, i, x, c = problem
    st = wref.iterate(wref.initial_state(7, U, I, K, True), u, i, x, c, SIGMA2, ETA_T, ETA_B, ETA_BIAS)
    sel = np.flatnonzero(u == 5)
    m, V, b = wref.fold_in(st["m_beta"], st["V_beta"], st["b_item"], np.array([0, len(sel)]), i[sel], x[sel], c[sel],
                           SIGMA2, ETA_T, ETA_BIAS, n_iter=1)
    zero = np.zeros(1)
    ids = np.zeros(len(sel), dtype=np.int64)
    m1, V1 = wref.factor_sweep(np.zeros((1, K)), np.zeros((1, K, K)), st["m_beta"], st["V_beta"], zero, st["b_item"], ids,
                               i[sel], x[sel], c[sel], SIGMA2, ETA_T)
    b1 = wref.bias_sweep(zero, st["b_item"], m1, st["m_beta"], ids, i[sel], x[sel], c[sel], SIGMA2, ETA_BIAS)
    assert max_abs(m, m1) <= 1e-12 and max_abs(V, V1) <= 1e-12 and max_abs(b, b1) <= 1e-12


# ---- elbo_from_terms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
def test_elbo_from_terms_with_the_weight_keywords_against_the_rating_by_rating_bound(problem, bias):
    from src.models._gaussian_host import elbo_from_terms
    u, i, x, c = problem
    eb = ETA_BIAS if bias else None
    st = wref.iterate(wref.initial_state(8, U, I, K, bias), u, i, x, c, SIGMA2, ETA_T, ETA_B, eb)
    user, _ = wref.side_terms(st["m_theta"], st["V_theta"], st["b_user"], st["m_beta"], st["V_beta"], st["b_item"], u, i, x, c)
    item, _ = wref.side_terms(st["m_beta"], st["V_beta"], st["b_item"], st["m_theta"], st["V_theta"], st["b_user"], i, u, x, c)
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    want = wref.elbo_ratings(st, u, i, x, c, SIGMA2, ETA_T, ETA_B, eb)
    kw = dict(user_weight_sums=wref.weight_sums(u, c, U), item_weight_sums=wref.weight_sums(i, c, I),
              log_weight_sum=float(np.log(c).sum()))
    for data_side in (0, 1):
        got, parts = elbo_from_terms(user.sum(axis=0), item.sum(axis=0), nu, ni, len(x), K, SIGMA2, ETA_T, ETA_B, eb,
                                     data_side=data_side, **kw)
        assert abs(got - want) <= 1e-12 * abs(want), (data_side, got, want)
        assert abs(sum(parts.values()) - got) <= 1e-12 * abs(got)
    with pytest.raises(ValueError, match="go together"):
        elbo_from_terms(user.sum(axis=0), item.sum(axis=0), nu, ni, len(x), K, SIGMA2, ETA_T, ETA_B, eb, log_weight_sum=0.0)


@pytest.mark.parametrize("bias", [False, True])
def test_elbo_from_terms_without_the_keywords_is_what_it_was(problem, bias):
    """against tests/elbo_reference.py (the unweighted bound, untouched), on unweighted terms; and keywords that say
    'every weight is 1' change nothing but rounding-free zeros"""
    import elbo_reference as dref
    from src.models._gaussian_host import elbo_from_terms
    u, i, x, _ = problem
    one = np.ones(len(x))
    eb = ETA_BIAS if bias else None
    st = wref.iterate(wref.initial_state(9, U, I, K, bias), u, i, x, one, SIGMA2, ETA_T, ETA_B, eb)
    ost = _oracle_state(st, True)
    user, _ = dref.side_terms(st["m_theta"], st["V_theta"], st["b_user"], st["m_beta"], st["V_beta"], st["b_item"], u, i, x)
    item, _ = dref.side_terms(st["m_beta"], st["V_beta"], st["b_item"], st["m_theta"], st["V_theta"], st["b_user"], i, u, x)
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    want = dref.elbo(ost, u, i, x, SIGMA2, ETA_T, ETA_B, eb)
    got, parts = elbo_from_terms(user.sum(axis=0), item.sum(axis=0), nu, ni, len(x), K, SIGMA2, ETA_T, ETA_B, eb)
    assert abs(got - want) <= 1e-12 * abs(want)
    same, parts1 = elbo_from_terms(user.sum(axis=0), item.sum(axis=0), nu, ni, len(x), K, SIGMA2, ETA_T, ETA_B, eb,
                                   user_weight_sums=nu, item_weight_sums=ni, log_weight_sum=0.0)
    assert same == got and parts1 == parts


# ---- fit(weights=): what is refused before any device call ------------------------------------------------------------
def _model(**kw):
    from src.models.gaussian_mf_cavi import GaussianMFCAVI, GaussianMFCAVIConfig
    return GaussianMFCAVI(GaussianMFCAVIConfig(n_factors=4, max_iter=1, verbose=False), **kw)


def _frame():
    return pd.DataFrame({"u": [0, 1, 2], "i": [0, 2, 1], "rating": [1.0, -2.0, 0.0], "conf": [1.0, 2.0, 0.5]})


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_fit_refuses_a_weight_that_is_not_finite_and_positive(bad):
    with pytest.raises(ValueError, match=r"weights must be finite and > 0.*position 1"):
        _model().fit(_frame(), weights=[1.0, bad, 2.0])
    frame = _frame()
    frame.loc[1, "conf"] = bad
    with pytest.raises(ValueError, match=r"weights must be finite and > 0.*position 1"):
        _model().fit(frame, weights="conf")


def test_fit_refuses_a_wrong_length_and_an_unknown_column():
    with pytest.raises(ValueError, match="one entry per row"):
        _model().fit(_frame(), weights=[1.0, 2.0])
    with pytest.raises(KeyError):
        _model().fit(_frame(), weights="no_such_column")


def test_fit_refuses_weights_with_a_communicator():
    class TwoRanks:
        world, rank = 2, 0

    with pytest.raises(ValueError, match="weights with comm=.*several ranks"):
        _model(comm=TwoRanks()).fit(_frame(), weights="conf")


def test_the_gradient_class_refuses_weights():
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    with pytest.raises(NotImplementedError, match="gradient mode"):
        GaussianMFSGD(GaussianMFSGDConfig(n_factors=4, verbose=False)).fit(_frame(), weights="conf")


def test_fold_in_checks_its_weights_before_the_context():
    with pytest.raises(ValueError, match=r"weights must be finite and > 0.*position 2"):
        _model().fold_in_users(_frame(), weights=[1.0, 1.0, -3.0])
