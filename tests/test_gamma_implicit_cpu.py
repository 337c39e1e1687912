"""Unlisted cells counted as zeros (PMF_ZEROS_OBSERVED, `fit(unobserved="zero")`), without a device: the identity the
feature rests on -- zero mode on a sparse rating list P equals the existing formulae on the same matrix with every
missing cell listed as an explicit 0 (D) -- shown with the dense float64 references, and the argument checks of `fit`
that need no GPU.

Tolerances: the two sides of the identity are the same real numbers summed in a different order in float64.  A rate is
a sum of at most 90 positive addends (1e-13 relative leaves three digits over 90 roundings of 1.1e-16); the bound is a
sum of 6300 cells and some thousand row terms with cancellation between the blocks: 1e-10 relative."""
import numpy as np
import pandas as pd
import pytest

import gamma_elbo_reference as ref
import gamma_implicit_reference as zref
from gamma_fold_in_reference import batch, fold_in_reference
from helpers import rel_err

U, I, N = 90, 70, 4000
K = 20
POISSON = ((0.3, 0.7), (0.3, 0.7))
HPF = ((0.3, 0.3, 1.0), (0.3, 0.3, 1.0))


@pytest.fixture(scope="module")
def problems():
    P = zref.problem_p(5, U, I, N)
    return P, zref.dense_completion(*P, U, I)


def test_problem_has_split_rows_and_empty_rows_on_both_sides(problems):
    (u, i, x), (du, di, dx) = problems
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    assert len(u) == 1984 and len(np.unique(u.astype(np.int64) * I + i)) == 1984
    assert nu.max() == 67 and ni.max() == 87 and (nu == 0).sum() == 3 and (ni == 0).sum() == 2
    assert (x == 0).sum() >= 1984 // 11
    assert len(du) == U * I and len(np.unique(du.astype(np.int64) * I + di)) == U * I
    assert np.array_equal(du[:1984], u) and np.array_equal(dx[:1984], x) and (dx[1984:] == 0).all()


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("hierarchical", [False, True])
def test_zero_mode_on_the_sparse_list_is_the_existing_update_on_the_dense_list(problems, hierarchical, exact):
    """15 iterations, every shape, rate and hyper rate after every half-step, and the bound after every iteration."""
    P, D = problems
    priors = HPF if hierarchical else POISSON
    st_p = st_d = ref.initial_state(3, U, I, K, priors, hierarchical)
    for it in range(15):
        for st_p, st_d in zip(zref.half_steps(st_p, *P, priors, hierarchical, exact), ref.half_steps(st_d, *D, priors, hierarchical, exact)):
            for key in st_p:
                assert rel_err(st_p[key], st_d[key]) <= 1e-13, (it, key)
        if hierarchical:
            got, want = zref.elbo_hpf(st_p, *P, *priors), ref.elbo_hpf(st_d, *D, *priors)
        else:
            got, want = zref.elbo_poisson(st_p, *P, *priors[0]), ref.elbo_poisson(st_d, *D, *priors[0])
        assert abs(got - want) <= 1e-10 * abs(want), (it, got, want)


@pytest.mark.parametrize("hierarchical", [False, True])
def test_data_term_by_rows_from_either_side(problems, hierarchical):
    """The per-row data terms of the two sides add up to the data block over all cells, which is the dense list's."""
    P, D = problems
    priors = HPF if hierarchical else POISSON
    st = ref.initial_state(4, U, I, K, priors, hierarchical)
    for st in zref.half_steps(st, *P, priors, hierarchical, True):
        pass
    want = ref.data_block(st, *D)
    assert abs(zref.data_block(st, *P) - want) <= 1e-10 * abs(want)
    for side in (0, 1):
        data, logfact, _, dot, count = zref.data_by_rows(st, side, *P)
        assert abs((data - logfact).sum() - want) <= 1e-10 * abs(want), side
        assert (data[count == 0] == -dot[count == 0]).all() and (dot > 0).all()


@pytest.mark.parametrize("hierarchical", [False, True])
def test_bound_does_not_fall_over_15_exact_iterations(problems, hierarchical):
    P, _ = problems
    priors = HPF if hierarchical else POISSON
    st = ref.initial_state(6, U, I, K, priors, hierarchical)
    bound = (lambda s: zref.elbo_hpf(s, *P, *priors)) if hierarchical else (lambda s: zref.elbo_poisson(s, *P, *priors[0]))
    trace = [bound(st)]
    for _ in range(15):
        for st in zref.half_steps(st, *P, priors, hierarchical, True):
            trace.append(bound(st))
    steps = np.diff(trace)
    assert (steps >= -1e-10 * np.abs(trace[:-1])).all(), steps.min()
    assert trace[-1] > trace[0]


@pytest.mark.parametrize("hierarchical", [False, True])
@pytest.mark.parametrize("n_iter", [1, 10])
def test_fold_in_is_the_existing_recursion_with_every_other_id_listed(hierarchical, n_iter):
    """Rows of 0 .. 40 distinct ids; the dense batch lists a row's ids, then every other id of the side with a 0."""
    rng = np.random.default_rng(8)
    n_other = 50
    E_other = rng.gamma(2.0, 0.3, size=(n_other, K))
    lengths = (0, 1, 7, 40)
    ids = np.concatenate([rng.permutation(n_other)[:n] for n in lengths]).astype(np.int32)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    x = rng.integers(0, 6, len(ids)).astype(np.float64)
    dense_ids, dense_x = [], []
    for r in range(len(lengths)):
        mine = ids[row_ptr[r]:row_ptr[r + 1]]
        rest = np.setdiff1d(np.arange(n_other), mine)
        dense_ids.append(np.concatenate([mine, rest]))
        dense_x.append(np.concatenate([x[row_ptr[r]:row_ptr[r + 1]], np.zeros(len(rest))]))
    dense_ptr = np.arange(len(lengths) + 1, dtype=np.int64) * n_other
    prior = (0.3, 0.0, True, 0.3 + K * 0.3, 1.0) if hierarchical else (0.3, 1.5, False, 0.0, 0.0)
    init = (rng.gamma(1.0, 0.3, size=(len(lengths), K)), rng.gamma(2.0, 0.5, size=len(lengths)) if hierarchical else None)
    for start in ((None, None), init):
        got = zref.fold_in(E_other, row_ptr, ids, x, *prior, n_iter=n_iter, init_factor=start[0], init_prior_rate=start[1])
        want = fold_in_reference(E_other, dense_ptr, np.concatenate(dense_ids), np.concatenate(dense_x), *prior, n_iter=n_iter,
                                 init_factor=start[0], init_prior_rate=start[1])
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert rel_err(g, w) <= 1e-13


def test_the_shared_fold_in_batch_has_a_long_row():
    row_ptr, ids, x = batch(7, I)
    assert np.diff(row_ptr).max() == 700 and np.diff(row_ptr).min() == 0


# ---- fit(unobserved=...): what is refused before any device call ----------------------------------------------------
def _models():
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    return (HPF_CAVI(HPF_CAVI_Config(n_factors=4, max_iter=1, verbose=False)),
            PoissonMFCAVI(PoissonMFCAVIConfig(n_factors=4, max_iter=1, verbose=False)))


def _frame(ratings=(1.0, 2.0, 0.0), pairs=((0, 0), (1, 2), (2, 1))):
    return pd.DataFrame({"u": [p[0] for p in pairs], "i": [p[1] for p in pairs], "rating": list(ratings)})


def test_fit_refuses_an_unknown_value():
    for model in _models():
        with pytest.raises(ValueError, match="unobserved must be 'missing' or 'zero'"):
            model.fit(_frame(), unobserved="zeros")


def test_zero_mode_refuses_a_negative_rating():
    for model in _models():
        with pytest.raises(ValueError, match="unobserved='zero'.*negative"):
            model.fit(_frame(ratings=(1.0, -1.0, 2.0)), unobserved="zero")


def test_zero_mode_refuses_duplicate_pairs():
    for model in _models():
        with pytest.raises(ValueError, match="unobserved='zero'.*more than once"):
            model.fit(_frame(pairs=((0, 0), (1, 2), (0, 0))), unobserved="zero")


def test_zero_mode_refuses_a_communicator():
    class TwoRanks:
        world, rank = 2, 0

    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    model = HPF_CAVI(HPF_CAVI_Config(n_factors=4, max_iter=1, verbose=False), comm=TwoRanks())
    with pytest.raises(ValueError, match="unobserved='zero'.*several ranks"):
        model.fit(_frame(), unobserved="zero")


def test_the_extended_model_has_no_such_keyword():
    import inspect
    from src.models.poisson_mf_extended_cavi import PoissonMFExtendedCAVI
    assert "unobserved" not in inspect.signature(PoissonMFExtendedCAVI.fit).parameters
