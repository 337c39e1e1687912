"""What the Poisson MF / HPF ELBO surface (`pmf_gamma_elbo_terms`, `Context.gamma_elbo_terms`, `elbo_from_gamma_terms`,
`elbo`, `fit(track_elbo=)`) promises without a GPU: the binding, the null-context error, the model classes' refusals, and
the bound itself -- written out densely in float64 (tests/gamma_elbo_reference.py) it rises at every half-step of EXACT
coordinate ascent (the xi / eta steps of HPF included), no auxiliary multinomial beats the optimal one, the data term
comes out the same rating by rating, by user rows and by item rows, and `elbo_from_gamma_terms` fed the reference's
per-row sums equals the block-by-block bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gamma_elbo_reference as ref
from helpers import skewed_problem

PMF_EINVAL = -1                                   # include/pmf_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I, N, K = 37, 29, 1500, 5
ITERATIONS = 15
POISSON = ((0.3, 1.0), (0.3, 1.0))
HPF = ((0.3, 0.3, 1.0), (0.4, 0.5, 1.5))          # (a, a', b'), (c, c', d')
MODELS = {"poisson": (POISSON, False), "hpf": (HPF, True)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import pmf_hip
    return pmf_hip.load()


def test_header_prototype_equals_the_binding_and_the_symbol_is_exported_by_both_libraries(lib):
    import pmf_hip
    header = open(os.path.join(ROOT, "include", "pmf_hip.h")).read()
    proto = re.search(r"\nint pmf_gamma_elbo_terms\((.*?)\);", header, re.S)
    assert proto, "include/pmf_hip.h does not declare pmf_gamma_elbo_terms"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",")]
    ctype = {"pmf_ctx *": C.c_void_p, "int": C.c_int, "double *": C.POINTER(C.c_double)}
    want = [ctype[re.sub(r"\w+$", "", a).strip()] for a in args]
    assert len(want) == 6
    res, got = pmf_hip.SIGNATURES["pmf_gamma_elbo_terms"]
    assert res is C.c_int and got == want
    assert lib.pmf_gamma_elbo_terms.argtypes == want
    names = ("SUM_FACTOR", "SUM_ELOG", "ENTROPY", "LOG_HYPER", "INV_HYPER", "FACTOR_OVER_HYPER", "DATA", "LOGFACT", "TERMS")
    for value, name in enumerate(names):
        assert re.search(r"#define PMF_GAMMA_ELBO_%s %d\b" % (name, value), header)
        assert getattr(pmf_hip, "GAMMA_ELBO_" + name) == value
        assert getattr(ref, name) == value
    assert re.search(r"#define PMF_ABI_VERSION 3\b", header)
    assert callable(pmf_hip.Context.gamma_elbo_terms)
    for path in (pmf_hip.LIB_PATH, pmf_hip.TEST_LIB_PATH):
        assert hasattr(C.CDLL(path), "pmf_gamma_elbo_terms"), path


def test_no_kernel_class_is_added():
    import pmf_hip
    header = open(os.path.join(ROOT, "include", "pmf_hip.h")).read()
    assert len(pmf_hip.KERNEL_NAMES) == 13 and re.search(r"#define PMF_KERNEL_COUNT 13\b", header)


def test_null_context_is_einval_and_writes_nothing(lib):
    totals = (C.c_double * 8)(*[7.0] * 8)
    rows = (C.c_double * 16)(*[7.0] * 16)
    for with_data in (0, 1):
        for hierarchical in (0, 1):
            assert lib.pmf_gamma_elbo_terms(None, 0, with_data, hierarchical, totals, rows) == PMF_EINVAL
            assert lib.pmf_last_error().startswith(b"pmf_gamma_elbo_terms: null context")
    assert lib.pmf_gamma_elbo_terms(None, 5, 0, 0, None, None) == PMF_EINVAL
    assert lib.pmf_last_error().startswith(b"pmf_gamma_elbo_terms: null context")
    assert list(totals) == [7.0] * 8 and list(rows) == [7.0] * 16


# ---- the bound --------------------------------------------------------------------------------------------------------
def _problem():
    u, i, x = skewed_problem(K, U, I, N, "count")
    return u, i, x


def _bound(model, st, u, i, x, phi=None):
    priors, hierarchical = MODELS[model]
    return ref.elbo_hpf(st, u, i, x, *priors, phi=phi) if hierarchical else ref.elbo_poisson(st, u, i, x, *priors[0], phi=phi)


def _trajectory(model, exact):
    """Every state of ITERATIONS iterations, half-step by half-step, the initial state first."""
    priors, hierarchical = MODELS[model]
    u, i, x = _problem()
    st = ref.initial_state(11, U, I, K, priors, hierarchical)
    states = [st]
    for _ in range(ITERATIONS):
        for st in ref.half_steps(st, u, i, x, priors, hierarchical, exact):
            states.append(st)
    return (u, i, x), states


@pytest.mark.parametrize("model", ["poisson", "hpf"])
def test_bound_rises_at_every_half_step_of_exact_coordinate_ascent(model):
    (u, i, x), states = _trajectory(model, exact=True)
    assert len(states) == 1 + ITERATIONS * (4 if model == "hpf" else 2)
    values = np.array([_bound(model, st, u, i, x) for st in states])
    steps = np.diff(values)
    _, reference_style = _trajectory(model, exact=False)
    print(f"{model}: exact updates {values[0]:.1f} -> {values[-1]:.1f}, smallest step {steps.min():.3g}; the reference's "
          f"updates end at {_bound(model, reference_style[-1], u, i, x):.1f}")
    assert (steps > 0).all(), steps


@pytest.mark.parametrize("model", ["poisson", "hpf"])
def test_no_auxiliary_multinomial_beats_the_optimal_one(model):
    (u, i, x), states = _trajectory(model, exact=False)
    rng = np.random.default_rng(3)
    for st in (states[0], states[len(states) // 2], states[-1]):
        best = _bound(model, st, u, i, x)
        s = ref.expectations(st["a_theta"], st["b_theta"])[1][u] + ref.expectations(st["a_beta"], st["b_beta"])[1][i]
        optimal = np.exp(s - s.max(axis=1)[:, None])
        optimal /= optimal.sum(axis=1)[:, None]
        assert np.isclose(_bound(model, st, u, i, x, phi=optimal), best, rtol=1e-12, atol=0)
        for _ in range(5):
            phi = rng.dirichlet(np.full(K, rng.choice([0.2, 1.0, 5.0])), size=len(x))
            phi = np.maximum(phi, 1e-300)
            assert _bound(model, st, u, i, x, phi=phi) <= best


@pytest.mark.parametrize("model", ["poisson", "hpf"])
def test_three_data_routes_agree_and_the_assembly_equals_the_block_by_block_bound(model):
    from src.models._gamma_elbo import elbo_from_gamma_terms
    from pmf_hip import ITEM, USER
    priors, hierarchical = MODELS[model]
    (u, i, x), states = _trajectory(model, exact=False)
    for st in states[::7]:
        per_rating = ref.data_per_rating(st, u, i, x).sum() - ref.gammaln(x + 1.0).sum()
        user = ref.side_terms(st, 0, u, i, x, hierarchical)[0].sum(axis=0)
        item = ref.side_terms(st, 1, u, i, x, hierarchical)[0].sum(axis=0)
        by_user, by_item = user[ref.DATA] - user[ref.LOGFACT], item[ref.DATA] - item[ref.LOGFACT]
        assert np.isclose(by_user, per_rating, rtol=1e-12, atol=0)
        assert np.isclose(by_item, per_rating, rtol=1e-12, atol=0)
        assert np.isclose(by_user, by_item, rtol=1e-12, atol=0)
        want = _bound(model, st, u, i, x)
        L, parts = elbo_from_gamma_terms(user, item, U, I, K, *priors, hierarchical=hierarchical)
        L_item, _ = elbo_from_gamma_terms(user, item, U, I, K, *priors, hierarchical=hierarchical, data_side=ITEM)
        assert L == elbo_from_gamma_terms(user, item, U, I, K, *priors, hierarchical=hierarchical, data_side=USER)[0]
        assert np.isclose(L, want, rtol=1e-12, atol=0)
        assert np.isclose(L_item, want, rtol=1e-12, atol=0)
        assert np.isclose(sum(parts.values()), L, rtol=1e-15, atol=0)
        assert set(parts) == {"data", "prior_theta", "entropy_theta", "prior_beta", "entropy_beta"} | (
            {"prior_xi", "entropy_xi", "prior_eta", "entropy_eta"} if hierarchical else set())
        # a side without data leaves the two data columns to the other
        no_data = ref.side_terms(st, 1, u, i, x, hierarchical, with_data=False)[0].sum(axis=0)
        assert no_data[ref.DATA] == 0 and no_data[ref.LOGFACT] == 0
        assert elbo_from_gamma_terms(user, no_data, U, I, K, *priors, hierarchical=hierarchical)[0] == L


# ---- refusals of the model classes, before any device call -----------------------------------------------------------
def _frame(ratings=(1.0, 2.0)):
    import pandas as pd
    return pd.DataFrame({"u": [0, 1], "i": [0, 1], "rating": list(ratings)})


def _models():
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    return ((PoissonMFCAVI, PoissonMFCAVIConfig), (HPF_CAVI, HPF_CAVI_Config))


@pytest.mark.parametrize("which", [0, 1], ids=["poisson", "hpf"])
def test_unfitted_model_says_so_and_fit_takes_the_arguments_by_keyword_only(which):
    import inspect
    cls, cfg = _models()[which]
    model = cls(cfg(n_factors=4, verbose=False))
    with pytest.raises(RuntimeError, match="has not been fitted"):
        model.elbo()
    params = inspect.signature(model.fit).parameters
    assert params["track_elbo"].kind is inspect.Parameter.KEYWORD_ONLY and params["track_elbo"].default is False
    assert params["elbo_tol"].kind is inspect.Parameter.KEYWORD_ONLY and params["elbo_tol"].default is None


@pytest.mark.parametrize("which", [0, 1], ids=["poisson", "hpf"])
def test_sharded_fit_and_negative_ratings_are_refused(which):
    cls, cfg = _models()[which]
    model = cls(cfg(n_factors=4, verbose=False))
    model._ctx, model._shard_ctx = object(), object()
    try:
        with pytest.raises(NotImplementedError, match="elbo after a sharded fit"):
            model.elbo()
    finally:
        model._ctx = model._shard_ctx = None

    class World:          # what DeviceModel looks at of a communicator
        world, rank = 2, 0
    sharded = cls(cfg(n_factors=4, verbose=False), comm=World())
    with pytest.raises(NotImplementedError, match="communicator"):
        sharded.fit(_frame(), track_elbo=True)
    with pytest.raises(NotImplementedError, match="communicator"):
        sharded.fit(_frame(), elbo_tol=1e-3)
    for kwargs in ({"track_elbo": True}, {"elbo_tol": 1e-3}):
        with pytest.raises(ValueError, match="negative"):
            model.fit(_frame((1.0, -2.0)), **kwargs)
    assert model._ctx is None        # refused before a context was opened


def test_extended_model_has_no_elbo():
    from src.models.poisson_mf_extended_cavi import PoissonMFExtendedCAVI, PoissonMFExtendedCAVIConfig
    model = PoissonMFExtendedCAVI(PoissonMFExtendedCAVIConfig(n_factors=4, verbose=False))
    with pytest.raises(NotImplementedError, match="PoissonMFExtendedCAVI"):
        model.elbo()
    with pytest.raises(NotImplementedError, match="PoissonMFExtendedCAVI"):
        model.fit(_frame(), track_elbo=True)
    with pytest.raises(NotImplementedError, match="PoissonMFExtendedCAVI"):
        model.fit(_frame(), elbo_tol=1e-3)
