"""What the ELBO surface (`pmf_gauss_elbo_terms`, `Context.gauss_elbo_terms`, `elbo_from_terms`, `elbo`, `fit(track_elbo=)`)
promises without a GPU: the binding, the null-context error, the model classes' refusals, and the assembly formula --
`elbo_from_terms` fed with sums formed densely in float64 NumPy (tests/elbo_reference.py) from the states of an
`oracle.cavi_oracle` run rises at every half-sweep of the reference's iteration, and the expected squared residual
comes out the same from the user statistics, the item statistics and rating by rating."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import elbo_reference as ref
from helpers import skewed_problem

PMF_EINVAL = -1                                   # include/pmf_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA2, ETA_T, ETA_B, ETA_BIAS = 0.3, 0.5, 0.7, 1.0
ITERATIONS = 4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import pmf_hip
    return pmf_hip.load()


def test_header_prototype_equals_the_binding_and_the_symbol_is_exported(lib):
    import pmf_hip
    header = open(os.path.join(ROOT, "include", "pmf_hip.h")).read()
    proto = re.search(r"\nint pmf_gauss_elbo_terms\((.*?)\);", header, re.S)
    assert proto, "include/pmf_hip.h does not declare pmf_gauss_elbo_terms"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",")]
    ctype = {"pmf_ctx *": C.c_void_p, "int": C.c_int, "double *": C.POINTER(C.c_double)}
    want = [ctype[re.sub(r"\w+$", "", a).strip()] for a in args]
    res, got = pmf_hip.SIGNATURES["pmf_gauss_elbo_terms"]
    assert res is C.c_int and got == want
    assert lib.pmf_gauss_elbo_terms.argtypes == want
    for name, value in (("SQNORM", 0), ("LOGDET", 1), ("BIAS_SQ", 2), ("ESS", 3), ("TERMS", 4)):
        assert re.search(r"#define PMF_ELBO_%s %d\b" % (name, value), header)
        assert getattr(pmf_hip, "ELBO_" + name) == value
    assert re.search(r"#define PMF_ABI_VERSION 3\b", header)
    assert callable(pmf_hip.Context.gauss_elbo_terms)


def test_no_kernel_class_is_added():
    import pmf_hip
    assert len(pmf_hip.KERNEL_NAMES) == 13          # the ELBO kernels are timed under the existing Gaussian classes


def test_null_context_and_null_totals_are_einval_and_write_nothing(lib):
    totals = (C.c_double * 4)(*[7.0] * 4)
    rows = (C.c_double * 8)(*[7.0] * 8)
    for with_data in (0, 1):
        assert lib.pmf_gauss_elbo_terms(None, 0, with_data, totals, rows) == PMF_EINVAL
        assert lib.pmf_last_error().startswith(b"pmf_gauss_elbo_terms: null context")
    assert lib.pmf_gauss_elbo_terms(None, 5, 0, None, None) == PMF_EINVAL
    assert lib.pmf_last_error().startswith(b"pmf_gauss_elbo_terms: null context")
    assert list(totals) == [7.0] * 4 and list(rows) == [7.0] * 8


# ---- the assembly formula against an oracle run ---------------------------------------------------------------------
def _half_sweeps(K, bias):
    """The states after every half-sweep of ITERATIONS reference iterations (theta, beta, then -- bias model -- user
    biases, item biases: gaussian_mf_cavi_bias.py:129-263), the initial state first."""
    from oracle import cavi_oracle as orc
    u, i, x = skewed_problem(K, 90, 40, 2500, "centered")
    U, I = orc.infer_dims(u, i)
    st = orc.init_gaussian(U, I, K, seed=K, bias=bias)
    (uptr, upos), (iptr, ipos) = orc.group_positions(u, U), orc.group_positions(i, I)
    bu, bi = (st["m_user_bias"], st["m_item_bias"]) if bias else (np.zeros(U), np.zeros(I))
    states = [dict(st)]
    for _ in range(ITERATIONS):
        st["m_theta"], st["V_theta"] = orc.gauss_factor_sweep_rows(st["m_theta"], st["V_theta"], st["m_beta"], st["V_beta"],
                                                                   uptr, upos, i, x, bu, bi, SIGMA2, ETA_T)
        states.append(dict(st))
        st["m_beta"], st["V_beta"] = orc.gauss_factor_sweep_rows(st["m_beta"], st["V_beta"], st["m_theta"], st["V_theta"],
                                                                 iptr, ipos, u, x, bi, bu, SIGMA2, ETA_B)
        states.append(dict(st))
        if bias:
            bu = st["m_user_bias"] = orc.gauss_bias_sweep_rows(bu, bi, st["m_theta"], st["m_beta"], uptr, upos, i, x,
                                                               SIGMA2, ETA_BIAS)
            states.append(dict(st))
            bi = st["m_item_bias"] = orc.gauss_bias_sweep_rows(bi, bu, st["m_beta"], st["m_theta"], iptr, ipos, u, x,
                                                               SIGMA2, ETA_BIAS)
            states.append(dict(st))
    return (u, i, x), states


def _terms(st, u, i, x, bias):
    U, I = len(st["m_theta"]), len(st["m_beta"])
    bu = st["m_user_bias"] if bias else np.zeros(U)
    bi = st["m_item_bias"] if bias else np.zeros(I)
    user = ref.side_terms(st["m_theta"], st["V_theta"], bu, st["m_beta"], st["V_beta"], bi, u, i, x)[0].sum(axis=0)
    item = ref.side_terms(st["m_beta"], st["V_beta"], bi, st["m_theta"], st["V_theta"], bu, i, u, x)[0].sum(axis=0)
    return user, item


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("K", [3, 8])
def test_elbo_rises_at_every_half_sweep_and_the_three_data_terms_agree(K, bias):
    from src.models._gaussian_host import elbo_from_terms
    from pmf_hip import ITEM, USER
    (u, i, x), states = _half_sweeps(K, bias)
    assert len(states) == 1 + ITERATIONS * (4 if bias else 2)
    eta_bias2 = ETA_BIAS if bias else None
    nu, ni = np.bincount(u, minlength=len(states[0]["m_theta"])), np.bincount(i, minlength=len(states[0]["m_beta"]))
    values = []
    for st in states:
        user, item = _terms(st, u, i, x, bias)
        L, parts = elbo_from_terms(user, item, nu, ni, len(x), K, SIGMA2, ETA_T, ETA_B, eta_bias2)
        L_item, _ = elbo_from_terms(user, item, nu, ni, len(x), K, SIGMA2, ETA_T, ETA_B, eta_bias2, data_side=ITEM)
        assert L == elbo_from_terms(user, item, nu, ni, len(x), K, SIGMA2, ETA_T, ETA_B, eta_bias2, data_side=USER)[0]
        assert np.isclose(sum(parts.values()), L, rtol=1e-15, atol=0)
        assert set(parts) == {"data", "prior_theta", "entropy_theta", "prior_beta", "entropy_beta"} | (
            {"prior_user_bias", "entropy_user_bias", "prior_item_bias", "entropy_item_bias"} if bias else set())
        # the data term three ways
        per_rating = ref.ess_per_rating(st["m_theta"], st["V_theta"], st.get("m_user_bias", np.zeros(len(nu))), st["m_beta"],
                                        st["V_beta"], st.get("m_item_bias", np.zeros(len(ni))), u, i, x)
        assert np.isclose(user[ref.ESS], item[ref.ESS], rtol=1e-12, atol=0)
        assert np.isclose(user[ref.ESS], per_rating, rtol=1e-12, atol=0)
        assert np.isclose(L, L_item, rtol=1e-12, atol=0)
        # and the whole bound against the block-by-block formula
        assert np.isclose(L, ref.elbo(st, u, i, x, SIGMA2, ETA_T, ETA_B, eta_bias2), rtol=1e-12, atol=0)
        values.append(L)
    steps = np.diff(values)
    print(f"K={K} bias={bias}: L from {values[0]:.3f} to {values[-1]:.3f}, smallest step {steps.min():.4g}")
    assert (steps > 0).all(), steps


# ---- refusals of the model classes, before any device call -----------------------------------------------------------
def _frame():
    import pandas as pd
    return pd.DataFrame({"u": [0, 1], "i": [0, 1], "rating": [1.0, 2.0]})


def test_gradient_model_has_no_elbo():
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    model = GaussianMFSGD(GaussianMFSGDConfig(n_factors=4, verbose=False))
    with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
        model.elbo()
    with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
        model.fit(_frame(), track_elbo=True)
    with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
        model.fit(_frame(), elbo_tol=1e-3)


@pytest.mark.parametrize("module", ["gaussian_mf_cavi_bias", "gaussian_mf_cavi"])
def test_unfitted_model_says_so_and_fit_takes_the_arguments_by_keyword_only(module):
    import importlib
    import inspect
    mod = importlib.import_module("src.models." + module)
    model = mod.GaussianMFCAVI(mod.GaussianMFCAVIConfig(n_factors=4, verbose=False))
    with pytest.raises(RuntimeError, match="has not been fitted"):
        model.elbo()
    params = inspect.signature(model.fit).parameters
    assert params["track_elbo"].kind is inspect.Parameter.KEYWORD_ONLY and params["track_elbo"].default is False
    assert params["elbo_tol"].kind is inspect.Parameter.KEYWORD_ONLY and params["elbo_tol"].default is None


def test_sharded_fit_is_refused():
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    model = GaussianMFCAVI(GaussianMFCAVIConfig(n_factors=4, verbose=False))
    model._ctx, model._shard_ctx = object(), object()
    try:
        with pytest.raises(NotImplementedError, match="elbo after a sharded fit"):
            model.elbo()
    finally:
        model._ctx = model._shard_ctx = None

    class World:          # what DeviceModel looks at of a communicator
        world, rank = 2, 0
    model = GaussianMFCAVI(GaussianMFCAVIConfig(n_factors=4, verbose=False), comm=World())
    with pytest.raises(NotImplementedError, match="communicator"):
        model.fit(_frame(), track_elbo=True)
