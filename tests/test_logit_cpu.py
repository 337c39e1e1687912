"""What the logistic model (`pmf_gauss_logit_refresh`, src/models/logistic_mf_cavi.py) promises
without a GPU: lambda(xi) and its series switch, the Jaakkola-Jordan inequality, the monotone bound of the NumPy reference
fit (tests/logit_reference.py) with its own rounding floor, the exported symbols, and the model class's refusals."""
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import logit_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)

# the planted problem the GPU tests fit as well (tests/test_logit_gpu.py)
SMALL = dict(seed=11, U=40, I=30, K=3, N=600)
ETA2 = 1.0
# A step of the reference fit may fall by rounding only.  L is a sum of N data terms and (U + I) K prior / entropy terms of
# magnitude O(1) each, accumulated in double: an evaluation is within about (N + (U + I) K) eps |L| of exact, and a fall is
# the difference of two.  Asserted below; the measured fall is what the GPU test's margin rests on.
REFERENCE_FALL_BOUND = 2.0 * (SMALL["N"] + (SMALL["U"] + SMALL["I"]) * SMALL["K"]) * EPS


def _lambdas():
    from src.models.logistic_mf_cavi import jj_lambda
    return {"reference": ref.lam, "model": jj_lambda}


def _quotient(xi):
    return np.tanh(0.5 * xi) / (4.0 * xi)


def _series(xi):
    return 0.125 - xi * xi / 96.0 + xi ** 4 / 960.0


@pytest.mark.parametrize("which", ["reference", "model"])
def test_lambda_values_and_the_series_switch(which):
    lam = _lambdas()[which]
    assert float(lam(0.0)) == 0.125
    assert float(lam(1e-9)) == 0.125                       # 1e-18 / 96 is below half an ulp of 1/8
    assert abs(float(lam(40.0)) - 1.0 / 160.0) <= 2 * EPS / 160.0   # tanh(20) = 1 to the last bit
    assert float(lam(-2.0)) == float(lam(2.0))
    below, at = np.nextafter(ref.SERIES_BELOW, 0.0), ref.SERIES_BELOW
    assert float(lam(below)) == _series(below) and float(lam(at)) == _quotient(at)     # the switch is where it says
    # continuity across the switch: the two forms agree to rounding on both sides of it, relative to the value
    for xi in (below, at, np.nextafter(at, 1.0)):
        gap = abs(_series(xi) - _quotient(xi)) / _quotient(xi)
        print(f"lambda switch at {xi!r}: series vs quotient {gap / EPS:.2f} eps")
        assert gap <= 4 * EPS, (xi, gap / EPS)
    # and the step across the switch is the function's own slope, not a jump: |lambda'| = xi / 48 there
    step = abs(float(lam(at)) - float(lam(below)))
    assert step <= 4 * EPS * 0.125
    xs = np.array([0.0, 1e-9, 5e-4, 1e-3, 0.3, 2.0, 40.0])
    assert np.array_equal(lam(xs), np.array([float(lam(v)) for v in xs]))               # vector and scalar forms agree
    assert np.all(np.diff(lam(np.linspace(0.0, 50.0, 2001))) <= 0.0)                    # decreasing from 1/8


def test_jaakkola_jordan_inequality_on_a_grid():
    """log sigmoid(s) >= log sigmoid(xi) + (s - xi) / 2 - lambda(xi) (s^2 - xi^2), with equality at s = +-xi."""
    s = np.linspace(-30.0, 30.0, 601)[:, None]
    xi = np.concatenate([[0.0, 1e-9, 5e-4, 1e-3], np.linspace(0.01, 30.0, 300)])[None, :]
    lhs = ref.log_sigmoid(s)
    rhs = ref.log_sigmoid(xi) + 0.5 * (s - xi) - ref.lam(xi) * (s * s - xi * xi)
    slack = lhs - rhs
    # rounding of the right-hand side: a few eps of its largest term
    tol = 8 * EPS * (np.abs(ref.log_sigmoid(xi)) + 0.5 * np.abs(s - xi) + ref.lam(xi) * np.abs(s * s - xi * xi) + np.abs(lhs))
    assert np.all(slack >= -tol), float(np.min(slack + tol))
    for sign in (1.0, -1.0):
        at = sign * xi
        eq = ref.log_sigmoid(at) - (ref.log_sigmoid(xi) + 0.5 * (at - xi))
        assert np.all(np.abs(eq) <= 8 * EPS * (1.0 + np.abs(xi))), float(np.max(np.abs(eq)))
    assert slack.max() > 1.0                                # the bound is not tight away from s = +-xi


def reference_trace(n_iter=30):
    u, i, x, _, _ = ref.planted(SMALL["seed"], SMALL["U"], SMALL["I"], SMALL["K"], SMALL["N"])
    return ref.fit(u, i, x, SMALL["U"], SMALL["I"], SMALL["K"], ETA2, n_iter, seed=5)[1]


def test_reference_bound_is_monotone_and_records_its_rounding_floor():
    trace = np.array(reference_trace(30))
    fall = ref.max_fall(trace) / np.abs(trace).max()
    print(f"reference fit, 30 iterations: L {trace[0]:.6f} -> {trace[-1]:.6f}, largest relative fall {fall:.3e} "
          f"(bound {REFERENCE_FALL_BOUND:.3e})")
    assert trace[-1] > trace[0] + 1.0                       # the fit moves: a constant trace would be monotone too
    assert fall <= REFERENCE_FALL_BOUND
    # `bound` (a fresh refresh at the final state) is at least the last recorded value: the item sweep came between
    u, i, x, _, _ = ref.planted(SMALL["seed"], SMALL["U"], SMALL["I"], SMALL["K"], SMALL["N"])
    st, tr = ref.fit(u, i, x, SMALL["U"], SMALL["I"], SMALL["K"], ETA2, 3, seed=5)
    assert ref.bound(*st, u, i, x, ETA2) >= tr[-1] - REFERENCE_FALL_BOUND * abs(tr[-1])


def test_reference_refresh_and_sweep_are_the_weighted_gaussian_update():
    """c_j y_j = x_j - 1/2 and the label is the sign of y: the logistic sweep is the weighted Gaussian sweep of
    tests/gauss_weighted_reference.py with sigma2 = 1."""
    import gauss_weighted_reference as wref
    u, i, x, _, _ = ref.planted(3, 12, 9, 4, 60)
    m_u, V_u, m_i, V_i = ref.initial_state(1, 12, 9, 4)
    xi, c, y, D, mag = ref.refresh(m_u, V_u, m_i, V_i, u, i, x)
    assert np.array_equal(y > 0, x > 0.5) and np.allclose(c * y, x - 0.5, rtol=4 * EPS, atol=0)
    assert np.all(c > 0) and np.all(c <= 0.25) and np.all(mag >= xi * xi * (1.0 - 8 * EPS))
    m, V = ref.sweep(m_u, V_u, m_i, V_i, u, i, x, c, 0.7)
    zeros_u, zeros_i = np.zeros(12), np.zeros(9)
    wm, wV = wref.factor_sweep(m_u, V_u, m_i, V_i, zeros_u, zeros_i, u, i, y, c, 1.0, 0.7)
    np.testing.assert_allclose(m, wm, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(V, wV, rtol=1e-12, atol=1e-13)


def test_library_and_binding_expose_the_new_entry_points():
    import __graft_entry__ as g
    g.build()
    import pmf_hip
    from pmf_hip.engine import Context
    lib = pmf_hip.load()
    header = open(os.path.join(ROOT, "include", "pmf_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", pmf_hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    test_out = subprocess.run(["nm", "-D", "--defined-only", pmf_hip.TEST_LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("pmf_gauss_logit_refresh", "pmf_ctx_side_ratings"):
        assert re.search(rf"^int {name}\(pmf_ctx \*ctx, int side,", header, flags=re.M), name
        assert name in pmf_hip.SIGNATURES and hasattr(lib, name), name
        assert f" T {name}" in out and f" T {name}" in test_out, name
    assert callable(Context.gauss_logit_refresh) and callable(Context.side_ratings)
    assert lib.pmf_abi_version() == 3 and re.search(r"#define PMF_ABI_VERSION 3\b", header)
    # a null context and a bad side are argument errors, not crashes, with or without a GPU
    assert lib.pmf_gauss_logit_refresh(None, 0, None) == -1
    assert b"pmf_gauss_logit_refresh: null context" in lib.pmf_last_error()
    assert lib.pmf_ctx_side_ratings(None, 0, None, None, None, None) == -1
    assert b"pmf_ctx_side_ratings" in lib.pmf_last_error()


def test_model_class_refuses_what_it_does_not_support():
    from src.models.logistic_mf_cavi import LogisticMFCAVI, LogisticMFCAVIConfig
    cfg = LogisticMFCAVIConfig(n_factors=3, max_iter=1, verbose=False)
    assert (cfg.eta2, cfg.xi_init, cfg.seed, cfg.dtype) == (1.0, 1.0, 42, None)
    df = pd.DataFrame({"u": [0, 1, 2, 2], "i": [0, 1, 1, 0], "rating": [1.0, 0.0, 0.5, 2.0]})
    with pytest.raises(ValueError, match=r"0 or 1.*0\.5.*position 2"):
        LogisticMFCAVI(cfg).fit(df)
    ok = df.assign(rating=[1.0, 0.0, 1.0, 0.0])
    with pytest.raises(NotImplementedError, match="comm="):
        LogisticMFCAVI(cfg, comm=object())
    with pytest.raises(NotImplementedError, match="unobserved='zero'"):
        LogisticMFCAVI(cfg).fit(ok, unobserved="zero")
    with pytest.raises(NotImplementedError, match="weights="):
        LogisticMFCAVI(cfg).fit(ok, weights=np.ones(4))
    model = LogisticMFCAVI(cfg)
    for call in (lambda: model.fold_in_users(ok), lambda: model.fold_in_items(ok), lambda: model.log_predictive_density(ok)):
        with pytest.raises(NotImplementedError, match="logistic"):
            call()
    with pytest.raises(RuntimeError, match="not been fitted"):
        model.predict_proba([0], [0])
