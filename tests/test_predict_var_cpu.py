"""What the posterior predictive variance surface (`pmf_predict_var`, `pmf_eval_run_var`, `predict_variance`,
`log_predictive_density`) promises without a GPU: error codes across the C ABI, and the model classes' refusals, which
come before any device context is touched."""
import ctypes as C

import pytest

PMF_EINVAL = -1                                   # include/pmf_hip.h


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import pmf_hip
    return pmf_hip.load()


def test_null_context_is_einval_with_a_message(lib):
    """Both entry points: a null context (whatever the other arguments are) returns PMF_EINVAL and sets
    pmf_last_error; nothing is dereferenced -- `n = 0` does not turn a null context into success."""
    u = (C.c_int32 * 2)(0, 1)
    out = (C.c_double * 2)(7.0, 7.0)
    for n in (0, 2):
        assert lib.pmf_predict_var(None, n, u, u, out) == PMF_EINVAL
        assert b"pmf_predict_var: null context" in lib.pmf_last_error()
    assert list(out) == [7.0, 7.0]
    sv, sl = C.c_double(7.0), C.c_double(7.0)
    assert lib.pmf_eval_run_var(None, 0, 0.0, 1.0, C.byref(sv), C.byref(sl)) == PMF_EINVAL
    assert b"pmf_eval_run_var: null context" in lib.pmf_last_error()
    assert lib.pmf_eval_run_var(None, 0, 0.0, 1.0, None, None) == PMF_EINVAL
    assert (sv.value, sl.value) == (7.0, 7.0)


def test_binding_names_the_new_kernel_class():
    import pmf_hip
    assert pmf_hip.KERNEL_NAMES[12] == "predict_var" and len(pmf_hip.KERNEL_NAMES) == 13
    assert {"pmf_predict_var", "pmf_eval_run_var"} <= set(pmf_hip.SIGNATURES)


def _frame():
    import pandas as pd
    return pd.DataFrame({"u": [0, 1], "i": [0, 1], "rating": [1.0, 2.0]})


def test_gradient_model_has_no_predictive_variance():
    """GaussianMFSGD keeps point estimates: both methods raise NotImplementedError naming the class, fitted or not,
    before a context is looked for (an unfitted model would otherwise say "has not been fitted")."""
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    model = GaussianMFSGD(GaussianMFSGDConfig(n_factors=4, verbose=False))
    with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
        model.predict_variance([0], [0])
    with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
        model.log_predictive_density(_frame())


@pytest.mark.parametrize("module", ["gaussian_mf_cavi_bias", "gaussian_mf_cavi"])
def test_unfitted_cavi_model_says_so(module):
    import importlib
    mod = importlib.import_module("src.models." + module)
    model = mod.GaussianMFCAVI(mod.GaussianMFCAVIConfig(n_factors=4, verbose=False))
    with pytest.raises(RuntimeError, match="has not been fitted"):
        model.predict_variance([0], [0])
    with pytest.raises(RuntimeError, match="has not been fitted"):
        model.log_predictive_density(_frame())
