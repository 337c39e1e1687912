"""What the fold-in surface (`pmf_gauss_fold_in`, `Context.gauss_fold_in`, `fold_in_users` / `fold_in_items`) promises
without a GPU: the null-context error across the C ABI, the binding, and the model classes' refusals, which come before
any device call."""
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
    """A null context is refused before anything else is looked at -- `n_rows = 0` does not turn it into success --
    and no output buffer is written."""
    row_ptr = (C.c_int64 * 3)(0, 1, 2)
    ids = (C.c_int32 * 2)(0, 1)
    x = (C.c_double * 2)(1.0, -1.0)
    out_f = (C.c_double * 8)(*[7.0] * 8)
    out_b = (C.c_double * 2)(7.0, 7.0)
    for n in (0, 2):
        assert lib.pmf_gauss_fold_in(None, 0, n, row_ptr, ids, x, 0.3, 0.5, 1.0, 1, out_f, None, out_b) == PMF_EINVAL
        assert lib.pmf_last_error().startswith(b"pmf_gauss_fold_in: null context")
    assert lib.pmf_gauss_fold_in(None, 5, -1, None, None, None, 0.0, 0.0, 0.0, 0, None, None, None) == PMF_EINVAL
    assert lib.pmf_last_error().startswith(b"pmf_gauss_fold_in: null context")
    assert list(out_f) == [7.0] * 8 and list(out_b) == [7.0, 7.0]


def test_binding_lists_the_entry_point_and_adds_no_kernel_class():
    import pmf_hip
    assert "pmf_gauss_fold_in" in pmf_hip.SIGNATURES
    assert len(pmf_hip.SIGNATURES["pmf_gauss_fold_in"][1]) == 13
    assert len(pmf_hip.KERNEL_NAMES) == 13          # fold-in is timed under the existing Gaussian classes
    assert callable(pmf_hip.Context.gauss_fold_in)


def _frame():
    import pandas as pd
    return pd.DataFrame({"u": ["a", "b"], "i": [0, 1], "rating": [1.0, 2.0]})


def test_gradient_model_has_no_fold_in():
    """GaussianMFSGD keeps point estimates, no covariances of the frozen side: NotImplementedError naming the class,
    before a context is looked for (an unfitted model would otherwise say "has not been fitted")."""
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    model = GaussianMFSGD(GaussianMFSGDConfig(n_factors=4, verbose=False))
    with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
        model.fold_in_users(_frame())
    with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
        model.fold_in_items(_frame())


@pytest.mark.parametrize("module", ["gaussian_mf_cavi_bias", "gaussian_mf_cavi"])
def test_unfitted_cavi_model_says_so(module):
    import importlib
    mod = importlib.import_module("src.models." + module)
    model = mod.GaussianMFCAVI(mod.GaussianMFCAVIConfig(n_factors=4, verbose=False))
    with pytest.raises(RuntimeError, match="has not been fitted"):
        model.fold_in_users(_frame())
    with pytest.raises(RuntimeError, match="has not been fitted"):
        model.fold_in_items(_frame())


def test_sharded_fit_is_refused():
    """After a sharded fit the full-size context holds no covariances: NotImplementedError, as `predict_variance`
    raises.  (The state of such a model is imitated: a context on each of the two attributes.)"""
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    model = GaussianMFCAVI(GaussianMFCAVIConfig(n_factors=4, verbose=False))
    model._ctx, model._shard_ctx = object(), object()
    try:
        with pytest.raises(NotImplementedError, match="fold_in_users after a sharded fit"):
            model.fold_in_users(_frame())
        with pytest.raises(NotImplementedError, match="fold_in_items after a sharded fit"):
            model.fold_in_items(_frame())
    finally:
        model._ctx = model._shard_ctx = None


def test_fold_in_record_predicts_on_the_host():
    import numpy as np
    from src.models._gaussian_host import FoldIn
    rng = np.random.default_rng(0)
    mean, m_other, bias, b_other = rng.normal(size=(3, 4)), rng.normal(size=(5, 4)), rng.normal(size=3), rng.normal(size=5)
    rows, ids = np.array([2, 0, 0]), np.array([4, 4, 1])
    want = (mean[rows] * m_other[ids]).sum(1) + bias[rows] + b_other[ids] + 3.5
    assert np.allclose(FoldIn(np.arange(3), mean, None, bias, m_other, b_other).predict(rows, ids, 3.5), want, rtol=0, atol=1e-14)
    assert np.allclose(FoldIn(np.arange(3), mean, None, bias, m_other, None).predict(rows, ids), want - b_other[ids] - 3.5,
                       rtol=0, atol=1e-14)
