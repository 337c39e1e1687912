"""What the Poisson / HPF fold-in surface (`pmf_gamma_fold_in`, `Context.gamma_fold_in`, `fold_in_users` / `fold_in_items`)
promises without a GPU: the null-context error across the C ABI, the binding, the model classes' refusals (which come
before any device call), the record's host predict -- and that the literal recursion the GPU tests compare against is the
oracle's own half-sweep, and reaches the GPU tests' bounds in float32."""
import ctypes as C

import numpy as np
import pytest

from gamma_fold_in_reference import TOL, batch, fold_in_reference
from helpers import rel_err, skewed_problem
from oracle import cavi_oracle as orc

PMF_EINVAL = -1                                   # include/pmf_hip.h
A, A_PRIME, B_PRIME = 0.3, 5.0, 5.0               # the priors of tests/test_gamma_gpu.py


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
    x = (C.c_double * 2)(1.0, 2.0)
    outs = [(C.c_double * 8)(*[7.0] * 8) for _ in range(3)] + [(C.c_double * 2)(7.0, 7.0) for _ in range(2)]
    for n in (0, 2):
        assert lib.pmf_gamma_fold_in(None, 0, n, row_ptr, ids, x, 0.3, 1.0, 1, 1.5, 5.0, 3, None, None, *outs) == PMF_EINVAL
        assert lib.pmf_last_error().startswith(b"pmf_gamma_fold_in: null context")
    assert lib.pmf_gamma_fold_in(None, 5, -1, None, None, None, 0.0, 0.0, 0, 0.0, 0.0, 0, None, None, None, None, None, None,
                                 None) == PMF_EINVAL
    assert lib.pmf_last_error().startswith(b"pmf_gamma_fold_in: null context")
    assert all(list(o) == [7.0] * len(o) for o in outs)


def test_binding_lists_the_entry_point_and_adds_no_kernel_class():
    import pmf_hip
    assert "pmf_gamma_fold_in" in pmf_hip.SIGNATURES
    assert len(pmf_hip.SIGNATURES["pmf_gamma_fold_in"][1]) == 19
    assert len(pmf_hip.KERNEL_NAMES) == 13          # the fold-in is timed under the two existing gamma classes
    assert callable(pmf_hip.Context.gamma_fold_in)


def _frame():
    import pandas as pd
    return pd.DataFrame({"u": ["a", "b"], "i": [0, 1], "rating": [1.0, 2.0]})


@pytest.mark.parametrize("module,cls", [("poisson_mf_cavi", "PoissonMFCAVI"), ("hpf_cavi", "HPF_CAVI")])
def test_unfitted_model_says_so(module, cls):
    import importlib
    mod = importlib.import_module("src.models." + module)
    config = getattr(mod, "PoissonMFCAVIConfig" if cls == "PoissonMFCAVI" else "HPF_CAVI_Config")
    model = getattr(mod, cls)(config(n_factors=4, verbose=False))
    with pytest.raises(RuntimeError, match="has not been fitted"):
        model.fold_in_users(_frame())
    with pytest.raises(RuntimeError, match="has not been fitted"):
        model.fold_in_items(_frame())


def test_extended_model_has_no_fold_in():
    """The scalar factors phi / psi are not covered: NotImplementedError naming the class, fitted or not."""
    from src.models.poisson_mf_extended_cavi import PoissonMFExtendedCAVI, PoissonMFExtendedCAVIConfig
    model = PoissonMFExtendedCAVI(PoissonMFExtendedCAVIConfig(n_factors=4, verbose=False))
    with pytest.raises(NotImplementedError, match="PoissonMFExtendedCAVI"):
        model.fold_in_users(_frame())
    with pytest.raises(NotImplementedError, match="PoissonMFExtendedCAVI"):
        model.fold_in_items(_frame())


def test_fold_in_record_predicts_on_the_host():
    from src.models._gamma_fold_in import GammaFoldIn
    rng = np.random.default_rng(0)
    E, E_other = rng.gamma(1.0, 1.0, size=(3, 4)), rng.gamma(1.0, 1.0, size=(5, 4))
    rows, ids = np.array([2, 0, 0]), np.array([4, 4, 1])
    fold = GammaFoldIn(np.arange(3), E, E * 2.0, np.full((3, 4), 2.0), None, E_other)
    assert np.allclose(fold.predict(rows, ids), (E[rows] * E_other[ids]).sum(1), rtol=0, atol=1e-14)


def test_frame_to_batch_keeps_frame_order_and_drops_unseen_ids():
    """The helper both fold-ins share: labels sorted, an id outside the fitted side dropped, frame order inside a row."""
    import pandas as pd
    from src.models._device_model import ITEM, USER, fold_in_batch
    df = pd.DataFrame({"u": ["zed", "amy", "zed", "bob", "amy", "zed"], "i": [3, 1, 0, 9, 2, 1], "rating": [1., 2., 3., 4., 5., 6.]})
    ids, row_ptr, other, x = fold_in_batch(df, USER, 5)
    assert list(ids) == ["amy", "bob", "zed"] and list(row_ptr) == [0, 2, 2, 5]
    assert list(other) == [1, 2, 3, 0, 1] and list(x) == [2., 5., 1., 3., 6.]
    df = pd.DataFrame({"u": [4, 0, 7, 2], "i": [10**6, 777, 777, 10**6], "rating": [1., 2., 3., 4.]})
    ids, row_ptr, other, x = fold_in_batch(df, ITEM, 5)
    assert list(ids) == [777, 10**6] and list(row_ptr) == [0, 1, 3] and list(other) == [0, 4, 2] and list(x) == [2., 1., 4.]


@pytest.fixture(scope="module")
def fitted():
    """skewed_problem after two oracle HPF iterations, per K: (state, ids, ratings, index lists)."""
    out = {}
    for K in (8, 64):
        U, I, N = 600, 120, 12000
        u, i, x = skewed_problem(100 + K, U, I, N)
        st = orc.init_hpf(U, I, K, A, A_PRIME, B_PRIME, A, A_PRIME, B_PRIME, seed=3)
        idx = (orc.group_positions(u, U), orc.group_positions(i, I))
        for _ in range(2):
            orc.hpf_iteration(st, idx, u, i, x, A, B_PRIME, A, B_PRIME)
        out[K] = (st, u, i, x, idx)
    return out


@pytest.mark.parametrize("K", [8, 64])
def test_the_reference_is_the_oracles_half_sweep(fitted, K):
    """n_iter = 1 from the state's own E_theta / E_xi on every user's training ratings (rows without ratings included)
    is `gamma_half_sweep_rows` + the xi update of `hpf_iteration`; with a scalar rate prior, the Poisson MF update."""
    st, u, i, x, ((uptr, upos), _) = fitted[K]
    assert (np.diff(uptr) == 0).any() and np.diff(uptr).max() > 64
    ids, xs = i[upos], x[upos]
    got = fold_in_reference(st["E_beta"], uptr, ids, xs, A, 0.0, True, st["gamma_a_xi"], B_PRIME, 1, st["E_theta"], st["E_xi"])
    shape, rate = orc.gamma_half_sweep_rows(st["E_theta"], st["E_beta"], uptr, upos, i, x, A, st["E_xi"])
    hyper = B_PRIME + np.sum(shape / rate, axis=1)
    for g, w in zip(got, (shape / rate, shape, rate, st["gamma_a_xi"] / hyper, hyper)):
        assert rel_err(g, w) <= 1e-13
    got = fold_in_reference(st["E_beta"], uptr, ids, xs, A, 1.5, False, n_iter=1, init_factor=st["E_theta"])
    shape, rate = orc.gamma_half_sweep_rows(st["E_theta"], st["E_beta"], uptr, upos, i, x, A, 1.5)
    for g, w in zip(got[:3], (shape / rate, shape, rate)):
        assert rel_err(g, w) <= 1e-13
    assert got[3] is None and got[4] is None


@pytest.mark.parametrize("hierarchical", [True, False])
@pytest.mark.parametrize("K", [8, 64])
def test_float32_arithmetic_reaches_a_quarter_of_the_gpu_bounds(fitted, K, hierarchical):
    """The recursion in float32 NumPy on the GPU tests' batch (rows of 0 .. 700 ratings from {0 .. 5}) stays within a
    quarter of tests/test_gamma_gpu.py:TOL of the float64 run, for 1, 3 and 20 updates: the GPU bounds are reachable."""
    st = fitted[K][0]
    E_beta = st["E_beta"].astype(np.float32).astype(np.float64)        # the table a float32 context holds
    row_ptr, ids, x = batch(7, E_beta.shape[0])
    prior = (A, 0.0, True, st["gamma_a_xi"], B_PRIME) if hierarchical else (A, 1.5, False, 0.0, 0.0)
    for n_iter in (1, 3, 20):
        want = fold_in_reference(E_beta, row_ptr, ids, x, *prior, n_iter=n_iter)
        got = fold_in_reference(E_beta, row_ptr, ids, x, *prior, n_iter=n_iter, dtype=np.float32)
        errs = [rel_err(g, w) for g, w in zip(got, want) if w is not None]
        print(f"K={K} hierarchical={hierarchical} n_iter={n_iter}: " + " ".join("%.3g" % e for e in errs))
        assert max(errs) <= TOL["f32"][n_iter] / 4, (n_iter, errs)
