"""What the exact fold-in of the count models (`pmf_gamma_fold_in_exact`, `Context.gamma_fold_in_exact`,
`fold_in_users(update="exact")`) promises without a GPU: the recursion the GPU tests compare against
(tests/gamma_fold_in_exact_reference.py) is the reference ELBO module's own exact half-sweep, its row bound does not fall
and tells the two updates apart on the GPU tests' batch, two summation orders of it stay within a tenth of the fp64
bounds the GPU tests use, and the model surface's refusals, which come before any device call.

The argument checks of the C call live in pmf_gamma.hip (shared with `pmf_gamma_fold_in`), not in pmf_batch.h: they run
on the device machine, in tests/test_gamma_fold_in_exact_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import gamma_elbo_reference as ref
from gamma_fold_in_exact_reference import (FLAT_PRIORS, KAPPA_PRIORS, call_prior, exact_batch, fold_in_exact_reference, frozen_state,
                                           reverse_rows, row_bound)
from gamma_fold_in_reference import fold_in_reference
from helpers import rel_err

PMF_EINVAL = -1
F64_TOL = {1: 1e-12, 3: 1e-11, 20: 1e-9}          # the fp64 bounds of tests/test_gamma_fold_in_exact_gpu.py
K = 64                                            # the K of the GPU test's monotonicity check


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import pmf_hip
    return pmf_hip.load()


def test_null_context_is_einval_with_a_message(lib):
    row_ptr = (C.c_int64 * 3)(0, 1, 2)
    ids = (C.c_int32 * 2)(0, 1)
    x = (C.c_double * 2)(1.0, 2.0)
    outs = [(C.c_double * 8)(*[7.0] * 8) for _ in range(3)] + [(C.c_double * 2)(7.0, 7.0) for _ in range(2)]
    for n in (0, 2):
        assert lib.pmf_gamma_fold_in_exact(None, 0, n, row_ptr, ids, x, 0.3, 1.0, 1, 1.5, 5.0, 3, None, None, None, *outs) == PMF_EINVAL
        assert lib.pmf_last_error().startswith(b"pmf_gamma_fold_in_exact: null context")
    assert all(list(o) == [7.0] * len(o) for o in outs)


def test_binding_lists_the_entry_point_and_adds_no_kernel_class():
    import pmf_hip
    assert len(pmf_hip.SIGNATURES["pmf_gamma_fold_in_exact"][1]) == 20        # pmf_gamma_fold_in's 19 and init_rate
    assert len(pmf_hip.KERNEL_NAMES) == 13          # timed under the two existing gamma classes
    assert callable(pmf_hip.Context.gamma_fold_in_exact)


# ---- the reference recursion -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hierarchical", [True, False])
@pytest.mark.parametrize("side", [0, 1])
def test_one_pass_is_the_reference_half_sweep_bit_for_bit(side, hierarchical):
    """From a state's own (a, b) and kappa / h on its own ratings, one pass equals `factor_half_sweep(exact=True)` then
    `hyper_half_sweep`: the same bits in every element of every row, rows without ratings included."""
    from test_gamma_exact_gpu import HPF_PRIORS, POISSON_PRIORS, SIDE_KEYS, I, U, _problem
    u, i, x = _problem()
    k = 12
    priors = HPF_PRIORS if hierarchical else POISSON_PRIORS
    st = ref.initial_state(7, U, I, k, priors, hierarchical)
    rows, others = (u, i) if side == 0 else (i, u)
    R = (U, I)[side]
    order = np.argsort(rows, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=R))])
    assert (np.diff(row_ptr) == 0).any() and np.diff(row_ptr).max() > 32
    (ka, kb), (oa, ob) = SIDE_KEYS[side], SIDE_KEYS[1 - side]
    prior = priors[side]
    if hierarchical:
        kappa = prior[1] + k * prior[0]
        rho = kappa / st[("h_xi", "h_eta")[side]]
        got = fold_in_exact_reference(st[oa], st[ob], row_ptr, others[order], x[order], prior[0], 0.0, True, kappa, prior[2], n_iter=1,
                                      init_shape=st[ka], init_rate=st[kb], init_prior_rate=rho)
        a, b = ref.factor_half_sweep(st, side, u, i, x, prior[0], rho, exact=True)
        after = dict(st)
        after[ka], after[kb] = a, b
        h = ref.hyper_half_sweep(after, side, prior[2])
        want = (a / b, a, b, kappa / h, h)
    else:
        got = fold_in_exact_reference(st[oa], st[ob], row_ptr, others[order], x[order], prior[0], prior[1], n_iter=1,
                                      init_shape=st[ka], init_rate=st[kb])
        a, b = ref.factor_half_sweep(st, side, u, i, x, prior[0], prior[1], exact=True)
        want = (a / b, a, b, None, None)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if w is not None:
            assert np.asarray(g).tobytes() == np.asarray(w).tobytes()


def _bound_inputs(hierarchical, small=True):
    row_ptr, ids, x = exact_batch(7)
    st = frozen_state(K, small, row_ptr, ids)
    prior = KAPPA_PRIORS if hierarchical else FLAT_PRIORS
    return row_ptr, ids, x, st, prior


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("hierarchical", [True, False])
def test_row_bound_does_not_fall_and_tells_the_updates_apart(hierarchical, small):
    """float64, 20 passes from the cold start on the GPU test's batch: every row's bound after pass t is at least the one
    after pass t - 1 minus 2 x the evaluation slack (the rule of tests/test_gamma_exact_gpu.py); and the reference's
    update, run for the same 20 passes against the same frozen side, ends lower on at least one row by more than that
    slack -- the inputs can tell the two updates apart."""
    row_ptr, ids, x, st, prior = _bound_inputs(hierarchical, small)
    a_o, b_o = st["a_beta"], st["b_beta"]
    trace = []
    out = fold_in_exact_reference(a_o, b_o, row_ptr, ids, x, *call_prior(K, hierarchical), n_iter=20, trace=trace)
    previous, tightest = None, np.inf
    for t, (s, r, h) in enumerate(trace):
        value, allowed = row_bound(a_o, b_o, row_ptr, ids, x, s, r, h, prior, hierarchical)
        assert np.isfinite(value).all()
        if previous is not None:
            tightest = min(tightest, float(np.min((value - previous) / (2.0 * allowed))))
            assert (value >= previous - 2.0 * allowed).all(), (t, np.flatnonzero(value < previous - 2.0 * allowed))
        previous = value
    assert np.array_equal(trace[-1][0], out[1]) and np.array_equal(trace[-1][1], out[2])
    exact_end, allowed = previous, allowed
    plain = fold_in_reference(a_o / b_o, row_ptr, ids, x, *call_prior(K, hierarchical), n_iter=20)
    plain_end, plain_allowed = row_bound(a_o, b_o, row_ptr, ids, x, plain[1], plain[2], plain[4], prior, hierarchical)
    lower = plain_end < exact_end - 2.0 * (allowed + plain_allowed)
    print(f"hierarchical={hierarchical} small={small}: smallest rise {tightest:.3g} slacks; the reference's update ends lower on "
          f"{int(lower.sum())} of {len(lower)} rows, by up to {float(np.max(exact_end - plain_end)):.3g}")
    assert lower.any()


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("k", [5, 64, 129])
def test_two_summation_orders_stay_within_a_tenth_of_the_fp64_bounds(k, small):
    """The condition of the GPU test's fp64 bounds (1e-12 / 1e-11 / 1e-9 relative after 1 / 3 / 20 passes): the float64
    restatement with every row's ratings forward and reversed -- the same sums in two orders -- agrees within a tenth of
    them on the GPU test's batch, warm and cold, for every K the fp64 GPU cases use."""
    row_ptr, ids, x = exact_batch(7)
    st = frozen_state(k, small, row_ptr, ids)
    back_ids, back_x = reverse_rows(row_ptr, ids, x)
    for hierarchical, warm in ((True, False), (False, True), (True, True)):
        prior = call_prior(k, hierarchical)
        start = dict(init_shape=st["init_a"], init_rate=st["init_b"],
                     init_prior_rate=prior[3] / st["init_h"] if hierarchical else None) if warm else {}
        fwd, back = [], []
        fold_in_exact_reference(st["a_beta"], st["b_beta"], row_ptr, ids, x, *prior, n_iter=20, trace=fwd, **start)
        fold_in_exact_reference(st["a_beta"], st["b_beta"], row_ptr, back_ids, back_x, *prior, n_iter=20, trace=back, **start)
        for n_iter, tol in F64_TOL.items():
            errs = [rel_err(g, w) for g, w in zip(fwd[n_iter - 1], back[n_iter - 1]) if hierarchical or np.ndim(w) == 2]
            print(f"K={k} small={small} hier={hierarchical} warm={warm} n_iter={n_iter}: " + " ".join("%.3g" % e for e in errs))
            assert max(errs) <= tol / 10.0, (n_iter, errs)


# ---- model surface -----------------------------------------------------------------------------------------------------
def _frame():
    import pandas as pd
    return pd.DataFrame({"u": ["a", "b"], "i": [0, 1], "rating": [1.0, 2.0]})


def _model(cls):
    if cls == "HPF_CAVI":
        from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
        return HPF_CAVI(HPF_CAVI_Config(n_factors=4, verbose=False))
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    return PoissonMFCAVI(PoissonMFCAVIConfig(n_factors=4, verbose=False))


class _Closed:
    """stands in for a context no call may reach"""
    def close(self):
        pass


@pytest.mark.parametrize("cls", ["PoissonMFCAVI", "HPF_CAVI"])
def test_model_surface_refusals(cls):
    """An unknown `update` is a ValueError (before anything else), an unfitted model says so under either update, and
    after a sharded fit -- the serving context holds FACTOR only -- `update="exact"` is a NotImplementedError that names
    the reason, as `elbo()` and the predictive are; so is a fit that ran no iteration (a RuntimeError)."""
    model = _model(cls)
    for fold in (model.fold_in_users, model.fold_in_items):
        with pytest.raises(ValueError, match="update must be one of"):
            fold(_frame(), update="cavi")
        for update in ("reference", "exact"):
            with pytest.raises(RuntimeError, match="has not been fitted"):
                fold(_frame(), update=update)
    model._ctx, model._shard_ctx = _Closed(), _Closed()        # what `_finish_sharded` leaves
    model.history_["iterations"] = 3
    for fold in (model.fold_in_users, model.fold_in_items):
        with pytest.raises(NotImplementedError, match="sharded fit: the full-size context holds FACTOR only"):
            fold(_frame(), update="exact")
        with pytest.raises(ValueError, match="update must be one of"):
            fold(_frame(), update=None)
    model._shard_ctx = None
    model.history_["iterations"] = 0
    with pytest.raises(RuntimeError, match="has run no iteration"):
        model.fold_in_users(_frame(), update="exact")
    model._ctx = None


def test_record_names_the_update():
    from src.models._gamma_fold_in import GammaFoldIn
    E = np.ones((2, 3))
    assert GammaFoldIn(np.arange(2), E, E, E, None, E).update == "reference"
