"""Fold-in of new rows against a fitted Gaussian model (`pmf_gauss_fold_in`) against the literal factor / bias
alternation in float64 NumPy, evaluated on the state read back from the device (so the rounding of the inputs is not
part of the error).

Bounds of the parity tests are the project's own for these kernels (tests/test_gauss_gpu.py:
test_half_sweeps_vs_oracle_skewed, test_gaussian_beyond_128_factors): f64 1e-10, f32 2e-4 (3e-4 at K = 136), max abs on
means and biases, relative to the row's largest entry on covariances."""
import ctypes as C

import numpy as np
import pytest

from helpers import max_abs, skewed_problem

pytestmark = pytest.mark.gpu

SIGMA2, ETA2, ETA_B2 = 0.3, 0.5, 1.0
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 129, 700)   # 700: many tasks of a split row at this problem size
PMF_EINVAL, PMF_ERANGE = -1, -4


def _tol(K, dtype):
    return 1e-10 if dtype == "f64" else (3e-4 if K == 136 else 2e-4)


def _sizes(K):
    return (600, 120, 12000) if K <= 64 else (800, 50, 7000)


_STATE = {}


def _fitted_state(K, dtype, bias):
    """Ratings and the model arrays after two real device iterations (as tests/test_gauss_gpu.py::_oracle_vs_device),
    read back with get_array: computed once per (K, dtype, bias) and never changed."""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER
    key = (K, dtype, bias)
    if key in _STATE:
        return _STATE[key]
    U, I, N = _sizes(K)
    u, i, x = skewed_problem(100 + K, U, I, N, "centered")
    rng = np.random.default_rng(5)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_ratings(u, i, x)
        ctx.set_array(USER, ARR_FACTOR, 0.1 * rng.standard_normal((U, K)))
        ctx.set_array(ITEM, ARR_FACTOR, 0.1 * rng.standard_normal((I, K)))
        ctx.set_cov_identity(USER); ctx.set_cov_identity(ITEM)
        if bias:
            ctx.set_array(USER, ARR_BIAS, np.zeros(U)); ctx.set_array(ITEM, ARR_BIAS, np.zeros(I))
        for _ in range(2):
            ctx.gauss_factor_sweep(USER, SIGMA2, ETA2)
            ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA2)
            if bias:
                ctx.gauss_bias_sweep(USER, SIGMA2, ETA_B2)
                ctx.gauss_bias_sweep(ITEM, SIGMA2, ETA_B2)
        arrays = {(s, a): ctx.get_array(s, a) for s in (USER, ITEM) for a in (ARR_FACTOR, ARR_COV) + ((ARR_BIAS,) if bias else ())}
    for a in arrays.values():
        a.setflags(write=False)
    _STATE[key] = {"dims": (U, I), "ratings": (u, i, x), "arrays": arrays, "bias": bias}
    return _STATE[key]


def _open(state, K, dtype):
    """A fresh context holding `state` (float64 -> device dtype is exact: the arrays came from that dtype)."""
    import pmf_hip
    ctx = pmf_hip.Context(*state["dims"], K, dtype=dtype)
    ctx.set_ratings(*state["ratings"])
    for (side, array), host in state["arrays"].items():
        ctx.set_array(side, array, host)
    return ctx


def _batch(seed, n_other, lengths=LENGTHS):
    """CSR batch: ids on the opposite side drawn with repeats, ratings from {-2 .. 2}."""
    rng = np.random.default_rng(seed)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return row_ptr, rng.integers(0, n_other, row_ptr[-1]).astype(np.int32), rng.integers(-2, 3, row_ptr[-1]).astype(np.float64)


def _reference(state, side, row_ptr, ids, x, n_iter, sigma2=SIGMA2, eta2=ETA2, eta_b2=ETA_B2):
    """The literal alternation of the issue in float64, per row, ratings in the given order."""
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR
    other = 1 - side
    M, V = state["arrays"][(other, ARR_FACTOR)], state["arrays"][(other, ARR_COV)]
    b_o = state["arrays"][(other, ARR_BIAS)] if state["bias"] else None
    K, n_rows = M.shape[1], len(row_ptr) - 1
    mean, cov, bias = np.zeros((n_rows, K)), np.zeros((n_rows, K, K)), np.zeros(n_rows)
    for r in range(n_rows):
        o, xr = ids[row_ptr[r]:row_ptr[r + 1]], x[row_ptr[r]:row_ptr[r + 1]]
        n = len(o)
        if n == 0:
            cov[r] = eta2 * np.eye(K)
            continue
        m_j = M[o]
        S = np.zeros((K, K))
        for j in range(n):
            S += V[o[j]] + np.outer(m_j[j], m_j[j])
        Vr = np.linalg.inv(np.eye(K) / eta2 + S / sigma2)
        res = xr - (b_o[o] if state["bias"] else 0.0)
        b = 0.0
        for _ in range(n_iter if state["bias"] else 1):
            m = Vr @ (m_j.T @ (res - b)) / sigma2
            if state["bias"]:
                b = np.sum(res - m_j @ m) / (sigma2 * (1.0 / eta_b2 + n / sigma2))
        mean[r], cov[r], bias[r] = m, Vr, b
    return mean, cov, bias


def _errors(got, want):
    """(max abs on the means, max over rows of the covariance error relative to the row's largest entry, max abs on
    the biases)"""
    scale = np.abs(want[1]).max(axis=(1, 2), keepdims=True)
    return max_abs(got[0], want[0]), float(np.max(np.abs(got[1] - want[1]) / scale)), max_abs(got[2], want[2])


def _check(got, want, tol, what):
    errs = _errors(got, want)
    print(what, "mean %.3g cov %.3g bias %.3g (bound %.1g)" % (errs + (tol,)))
    assert max(errs) <= tol, (what, errs)
    assert np.array_equal(got[1], np.swapaxes(got[1], 1, 2)), what


CASES = [(K, "f32") for K in (1, 5, 8, 16, 33, 64, 72, 128, 136)] + [(K, "f64") for K in (5, 16, 64, 72)]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("K,dtype", CASES)
def test_parity_with_the_literal_alternation(K, dtype, bias):
    """Both sides, n_iter 1 / 3 / 10: every accumulate kernel (MFMA K <= 64, two-wave MFMA K <= 128, generic for fp64
    and K > 128), every solver range, rows of 0 .. 700 ratings (whole-row tasks, 64-rating batch edges, a split row)."""
    from pmf_hip import ITEM, USER
    state = _fitted_state(K, dtype, bias)
    with _open(state, K, dtype) as ctx:
        for side in (USER, ITEM):
            row_ptr, ids, x = _batch(7 + side, state["dims"][1 - side])
            for n_iter in (1, 3, 10):
                got = ctx.gauss_fold_in(side, row_ptr, ids, x, SIGMA2, ETA2, ETA_B2, n_iter)
                want = _reference(state, side, row_ptr, ids, x, n_iter)
                _check(got, want, _tol(K, dtype), f"K={K} {dtype} bias={bias} side={side} n_iter={n_iter}")
                # the row without ratings is the prior, exactly
                assert np.array_equal(got[0][0], np.zeros(K)) and np.array_equal(got[1][0], ETA2 * np.eye(K)) and got[2][0] == 0.0
                if not bias:
                    assert np.array_equal(got[2], np.zeros(len(LENGTHS)))


def test_covariance_rows_are_gathered_once_whatever_n_iter():
    from pmf_hip import USER
    state = _fitted_state(16, "f32", True)
    row_ptr, ids, x = _batch(7, state["dims"][1])
    with _open(state, 16, "f32") as ctx:
        ctx.prof_enable(True)
        counts = []
        for n_iter in (1, 10):
            ctx.prof_reset()
            ctx.gauss_fold_in(USER, row_ptr, ids, x, SIGMA2, ETA2, ETA_B2, n_iter)
            prof = ctx.prof_get()
            counts.append({k: prof[k][1] for k in ("gauss_accum", "gauss_combine", "gauss_solve", "gauss_bias")})
        assert counts[0] == counts[1] == {"gauss_accum": 1, "gauss_combine": 1, "gauss_solve": 1, "gauss_bias": 1}, counts


@pytest.mark.parametrize("K,dtype,tol", [(16, "f64", 1e-10), (16, "f32", 3e-5), (64, "f32", 3e-5)])
def test_folding_in_the_training_rows_is_the_user_half_sweep(K, dtype, tol):
    """Every user's own training ratings, n_iter = 1, against `gauss_factor_sweep(USER)` + `gauss_bias_sweep(USER)` from
    a zero user bias: the same posterior (f32: the bound of test_mfma_kernel_matches_generic_kernel)."""
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, USER
    state = _fitted_state(K, dtype, True)
    U = state["dims"][0]
    u, i, x = state["ratings"]
    order = np.argsort(u, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=U))])
    with _open(state, K, dtype) as ctx:
        ctx.set_array(USER, ARR_BIAS, np.zeros(U))
        got = ctx.gauss_fold_in(USER, row_ptr, i[order], x[order], SIGMA2, ETA2, ETA_B2, 1)
        ctx.gauss_factor_sweep(USER, SIGMA2, ETA2)
        ctx.gauss_bias_sweep(USER, SIGMA2, ETA_B2)
        want = tuple(ctx.get_array(USER, a) for a in (ARR_FACTOR, ARR_COV, ARR_BIAS))
    rated = np.diff(row_ptr) > 0
    assert rated.sum() > 100 and not rated.all()
    errs = [max_abs(g[rated], w[rated]) for g, w in zip(got, want)]
    print(f"K={K} {dtype} mean %.3g cov %.3g bias %.3g (bound {tol})" % tuple(errs))
    assert max(errs) <= tol, errs


def test_the_context_is_only_read():
    from pmf_hip import ITEM, USER
    state = _fitted_state(16, "f32", True)
    u, i, x = state["ratings"]
    with _open(state, 16, "f32") as ctx:
        assert ctx.eval_set(u[:500], i[:500], x[:500])
        before = ctx.eval_run(True, 0.25)
        for side in (USER, ITEM):
            row_ptr, ids, xs = _batch(3, state["dims"][1 - side])
            ctx.gauss_fold_in(side, row_ptr, ids, xs, SIGMA2, ETA2, ETA_B2, 3)
        assert len(state["arrays"]) == 6
        for (side, array), host in state["arrays"].items():
            assert np.array_equal(ctx.get_array(side, array), host), (side, array)
        assert ctx.eval_run(True, 0.25) == before
        # ... and the work lists still drive the same sweep
        ctx.gauss_factor_sweep(USER, SIGMA2, ETA2)
        with _open(state, 16, "f32") as fresh:
            fresh.gauss_factor_sweep(USER, SIGMA2, ETA2)
            assert np.array_equal(ctx.get_array(USER, 0), fresh.get_array(USER, 0))


def test_row_blocks_give_the_same_bits(monkeypatch):
    from pmf_hip import USER
    state = _fitted_state(16, "f32", True)
    rng = np.random.default_rng(11)
    lengths = rng.integers(0, 90, 70)
    lengths[[3, 40]] = 0
    lengths[33] = 300
    row_ptr, ids, x = _batch(12, state["dims"][1], lengths)
    with _open(state, 16, "f32") as ctx:
        whole = ctx.gauss_fold_in(USER, row_ptr, ids, x, SIGMA2, ETA2, ETA_B2, 3)
    monkeypatch.setenv("PMF_FOLD_IN_ROWS", "32")
    with _open(state, 16, "f32") as ctx:
        ctx.prof_enable(True)
        blocks = ctx.gauss_fold_in(USER, row_ptr, ids, x, SIGMA2, ETA2, ETA_B2, 3)
        assert ctx.prof_get()["gauss_solve"][1] == 3           # 32 + 32 + 6 rows
    for a, b in zip(whole, blocks):
        assert np.array_equal(a, b)
    _check(whole, _reference(state, USER, row_ptr, ids, x, 3), 2e-4, "70 rows")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("chunk", [64, 512])
def test_task_length_changes_the_summation_order_only(chunk, dtype, monkeypatch):
    """PMF_TASK_CHUNK = 64: the 129 and 700 rows are split rows of 64-rating batches; 512: only the 700 row is split."""
    from pmf_hip import USER
    state = _fitted_state(16, dtype, True)
    row_ptr, ids, x = _batch(7, state["dims"][1])
    monkeypatch.setenv("PMF_TASK_CHUNK", str(chunk))
    with _open(state, 16, dtype) as ctx:
        assert ctx.task_max_len(USER, "gauss") > 32
        got = ctx.gauss_fold_in(USER, row_ptr, ids, x, SIGMA2, ETA2, ETA_B2, 3)
    _check(got, _reference(state, USER, row_ptr, ids, x, 3), _tol(16, dtype), f"chunk {chunk} {dtype}")


def test_errors_leave_the_outputs_alone():
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    lib = pmf_hip.load()
    K = 8
    state = _fitted_state(K, "f32", True)
    U, I = state["dims"]
    row_ptr, ids, x = _batch(7, I, (3, 0, 4))
    n = 3
    out_f, out_c, out_b = np.full((n, K), 7.0), np.full((n, K, K), 7.0), np.full(n, 7.0)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(C.POINTER(t))

    def call(h, side=USER, n_rows=n, rp=row_ptr, o=ids, xs=x, s2=SIGMA2, e2=ETA2, eb2=ETA_B2, n_iter=1, f=out_f, c=out_c, b=out_b):
        return lib.pmf_gauss_fold_in(h, side, n_rows, ptr(rp, C.c_int64), ptr(o, C.c_int32), ptr(xs, C.c_double), s2, e2, eb2,
                                     n_iter, ptr(f, C.c_double), ptr(c, C.c_double), ptr(b, C.c_double))

    def refused(code, fragment, **kw):
        h = kw.pop("h", ctx._h)
        assert call(h, **kw) == code, (kw, lib.pmf_last_error())
        msg = lib.pmf_last_error().decode()
        assert msg.startswith("pmf_gauss_fold_in:") and fragment in msg, msg
        assert (out_f == 7.0).all() and (out_c == 7.0).all() and (out_b == 7.0).all(), kw

    with _open(state, K, "f32") as ctx:
        refused(PMF_EINVAL, "null context", h=None)
        refused(PMF_EINVAL, "null context", h=None, n_rows=0)
        refused(PMF_EINVAL, "bad side", side=2)
        refused(PMF_EINVAL, "negative", n_rows=-1)
        for name in ("rp", "o", "xs", "f"):
            refused(PMF_EINVAL, "null argument", **{name: None})
        refused(PMF_EINVAL, "row_ptr[0]", rp=row_ptr + 1)
        refused(PMF_EINVAL, "decreases", rp=np.array([0, 5, 3, 7], dtype=np.int64))
        for name in ("s2", "e2", "eb2"):
            refused(PMF_EINVAL, "variances", **{name: 0.0})
            refused(PMF_EINVAL, "variances", **{name: -1.0})
        refused(PMF_EINVAL, "n_iter", n_iter=0)
        bad = ids.copy()
        bad[-1] = I                          # the last position of the last row
        refused(PMF_ERANGE, f"id {I} at position {len(ids) - 1}", o=bad)
        bad[-1] = -1
        refused(PMF_ERANGE, "id -1", o=bad)
        refused(PMF_ERANGE, f"id {U} at position 0", side=ITEM, o=np.full_like(ids, U))   # the opposite side of ITEM is the users
        # n_rows = 0 with a valid context: success, nothing touched (the arrays may then be null)
        assert call(ctx._h, n_rows=0) == 0 and call(ctx._h, n_rows=0, rp=None, o=None, xs=None, f=None, c=None, b=None) == 0
        assert (out_f == 7.0).all() and (out_c == 7.0).all() and (out_b == 7.0).all()
        # the optional outputs
        assert call(ctx._h, c=None, b=None) == 0
        assert (out_c == 7.0).all() and (out_b == 7.0).all()
        want = _reference(state, USER, row_ptr, ids, x, 1)
        assert max_abs(out_f, want[0]) <= 2e-4
        assert call(ctx._h) == 0
        _check((out_f, out_c, out_b), want, 2e-4, "raw call")
    out_f[:], out_c[:], out_b[:] = 7.0, 7.0, 7.0
    # the opposite side's FACTOR and COV are needed (and named); those of `side` itself are not
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        refused(PMF_EINVAL, "array FACTOR of side 1")
        ctx.set_array(ITEM, ARR_FACTOR, state["arrays"][(ITEM, ARR_FACTOR)])
        refused(PMF_EINVAL, "array COV of side 1")
        ctx.set_array(ITEM, ARR_COV, state["arrays"][(ITEM, ARR_COV)])
        assert call(ctx._h) == 0                        # no BIAS arrays: the bias-free posterior, out_bias zeros
        assert np.array_equal(out_b, np.zeros(n))
        free = dict(state, bias=False)
        _check((out_f, out_c, out_b), _reference(free, USER, row_ptr, ids, x, 1), 2e-4, "no arrays of the side itself")


def _model(bias, K=16):
    import pandas as pd
    if bias:
        from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    else:
        from src.models.gaussian_mf_cavi import GaussianMFCAVI, GaussianMFCAVIConfig
    u, i, x = skewed_problem(100 + K, 600, 120, 12000, "centered")
    kw = dict(n_factors=K, sigma2=SIGMA2, eta_theta2=ETA2, eta_beta2=0.7, max_iter=3, tol=0.0, random_state=3, verbose=False)
    if bias:
        kw["eta_bias2"] = 2.0
    return GaussianMFCAVI(GaussianMFCAVIConfig(**kw)).fit(pd.DataFrame({"u": u, "i": i, "rating": x}))


def _model_state(m, bias):
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER
    arrays = {(USER, ARR_FACTOR): m.m_theta, (ITEM, ARR_FACTOR): m.m_beta, (USER, ARR_COV): m.V_theta, (ITEM, ARR_COV): m.V_beta}
    if bias:
        arrays.update({(USER, ARR_BIAS): m.m_user_bias, (ITEM, ARR_BIAS): m.m_item_bias})
    return {"arrays": arrays, "bias": bias}


def test_model_surface():
    """`fold_in_users` of a frame with string labels (interleaved, so grouping must keep each user's frame order) and
    one item id the fit has not seen; `fold_in_items`; `FoldIn.predict`; the bias-free class."""
    import pandas as pd
    from pmf_hip import ITEM, USER
    rng = np.random.default_rng(2)
    m = _model(True)
    n = 90
    labels = rng.choice(np.array(["zed", "amy", "bob"]), n)
    items = rng.integers(0, m.n_items, n)
    items[17] = m.n_items + 5                                   # unseen: dropped
    ratings = rng.integers(-2, 3, n).astype(float)
    fold = m.fold_in_users(pd.DataFrame({"u": labels, "i": items, "rating": ratings}), return_cov=True)
    assert list(fold.ids) == ["amy", "bob", "zed"]
    keep = np.arange(n) != 17
    rows = [np.flatnonzero((labels == name) & keep) for name in fold.ids]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    pos = np.concatenate(rows)
    state = _model_state(m, True)
    want = _reference(state, USER, row_ptr, items[pos], ratings[pos], 10, eta2=ETA2, eta_b2=2.0)
    _check((fold.mean, fold.cov, fold.bias), want, 2e-4, "fold_in_users")
    assert m.fold_in_users(pd.DataFrame({"u": labels, "i": items, "rating": ratings})).cov is None
    q_rows, q_items = np.array([2, 0, 1, 1]), np.array([0, 5, 7, m.n_items - 1])
    formula = np.einsum("nk,nk->n", fold.mean[q_rows], m.m_beta[q_items]) + fold.bias[q_rows] + m.m_item_bias[q_items] + 3.25
    assert max_abs(fold.predict(q_rows, q_items, 3.25), formula) <= 1e-14
    # items: integer labels far outside the trained range, the item prior variance
    users = rng.integers(0, m.n_users, 40)
    new_items = rng.choice(np.array([10**6, 777777]), 40)
    fi = m.fold_in_items(pd.DataFrame({"u": users, "i": new_items, "rating": ratings[:40]}), n_iter=3, return_cov=True)
    assert list(fi.ids) == [777777, 10**6]
    rows = [np.flatnonzero(new_items == name) for name in fi.ids]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    pos = np.concatenate(rows)
    want = _reference(state, ITEM, row_ptr, users[pos], ratings[:40][pos], 3, eta2=0.7, eta_b2=2.0)
    _check((fi.mean, fi.cov, fi.bias), want, 2e-4, "fold_in_items")
    m.close()
    free = _model(False)
    fold = free.fold_in_users(pd.DataFrame({"u": labels, "i": items, "rating": ratings}), n_iter=4, return_cov=True)
    assert np.array_equal(fold.bias, np.zeros(3))
    rows = [np.flatnonzero((labels == name) & keep) for name in fold.ids]
    pos = np.concatenate(rows)
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    want = _reference(_model_state(free, False), USER, row_ptr, items[pos], ratings[pos], 4, eta2=ETA2)
    _check((fold.mean, fold.cov, fold.bias), want, 2e-4, "bias-free fold_in_users")
    assert np.array_equal(fold.predict([0, 2], [1, 1]), np.einsum("nk,nk->n", fold.mean[[0, 2]], free.m_beta[[1, 1]]))
    free.close()
