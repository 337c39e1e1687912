"""Unlisted cells as weighted zeros in the bias-free Gaussian model on the device (pmf_ctx_set_gauss_zeros /
PMF_ZEROS_OBSERVED, pmf_gauss_gram, `fit(unobserved="zero", zero_weight=)`) against dense float64 NumPy
(tests/gauss_implicit_reference.py).  State is read back from the device before the reference is evaluated, so the
rounding of the inputs is not in the error.

Bounds.
  Gram.  Every addend V_r[p] + m_r m_c is one fma in double from the stored values and the R addends of an entry are
  added in double in a fixed tree (rows of a wavefront, four wavefronts, row blocks): at most R + 1 roundings, the
  reference's own R + 1 in another order:  |got - ref| <= (R + 2) 2^-53 sum_r (|V_r[p]| + |m_r m_c|).
  Half-sweeps, fold-in.  The project's own bars for these solvers (tests/test_fold_in_gpu.py): f64 1e-10, f32 2e-4
  (3e-4 at K = 136), max abs on means, relative to the row's largest entry on covariances.
  ELBO terms.  f64: rtol 1e-10 on every term and row.  f32: SQNORM / LOGDET as in tests/test_elbo_gpu.py; ESS its bound
  with c_acc + 3 (the blend adds the roundings of 1 - w0 and of w0 G and one fma), on the magnitude with
  (1 - w0) |S| + w0 |G| in the place of |S|; the reference's own rounding counts the rows of the other side too (G).
No tolerance below is a number found by running the kernel."""
import ctypes as C
import multiprocessing as mp
import os
import sys

import numpy as np
import pandas as pd
import pytest

import gauss_implicit_reference as zref
from helpers import max_abs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PMF_EINVAL = -1
U, I, N = 90, 70, 4000
SIGMA2, ETA_T, ETA_B = 0.3, 0.5, 0.5
CASES = [(K, dtype) for K in (3, 20, 64, 100, 136) for dtype in ("f32", "f64")]
U32 = 2.0 ** -24


def _tol(K, dtype):
    return 1e-10 if dtype == "f64" else (3e-4 if K == 136 else 2e-4)


def _spd_rows(rng, rows, K):
    A = rng.standard_normal((rows, K, K))
    return A @ A.transpose(0, 2, 1) / K + 0.1 * np.eye(K)


_PROBLEMS = {}


def _problems():
    if not _PROBLEMS:
        P = zref.problem_p(5, U, I, N)
        _PROBLEMS["P"], _PROBLEMS["D"] = P, zref.dense_completion(*P, U, I)
    return _PROBLEMS["P"], _PROBLEMS["D"]


def _state(ctx):
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    return {"m_theta": ctx.get_array(USER, ARR_FACTOR), "V_theta": ctx.get_array(USER, ARR_COV),
            "m_beta": ctx.get_array(ITEM, ARR_FACTOR), "V_beta": ctx.get_array(ITEM, ARR_COV)}


def _upload(ctx, st):
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    ctx.set_array(USER, ARR_FACTOR, st["m_theta"])
    ctx.set_array(USER, ARR_COV, st["V_theta"])
    ctx.set_array(ITEM, ARR_FACTOR, st["m_beta"])
    ctx.set_array(ITEM, ARR_COV, st["V_beta"])


def _bits(ctx):
    return [a.tobytes() for a in _state(ctx).values()]


def _context(K, dtype, problem, seed=3):
    """a context with the problem's ratings and the reference's initial state"""
    import pmf_hip
    ctx = pmf_hip.Context(U, I, K, dtype=dtype)
    ctx.set_ratings(*problem)
    _upload(ctx, zref.initial_state(seed, U, I, K))
    return ctx


_FITTED = {}


def _fitted(K, dtype):
    """the state of P after two default device iterations, as read back (computed once per K and dtype)"""
    from pmf_hip import ITEM, USER
    if (K, dtype) not in _FITTED:
        with _context(K, dtype, _problems()[0]) as ctx:
            for _ in range(2):
                ctx.gauss_factor_sweep(USER, SIGMA2, ETA_T)
                ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA_B)
            _FITTED[(K, dtype)] = _state(ctx)
    return _FITTED[(K, dtype)]


def _errors(got_m, got_V, want_m, want_V):
    scale = np.abs(want_V).max(axis=(1, 2), keepdims=True)
    return max_abs(got_m, want_m), float(np.max(np.abs(got_V - want_V) / scale))


def _sides():
    from pmf_hip import ITEM, USER
    (u, i, x), _ = _problems()
    return ((USER, "theta", "beta", u, i, ETA_T), (ITEM, "beta", "theta", i, u, ETA_B))


# ---- 1. Gram against NumPy ------------------------------------------------------------------------------------------
def _gram_case(K, dtype, rows, seed=None):
    """G of a user side of `rows` rows with random means and a different SPD matrix per row: (got, state read back, the
    context's checks run on the way)"""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, USER
    rng = np.random.default_rng(1000 * K + rows if seed is None else seed)
    with pmf_hip.Context(rows, 2, K, dtype=dtype) as ctx:
        ctx.set_array(USER, ARR_FACTOR, rng.standard_normal((rows, K)))
        ctx.set_array(USER, ARR_COV, _spd_rows(rng, rows, K))
        m, V = ctx.get_array(USER, ARR_FACTOR), ctx.get_array(USER, ARR_COV)
        got = ctx.gauss_gram(USER)
        held = ctx.device_bytes()
        again = ctx.gauss_gram(USER)
        assert ctx.device_bytes() == held                         # grows on the first call only
        assert got.tobytes() == again.tobytes()
        assert ctx.get_array(USER, ARR_FACTOR).tobytes() == m.tobytes() and ctx.get_array(USER, ARR_COV).tobytes() == V.tobytes()
        assert ctx.gauss_zeros == (False, 1.0)                    # works in the default mode
    return got, m, V


def _check_gram(got, m, V, what):
    want, mag = zref.gram(m, V)
    bound = (len(m) + 2) * 2.0 ** -53 * mag
    err = np.abs(got - want)
    print(f"{what}: Gram err {err.max():.3g} (bound {bound[err.argmax() // len(want), err.argmax() % len(want)]:.3g})")
    assert (err <= bound).all(), (what, float((err / bound).max()))
    assert np.array_equal(got, got.T), what


@pytest.mark.parametrize("K,dtype", CASES)
def test_gram_against_numpy(K, dtype):
    for rows in (1, 255, 256, 257):
        _check_gram(*_gram_case(K, dtype, rows), f"K={K} {dtype} rows={rows}")


@pytest.mark.parametrize("K,dtype", [(K, dtype) for K in (3, 20) for dtype in ("f32", "f64")])
def test_gram_of_many_rows(K, dtype):
    """20011 rows: more rows than row blocks, ranges of 19 and 20 rows, every wavefront with several batches"""
    _check_gram(*_gram_case(K, dtype, 20011), f"K={K} {dtype} rows=20011")


def _gram_worker(out_path):
    """A fresh interpreter with another task length: the Gram matrices of every case at 257 rows, and of the fitted P."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd"), os.path.join(ROOT, "tests")]
    os.environ["PMF_TASK_CHUNK"] = "64"
    out = {}
    for K, dtype in CASES:
        out[f"{K}_{dtype}"] = _gram_case(K, dtype, 257)[0]
    out["P"], out["longest"] = _gram_of_p()
    np.savez(out_path, **out)


def _gram_of_p():
    from pmf_hip import ITEM, USER
    with _context(20, "f32", _problems()[0]) as ctx:
        return ctx.gauss_gram(ITEM), np.array([ctx.task_max_len(s, "gauss") for s in (USER, ITEM)])


def test_gram_does_not_depend_on_the_task_length(tmp_path, monkeypatch):
    monkeypatch.delenv("PMF_TASK_CHUNK", raising=False)
    path = str(tmp_path / "gram.npz")
    proc = mp.get_context("spawn").Process(target=_gram_worker, args=(path,))
    proc.start()
    proc.join(120)
    if proc.is_alive():
        proc.kill()
        proc.join()
        raise AssertionError("the child hung")
    assert proc.exitcode == 0
    child = np.load(path)
    for K, dtype in CASES:
        assert child[f"{K}_{dtype}"].tobytes() == _gram_case(K, dtype, 257)[0].tobytes(), (K, dtype)
    here, longest = _gram_of_p()
    assert longest.max() <= 32 and child["longest"].min() > 32, (longest, child["longest"])
    assert child["P"].tobytes() == here.tobytes()


# ---- 2. half-sweeps against NumPy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", CASES)
def test_half_sweeps_against_numpy(K, dtype):
    """Problem P from the state after two default device iterations; both sides, three weights; every row and element."""
    from pmf_hip import ARR_COV, ARR_FACTOR
    st = _fitted(K, dtype)
    (u, i, x), _ = _problems()
    tol = _tol(K, dtype)
    with _context(K, dtype, (u, i, x)) as ctx:
        for w0 in (1.0, 0.25, 0.025):
            ctx.set_gauss_zeros(True, w0)
            assert ctx.gauss_zeros == (True, w0)
            for side, name, other, ids, oids, eta2 in _sides():
                _upload(ctx, st)
                ctx.gauss_factor_sweep(side, SIGMA2, eta2)
                got_m, got_V = ctx.get_array(side, ARR_FACTOR), ctx.get_array(side, ARR_COV)
                want_m, want_V = zref.half_sweep(st["m_" + other], st["V_" + other], ids, oids, x, len(got_m), SIGMA2, eta2, w0)
                errs = _errors(got_m, got_V, want_m, want_V)
                print(f"K={K} {dtype} w0={w0} side={side}: mean {errs[0]:.3g} cov {errs[1]:.3g} (bar {tol:.1g})")
                assert max(errs) <= tol, (w0, side, errs)
                empty = np.bincount(ids, minlength=len(got_m)) == 0
                assert empty.sum() in (2, 3) and (got_m[empty] == 0.0).all()
                # the other side is not written
                assert ctx.get_array(1 - side, ARR_FACTOR).tobytes() == st["m_" + other].tobytes()
                assert ctx.get_array(1 - side, ARR_COV).tobytes() == st["V_" + other].tobytes()


# ---- 3. the dense identity on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", CASES)
def test_zero_mode_on_the_sparse_list_is_the_default_mode_on_the_dense_list(K, dtype):
    """w0 = 1 on P against the default mode on D (every row has 70 / 90 ratings), same initial state, one half-sweep per
    side: no reference at all.  Within the sum of the two bars."""
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    P, D = _problems()
    with _context(K, dtype, P) as zp, _context(K, dtype, D) as dd:
        zp.set_gauss_zeros(True, 1.0)
        for side, eta2 in ((USER, ETA_T), (ITEM, ETA_B)):
            zp.gauss_factor_sweep(side, SIGMA2, eta2)
            dd.gauss_factor_sweep(side, SIGMA2, eta2)
            errs = _errors(zp.get_array(side, ARR_FACTOR), zp.get_array(side, ARR_COV), dd.get_array(side, ARR_FACTOR),
                           dd.get_array(side, ARR_COV))
            print(f"K={K} {dtype} side={side}: mean {errs[0]:.3g} cov {errs[1]:.3g} (bar {2 * _tol(K, dtype):.1g})")
            assert max(errs) <= 2 * _tol(K, dtype), (side, errs)


# ---- 4. fold-in -----------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 31, 32, 33, 65, 129)


def _batch(seed, n_other):
    rng = np.random.default_rng(seed)
    row_ptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    ids = rng.integers(0, n_other, row_ptr[-1]).astype(np.int32)
    return row_ptr, ids, rng.integers(-1, 5, row_ptr[-1]).astype(np.float64)


@pytest.mark.parametrize("K,dtype", [(K, dtype) for K in (20, 64, 100) for dtype in ("f32", "f64")])
def test_fold_in_against_numpy(K, dtype):
    st = _fitted(K, dtype)
    tol = _tol(K, dtype)
    with _context(K, dtype, _problems()[0]) as ctx:
        _upload(ctx, st)
        before = _bits(ctx)
        for w0 in (1.0, 0.1):
            ctx.set_gauss_zeros(True, w0)
            for side, name, other, _, _, eta2 in _sides():
                m_o, V_o = st["m_" + other], st["V_" + other]
                row_ptr, ids, x = _batch(11 + side, len(m_o))
                got_m, got_V, got_b = ctx.gauss_fold_in(side, row_ptr, ids, x, SIGMA2, eta2)
                want_m, want_V = zref.fold_in(m_o, V_o, row_ptr, ids, x, SIGMA2, eta2, w0)
                errs = _errors(got_m, got_V, want_m, want_V)
                print(f"K={K} {dtype} w0={w0} side={side}: mean {errs[0]:.3g} cov {errs[1]:.3g} (bar {tol:.1g})")
                assert max(errs) <= tol, (w0, side, errs)
                assert np.array_equal(got_V, np.swapaxes(got_V, 1, 2)) and (got_b == 0.0).all()
                # the row without ratings: mean 0, inv(I / eta2 + w0 G / sigma2), which is not the prior
                G, _ = zref.gram(m_o, V_o)
                empty_V = np.linalg.inv(np.eye(K) / eta2 + w0 * G / SIGMA2)
                assert (got_m[0] == 0.0).all()
                assert np.max(np.abs(got_V[0] - empty_V)) <= tol * np.abs(empty_V).max()
                assert np.max(np.abs(got_V[0] - eta2 * np.eye(K))) > 0.1 * eta2
        assert _bits(ctx) == before                                # the context is only read


# ---- 5. ELBO terms --------------------------------------------------------------------------------------------------
def _elbo_bounds(ctx, K, dtype, side, terms, mag, m, V, n, rows_other):
    """(rows, 4) bounds of the four terms (module docstring; the f32 forms are tests/test_elbo_gpu.py's)"""
    import test_elbo_gpu as eg
    out = np.zeros((len(n), 4))
    if dtype == "f64":
        out[:] = 1e-10 * np.abs(terms)
        return out
    chunks, L = ctx.cov_stride // 4, 64 if K <= 64 else 256
    per_lane, per_k = -(-chunks // L), -(-K // L)
    T = ctx.task_max_len(side, "gauss")
    n_slots = int(np.max(np.where(n > T, -(-n // max(T, 1)), 0)))
    out[:, zref.SQNORM] = eg._gamma(2 * per_lane + per_k + 9) * ((m * m).sum(axis=1) + np.abs(np.diagonal(V, axis1=1, axis2=2)).sum(axis=1))
    out[:, zref.LOGDET] = eg._logdet_bound(V, K, terms[:, zref.LOGDET])
    c_ess = (2 * T + 6 + n_slots + 3) + (1 + per_lane + 2 + per_k + 10)
    out[:, zref.ESS] = (eg._gamma(c_ess) + 4.0 * (K * K + n + rows_other) * 2.0 ** -53) * mag
    return out


@pytest.mark.parametrize("K,dtype", CASES)
def test_elbo_terms_against_numpy(K, dtype):
    from pmf_hip import ELBO_ESS
    st = _fitted(K, dtype)
    (u, i, x), D = _problems()
    with _context(K, dtype, (u, i, x)) as ctx:
        _upload(ctx, st)
        plain = [ctx.gauss_elbo_terms(side, with_data=False, per_row=True) for side in (0, 1)]
        for w0 in (1.0, 0.25):
            ctx.set_gauss_zeros(True, w0)
            ess, slack = [], []
            for side, name, other, ids, oids, _ in _sides():
                m, V = st["m_" + name], st["V_" + name]
                want, mag = zref.side_terms(m, V, st["m_" + other], st["V_" + other], ids, oids, x, w0)
                n = np.bincount(ids, minlength=len(m))
                bound = _elbo_bounds(ctx, K, dtype, side, want, mag, m, V, n, len(st["m_" + other]))
                totals, rows = ctx.gauss_elbo_terms(side, with_data=True, per_row=True)
                err = np.abs(rows - want)
                names = ("SQNORM", "LOGDET", "BIAS_SQ", "ESS")
                print(f"K={K} {dtype} w0={w0} side={side}: " + ", ".join(f"{names[t]} err {err[:, t].max():.3g} (bound {bound[:, t].max():.3g})" for t in range(4)))
                for t in range(4):
                    bad = np.flatnonzero(~(err[:, t] <= bound[:, t]))
                    assert bad.size == 0, f"{names[t]} of row {bad[0]}: got {rows[bad[0], t]!r}, want {want[bad[0], t]!r}, bound {bound[bad[0], t]:.3g}"
                assert (rows[n == 0, ELBO_ESS] > 0.0).all()          # a row without ratings has an ESS: <V, w0 G>
                acc = np.zeros(4)
                for r in range(len(rows)):
                    acc += rows[r]
                assert np.array_equal(totals, acc)
                again = ctx.gauss_elbo_terms(side, with_data=True, per_row=True)
                assert again[0].tobytes() == totals.tobytes() and again[1].tobytes() == rows.tobytes()
                # without data nothing changes
                nodata = ctx.gauss_elbo_terms(side, with_data=False, per_row=True)
                assert nodata[0].tobytes() == plain[side][0].tobytes() and nodata[1].tobytes() == plain[side][1].tobytes()
                ess.append(totals[ELBO_ESS])
                slack.append(bound[:, zref.ESS].sum())
            assert abs(ess[0] - ess[1]) <= (1e-10 * abs(ess[0]) if dtype == "f64" else slack[0] + slack[1]), (w0, ess)
            if dtype == "f64" and w0 == 1.0:
                with _context(K, dtype, D) as dd:
                    _upload(dd, st)
                    dense = dd.gauss_elbo_terms(0, with_data=True)[ELBO_ESS]
                assert abs(ess[0] - dense) <= 1e-10 * abs(dense) and abs(ess[1] - dense) <= 1e-10 * abs(dense)


# ---- 6. model surface, f64 ------------------------------------------------------------------------------------------
def _frame(problem):
    u, i, x = problem
    return pd.DataFrame({"u": u, "i": i, "rating": x})


def _model(K=6, dtype="f64", max_iter=5, **kw):
    from src.models.gaussian_mf_cavi import GaussianMFCAVI, GaussianMFCAVIConfig
    cfg = dict(n_factors=K, sigma2=SIGMA2, eta_theta2=ETA_T, eta_beta2=0.7, max_iter=max_iter, tol=0.0, random_state=1, verbose=False)
    cfg.update(kw)
    return GaussianMFCAVI(GaussianMFCAVIConfig(**cfg), dtype=dtype)


def test_fit_in_zero_mode_is_the_default_fit_of_the_dense_frame():
    P, D = _problems()
    zero = _model().fit(_frame(P), unobserved="zero")
    dense = _model().fit(_frame(D))
    assert zero.history_["unobserved"] == "zero" and zero.history_["zero_weight"] == 1.0
    assert dense.history_["unobserved"] == "missing"
    for name in ("m_theta", "m_beta"):
        assert np.allclose(getattr(zero, name), getattr(dense, name), rtol=1e-9, atol=1e-12), name
    rows = np.arange(0, U, 7)
    assert np.allclose(zero.V_theta_rows(rows), dense.V_theta_rows(rows), rtol=1e-9, atol=1e-12)
    rows = np.arange(0, I, 5)
    assert np.allclose(zero.V_beta_rows(rows), dense.V_beta_rows(rows), rtol=1e-9, atol=1e-12)
    got, want = zero.elbo(), dense.elbo()
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    # the bound of the fitted state is the reference's, cell by cell
    st = {"m_theta": zero.m_theta, "V_theta": zero.V_theta, "m_beta": zero.m_beta, "V_beta": zero.V_beta}
    cells = zref.elbo_cells(st, *P, SIGMA2, ETA_T, 0.7, 1.0)
    assert abs(got - cells) <= 1e-9 * abs(cells), (got, cells)


def test_tracked_bound_never_falls_and_a_plain_fit_follows_with_a_fresh_models_bytes():
    P, _ = _problems()
    model = _model(max_iter=8).fit(_frame(P), unobserved="zero", zero_weight=0.1, track_elbo=True)
    trace = np.array(model.history_["elbo"])
    assert len(trace) == 8 and model.history_["zero_weight"] == 0.1
    assert (np.diff(trace) >= -1e-9 * np.abs(trace[:-1])).all(), np.diff(trace).min()
    assert trace[-1] > trace[0]
    st = {"m_theta": model.m_theta, "V_theta": model.V_theta, "m_beta": model.m_beta, "V_beta": model.V_beta}
    cells = zref.elbo_cells(st, *P, SIGMA2, ETA_T, 0.7, 0.1)
    assert abs(model.elbo() - cells) <= 1e-9 * abs(cells) and model.elbo() == trace[-1]
    # fold-in follows the mode of the fitted context: a user without ratings is not the prior
    fold = model.fold_in_users(pd.DataFrame({"u": [5, 5, 9], "i": [0, 3, 10_000], "rating": [1.0, 2.0, 1.0]}), return_cov=True)
    want_m, want_V = zref.fold_in(model.m_beta, model.V_beta, np.array([0, 2, 2]), np.array([0, 3]), np.array([1.0, 2.0]), SIGMA2, ETA_T, 0.1)
    assert np.allclose(fold.mean, want_m, rtol=1e-9, atol=1e-12) and np.allclose(fold.cov, want_V, rtol=1e-9, atol=1e-12)
    assert (fold.mean[1] == 0.0).all()
    model.fit(_frame(P))
    fresh = _model(max_iter=8).fit(_frame(P))
    assert model.history_["unobserved"] == "missing"
    for name in ("m_theta", "m_beta", "V_theta", "V_beta"):
        assert np.asarray(getattr(model, name)).tobytes() == np.asarray(getattr(fresh, name)).tobytes(), name
    assert model.elbo() == fresh.elbo()


# ---- 7. behaviour ---------------------------------------------------------------------------------------------------
def test_zero_mode_ranks_held_out_items_of_implicit_feedback():
    """Planted groups, every listed rating 1 (seed 0, fp32, K = 4, sigma2 = eta2 = 1, ten iterations): the default fit
    learns "predict 1 everywhere" and ranks the held-out items no better than chance among the unlisted ones; the
    zero-mode fit recovers the groups.  The float64 restatement gives recall@10 = 0.75 against 0.26 and a margin of at
    least 0.41 over four seeds: the bar is half of that."""
    (u, i, x), (hu, hi) = zref.planted_problem(0)
    train = pd.DataFrame({"u": u, "i": i, "rating": x})
    held = pd.DataFrame({"u": hu, "i": hi, "rating": np.ones(len(hu))})
    recall = {}
    for mode in ("missing", "zero"):
        model = _model(K=4, dtype="f32", max_iter=10, sigma2=1.0, eta_theta2=1.0, eta_beta2=1.0, random_state=0)
        model.fit(train, unobserved=mode)
        recall[mode] = model.evaluate_ranking(held, ks=(10,), exclude_train=True)["recall@10"]
    print(f"recall@10 without training items: default {recall['missing']:.3f}, zero mode {recall['zero']:.3f}")
    assert recall["zero"] - recall["missing"] >= 0.2, recall


# ---- 8. modes and refusals ------------------------------------------------------------------------------------------
def _refused(lib, status, *words):
    assert status == PMF_EINVAL
    message = lib.pmf_last_error().decode()
    for word in words:
        assert word in message, message


def test_calls_that_zero_mode_does_not_cover_are_refused_and_write_nothing():
    import torch
    import pmf_hip
    from helpers import gauss_stats, sgd_stats
    from pmf_hip import ARR_BIAS, ITEM, USER
    lib = pmf_hip.load()
    dp = C.POINTER(C.c_double)
    with _context(20, "f32", _problems()[0]) as ctx:
        h = ctx._h
        for mode, weight, word in ((2, 1.0, "bad mode"), (-1, 1.0, "bad mode"), (1, 0.0, "weight"), (1, -0.5, "weight"), (1, 1.5, "weight"),
                                   (1, float("nan"), "weight"), (1, float("inf"), "weight")):
            _refused(lib, lib.pmf_ctx_set_gauss_zeros(h, mode, weight), "pmf_ctx_set_gauss_zeros", word)
            assert ctx.gauss_zeros == (False, 1.0)
        ctx.set_gauss_zeros(False, 7.0)                             # the weight is ignored under MISSING
        assert ctx.gauss_zeros == (False, 1.0)
        ctx.set_gamma_zeros(True)                                   # the two switches are independent
        assert ctx.gauss_zeros == (False, 1.0)
        ctx.set_gauss_zeros(True, 0.5)
        assert ctx.gauss_zeros == (True, 0.5) and ctx.gamma_zeros is True
        ctx.set_gamma_zeros(False)
        assert ctx.gauss_zeros == (True, 0.5)
        factor, bias = gauss_stats(ctx, torch.device("cuda", 0))
        grad = sgd_stats(ctx, torch.device("cuda", 0))
        for t in (factor, bias, grad):
            t.tensor.fill_(7.0)
        before = _bits(ctx)
        p = lambda s: C.c_void_p(s.ptr)
        _refused(lib, lib.pmf_gauss_factor_accumulate(h, ITEM, p(factor)), "pmf_gauss_factor_accumulate", "pmf_ctx_set_gauss_zeros")
        _refused(lib, lib.pmf_gauss_factor_finalize(h, ITEM, p(factor), 0.3, 0.5), "pmf_gauss_factor_finalize", "pmf_ctx_set_gauss_zeros")
        _refused(lib, lib.pmf_gauss_bias_sweep(h, USER, 0.3, 1.0), "pmf_gauss_bias_sweep", "pmf_ctx_set_gauss_zeros")
        _refused(lib, lib.pmf_gauss_bias_accumulate(h, ITEM, p(bias)), "pmf_gauss_bias_accumulate", "pmf_ctx_set_gauss_zeros")
        _refused(lib, lib.pmf_gauss_bias_finalize(h, ITEM, p(bias), 0.3, 1.0), "pmf_gauss_bias_finalize", "pmf_ctx_set_gauss_zeros")
        _refused(lib, lib.pmf_gauss_sgd_sweep(h, USER, 0.01, 0.3, 0.5, 1.0), "pmf_gauss_sgd_sweep", "pmf_ctx_set_gauss_zeros")
        _refused(lib, lib.pmf_gauss_sgd_accumulate(h, ITEM, p(grad), 0.01, 0.3, 0.5, 1.0), "pmf_gauss_sgd_accumulate", "pmf_ctx_set_gauss_zeros")
        _refused(lib, lib.pmf_gauss_sgd_finalize(h, ITEM, p(grad)), "pmf_gauss_sgd_finalize", "pmf_ctx_set_gauss_zeros")
        _refused(lib, lib.pmf_ctx_get_gauss_zeros(h, None, None), "pmf_ctx_get_gauss_zeros")
        _refused(lib, lib.pmf_gauss_gram(h, USER, None), "pmf_gauss_gram", "null out")
        _refused(lib, lib.pmf_gauss_gram(h, 2, None), "pmf_gauss_gram", "bad side")
        ctx.sync()
        assert all(bool((t.tensor == 7.0).all()) for t in (factor, bias, grad)) and _bits(ctx) == before
        # both sides with a BIAS array: the three calls that follow the mode refuse
        for side in (USER, ITEM):
            ctx.set_array(side, ARR_BIAS, np.zeros(ctx.rows(side)))
        _refused(lib, lib.pmf_gauss_factor_sweep(h, USER, 0.3, 0.5), "pmf_gauss_factor_sweep", "bias", "pmf_ctx_set_gauss_zeros")
        tot = np.full(4, 7.0)
        _refused(lib, lib.pmf_gauss_elbo_terms(h, USER, 1, tot.ctypes.data_as(dp), None), "pmf_gauss_elbo_terms", "bias", "pmf_ctx_set_gauss_zeros")
        row_ptr, ids, x = _batch(3, I)
        out = np.full((len(LENGTHS), 20), 7.0)
        _refused(lib, lib.pmf_gauss_fold_in(h, USER, len(LENGTHS), pmf_hip.ptr(row_ptr, C.c_int64), pmf_hip.ptr(ids, C.c_int32),
                                            pmf_hip.ptr(x, C.c_double), 0.3, 0.5, 1.0, 1, out.ctypes.data_as(dp), None, None),
                 "pmf_gauss_fold_in", "bias", "pmf_ctx_set_gauss_zeros")
        ctx.sync()
        assert (tot == 7.0).all() and (out == 7.0).all() and _bits(ctx) == before
        # back in MISSING mode the same calls run
        ctx.set_gauss_zeros(False)
        assert ctx.gauss_zeros == (False, 0.5)                      # the getter returns the stored weight
        ctx.gauss_factor_accumulate(ITEM, factor.ptr)
        ctx.gauss_factor_finalize(ITEM, factor.ptr, 0.3, 0.5)
        ctx.gauss_bias_sweep(USER, 0.3, 1.0)
        ctx.sync()
    with pmf_hip.Context(5, 4, 3) as bare:
        out = np.full((3, 3), 7.0)
        _refused(lib, lib.pmf_gauss_gram(bare._h, USER, out.ctypes.data_as(dp)), "pmf_gauss_gram", "FACTOR")
        assert (out == 7.0).all()


def test_zero_mode_and_a_communicator_refuse_each_other():
    import pmf_hip
    from pmf_hip import PmfError, dist as pdist
    from pmf_hip.engine import Context
    lib = pmf_hip.load()
    comm = pdist.Comm(0, 1, 0, Context.comm_unique_id(), "rccl")
    try:
        with pmf_hip.Context(U, I, 8) as ctx:
            comm.attach(ctx)
            _refused(lib, lib.pmf_ctx_set_gauss_zeros(ctx._h, 1, 0.5), "pmf_ctx_set_gauss_zeros", "communicator")
            assert ctx.gauss_zeros == (False, 1.0)
            ctx.set_gauss_zeros(False)                              # the default stays available
        with pmf_hip.Context(U, I, 8) as ctx:
            ctx.set_gauss_zeros(True, 0.5)
            with pytest.raises(PmfError, match="pmf_comm_attach.*pmf_ctx_set_gauss_zeros"):
                comm.attach(ctx)
            with pytest.raises(PmfError, match="pmf_comm_init.*pmf_ctx_set_gauss_zeros"):
                ctx.comm_init(1, 0, Context.comm_unique_id())
            assert ctx.comm_info() == (1, 0, -1) and ctx.gauss_zeros == (True, 0.5)
            ctx.set_gauss_zeros(False)
            comm.attach(ctx)
            assert ctx.comm_info()[2] == pmf_hip.TRANSPORT_RCCL
    finally:
        comm.close()


def _hostshm_worker(out_path):
    """A fresh interpreter on the test build of the library: its rehearsal transport on a context in the mode."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd"), os.path.join(ROOT, "tests")]
    os.environ["PMF_HIP_TEST_LIBRARY"] = "1"
    import pmf_hip
    from pmf_hip import PmfError
    message = "not refused"
    with pmf_hip.Context(U, I, 8) as ctx:
        ctx.set_gauss_zeros(True, 0.5)
        try:
            ctx.comm_init(1, 0, bytes(pmf_hip.UNIQUE_ID_BYTES), transport="hostshm")
        except PmfError as e:
            message = str(e)
        info = ctx.comm_info()
    with open(out_path, "w") as f:
        f.write(f"{info}\n{message}")


def test_the_test_transport_refuses_a_context_in_zero_mode(tmp_path):
    path = str(tmp_path / "hostshm.txt")
    proc = mp.get_context("spawn").Process(target=_hostshm_worker, args=(path,))
    proc.start()
    proc.join(120)
    if proc.is_alive():
        proc.kill()
        proc.join()
        raise AssertionError("the child hung")
    assert proc.exitcode == 0
    info, message = open(path).read().split("\n", 1)
    assert info == "(1, 0, -1)" and "pmf_comm_init" in message and "pmf_ctx_set_gauss_zeros" in message, (info, message)


def _windows_case(K, dtype):
    """zero-mode sweeps of both sides and the ELBO terms of the fitted P, and a default sweep after the mode is unset"""
    from pmf_hip import ITEM, USER
    st = _fitted(K, dtype)
    out = []
    with _context(K, dtype, _problems()[0]) as ctx:
        _upload(ctx, st)
        ctx.set_gauss_zeros(True, 0.25)
        for side, eta2 in ((USER, ETA_T), (ITEM, ETA_B)):
            terms = ctx.gauss_elbo_terms(side, with_data=True, per_row=True)
            out += [terms[0].tobytes(), terms[1].tobytes()]
            ctx.gauss_factor_sweep(side, SIGMA2, eta2)
            out += _bits(ctx)
        ctx.set_gauss_zeros(False)
        _upload(ctx, st)
        for side, eta2 in ((USER, ETA_T), (ITEM, ETA_B)):
            terms = ctx.gauss_elbo_terms(side, with_data=True, per_row=True)
            out += [terms[0].tobytes(), terms[1].tobytes()]
            ctx.gauss_factor_sweep(side, SIGMA2, eta2)
        default = _bits(ctx)
    return out, default


@pytest.mark.parametrize("K,dtype", [(20, "f32"), (100, "f32"), (20, "f64")])
def test_row_windows_change_no_bit_and_unsetting_the_mode_restores_the_default(K, dtype, monkeypatch):
    """PMF_ELBO_ROWS = 17 (six / five windows; P's rows without ratings fall into windows with and without tasks) and
    one window: the same bits.  Mode set -> unset -> default calls: the bytes of a context that never had the mode."""
    from pmf_hip import ITEM, USER
    st = _fitted(K, dtype)
    monkeypatch.delenv("PMF_ELBO_ROWS", raising=False)
    one, default_one = _windows_case(K, dtype)
    with _context(K, dtype, _problems()[0]) as ctx:              # never in the mode
        _upload(ctx, st)
        never = []
        for side, eta2 in ((USER, ETA_T), (ITEM, ETA_B)):
            terms = ctx.gauss_elbo_terms(side, with_data=True, per_row=True)
            never += [terms[0].tobytes(), terms[1].tobytes()]
            ctx.gauss_factor_sweep(side, SIGMA2, eta2)
        assert _bits(ctx) == default_one
        assert never == one[-4:]
    for rows in ("17", "1"):                                     # ("1": windows that hold nothing but a row without ratings)
        monkeypatch.setenv("PMF_ELBO_ROWS", rows)
        many, default_many = _windows_case(K, dtype)
        assert many == one and default_many == default_one, rows
