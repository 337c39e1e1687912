"""Logistic matrix factorisation on the device (`pmf_gauss_logit_refresh`, `LogisticMFCAVI`)
against dense float64 NumPy (tests/logit_reference.py).  The reference always starts from state read back from the device.

The bound on E[s^2] = <S_u, S_i>
--------------------------------
The kernel (csrc/pmf_logit.hip) forms, per packed entry p = (r, c) of the lower triangle,
    s_p = w_p fma(m_r[r], m_r[c], V_r[p])      (one rounding; w_p = 1 or 2 is exact)
    e_p = fma(m_o[r], m_o[c], V_o[p])          (one rounding)
    acc = fma(s_p, e_p, acc)                   (one rounding: the addition)
so a term carries two roundings of its factors and every addition along its way to the total one more.  A lane adds
every L-th 16-byte chunk of the row into four accumulators: T = ceil(chunks / L) additions on the longest chain, then two
for (a0 + a1) + (a2 + a3) and log2(L) levels of the lane-group sum.  gamma's inputs: chunks = cov_stride / 4 = ceil(K (K + 1) /
8); L = the power of two in [4, 64] that ceil(chunks / 4) rounds up to -- 4 for K <= 10 (T = 1 .. 4), 8 for K = 11 .. 15 (T =
3 .. 4), 16 for K = 16 .. 22 (T = 3 .. 4), 32 for K = 23 .. 31 (T = 3 .. 4), 64 from K = 32 (T = 3 at K = 32, 9 at K = 64, 37 at
K = 136).  With gamma = 2 + T + 2 + log2(L), to first order,
    |dE| <= gamma eps(dtype) sum_p |terms|,      sum |terms| <= <|V_u| + |m_u||m_u|', |V_i| + |m_i||m_i|'>  = `abs_terms`
(eps = 2^-23 / 2^-52, twice the unit roundoff, so the first-order form has a factor 2 in hand).  It does not depend on the
conditioning of the covariances.  Nothing in it comes from running the kernel.

Propagated, everything from xi on being double on the device (a few eps64, covered by `LIBM`):
    xi = sqrt(E):            |dxi| <= |dE| / xi                       (xi' >= 0: |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)))
    c = 2 lambda(xi):        |dc| <= 2 SLOPE |dxi| + LIBM c,   then one rounding to the dtype: + eps c
                             SLOPE = sup |lambda'| < 0.022 (asserted on a grid below)
    y = (x - 1/2) / c:       |dy| <= |y| (|dc_double| / (c - |dc_double|)) + eps |y|
    D = sum_j f(xi_j) + (x_j - 1/2) m_u.m_i,  |f'| = |sigmoid(-xi) - 1/2| <= 1/2:
                             |dD| <= sum_j (|dxi_j| + |ddot_j|) / 2 + N eps64 sum_j |terms_j|
    m_u.m_i in the dtype: kpad products and fmas on chains of at most ceil(kpad / (4 L)) * 4 + log2(L) <= K + 6 additions:
                             |ddot| <= (K + 7) eps sum_k |m_u[k]| |m_i[k]|

Sweeps: tests/test_gauss_weighted_gpu.py's bars for a weighted half-sweep (it is the same kernel): fp64 1e-10, fp32 2e-4
(3e-4 at K >= 136), max abs on means, relative to the row's largest entry on covariances.

Fits: the bound of every iteration against the reference fit's in fp64 at rtol 1e-9 (the project's fp64 bar of 1e-10 per
two iterations, over up to 30); a step may fall by at most 10 x the rounding bound the CPU reference is held to
(tests/test_logit_cpu.py: its measured fall is 0, so the margin rests on that bound, 2 (N + (U + I) K) eps64 |L|; the
device sums the same terms in another order).  fp32: D moves by the bound on dD above at the fitted state and the KL terms
by the fp32 elimination's K^2 eps per row; a step may fall by twice that (two evaluations)."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest

import logit_reference as ref
from test_logit_cpu import ETA2, SMALL, reference_trace

pytestmark = pytest.mark.gpu

PMF_EINVAL = -1
USER, ITEM = 0, 1
U, I = 50, 40
# Lane-group widths: L = 4 up to K = 10, 8 for K = 11 .. 15, 16 for 16 .. 22, 32 for 23 .. 31, 64 from K = 32 (both neighbours of
# every switch).  LDS forms at L = 64: the row's own second moment in LDS with 256 threads per block up to K = 59 (fp64) /
# 84 (fp32; kpad is 96 there), with 128 threads up to K = 85 (fp64) / 121 (fp32), the generic form above.
KS = (1, 3, 8, 10, 11, 15, 16, 22, 23, 31, 32, 59, 60, 63, 64, 65, 72, 84, 85, 86, 121, 122, 128, 136)
LIBM = 16 * 2.0 ** -52
SLOPE = 0.022


def _eps(dtype):
    return 2.0 ** -52 if dtype == "f64" else 2.0 ** -23


def _bar(dtype, K):
    return 1e-10 if dtype == "f64" else (3e-4 if K >= 136 else 2e-4)


def _lanes(cov_stride):
    n, lanes = (cov_stride // 4 + 3) // 4, 4
    while lanes < n and lanes < 64:
        lanes *= 2
    return lanes


def _gamma(cov_stride):
    lanes = _lanes(cov_stride)
    chunks = cov_stride // 4
    return 2 + -(-chunks // lanes) + 2 + int(np.log2(lanes))


def _form(ctx):
    """the kernel's rule (logit_launch_refresh: logit_lds_bytes against kLogitOwnLdsMax): which form served this context"""
    lanes = _lanes(ctx.cov_stride)
    group = (2 * ctx.kpad + ctx.cov_stride) * (8 if ctx.np_dtype == np.float64 else 4)
    if (256 // lanes) * group <= 60 * 1024:
        return f"L={lanes} own-in-LDS block=256"
    return "L=64 own-in-LDS block=128" if 2 * group <= 60 * 1024 else "L=64 generic"


LONG = (64, 65, 128, 150)     # the row lengths of the long-task cases (PMF_TASK_CHUNK = 64 / 128)


@functools.lru_cache(maxsize=None)
def _ratings(lengths=(64, 65, 70)):
    """(u, i, x): users 0, 1, 2, 4 .. have exactly `lengths` ratings and user 3 none; items 5, 6, 7, 9 .. exactly `lengths`
    and item 8 none; every other row has a few; duplicate pairs occur.  By default 70 > the task length at this size (32):
    split rows on both sides."""
    rng = np.random.default_rng(77)
    n, tot = len(lengths), sum(lengths)
    long_u, long_i = np.array((0, 1, 2, 4, 10, 11)[:n]), np.array((5, 6, 7, 9, 10, 11)[:n])
    items = np.setdiff1d(np.arange(I), np.concatenate([long_i, [8]]))
    users = np.setdiff1d(np.arange(U), np.concatenate([long_u, [3]]))
    u = np.concatenate([np.repeat(long_u, lengths), rng.choice(users, tot), rng.choice(users, 150)])
    i = np.concatenate([rng.choice(items, tot), np.repeat(long_i, lengths), rng.choice(items, 150)])
    order = rng.permutation(len(u))
    u, i = u[order], i[order]
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    assert tuple(nu[long_u]) == tuple(lengths) and tuple(ni[long_i]) == tuple(lengths) and nu[3] == 0 and ni[8] == 0
    assert np.delete(nu, long_u).max() < 64 and np.delete(ni, long_i).max() < 64
    return u.astype(np.int64), i.astype(np.int64), (rng.uniform(size=len(u)) < 0.5).astype(np.float64)


def _tables(K):
    """means in [-0.5, 0.5] and random SPD covariances, every one a different matrix"""
    rng = np.random.default_rng(500 + K)
    out = []
    for rows in (U, I):
        A = rng.uniform(-1.0, 1.0, (rows, K, K))
        V = rng.uniform(0.5, 1.0, rows)[:, None, None] * (A @ np.swapaxes(A, 1, 2) / K + np.eye(K))
        out += [rng.uniform(-0.5, 0.5, (rows, K)), V]
    return out


def _open(K, dtype, c0=0.25, weighted=True, lengths=(64, 65, 70)):
    """a context with the ratings loaded as the model class loads them and the random state"""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR
    u, i, x = _ratings(lengths)
    ctx = pmf_hip.Context(U, I, K, dtype=dtype)
    ctx.set_ratings(u, i, (x - 0.5) / c0, np.full(len(x), c0) if weighted else None)
    m_u, V_u, m_i, V_i = _tables(K)
    ctx.set_array(USER, ARR_FACTOR, m_u)
    ctx.set_array(USER, ARR_COV, V_u)
    ctx.set_array(ITEM, ARR_FACTOR, m_i)
    ctx.set_array(ITEM, ARR_COV, V_i)
    return ctx


def _state(ctx):
    from pmf_hip import ARR_COV, ARR_FACTOR
    return (ctx.get_array(USER, ARR_FACTOR), ctx.get_array(USER, ARR_COV), ctx.get_array(ITEM, ARR_FACTOR), ctx.get_array(ITEM, ARR_COV))


def _side_order(side, lengths=(64, 65, 70)):
    """positions of the ratings in `side`'s stream: by row, ascending original position inside a row"""
    u, i, _ = _ratings(lengths)
    return np.argsort(u if side == USER else i, kind="stable")


def test_lambda_slope_constant():
    xi = np.linspace(1e-3, 60.0, 600001)
    slope = np.abs((0.5 * xi / np.cosh(0.5 * xi) ** 2 - np.tanh(0.5 * xi)) / (4.0 * xi * xi))
    assert slope.max() < SLOPE and xi[0] / 48.0 < SLOPE


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K", KS)
def test_refresh_against_the_reference(K, dtype, monkeypatch):
    monkeypatch.delenv("PMF_TASK_CHUNK", raising=False)
    _check_refresh(K, dtype, (64, 65, 70), 32)


@pytest.mark.parametrize("chunk", [64, 128])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K", [16, 64, 136])
def test_refresh_on_tasks_of_a_wavefront_and_longer(K, dtype, chunk, monkeypatch):
    """PMF_TASK_CHUNK = 64: the row of 64 ratings is one task that fills the lane group at L = 64 (every lane owns a rating)
    and the rows of 65, 128 and 150 are split; = 128: the rows of 65 and 128 are one task each -- a second pass of the
    batch loop with one and with 64 ratings -- and the row of 150 is split into two tasks of 75.  K = 16: four groups of 16
    lanes per wavefront with tasks of different lengths and up to eight passes; K = 64 and 136: both LDS forms and the
    generic one over the two dtypes."""
    monkeypatch.setenv("PMF_TASK_CHUNK", str(chunk))
    _check_refresh(K, dtype, LONG, chunk)


def _check_refresh(K, dtype, lengths, max_len):
    u, i, x = _ratings(lengths)
    eps = _eps(dtype)
    with _open(K, dtype, lengths=lengths) as ctx:
        assert ctx.task_max_len(USER, "gauss") == max_len and ctx.task_max_len(ITEM, "gauss") == max_len
        st = _state(ctx)
        xi, c, y, D, mag = ref.refresh(*st, u, i, x)
        dot_mag = (np.abs(st[0][u]) * np.abs(st[2][i])).sum(axis=1)
        d_e = _gamma(ctx.cov_stride) * eps * mag
        d_xi = d_e / xi
        d_c64 = 2.0 * SLOPE * d_xi + LIBM * c
        d_c = d_c64 + eps * c
        d_y = np.abs(y) * (d_c64 / (c - d_c64)) + (eps + LIBM) * np.abs(y)
        d_D = 0.5 * np.sum(d_xi + (K + 7) * eps * dot_mag) + len(x) * 2.0 ** -52 * np.sum(np.abs(ref.log_sigmoid(xi)) + 0.5 * xi + 0.5 * dot_mag)
        assert np.all(d_c64 < 0.5 * c)
        worst = {}
        for side in (USER, ITEM):
            order = _side_order(side, lengths)
            got_D = ctx.gauss_logit_refresh(side)
            rp, other, val, wgt = ctx.side_ratings(side)
            ids, oids = (u, i) if side == USER else (i, u)
            assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=ctx.rows(side)))]))
            assert np.array_equal(other, oids[order])
            # xi is not stored: E[s^2] is recovered from c through lambda only to lambda's slope, so c, y and D carry the check
            r_c = np.abs(wgt - c[order]) / d_c[order]
            r_y = np.abs(val - y[order]) / d_y[order]
            r_D = abs(got_D - D) / d_D
            worst[side] = (float(r_c.max()), float(r_y.max()), float(r_D))
            assert r_c.max() <= 1.0, (K, dtype, side, "c", int(r_c.argmax()), float(r_c.max()))
            assert r_y.max() <= 1.0, (K, dtype, side, "y", int(r_y.argmax()), float(r_y.max()))
            assert r_D <= 1.0, (K, dtype, side, "D", got_D, D, d_D)
            assert np.array_equal(val > 0, x[order] > 0.5)
            # the weight sums: the double sum of the refreshed weights in the row's order, rounded once
            sums = ctx.rating_weight_sums(side)
            want = np.zeros(ctx.rows(side))
            for r in range(ctx.rows(side)):
                s = 0.0
                for k in range(int(rp[r]), int(rp[r + 1])):
                    s += float(wgt[k])
                want[r] = np.float64(ctx.np_dtype(s))
            assert np.array_equal(sums, want) and ctx.rating_weights
            assert sums[3 if side == USER else 8] == 0.0
            # a second call on the same state: the same bytes
            again_D = ctx.gauss_logit_refresh(side)
            _, _, val2, wgt2 = ctx.side_ratings(side)
            assert again_D == got_D and np.array_equal(val2, val) and np.array_equal(wgt2, wgt)
            assert np.array_equal(ctx.rating_weight_sums(side), sums)
        print(f"refresh K={K} {dtype} tasks<={max_len} {_form(ctx)} gamma={_gamma(ctx.cov_stride)}: worst ratio to the bound (c, y, D) "
              f"user {worst[USER][0]:.3g} {worst[USER][1]:.3g} {worst[USER][2]:.3g}  item {worst[ITEM][0]:.3g} {worst[ITEM][1]:.3g} {worst[ITEM][2]:.3g}")


@pytest.mark.parametrize("K,dtype", [(3, "f32"), (3, "f64"), (64, "f32"), (64, "f64"), (72, "f32"), (136, "f32"), (136, "f64")])
def test_refresh_then_sweep_is_the_reference_sweep(K, dtype):
    u, i, x = _ratings()
    from pmf_hip import ARR_COV, ARR_FACTOR
    with _open(K, dtype) as ctx:
        for side, ids, oids in ((USER, u, i), (ITEM, i, u)):
            st = _state(ctx)
            c = ref.refresh(*st, u, i, x)[1]
            own, oth = (st[0], st[1]), (st[2], st[3])
            if side == ITEM:
                own, oth = oth, own
            m, V = ref.sweep(*own, *oth, ids, oids, x, c, 0.7)
            ctx.gauss_logit_refresh(side, want_data_term=False)
            ctx.gauss_factor_sweep(side, 1.0, 0.7)
            got_m, got_V = ctx.get_array(side, ARR_FACTOR), ctx.get_array(side, ARR_COV)
            bar = _bar(dtype, K)
            err_m = np.max(np.abs(got_m - m))
            err_V = np.max(np.abs(got_V - V) / np.abs(V).max(axis=(1, 2), keepdims=True))
            print(f"refresh + sweep K={K} {dtype} side {side}: mean err {err_m:.3g}, cov err {err_V:.3g} (bar {bar:g})")
            assert err_m <= bar and err_V <= bar, (K, dtype, side, float(err_m), float(err_V))


def test_labels_survive_refresh_and_sweep_rounds():
    u, i, x = _ratings()
    with _open(8, "f32") as ctx:
        for _ in range(5):
            for side in (USER, ITEM):
                ctx.gauss_logit_refresh(side, want_data_term=False)
                ctx.gauss_factor_sweep(side, 1.0, 1.0)
        for side in (USER, ITEM):
            _, _, val, wgt = ctx.side_ratings(side)
            assert np.array_equal(val > 0, x[_side_order(side)] > 0.5), side
            assert np.all(wgt > 0) and np.all(wgt <= 0.25)
            np.testing.assert_allclose(val * wgt, x[_side_order(side)] - 0.5, rtol=4 * _eps("f32"), atol=0)


def _raw_refresh(ctx, side):
    d = np.full(1, 777.0)
    rc = ctx._lib.pmf_gauss_logit_refresh(ctx._h, side, d.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, ctx._lib.pmf_last_error().decode(), d[0]


def test_refusals_write_nothing():
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ARR_RATE, ARR_SHAPE
    u, i, x = _ratings()
    with _open(3, "f32", weighted=False) as ctx:                      # an unweighted context
        before = ctx.side_ratings(USER, weights=False)[2]
        rc, msg, d = _raw_refresh(ctx, USER)
        assert rc == PMF_EINVAL and msg.startswith("pmf_gauss_logit_refresh: ") and "pmf_ctx_set_ratings_weighted" in msg and d == 777.0
        assert np.array_equal(ctx.side_ratings(USER, weights=False)[2], before)
        with pytest.raises(pmf_hip.PmfError, match="holds no rating weights"):
            ctx.side_ratings(USER)
    with _open(3, "f32") as ctx:
        for side in (-1, 2):                                          # a bad side
            rc, msg, d = _raw_refresh(ctx, side)
            assert rc == PMF_EINVAL and f"bad side {side}" in msg and d == 777.0
        before = ctx.side_ratings(ITEM)
        ctx.set_gauss_zeros(True, 0.5)                                # zero mode
        rc, msg, d = _raw_refresh(ctx, ITEM)
        assert rc == PMF_EINVAL and msg.startswith("pmf_gauss_logit_refresh: ") and "PMF_ZEROS_OBSERVED" in msg and d == 777.0
        ctx.set_gauss_zeros(False)
        assert all(np.array_equal(a, b) for a, b in zip(ctx.side_ratings(ITEM), before))
        assert _raw_refresh(ctx, ITEM)[0] == 0
    with pmf_hip.Context(U, I, 3) as ctx:                             # a count-model context: SHAPE / RATE, no covariances
        assert _raw_refresh(ctx, USER)[0] == PMF_EINVAL and "ratings have not been set" in ctx._lib.pmf_last_error().decode()
        ctx.set_ratings(u, i, x + 1.0, np.ones(len(x)))
        for side in (USER, ITEM):
            ctx.set_array(side, ARR_SHAPE, np.ones((ctx.rows(side), 3)))
            ctx.set_array(side, ARR_RATE, np.ones((ctx.rows(side), 3)))
        rc, msg, d = _raw_refresh(ctx, USER)
        assert rc == PMF_EINVAL and "pmf_gauss_logit_refresh: array FACTOR of side 0" in msg and d == 777.0
        for side in (USER, ITEM):
            ctx.set_array(side, ARR_FACTOR, np.ones((ctx.rows(side), 3)))
        ctx.set_cov_identity(USER)
        rc, msg, d = _raw_refresh(ctx, USER)
        assert rc == PMF_EINVAL and "pmf_gauss_logit_refresh: array COV of side 1" in msg and d == 777.0
    assert ctx._lib.pmf_gauss_logit_refresh(None, USER, None) == PMF_EINVAL


# ---- the model class ---------------------------------------------------------------------------------------------------
def _frame(u, i, x):
    return pd.DataFrame({"u": u, "i": i, "rating": x})


def _fit(problem, dtype, n_iter, seed=5):
    from src.models.logistic_mf_cavi import LogisticMFCAVI, LogisticMFCAVIConfig
    u, i, x, _, _ = ref.planted(problem["seed"], problem["U"], problem["I"], problem["K"], problem["N"])
    cfg = LogisticMFCAVIConfig(n_factors=problem["K"], eta2=ETA2, max_iter=n_iter, tol=None, seed=seed, dtype=dtype, verbose=False)
    return LogisticMFCAVI(cfg).fit(_frame(u, i, x)), (u, i, x)


LARGE = dict(seed=12, U=64, I=48, K=64, N=1500)


@pytest.mark.parametrize("problem,n_iter", [(SMALL, 30), (LARGE, 6)], ids=["K3", "K64"])
def test_fit_fp64_follows_the_reference_and_is_monotone(problem, n_iter):
    model, (u, i, x) = _fit(problem, "f64", n_iter)
    got = np.array(model.history_["elbo"])
    st, want = ref.fit(u, i, x, problem["U"], problem["I"], problem["K"], ETA2, n_iter, seed=5)
    want = np.array(want)
    assert problem is not SMALL or np.array_equal(want, reference_trace(n_iter))     # the trace the CPU test holds to its bound
    assert len(got) == n_iter and model.history_["iterations"] == n_iter
    rel = np.max(np.abs(got - want) / np.abs(want))
    margin = 10.0 * 2.0 * (problem["N"] + (problem["U"] + problem["I"]) * problem["K"]) * 2.0 ** -52   # 10 x test_logit_cpu's bound
    fall = ref.max_fall(got) / np.abs(got).max()
    print(f"fp64 fit K={problem['K']}: L {got[0]:.6f} -> {got[-1]:.6f}; max relative difference to the reference {rel:.3e}; "
          f"largest relative fall {fall:.3e} (margin {margin:.3e}; reference's own {ref.max_fall(want) / np.abs(want).max():.3e})")
    assert rel <= 1e-9
    assert fall <= margin
    assert got[-1] > got[0]
    # elbo(): a fresh bound at the fitted state, at least the last recorded one (the item sweep came between)
    assert model.elbo() >= got[-1] - margin * abs(got[-1])
    np.testing.assert_allclose(model.m_theta, st[0], rtol=0, atol=1e-8)
    np.testing.assert_allclose(model.V_beta, st[3], rtol=0, atol=1e-8)
    model.close()


def test_fit_fp32_falls_by_rounding_only():
    n_iter, p = 30, SMALL
    model, (u, i, x) = _fit(p, "f32", n_iter)
    got = np.array(model.history_["elbo"])
    m64, _ = _fit(p, "f64", n_iter)
    want = np.array(m64.history_["elbo"])
    # the bound on one evaluation of L in an fp32 context at the fitted state (module docstring)
    st = (m64.m_theta, m64.V_theta, m64.m_beta, m64.V_beta)
    xi, _, _, _, mag = ref.refresh(*st, u, i, x)
    eps, K = _eps("f32"), p["K"]
    dot_mag = (np.abs(st[0][u]) * np.abs(st[2][i])).sum(axis=1)
    cov_stride = -(-(K * (K + 1) // 2) // 4) * 4
    d_D = 0.5 * np.sum(_gamma(cov_stride) * eps * mag / xi + (K + 7) * eps * dot_mag)
    d_KL = (p["U"] + p["I"]) * K * K * eps
    margin = 2.0 * (d_D + d_KL)
    fall = ref.max_fall(got)
    print(f"fp32 fit K={K}: L {got[0]:.4f} -> {got[-1]:.4f}; max |L32 - L64| {np.max(np.abs(got - want)):.3e}; largest fall {fall:.3e} "
          f"(margin {margin:.3e} = 2 (dD {d_D:.3e} + dKL {d_KL:.3e}))")
    assert fall <= margin
    # every entry against the fp64 run: one evaluation's bound.  (The two runs' q differ by fp32 rounding as well; each
    # step maximises L over a block of q, so L moves with that difference to second order only.)
    assert np.max(np.abs(got - want)) <= d_D + d_KL
    assert got[-1] > got[0] + 1.0
    model.close()
    m64.close()


def test_held_out_log_loss_beats_the_base_rate():
    """Planted data at a signal scale where the NumPy reference fit clears the condition on the CPU (0.44 against 0.69)."""
    from src.models.logistic_mf_cavi import LogisticMFCAVI, LogisticMFCAVIConfig
    Uh, Ih, K = 60, 50, 3
    u, i, x, _, _ = ref.planted(11, Uh, Ih, K, int(Uh * Ih * 0.8), scale=2.0)
    held = np.random.default_rng(12).uniform(size=len(x)) < 0.2
    train, test = _frame(u[~held], i[~held], x[~held]), _frame(u[held], i[held], x[held])
    model = LogisticMFCAVI(LogisticMFCAVIConfig(n_factors=K, max_iter=15, tol=None, seed=5, verbose=False)).fit(train)
    base = float(train["rating"].mean())
    base_loss = float(-np.mean(np.where(test["rating"] > 0.5, np.log(base), np.log1p(-base))))
    loss, plain = model.log_loss(test), model.log_loss(test, moderated=False)
    print(f"held-out log-loss {loss:.4f} (unmoderated {plain:.4f}) against the base rate's {base_loss:.4f}")
    assert loss < base_loss
    p = model.predict_proba(test["u"], test["i"])
    assert p.shape == (len(test),) and np.all((p > 0) & (p < 1)) and np.array_equal(model.predict(test["u"], test["i"]), p)
    s = model.decision_function(test["u"], test["i"])
    assert np.allclose(model.predict_proba(test["u"], test["i"], moderated=False), 1.0 / (1.0 + np.exp(-s)), rtol=1e-12)
    assert np.all(np.abs(p - 0.5) <= np.abs(1.0 / (1.0 + np.exp(-s)) - 0.5) + 1e-15)          # moderation pulls towards 1/2
    assert np.array_equal(model.predict_proba([Uh, 0], [0, Ih]), [0.5, 0.5])                  # ids the fit has not seen
    model.close()


def test_read_side_surface_equals_the_gaussian_classes():
    """top-k (also Thompson-sampled, also without the training items), posterior draws, ranking metrics and similar items
    on the fitted logistic model equal the same calls on a `GaussianMFCAVI` whose context holds the same FACTOR / COV."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR
    from src.models.gaussian_mf_cavi import GaussianMFCAVI, GaussianMFCAVIConfig
    model, (u, i, x) = _fit(SMALL, "f32", 4)
    nu, ni, K = SMALL["U"], SMALL["I"], SMALL["K"]
    g = GaussianMFCAVI(GaussianMFCAVIConfig(n_factors=K, verbose=False), dtype="f32")
    g.n_users, g.n_items = nu, ni
    g._ctx = pmf_hip.Context(nu, ni, K, dtype="f32")
    g._ctx.set_ratings(u, i, x)
    g._train_pairs = (u, i)
    for side in (USER, ITEM):
        for arr in (ARR_FACTOR, ARR_COV):
            g._ctx.set_array(side, arr, model._ctx.get_array(side, arr))
    users = np.arange(0, nu, 3)
    held = _frame(np.arange(nu), (np.arange(nu) * 7) % ni, np.ones(nu))
    calls = {
        "top_k_items": lambda m: m.top_k_items(users, k=5),
        "top_k_items exclude_train": lambda m: m.top_k_items(users, k=5, exclude_train=True),
        "top_k_items sample_seed": lambda m: m.top_k_items(users, k=5, sample_seed=3, draw=2),
        "top_k_items sample_seed exclude_train": lambda m: m.top_k_items(users, k=5, exclude_train=True, sample_seed=3),
        "sample_factors": lambda m: (m.sample_factors("item", [0, 5, 2], n_draws=4, seed=9),),
        "predict_draws": lambda m: (m.predict_draws([0, 1, 1], [2, 2, 3], 6, seed=4),),
        "similar_items": lambda m: m.similar_items([0, 1, 2], k=4),
        "top_k_users": lambda m: m.top_k_users([0, 1], k=3),
    }
    shapes = {"top_k_items": (len(users), 5), "sample_factors": (3, 4, K), "predict_draws": (3, 6), "similar_items": (3, 4)}
    for name, call in calls.items():
        a, b = call(model), call(g)
        assert len(a) == len(b)
        for p, q in zip(a, b):
            assert np.array_equal(p, q), name
        if name.split(" ")[0] in shapes:
            assert a[0].shape == shapes[name.split(" ")[0]], (name, a[0].shape)
    ra, rb = model.evaluate_ranking(held, ks=(5,)), g.evaluate_ranking(held, ks=(5,))
    assert ra == rb and "recall@5" in ra, ra
    ex_items, _ = model.top_k_items(users, k=5, exclude_train=True)
    for row, usr in zip(ex_items, users):
        assert not set(row[row >= 0]) & set(i[u == usr])
    var = model.predict_variance([0, 1], [2, 3])
    assert var.shape == (2,) and np.all(var > 0) and np.array_equal(var, g.predict_variance([0, 1], [2, 3], include_noise=False))
    model.close()
    g.close()
