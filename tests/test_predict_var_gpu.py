"""Posterior predictive variance on the device (`pmf_predict_var`, `pmf_eval_run_var`, csrc/pmf_eval.hip) and its
model surface (`predict_variance`, `log_predictive_density`) against the dense formula in NumPy, with a derived error
bound asserted on every pair and every sum.

Reference.  FACTOR and COV are read back from the device (`get_array`; COV comes back as dense K x K float64), so the
rounding of the inputs is not part of the error.  With q(theta_u) = N(mu, Vu), q(beta_i) = N(mi, Vi):

    Var[f] = mu' Vi mu + mi' Vu mi + tr(Vu Vi)

is evaluated densely (outer products and full matrices, the trace with the transposed factor), in float64 for fp32
contexts (fp32 inputs and their pairwise products are exact there; the reference's own rounding is ~K^2 2^-53 of the
magnitude, far below u = 2^-24) and in `np.longdouble` for fp64 contexts where that is wider.  The dense form shares
nothing with the kernel's packed single pass.

Per pair.  The kernel (predict_var_pair) adds, for every packed entry p = (r, c),
    e = Vu[p] Vi[p];  e = fma(Vu[p], mi[r] mi[c], e);  e = fma(Vi[p], mu[r] mu[c], e);  acc[j] = fma(w, e, acc[j])
(w = 1 or 2: exact).  A product is rounded once when it is formed and again by each fma it passes through: at most 3
roundings before the accumulate.  acc[j] (one partial sum per position j in a 16-byte chunk) takes one fma per chunk
the lane owns: ceil(chunks / L) of them, chunks = cov_stride / 4, L lanes per pair.  (acc0 + acc1) + (acc2 + acc3) adds
2, the lane-group sum log2(L).  So the longest path has

    c = 3 + ceil(chunks / L) + 2 + log2(L)

roundings (K = 256: 3 + 129 + 2 + 6 = 140; K = 1: 3 + 1 + 2 + 2 = 8), computed per case by `_roundings`, and with
gamma_c = c u / (1 - c u)

    |got - ref| <= gamma_c * sum_p w_p ( |Vi[p] mu[r] mu[c]| + |Vu[p] mi[r] mi[c]| + |Vu[p] Vi[p]| ) = gamma_c * mag

(the conversion to double is exact), to which the reference's own worst-case rounding is added (`_bound`: 3 K^2 2^-53 * mag
for fp32 contexts, 2e-11 against gamma_c = 8e-6 at K = 256; 66 * 2^-64 * mag = 0.03 u for fp64 contexts, whose reference
is summed pairwise in an 80-bit long double; where long double is no wider than double those 66 units are asserted as
they are).  The magnitude is formed densely too (the matrices are symmetric, so the dense
sum of absolute values is the weighted packed one).  A pair with an id outside the trained dimensions is exactly 0.
There is no outlier allowance.

Fused sums (`eval_var_sums`).  With e = y - predict, d = sigma2 + v, the term is t(e, v) = a + b,
a = -1/2 log(2 pi d), b = -e^2 / (2 d).  The device's e and v lie within delta_e (the bound of tests/test_eval_gpu.py:
16 u (sum |a_k b_k| + |bu| + |bi|) + 4 * 2^-53 |ref|) and delta_v (above) of the references.  First order:
    |dt| ~ |e| / d * delta_e + (1 / (2 d) + e^2 / (2 d^2)) * delta_v.
Remainder: by the mean value theorem the same expression bounds |dt| rigorously when the partial derivatives are taken
at their largest over the box, i.e. with |e| + delta_e for |e| and d - delta_v for d; the asserted per-pair bound is
that one (it exceeds the first-order figure by the second-order remainder and needs d - delta_v > 0, asserted).  The
device evaluates t in double from its e and v: fewer than 8 roundings on each of a and b, and the argument of the
logarithm carries 3 relative roundings (d, 2 pi d, the constant), i.e. 3 * 2^-53 absolute on the logarithm whatever its
size.  Summation of n terms in some order: n 2^-53 relative per term.  Together

    |sum_ld - sum t_ref| <= sum_i box_i + (n + 8) 2^-52 sum_i (|a_i| + |b_i|) + n 2^-52
    |sum_var - sum v_ref| <= sum_i delta_v_i + n 2^-52 sum_i |v_ref_i|.

Tighter check: `predict_var` and `predict` on the same pairs return the bits the reduction saw (same device functions,
same lane-group widths); the terms formed from them on the host and added with `math.fsum` must agree with the device
sums with the box term gone: only the evaluation / summation terms of the two lines above remain.  Two calls in a row
are bit-identical (block-ordered partial sums, no atomics).

No tolerance below is a number found by running the kernel."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT32_MAX = np.iinfo(np.int32).max
INT32_MIN = np.iinfo(np.int32).min
PMF_EINVAL = -1                                   # include/pmf_hip.h
WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else np.float64
U, I = 37, 29
ALL_KS = [1, 3, 4, 5, 8, 12, 16, 17, 24, 32, 33, 64, 65, 100, 128, 129, 256]      # 24: the one K here with 32 lanes per pair
BOTH_DTYPES = (1, 5, 16, 64, 129)
CASES = [(K, "f32") for K in ALL_KS] + [(K, "f64") for K in BOTH_DTYPES]
RATINGS = np.array([1.0, 2.0, 3.0, 4.0, 5.0])


# ---- geometry of the kernel, restated from csrc/pmf_eval.hip ---------------------------------------------------------
def _lanes(ctx):
    """lanes per pair: the power of two in [4, 64] that ceil(chunks / 4) rounds up to"""
    want, lanes = (ctx.cov_stride // 4 + 3) // 4, 4
    while lanes < min(want, 64):
        lanes <<= 1
    return lanes


def _roundings(ctx):
    chunks, lanes = ctx.cov_stride // 4, _lanes(ctx)
    return 3 + -(-chunks // lanes) + 2 + int(math.log2(lanes))


def _gamma(ctx):
    from pmf_hip import F64
    cu = _roundings(ctx) * (2.0 ** -53 if ctx.dtype == F64 else 2.0 ** -24)
    return cu / (1.0 - cu)


def test_lane_groups_cover_every_width_and_every_packed_remainder():
    """The K list reaches every lane-group width and every K (K + 1) / 2 mod 4 (pad entries 0 .. 3)."""
    import pmf_hip
    seen_l, seen_pad = set(), set()
    for K in ALL_KS:
        with pmf_hip.Context(U, I, K) as ctx:
            seen_l.add(_lanes(ctx))
            seen_pad.add(ctx.cov_stride - K * (K + 1) // 2)
            assert ctx.cov_stride % 4 == 0 and 0 <= ctx.cov_stride - K * (K + 1) // 2 < 4
    assert seen_l == {4, 8, 16, 32, 64} and seen_pad == {0, 1, 2, 3}, (seen_l, seen_pad)


# ---- the dense reference ---------------------------------------------------------------------------------------------
def _dense_table(mu, mi, Vu, Vi, acc):
    """(ref, mag) of every (user, item) pair from dense tables: ref in `acc`, mag in float64.  `mag` is the sum of the
    absolute values of every product of the dense formula.  With acc = float64 (fp32 contexts) the sums are BLAS dot
    products; otherwise (fp64 contexts) every product is formed element-wise in `acc` and added by NumPy's pairwise
    summation along the contiguous axis, which keeps the reference's own rounding to a few dozen units of `acc`."""
    nu, ni = len(mu), len(mi)
    ref, mag = np.zeros((nu, ni), acc), np.zeros((nu, ni))
    mu_w, mi_w, Vu_w, Vi_w = (np.asarray(t).astype(acc) for t in (mu, mi, Vu, Vi))
    Vi_t = np.ascontiguousarray(Vi_w.transpose(0, 2, 1))
    Mi = mi_w[:, :, None] * mi_w[:, None, :]                        # outer products of the item means
    aVi, aMi = np.abs(Vi_w).astype(np.float64), np.abs(Mi).astype(np.float64)
    if acc is np.float64:
        def contract(stack, mat):
            return np.tensordot(stack, mat, 2)
    else:
        def contract(stack, mat):
            return (stack * mat).reshape(len(stack), -1).sum(axis=1)
    for u in range(nu):
        Mu = np.multiply.outer(mu_w[u], mu_w[u])
        aVu = np.abs(Vu_w[u]).astype(np.float64)
        ref[u] = contract(Vi_w, Mu) + contract(Mi, Vu_w[u]) + contract(Vi_t, Vu_w[u])
        mag[u] = np.tensordot(aVi, np.abs(Mu).astype(np.float64), 2) + np.tensordot(aMi, aVu, 2) + np.tensordot(aVi, aVu, 2)
    return ref, mag


def _bound(ctx, mag, acc):
    """gamma_c * mag, plus the dense reference's own worst-case rounding in units of `acc`: the 3 K^2 terms of a dot
    product (float64), or 2 per product + 64 for a pairwise sum (blocks of 128 with 8 partial sums, then a tree)"""
    own = 3.0 * ctx.K * ctx.K if acc is np.float64 else 66.0
    return (_gamma(ctx) + own * 0.5 * float(np.finfo(acc).eps)) * mag


def _spd_rows(rng, rows, K):
    """a different SPD matrix per row: A A' / K + 0.1 I"""
    A = rng.standard_normal((rows, K, K))
    return A @ A.transpose(0, 2, 1) / K + 0.1 * np.eye(K)


class _Case:
    """One context with signed standard-normal means, per-row SPD covariances, standard-normal biases, and the dense
    reference table of all U x I pairs (computed once, never changed)."""

    def __init__(self, K, dtype):
        import pmf_hip
        from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, F64, ITEM, USER
        rng = np.random.default_rng(5000 + K)
        self.ctx = ctx = pmf_hip.Context(U, I, K, dtype=dtype)
        self.acc = WIDE if ctx.dtype == F64 else np.float64
        self.unit = 2.0 ** -53 if ctx.dtype == F64 else 2.0 ** -24
        for side, rows in ((USER, U), (ITEM, I)):
            ctx.set_array(side, ARR_FACTOR, rng.standard_normal((rows, K)))
            ctx.set_array(side, ARR_COV, _spd_rows(rng, rows, K))
            ctx.set_array(side, ARR_BIAS, rng.standard_normal(rows))
        self.mu, self.mi = ctx.get_array(USER, ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
        self.bu, self.bi = ctx.get_array(USER, ARR_BIAS), ctx.get_array(ITEM, ARR_BIAS)
        Vu, Vi = ctx.get_array(USER, ARR_COV), ctx.get_array(ITEM, ARR_COV)
        assert np.array_equal(Vu, Vu.transpose(0, 2, 1)) and np.array_equal(Vi, Vi.transpose(0, 2, 1))
        self.ref, self.mag = _dense_table(self.mu, self.mi, Vu, Vi, self.acc)
        self.delta = _bound(ctx, self.mag, self.acc)
        # predict's reference and bound (tests/test_eval_gpu.py), flag 0 / 1 added by `mean`
        prod = self.mu[:, None, :].astype(self.acc) * self.mi[None, :, :]
        self.dot, self.dot_mag = prod.sum(axis=2), np.abs(prod).sum(axis=2).astype(np.float64)

    def var(self, u, i):
        """(ok, ref, delta_v) for the pairs"""
        u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
        ok = (u >= 0) & (u < U) & (i >= 0) & (i < I)
        uu, ii = np.where(ok, u, 0), np.where(ok, i, 0)
        return ok, np.where(ok, self.ref[uu, ii], self.acc(0)), np.where(ok, self.delta[uu, ii], 0.0)

    def mean(self, u, i, flag, offset):
        """(ref, delta_e) of `predict` for the pairs"""
        u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
        ok = (u >= 0) & (u < U) & (i >= 0) & (i < I)
        uu, ii = np.where(ok, u, 0), np.where(ok, i, 0)
        val, mag = self.dot[uu, ii].copy(), self.dot_mag[uu, ii].copy()
        if flag & 1:
            val += self.bu[uu].astype(self.acc) + self.bi[ii]
            mag += np.abs(self.bu[uu]) + np.abs(self.bi[ii])
        ref = np.where(ok, val + offset, self.acc(offset))
        return ref, np.where(ok, 16.0 * self.unit * mag + 4.0 * 2.0 ** -53 * np.abs(ref).astype(np.float64), 0.0)


@pytest.fixture(scope="module")
def case():
    made = {}

    def get(K, dtype):
        if (K, dtype) not in made:
            made[K, dtype] = _Case(K, dtype)
        return made[K, dtype]
    yield get
    for c in made.values():
        c.ctx.close()


def _check_pairs(got, ref, delta, what):
    """|got - ref| <= delta on EVERY pair (delta = 0: exact)."""
    err = np.abs(got - ref).astype(np.float64)
    over = err > delta
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(delta > 0, err / delta, 0.0)
    print(f"{what}: n={len(got)} max |got-ref|/delta = {ratio.max():.3f}, pairs over the bound: {int(over.sum())}")
    if over.any():
        k = int(np.argmax(np.where(over, err - delta, -1.0)))
        raise AssertionError(f"{what}: {int(over.sum())} of {len(got)} pairs over the bound; worst at {k}: got "
                             f"{got[k]!r}, ref {float(ref[k])!r}, |diff| {err[k]:.3e} > delta {delta[k]:.3e}")


def _raw_predict_var(ctx, u, i, out):
    from pmf_hip import ptr
    u, i = np.ascontiguousarray(u, np.int32), np.ascontiguousarray(i, np.int32)
    return ctx._lib.pmf_predict_var(ctx._h, len(u), ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(out, C.c_double))


# ---- 1. per pair: every lane-group width, block edges, grid-stride rounds, ids at and beyond the edges -------------
@pytest.mark.parametrize("K,dtype", CASES)
def test_predict_var_every_pair_within_the_derived_bound(case, K, dtype):
    """Pair lists: n = 1; one pair fewer / more than a block holds (G = 256 / L); 3001 pairs with repeats; one more
    than a full grid of 8192 blocks plus one block (every block runs two grid-stride rounds, the second ragged).
    The first pairs of every list sit at ids 0 and rows - 1; ids -1, rows, INT32_MAX, INT32_MIN are mixed in through
    the raw ABI (the wrapper would clip the negative ones) and give exactly 0; the doubles behind out[n - 1] keep
    their value."""
    cs = case(K, dtype)
    ctx, rng = cs.ctx, np.random.default_rng(K)
    G = 256 // _lanes(ctx)
    for n in (1, G - 1, G + 1, 3001, 8192 * G + G + 1):
        u, i = rng.integers(0, U, n), rng.integers(0, I, n)
        corners = [(0, 0), (U - 1, I - 1), (0, I - 1), (U - 1, 0)][:n]
        for k, (a, b) in enumerate(corners):
            u[k], i[k] = a, b
        bad = np.empty(0, np.int64)
        if n > 8:
            bad = np.unique(np.concatenate([rng.choice(np.arange(4, n), min(n - 4, 40), replace=False), [n - 1]]))
            kinds = rng.integers(0, 6, len(bad))
            u[bad[kinds == 0]], i[bad[kinds == 1]] = -1, -1
            u[bad[kinds == 2]], i[bad[kinds == 3]] = U, I
            u[bad[kinds == 4]], i[bad[kinds == 4]] = INT32_MAX, INT32_MIN
            u[bad[kinds == 5]], i[bad[kinds == 5]] = INT32_MIN, INT32_MAX
        out = np.full(n + 8, 777.0)
        assert _raw_predict_var(ctx, u, i, out) == 0
        assert (out[n:] == 777.0).all()
        ok, ref, delta = cs.var(u, i)
        assert ok.sum() == n - len(bad) and (out[:n][~ok] == 0.0).all()
        _check_pairs(out[:n], ref, delta, f"predict_var K={K} {dtype} n={n} c={_roundings(ctx)}")
        if n == 3001:
            # the wrapper: ids beyond int32 and below zero are out of range too, the valid pairs are the same bits
            got = ctx.predict_var(np.where(u == -1, -2 ** 40, u.astype(np.int64)), np.where(i == I, 2 ** 40, i.astype(np.int64)))
            assert got.dtype == np.float64 and np.array_equal(got, out[:n])
    with pytest.raises(ValueError):
        ctx.predict_var([0, 1], [0])


def test_n_zero_touches_nothing_and_null_pointers_are_refused(case):
    ctx = case(5, "f32").ctx
    out = np.full(4, 777.0)
    assert ctx._lib.pmf_predict_var(ctx._h, 0, None, None, None) == 0
    assert _raw_predict_var(ctx, np.empty(0), np.empty(0), out) == 0 and (out == 777.0).all()
    assert ctx.predict_var([], []).shape == (0,)
    assert ctx._lib.pmf_predict_var(ctx._h, 2, None, None, None) == PMF_EINVAL
    assert b"null argument" in ctx._lib.pmf_last_error()
    assert ctx._lib.pmf_predict_var(ctx._h, -1, None, None, None) == PMF_EINVAL


def test_staging_rounds_cross_the_boundary_by_one_pair(case):
    """`pmf_predict_var` stages 4 Mi pairs per round: 4 Mi + 1 pairs at K = 4 are two launches (the profiler's count of
    the class says so), the second of one pair, written at its own place of the output."""
    cs = case(4, "f32")
    ctx, rng = cs.ctx, np.random.default_rng(4)
    n = (4 << 20) + 1
    u, i = rng.integers(0, U, n), rng.integers(0, I, n)
    u[[0, n - 2, n - 1]], i[[0, n - 2, n - 1]] = [U, U - 1, U - 1], [0, I - 1, 0]
    ctx.prof_enable(True)
    ctx.prof_reset()
    got = ctx.predict_var(u, i)
    assert ctx.prof_get()["predict_var"][1] == 2 and ctx.prof_get()["predict"][1] == 0
    ctx.prof_enable(False)
    ok, ref, delta = cs.var(u, i)
    assert got[0] == 0.0 and ok.sum() == n - 1
    _check_pairs(got, ref, delta, "predict_var staging 4Mi+1 K=4")


def test_row_offsets_beyond_2_31_elements():
    """K = 64 fp32: cov_stride = 2080, so user rows from 1,032,445 start beyond 2^31 elements of the table (8.7 GB).
    Identity covariances everywhere, per-row SPD ones and normal means on the rows around that edge and the last row;
    the reference is read back row-wise.  A 32-bit row offset would read before the table."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    K, NU, NI = 64, 1_040_000, 11
    rng = np.random.default_rng(64)
    with pmf_hip.Context(NU, NI, K) as ctx:
        assert ctx.cov_stride == 2080
        edge = -(-2 ** 31 // ctx.cov_stride)
        rows = np.array([0, edge - 1, edge, edge + 1, NU - 1], np.int64)
        assert edge == 1_032_445 and ((rows * ctx.cov_stride >= 2 ** 31) == [False, False, True, True, True]).all()
        ctx.set_cov_identity(USER, 1.0)
        ctx.set_array_rows(USER, ARR_FACTOR, rows, rng.standard_normal((len(rows), K)))
        ctx.set_array_rows(USER, ARR_COV, rows, _spd_rows(rng, len(rows), K))
        ctx.set_array(ITEM, ARR_FACTOR, rng.standard_normal((NI, K)))
        ctx.set_array(ITEM, ARR_COV, _spd_rows(rng, NI, K))
        ref, mag = _dense_table(ctx.get_array_rows(USER, ARR_FACTOR, rows), ctx.get_array(ITEM, ARR_FACTOR),
                                ctx.get_array_rows(USER, ARR_COV, rows), ctx.get_array(ITEM, ARR_COV), np.float64)
        k, i = np.repeat(np.arange(len(rows)), NI), np.tile(np.arange(NI), len(rows))
        got = ctx.predict_var(rows[k], i)
        _check_pairs(got, ref[k, i], _bound(ctx, mag[k, i], np.float64), "predict_var rows beyond 2^31 elements")
        # an untouched row: identity covariance, zero mean  ->  mi' mi + tr(Vi)
        mi, Vi = ctx.get_array(ITEM, ARR_FACTOR), ctx.get_array(ITEM, ARR_COV)
        want = (mi * mi).sum(axis=1) + np.trace(Vi, axis1=1, axis2=2)
        got = ctx.predict_var(np.full(NI, edge + 7), np.arange(NI))
        _check_pairs(got, want, _bound(ctx, want, np.float64), "predict_var identity row beyond 2^31 elements")


# ---- 2. after real sweeps: whatever the solves leave in the pad entries ---------------------------------------------
@pytest.mark.parametrize("K,dtype", [(8, "f32"), (80, "f32"), (16, "f64"), (10, "f32"), (82, "f32")])
def test_model_predict_variance_after_real_sweeps(K, dtype):
    """Three Gaussian-bias CAVI iterations through the class API, then `predict_variance` against the dense formula
    from the model's own V_theta, V_beta, m_theta, m_beta, within the per-pair bound.  K = 80 and 82 take the MFMA
    block-sweep solve; K = 10 and 82 have K (K + 1) / 2 = 55 and 3403, i.e. one pad entry per packed row, which holds
    whatever the solve's epilogue left.  `include_noise` adds exactly sigma2; unseen ids give 0 (+ sigma2)."""
    import pandas as pd
    from helpers import skewed_problem
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    u, i, x = skewed_problem(K, 90, 40, 2500, rating_kind="centered")
    cfg = GaussianMFCAVIConfig(n_factors=K, sigma2=0.3, eta_theta2=0.5, eta_beta2=0.5, eta_bias2=1.0, max_iter=3,
                               tol=-1.0, random_state=3, verbose=False)
    model = GaussianMFCAVI(cfg, dtype=dtype).fit(pd.DataFrame({"u": u, "i": i, "rating": x}), global_mean=3.5)
    try:
        assert model.history_["iterations"] == 3
        ctx, nu, ni = model._ctx, model.n_users, model.n_items
        acc = WIDE if dtype == "f64" else np.float64
        ref, mag = _dense_table(model.m_theta, model.m_beta, model.V_theta, model.V_beta, acc)
        pu, pi = np.repeat(np.arange(nu), ni), np.tile(np.arange(ni), nu)
        got = model.predict_variance(pu, pi, include_noise=False)
        assert (got > 0).all()
        _check_pairs(got, ref[pu, pi], _bound(ctx, mag[pu, pi], acc), f"predict_variance after sweeps K={K} {dtype}")
        assert np.array_equal(model.predict_variance(pu, pi), got + cfg.sigma2)
        assert np.array_equal(model.predict_variance(pu, pi, include_noise=True), got + cfg.sigma2)
        unseen = model.predict_variance([nu, 0, 2 ** 40], [0, ni, 1], include_noise=False)
        assert (unseen == 0.0).all()
        assert (model.predict_variance([nu], [0]) == cfg.sigma2).all()
    finally:
        model.close()


# ---- 3. the fused reduction -----------------------------------------------------------------------------------------
def _terms(e, v, sigma2):
    d = sigma2 + v
    return -0.5 * np.log(2.0 * np.pi * d), -e * e / (2.0 * d)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K", [5, 64, 129])
def test_eval_var_sums_against_pairs_and_against_predict(case, K, dtype):
    """n = 1024 G + G + 1 pairs: the grid is capped at 1024 blocks, so every block runs two grid-stride rounds, the
    second ragged.  Flags 0 and 1, offset 3.625, sigma2 = 0.3 (2 pi sigma2 > 1: both parts of every term are negative,
    no cancellation inside a term).  A few ids outside the tables: v = 0, e = y - offset."""
    cs = case(K, dtype)
    ctx, rng = cs.ctx, np.random.default_rng(3000 + K)
    sigma2, offset = 0.3, 3.625
    n = 1024 * (256 // _lanes(ctx)) + 256 // _lanes(ctx) + 1
    u, i = rng.integers(0, U, n), rng.integers(0, I, n)
    bad = np.concatenate([rng.choice(n - 1, 12, replace=False), [n - 1]])
    u[bad[::2]], i[bad[1::2]] = U, 2 ** 40
    y = rng.choice(RATINGS, n)
    assert ctx.eval_set(u, i, y) is True
    ok, v_ref, dv = cs.var(u, i)
    assert ok.sum() == n - len(bad)
    for flag in (0, 1):
        what = f"eval_var K={K} {dtype} flag={flag}"
        cnt, sv, sl = ctx.eval_var_sums(flag, offset, sigma2)
        assert (cnt, sv, sl) == ctx.eval_var_sums(flag, offset, sigma2), f"{what}: two runs differ"
        assert cnt == n
        # against the per-pair references
        p_ref, de = cs.mean(u, i, flag, offset)
        e_ref = y.astype(cs.acc) - p_ref
        a, b = _terms(e_ref, v_ref, cs.acc(sigma2))
        e64, d64 = np.abs(e_ref).astype(np.float64), sigma2 + v_ref.astype(np.float64)
        d_min, e_max = d64 - dv, e64 + de
        assert (d_min > 0).all()
        box = e_max / d_min * de + (0.5 / d_min + e_max ** 2 / (2.0 * d_min ** 2)) * dv
        first = e64 / d64 * de + (0.5 / d64 + e64 ** 2 / (2.0 * d64 ** 2)) * dv
        size = float(np.sum(np.abs(a) + np.abs(b)))
        b_eval = (n + 8) * 2.0 ** -52 * size + n * 2.0 ** -52
        b_ld = float(box.sum()) + b_eval
        want_ld, want_v = float(np.sum(a + b)), float(np.sum(v_ref))
        b_v = float(dv.sum()) + n * 2.0 ** -52 * float(np.abs(v_ref).sum())
        print(f"{what}: n={n} |sum_var-ref|/bound = {abs(sv - want_v) / b_v:.3f}, |sum_ld-ref|/bound = "
              f"{abs(sl - want_ld) / b_ld:.3f} (first order {first.sum():.3e}, remainder {box.sum() - first.sum():.3e})")
        assert abs(sv - want_v) <= b_v, (what, sv, want_v, b_v)
        assert abs(sl - want_ld) <= b_ld, (what, sl, want_ld, b_ld)
        # against predict_var / predict on the same pairs: the bits the reduction saw
        v_dev, p_dev = ctx.predict_var(u, i), ctx.predict(u, i, flag, offset)
        a, b = _terms(y - p_dev, v_dev, sigma2)
        host_ld, host_v = math.fsum(a + b), math.fsum(v_dev)
        size = math.fsum(np.abs(a) + np.abs(b))
        print(f"{what} [vs predict]: |sum_var-host| = {abs(sv - host_v):.3e}, |sum_ld-host| = {abs(sl - host_ld):.3e}")
        assert abs(sv - host_v) <= n * 2.0 ** -52 * math.fsum(np.abs(v_dev)), (what, sv, host_v)
        assert abs(sl - host_ld) <= (n + 8) * 2.0 ** -52 * size + n * 2.0 ** -52, (what, sl, host_ld)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_model_log_predictive_density_drops_unseen_ids(dtype):
    """`log_predictive_density(df)` is the TOTAL over the rows with seen ids: a frame with unseen users and items
    appended gives the figure of the seen rows, which equals the host sum over `predict` / `predict_variance` of those
    rows (the evaluation / summation term of the module docstring).  More than 32 distinct ratings take the
    predict-and-sum path: the same host computation, rel 1e-12.  No seen row: nan with the warning."""
    import pandas as pd
    from helpers import skewed_problem
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    nu, ni, gm = 120, 40, 3.75
    u, i, x = skewed_problem(9, nu, ni, 3000, rating_kind="centered")
    rng = np.random.default_rng(2)
    cfg = GaussianMFCAVIConfig(n_factors=12, sigma2=0.3, eta_theta2=0.5, eta_beta2=0.5, eta_bias2=1.0, max_iter=2,
                               tol=-1.0, random_state=3, verbose=False)
    model = GaussianMFCAVI(cfg, dtype=dtype).fit(pd.DataFrame({"u": u, "i": i, "rating": x}), global_mean=gm)
    try:
        n = 700
        vu, vi = rng.integers(0, nu, n), rng.integers(0, ni, n)
        coarse = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0], n)
        smooth = np.round(rng.normal(0.0, 1.5, n), 2)
        assert len(np.unique(smooth)) > 32
        v = model.predict_variance(vu, vi, include_noise=False)
        p = model.predict(vu, vi, gm)
        for name, rating in (("fused", coarse), ("fallback", smooth)):
            a, b = _terms(rating + gm - p, v, cfg.sigma2)
            want = math.fsum(a + b)
            seen = pd.DataFrame({"u": vu, "i": vi, "rating": rating})
            more = pd.concat([seen, pd.DataFrame({"u": [nu, 0, nu + 5], "i": [0, ni, ni], "rating": [1.0, 2.0, 0.0]})])
            got, got_more = model.log_predictive_density(seen, gm), model.log_predictive_density(more.sample(frac=1.0, random_state=1), gm)
            bound = ((n + 8) * 2.0 ** -52 * math.fsum(np.abs(a) + np.abs(b)) + n * 2.0 ** -52) if name == "fused" else 1e-12 * abs(want)
            print(f"log_predictive_density {name} {dtype}: got {got!r}, host {want!r}, bound {bound:.3e}")
            assert abs(got - want) <= bound and abs(got_more - want) <= bound
        assert np.isnan(model.log_predictive_density(pd.DataFrame({"u": [nu], "i": [0], "rating": [1.0]}), gm))
    finally:
        model.close()


# ---- 4. what is refused ---------------------------------------------------------------------------------------------
def test_missing_arrays_bad_sigma2_and_no_validation_set_are_einval():
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER, PmfError
    rng = np.random.default_rng(1)
    K = 6
    for have, missing in ((ITEM, USER), (USER, ITEM)):
        with pmf_hip.Context(U, I, K) as ctx:
            ctx.set_array(USER, ARR_FACTOR, rng.standard_normal((U, K)))
            with pytest.raises(PmfError, match=r"\(-1\).*pmf_predict_var: array FACTOR of side 1"):
                ctx.predict_var([0], [0])
            ctx.set_array(ITEM, ARR_FACTOR, rng.standard_normal((I, K)))
            ctx.set_cov_identity(have, 1.0)
            with pytest.raises(PmfError, match=rf"\(-1\).*pmf_predict_var: array COV of side {missing}"):
                ctx.predict_var([0], [0])
            assert ctx.eval_set([0, 1], [0, 1], [1.0, 2.0])
            with pytest.raises(PmfError, match=rf"\(-1\).*pmf_eval_run_var: array COV of side {missing}"):
                ctx.eval_var_sums(0, 0.0, 1.0)
            ctx.set_cov_identity(missing, 1.0)
            assert ctx.predict_var([0], [0]).shape == (1,)
            with pytest.raises(PmfError, match=r"\(-1\).*array BIAS"):       # needed only when the flag asks for it
                ctx.eval_var_sums(1, 0.0, 1.0)
            assert ctx.eval_var_sums(0, 0.0, 1.0)[0] == 2
            for sigma2 in (0.0, -1.0, float("nan")):
                with pytest.raises(PmfError, match=r"\(-1\).*sigma2"):
                    ctx.eval_var_sums(0, 0.0, sigma2)
            sv = C.c_double(0.0)
            assert ctx._lib.pmf_eval_run_var(ctx._h, 0, 0.0, 1.0, None, C.byref(sv)) == PMF_EINVAL
    with pmf_hip.Context(U, I, K) as ctx:
        for side, rows in ((USER, U), (ITEM, I)):
            ctx.set_array(side, ARR_FACTOR, rng.standard_normal((rows, K)))
            ctx.set_cov_identity(side, 1.0)
        with pytest.raises(PmfError, match=r"\(-1\).*no validation set"):
            ctx.eval_var_sums(0, 0.0, 1.0)


def test_fitted_gradient_model_raises_not_implemented():
    import pandas as pd
    from helpers import skewed_problem
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    u, i, x = skewed_problem(3, 60, 30, 800, rating_kind="centered")
    df = pd.DataFrame({"u": u, "i": i, "rating": x})
    model = GaussianMFSGD(GaussianMFSGDConfig(n_factors=4, max_iter=1, verbose=False)).fit(df)
    try:
        assert model.predict(u[:3], i[:3]).shape == (3,)
        with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
            model.predict_variance(u[:3], i[:3])
        with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
            model.log_predictive_density(df)
    finally:
        model.close()


# ---- 5. profiling ---------------------------------------------------------------------------------------------------
def test_profiler_counts_both_kernels_under_predict_var(case):
    ctx = case(16, "f32").ctx
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.predict_var([0, 1, 2], [0, 1, 2])
    ctx.predict_var([0], [0])
    assert ctx.prof_get()["predict_var"][1] == 2
    assert ctx.eval_set([0, 1, U], [0, 1, 0], [1.0, 2.0, 2.0])
    ctx.eval_var_sums(1, 0.5, 0.3)
    prof = ctx.prof_get()
    assert prof["predict_var"][1] == 3 and prof["predict_var"][0] > 0.0
    assert prof["predict"][1] == 0 and prof["eval"][1] == 0
    ctx.prof_enable(False)
