"""The sums behind the Gaussian ELBO on the device (`pmf_gauss_elbo_terms`, csrc/pmf_gauss.hip) and their model surface
(`elbo`, `fit(track_elbo=, elbo_tol=)`) against dense float64 NumPy (tests/elbo_reference.py: full matrices, per-row and
per-rating loops, `np.linalg.slogdet`), with a derived error bound asserted on every row.

Reference.  FACTOR, COV and BIAS are read back from the device, so the rounding of the inputs is not in the error.

Bounds for fp32 contexts (u = 2^-24; gamma_c = c u / (1 - c u)); fp64 contexts are held to rtol 1e-10 on every term.

SQNORM = |m|^2 + tr V.  A lane adds the diagonal entries of the 16-byte chunks it owns (at most two per chunk) one by
one, then one fma with m_k^2 per element it owns, then the sum over the lanes: 6 levels in a wavefront, 3 more additions
over the four wavefronts of a block (K > 64).  c_sq = 2 ceil(chunks / L) + ceil(K / L) + 9 with chunks = cov_stride / 4
and L = 64 lanes (K <= 64) or 256 (K > 64);  |got - ref| <= gamma_c_sq (sum m_k^2 + sum |V_kk|).

BIAS_SQ = b^2: one rounding.

ESS = c_r - 2 m.w + <V + m m', S>.  S, w and c_r come out of sums over the row's ratings: a task of at most T ratings
(T = `task_max_len`) adds one term per rating, each formed with at most two roundings (the generic accumulate's
acc += fma(m, m, V); the MFMA form rounds once per rating in each of its two chains and adds the chains once; the
residual x - b - b' is two roundings before it is multiplied), the lanes of a c_r task are added in 4 levels, and a
split row adds its n_slots partial sums one by one: c_acc = 2 T + 6 + n_slots.  The row kernel forms fma(m_r, m_c, V)
(1), doubles it off the diagonal (exact), and adds it times S with one fma per chunk the lane owns into one of four sums
(ceil(chunks / L)), adds the four (2), the -2 m_k w_k fma per element it owns (ceil(K / L)), the lanes (6, and 3 over
the wavefronts), and c_r (1):  c_row = 1 + ceil(chunks / L) + 2 + ceil(K / L) + 10.  ESS is a difference of large terms,
so the magnitude is the sum of the absolute values of EVERY product, the rating-level ones behind S, w and c included
(`elbo_reference.side_terms` returns it):  |got - ref| <= gamma_(c_acc + c_row) mag_r + the reference's own
4 (K^2 + n_r) 2^-53 mag_r.  A row without ratings is exactly 0.

LOGDET, derived from the elimination.  The kernel scales V to H = G V G, G = diag(g), g_k = fl(1 / sqrt(V_kk)) (two
roundings per entry: a relative perturbation 2u of H, whose entries are at most 1 + 4u in size), eliminates H
symmetrically without pivoting (LDL^T, pivots only; one multiply by the reciprocal pivot and one fma per update) and
returns sum_k log d_k - 2 log g_k, the logarithms and their sum in double.  -2 sum log g_k is the exact log det of
G^-2 for the g actually used, so what is left is the error of log det H.  By the backward error result for LDL^T /
Cholesky of a symmetric positive definite matrix (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
Theorem 10.3, with one more rounding for the reciprocal), the computed pivots are the exact ones of H + dH with
|dH_ij| <= gamma_(c_ij) (|L||D||L'|)_ij, c_ij = min(i, j) + 4 (entry (i, j) takes min(i, j) updates, the division, and
margin), to which the scaling adds 2u |H_ij|: |dH| <= W.  |L||D||L'| = |C||C'| with the float64 Cholesky factor C of H
from the matrices read back; its off-diagonal entries are well below the Cauchy-Schwarz bound 1, which is what makes
this bound several times smaller than the one with |dH_ij| <= gamma_(K+4) throughout.
log det(H + dH) - log det H = tr(H^-1 dH) + r with |tr(H^-1 dH)| <= sum_ij |H^-1_ij| W_ij =: e and
|r| <= ||H^-1 dH||_F^2 <= (||H^-1||_F ||W||_F)^2 =: f^2 while f < 1/2 (asserted):
    |got - ref| <= e + f^2 + 8 K 2^-53 (|ref| + 1)
(the last term: K double logarithms and their sum, and slogdet's own rounding).  It is a worst-case bound and stays
orders of magnitude above the errors seen on an MI355X, which the test prints (9e-8 at K = 1, 3e-6 at K = 32, 8e-6 at
K = 64): every rounding is taken at its largest and with the same sign.

No tolerance below is a number found by running the kernel."""
import ctypes as C

import numpy as np
import pytest

import elbo_reference as ref
from helpers import skewed_problem

pytestmark = pytest.mark.gpu

PMF_EINVAL, PMF_ERANGE = -1, -4                    # include/pmf_hip.h
U, I, NNZ = 37, 29, 1500
F32_KS = [1, 3, 5, 8, 12, 16, 17, 32, 33, 64, 65, 80, 128, 129, 256]
F64_KS = [5, 16, 64, 129]
CASES = [(K, "f32") for K in F32_KS] + [(K, "f64") for K in F64_KS]
SIGMA2, ETA_T, ETA_B, ETA_BIAS = 0.3, 0.5, 0.7, 1.0
U32 = 2.0 ** -24


def _gamma(c, unit=U32):
    return c * unit / (1.0 - c * unit)


def _spd_rows(rng, rows, K):
    """a different SPD matrix per row: A A' / K + 0.1 I"""
    A = rng.standard_normal((rows, K, K))
    return A @ A.transpose(0, 2, 1) / K + 0.1 * np.eye(K)


def _problem():
    u, i, x = skewed_problem(7, U, I, NNZ, "centered")
    return u.astype(np.int64), i.astype(np.int64), x


def _logdet_bound(V, K, ld_ref):
    d = np.sqrt(np.diagonal(V, axis1=1, axis2=2))
    H = V / d[:, :, None] / d[:, None, :]
    Hinv, C = np.linalg.inv(H), np.abs(np.linalg.cholesky(H))
    idx = np.arange(K)
    count = np.minimum(idx[:, None], idx[None, :]) + 4.0              # updates of entry (i, j), the division, margin
    W = _gamma(count) * (C @ C.transpose(0, 2, 1)) + 2.0 * U32 * np.abs(H)
    e = (np.abs(Hinv) * W).sum(axis=(1, 2))
    fro = np.sqrt((Hinv * Hinv).sum(axis=(1, 2)) * (W * W).sum(axis=(1, 2)))
    assert (fro < 0.5).all()
    return e + fro * fro + 8.0 * K * 2.0 ** -53 * (np.abs(ld_ref) + 1.0)


class _Case:
    """One context of the 37 x 29 problem with standard-normal means, per-row SPD covariances and -- once `add_bias`
    has been called -- standard-normal biases; the reference terms of both sides for the state read back."""

    def __init__(self, K, dtype):
        import pmf_hip
        from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
        self.K, self.f64 = K, dtype == "f64"
        self.u, self.i, self.x = _problem()
        rng = np.random.default_rng(7000 + K)
        self.ctx = ctx = pmf_hip.Context(U, I, K, dtype=dtype)
        ctx.set_ratings(self.u, self.i, self.x)
        for side, rows in ((USER, U), (ITEM, I)):
            ctx.set_array(side, ARR_FACTOR, rng.standard_normal((rows, K)))
            ctx.set_array(side, ARR_COV, _spd_rows(rng, rows, K))
        self.rng = rng
        self.m = [ctx.get_array(s, ARR_FACTOR) for s in (USER, ITEM)]
        self.V = [ctx.get_array(s, ARR_COV) for s in (USER, ITEM)]
        self.b = [np.zeros(U), np.zeros(I)]
        self.ids = [(self.u, self.i), (self.i, self.u)]
        self.stats = [ref.row_stats(self.m[1 - s], self.V[1 - s], self.ids[s][0], self.ids[s][1], len(self.m[s])) for s in (0, 1)]
        self.has_bias = False
        self._refs = {}

    def add_bias(self):
        from pmf_hip import ARR_BIAS, ITEM, USER
        for side, rows in ((USER, U), (ITEM, I)):
            self.ctx.set_array(side, ARR_BIAS, self.rng.standard_normal(rows))
        self.b = [self.ctx.get_array(s, ARR_BIAS) for s in (USER, ITEM)]
        self.has_bias = True
        self._refs = {}

    def reference(self, side):
        """(terms (rows, 4), magnitude of ESS (rows,)) of `side`, computed once per bias state"""
        if side not in self._refs:
            o = 1 - side
            self._refs[side] = ref.side_terms(self.m[side], self.V[side], self.b[side], self.m[o], self.V[o], self.b[o],
                                              self.ids[side][0], self.ids[side][1], self.x, stats=self.stats[side])
        return self._refs[side]

    def counts(self, side):
        return np.bincount(self.ids[side][0], minlength=len(self.m[side]))

    def bounds(self, side):
        """(rows, 4) error bounds of the four terms (module docstring)"""
        terms, mag = self.reference(side)
        K, ctx = self.K, self.ctx
        n = self.counts(side)
        out = np.zeros((len(n), 4))
        if self.f64:
            out[:] = 1e-10 * np.abs(terms)
            return out
        chunks, L = ctx.cov_stride // 4, 64 if K <= 64 else 256
        per_lane, per_k = -(-chunks // L), -(-K // L)
        T = ctx.task_max_len(side, "gauss")
        n_slots = int(np.max(np.where(n > T, -(-n // max(T, 1)), 0)))
        m, V = self.m[side], self.V[side]
        out[:, ref.SQNORM] = _gamma(2 * per_lane + per_k + 9) * ((m * m).sum(axis=1) + np.abs(np.diagonal(V, axis1=1, axis2=2)).sum(axis=1))
        out[:, ref.LOGDET] = _logdet_bound(V, K, terms[:, ref.LOGDET])
        out[:, ref.BIAS_SQ] = _gamma(1) * self.b[side] ** 2
        c_ess = (2 * T + 6 + n_slots) + (1 + per_lane + 2 + per_k + 10)
        out[:, ref.ESS] = (_gamma(c_ess) + 4.0 * (K * K + n) * 2.0 ** -53) * mag
        return out

    def check(self, side, with_data, what):
        terms, _ = self.reference(side)
        want = np.array(terms, dtype=np.float64)
        if not with_data:
            want[:, ref.ESS] = 0.0
        totals, rows = self.ctx.gauss_elbo_terms(side, with_data=with_data, per_row=True)
        err, bound = np.abs(rows - want), self.bounds(side)
        names = ("SQNORM", "LOGDET", "BIAS_SQ", "ESS")
        print(f"{what}: " + ", ".join(f"{names[t]} err {err[:, t].max():.3g} (bound {bound[:, t].max():.3g})" for t in range(4)))
        for t in range(4):
            bad = np.flatnonzero(~(err[:, t] <= bound[:, t]))
            assert bad.size == 0, f"{what}: {names[t]} of row {bad[0]}: got {rows[bad[0], t]!r}, want {want[bad[0], t]!r}, bound {bound[bad[0], t]:.3g}"
        empty = self.counts(side) == 0
        assert empty.any() and (rows[empty, ref.ESS] == 0.0).all()
        if not self.has_bias:
            assert (rows[:, ref.BIAS_SQ] == 0.0).all()
        # totals: the per-row values added in row order, in double
        acc = np.zeros(4)
        for r in range(len(rows)):
            acc += rows[r]
        assert np.array_equal(totals, acc)
        assert (np.abs(totals - rows.sum(axis=0)) <= len(rows) * 2.0 ** -52 * np.abs(rows).sum(axis=0)).all()
        return totals, rows

    def close(self):
        self.ctx.close()


# ---- 1. per-row terms against NumPy ---------------------------------------------------------------------------------
def test_problem_has_empty_rows_duplicates_and_a_row_longer_than_a_task():
    import pmf_hip
    from pmf_hip import ITEM, USER
    u, i, x = _problem()
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    assert len(nu) == U and len(ni) == I and (nu == 0).any() and (ni == 0).any()
    assert len(np.unique(u * I + i)) < len(u)                       # duplicate (u, i) pairs are kept
    with pmf_hip.Context(U, I, 8) as ctx:
        ctx.set_ratings(u, i, x)
        for side, n in ((USER, nu), (ITEM, ni)):
            T = ctx.task_max_len(side, "gauss")
            assert T <= 32 < n.max()                                 # 32-rating tasks: the split path runs on both sides
    pads = set()
    for K in F32_KS:
        with pmf_hip.Context(U, I, K) as ctx:
            pads.add(ctx.cov_stride - K * (K + 1) // 2)
    assert pads == {0, 1, 2, 3}                                      # every K (K + 1) / 2 mod 4 (1 pad entry: K = 5 only)


@pytest.mark.parametrize("K,dtype", CASES)
def test_per_row_terms_against_numpy(K, dtype):
    """Both sides, with and without the data term, without and then with BIAS arrays; two calls are bit-identical; the
    doubles behind the end of `per_row` keep their value."""
    import pmf_hip
    from pmf_hip import ELBO_TERMS, ITEM, USER
    case = _Case(K, dtype)
    try:
        for with_bias in (False, True):
            if with_bias:
                case.add_bias()
            for side in (USER, ITEM):
                for with_data in (False, True):
                    what = f"K={K} {dtype} side={side} data={with_data} bias={with_bias}"
                    totals, rows = case.check(side, with_data, what)
                    totals2, rows2 = case.ctx.gauss_elbo_terms(side, with_data=with_data, per_row=True)
                    assert totals.tobytes() == totals2.tobytes() and rows.tobytes() == rows2.tobytes(), what
                    assert case.ctx.gauss_elbo_terms(side, with_data=with_data).tobytes() == totals.tobytes(), what
        # the raw call into a longer buffer: nothing is written behind rows x PMF_ELBO_TERMS
        lib, n = pmf_hip.load(), U * ELBO_TERMS
        buf, tot = np.full(n + 16, 7.25), np.zeros(ELBO_TERMS)
        assert lib.pmf_gauss_elbo_terms(case.ctx._h, USER, 1, pmf_hip.ptr(tot, C.c_double), pmf_hip.ptr(buf, C.c_double)) == 0
        assert (buf[n:] == 7.25).all() and buf[:n].tobytes() == rows_of(case, USER).tobytes()
    finally:
        case.close()


def rows_of(case, side):
    return case.ctx.gauss_elbo_terms(side, with_data=True, per_row=True)[1]


def test_fp64_triangle_in_global_scratch():
    """fp64 at K = 256: the packed triangle (263 KB) does not fit the LDS, so the row kernel eliminates in its block's
    slice of a global scratch buffer.  Held to the fp64 tolerance on both sides."""
    from pmf_hip import ITEM, USER
    case = _Case(256, "f64")
    try:
        case.add_bias()
        for side in (USER, ITEM):
            case.check(side, True, f"K=256 f64 side={side}")
    finally:
        case.close()


# ---- 2. windows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 80])
def test_row_windows_change_no_bit(K, monkeypatch):
    """PMF_ELBO_ROWS = 1, 7 and unset (one window): the same state gives the same bits, per row and in total."""
    from pmf_hip import ITEM, USER
    got = []
    for rows in ("1", "7", None):
        if rows is None:
            monkeypatch.delenv("PMF_ELBO_ROWS", raising=False)
        else:
            monkeypatch.setenv("PMF_ELBO_ROWS", rows)
        case = _Case(K, "f32")
        try:
            case.add_bias()
            got.append([case.ctx.gauss_elbo_terms(side, with_data=True, per_row=True) for side in (USER, ITEM)])
            if rows == "7":
                case.check(USER, True, f"K={K} windows of 7 rows")
        finally:
            case.close()
    for other in got[1:]:
        for (t0, r0), (t1, r1) in zip(got[0], other):
            assert t0.tobytes() == t1.tobytes() and r0.tobytes() == r1.tobytes()


# ---- 3. two routes to the data term ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", [(8, "f32"), (33, "f32"), (80, "f32"), (16, "f64")])
def test_data_term_from_either_side_and_per_rating(K, dtype):
    from pmf_hip import ELBO_ESS, ITEM, USER
    case = _Case(K, dtype)
    try:
        case.add_bias()
        ess = [case.ctx.gauss_elbo_terms(side, with_data=True)[ELBO_ESS] for side in (USER, ITEM)]
        bound = [case.bounds(side)[:, ref.ESS].sum() for side in (USER, ITEM)]
        per_rating = float(ref.ess_per_rating(case.m[0], case.V[0], case.b[0], case.m[1], case.V[1], case.b[1], case.u, case.i, case.x))
        own = 4.0 * (K * K + 8) * 2.0 ** -53 * sum(case.reference(USER)[1])       # the per-rating sum's own rounding
        print(f"K={K} {dtype}: ESS user {ess[0]!r} item {ess[1]!r} per rating {per_rating!r}; bounds {bound[0]:.3g} {bound[1]:.3g}")
        assert abs(ess[0] - ess[1]) <= bound[0] + bound[1]
        assert abs(ess[0] - per_rating) <= bound[0] + own and abs(ess[1] - per_rating) <= bound[1] + own
    finally:
        case.close()


# ---- 4. monotone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("K", [3, 8, 80])
def test_elbo_never_drops_over_the_half_sweeps_of_a_fit(K, bias):
    """fp64 contexts, the problem and hyperparameters of tests/test_elbo_cpu.py, 4 iterations issued half-sweep by
    half-sweep in the reference's order.  L from the device's sums never drops by more than 1e-9 |L| (the NumPy steps at
    these shapes are >= +1.25) and equals the NumPy ELBO of the state read back at rtol 1e-10."""
    import pmf_hip
    from oracle import cavi_oracle as orc
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER
    from src.models._gaussian_host import elbo_from_terms
    u, i, x = skewed_problem(K, 90, 40, 2500, "centered")
    nU, nI = orc.infer_dims(u, i)
    st = orc.init_gaussian(nU, nI, K, seed=K, bias=bias)
    nu, ni = np.bincount(u, minlength=nU), np.bincount(i, minlength=nI)
    eta_bias2 = ETA_BIAS if bias else None
    with pmf_hip.Context(nU, nI, K, dtype="f64") as ctx:
        ctx.set_ratings(u, i, x)
        ctx.set_array(USER, ARR_FACTOR, st["m_theta"])
        ctx.set_array(ITEM, ARR_FACTOR, st["m_beta"])
        ctx.set_cov_identity(USER, 1.0)
        ctx.set_cov_identity(ITEM, 1.0)
        if bias:
            ctx.set_array(USER, ARR_BIAS, st["m_user_bias"])
            ctx.set_array(ITEM, ARR_BIAS, st["m_item_bias"])

        def value():
            user = ctx.gauss_elbo_terms(USER, with_data=True)
            item = ctx.gauss_elbo_terms(ITEM, with_data=False)
            L = elbo_from_terms(user, item, nu, ni, len(x), K, SIGMA2, ETA_T, ETA_B, eta_bias2)[0]
            back = {"m_theta": ctx.get_array(USER, ARR_FACTOR), "V_theta": ctx.get_array(USER, ARR_COV),
                    "m_beta": ctx.get_array(ITEM, ARR_FACTOR), "V_beta": ctx.get_array(ITEM, ARR_COV)}
            if bias:
                back["m_user_bias"], back["m_item_bias"] = ctx.get_array(USER, ARR_BIAS), ctx.get_array(ITEM, ARR_BIAS)
            want = ref.elbo(back, u, i, x, SIGMA2, ETA_T, ETA_B, eta_bias2, data="item")
            assert abs(L - want) <= 1e-10 * abs(want), (L, want)
            return L
        sweeps = [lambda: ctx.gauss_factor_sweep(USER, SIGMA2, ETA_T), lambda: ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA_B)]
        if bias:
            sweeps += [lambda: ctx.gauss_bias_sweep(USER, SIGMA2, ETA_BIAS), lambda: ctx.gauss_bias_sweep(ITEM, SIGMA2, ETA_BIAS)]
        values = [value()]
        for _ in range(4):
            for sweep in sweeps:
                sweep()
                values.append(value())
        steps = np.diff(values)
        print(f"K={K} bias={bias}: L from {values[0]:.3f} to {values[-1]:.3f}, smallest step {steps.min():.4g}")
        assert len(values) == 1 + 4 * len(sweeps)
        assert (steps >= -1e-9 * np.abs(values[:-1])).all(), steps


# ---- 5. read-only ---------------------------------------------------------------------------------------------------
def test_the_call_reads_only():
    """State arrays and the stored validation set's sums are the same bits after a call, and a factor sweep after a
    call gives the bits it gives without one."""
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER
    cases = [_Case(12, "f32"), _Case(12, "f32")]
    try:
        for c in cases:
            c.add_bias()
        a, b = cases
        vu, vi = np.arange(40) % U, (np.arange(40) * 7) % I
        vy = np.round(np.sin(np.arange(40.0)) * 2.0)
        assert a.ctx.eval_set(vu, vi, vy)

        def state(ctx):
            return [ctx.get_array(s, arr).tobytes() for s in (USER, ITEM) for arr in (ARR_FACTOR, ARR_COV, ARR_BIAS)]
        before, sums = state(a.ctx), np.asarray(a.ctx.eval_sums(True, 0.5)).tobytes()
        for side in (USER, ITEM):
            for with_data in (False, True):
                a.ctx.gauss_elbo_terms(side, with_data=with_data, per_row=True)
        assert state(a.ctx) == before
        assert np.asarray(a.ctx.eval_sums(True, 0.5)).tobytes() == sums
        assert state(b.ctx) == before                      # the twin context holds the same state, and never ran the call
        for ctx in (a.ctx, b.ctx):
            ctx.gauss_factor_sweep(USER, SIGMA2, ETA_T)
            ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA_B)
        assert state(a.ctx) == state(b.ctx) and state(a.ctx) != before
    finally:
        for c in cases:
            c.close()


# ---- 6. model surface -----------------------------------------------------------------------------------------------
def _fit(dtype, bias=True, verbose=False, **kw):
    import importlib

    import pandas as pd
    mod = importlib.import_module("src.models." + ("gaussian_mf_cavi_bias" if bias else "gaussian_mf_cavi"))
    u, i, x = skewed_problem(12, 90, 40, 2500, "centered")
    hyper = dict(n_factors=12, sigma2=SIGMA2, eta_theta2=ETA_T, eta_beta2=ETA_B, max_iter=3, tol=-1.0, random_state=3, verbose=verbose)
    if bias:
        hyper["eta_bias2"] = ETA_BIAS
    model = mod.GaussianMFCAVI(mod.GaussianMFCAVIConfig(**hyper), dtype=dtype)
    return model.fit(pd.DataFrame({"u": u, "i": i, "rating": x}), **kw)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fit_tracks_the_elbo(dtype, bias):
    tracked, plain = _fit(dtype, bias, track_elbo=True), _fit(dtype, bias)
    try:
        L = tracked.history_["elbo"]
        assert len(L) == 3 and tracked.history_["iterations"] == 3 and not tracked.history_["stopped_early"]
        if dtype == "f64":
            assert L[0] <= L[1] <= L[2]
        assert tracked.elbo() == L[-1]
        value, parts = tracked.elbo(parts=True)
        assert value == L[-1] and abs(sum(parts.values()) - value) <= 1e-12 * abs(value)
        # tracking changes no bit of the fit, and the default fit has no trace of it
        assert "elbo" not in plain.history_
        for name in ("m_theta", "m_beta", "V_theta", "V_beta") + (("m_user_bias", "m_item_bias") if bias else ()):
            assert getattr(tracked, name).tobytes() == getattr(plain, name).tobytes(), name
        assert plain.elbo() == L[-1]
    finally:
        tracked.close()
        plain.close()


def test_elbo_tol_stops_without_a_validation_frame():
    model = _fit("f32", elbo_tol=1.0)
    try:
        assert model.history_["iterations"] == 2 and model.history_["stopped_early"] and len(model.history_["elbo"]) == 2
    finally:
        model.close()


def test_default_fit_prints_what_it_printed(capsys):
    """With the two arguments left alone the text is the tracked fit's minus its ELBO lines."""
    plain = _fit("f32", verbose=True)
    text_plain = capsys.readouterr().out
    tracked = _fit("f32", verbose=True, track_elbo=True)
    text_tracked = capsys.readouterr().out
    plain.close()
    tracked.close()
    assert "ELBO" not in text_plain and "CAVI iteration 3/3" in text_plain
    lines = text_tracked.splitlines(keepends=True)
    elbo_lines = [ln for ln in lines if ln.startswith("ELBO: ")]
    assert len(elbo_lines) == 3 and elbo_lines[-1] == f"ELBO: {tracked.history_['elbo'][-1]:.4f}\n"
    assert "".join(ln for ln in lines if not ln.startswith("ELBO: ")) == text_plain


def test_gradient_model_refuses():
    import pandas as pd
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    u, i, x = skewed_problem(12, 90, 40, 2500, "centered")
    model = GaussianMFSGD(GaussianMFSGDConfig(n_factors=4, max_iter=1, verbose=False)).fit(pd.DataFrame({"u": u, "i": i, "rating": x}))
    try:
        with pytest.raises(NotImplementedError, match="GaussianMFSGD"):
            model.elbo()
    finally:
        model.close()


# ---- 7. refusals and a row that is not positive definite ------------------------------------------------------------
def test_refusals():
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    lib = pmf_hip.load()
    tot = np.full(4, 7.0)
    rows = np.full(U * 4, 7.0)
    pt, pr = pmf_hip.ptr(tot, C.c_double), pmf_hip.ptr(rows, C.c_double)

    def refused(ctx, side, with_data, totals, code, text):
        h = ctx._h if ctx is not None else None
        assert lib.pmf_gauss_elbo_terms(h, side, with_data, totals, pr) == code
        assert text in lib.pmf_last_error().decode(), lib.pmf_last_error()
        assert (tot == 7.0).all() and (rows == 7.0).all()           # an argument error writes nothing
    u, i, x = _problem()
    rng = np.random.default_rng(1)
    with pmf_hip.Context(U, I, 5) as ctx:
        refused(None, USER, 0, pt, PMF_EINVAL, "null context")
        refused(ctx, 2, 0, pt, PMF_EINVAL, "bad side 2")
        refused(ctx, -1, 1, pt, PMF_EINVAL, "bad side -1")
        refused(ctx, USER, 0, None, PMF_EINVAL, "null totals")
        refused(ctx, USER, 0, pt, PMF_EINVAL, "array FACTOR of side 0")
        ctx.set_array(USER, ARR_FACTOR, rng.standard_normal((U, 5)))
        refused(ctx, USER, 0, pt, PMF_EINVAL, "array COV of side 0")
        ctx.set_array(USER, ARR_COV, _spd_rows(rng, U, 5))
        refused(ctx, USER, 1, pt, PMF_EINVAL, "array FACTOR of side 1")
        refused(ctx, ITEM, 0, pt, PMF_EINVAL, "array FACTOR of side 1")
        ctx.set_array(ITEM, ARR_FACTOR, rng.standard_normal((I, 5)))
        refused(ctx, USER, 1, pt, PMF_EINVAL, "array COV of side 1")
        ctx.set_array(ITEM, ARR_COV, _spd_rows(rng, I, 5))
        refused(ctx, USER, 1, pt, PMF_EINVAL, "ratings have not been set")
        # without the data term no ratings are needed
        got = ctx.gauss_elbo_terms(USER, with_data=False)
        assert np.isfinite(got).all() and got[3] == 0.0 and got[2] == 0.0
        ctx.set_ratings(u, i, x)
        assert np.isfinite(ctx.gauss_elbo_terms(USER, with_data=True)).all()
    # n_factors > 256 never reaches the entry point: a context refuses such a K
    h = C.c_void_p()
    assert lib.pmf_ctx_create(0, U, I, 257, pmf_hip.F32, C.byref(h)) == PMF_ERANGE and not h


@pytest.mark.parametrize("K,dtype", [(8, "f32"), (80, "f32"), (16, "f64")])
def test_a_row_that_is_not_positive_definite_is_nan_and_nothing_else(K, dtype):
    from pmf_hip import ARR_COV, USER
    case = _Case(K, dtype)
    try:
        case.add_bias()
        bad = 5
        assert case.counts(USER)[bad] > 0
        case.ctx.set_array_rows(USER, ARR_COV, [bad], -np.eye(K)[None])
        case.V[0] = case.ctx.get_array(USER, ARR_COV)
        totals, rows = case.ctx.gauss_elbo_terms(USER, with_data=True, per_row=True)     # return code 0: no exception
        assert np.isnan(rows[bad, ref.LOGDET]) and np.isnan(totals[ref.LOGDET])
        assert np.isfinite(np.delete(totals, ref.LOGDET)).all() and np.isfinite(np.delete(rows, bad, axis=0)).all()
        case.V[0][bad] = np.eye(K)                     # the bound's H^-1 needs a matrix there; the row itself is not compared
        terms, _ = case.reference(USER)
        err, bound = np.abs(rows - terms), case.bounds(USER)
        keep = np.arange(U) != bad
        assert (err[keep] <= bound[keep]).all()
        # the bad row's other terms are those of V = -I
        m = case.m[0][bad]
        assert abs(rows[bad, ref.SQNORM] - ((m * m).sum() - K)) <= 1e-5 * ((m * m).sum() + K)
    finally:
        case.close()


# ---- 8. rows beyond 2^31 elements -----------------------------------------------------------------------------------
def test_row_offsets_beyond_2_31_elements():
    """K = 64 fp32, 1,040,000 users x 11 items: cov_stride = 2080, so user rows from 1,032,445 start beyond 2^31 elements
    of the table.  Identity covariances and zero means everywhere except five rows (0, the edge - 1, the edge, the
    edge + 1, the last), which hold all the ratings; one of them is longer than a task.  Those rows against NumPy within
    the bounds of test 1; an untouched row is exactly (K, 0, 0, 0)."""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER
    K, NU, NI = 64, 1_040_000, 11
    rng = np.random.default_rng(64)
    with pmf_hip.Context(NU, NI, K) as ctx:
        assert ctx.cov_stride == 2080
        edge = -(-2 ** 31 // ctx.cov_stride)
        rows = np.array([0, edge - 1, edge, edge + 1, NU - 1], np.int64)
        assert edge == 1_032_445 and ((rows * ctx.cov_stride >= 2 ** 31) == [False, False, True, True, True]).all()
        lengths = [3, 7, 45, 1, 20]
        u = np.repeat(rows, lengths)
        i = rng.integers(0, NI, len(u))
        x = rng.standard_normal(len(u))
        ctx.set_ratings(u, i, x)
        assert ctx.task_max_len(USER, "gauss") <= 32 < max(lengths)
        ctx.set_cov_identity(USER, 1.0)
        ctx.set_array_rows(USER, ARR_FACTOR, rows, rng.standard_normal((len(rows), K)))
        ctx.set_array_rows(USER, ARR_COV, rows, _spd_rows(rng, len(rows), K))
        ctx.set_array_rows(USER, ARR_BIAS, rows, rng.standard_normal(len(rows)))
        ctx.set_array(ITEM, ARR_FACTOR, rng.standard_normal((NI, K)))
        ctx.set_array(ITEM, ARR_COV, _spd_rows(rng, NI, K))
        ctx.set_array(ITEM, ARR_BIAS, rng.standard_normal(NI))
        totals, got = ctx.gauss_elbo_terms(USER, with_data=True, per_row=True)
        # the five rows as a 5-row side of their own
        case = _Case.__new__(_Case)
        case.K, case.f64, case.ctx, case.has_bias, case._refs = K, False, ctx, True, {}
        local = np.repeat(np.arange(len(rows)), lengths)
        case.u, case.i, case.x = local, i, x
        case.m = [ctx.get_array_rows(USER, ARR_FACTOR, rows), ctx.get_array(ITEM, ARR_FACTOR)]
        case.V = [ctx.get_array_rows(USER, ARR_COV, rows), ctx.get_array(ITEM, ARR_COV)]
        case.b = [ctx.get_array_rows(USER, ARR_BIAS, rows), ctx.get_array(ITEM, ARR_BIAS)]
        case.ids = [(local, i), (i, local)]
        case.stats = [ref.row_stats(case.m[1], case.V[1], local, i, len(rows)), None]
        terms, _ = case.reference(USER)
        err, bound = np.abs(got[rows] - terms), case.bounds(USER)
        print("rows beyond 2^31: err", err.max(axis=0), "bound", bound.max(axis=0))
        assert (err <= bound).all(), (err, bound)
        untouched = np.ones(NU, bool)
        untouched[rows] = False
        assert (got[untouched] == np.array([float(K), 0.0, 0.0, 0.0])).all()
        assert np.isfinite(totals).all()
