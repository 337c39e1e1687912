"""Unlisted cells counted as zeros on the device (`pmf_ctx_set_gamma_zeros`, PMF_ZEROS_OBSERVED; `fit(unobserved="zero")`)
against tests/gamma_implicit_reference.py (dense float64), evaluated on the state read back from the device (so the
rounding of the inputs is not part of the error), every row and every element; against the existing calls on the same
matrix with every missing cell listed as an explicit 0; then the model surface and the refusals.

The shared problem P is `gamma_implicit_reference.problem_p()`: 90 x 70, 1984 distinct pairs, every eleventh rating 0,
rows split over several 32-rating tasks and empty rows on both sides (asserted).  D is P plus an explicit 0 for each of
the 4316 other cells.

Bounds.  None is a number found by running the kernels.  eps is the unit roundoff 2^-24 (fp32) or 2^-53 (fp64) of the
context, R the rows that are summed, n_r the listed ratings of row r.

Column sum  C_k = sum_r v_rk, v > 0 exact inputs (read back), every addition in double, each value passing through at
most R additions of half an ulp of a partial sum below C:  |got - ref| <= R 2^-53 C.  From q (v = SHAPE / RATE as the
(E log, E) table holds it) one eps of C more: the quotient is rounded to the context's dtype, the reference is not.

Shape sums.  Exact update: the bound tests/test_gamma_exact_gpu.py derives, unchanged (same code, same ratings),
    eps (n_r + (K + 16)(1 + M_r)) A_rk + 2^-126 sum_j x_j.
Reference update: no existing test derives a bound for it (tests/test_gamma_gpu.py holds it to a relative 1e-12 / 2e-5
after one update); the following is a new derivation, tighter than that.  A_rk = sum_j x_j E_ok E_rk / (E_o . E_r): the dot product of positive terms is four fused steps per
lane and at most six DPP steps, below eps (4 + log2 K) relative; the quotient and the two products one rounding each:
below eps (K + 16) / 2 relative per addend for every K >= 1; every value passes through at most n_r additions:
    eps (n_r + K + 16) A_rk.
The float64 NumPy reference forms the same quotient, products and n_r additions, so in a float64 context its own error,
2^-53 (n_r + K + 16) A_rk by the same derivation, is as large as the device's: it is added to the bound of this update
(negligible in fp32; the exact update's bound has the room).
SHAPE = prior + A: that plus one eps of the value, the device's final rounding.  The reference adds the priors, divides
and sums the factors in extended precision (np.longdouble), so that it does not round a second time where the bounds
count one rounding.

RATE = prior_r + C:  the column sum's bound, one eps of C for its conversion to the context's dtype, one eps of the
value for the addition.  Explicit zeros (MISSING mode on D): the rate sum is n_r table entries added in the context's
dtype, eps (n_r + 2) B as tests/test_gamma_exact_gpu.py derives, plus one eps of the value.
FACTOR, HYPER_RATE and PRIOR_RATE follow from those as in tests/test_gamma_exact_gpu.py.

DATA_r = sum_j x_j lse_j - E_r . C:  the bound tests/test_gamma_elbo_gpu.py derives for the x lse part,
eps (n_r + K + 16) sum_j x_j (max_k |Elog_rk| + max_k |Elog_ok| + |lse_j|), plus
(K + R_other 2^-53 / eps + 3) eps E_r . C for the product (K additions, the column sum, three conversions).

Fold-in: tests/test_gamma_fold_in_gpu.py's bounds by the number of updates (1: 1e-12 / 2e-5; up to 20: 1e-9 / 5e-4,
used for 10); B is the column sum, whose own bound (R 2^-53 + 2 eps) is far inside them.

The model surface is held to the project's f64 parity bar, rtol 1e-9.
Worst fractions of these bounds measured on an MI355X (printed by the tests): DESIGN.md section 4.16."""
import ctypes as C
import multiprocessing as mp
import os
import sys

import numpy as np
import pandas as pd
import pytest
from scipy.special import logsumexp

import gamma_elbo_reference as ref
import gamma_implicit_reference as zref
import test_gamma_exact_gpu as ex
from gamma_fold_in_reference import TOL, batch
from helpers import gamma_stats, rel_err

pytestmark = pytest.mark.gpu

PMF_EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I = 90, 70
EPS, NP, HIER, FLAT, KAPPA, SIDE_KEYS = ex.EPS, ex.NP, ex.HIER, ex.FLAT, ex.KAPPA, ex.SIDE_KEYS
CASES = [(K, dtype) for dtype in ("f32", "f64") for K in (3, 20, 64, 100)]
COLSUM_ROWS = (1, 255, 256, 257, 20011)

_SHARED = {}


def _problems():
    """(P, D), built once and never changed"""
    if not _SHARED:
        P = zref.problem_p(5, U, I, 4000)
        D = zref.dense_completion(*P, U, I)
        for a in P + D:
            a.setflags(write=False)
        _SHARED["P"], _SHARED["D"] = P, D
    return _SHARED["P"], _SHARED["D"]


def test_problem_has_split_rows_and_empty_rows_on_both_sides():
    import pmf_hip
    from pmf_hip import ITEM, USER
    (u, i, x), D = _problems()
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    assert len(u) == 1984 and nu.max() == 67 and ni.max() == 87 and (nu == 0).sum() == 3 and (ni == 0).sum() == 2
    assert len(D[0]) == U * I
    with pmf_hip.Context(U, I, 3) as ctx:
        ctx.set_ratings(u, i, x)
        assert ctx.task_max_len(USER, "gamma") <= 32 and ctx.task_max_len(ITEM, "gamma") <= 32    # the default task length
        assert ctx.gamma_zeros is False
        ctx.set_gamma_zeros(True)
        assert ctx.gamma_zeros is True
        ctx.set_gamma_zeros(False)
        assert ctx.gamma_zeros is False


# ---- 1. the column sums -----------------------------------------------------------------------------------------------
def _colsum_arrays(K, rows):
    rng = np.random.default_rng(1000 * K + rows)
    lu = lambda lo, hi, size: np.exp(rng.uniform(np.log(lo), np.log(hi), size=size))
    return rng.gamma(1.0, 0.5, size=(rows, K)) + 1e-3, lu(0.3, 1e4, (rows, K)), lu(0.5, 1e3, (rows, K))


def _colsum_case(K, dtype, rows):
    """({from_q: C}, context arrays read back) of a context with `rows` users"""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ARR_RATE, ARR_SHAPE, USER
    f, a, b = _colsum_arrays(K, rows)
    with pmf_hip.Context(rows, 1, K, dtype=dtype) as ctx:
        for arr, host in ((ARR_FACTOR, f), (ARR_SHAPE, a), (ARR_RATE, b)):
            ctx.set_array(USER, arr, host)
        back = [ctx.get_array(USER, arr) for arr in (ARR_FACTOR, ARR_SHAPE, ARR_RATE)]
        got = {}
        for from_q in (False, True):
            got[from_q] = ctx.gamma_column_sums(USER, from_q=from_q)
            assert ctx.gamma_column_sums(USER, from_q=from_q).tobytes() == got[from_q].tobytes()      # two calls, the same bits
        held = ctx.device_bytes()
        ctx.gamma_column_sums(USER, from_q=True)
        ctx.gamma_column_sums(USER)
        assert ctx.device_bytes() == held                                     # grows on the first calls only
        assert [ctx.get_array(USER, arr).tobytes() for arr in (ARR_FACTOR, ARR_SHAPE, ARR_RATE)] == [h.tobytes() for h in back]
    return got, back


@pytest.mark.parametrize("K,dtype", CASES)
def test_column_sums_against_numpy(K, dtype):
    for rows in COLSUM_ROWS:
        got, (f, a, b) = _colsum_case(K, dtype, rows)
        for from_q, want in ((False, np.sum(f, axis=0)), (True, np.sum(a / b, axis=0))):
            bound = (rows * 2.0 ** -53 + (EPS[dtype] if from_q else 0.0)) * want
            err = np.abs(got[from_q] - want)
            print(f"K={K} {dtype} rows={rows} from_q={from_q}: {np.max(err / bound):.2g} of the bound")
            assert np.isfinite(got[from_q]).all() and (err <= bound).all(), (rows, from_q, np.max(err / bound))


def _task_length_case(K, dtype):
    """On a context that holds P's ratings -- so the work lists exist and are cut at the task length in force -- the
    column sums of both sides and RATE after a zero-mode half-sweep of each side under each update: what must not
    depend on the task length.  Also the longest user task."""
    from pmf_hip import ARR_RATE, ITEM, USER
    P, _ = _problems()
    out = {}
    ctx = _context(K, dtype, P, True)
    try:
        out["longest"] = np.array([ctx.task_max_len(USER, "gamma"), ctx.task_max_len(ITEM, "gamma")])
        drawn = ex._draw_state(K + 7, U, I, K)
        ex._upload(ctx, drawn)
        for side in (USER, ITEM):
            for from_q in (False, True):
                out[f"C_{side}_{int(from_q)}"] = ctx.gamma_column_sums(side, from_q=from_q)
            for exact in (False, True):
                ex._upload(ctx, drawn)
                _sweep(ctx, side, HIER, exact)
                out[f"RATE_{side}_{int(exact)}"] = ctx.get_array(side, ARR_RATE)
    finally:
        ctx.close()
    return out


def _colsum_worker(out_path):
    """A fresh interpreter with another task length: the column sums of every case at 257 rows, and `_task_length_case`."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd"), os.path.join(ROOT, "tests")]
    os.environ["PMF_TASK_CHUNK"] = "64"
    out = {}
    for K, dtype in CASES:
        got, _ = _colsum_case(K, dtype, 257)
        out[f"{K}_{dtype}_0"], out[f"{K}_{dtype}_1"] = got[False], got[True]
        for name, value in _task_length_case(K, dtype).items():
            out[f"{K}_{dtype}_{name}"] = value
    np.savez(out_path, **out)


def test_column_sums_do_not_depend_on_the_task_length(tmp_path, monkeypatch):
    monkeypatch.delenv("PMF_TASK_CHUNK", raising=False)
    path = str(tmp_path / "colsum.npz")
    proc = mp.get_context("spawn").Process(target=_colsum_worker, args=(path,))
    proc.start()
    proc.join(120)
    if proc.is_alive():
        proc.kill()
        proc.join()
        raise AssertionError("the child hung")
    assert proc.exitcode == 0
    child = np.load(path)
    for K, dtype in CASES:
        got, _ = _colsum_case(K, dtype, 257)
        for from_q in (False, True):
            assert child[f"{K}_{dtype}_{int(from_q)}"].tobytes() == got[from_q].tobytes(), (K, dtype, from_q)
        # with ratings set: other cuts of the rows in the child, the same column sums and the same zero-mode RATE
        here = _task_length_case(K, dtype)
        assert here["longest"].max() <= 32 and child[f"{K}_{dtype}_longest"].min() > 32, (here["longest"], child[f"{K}_{dtype}_longest"])
        for name, value in here.items():
            if name != "longest":
                assert child[f"{K}_{dtype}_{name}"].tobytes() == value.tobytes(), (K, dtype, name)


# ---- 2. / 3. one half-sweep, every row and element ----------------------------------------------------------------------
def _expected(st, side, ratings, prior, prior_rate_vec, dtype, exact, zeros):
    """({array: reference}, {array: allowed |got - ref|}, ratings per row) of one half-sweep of `side` from `st` -- for
    the reference update `st` holds FACTOR as its shapes over rates of 1 -- with unlisted cells as zeros or not."""
    u, i, x = ratings
    hierarchical = prior[2]
    shape_prior, rate_prior, hyper_shape, hyper_rate_prior = (float(NP[dtype](prior[k])) for k in (0, 1, 3, 4))
    eps, K = EPS[dtype], st["a_theta"].shape[1]
    rows, others = (u, i) if side == 0 else (i, u)
    R, R_other = len(st[SIDE_KEYS[side][0]]), len(st[SIDE_KEYS[1 - side][0]])
    A, B = ref.factor_half_sweep(st, side, u, i, x, 0.0, 0.0, exact=exact)
    n = np.bincount(rows, minlength=R).astype(np.float64)
    if exact:
        Ls = ref.expectations(st[SIDE_KEYS[side][0]], st[SIDE_KEYS[side][1]])[1]
        Lo = ref.expectations(st[SIDE_KEYS[1 - side][0]], st[SIDE_KEYS[1 - side][1]])[1]
        lse = logsumexp(Ls[rows] + Lo[others], axis=1)
        M = np.zeros(R)
        np.maximum.at(M, rows, np.abs(Ls).max(axis=1)[rows] + np.abs(Lo).max(axis=1)[others] + np.abs(lse))
        sum_x = np.bincount(rows, weights=x, minlength=R)
        bound_A = eps * (n + (K + 16) * (1.0 + M))[:, None] * A + (2.0 ** -126 * sum_x)[:, None]
    else:
        bound_A = (eps + 2.0 ** -53) * (n + K + 16)[:, None] * A          # (the device's error and the float64 reference's own)
    if zeros:
        Cs = zref.column_sums(st, 1 - side)
        B = np.broadcast_to(Cs, A.shape)
        bound_B = np.broadcast_to((R_other * 2.0 ** -53 + (eps if exact else 0.0) + eps) * Cs, A.shape)
    else:
        bound_B = eps * (n + 2.0)[:, None] * B
    rp = prior_rate_vec if hierarchical else np.full(R, float(rate_prior))
    LD = np.longdouble                  # (the priors, quotients and factor sums of the reference: no second rounding)
    want = {"SHAPE": LD(shape_prior) + A.astype(LD), "RATE": rp.astype(LD)[:, None] + np.asarray(B, dtype=LD)}
    bound = {"SHAPE": bound_A + eps * want["SHAPE"], "RATE": bound_B + eps * want["RATE"]}
    want["FACTOR"] = want["SHAPE"] / want["RATE"]
    bound["FACTOR"] = want["FACTOR"] * (bound["SHAPE"] / want["SHAPE"] + bound["RATE"] / want["RATE"] + eps)
    if hierarchical:
        want["HYPER_RATE"] = LD(hyper_rate_prior) + want["FACTOR"].sum(axis=1)
        bound["HYPER_RATE"] = bound["FACTOR"].sum(axis=1) + 5.0 * eps * want["HYPER_RATE"]
        want["PRIOR_RATE"] = LD(hyper_shape) / want["HYPER_RATE"]
        bound["PRIOR_RATE"] = want["PRIOR_RATE"] * (bound["HYPER_RATE"] / want["HYPER_RATE"] + eps)
    return want, bound, n


def _input_state(ctx, exact):
    """What the update reads, as the device holds it: q (exact), or FACTOR as shapes over rates of 1 (reference)."""
    from pmf_hip import ARR_FACTOR, ITEM, USER
    if exact:
        return ex._device_state(ctx)
    f = {USER: ctx.get_array(USER, ARR_FACTOR), ITEM: ctx.get_array(ITEM, ARR_FACTOR)}
    return {"a_theta": f[USER], "b_theta": np.ones_like(f[USER]), "a_beta": f[ITEM], "b_beta": np.ones_like(f[ITEM])}


def _sweep(ctx, side, prior, exact):
    (ctx.gamma_exact_sweep if exact else ctx.gamma_sweep)(side, *prior)


def _check_sweep(ctx, side, ratings, prior, dtype, exact, zeros, what):
    """One half-sweep from whatever the device holds against the reference computed from that state; returns
    (arrays written, reference, bound)."""
    from pmf_hip import ARR_PRIOR_RATE
    hierarchical = prior[2]
    assert ctx.gamma_zeros is zeros
    st = _input_state(ctx, exact)
    prv = ctx.get_array(side, ARR_PRIOR_RATE) if hierarchical else None
    want, bound, n = _expected(st, side, ratings, prior, prv, dtype, exact, zeros)
    c_dev = ctx.gamma_column_sums(1 - side, from_q=exact) if zeros else None
    _sweep(ctx, side, prior, exact)
    got = ex._outputs(ctx, side, hierarchical)
    worst = {}
    for name in got:
        err = np.abs(got[name] - want[name])
        assert np.isfinite(got[name]).all(), (what, name)
        worst[name] = float(np.max(err / bound[name]))
        assert (err <= bound[name]).all(), (what, name, np.argwhere(err > bound[name])[:5], worst[name])
    print(what, " ".join("%s %.2g" % kv for kv in worst.items()), "(fractions of the bound)")
    if zeros:    # a row without ratings: shape_prior and fl(prior_r + C), to the bit
        T = NP[dtype]
        empty = n == 0
        assert empty.any()
        rpe = prv[empty].astype(T) if hierarchical else np.full(int(empty.sum()), T(prior[1]))
        rate = (rpe[:, None] + c_dev.astype(T)[None, :]).astype(T)
        assert (got["SHAPE"][empty] == T(prior[0])).all(), what
        assert got["RATE"][empty].tobytes() == rate.astype(np.float64).tobytes(), what
        assert got["FACTOR"][empty].tobytes() == (T(prior[0]) / rate).astype(T).astype(np.float64).tobytes(), what
    return got, want, bound


def _context(K, dtype, ratings, zeros):
    import pmf_hip
    ctx = pmf_hip.Context(U, I, K, dtype=dtype)
    ctx.set_ratings(*ratings)
    ctx.set_gamma_zeros(zeros)
    return ctx


@pytest.mark.parametrize("K,dtype", CASES)
def test_half_sweeps_against_the_reference_and_against_explicit_zeros(K, dtype):
    """Both sides, both updates, hierarchical and not, from state (a) of tests/test_gamma_exact_gpu.py: zero mode on P
    within its bounds of the reference; MISSING mode on D within its own; the two within the sum of the two bounds."""
    from pmf_hip import ITEM, USER
    P, D = _problems()
    drawn = ex._draw_state(K, U, I, K)
    sparse, dense = _context(K, dtype, P, True), _context(K, dtype, D, False)
    try:
        for exact in (False, True):
            for side in (USER, ITEM):
                for prior in (HIER, FLAT):
                    what = f"K={K} {dtype} exact={exact} side={side} hier={prior[2]}"
                    ex._upload(sparse, drawn)
                    ex._upload(dense, drawn)
                    got, _, bound = _check_sweep(sparse, side, P, prior, dtype, exact, True, what + " zeros on P:")
                    again = None
                    ex._upload(sparse, drawn)
                    _sweep(sparse, side, prior, exact)
                    again = ex._outputs(sparse, side, prior[2])
                    assert ex._bits(again) == ex._bits(got), what                      # two calls, the same bits
                    listed, _, bound_d = _check_sweep(dense, side, D, prior, dtype, exact, False, what + " explicit on D:")
                    for name in got:
                        err = np.abs(got[name] - listed[name])
                        allowed = bound[name] + bound_d[name]
                        assert (err <= allowed).all(), (what, name, float(np.max(err / allowed)))
    finally:
        sparse.close()
        dense.close()


def test_zero_mode_does_not_grow_the_context_after_the_first_calls():
    from pmf_hip import ITEM, USER
    P, _ = _problems()
    ctx = _context(20, "f32", P, True)
    try:
        ex._upload(ctx, ex._draw_state(2, U, I, 20))
        for side in (USER, ITEM):
            ctx.gamma_sweep(side, *HIER)
            ctx.gamma_exact_sweep(side, *HIER)
            ctx.gamma_elbo_terms(side, with_data=True, hierarchical=True)
        held = ctx.device_bytes()
        for side in (USER, ITEM, USER):
            ctx.gamma_sweep(side, *FLAT)
            ctx.gamma_exact_sweep(side, *HIER)
            ctx.gamma_elbo_terms(side, with_data=True, hierarchical=True)
            ctx.gamma_column_sums(side, from_q=True)
        assert ctx.device_bytes() == held
    finally:
        ctx.close()


# ---- 4. the bound's terms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", CASES)
def test_elbo_terms_against_the_reference_and_against_explicit_zeros(K, dtype):
    from pmf_hip import ITEM, USER
    P, D = _problems()
    eps = EPS[dtype]
    drawn = ex._draw_state(K + 1, U, I, K)
    sparse, dense = _context(K, dtype, P, True), _context(K, dtype, D, False)
    try:
        ex._upload(sparse, drawn)
        ex._upload(dense, drawn)
        st = ex._device_state(sparse)
        L = {n: ref.expectations(st["a_" + n], st["b_" + n])[1] for n in ("theta", "beta")}
        # (the derivation of the x lse bound assumes this, as tests/test_gamma_elbo_gpu.py asserts)
        assert np.abs(L["theta"]).max(axis=1).min() + np.abs(L["beta"]).max(axis=1).min() >= 1.1      # (every cell: D lists them all)
        sums = {}
        for side in (USER, ITEM):
            R_other = (I, U)[side]
            data, logfact, mag, dot, count = zref.data_by_rows(st, side, *P)
            plain, plain_mag = ref.row_terms(st[SIDE_KEYS[side][0]], st[SIDE_KEYS[side][1]])
            bound = eps * (count + K + 16) * mag + (K + R_other * 2.0 ** -53 / eps + 3) * eps * dot
            totals, got = sparse.gamma_elbo_terms(side, with_data=True, hierarchical=False, per_row=True)
            err = np.abs(got[:, ref.DATA] - data)
            print(f"K={K} {dtype} side={side}: DATA {np.max(err / bound):.2g} of the bound")
            assert np.isfinite(got).all() and (err <= bound).all(), (side, np.argwhere(err > bound)[:5], np.max(err / bound))
            assert (np.abs(got[:, ref.LOGFACT] - logfact) <= ex.DOUBLE_TOL * np.abs(logfact)).all()
            empty = count == 0
            assert empty.any() and (got[empty, ref.DATA] < 0).all() and (got[empty, ref.LOGFACT] == 0).all()
            for term in (ref.SUM_FACTOR, ref.SUM_ELOG, ref.ENTROPY):     # the row terms do not read the mode
                assert (np.abs(got[:, term] - plain[:, term]) <= ex.DOUBLE_TOL * plain_mag[:, term]).all()
            seq = np.zeros(ref.TERMS)
            for row in got:
                seq = seq + row
            assert totals.tobytes() == seq.tobytes()
            assert sparse.gamma_elbo_terms(side, with_data=True, hierarchical=False).tobytes() == totals.tobytes()
            none = sparse.gamma_elbo_terms(side, with_data=False, hierarchical=False)
            assert none[ref.DATA] == 0 and none[ref.LOGFACT] == 0
            sums[side] = (totals[ref.DATA] - totals[ref.LOGFACT], bound.sum() + ex.DOUBLE_TOL * np.abs(logfact).sum())
            # MISSING mode on D: the existing call, within the existing bound
            d_terms, d_mags, d_count = ref.side_terms(st, side, *D, hierarchical=False)
            d_totals = dense.gamma_elbo_terms(side, with_data=True, hierarchical=False)
            d_bound = (eps * (d_count + K + 16) * d_mags[:, ref.DATA]).sum() + ex.DOUBLE_TOL * d_mags[:, ref.LOGFACT].sum()
            gap = abs(sums[side][0] - (d_totals[ref.DATA] - d_totals[ref.LOGFACT]))
            print(f"K={K} {dtype} side={side}: zeros on P {sums[side][0]:.12g}, explicit on D gap {gap:.3g} of {sums[side][1] + d_bound:.3g}")
            assert gap <= sums[side][1] + d_bound
        gap = abs(sums[USER][0] - sums[ITEM][0])
        print(f"K={K} {dtype}: data term by users {sums[USER][0]:.12g}, by items {sums[ITEM][0]:.12g}, gap {gap:.3g}")
        assert gap <= sums[USER][1] + sums[ITEM][1]
    finally:
        sparse.close()
        dense.close()


def test_profile_brackets_of_a_zero_mode_elbo_call():
    """Profiling enabled on a fresh context, then zero-mode calls: `prof_get()` succeeds, every bracket has a positive
    time and the counts are the launches' -- row pass (with the column sum), data pass, split rows."""
    from pmf_hip import ITEM, USER
    P, _ = _problems()
    ctx = _context(20, "f32", P, True)
    try:
        ctx.prof_enable(True)
        ex._upload(ctx, ex._draw_state(3, U, I, 20))
        for side in (USER, ITEM):
            for _ in range(2):
                ctx.prof_reset()
                ctx.gamma_elbo_terms(side, with_data=True, hierarchical=True)
                prof = ctx.prof_get()
                assert prof["gamma_final"][1] == 2 and prof["gamma_sweep"][1] == 1, prof      # row pass, split rows; data pass
                assert 0 < prof["gamma_final"][0] < 100 and 0 < prof["gamma_sweep"][0] < 100, prof
            ctx.prof_reset()
            ctx.gamma_elbo_terms(side, with_data=False, hierarchical=True)
            prof = ctx.prof_get()
            assert prof["gamma_final"][1] == 1 and prof["gamma_sweep"][1] == 0 and 0 < prof["gamma_final"][0] < 100, prof
            for sweep in (ctx.gamma_sweep, ctx.gamma_exact_sweep):
                ctx.prof_reset()
                sweep(side, *HIER)
                prof = ctx.prof_get()
                # the column sum, the split rows and (exact) the tables; the sweep itself
                assert prof["gamma_final"][1] == (3 if sweep == ctx.gamma_exact_sweep else 2) and prof["gamma_sweep"][1] == 1, prof
                assert 0 < prof["gamma_final"][0] < 100 and 0 < prof["gamma_sweep"][0] < 100, prof
            ctx.prof_reset()
            ctx.gamma_column_sums(side, from_q=True)
            prof = ctx.prof_get()
            assert prof["gamma_final"][1] == 2 and prof["gamma_sweep"][1] == 0 and 0 < prof["gamma_final"][0] < 100, prof
        for name, (ms, launches) in ctx.prof_get().items():
            assert ms >= 0 and launches >= 0, (name, ms, launches)
    finally:
        ctx.close()


# ---- 5. fold-in ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", CASES)
def test_fold_in_against_the_reference(K, dtype):
    """The shared batch (rows of 0 .. 700 ids) and one of (0, 5, 800) ids -- the block-per-row kernel under the default
    threshold -- hierarchical and not, cold and warm start, 1 and 10 updates, both sides."""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    from test_gamma_fold_in_gpu import _inits, _prior
    rng = np.random.default_rng(K)
    dims = (40, 120)
    with pmf_hip.Context(*dims, K, dtype=dtype) as ctx:
        for side in (USER, ITEM):
            ctx.set_array(side, ARR_FACTOR, rng.gamma(2.0, 0.2, size=(dims[side], K)))
        ctx.set_gamma_zeros(True)
        ctx.prof_enable(True)
        for side in (USER, ITEM):
            E_other = ctx.get_array(1 - side, ARR_FACTOR)
            for lengths in (None, (0, 5, 800)):
                row_ptr, ids, x = batch(7 + side, dims[1 - side]) if lengths is None else batch(9 + side, dims[1 - side], lengths)
                n = len(row_ptr) - 1
                init_f, init_r = _inits(20 + side, n, K, dtype)
                for hierarchical in (True, False):
                    prior = _prior(K, hierarchical)
                    for n_iter, tol in ((1, TOL[dtype][1]), (10, TOL[dtype][20])):
                        for warm in (False, True):
                            start = (init_f, init_r if hierarchical else None) if warm else (None, None)
                            ctx.prof_reset()
                            got = ctx.gamma_fold_in(side, row_ptr, ids, x, *prior, n_iter=n_iter, init_factor=start[0],
                                                    init_prior_rate=start[1])
                            prof = ctx.prof_get()
                            # the column sum (two launches in one bracket), the lane-group kernel, the block kernel for the long row
                            assert (prof["gamma_sweep"][1] == 1) and (prof["gamma_final"][1] == (1 if lengths is None else 2))
                            want = zref.fold_in(E_other, row_ptr, ids, x, *prior, n_iter=n_iter, init_factor=start[0],
                                                init_prior_rate=start[1])
                            errs = [rel_err(g, w) for g, w in zip(got, want) if w is not None]
                            assert all((g is None) == (w is None) for g, w in zip(got, want))
                            assert max(errs) <= tol, (side, lengths, hierarchical, n_iter, warm, errs)
                            empty = np.diff(row_ptr) == 0
                            assert empty.any() and np.isfinite(got[0]).all()
                print(f"K={K} {dtype} side={side} lengths={'shared' if lengths is None else lengths}: last errors",
                      " ".join("%.3g" % e for e in errs))


# ---- 6. the model surface -------------------------------------------------------------------------------------------------
def _frame(ratings):
    return pd.DataFrame({"u": ratings[0], "i": ratings[1], "rating": ratings[2]})


def _model(kind, max_iter=5):
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    if kind == "hpf":
        return HPF_CAVI(HPF_CAVI_Config(n_factors=8, max_iter=max_iter, tol=None, random_state=3, verbose=False), dtype="f64")
    return PoissonMFCAVI(PoissonMFCAVIConfig(n_factors=8, max_iter=max_iter, tol=None, random_state=3, verbose=False), dtype="f64")


ATTRS = {"hpf": ("E_theta", "E_beta", "gamma_a_theta", "gamma_b_theta", "gamma_a_beta", "gamma_b_beta", "gamma_b_xi", "gamma_b_eta"),
         "poisson": ("E_theta", "E_beta", "a_theta", "b_theta", "a_beta", "b_beta")}


@pytest.mark.parametrize("update", ["reference", "exact"])
@pytest.mark.parametrize("kind", ["hpf", "poisson"])
def test_fit_with_zeros_is_the_fit_of_the_dense_frame(kind, update):
    from pmf_hip import USER
    from src.models._device_model import fold_in_batch
    P, D = _problems()
    zero, dense = _model(kind), _model(kind)
    try:
        zero.fit(_frame(P), update=update, unobserved="zero")
        dense.fit(_frame(D), update=update)
        assert zero.history_["unobserved"] == "zero" and dense.history_["unobserved"] == "missing"
        assert zero.history_["iterations"] == dense.history_["iterations"] == 5
        for attr in ATTRS[kind]:
            np.testing.assert_allclose(getattr(zero, attr), getattr(dense, attr), rtol=1e-9, atol=0, err_msg=attr)
        a, b = zero.elbo(), dense.elbo()
        print(f"{kind} {update}: elbo with zeros {a:.12g}, of the dense frame {b:.12g}")
        assert abs(a - b) <= 1e-9 * abs(b)
        # fold-in of the zero-mode model runs in zero mode: the context's own call on the same batch
        new = pd.DataFrame({"u": [7, 7, 7, 3, 9], "i": [0, 5, 69, 2, 500], "rating": [2.0, 0.0, 1.0, 4.0, 1.0]})
        fold = zero.fold_in_users(new, n_iter=4)
        _, row_ptr, other, x = fold_in_batch(new, USER, zero.n_items)
        assert zero._ctx.gamma_zeros is True
        direct = zero._ctx.gamma_fold_in(USER, row_ptr, other, x, *zero._priors()[USER], n_iter=4)
        assert fold.E.tobytes() == direct[0].tobytes() and fold.rate.tobytes() == direct[2].tobytes()
        C_beta = zero._ctx.gamma_column_sums(1, from_q=False)
        assert (fold.rate > C_beta[None, :] * (1 - 1e-12)).all()          # every row's rate sum is the column sum
    finally:
        zero.close()
        dense.close()


@pytest.mark.parametrize("kind", ["hpf", "poisson"])
def test_tracked_bound_of_an_exact_zero_mode_fit_never_falls(kind):
    P, _ = _problems()
    model = _model(kind, max_iter=10)
    try:
        model.fit(_frame(P), update="exact", unobserved="zero", track_elbo=True)
        trace = np.asarray(model.history_["elbo"])
        assert len(trace) == 10 and np.isfinite(trace).all()
        assert (np.diff(trace) >= -1e-9 * np.abs(trace[:-1])).all(), np.diff(trace)
        assert abs(model.elbo() - trace[-1]) <= 1e-12 * abs(trace[-1])
    finally:
        model.close()


@pytest.mark.parametrize("kind", ["hpf", "poisson"])
def test_a_plain_fit_after_a_zero_mode_fit_is_a_plain_fit(kind):
    P, _ = _problems()
    model, fresh = _model(kind), _model(kind)
    try:
        model.fit(_frame(P), unobserved="zero")
        with_zeros = np.array(model.E_theta)
        model.fit(_frame(P))
        fresh.fit(_frame(P))
        assert model.history_["unobserved"] == "missing" and model._ctx.gamma_zeros is False
        for attr in ATTRS[kind]:
            assert np.asarray(getattr(model, attr)).tobytes() == np.asarray(getattr(fresh, attr)).tobytes(), attr
        assert with_zeros.tobytes() != np.asarray(model.E_theta).tobytes()
    finally:
        model.close()
        fresh.close()


# ---- 7. what is refused ---------------------------------------------------------------------------------------------------
def _state_bits(ctx):
    from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER
    return [ctx.get_array(s, a).tobytes() for s in (USER, ITEM) for a in (ARR_FACTOR, ARR_SHAPE, ARR_RATE, ARR_PRIOR_RATE, ARR_HYPER_RATE)]


def _refused(lib, status, *words):
    assert status == PMF_EINVAL
    message = lib.pmf_last_error().decode()
    for word in words:
        assert word in message, message


def test_calls_that_zero_mode_does_not_cover_are_refused_and_write_nothing():
    import torch
    import pmf_hip
    from pmf_hip import ARR_SCALE, ITEM, USER
    lib = pmf_hip.load()
    P, _ = _problems()
    ctx = _context(20, "f32", P, True)
    try:
        ex._upload(ctx, ex._draw_state(1, U, I, 20))
        for side in (USER, ITEM):
            ctx.set_array(side, ARR_SCALE, np.ones(ctx.rows(side)))
        stats = gamma_stats(ctx, torch.device("cuda", 0))
        stats.tensor.fill_(7.0)
        before = _state_bits(ctx)
        h = ctx._h
        _refused(lib, lib.pmf_gamma_accumulate(h, ITEM, C.c_void_p(stats.ptr)), "pmf_gamma_accumulate", "zeros")
        _refused(lib, lib.pmf_gamma_exact_accumulate(h, ITEM, C.c_void_p(stats.ptr)), "pmf_gamma_exact_accumulate", "zeros")
        _refused(lib, lib.pmf_gamma_finalize(h, ITEM, C.c_void_p(stats.ptr), 0.3, 0.7, 0, 0.0, 0.0), "pmf_gamma_finalize", "zeros")
        _refused(lib, lib.pmf_gamma_ext_sweep(h, USER, 0.3, 0.7), "pmf_gamma_ext_sweep", "zeros")
        ctx.sync()
        assert bool((stats.tensor == 7.0).all()) and _state_bits(ctx) == before
        for mode in (2, -1):
            _refused(lib, lib.pmf_ctx_set_gamma_zeros(h, mode), "pmf_ctx_set_gamma_zeros", "bad mode")
        assert ctx.gamma_zeros is True
        _refused(lib, lib.pmf_ctx_get_gamma_zeros(h, None), "pmf_ctx_get_gamma_zeros")
        _refused(lib, lib.pmf_gamma_column_sums(h, USER, 0, None), "pmf_gamma_column_sums", "null out")
        _refused(lib, lib.pmf_gamma_column_sums(h, 2, 0, None), "pmf_gamma_column_sums", "bad side")
        # back in MISSING mode the same calls run
        ctx.set_gamma_zeros(False)
        ctx.gamma_accumulate(ITEM, stats.ptr)
        ctx.gamma_finalize(ITEM, stats.ptr, *FLAT)
        ctx.sync()
    finally:
        ctx.close()
    with pmf_hip.Context(5, 4, 3) as bare:
        out = np.full(3, 7.0)
        _refused(lib, lib.pmf_gamma_column_sums(bare._h, USER, 0, out.ctypes.data_as(C.POINTER(C.c_double))), "pmf_gamma_column_sums", "FACTOR")
        _refused(lib, lib.pmf_gamma_column_sums(bare._h, USER, 1, out.ctypes.data_as(C.POINTER(C.c_double))), "pmf_gamma_column_sums", "SHAPE")
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
            _refused(lib, lib.pmf_ctx_set_gamma_zeros(ctx._h, 1), "pmf_ctx_set_gamma_zeros", "communicator")
            assert ctx.gamma_zeros is False
            ctx.set_gamma_zeros(False)                         # the default stays available
        with pmf_hip.Context(U, I, 8) as ctx:
            ctx.set_gamma_zeros(True)
            with pytest.raises(PmfError, match="pmf_comm_attach.*zeros"):
                comm.attach(ctx)
            with pytest.raises(PmfError, match="pmf_comm_init.*zeros"):
                ctx.comm_init(1, 0, Context.comm_unique_id())
            assert ctx.comm_info() == (1, 0, -1) and ctx.gamma_zeros is True
            ctx.set_gamma_zeros(False)
            comm.attach(ctx)
            assert ctx.comm_info()[2] == pmf_hip.TRANSPORT_RCCL
    finally:
        comm.close()
