"""`pmf_gamma_fold_in_exact` -- the exact coordinate-ascent fold-in of the Poisson MF and HPF models -- against the
recursion of include/pmf_hip.h in float64 NumPy (tests/gamma_fold_in_exact_reference.py) and, at one pass, against
`factor_half_sweep(exact=True)` / `hyper_half_sweep` of tests/gamma_elbo_reference.py, evaluated on the frozen state read
back from the device (so the rounding of the inputs is not part of the error): every output, every row, every element.
The start values are numbers the context's dtype holds exactly.

Bounds.  None is a number found by running the kernel.  eps is the unit roundoff 2^-24 (fp32) or 2^-53 (fp64).

One pass.  The pass's summation tree is `gamma_exact_kernel`'s (the row variant walks a row's ratings one by one, the
block variant adds fewer values per chain), so the bounds are the ones tests/test_gamma_exact_gpu.py derives for that
tree, taken from its `_expected` with (s^0, r^0) as the row's own q and rho^0 as its prior rate:
    shape sum A_rk:  eps (n_r + (K + 16)(1 + M_r)) A_rk + 2^-126 sum_j x_j,     rate sum B_rk:  eps (n_r + 2) B_rk,
SHAPE, RATE, FACTOR, HYPER_RATE, PRIOR_RATE as composed there.  One term is added: the row's own l_k = psi(s_k) - log r_k
is formed in double and rounded once to the context's dtype, |dl_k| <= (eps / 2) |l_k| (the double evaluation's own
error, a few 2^-53 of |psi| + |log r|, is far below it in fp32 and within the (K + 16) eps slack in fp64).  phi_j is a
softmax of l + L_o: d log phi_jk = dl_k - sum_m phi_jm dl_m, so |d phi_jk| <= 2 max_k |dl_k| phi_jk <= eps max_k |l_k| phi_jk
and A_rk moves by at most  eps max_k |l_rk| A_rk.  (The sweep's derivation already counts the table roundings of both
sides inside 2.5 (max + max); the term is stated on its own, as the recursion re-forms l in every pass.)

Several passes, fp64: the project's bounds for the reference fold-in, 1e-11 (3 passes) and 1e-9 (20) relative, and 1e-12 at
one pass as a sanity cap on top of the derived bound.  tests/test_gamma_fold_in_exact_cpu.py shows that two float64
restatements which differ only in the order of the ratings stay within a tenth of them on this batch.

Several passes, fp32: the yardstick is the reference alone.  F = the largest relative distance, per output, between the
float32 restatement and the float64 one on the same batch (computed here); the device may be off by 4 F |value| plus the
one-pass bound of its last pass.  The 4 is not a measurement of this kernel: the reference fold-in's kernel stood at 1.7 x
its float32 twin, and this one adds an exp, a division and l's rounding per pass.  The worst fractions are printed
(DESIGN.md section 4.20)."""
import ctypes as C

import numpy as np
import pytest

import gamma_elbo_reference as ref
from gamma_fold_in_exact_reference import (FLAT_PRIORS, FROZEN, KAPPA_PRIORS, call_prior, exact_batch, fold_in_exact_reference,
                                           frozen_state, row_bound)
from helpers import rel_err

pytestmark = pytest.mark.gpu

PMF_EINVAL, PMF_ERANGE = -1, -4
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP = {"f32": np.float32, "f64": np.float64}
F64_TOL = {1: 1e-12, 3: 1e-11, 20: 1e-9}
NAMES = ("FACTOR", "SHAPE", "RATE", "PRIOR_RATE", "HYPER_RATE")
KEYS = (("a_theta", "b_theta"), ("a_beta", "b_beta"))


def _round(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(NP[dtype]).astype(np.float64)


def _open(K, dtype, st, dims=(FROZEN, FROZEN)):
    """A context that holds q of both sides -- SHAPE and RATE, no FACTOR, no ratings -- and that state as the device holds it"""
    import pmf_hip
    from pmf_hip import ARR_RATE, ARR_SHAPE
    ctx = pmf_hip.Context(*dims, K, dtype=dtype)
    dev = {}
    for side, (ka, kb) in enumerate(KEYS):
        ctx.set_array(side, ARR_SHAPE, st[ka])
        ctx.set_array(side, ARR_RATE, st[kb])
        dev[ka], dev[kb] = ctx.get_array(side, ARR_SHAPE), ctx.get_array(side, ARR_RATE)
    return ctx, dev


def _one_pass(dev, side, batch, prior, dtype, s0, r0, rho0, colsum=None):
    """({output: reference}, {output: allowed |got - ref|}) of one pass of the rows of `batch` from (s0, r0, rho0) against the
    opposite side of `dev`: `_expected` of tests/test_gamma_exact_gpu.py plus the l term of the docstring.  `colsum`: the
    zero mode's B (RATE = rho + C: C is rounded once and added once)."""
    from test_gamma_exact_gpu import _expected
    row_ptr, ids, x = batch
    eps = EPS[dtype]
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    st = {KEYS[side][0]: s0, KEYS[side][1]: r0, KEYS[1 - side][0]: dev[KEYS[1 - side][0]], KEYS[1 - side][1]: dev[KEYS[1 - side][1]]}
    ratings = (rows, np.asarray(ids, dtype=np.int64), x) if side == 0 else (np.asarray(ids, dtype=np.int64), rows, x)
    want, bound, _ = _expected(st, side, ratings, prior, rho0, dtype)
    shape_prior = float(NP[dtype](prior[0]))
    l_max = np.abs(ref.expectations(s0, r0)[1]).max(axis=1)
    bound["SHAPE"] = bound["SHAPE"] + eps * l_max[:, None] * (want["SHAPE"] - shape_prior)
    if colsum is not None:
        want["RATE"] = rho0[:, None] + colsum[None, :]
        bound["RATE"] = 2.0 * eps * want["RATE"]
        want["FACTOR"] = want["SHAPE"] / want["RATE"]
    bound["FACTOR"] = want["FACTOR"] * (bound["SHAPE"] / want["SHAPE"] + bound["RATE"] / want["RATE"] + eps)
    if prior[2]:
        if colsum is not None:
            want["HYPER_RATE"] = float(NP[dtype](prior[4])) + want["FACTOR"].sum(axis=1)
            want["PRIOR_RATE"] = float(NP[dtype](prior[3])) / want["HYPER_RATE"]
        bound["HYPER_RATE"] = bound["FACTOR"].sum(axis=1) + 5.0 * eps * want["HYPER_RATE"]
        bound["PRIOR_RATE"] = want["PRIOR_RATE"] * (bound["HYPER_RATE"] / want["HYPER_RATE"] + eps)
    return want, bound


def _start(prior, dtype, n_rows, K, warm=None):
    """(s0, r0, rho0) as float64 arrays of numbers the dtype holds: the cold start of the header, or `warm` = (a, b, h)"""
    T = NP[dtype]
    if warm is not None:
        a, b, h = warm
        rho = _round(prior[3] / h, dtype) if prior[2] else np.full(n_rows, float(T(prior[1])))
        return _round(a, dtype), _round(b, dtype), rho
    rho = float(T(prior[3]) / T(prior[4])) if prior[2] else float(T(prior[1]))
    return np.full((n_rows, K), float(T(prior[0]))), np.full((n_rows, K), rho), np.full(n_rows, rho)


def _as_dict(got, hierarchical):
    return {n: g for n, g in zip(NAMES, got) if hierarchical or n not in ("PRIOR_RATE", "HYPER_RATE")}


def _check_one_pass(got, want, bound, what):
    worst = {}
    for name, g in got.items():
        err = np.abs(g - want[name])
        assert np.isfinite(g).all(), (what, name)
        worst[name] = float(np.max(err / bound[name]))
        assert (err <= bound[name]).all(), (what, name, np.argwhere(err > bound[name])[:5], worst[name])
    print(what, " ".join("%s %.2g" % kv for kv in worst.items()), "(fractions of the one-pass bound)")
    return max(worst.values())


def _call(ctx, side, batch, prior, n_iter, start, warm):
    kw = dict(init_shape=start[0], init_rate=start[1], init_prior_rate=start[2] if prior[2] else None) if warm else {}
    return ctx.gamma_fold_in_exact(side, *batch, *prior, n_iter=n_iter, **kw)


# ---- 1. every shape, both states, 1 / 3 / 20 passes --------------------------------------------------------------------
CASES = [(K, "f32") for K in (1, 3, 20, 64, 100, 136, 256)] + [(K, "f64") for K in (5, 64, 129)]
# (state, side, hierarchical, warm): both states, both sides, both models, both starts
CONFIGS = ((False, 0, True, False), (False, 1, False, True), (True, 1, True, True), (True, 0, False, False))


@pytest.mark.parametrize("K,dtype", CASES)
def test_parity_with_the_recursion(K, dtype):
    """Rows of 0 .. 700 ratings with the lane-group kernel, 769 and 1500 with the block kernel (default threshold), every
    LPR and a K with pads; the second state has a frozen row and a start row whose E log is -107.5 in every element."""
    from pmf_hip import ARR_RATE, ARR_SHAPE  # noqa: F401
    batch = exact_batch(7)
    row_ptr, ids, x = batch
    n_rows = len(row_ptr) - 1
    assert np.diff(row_ptr).max() == 1500 and (np.diff(row_ptr) > 768).sum() == 2 and (np.diff(row_ptr) == 0).any()
    worst_one, worst_many = 0.0, 0.0
    for small in (False, True):
        st = frozen_state(K, small, row_ptr, ids)
        if small and dtype == "f32":     # a product of exp(E log) tables is 0 on the tiny rows
            el = np.exp(ref.expectations(st["init_a"], st["init_b"])[1]).astype(np.float32)
            tiny = int(np.argmax(np.bincount(ids, minlength=FROZEN)))
            assert (el[n_rows - 1] * np.exp(ref.expectations(st["a_beta"][tiny], st["b_beta"][tiny])[1]).astype(np.float32) == 0).all()
        ctx, dev = _open(K, dtype, st)
        try:
            for use_small, side, hierarchical, warm in CONFIGS:
                if use_small != small:
                    continue
                prior = call_prior(K, hierarchical)
                what = f"K={K} {dtype} state={'ab'[small]} side={side} hier={hierarchical} warm={warm}"
                s0, r0, rho0 = _start(prior, dtype, n_rows, K, (st["init_a"], st["init_b"], st["init_h"]) if warm else None)
                oa, ob = dev[KEYS[1 - side][0]], dev[KEYS[1 - side][1]]
                kw = dict(init_shape=s0, init_rate=r0, init_prior_rate=rho0 if hierarchical else None) if warm else {}
                prior_t = tuple(float(NP[dtype](p)) if k != 2 else p for k, p in enumerate(prior))   # the priors as the context holds them
                trace64, trace32 = [], []
                fold_in_exact_reference(oa, ob, row_ptr, ids, x, *prior_t, n_iter=20, trace=trace64, **kw)
                if dtype == "f32":
                    fold_in_exact_reference(oa, ob, row_ptr, ids, x, *prior_t, n_iter=20, trace=trace32, dtype=np.float32, **kw)

                def outputs(trace, n):
                    s, r, h = (np.asarray(a, dtype=np.float64) for a in trace[n - 1])
                    out = {"FACTOR": s / r, "SHAPE": s, "RATE": r}
                    if hierarchical:
                        out["HYPER_RATE"], out["PRIOR_RATE"] = h, prior_t[3] / h
                    return out
                for n_iter in (1, 3, 20):
                    got = _as_dict(_call(ctx, side, batch, prior, n_iter, (s0, r0, rho0), warm), hierarchical)
                    want64 = outputs(trace64, n_iter)
                    # the one-pass bound of the LAST pass, from the reference's state before it
                    if n_iter == 1:
                        before = (s0, r0, rho0)
                    else:
                        s, r, h = trace64[n_iter - 2]
                        before = (s, r, prior_t[3] / h if hierarchical else rho0)
                    want1, bound1 = _one_pass(dev, side, batch, prior, dtype, *before)
                    if n_iter == 1:
                        worst_one = max(worst_one, _check_one_pass(got, want1, bound1, what + " n_iter=1"))
                    if dtype == "f64":
                        errs = {n: rel_err(g, want64[n]) for n, g in got.items()}
                        print(what, f"n_iter={n_iter}", " ".join("%s %.2g" % kv for kv in errs.items()), f"(bound {F64_TOL[n_iter]})")
                        assert max(errs.values()) <= F64_TOL[n_iter], (what, n_iter, errs)
                    elif n_iter > 1:
                        want32 = outputs(trace32, n_iter)
                        for name, g in got.items():
                            F = rel_err(want32[name], want64[name])
                            allowed = 4.0 * F * np.abs(want64[name]) + bound1[name]
                            err = np.abs(g - want64[name])
                            frac = float(np.max(err / allowed))
                            worst_many = max(worst_many, frac)
                            print(what, f"n_iter={n_iter} {name}: F {F:.2g}, worst fraction of 4 F + one pass {frac:.2g}")
                            assert np.isfinite(g).all() and (err <= allowed).all(), (what, n_iter, name, frac)
        finally:
            ctx.close()
    print(f"K={K} {dtype}: worst fraction of the one-pass bound {worst_one:.3g}, of the several-pass allowance {worst_many:.3g}")


# ---- 2. against the sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hierarchical", [True, False])
@pytest.mark.parametrize("K,dtype", [(20, "f32"), (64, "f64")])
def test_one_warm_pass_on_the_training_rows_is_the_exact_sweep(K, dtype, hierarchical, monkeypatch):
    """Every row's own training ratings, warm start from the context's own SHAPE / RATE / PRIOR_RATE, one pass, against
    one `pmf_gamma_exact_sweep` on a copy of the context: within the sum of the two one-pass bounds under the default task
    length (rows cut into several tasks), bit for bit when every row is one task.  Both sides."""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE
    from test_gamma_exact_gpu import FLAT, HIER, I, U, _draw_state, _problem, _upload
    u, i, x = _problem()
    prior = HIER if hierarchical else FLAT
    drawn = _draw_state(K, U, I, K, True, u, i)
    arrays = (ARR_FACTOR, ARR_SHAPE, ARR_RATE) + ((ARR_PRIOR_RATE, ARR_HYPER_RATE) if hierarchical else ())
    for chunk in (None, "512"):
        if chunk is None:
            monkeypatch.delenv("PMF_TASK_CHUNK", raising=False)
        else:
            monkeypatch.setenv("PMF_TASK_CHUNK", chunk)
        for side in (0, 1):
            rows, others = (u, i) if side == 0 else (i, u)
            R = (U, I)[side]
            order = np.argsort(rows, kind="stable")
            row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=R))])
            batch = (row_ptr, others[order].astype(np.int32), x[order])
            with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
                ctx.set_ratings(u, i, x)
                _upload(ctx, drawn)
                one_task = ctx.task_max_len(side, "gamma") >= int(np.diff(row_ptr).max())
                assert one_task == (chunk == "512")
                dev = {KEYS[s][0]: ctx.get_array(s, ARR_SHAPE) for s in (0, 1)}
                dev.update({KEYS[s][1]: ctx.get_array(s, ARR_RATE) for s in (0, 1)})
                s0, r0 = dev[KEYS[side][0]], dev[KEYS[side][1]]
                rho0 = ctx.get_array(side, ARR_PRIOR_RATE) if hierarchical else np.full(R, float(NP[dtype](prior[1])))
                got = ctx.gamma_fold_in_exact(side, *batch, *prior, n_iter=1, init_shape=s0, init_rate=r0,
                                              init_prior_rate=rho0 if hierarchical else None)
                ctx.gamma_exact_sweep(side, *prior)          # (the fold-in read the context only: the sweep starts from the same state)
                swept = [ctx.get_array(side, a) for a in arrays]
            _, bound = _one_pass(dev, side, batch, prior, dtype, s0, r0, rho0)
            for name, g, w in zip(NAMES, got, swept):
                if one_task:
                    assert np.array_equal(g, w), (chunk, side, name)
                else:
                    assert (np.abs(g - w) <= 2.0 * bound[name]).all(), (chunk, side, name, float(np.max(np.abs(g - w) / bound[name])))


# ---- 3. the bound of a folded row does not fall -------------------------------------------------------------------------
@pytest.mark.parametrize("hierarchical", [True, False])
def test_row_bound_is_monotone_on_the_device(hierarchical):
    """fp64, K = 64, cold start: the row bound (NumPy, from the outputs of calls with n_iter = 1 .. 10) never falls by
    more than 2 x the evaluation slack, on any row."""
    K = 64
    batch = exact_batch(7)
    st = frozen_state(K, True, *batch[:2])
    prior = KAPPA_PRIORS if hierarchical else FLAT_PRIORS
    ctx, dev = _open(K, "f64", st)
    try:
        previous, tightest = None, np.inf
        for n_iter in range(1, 11):
            got = ctx.gamma_fold_in_exact(0, *batch, *call_prior(K, hierarchical), n_iter=n_iter)
            value, allowed = row_bound(dev["a_beta"], dev["b_beta"], *batch, got[1], got[2], got[4], prior, hierarchical)
            if previous is not None:
                tightest = min(tightest, float(np.min((value - previous) / (2.0 * allowed))))
                assert (value >= previous - 2.0 * allowed).all(), (n_iter, np.flatnonzero(value < previous - 2.0 * allowed))
            previous = value
        print(f"hierarchical={hierarchical}: smallest rise {tightest:.3g} slacks")
    finally:
        ctx.close()


# ---- 4. unlisted cells as zeros ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", [(20, "f32"), (20, "f64")])
def test_zero_mode(K, dtype):
    """After set_gamma_zeros(True), B of every row is C of the opposite side (`gamma_column_sums(other, from_q=True)`): the
    call equals the reference with that B (one pass within the derived bounds; in fp64 three passes too; rows through both
    kernels).  On the small problem P it also
    equals, within the sum of the one-pass bounds, the default mode's exact fold-in of the dense completion D, where every
    unlisted cell is an explicit 0."""
    from gamma_implicit_reference import dense_completion, problem_p
    from test_gamma_exact_gpu import _draw_state
    batch = exact_batch(9)
    row_ptr, ids, x = batch
    st = frozen_state(K, True, row_ptr, ids)
    hier, flat = call_prior(K, True), call_prior(K, False)
    ctx, dev = _open(K, dtype, st)
    try:
        ctx.set_gamma_zeros(True)
        for side, prior in ((0, hier), (1, flat)):
            C_o = ctx.gamma_column_sums(1 - side, from_q=True)
            C_t = _round(C_o, dtype)                 # rounded once to the context's dtype before it is added
            s0, r0, rho0 = _start(prior, dtype, len(row_ptr) - 1, K)
            got = _as_dict(ctx.gamma_fold_in_exact(side, *batch, *prior, n_iter=1), prior[2])
            want, bound = _one_pass(dev, side, batch, prior, dtype, s0, r0, rho0, colsum=C_t)
            _check_one_pass(got, want, bound, f"zero mode K={K} {dtype} side={side}")
            if dtype == "f64":                       # three passes: the recursion with B = C, the fp64 bound of case 1
                got = ctx.gamma_fold_in_exact(side, *batch, *prior, n_iter=3)
                want3 = fold_in_exact_reference(dev[KEYS[1 - side][0]], dev[KEYS[1 - side][1]], row_ptr, ids, x, *prior, n_iter=3, colsum=C_t)
                errs = [rel_err(g, w) for g, w in zip(got, want3) if w is not None]
                assert max(errs) <= F64_TOL[3], (side, errs)
    finally:
        ctx.close()
    # P against D
    U, I = 90, 70
    u, i, xp = problem_p()
    du, di, dx = dense_completion(u, i, xp, U, I)
    drawn = _draw_state(K, U, I, K, False)

    def user_batch(uu, ii, xx):
        order = np.argsort(uu, kind="stable")
        return np.concatenate([[0], np.cumsum(np.bincount(uu, minlength=U))]), ii[order].astype(np.int32), xx[order]
    bp, bd = user_batch(u, i, xp), user_batch(du, di, dx)
    ctx, dev = _open(K, dtype, drawn, dims=(U, I))
    try:
        s0, r0, rho0 = _start(hier, dtype, U, K)
        dense = ctx.gamma_fold_in_exact(0, *bd, *hier, n_iter=1)
        _, bound_d = _one_pass(dev, 0, bd, hier, dtype, s0, r0, rho0)
        ctx.set_gamma_zeros(True)
        sparse = ctx.gamma_fold_in_exact(0, *bp, *hier, n_iter=1)
        _, bound_p = _one_pass(dev, 0, bp, hier, dtype, s0, r0, rho0, colsum=_round(ctx.gamma_column_sums(1, from_q=True), dtype))
        for name, g, w in zip(NAMES, sparse, dense):
            allowed = bound_p[name] + bound_d[name]
            assert (np.abs(g - w) <= allowed).all(), (name, float(np.max(np.abs(g - w) / allowed)))
    finally:
        ctx.close()


# ---- 5. determinism, row blocks, the two kernels ------------------------------------------------------------------------------
def _launches(ctx):
    prof = ctx.prof_get()
    return {k: prof[k][1] for k in ("gamma_sweep", "gamma_final")}


def test_same_bits_whatever_the_row_blocks_and_both_kernels(monkeypatch):
    """Two calls give the same bits; PMF_FOLD_IN_ROWS = 1 and 7 give the bits of one block; PMF_GAMMA_FOLD_LONG=64 (the
    rows of 65 .. 768 ratings through the block variant: another order of the same sums) agrees with the default within
    the one-pass bound.  The context is only read, and its device bytes grow on the first call only."""
    K, dtype = 20, "f32"
    batch = exact_batch(11)
    row_ptr = batch[0]
    st = frozen_state(K, True, *batch[:2])
    prior = call_prior(K, True)
    results, single = {}, {}
    for rows_env, long_env in ((None, None), ("1", None), ("7", None), (None, "64")):
        for name, value in (("PMF_FOLD_IN_ROWS", rows_env), ("PMF_GAMMA_FOLD_LONG", long_env)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, value)
        ctx, dev = _open(K, dtype, st)
        try:
            ctx.prof_enable(True)
            held = None
            outs = []
            for _ in range(2):
                outs.append(ctx.gamma_fold_in_exact(0, *batch, *prior, n_iter=3))
                held = held or ctx.device_bytes()
                assert ctx.device_bytes() == held               # grows on the first call only
            assert all(np.array_equal(a, b) for a, b in zip(*outs))
            assert (np.diff(row_ptr) > 768).sum() == 2 and _launches(ctx)["gamma_sweep"] > 0 and _launches(ctx)["gamma_final"] > 0
            single[(rows_env, long_env)] = ctx.gamma_fold_in_exact(0, *batch, *prior, n_iter=1)
            for side in (0, 1):                 # the context was only read
                from pmf_hip import ARR_RATE, ARR_SHAPE
                assert np.array_equal(ctx.get_array(side, ARR_SHAPE), dev[KEYS[side][0]])
                assert np.array_equal(ctx.get_array(side, ARR_RATE), dev[KEYS[side][1]])
            results[(rows_env, long_env)] = outs[0]
        finally:
            ctx.close()
    base = results[(None, None)]
    for key in (("1", None), ("7", None)):
        assert all(np.array_equal(a, b) for a, b in zip(base, results[key])), key
    s0, r0, rho0 = _start(prior, dtype, len(row_ptr) - 1, K)
    _, bound = _one_pass(dev, 0, batch, prior, dtype, s0, r0, rho0)
    for name, a, b in zip(NAMES, single[(None, None)], single[(None, "64")]):
        print(f"PMF_GAMMA_FOLD_LONG=64 against the default, {name}: {float(np.max(np.abs(a - b) / bound[name])):.2g} of the one-pass bound")
        assert (np.abs(a - b) <= bound[name]).all(), name


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ARR_RATE, ARR_SCALE, ARR_SHAPE
    lib = pmf_hip.load()
    K, dtype = 8, "f32"
    batch = exact_batch(7)
    st = frozen_state(K, False, *batch[:2])
    row_ptr = np.array([0, 3, 3, 7], dtype=np.int64)
    ids, x = batch[1][:7].copy(), batch[2][:7].copy()
    n = 3
    outs = [np.full((n, K), 7.0) for _ in range(3)] + [np.full(n, 7.0) for _ in range(2)]
    init_s, init_b = _round(st["init_a"][:n], dtype), _round(st["init_b"][:n], dtype)
    init_r = _round(st["init_h"][:n], dtype)
    hier = call_prior(K, True)

    def call(h, side=0, rp=row_ptr, o=ids, xs=x, prior=hier, n_iter=2, s0=init_s, b0=init_b, r0=init_r, out=outs, n_rows=None):
        def p(a, t=C.c_double):
            return None if a is None else a.ctypes.data_as(C.POINTER(t))
        return lib.pmf_gamma_fold_in_exact(h, side, n if n_rows is None else n_rows, p(rp, C.c_int64), p(o, C.c_int32), p(xs),
                                           prior[0], prior[1], int(prior[2]), prior[3], prior[4], n_iter, p(s0), p(b0), p(r0),
                                           *[p(a) for a in out])

    def refused(code, fragment, **kw):
        h = kw.pop("h", ctx._h)
        assert call(h, **kw) == code, (kw, lib.pmf_last_error())
        msg = lib.pmf_last_error().decode()
        assert msg.startswith("pmf_gamma_fold_in_exact:") and fragment in msg, msg
        assert all((a == 7.0).all() for a in outs), kw

    ctx, dev = _open(K, dtype, st)
    try:
        refused(PMF_EINVAL, "null context", h=None)
        refused(PMF_EINVAL, "null context", h=None, n_rows=0)
        refused(PMF_EINVAL, "bad side", side=2)
        refused(PMF_EINVAL, "negative", n_rows=-1)
        for name in ("rp", "o", "xs"):
            refused(PMF_EINVAL, "null argument", **{name: None})
        refused(PMF_EINVAL, "null argument", out=[None] + outs[1:])
        refused(PMF_EINVAL, "row_ptr[0]", rp=row_ptr + 1)
        refused(PMF_EINVAL, "decreases", rp=np.array([0, 5, 3, 7], dtype=np.int64))
        for bad in (0.0, -1.0):
            refused(PMF_EINVAL, "shape_prior", prior=(bad,) + hier[1:])
            refused(PMF_EINVAL, "rate_prior", prior=(0.3, bad, False, 0.0, 0.0))
            refused(PMF_EINVAL, "hyper_shape", prior=(0.3, 1.0, True, bad, 1.5))
            refused(PMF_EINVAL, "hyper_rate_prior", prior=(0.3, 1.0, True, hier[3], bad))
        refused(PMF_EINVAL, "n_iter", n_iter=0)
        refused(PMF_EINVAL, "init_shape and init_rate", b0=None)
        refused(PMF_EINVAL, "init_shape and init_rate", s0=None)
        bad = ids.copy()
        bad[-1] = FROZEN
        refused(PMF_ERANGE, f"id {FROZEN} at position {len(ids) - 1}", o=bad)
        bad[-1] = -1
        refused(PMF_ERANGE, "id -1", o=bad)
        # n_rows = 0 with a valid context: success, nothing touched
        assert call(ctx._h, n_rows=0) == 0
        assert call(ctx._h, n_rows=0, rp=None, o=None, xs=None, s0=None, b0=None, r0=None, out=[None] * 5) == 0
        assert all((a == 7.0).all() for a in outs)
        # the optional outputs; FACTOR of neither side exists, and none is needed
        with pytest.raises(pmf_hip.PmfError, match="FACTOR"):
            ctx.get_array(1, ARR_FACTOR)
        assert call(ctx._h, out=[outs[0], None, None, None, None]) == 0
        assert all((a == 7.0).all() for a in outs[1:]) and not (outs[0] == 7.0).any()
        want = ctx.gamma_fold_in_exact(0, row_ptr, ids, x, *hier, n_iter=2, init_shape=init_s, init_rate=init_b, init_prior_rate=init_r)
        assert np.array_equal(outs[0], want[0])
        outs[0][:] = 7.0
        # a context of the extended model
        ctx.set_array(0, ARR_SCALE, np.ones(FROZEN))
        refused(PMF_EINVAL, "SCALE")
    finally:
        ctx.close()
    # SHAPE and RATE of the opposite side are needed (and named); FACTOR is not enough
    with pmf_hip.Context(FROZEN, FROZEN, K, dtype=dtype) as ctx:
        ctx.set_array(1, ARR_FACTOR, st["a_beta"] / st["b_beta"])
        refused(PMF_EINVAL, "array SHAPE of side 1")
        ctx.set_array(1, ARR_SHAPE, st["a_beta"])
        refused(PMF_EINVAL, "array RATE of side 1")
        refused(PMF_EINVAL, "array SHAPE of side 0", side=1)
        ctx.set_array(1, ARR_RATE, st["b_beta"])
        assert call(ctx._h) == 0


# ---- 7. the model classes ----------------------------------------------------------------------------------------------------
def _fit(kind, K=12):
    import pandas as pd
    from helpers import skewed_problem
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    u, i, x = skewed_problem(100 + K, 300, 80, 5000)
    df = pd.DataFrame({"u": u, "i": i, "rating": x})
    if kind == "hpf":
        cfg = HPF_CAVI_Config(n_factors=K, a=0.3, a_prime=0.5, b_prime=1.5, c=0.4, c_prime=0.6, d_prime=2.0, max_iter=3, tol=None,
                              random_state=3, verbose=False)
        return HPF_CAVI(cfg, dtype="f64").fit(df, update="exact")
    cfg = PoissonMFCAVIConfig(n_factors=K, a0=0.3, b0=1.5, max_iter=3, tol=None, random_state=3, verbose=False)
    return PoissonMFCAVI(cfg, dtype="f64").fit(df, update="exact")


@pytest.mark.parametrize("kind", ["hpf", "poisson"])
def test_model_surface(kind):
    """A model fitted with update="exact": `fold_in_users(df, update="exact")` / `fold_in_items` equal the reference
    recursion on the model's own shapes and rates (fp64: 1e-11 at 3 passes); the default is `update="reference"`, which
    gives the bits of `ctx.gamma_fold_in` called directly."""
    import pandas as pd
    rng = np.random.default_rng(2)
    m = _fit(kind)
    try:
        cfg, K = m.config, m.config.n_factors
        if kind == "hpf":
            priors = ((cfg.a, 0.0, True, cfg.a_prime + K * cfg.a, cfg.b_prime), (cfg.c, 0.0, True, cfg.c_prime + K * cfg.c, cfg.d_prime))
            q = {0: (m.gamma_a_theta, m.gamma_b_theta), 1: (m.gamma_a_beta, m.gamma_b_beta)}
        else:
            priors = ((cfg.a0, cfg.b0, False, 0.0, 0.0),) * 2
            q = {0: (m.a_theta, m.b_theta), 1: (m.a_beta, m.b_beta)}
        n = 90
        labels = rng.choice(np.array(["zed", "amy", "bob"]), n)
        items = rng.integers(0, m.n_items, n)
        ratings = rng.integers(0, 6, n).astype(float)
        df = pd.DataFrame({"u": labels, "i": items, "rating": ratings})
        fold = m.fold_in_users(df, n_iter=3, update="exact")
        assert list(fold.ids) == ["amy", "bob", "zed"] and fold.update == "exact"
        rows = [np.flatnonzero(labels == name) for name in fold.ids]
        row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        pos = np.concatenate(rows)
        want = fold_in_exact_reference(*q[1], row_ptr, items[pos], ratings[pos], *priors[0], n_iter=3)
        errs = [rel_err(g, w) for g, w in zip((fold.E, fold.shape, fold.rate, fold.prior_rate), want[:4]) if w is not None]
        print(kind, "fold_in_users(update='exact'):", errs)
        assert max(errs) <= F64_TOL[3] and (fold.prior_rate is None) == (kind == "poisson")
        users = rng.integers(0, m.n_users, 40)
        new_items = rng.choice(np.array([10**6, 777777]), 40)
        fi = m.fold_in_items(pd.DataFrame({"u": users, "i": new_items, "rating": ratings[:40]}), n_iter=3, update="exact")
        rows = [np.flatnonzero(new_items == name) for name in fi.ids]
        row_ptr_i = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        pos_i = np.concatenate(rows)
        want = fold_in_exact_reference(*q[0], row_ptr_i, users[pos_i], ratings[:40][pos_i], *priors[1], n_iter=3)
        errs = [rel_err(g, w) for g, w in zip((fi.E, fi.shape, fi.rate, fi.prior_rate), want[:4]) if w is not None]
        assert max(errs) <= F64_TOL[3] and fi.update == "exact", errs
        # the default is the reference's update, bit for bit what the direct call gives
        plain, named = m.fold_in_users(df, n_iter=3), m.fold_in_users(df, n_iter=3, update="reference")
        direct = m._need_ctx().gamma_fold_in(0, row_ptr, items[pos], ratings[pos], *priors[0], n_iter=3)
        for a, b, c in zip((plain.E, plain.shape, plain.rate), (named.E, named.shape, named.rate), direct[:3]):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        assert plain.update == named.update == "reference"
        assert not np.array_equal(plain.shape, fold.shape)
    finally:
        m.close()
