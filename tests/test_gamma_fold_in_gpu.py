"""Fold-in of new rows against a fitted Poisson MF / HPF model (`pmf_gamma_fold_in`) against the literal recursion in
float64 NumPy (tests/gamma_fold_in_reference.py), evaluated on the state read back from the device (so the rounding of
the inputs is not part of the error).

Bounds are the project's own for these kernels, elementwise `helpers.rel_err` on every output:
tests/test_gamma_gpu.py:TOL by the number of updates (f64 1e-12 / 1e-11 / 1e-9, f32 2e-5 / 5e-5 / 5e-4 at 1 / 3 / 20), and
f64 1e-11, f32 3e-5 where the fold-in is compared with the sweep kernel itself (test_half_sweeps_vs_oracle_skewed).
tests/test_gamma_fold_in_cpu.py shows float32 NumPy within a quarter of them on the same batch."""
import ctypes as C

import numpy as np
import pytest

from gamma_fold_in_reference import LENGTHS, TOL, batch, fold_in_reference
from helpers import rel_err, skewed_problem
from oracle import cavi_oracle as orc

pytestmark = pytest.mark.gpu

A, A_PRIME, B_PRIME = 0.3, 5.0, 5.0               # user and item priors alike, as tests/test_gamma_gpu.py
B0 = 1.5                                          # rate prior of the non-hierarchical calls
PMF_EINVAL, PMF_ERANGE = -1, -4
NAMES = ("factor", "shape", "rate", "prior_rate", "hyper_rate")


def _sizes(K):
    return (600, 120, 12000) if K <= 64 else (800, 50, 7000)


def _prior(K, hierarchical):
    """(shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior), the same for both sides"""
    return (A, 0.0, True, A_PRIME + K * A, B_PRIME) if hierarchical else (A, B0, False, 0.0, 0.0)


_STATE = {}


def _fitted_state(K, dtype):
    """Ratings and every state array after two real device HPF iterations, read back with get_array: computed once
    per (K, dtype) and never changed."""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER
    key = (K, dtype)
    if key in _STATE:
        return _STATE[key]
    U, I, N = _sizes(K)
    u, i, x = skewed_problem(100 + K, U, I, N)
    st = orc.init_hpf(U, I, K, A, A_PRIME, B_PRIME, A, A_PRIME, B_PRIME, seed=3)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_ratings(u, i, x)
        ctx.set_array(USER, ARR_FACTOR, st["E_theta"]); ctx.set_array(ITEM, ARR_FACTOR, st["E_beta"])
        ctx.set_array(USER, ARR_PRIOR_RATE, st["E_xi"]); ctx.set_array(ITEM, ARR_PRIOR_RATE, st["E_eta"])
        for _ in range(2):
            ctx.gamma_sweep(USER, *_prior(K, True))
            ctx.gamma_sweep(ITEM, *_prior(K, True))
        arrays = {(s, a): ctx.get_array(s, a) for s in (USER, ITEM)
                  for a in (ARR_FACTOR, ARR_SHAPE, ARR_RATE, ARR_PRIOR_RATE, ARR_HYPER_RATE)}
    for a in arrays.values():
        a.setflags(write=False)
    _STATE[key] = {"dims": (U, I), "ratings": (u, i, x), "arrays": arrays}
    return _STATE[key]


def _open(state, K, dtype):
    """A fresh context holding `state` (float64 -> device dtype is exact: the arrays came from that dtype)."""
    import pmf_hip
    ctx = pmf_hip.Context(*state["dims"], K, dtype=dtype)
    ctx.set_ratings(*state["ratings"])
    for (side, array), host in state["arrays"].items():
        ctx.set_array(side, array, host)
    return ctx


def _inits(seed, n_rows, K, dtype):
    """Warm-start values that the context's dtype holds exactly."""
    rng = np.random.default_rng(seed)
    np_dtype = np.float64 if dtype == "f64" else np.float32
    return (rng.gamma(1.0, 0.3, size=(n_rows, K)).astype(np_dtype).astype(np.float64),
            rng.gamma(2.0, 0.5, size=n_rows).astype(np_dtype).astype(np.float64))


def _reference(state, side, row_ptr, ids, x, prior, n_iter, init_factor=None, init_prior_rate=None):
    from pmf_hip import ARR_FACTOR
    return fold_in_reference(state["arrays"][(1 - side, ARR_FACTOR)], row_ptr, ids, x, *prior, n_iter=n_iter,
                             init_factor=init_factor, init_prior_rate=init_prior_rate)


def _check(got, want, tol, what):
    errs = [rel_err(g, w) for g, w in zip(got, want) if w is not None]
    print(what, " ".join("%s %.3g" % (n, e) for n, e in zip(NAMES, errs)), "(bound %.1g)" % tol)
    assert all((g is None) == (w is None) for g, w in zip(got, want)), what
    assert max(errs) <= tol, (what, errs)


CASES = [(K, "f32") for K in (1, 3, 8, 20, 28, 64, 100, 128, 256)] + [(K, "f64") for K in (3, 20, 64, 256)]


def _raw_call(lib, h, side, row_ptr, ids, x, prior, n_iter, init_f, init_r, outs):
    def p(a, t=C.c_double):
        return None if a is None else a.ctypes.data_as(C.POINTER(t))
    return lib.pmf_gamma_fold_in(h, side, len(row_ptr) - 1 if row_ptr is not None else 0, p(row_ptr, C.c_int64), p(ids, C.c_int32),
                                 p(x), prior[0], prior[1], int(prior[2]), prior[3], prior[4], n_iter, p(init_f), p(init_r),
                                 *[p(o) for o in outs])


@pytest.mark.parametrize("K,dtype", CASES)
def test_parity_with_the_literal_recursion(K, dtype):
    """Hierarchical and not, both sides, 1 / 3 / 20 updates, cold and warm start, rows of 0 .. 700 ratings (every LPR
    batch edge up to 64 lanes, the four-in-flight edge, many passes), ratings 0 .. 5: all five outputs.  Not
    hierarchical: the two per-row scalars keep their sentinel."""
    import pmf_hip
    from pmf_hip import ITEM, USER
    lib = pmf_hip.load()
    state = _fitted_state(K, dtype)
    n = len(LENGTHS)
    with _open(state, K, dtype) as ctx:
        for side in (USER, ITEM):
            row_ptr, ids, x = batch(7 + side, state["dims"][1 - side])
            init_f, init_r = _inits(20 + side, n, K, dtype)
            for hierarchical in (True, False):
                prior = _prior(K, hierarchical)
                for n_iter in (1, 3, 20):
                    for warm in (False, True):
                        start = (init_f, init_r if hierarchical else None) if warm else (None, None)
                        got = ctx.gamma_fold_in(side, row_ptr, ids, x, *prior, n_iter=n_iter, init_factor=start[0],
                                                init_prior_rate=start[1])
                        want = _reference(state, side, row_ptr, ids, x, prior, n_iter, *start)
                        _check(got, want, TOL[dtype][n_iter],
                               f"K={K} {dtype} side={side} hier={hierarchical} n_iter={n_iter} warm={warm}")
            # not hierarchical, through the raw call: out_prior_rate / out_hyper_rate are not written
            outs = [np.full((n, K), 7.0) for _ in range(3)] + [np.full(n, 7.0) for _ in range(2)]
            assert _raw_call(lib, ctx._h, side, row_ptr, ids, x, _prior(K, False), 3, None, init_r, outs) == 0
            assert (outs[3] == 7.0).all() and (outs[4] == 7.0).all()
            _check(outs[:3], _reference(state, side, row_ptr, ids, x, _prior(K, False), 3)[:3], TOL[dtype][3], "raw call")


def _launches(ctx):
    prof = ctx.prof_get()
    return {k: prof[k][1] for k in ("gamma_sweep", "gamma_final")}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K", [8, 64, 256])
def test_both_variants(K, dtype, monkeypatch):
    """The default threshold keeps rows of up to 700 ratings with the lane-group kernel; PMF_GAMMA_FOLD_LONG=64 sends the
    longer ones to the block kernel, =1 every row of two ratings and more (most groups of a block then have no work)."""
    from pmf_hip import USER
    state = _fitted_state(K, dtype)
    row_ptr, ids, x = batch(7, state["dims"][1])
    prior = _prior(K, True)
    want = _reference(state, USER, row_ptr, ids, x, prior, 3)
    for threshold, launches in ((None, {"gamma_sweep": 1, "gamma_final": 0}), ("64", {"gamma_sweep": 1, "gamma_final": 1}),
                                ("1", {"gamma_sweep": 1, "gamma_final": 1})):
        if threshold is None:
            monkeypatch.delenv("PMF_GAMMA_FOLD_LONG", raising=False)
        else:
            monkeypatch.setenv("PMF_GAMMA_FOLD_LONG", threshold)
        with _open(state, K, dtype) as ctx:
            ctx.prof_enable(True)
            got = ctx.gamma_fold_in(USER, row_ptr, ids, x, *prior, n_iter=3)
            assert _launches(ctx) == launches, (threshold, _launches(ctx))
        _check(got, want, TOL[dtype][3], f"K={K} {dtype} threshold={threshold}")


def test_launches_do_not_depend_on_n_iter(monkeypatch):
    from pmf_hip import USER
    state = _fitted_state(8, "f32")
    row_ptr, ids, x = batch(7, state["dims"][1])
    monkeypatch.setenv("PMF_GAMMA_FOLD_LONG", "64")
    with _open(state, 8, "f32") as ctx:
        ctx.prof_enable(True)
        counts = []
        for n_iter in (1, 20):
            ctx.prof_reset()
            ctx.gamma_fold_in(USER, row_ptr, ids, x, *_prior(8, True), n_iter=n_iter)
            counts.append(_launches(ctx))
        assert counts[0] == counts[1] == {"gamma_sweep": 1, "gamma_final": 1}, counts


@pytest.mark.parametrize("hierarchical", [True, False])
@pytest.mark.parametrize("K,dtype,tol", [(20, "f64", 1e-11), (20, "f32", 3e-5), (64, "f64", 1e-11), (64, "f32", 3e-5)])
def test_folding_in_the_training_rows_is_the_user_half_sweep(K, dtype, tol, hierarchical):
    """Every user's own training ratings, warm-started from the context's E_theta / E_xi, 1 and 3 updates, against one
    and three `gamma_sweep(USER)` calls on the same context (the item side is not swept): the same state arrays."""
    from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, USER
    state = _fitted_state(K, dtype)
    U = state["dims"][0]
    u, i, x = state["ratings"]
    order = np.argsort(u, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=U))])
    lengths = np.diff(row_ptr)
    assert (lengths == 0).any() and (lengths > 2 * 16).sum() > 10        # empty rows; rows of several 16-lane batches
    prior = _prior(K, hierarchical)
    arrays = (ARR_FACTOR, ARR_SHAPE, ARR_RATE) + ((ARR_PRIOR_RATE, ARR_HYPER_RATE) if hierarchical else ())
    with _open(state, K, dtype) as ctx:
        init = (state["arrays"][(USER, ARR_FACTOR)], state["arrays"][(USER, ARR_PRIOR_RATE)] if hierarchical else None)
        folds = {n: ctx.gamma_fold_in(USER, row_ptr, i[order], x[order], *prior, n_iter=n, init_factor=init[0],
                                      init_prior_rate=init[1]) for n in (1, 3)}
        for n_sweeps in (1, 2, 3):
            ctx.gamma_sweep(USER, *prior)
            if n_sweeps in folds:
                errs = [rel_err(g, ctx.get_array(USER, a)) for g, a in zip(folds[n_sweeps], arrays)]
                print(f"K={K} {dtype} hier={hierarchical} {n_sweeps} sweep(s): " + " ".join("%.3g" % e for e in errs), f"(bound {tol})")
                assert max(errs) <= tol, (n_sweeps, errs)


def test_the_context_is_only_read():
    from pmf_hip import ITEM, USER
    K = 20
    state = _fitted_state(K, "f32")
    u, i, x = state["ratings"]
    with _open(state, K, "f32") as ctx:
        assert ctx.eval_set(u[:500], i[:500], x[:500])
        before = ctx.eval_run()
        for side in (USER, ITEM):
            row_ptr, ids, xs = batch(3, state["dims"][1 - side])
            ctx.gamma_fold_in(side, row_ptr, ids, xs, *_prior(K, True), n_iter=3)
            ctx.gamma_fold_in(side, row_ptr, ids, xs, *_prior(K, False), n_iter=2)
        assert len(state["arrays"]) == 10
        for (side, array), host in state["arrays"].items():
            assert np.array_equal(ctx.get_array(side, array), host), (side, array)
        assert ctx.eval_run() == before
        # ... and the work lists still drive the same sweep
        ctx.gamma_sweep(USER, *_prior(K, True))
        with _open(state, K, "f32") as fresh:
            fresh.gamma_sweep(USER, *_prior(K, True))
            for array in range(5):
                assert np.array_equal(ctx.get_array(USER, array), fresh.get_array(USER, array)), array


def test_row_blocks_and_repeat_calls_give_the_same_bits(monkeypatch):
    from pmf_hip import USER
    K = 20
    state = _fitted_state(K, "f32")
    rng = np.random.default_rng(11)
    lengths = rng.integers(0, 90, 70)
    lengths[[3, 40]] = 0
    lengths[33] = 300
    row_ptr, ids, x = batch(12, state["dims"][1], lengths)
    prior = _prior(K, True)
    results = {}
    for threshold in (None, "16"):                       # the lane-group kernel alone; both kernels
        if threshold is None:
            monkeypatch.delenv("PMF_GAMMA_FOLD_LONG", raising=False)
        else:
            monkeypatch.setenv("PMF_GAMMA_FOLD_LONG", threshold)
        monkeypatch.delenv("PMF_FOLD_IN_ROWS", raising=False)
        with _open(state, K, "f32") as ctx:
            whole = ctx.gamma_fold_in(USER, row_ptr, ids, x, *prior, n_iter=3)
            again = ctx.gamma_fold_in(USER, row_ptr, ids, x, *prior, n_iter=3)
        monkeypatch.setenv("PMF_FOLD_IN_ROWS", "32")
        with _open(state, K, "f32") as ctx:
            ctx.prof_enable(True)
            blocks = ctx.gamma_fold_in(USER, row_ptr, ids, x, *prior, n_iter=3)
            # 32 + 32 + 6 rows: one launch per block and kernel that has rows
            limit = np.inf if threshold is None else int(threshold)
            blocks_of = [lengths[r:r + 32] for r in (0, 32, 64)]
            assert _launches(ctx) == {"gamma_sweep": sum(bool((b <= limit).any()) for b in blocks_of),
                                      "gamma_final": sum(bool((b > limit).any()) for b in blocks_of)}
            assert _launches(ctx)["gamma_sweep"] == 3
        for a, b, c in zip(whole, again, blocks):
            assert np.array_equal(a, b) and np.array_equal(a, c), threshold
        results[threshold] = whole
    want = _reference(state, USER, row_ptr, ids, x, prior, 3)
    for threshold, got in results.items():
        _check(got, want, TOL["f32"][3], f"70 rows, threshold {threshold}")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rate_floor(dtype):
    """An all-zero start row against a table of order 1e-3: every rate of the first update is the floor 1e-10
    (hpf_cavi.py:141); bounds of test_poisson_rate_floor_and_zero_ratings for one update, TOL for three."""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    U, I, K = 6, 5, 4
    np_dtype = np.float64 if dtype == "f64" else np.float32
    Eb = (np.abs(np.random.default_rng(0).normal(size=(I, K))) * 1e-3).astype(np_dtype).astype(np.float64)
    row_ptr = np.array([0, 2, 3, 3, 7], dtype=np.int64)
    ids = np.array([0, 1, 1, 0, 0, 3, 4], dtype=np.int32)
    x = np.array([3.0, 0.0, 2.0, 4.0, 4.0, 0.0, 1.0])
    init = np.zeros((4, K))
    init[1] = np.float64(np_dtype(1e-9))
    init[3] = 0.5
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_array(ITEM, ARR_FACTOR, Eb)
        for n_iter, tol in ((1, 1e-12 if dtype == "f64" else 1e-5), (3, TOL[dtype][3])):
            got = ctx.gamma_fold_in(USER, row_ptr, ids, x, 0.1, 0.5, n_iter=n_iter, init_factor=init)
            want = fold_in_reference(Eb, row_ptr, ids, x, 0.1, 0.5, n_iter=n_iter, init_factor=init)
            _check(got, want, tol, f"rate floor {dtype} n_iter={n_iter}")
            if n_iter == 1:
                assert np.array_equal(got[1][0], np.full(K, np.float64(np_dtype(0.1))))   # theta = 0: the ratings add nothing to the shape


def test_errors_leave_the_outputs_alone():
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    lib = pmf_hip.load()
    K = 8
    state = _fitted_state(K, "f32")
    U, I = state["dims"]
    row_ptr, ids, x = batch(7, I, (3, 0, 4))
    n = 3
    outs = [np.full((n, K), 7.0) for _ in range(3)] + [np.full(n, 7.0) for _ in range(2)]
    init_f, init_r = _inits(1, n, K, "f32")
    hier = _prior(K, True)

    def call(h, side=USER, rp=row_ptr, o=ids, xs=x, prior=hier, n_iter=2, f0=init_f, r0=init_r, out=outs, n_rows=None):
        def p(a, t=C.c_double):
            return None if a is None else a.ctypes.data_as(C.POINTER(t))
        return lib.pmf_gamma_fold_in(h, side, n if n_rows is None else n_rows, p(rp, C.c_int64), p(o, C.c_int32), p(xs),
                                     prior[0], prior[1], int(prior[2]), prior[3], prior[4], n_iter, p(f0), p(r0), *[p(a) for a in out])

    def untouched():
        return all((a == 7.0).all() for a in outs)

    def refused(code, fragment, **kw):
        h = kw.pop("h", ctx._h)
        assert call(h, **kw) == code, (kw, lib.pmf_last_error())
        msg = lib.pmf_last_error().decode()
        assert msg.startswith("pmf_gamma_fold_in:") and fragment in msg, msg
        assert untouched(), kw

    with _open(state, K, "f32") as ctx:
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
            refused(PMF_EINVAL, "rate_prior", prior=(A, bad, False, 0.0, 0.0))
            refused(PMF_EINVAL, "hyper_shape", prior=(A, 1.0, True, bad, B_PRIME))
            refused(PMF_EINVAL, "hyper_rate_prior", prior=(A, 1.0, True, hier[3], bad))
        refused(PMF_EINVAL, "n_iter", n_iter=0)
        bad = ids.copy()
        bad[-1] = I                          # the last position of the last row
        refused(PMF_ERANGE, f"id {I} at position {len(ids) - 1}", o=bad)
        bad[-1] = -1
        refused(PMF_ERANGE, "id -1", o=bad)
        refused(PMF_ERANGE, f"id {U} at position 0", side=ITEM, o=np.full_like(ids, U))   # the opposite side of ITEM is the users
        # n_rows = 0 with a valid context: success, nothing touched (the arrays may then be null)
        assert call(ctx._h, n_rows=0) == 0
        assert call(ctx._h, n_rows=0, rp=None, o=None, xs=None, f0=None, r0=None, out=[None] * 5) == 0
        assert untouched()
        # hierarchical ignores rate_prior, whatever it is
        want = _reference(state, USER, row_ptr, ids, x, hier, 2, init_f, init_r)
        # the optional outputs and start values
        assert call(ctx._h, out=[outs[0], None, None, None, None], prior=(A, -3.0) + hier[2:]) == 0
        assert all((a == 7.0).all() for a in outs[1:])
        assert rel_err(outs[0], want[0]) <= TOL["f32"][3]
        assert call(ctx._h) == 0
        _check(outs, want, TOL["f32"][3], "raw call, warm")
        assert call(ctx._h, f0=None, r0=None) == 0
        _check(outs, _reference(state, USER, row_ptr, ids, x, hier, 2), TOL["f32"][3], "raw call, cold")
    for a in outs:
        a[:] = 7.0
    # the opposite side's FACTOR is needed (and named); nothing of `side` itself, no ratings
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        refused(PMF_EINVAL, "array FACTOR of side 1")
        ctx.set_array(ITEM, ARR_FACTOR, state["arrays"][(ITEM, ARR_FACTOR)])
        refused(PMF_EINVAL, "array FACTOR of side 0", side=ITEM, o=np.zeros_like(ids))
        assert call(ctx._h) == 0
        _check(outs, _reference(state, USER, row_ptr, ids, x, hier, 2, init_f, init_r), TOL["f32"][3], "only the other side's FACTOR")


def _fit(kind, K=16):
    import pandas as pd
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    u, i, x = skewed_problem(100 + K, 600, 120, 12000)
    df = pd.DataFrame({"u": u, "i": i, "rating": x})
    if kind == "hpf":
        cfg = HPF_CAVI_Config(n_factors=K, a=0.3, a_prime=5.0, b_prime=4.0, c=0.4, c_prime=3.0, d_prime=2.0, max_iter=3, tol=None,
                              random_state=3, verbose=False)
        return HPF_CAVI(cfg).fit(df)
    return PoissonMFCAVI(PoissonMFCAVIConfig(n_factors=K, a0=0.3, b0=1.5, max_iter=3, tol=None, random_state=3, verbose=False)).fit(df)


@pytest.mark.parametrize("kind", ["hpf", "poisson"])
def test_model_surface(kind):
    """`fold_in_users` of a frame with string labels (interleaved, so grouping must keep each user's frame order) and one
    item id the fit has not seen; `fold_in_items` with integer labels far outside the trained range; the record."""
    import pandas as pd
    rng = np.random.default_rng(2)
    m = _fit(kind)
    cfg, K = m.config, m.config.n_factors
    dtype = m._dtype
    if kind == "hpf":
        priors = ((cfg.a, 0.0, True, cfg.a_prime + K * cfg.a, cfg.b_prime), (cfg.c, 0.0, True, cfg.c_prime + K * cfg.c, cfg.d_prime))
    else:
        priors = ((cfg.a0, cfg.b0, False, 0.0, 0.0),) * 2
    n = 90
    labels = rng.choice(np.array(["zed", "amy", "bob"]), n)
    items = rng.integers(0, m.n_items, n)
    items[17] = m.n_items + 5                                   # unseen: dropped
    ratings = rng.integers(0, 6, n).astype(float)
    fold = m.fold_in_users(pd.DataFrame({"u": labels, "i": items, "rating": ratings}), n_iter=3)
    assert list(fold.ids) == ["amy", "bob", "zed"]
    keep = np.arange(n) != 17
    rows = [np.flatnonzero((labels == name) & keep) for name in fold.ids]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    pos = np.concatenate(rows)
    want = fold_in_reference(m.E_beta, row_ptr, items[pos], ratings[pos], *priors[0], n_iter=3)
    _check((fold.E, fold.shape, fold.rate, fold.prior_rate), want[:4], TOL[dtype][3], f"{kind} fold_in_users")
    assert (fold.prior_rate is None) == (kind == "poisson") and fold.E_other is m.E_beta
    q_rows, q_items = np.array([2, 0, 1, 1]), np.array([0, 5, 7, m.n_items - 1])
    assert np.allclose(fold.predict(q_rows, q_items), np.einsum("nk,nk->n", fold.E[q_rows], m.E_beta[q_items]), rtol=0, atol=1e-14)
    users = rng.integers(0, m.n_users, 40)
    new_items = rng.choice(np.array([10**6, 777777]), 40)
    fi = m.fold_in_items(pd.DataFrame({"u": users, "i": new_items, "rating": ratings[:40]}), n_iter=20)
    assert list(fi.ids) == [777777, 10**6]
    rows = [np.flatnonzero(new_items == name) for name in fi.ids]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    pos = np.concatenate(rows)
    want = fold_in_reference(m.E_theta, row_ptr, users[pos], ratings[:40][pos], *priors[1], n_iter=20)
    _check((fi.E, fi.shape, fi.rate, fi.prior_rate), want[:4], TOL[dtype][20], f"{kind} fold_in_items")
    assert fi.E_other is m.E_theta
    assert m.fold_in_users(pd.DataFrame({"u": labels, "i": items, "rating": ratings})).E.shape == (3, K)    # n_iter defaults to 10
    m.close()
