"""`pmf_gamma_elbo_terms` -- the per-row sums of the Poisson MF / HPF evidence lower bound -- against the dense float64
restatement in tests/gamma_elbo_reference.py, evaluated on the state read back from the device (so the rounding of the
inputs is not part of the error), every row and every term; then the model surface (`elbo`, `fit(track_elbo=, elbo_tol=)`).

Bounds.  None is a number found by running the kernel.

Double terms (all but DATA): |got - ref| <= 1e-11 mag_r, mag_r = the sum of the absolute values of every product that
enters the term.  The row pass is double arithmetic over at most K <= 256 addends (a DPP tree of depth <= 8 over
4-element lane sums: under 12 roundings of 1.1e-16 on any path) with psi, lgamma and log good to about 1e-13 relative
-- 1e-11 leaves two digits and still fails by four orders of magnitude if the row pass runs in fp32 (6e-8).  LOGFACT is
a sum of at most n_r double values good to about 1e-13 relative (Stirling's series past 10, truncation below 6.4e-16; 0
exactly for the ratings 0 and 1), n_r <= 9000 roundings of 1.1e-16: below 1e-11 of sum_j |lgamma(x_j + 1)| as well.

DATA, with eps the unit roundoff 2^-24 (fp32) or 2^-53 (fp64) of the context, n_r the ratings of the row:
    |got - ref| <= eps (n_r + K + 16) mag_r,
    mag_r = sum_j [ x_j (max_k |Elog_rk| + max_k |Elog_ok| + |lse_j|) + sum_k E_rk E_ok ].
Per rating: each table entry carries one rounding (eps/2 relative) and so does the sum s_k = Elog_rk + Elog_ok, so
|d s_k| <= 1.5 eps (max|Elog_r| + max|Elog_o|); s_k - m rounds once more (<= eps (max + max)); exp turns an absolute
error of its argument into a relative one and adds 2 ulp of its own; the K addends are summed as 4 per lane and a DPP
tree (<= 2 + log2(K/4) roundings); log adds 2 ulp and m + log z one rounding of |lse|.  Together
    |d lse_j| <= eps [ 2.5 (max + max) + (6 + log2 K) + |lse_j| ]  <=  eps (K + 16)/2 (max + max + |lse_j|)
once max + max + |lse_j| >= (12 + 2 log2 K) / (K + 11), which is at most 1.1 (asserted for the states used; at K = 1
the constant term is absent: s - m = 0, z = 1 and log z = 0 exactly).  The dot product: two table roundings, the products and
the same tree, <= eps (4 + log2 K) sum_k E E <= eps (K + 16)/2 sum_k E E.  x_j times lse_j and the subtraction: 2 more
roundings of the rating's magnitude.  The row sum adds the n_r values one by one inside a task, the tasks of a split row
one by one in slot order: every value passes through at most n_r additions in all, whatever the task length, each
rounding at most eps/2 of a partial sum that is below mag_r -- n_r eps mag_r / 2.  Sum: below eps (n_r + K + 16) mag_r.
The kernel's tree is exactly this one (lane sum, DPP steps, sequential tasks and slots), so nothing is restated."""
import ctypes as C

import numpy as np
import pytest

import gamma_elbo_reference as ref
from helpers import skewed_problem

pytestmark = pytest.mark.gpu

PMF_EINVAL = -1
U, I, N = 37, 29, 1500
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
DOUBLE_TOL = 1e-11
HYPER_TERMS = (ref.LOG_HYPER, ref.INV_HYPER, ref.FACTOR_OVER_HYPER)
NAMES = ("SUM_FACTOR", "SUM_ELOG", "ENTROPY", "LOG_HYPER", "INV_HYPER", "FACTOR_OVER_HYPER", "DATA", "LOGFACT")
KAPPA = 2.7        # shape of q(xi) / q(eta) wherever a sweep needs one


def _problem():
    """The 37 x 29 problem of tests/test_gamma_elbo_cpu.py with every eleventh rating set to 0."""
    u, i, x = skewed_problem(5, U, I, N, "count")
    x = x.copy()
    x[::11] = 0.0
    return u, i, x


def _draw_state(seed, n_users, n_items, K):
    """Shapes log-uniform in [0.3, 1e4] plus one element of 1e6, rates and hyper rates log-uniform in [0.5, 1e3]."""
    rng = np.random.default_rng(seed)
    lu = lambda lo, hi, size: np.exp(rng.uniform(np.log(lo), np.log(hi), size=size))
    st = {"a_theta": lu(0.3, 1e4, (n_users, K)), "b_theta": lu(0.5, 1e3, (n_users, K)),
          "a_beta": lu(0.3, 1e4, (n_items, K)), "b_beta": lu(0.5, 1e3, (n_items, K)),
          "h_xi": lu(0.5, 1e3, n_users), "h_eta": lu(0.5, 1e3, n_items)}
    st["a_theta"][n_users // 2, K // 2] = 1e6
    return st


class _Case:
    """A context holding the ratings and a drawn state; `st` is that state as read back from the device."""

    def __init__(self, K, dtype, ratings=None, dims=(U, I), seed=None):
        import pmf_hip
        from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER
        self.K, self.dtype = K, dtype
        self.u, self.i, self.x = ratings if ratings is not None else _problem()
        drawn = _draw_state(K if seed is None else seed, *dims, K)
        self.ctx = ctx = pmf_hip.Context(*dims, K, dtype=dtype)
        ctx.set_ratings(self.u, self.i, self.x)
        self.st = {}
        for side, name, hyper in ((USER, "theta", "h_xi"), (ITEM, "beta", "h_eta")):
            for arr, key in ((ARR_SHAPE, "a_" + name), (ARR_RATE, "b_" + name), (ARR_HYPER_RATE, hyper)):
                ctx.set_array(side, arr, drawn[key])
                self.st[key] = ctx.get_array(side, arr)
            # what a following sweep reads
            ctx.set_array(side, ARR_FACTOR, self.st["a_" + name] / self.st["b_" + name])
            ctx.set_array(side, ARR_PRIOR_RATE, KAPPA / self.st[hyper])

    def reference(self, side):
        """(terms, mags, ratings per row) of a hierarchical call with data, computed once per side."""
        if not hasattr(self, "_ref"):
            self._ref = {}
        if side not in self._ref:
            self._ref[side] = ref.side_terms(self.st, side, self.u, self.i, self.x, hierarchical=True)
        return self._ref[side]

    def bounds(self, side):
        """[rows, TERMS]: the allowed |got - ref| of every term"""
        _, mags, count = self.reference(side)
        out = DOUBLE_TOL * mags
        out[:, ref.DATA] = EPS[self.dtype] * (count + self.K + 16) * mags[:, ref.DATA]
        return out

    def close(self):
        self.ctx.close()


def _check_rows(case, side, with_data, hierarchical, what):
    totals, got = case.ctx.gamma_elbo_terms(side, with_data=with_data, hierarchical=hierarchical, per_row=True)
    want, _, count = case.reference(side)
    want, bound = want.copy(), case.bounds(side)
    if not hierarchical:
        want[:, HYPER_TERMS] = 0.0
        assert (got[:, HYPER_TERMS] == 0.0).all(), what
    if not with_data:
        want[:, (ref.DATA, ref.LOGFACT)] = 0.0
        assert (got[:, (ref.DATA, ref.LOGFACT)] == 0.0).all(), what
    err = np.abs(got - want)
    worst = np.max(err / np.where(bound > 0, bound, 1.0), axis=0)
    print(what, " ".join("%s %.2g" % (n, w) for n, w in zip(NAMES, worst)), "(fractions of the bound)")
    assert np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, np.argwhere(err > bound)[:5], worst)
    empty = count == 0
    assert (got[empty][:, (ref.DATA, ref.LOGFACT)] == 0.0).all(), what       # a row without ratings: exactly 0
    # totals: the sequential double sum of the rows
    seq = np.zeros(ref.TERMS)
    for row in got:
        seq = seq + row
    assert totals.tobytes() == seq.tobytes(), what
    return totals, got


def test_problem_has_split_rows_empty_rows_and_zero_ratings():
    import pmf_hip
    from pmf_hip import ITEM, USER
    u, i, x = _problem()
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    assert nu.max() > 32 and ni.max() > 32 and (nu == 0).any() and (ni == 0).any()
    assert (x == 0).sum() > 100 and x.max() == 6
    with pmf_hip.Context(U, I, 5) as ctx:
        ctx.set_ratings(u, i, x)
        assert ctx.task_max_len(USER, "gamma") <= 32 and ctx.task_max_len(ITEM, "gamma") <= 32    # the default task length


CASES = [(K, "f32") for K in (1, 3, 5, 8, 16, 17, 33, 64, 65, 128, 129, 256)] + [(K, "f64") for K in (5, 16, 64, 129)]


@pytest.mark.parametrize("K,dtype", CASES)
def test_every_row_and_term_against_the_reference(K, dtype):
    """Every lane-group width (K = 1 .. 256), pad-carrying K (1, 3, 5, 17, 33, 65, 129), inactive lanes (K = 17, 33, 65,
    129: the group is wider than kpad / 4); hierarchical and not, with and without data, both sides; the data term from
    the two sides; the same bits from a second call."""
    from pmf_hip import ITEM, USER
    case = _Case(K, dtype)
    try:
        # the derivation of the DATA bound assumes max|Elog_r| + max|Elog_o| (+ |lse|) >= 1.1 for every rating when K > 1
        L = {n: ref.expectations(case.st["a_" + n], case.st["b_" + n])[1] for n in ("theta", "beta")}
        assert K == 1 or (np.abs(L["theta"]).max(axis=1)[case.u] + np.abs(L["beta"]).max(axis=1)[case.i]).min() >= 1.1
        sums = {}
        for side in (USER, ITEM):
            for hierarchical in (False, True):
                _check_rows(case, side, False, hierarchical, f"K={K} {dtype} side={side} hier={hierarchical} no data")
                totals, rows = _check_rows(case, side, True, hierarchical, f"K={K} {dtype} side={side} hier={hierarchical} data")
                again, rows_again = case.ctx.gamma_elbo_terms(side, with_data=True, hierarchical=hierarchical, per_row=True)
                assert again.tobytes() == totals.tobytes() and rows_again.tobytes() == rows.tobytes()
                assert case.ctx.gamma_elbo_terms(side, with_data=True, hierarchical=hierarchical).tobytes() == totals.tobytes()
            bound = case.bounds(side)
            sums[side] = (totals[ref.DATA] - totals[ref.LOGFACT], bound[:, ref.DATA].sum() + bound[:, ref.LOGFACT].sum())
        gap = abs(sums[USER][0] - sums[ITEM][0])
        print(f"K={K} {dtype}: data term by users {sums[USER][0]:.9g}, by items {sums[ITEM][0]:.9g}, gap {gap:.3g} of {sums[USER][1] + sums[ITEM][1]:.3g}")
        assert gap <= sums[USER][1] + sums[ITEM][1]
    finally:
        case.close()


@pytest.mark.parametrize("K,length", [(64, 700), (3, 9000)])
@pytest.mark.parametrize("chunk", ["32", "512"])
def test_long_rows_under_both_task_lengths(K, length, chunk, monkeypatch):
    """One row of 700 ratings at K = 64 (22 partial sums under task length 32: more than the 16 lane groups of a block)
    and one of 9000 at K = 3 (282: more than 256), each also as one or a few tasks under task length 512."""
    from pmf_hip import ITEM, USER
    rng = np.random.default_rng(length)
    n_items = 40
    u = np.concatenate([np.full(length, 1), [0, 2, 2]])
    i = np.concatenate([rng.integers(0, n_items, length), [0, 1, n_items - 1]])
    x = rng.integers(0, 7, len(u)).astype(np.float64)
    monkeypatch.setenv("PMF_TASK_CHUNK", chunk)
    case = _Case(K, "f32", ratings=(u, i, x), dims=(3, n_items), seed=length)
    try:
        longest = case.ctx.task_max_len(USER, "gamma")
        assert longest <= int(chunk) and (longest > 32) == (chunk == "512")
        for side in (USER, ITEM):
            _check_rows(case, side, True, True, f"K={K} row of {length}, task length {chunk}, side={side}")
    finally:
        case.close()


def test_the_call_reads_only():
    """Every state array is the same bits after the calls; a sweep after them gives the bits it gives on a twin context
    that never made one; the context's device memory does not grow on the second call."""
    from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER
    cases = [_Case(20, "f32"), _Case(20, "f32")]
    try:
        a, b = cases

        def state(ctx):
            return [ctx.get_array(s, arr).tobytes() for s in (USER, ITEM)
                    for arr in (ARR_FACTOR, ARR_SHAPE, ARR_RATE, ARR_PRIOR_RATE, ARR_HYPER_RATE)]

        def calls():
            for side in (USER, ITEM):
                for with_data in (False, True):
                    a.ctx.gamma_elbo_terms(side, with_data=with_data, hierarchical=True, per_row=True)
        before = state(a.ctx)
        calls()
        held = a.ctx.device_bytes()
        calls()
        assert a.ctx.device_bytes() == held
        assert state(a.ctx) == before and state(b.ctx) == before
        for ctx in (a.ctx, b.ctx):
            ctx.gamma_sweep(USER, 0.3, 0.0, True, KAPPA, 1.0)
            ctx.gamma_sweep(ITEM, 0.3, 0.0, True, KAPPA, 1.0)
        assert state(a.ctx) == state(b.ctx) and state(a.ctx) != before
    finally:
        for c in cases:
            c.close()


def test_refusals():
    import pmf_hip
    from pmf_hip import ARR_HYPER_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER
    lib = pmf_hip.load()
    tot = np.full(ref.TERMS, 7.0)
    rows = np.full(U * ref.TERMS, 7.0)
    pt, pr = pmf_hip.ptr(tot, C.c_double), pmf_hip.ptr(rows, C.c_double)

    def refused(ctx, side, with_data, hierarchical, totals, text):
        h = ctx._h if ctx is not None else None
        assert lib.pmf_gamma_elbo_terms(h, side, with_data, hierarchical, totals, pr) == PMF_EINVAL
        assert text in lib.pmf_last_error().decode(), lib.pmf_last_error()
        assert (tot == 7.0).all() and (rows == 7.0).all()           # an argument error writes nothing
    u, i, x = _problem()
    st = _draw_state(1, U, I, 5)
    with pmf_hip.Context(U, I, 5) as ctx:
        refused(None, USER, 0, 0, pt, "null context")
        refused(ctx, 2, 0, 0, pt, "bad side 2")
        refused(ctx, -1, 1, 1, pt, "bad side -1")
        refused(ctx, USER, 0, 0, None, "null totals")
        refused(ctx, USER, 0, 0, pt, "array SHAPE of side 0")
        ctx.set_array(USER, ARR_SHAPE, st["a_theta"])
        refused(ctx, USER, 0, 0, pt, "array RATE of side 0")
        ctx.set_array(USER, ARR_RATE, st["b_theta"])
        refused(ctx, USER, 1, 0, pt, "array SHAPE of side 1")
        refused(ctx, ITEM, 0, 0, pt, "array SHAPE of side 1")
        ctx.set_array(ITEM, ARR_SHAPE, st["a_beta"])
        refused(ctx, USER, 1, 0, pt, "array RATE of side 1")
        ctx.set_array(ITEM, ARR_RATE, st["b_beta"])
        refused(ctx, USER, 1, 0, pt, "ratings have not been set")
        refused(ctx, USER, 0, 1, pt, "array HYPER_RATE of side 0")
        # without the data term no ratings are needed
        got = ctx.gamma_elbo_terms(USER, with_data=False)
        assert np.isfinite(got).all() and got[ref.DATA] == 0.0 and got[ref.LOGFACT] == 0.0 and got[ref.LOG_HYPER] == 0.0
        ctx.set_ratings(u, i, x)
        assert np.isfinite(ctx.gamma_elbo_terms(USER, with_data=True)).all()
        refused(ctx, USER, 1, 1, pt, "array HYPER_RATE of side 0")
        ctx.set_array(USER, ARR_HYPER_RATE, st["h_xi"])
        assert np.isfinite(ctx.gamma_elbo_terms(USER, with_data=True, hierarchical=True)).all()     # eta is not needed


# ---- model surface -----------------------------------------------------------------------------------------------------
MODEL_K = 8
POISSON_CFG = dict(a0=0.3, b0=1.0)
HPF_CFG = dict(a=0.3, a_prime=0.3, b_prime=1.0, c=0.4, c_prime=0.5, d_prime=1.5)


def _frame(x=None):
    import pandas as pd
    u, i, x0 = _problem()
    return pd.DataFrame({"u": u, "i": i, "rating": x0 if x is None else x})


def _fit(model, dtype, verbose=False, max_iter=5, **kw):
    if model == "hpf":
        from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
        m = HPF_CAVI(HPF_CAVI_Config(n_factors=MODEL_K, max_iter=max_iter, tol=None, random_state=3, verbose=verbose, **HPF_CFG), dtype=dtype)
    else:
        from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
        m = PoissonMFCAVI(PoissonMFCAVIConfig(n_factors=MODEL_K, max_iter=max_iter, tol=None, random_state=3, verbose=verbose, **POISSON_CFG),
                          dtype=dtype)
    return m.fit(_frame(), **kw)


def _state_arrays(m, model):
    names = (("gamma_a_theta", "gamma_b_theta", "gamma_a_beta", "gamma_b_beta", "gamma_b_xi", "gamma_b_eta", "E_theta", "E_beta", "E_xi",
              "E_eta") if model == "hpf" else ("a_theta", "b_theta", "a_beta", "b_beta", "E_theta", "E_beta"))
    return [(n, np.asarray(getattr(m, n), dtype=np.float64)) for n in names]


def _reference_elbo(m, model, dtype):
    """(the bound of the pulled state in float64, the allowed distance): the bound is linear in the device's totals, so
    the distance is sum over terms of |coefficient| x the term's summed per-row bounds, plus 1e-12 of the parts'
    magnitudes for the host's own float64 assembly."""
    u, i, x = _problem()
    pre = "gamma_" if model == "hpf" else ""
    st = {k: getattr(m, pre + k) for k in ("a_theta", "b_theta", "a_beta", "b_beta")}
    eps = EPS[dtype]
    if model == "hpf":
        st["h_xi"], st["h_eta"] = m.gamma_b_xi, m.gamma_b_eta
        priors = ((HPF_CFG["a"], HPF_CFG["a_prime"], HPF_CFG["b_prime"]), (HPF_CFG["c"], HPF_CFG["c_prime"], HPF_CFG["d_prime"]))
        want = ref.elbo_hpf(st, u, i, x, *priors)
    else:
        priors = ((POISSON_CFG["a0"], POISSON_CFG["b0"]),) * 2
        want = ref.elbo_poisson(st, u, i, x, *priors[0])
    allowed = 0.0
    for side, prior in ((0, priors[0]), (1, priors[1])):
        _, mags, count = ref.side_terms(st, side, u, i, x, hierarchical=model == "hpf", with_data=side == 0)
        per_term = DOUBLE_TOL * mags.sum(axis=0)
        per_term[ref.DATA] = np.sum(eps * (count + MODEL_K + 16) * mags[:, ref.DATA])
        coef = np.zeros(ref.TERMS)
        coef[[ref.ENTROPY, ref.DATA, ref.LOGFACT]] = 1.0
        if model == "hpf":
            s, s1, r1 = prior
            kappa = s1 + MODEL_K * s
            coef[ref.SUM_ELOG], coef[ref.FACTOR_OVER_HYPER], coef[ref.INV_HYPER] = abs(s - 1.0), kappa, r1 * kappa
            coef[ref.LOG_HYPER] = abs(MODEL_K * s + (s1 - 1.0) + 1.0)
        else:
            coef[ref.SUM_ELOG], coef[ref.SUM_FACTOR] = abs(prior[0] - 1.0), prior[1]
        allowed += float(coef @ per_term)
    return want, allowed


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("model", ["poisson", "hpf"])
def test_fit_tracks_the_elbo_and_elbo_matches_the_reference(model, dtype):
    tracked, plain = _fit(model, dtype, track_elbo=True), _fit(model, dtype)
    try:
        L = tracked.history_["elbo"]
        assert len(L) == 5 and tracked.history_["iterations"] == 5 and not tracked.history_["stopped_early"]
        assert tracked.elbo() == L[-1]
        value, parts = tracked.elbo(parts=True)
        assert value == L[-1] and abs(sum(parts.values()) - value) <= 1e-12 * abs(value)
        want, allowed = _reference_elbo(tracked, model, dtype)
        allowed += 1e-12 * sum(abs(v) for v in parts.values())
        print(f"{model} {dtype}: elbo {value:.6f}, reference {want:.6f}, distance {abs(value - want):.3g} of {allowed:.3g}; trace {L}")
        assert abs(value - want) <= allowed
        # tracking changes no bit of the fit, and the default fit has no trace of it
        assert "elbo" not in plain.history_
        for (name, got), (_, base) in zip(_state_arrays(tracked, model), _state_arrays(plain, model)):
            assert got.tobytes() == base.tobytes(), name
        assert plain.elbo() == L[-1]
    finally:
        tracked.close()
        plain.close()


@pytest.mark.parametrize("model", ["poisson", "hpf"])
def test_elbo_tol_stops_after_the_second_iteration(model):
    m = _fit(model, "f32", elbo_tol=1.0)
    try:
        assert m.history_["iterations"] == 2 and m.history_["stopped_early"] and len(m.history_["elbo"]) == 2
    finally:
        m.close()


@pytest.mark.parametrize("model", ["poisson", "hpf"])
def test_default_fit_prints_no_elbo_line(model, capsys):
    """With the two arguments left alone the text is the tracked fit's minus its ELBO lines."""
    plain = _fit(model, "f32", verbose=True, max_iter=3)
    text_plain = capsys.readouterr().out
    tracked = _fit(model, "f32", verbose=True, max_iter=3, track_elbo=True)
    text_tracked = capsys.readouterr().out
    plain.close()
    tracked.close()
    assert "ELBO" not in text_plain and "iteration 3/3" in text_plain
    lines = text_tracked.splitlines(keepends=True)
    elbo_lines = [ln for ln in lines if ln.startswith("ELBO: ")]
    assert len(elbo_lines) == 3 and elbo_lines[-1] == f"ELBO: {tracked.history_['elbo'][-1]:.4f}\n"
    assert "".join(ln for ln in lines if not ln.startswith("ELBO: ")) == text_plain


def test_model_refusals():
    from src.models.poisson_mf_extended_cavi import PoissonMFExtendedCAVI, PoissonMFExtendedCAVIConfig

    class World:          # what DeviceModel looks at of a communicator
        world, rank = 2, 0
    for model in ("poisson", "hpf"):
        m = _fit(model, "f32", max_iter=0)
        try:
            with pytest.raises(RuntimeError, match="no iteration"):
                m.elbo()
            x = _problem()[2].copy()
            x[3] = -1.0
            with pytest.raises(ValueError, match="negative"):
                m.fit(_frame(x), track_elbo=True)
            m.fit(_frame(x))                      # (without the ELBO a negative rating is the caller's business, as before)
        finally:
            m.close()
        sharded = type(m)(m.config, comm=World())
        with pytest.raises(NotImplementedError, match="communicator"):
            sharded.fit(_frame(), track_elbo=True)
    ext = PoissonMFExtendedCAVI(PoissonMFExtendedCAVIConfig(n_factors=4, max_iter=1, verbose=False))
    with pytest.raises(NotImplementedError, match="PoissonMFExtendedCAVI"):
        ext.elbo()
    with pytest.raises(NotImplementedError, match="PoissonMFExtendedCAVI"):
        ext.fit(_frame(), track_elbo=True)
