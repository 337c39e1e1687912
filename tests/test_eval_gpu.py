"""`pmf_predict` and the fused validation reduction (`pmf_eval_set` / `pmf_eval_run`, csrc/pmf_eval.hip) against a
NumPy reference of the same operation, with a derived error bound asserted on every pair and every sum.

Reference.  The tables are read back from the device (`get_array`), so the fp32 rounding of the inputs is not part of
the error.  fp32 tables are exact in float64 and so are their products; the float64 reference is then far below
u = 2^-24.  For fp64 contexts the dot product is accumulated in NumPy's extended precision (`np.longdouble`, 64-bit
mantissa on x86) where that is wider than float64, so that the reference's own rounding ((K + 3) 2^-64 of the
magnitude below, < 0.13 u at K = 256) disappears in the slack between the 14 roundings counted and the constant 16;
where `longdouble` is float64 the reference is plain float64.

Per pair.  `predict_pair` rounds a product at most 4 times in its lane (one multiply, three fmas), log2(L) <= 6 times
in the lane-group sum, twice in the scale multiplies (su * si, then * dot) and twice in the bias adds
(bu + bi, then + dot): 14 roundings.  Standard forward-error analysis (every term's relative error <= gamma_14 < 16 u)
gives

    |got - ref| <= delta = 16 u (|su si| sum_k |a_k b_k| + |bu| + |bi|) + 4 * 2^-53 |ref|

with u = 2^-24 (fp32 contexts) or 2^-53 (fp64), the terms of a flag that is off left out; the last term is the
conversion to double and the added `offset`.  The bound scales with sum |a b|, not with |ref|: the factors are signed
(standard normal), so cancellation is real.  A pair with an id outside the trained dimensions is exactly `offset`
(delta = 0).  `_check_pairs` asserts the bound on every pair; there is no outlier allowance.

Sums.  With e_i = y_i - ref_i the device sums obey

    |sum_sq_err - sum e_i^2|        <= sum_i (2 |e_i| delta_i + delta_i^2) + n 2^-52 sum_i e_i^2
    |abs_err_per_label[l] - sum_l|e_i|| <= sum_{i in l} delta_i          + n 2^-52 sum_{i in l} |e_i|

(the second terms: each e_i and its square are rounded once, the n terms are added in some order, all in double;
(n + 2) 2^-53 <= n 2^-52 from n = 2, and in the n = 1 edge cases, K >= 16, the delta term is hundreds of u times
|e| and carries the missing 2^-53 e^2).  `count_per_label` and n are exact.  The vector of `eval_sums` is compared, not
only (rmse, macro_mae); where the final figures are compared the same bounds are pushed through
sqrt(sse / n) and mean_l(abs_l / cnt_l).

Second, tighter check: both kernels call `predict_pair` with the same lane-group width, so `predict` on the same
pairs returns the bits the reduction saw; the sums formed on the host from it (`math.fsum`) must agree within the
n 2^-52 summation term alone.  Two `eval_sums` calls in a row are bit-identical (block-ordered, no atomics).

No tolerance below is a number found by running the kernel."""
import ctypes as C
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT32_MAX = np.iinfo(np.int32).max
INT32_MIN = np.iinfo(np.int32).min
PMF_ERANGE = -4                                   # include/pmf_hip.h
WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else np.float64
LANE_KS = [1, 3, 4, 5, 8, 12, 16, 17, 32, 33, 64, 65, 100, 128, 129, 250, 256]   # L = 4, 4, 4, 8, ..., 64
ALL_FLAG_KS = (1, 20, 64, 256)
RATINGS = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
RATING_P = [0.038, 0.012, 0.036, 0.142, 0.772]    # helpers.skewed_problem's skew (its two rarest merged)


def _flags(K):
    return (0, 1, 2, 3) if K in ALL_FLAG_KS else (0, 3)


def _groups(ctx):
    """pairs per 256-thread block: 256 / max(4, lanes per row)"""
    lanes = 1
    while lanes < ctx.kpad // 4:
        lanes <<= 1
    return 256 // max(4, lanes)


def _fill(ctx, rng):
    """Standard-normal FACTOR, BIAS and SCALE tables; returns them as the device holds them."""
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ARR_SCALE, ITEM, USER
    tabs = {}
    for side, rows, s in ((USER, ctx.n_users, "u"), (ITEM, ctx.n_items, "i")):
        ctx.set_array(side, ARR_FACTOR, rng.standard_normal((rows, ctx.K)))
        ctx.set_array(side, ARR_BIAS, rng.standard_normal(rows))
        ctx.set_array(side, ARR_SCALE, rng.standard_normal(rows))
        tabs["f" + s], tabs["b" + s], tabs["s" + s] = (ctx.get_array(side, a) for a in (ARR_FACTOR, ARR_BIAS, ARR_SCALE))
    return tabs


class _Ref:
    """The reference prediction and its bound `delta` for the pairs (u, i); the dot products are formed once
    (in chunks, to bound memory) and shared by the flag values."""

    def __init__(self, ctx, tabs, u, i):
        from pmf_hip import F64
        self.t, self.K = tabs, ctx.K
        self.unit = 2.0 ** -53 if ctx.dtype == F64 else 2.0 ** -24
        self.acc = WIDE if ctx.dtype == F64 else np.float64
        u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
        self.ok = (u >= 0) & (u < ctx.n_users) & (i >= 0) & (i < ctx.n_items)
        self.u, self.i = np.where(self.ok, u, 0), np.where(self.ok, i, 0)
        n = len(u)
        self.dot, self.mag = np.zeros(n, self.acc), np.zeros(n)
        step = max(1, (1 << 20) // ctx.K)

        def work(lo):
            sl = slice(lo, lo + step)
            p = tabs["fu"][self.u[sl]].astype(self.acc)
            p *= tabs["fi"][self.i[sl]]
            self.dot[sl] = p.sum(axis=1)
            self.mag[sl] = np.abs(p).sum(axis=1)
        with ThreadPoolExecutor(8) as pool:
            list(pool.map(work, range(0, n, step)))

    def at(self, flag, offset):
        """(ref in the accumulation type, delta in float64)"""
        t, val, mag = self.t, self.dot.copy(), self.mag.copy()
        if flag & 2:
            s = t["su"][self.u].astype(self.acc) * t["si"][self.i]
            val *= s
            mag *= np.abs(s).astype(np.float64)
        if flag & 1:
            val += t["bu"][self.u].astype(self.acc) + t["bi"][self.i]
            mag += np.abs(t["bu"][self.u]) + np.abs(t["bi"][self.i])
        ref = np.where(self.ok, val + offset, self.acc(offset))
        delta = np.where(self.ok, 16.0 * self.unit * mag + 4.0 * 2.0 ** -53 * np.abs(ref).astype(np.float64), 0.0)
        return ref, delta


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


def _sum_reference(y, lab, n_labels, ref, delta):
    """Reference sums and their bounds (module docstring): sse, b_sse, abs_l[32], b_abs[32], cnt[32]."""
    from pmf_hip import MAX_LABELS
    n = len(y)
    e = y.astype(ref.dtype) - ref
    ae = np.abs(e)
    sse = float(np.sum(e * e))
    b_sse = float(np.sum(2.0 * ae * delta + delta * delta)) + n * 2.0 ** -52 * sse
    abs_l, b_abs, cnt = np.zeros(MAX_LABELS), np.zeros(MAX_LABELS), np.zeros(MAX_LABELS)
    for l in range(n_labels):
        m = lab == l
        cnt[l] = m.sum()
        abs_l[l] = float(np.sum(ae[m]))
        b_abs[l] = float(np.sum(delta[m])) + n * 2.0 ** -52 * abs_l[l]
    return sse, b_sse, abs_l, b_abs, cnt


def _check_sums(sums, y, lab, n_labels, ref, delta, what, summation_only=False):
    """The raw `eval_sums` vector against the reference sums.  `summation_only`: `ref` is what `predict` returned for
    the same pairs (the same bits as inside the reduction), so only the n 2^-52 summation term is allowed and the
    host sums are exact (`math.fsum`) sums of the rounded terms."""
    from pmf_hip import MAX_LABELS
    n = len(y)
    if summation_only:
        e = y - ref
        sse, abs_l, b_abs, cnt = math.fsum(e * e), np.zeros(MAX_LABELS), np.zeros(MAX_LABELS), np.zeros(MAX_LABELS)
        b_sse = n * 2.0 ** -52 * sse
        for l in range(n_labels):
            m = lab == l
            cnt[l], abs_l[l] = m.sum(), math.fsum(np.abs(e[m]))
            b_abs[l] = n * 2.0 ** -52 * abs_l[l]
    else:
        sse, b_sse, abs_l, b_abs, cnt = _sum_reference(y, lab, n_labels, ref, delta)
    got_abs, got_cnt = sums[2:2 + MAX_LABELS], sums[2 + MAX_LABELS:]
    d_abs = np.abs(got_abs - abs_l)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.max(np.where(b_abs > 0, d_abs / b_abs, 0.0))
    print(f"{what}: n={n} |sse-ref|/bound = {abs(sums[1] - sse) / b_sse if b_sse else 0.0:.3f}, "
          f"max_l |abs_l-ref|/bound = {worst:.3f}")
    assert sums.shape == (2 + 2 * MAX_LABELS,)
    assert sums[0] == n, what
    assert np.array_equal(got_cnt, cnt), (what, got_cnt, cnt)
    assert abs(sums[1] - sse) <= b_sse, (what, sums[1], sse, b_sse)
    assert (d_abs <= b_abs).all(), (what, got_abs, abs_l, b_abs)       # b_abs = 0 for an empty class: its sum is 0
    return sse, b_sse, abs_l, b_abs, cnt


def _check_eval(ctx, tabs, u, i, y, flag, offset, what, labels=None):
    """`eval_set` + `eval_sums` on (u, i, y): the whole vector against the reference (derived bounds) and against
    host sums of `predict` on the same pairs (summation term only); two runs bit-identical; the final figures against
    metrics.rmse / metrics.macro_mae of the reference predictions.  Returns the sums."""
    from src.evaluation.metrics import macro_mae, rmse
    y = np.asarray(y, np.float64)
    assert ctx.eval_set(u, i, y, labels=labels) is True
    values = np.unique(y) if labels is None else np.asarray(labels, np.float64)
    lab = np.searchsorted(values, y)
    sums = ctx.eval_sums(flag, offset)
    assert np.array_equal(sums, ctx.eval_sums(flag, offset)), f"{what}: two runs differ"
    ref, delta = _Ref(ctx, tabs, u, i).at(flag, offset)
    sse, b_sse, abs_l, b_abs, cnt = _check_sums(sums, y, lab, len(values), ref, delta, what)
    _check_sums(sums, y, lab, len(values), ctx.predict(u, i, flag, offset), None, what + " [vs predict]", summation_only=True)
    # the final figures: empty classes are skipped, the bounds go through the square root and the ratios
    got_rmse, got_mae = ctx.metrics_from_sums(sums)
    assert (got_rmse, got_mae) == ctx.eval_run(flag, offset)
    ref64 = ref.astype(np.float64)
    want_rmse, want_mae = float(rmse(y, ref64)), float(macro_mae(y, ref64))
    seen = cnt > 0
    b_rmse = b_sse / len(y) / want_rmse + 8 * 2.0 ** -53 * want_rmse if want_rmse > 0 else 0.0
    b_mae = float(np.mean(b_abs[seen] / cnt[seen])) + 8 * 2.0 ** -53 * want_mae
    assert abs(got_rmse - want_rmse) <= b_rmse, (what, got_rmse, want_rmse, b_rmse)
    assert abs(got_mae - want_mae) <= b_mae, (what, got_mae, want_mae, b_mae)
    return sums


def _bad_ids(rng, u, i, U, I, where):
    """Ids one past the tables and int32 max at the positions `where` (users, items, or both): they predict `offset`."""
    where = np.asarray(where)
    kinds = rng.integers(0, 5, len(where))
    u[where[kinds == 0]] = U
    i[where[kinds == 1]] = I
    u[where[kinds == 2]] = INT32_MAX
    i[where[kinds == 3]] = INT32_MAX
    u[where[kinds == 4]], i[where[kinds == 4]] = U, INT32_MAX
    return where


# ---- 1. predict: lane-group dispatch x grid-stride rounds ---------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K", sorted(set(LANE_KS) | set(ALL_FLAG_KS)))
def test_predict_every_lane_group_width_and_three_grid_rounds(K, dtype):
    """n = 2 * 8192 * G + 37 pairs: the grid is capped at 8192 blocks of G pairs, so every block runs three grid-stride
    rounds and the last one is ragged (37 pairs).  K sweeps the lane-group widths L = 4 .. 64 (DPP up to 16,
    `__shfl_xor` above; K > 128: one wavefront per pair).  Ids equal to n_users / n_items / int32 max, also inside the
    ragged tail, return exactly `offset`."""
    import pmf_hip
    rng = np.random.default_rng(1000 + K)
    U, I, offset = 311, 457, 3.625
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        tabs = _fill(ctx, rng)
        n = 2 * 8192 * _groups(ctx) + 37
        u, i = rng.integers(0, U, n), rng.integers(0, I, n)
        bad = _bad_ids(rng, u, i, U, I, np.concatenate([rng.choice(n - 37, 60, replace=False), [n - 30, n - 2]]))
        ref = _Ref(ctx, tabs, u, i)
        assert not ref.ok[bad].any() and ref.ok.sum() == n - len(bad)
        for flag in _flags(K):
            got = ctx.predict(u, i, flag, offset)
            want, delta = ref.at(flag, offset)
            assert (got[bad] == offset).all()
            _check_pairs(got, want, delta, f"predict K={K} {dtype} flag={flag}")


# ---- 2. ids below zero reach the kernels only through the C ABI ----------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_negative_ids_through_the_raw_abi_give_offset(dtype):
    """`Context._clip_ids` remaps negative ids before the library sees them, so the kernels' `u >= 0 && i >= 0` guard
    is reached through the C ABI only.  include/pmf_hip.h: "for ids inside the trained dimensions, 0 otherwise" -- a
    negative id predicts exactly `offset` (and a validation pair with one has error y - offset).  NumPy's wrap-around
    for negative indices (what the reference's fancy indexing would do with them) is deliberately NOT reproduced.
    Nothing else moves: every other pair equals, bit for bit, what `Context.predict` returns, and the doubles behind
    out[n - 1] keep their value."""
    import pmf_hip
    from pmf_hip import ptr
    rng = np.random.default_rng(7)
    U, I, K, n, offset, flag = 300, 200, 20, 5003, -1.25, 3
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        tabs = _fill(ctx, rng)
        u, i = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
        neg = rng.choice(n - 1, 90, replace=False)
        u[neg[:30]] = rng.choice([-1, -2, -U, INT32_MIN], 30)                     # user below zero, item valid
        i[neg[30:60]] = rng.choice([-1, -3, -I, INT32_MIN], 30)                   # item below zero, user valid
        u[neg[60:]], i[neg[60:]] = -1, rng.choice([-1, INT32_MIN, I], 30)         # both outside
        u[n - 1], i[0] = -1, -1
        neg = np.unique(np.concatenate([neg, [n - 1, 0]]))
        out = np.full(n + 16, 777.0)
        rc = ctx._lib.pmf_predict(ctx._h, n, ptr(u, C.c_int32), ptr(i, C.c_int32), flag, offset, ptr(out, C.c_double))
        assert rc == 0
        assert (out[neg] == offset).all()
        assert (out[n:] == 777.0).all()
        assert np.array_equal(out[:n], ctx.predict(u, i, flag, offset))           # (the wrapper clips them to int32 max)
        ref = _Ref(ctx, tabs, u, i)
        assert ref.ok.sum() == n - len(neg)
        want, delta = ref.at(flag, offset)
        _check_pairs(out[:n], want, delta, f"raw predict {dtype}")
        # the same ids as a validation set
        y = rng.choice(RATINGS, n, p=RATING_P)
        lab = np.searchsorted(RATINGS, y).astype(np.int32)
        rc = ctx._lib.pmf_eval_set(ctx._h, n, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(y, C.c_double), ptr(lab, C.c_int32), 5)
        assert rc == 0
        ctx._eval_n = n                                       # what Context.eval_set notes for eval_sums' first entry
        sums = ctx.eval_sums(flag, offset)
        _check_sums(sums, y, lab, 5, want, delta, f"raw eval {dtype}")
        _check_sums(sums, y, lab, 5, out[:n], None, f"raw eval {dtype} [vs predict]", summation_only=True)


# ---- 3. predict: staging rounds of 4 Mi pairs ---------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", [(8, "f32"), (20, "f64")])
def test_predict_staging_rounds_cover_the_whole_output(K, dtype):
    """`pmf_predict` stages 4 Mi pairs per round and writes each round at its own place of the output: exactly one
    round, a second round of 4099 pairs, and a third round of one pair.  The whole output is compared; the profiler's
    launch count of the predict kernel class says the rounds ran (1, 2, 3), and one `eval_sums` is one eval launch."""
    import pmf_hip
    rng = np.random.default_rng(K)
    U, I, offset, flag, step = 800, 900, 0.5, 3, 4 << 20
    sizes = (step, step + 4099, 2 * step + 1)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        tabs = _fill(ctx, rng)
        n = sizes[-1]
        u, i = rng.integers(0, U, n), rng.integers(0, I, n)       # the smaller cases are prefixes
        bad = _bad_ids(rng, u, i, U, I, np.concatenate([rng.choice(n, 40, replace=False),
                                                        [0, step - 1, step, step + 4098, 2 * step - 1, 2 * step]]))
        ref = _Ref(ctx, tabs, u, i)
        assert not ref.ok[bad].any()
        want, delta = ref.at(flag, offset)
        ctx.prof_enable(True)
        for rounds, m in enumerate(sizes, start=1):
            ctx.prof_reset()
            got = ctx.predict(u[:m], i[:m], flag, offset)
            prof = ctx.prof_get()
            assert prof["predict"][1] == rounds and prof["eval"][1] == 0
            assert got.shape == (m,)
            _check_pairs(got, want[:m], delta[:m], f"predict n={m} K={K} {dtype}")
        m = 100_003
        y = rng.choice(RATINGS, m, p=RATING_P)
        assert ctx.eval_set(u[:m], i[:m], y)
        for _ in range(2):
            ctx.prof_reset()
            sums = ctx.eval_sums(flag, offset)
            prof = ctx.prof_get()
            assert prof["eval"][1] == 1 and prof["predict"][1] == 0
        _check_sums(sums, y, np.searchsorted(RATINGS, y), 5, want[:m], delta[:m], f"eval n={m} K={K} {dtype}")


# ---- 4. the fused reduction over the same K x dtype grid ----------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K", sorted(set(LANE_KS) | set(ALL_FLAG_KS)))
def test_eval_sums_every_lane_group_width_and_three_grid_rounds(K, dtype):
    """n = 2 * 1024 * G + 37: the eval grid is capped at 1024 blocks, so three grid-stride rounds with a ragged last
    one.  Five skewed ratings plus a sixth that occurs exactly once, at the last index (inside the ragged tail): its
    class must report count 1 and that pair's |error|."""
    import pmf_hip
    rng = np.random.default_rng(2000 + K)
    U, I, offset = 257, 389, 3.625
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        tabs = _fill(ctx, rng)
        n = 2 * 1024 * _groups(ctx) + 37
        u, i = rng.integers(0, U, n), rng.integers(0, I, n)
        _bad_ids(rng, u, i, U, I, np.concatenate([rng.choice(n - 37, 20, replace=False), [n - 20]]))
        y = rng.choice(RATINGS, n, p=RATING_P)
        y[n - 1] = 2.5
        assert (y == 2.5).sum() == 1 and len(np.unique(y)) == 6
        for flag in _flags(K):
            sums = _check_eval(ctx, tabs, u, i, y, flag, offset, f"eval K={K} {dtype} flag={flag}")
            assert sums[2 + 32 + 2] == 1                                   # 2.5 is the third of the sorted labels


# ---- 5. edges of the reduction --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K", [16, 200])
def test_eval_edges_tiny_sets_label_sets_and_bad_ids(K, dtype):
    """Fewer pairs than one block holds, exactly one block, one more; one label and the maximum of 32; a fixed
    `labels=` set with classes that never occur (what the sharded monitor passes: count 0, sum 0, skipped by
    `metrics_from_sums`); pairs with ids outside the tables (error y - offset); and what is refused: 33 distinct values
    (`eval_set` returns False), n_labels = 33 and a label index equal to n_labels through the C ABI (PMF_ERANGE)."""
    import pmf_hip
    from pmf_hip import MAX_LABELS, ptr
    rng = np.random.default_rng(3000 + K)
    U, I, offset, flag = 97, 131, 2.0, 3
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        tabs = _fill(ctx, rng)
        G = _groups(ctx)
        assert G == (64 if K == 16 else 4)
        fixed = 0.5 * np.arange(MAX_LABELS)                 # 32 labels
        for n in sorted({1, 3, G - 1, G, G + 1, 1000}):
            u, i = rng.integers(0, U, n), rng.integers(0, I, n)
            tag = f"eval edge n={n} K={K} {dtype}"
            # one label
            sums = _check_eval(ctx, tabs, u, i, np.full(n, 4.0), flag, offset, tag + " one label")
            assert sums[2 + MAX_LABELS] == n and not sums[3 + MAX_LABELS:].any() and not sums[3:2 + MAX_LABELS].any()
            # 32 classes, most of them (all but at most n) empty: labels 3, 10, 11, 31 never occur
            present = np.setdiff1d(np.arange(MAX_LABELS), [3, 10, 11, 31])
            y = fixed[rng.choice(present, n)]
            y[n - 1] = fixed[30]
            sums = _check_eval(ctx, tabs, u, i, y, flag, offset, tag + " fixed labels", labels=fixed)
            for l in (3, 10, 11, 31):
                assert sums[2 + l] == 0.0 and sums[2 + MAX_LABELS + l] == 0.0
            # ids outside the tables: at the first and the last pair (and a few between)
            where = np.unique(np.concatenate([[0, n - 1], rng.choice(n, min(n, 5), replace=False)]))
            _bad_ids(rng, u, i, U, I, where)
            _check_eval(ctx, tabs, u, i, y, 1, offset, tag + " bad ids", labels=fixed)
        # all 32 classes present
        n = 1000
        u, i = rng.integers(0, U, n), rng.integers(0, I, n)
        y = fixed[rng.permutation(np.arange(n) % MAX_LABELS)]
        sums = _check_eval(ctx, tabs, u, i, y, flag, offset, f"eval 32 labels K={K} {dtype}")
        assert (sums[2 + MAX_LABELS:] >= 31).all()
        # 33 distinct values: refused, the caller falls back to predict
        assert ctx.eval_set(u, i, 0.25 * (np.arange(n) % 33)) is False
        assert ctx.eval_set(u, i, y, labels=0.5 * np.arange(33)) is False
        u32, i32 = u.astype(np.int32), i.astype(np.int32)
        lab = (np.arange(n) % MAX_LABELS).astype(np.int32)
        args = (ctx._h, n, ptr(u32, C.c_int32), ptr(i32, C.c_int32), ptr(y, C.c_double))
        assert ctx._lib.pmf_eval_set(*args, ptr(lab, C.c_int32), MAX_LABELS + 1) == PMF_ERANGE
        lab[n - 1] = 7                                        # an index equal to n_labels
        assert ctx._lib.pmf_eval_set(*args, ptr(lab, C.c_int32), 7) == PMF_ERANGE
        lab[n - 1] = -1
        assert ctx._lib.pmf_eval_set(*args, ptr(lab, C.c_int32), MAX_LABELS) == PMF_ERANGE


# ---- 6. a new validation set, new tables ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_eval_follows_a_replaced_set_and_replaced_tables(dtype):
    """150k pairs, then 1000 other pairs with another label set: the sums are the second set's alone (no stale pair,
    count or label).  Then new FACTOR tables: the sums follow them (no stale table pointer)."""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(11)
    U, I, K, offset, flag = 400, 500, 20, 3.5, 1
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        tabs = _fill(ctx, rng)
        n = 150_000
        u, i = rng.integers(0, U, n), rng.integers(0, I, n)
        big = _check_eval(ctx, tabs, u, i, rng.choice(RATINGS, n, p=RATING_P), flag, offset, f"eval 150k {dtype}")
        n = 1000
        u, i = rng.integers(0, U, n), rng.integers(0, I, n)
        y = rng.choice([0.5, 1.5, 7.0], n)
        small = _check_eval(ctx, tabs, u, i, y, flag, offset, f"eval 1000 after 150k {dtype}")
        assert small[0] == n and small[2 + 32:].sum() == n and big[2 + 32:].sum() == 150_000
        ctx.set_array(USER, ARR_FACTOR, rng.standard_normal((U, K)))
        ctx.set_array(ITEM, ARR_FACTOR, rng.standard_normal((I, K)))
        tabs["fu"], tabs["fi"] = ctx.get_array(USER, ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
        ref, delta = _Ref(ctx, tabs, u, i).at(flag, offset)
        sums = ctx.eval_sums(flag, offset)                    # the stored set, the new tables
        _check_sums(sums, y, np.searchsorted([0.5, 1.5, 7.0], y), 3, ref, delta, f"eval after set_array {dtype}")
        assert sums[1] != small[1]


# ---- 7. the models' validation monitor: fused path and host fallback ------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_model_monitor_fused_and_fallback_agree_with_host_metrics(dtype):
    """`_monitor_setup` evaluates through device predict + host metrics when the validation ratings have more than 32
    distinct values, through the fused reduction otherwise.  Both must report what metrics.rmse / metrics.macro_mae
    give for `model.predict` on that frame after the final iteration (the last history entry).

    Fallback: the same host computation on the same predictions, rel 1e-12.  Fused: the reference here is
    `model.predict`, i.e. the bits the reduction saw, so of the case-4 bounds only the summation term is left:
    sse and every abs_l are within n 2^-52 relative, hence rmse within n 2^-53 and macro-MAE within n 2^-52 relative;
    (n + 8) 2^-52 is asserted for both (8: the handful of roundings of the host's own mean / sqrt / divisions)."""
    import pandas as pd
    from helpers import skewed_problem
    from src.evaluation.metrics import macro_mae, rmse
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    u, i, x = skewed_problem(5, 300, 50, 6000, rating_kind="centered")
    rng = np.random.default_rng(1)
    is_val = rng.random(len(u)) < 0.15
    is_val[0] = False
    gm = 3.75
    train = pd.DataFrame({"u": u[~is_val], "i": i[~is_val], "rating": x[~is_val]})
    vu, vi = np.append(u[is_val], 305), np.append(i[is_val], 3)            # one pair with an unseen user: dropped
    smooth = np.round(rng.normal(0.0, 1.5, len(vu)), 2)                    # well over 32 distinct values
    coarse = np.clip(np.round(smooth), -2, 2)                              # 5 values
    assert len(np.unique(smooth)) >= 40 and len(np.unique(coarse)) == 5
    keep = vu < 300
    cfg = GaussianMFCAVIConfig(n_factors=12, sigma2=0.3, eta_theta2=0.5, eta_beta2=0.5, eta_bias2=1.0, max_iter=2,
                               tol=-1.0, random_state=3, verbose=False)
    for name, rating in (("fallback", smooth), ("fused", coarse)):
        model = GaussianMFCAVI(cfg, dtype=dtype)
        model.fit(train, pd.DataFrame({"u": vu, "i": vi, "rating": rating}), global_mean=gm)
        try:
            assert model.history_["iterations"] == 2 and len(model.history_["val_rmse"]) == 2
            y = rating[keep] + gm
            pred = model.predict(vu[keep], vi[keep], gm)
            want = float(rmse(y, pred)), float(macro_mae(y, pred))
            got = model.history_["val_rmse"][-1], model.history_["val_macro_mae"][-1]
            rel = 1e-12 if name == "fallback" else (keep.sum() + 8) * 2.0 ** -52
            print(f"monitor {name} {dtype}: got {got}, host {want}, rel bound {rel:.3e}")
            assert got[0] == pytest.approx(want[0], rel=rel, abs=0) and got[1] == pytest.approx(want[1], rel=rel, abs=0)
            # (a context remembers the size of a stored validation set: only the fused path stores one)
            assert hasattr(model._ctx, "_eval_n") == (name == "fused")
        finally:
            model.close()
