"""Posterior draws on the device (`pmf_gauss_sample_rows`) against float64 NumPy (tests/gauss_sample_reference.py).

State: covariances V = S R S with R = Q diag(lambda) Q', lambda log-spaced over [1e-3, 1] (condition 1e3) and S =
diag(10^s), s uniform in [-1.5, 1.5], so that the diagonals spread over 1e-3 .. 1e3 and the Jacobi scaling matters; means
m_j = nu_j sqrt(V_jj) with nu uniform in [-1, 1].  V and m below are ALWAYS the state read back from the context (what the
kernels read), not the float64 input.  eps = machine epsilon of the context's dtype.

Check 1 bound.  With unit vectors for z, draw k minus m is column k of the computed factor Ct.  The claim is
    |Ct Ct' - V|_ij <= c (K + 1) eps sqrt(V_ii V_jj),      c = 3 + 8 / (K + 1).
Higham (Accuracy and Stability of Numerical Algorithms, Thm 10.3) gives |C C' - A|_ij <= gamma_{K+1} (|C||C'|)_ij for
Cholesky, and (|C||C'|)_ij <= sqrt(A_ii A_jj) by Cauchy-Schwarz; neither depends on the condition number.  The kernels
differ from textbook Cholesky by roundings that are counted here, each as a multiple of eps sqrt(V_ii V_jj):
  (K + 1)  the theorem itself;
  (K + 1)  every multiplier of the elimination is v * fl(1 / d), two roundings where the theorem's division has one: one
           more per term of the at most K + 1 terms of an entry;
  (K + 1)  the test forms Ct = out - m from out = fl(m + x): |delta Ct_jk| <= eps |out_j| / 2, so the product moves by at
           most eps sqrt(K) (|m_i| sqrt(V_jj) + |m_j| sqrt(V_ii)) <= 2 sqrt(K) eps sqrt(V_ii V_jj) as |m_j| <= sqrt(V_jj),
           and 2 sqrt(K) <= K + 1;
  2        the scaled matrix is fl(fl(V_ij g_j) g_i): two roundings (the roundings INSIDE g = fl(1 / fl(sqrt V_jj)) cancel,
           the same g unscales the result);
  2        x_j = fl(acc_j / g_j): one rounding in each factor of the product;
  4        a column is v * fl(1 / fl(sqrt d)), three roundings where Cholesky's sqrt and division have two for an entry
           below the diagonal and one on it: at most two more in each factor.
Sum: (3 (K + 1) + 8) eps sqrt(V_ii V_jj).

Check 2 bound (the issue's): |out - (m + Ct z)|_j <= (K + 2) eps (|m_j| + sum_k |Ct_jk| |z_k|) for supplied z with
|z_k| <= 1, Ct from check 1 -- K fused multiply-adds, the division, the addition, and the rounding of Ct itself."""
import ctypes as C

import numpy as np
import pytest

import gauss_sample_reference as ref

pytestmark = pytest.mark.gpu

U, I = 12, 7             # rows per side: more than two blocks of four wavefronts on the user side


def _spd(rng, n, K):
    V = np.empty((n, K, K))
    for r in range(n):
        Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
        lam = np.logspace(0.0, -3.0, K) if K > 1 else np.ones(1)
        s = 10.0 ** rng.uniform(-1.5, 1.5, K)
        R = (Q * lam) @ Q.T
        V[r] = s[:, None] * (0.5 * (R + R.T)) * s[None, :]
    return V


_CTX = {}


def _context(K, dtype):
    """One context per (K, dtype) for the whole module; the tests only read it (test 5 restores what it changes)."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    if (K, dtype) not in _CTX:
        rng = np.random.default_rng(1000 * K + (dtype == "f64"))
        n_u = 3 if K == 200 else U
        ctx = pmf_hip.Context(n_u, I, K, dtype=dtype)
        for side, n in ((USER, n_u), (ITEM, I)):
            V = _spd(rng, n, K)
            ctx.set_array(side, ARR_COV, V)
            ctx.set_array(side, ARR_FACTOR, rng.uniform(-1.0, 1.0, (n, K)) * np.sqrt(np.einsum("nkk->nk", V)))
        _CTX[(K, dtype)] = ctx
    return _CTX[(K, dtype)]


def _state(ctx, side, rows):
    from pmf_hip import ARR_COV, ARR_FACTOR
    return ctx.get_array_rows(side, ARR_FACTOR, rows), ctx.get_array_rows(side, ARR_COV, rows)


def _eps(ctx):
    return float(np.finfo(ctx.np_dtype).eps)


def _factor(ctx, side, rows):
    """Ct [n, K, K] (lower triangular) from K draws on unit vectors, and the rows' m"""
    K = ctx.K
    m, _ = _state(ctx, side, rows)
    out = ctx.gauss_sample_rows(side, rows, K, z=np.broadcast_to(np.eye(K), (len(rows), K, K)))
    return (out - m[:, None, :]).transpose(0, 2, 1), m


SHAPES = [(K, "f32") for K in (1, 3, 8, 9, 16, 17, 33, 64, 65, 72, 130)] + [(64, "f64"), (200, "f64")]


def _rows(ctx, side, n):
    """n unsorted ids of the side with a repeat (n >= 4)"""
    from pmf_hip import USER
    r = np.random.default_rng(n).permutation(ctx.n_users if side == USER else ctx.n_items)[:n]
    if n >= 4:
        r[-1] = r[1]
    return r


@pytest.mark.parametrize("K,dtype", SHAPES)
def test_factor_from_unit_vectors_and_linearity(K, dtype):
    from pmf_hip import ITEM, USER
    ctx = _context(K, dtype)
    eps, c = _eps(ctx), 3.0 + 8.0 / (K + 1)
    rng = np.random.default_rng(K)
    counts = (1, 3) if K == 200 else (1, 4, 5, 9)
    for side, n in [(USER, n) for n in counts] + [(ITEM, 5 if K != 200 else 3)]:
        rows = _rows(ctx, side, n)
        Ct, m = _factor(ctx, side, rows)
        _, V = _state(ctx, side, rows)
        assert (np.triu(Ct, 1) == 0.0).all(), "entries above the diagonal"
        d = np.sqrt(np.einsum("nkk->nk", V))
        err = np.abs(Ct @ Ct.transpose(0, 2, 1) - V) / (d[:, :, None] * d[:, None, :])
        print(f"K={K} {dtype} side={side} n={n}: factor error {err.max() / ((K + 1) * eps):.3f} (K+1) eps, bound c = {c:.2f}")
        assert err.max() <= c * (K + 1) * eps
        # linearity on supplied z (rounded to the dtype beforehand: the call's conversion is then exact)
        for nd in (1, 8, 9):
            z = rng.uniform(-1.0, 1.0, (n, nd, K)).astype(ctx.np_dtype).astype(np.float64)
            out = ctx.gauss_sample_rows(side, rows, nd, z=z)
            want = m[:, None, :] + np.einsum("njk,ndk->ndj", Ct, z)
            bound = (K + 2) * eps * (np.abs(m)[:, None, :] + np.einsum("njk,ndk->ndj", np.abs(Ct), np.abs(z)))
            assert (np.abs(out - want) <= bound).all(), (nd, float((np.abs(out - want) / bound).max()))


@pytest.mark.parametrize("K,dtype", [(3, "f32"), (64, "f32"), (65, "f32"), (64, "f64"), (130, "f64")])
def test_stream_equals_the_host_reference(K, dtype):
    """Rows with V = I and m = 0 return z itself (every operation on them is exact): both sides, a seed below and one
    above 2^32 (the key's high word), draw indices away from 0.  f32: within one f32 ulp of the float64 reference rounded
    to f32 -- device and host libm differ by ulps of double, which moves the rounded value by at most one ulp; f64: 1e-13."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    with pmf_hip.Context(9, 6, K, dtype=dtype) as ctx:
        for side, n in ((USER, 9), (ITEM, 6)):
            ctx.set_cov_identity(side, 1.0)
            ctx.set_array(side, ARR_FACTOR, np.zeros((n, K)))
        for seed in (7, (0x9E3779B9 << 32) | 12345):
            for side, rows in ((USER, np.array([8, 0, 3, 3, 5])), (ITEM, np.array([5, 2]))):
                got = ctx.gauss_sample_rows(side, rows, 9, draw0=3, seed=seed)
                want = ref.normals(seed, side, rows, 3 + np.arange(9), K)
                assert got.shape == want.shape == (len(rows), 9, K) and np.isfinite(got).all()
                if dtype == "f32":
                    w32 = want.astype(np.float32)
                    assert (np.abs(got - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64)).all()
                    print(f"K={K} seed={seed:#x} side={side}: {np.mean(got != w32.astype(np.float64)):.4f} of the values differ by an ulp")
                else:
                    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("K,dtype", [(9, "f32"), (64, "f32"), (72, "f32"), (64, "f64"), (200, "f64")])
def test_draws_do_not_depend_on_the_shape_of_the_call(K, dtype):
    from pmf_hip import ITEM, USER
    ctx = _context(K, dtype)
    n_u = ctx.n_users
    batch = np.array([2, 0, 1, 2, 1, 0, 2, 2, 1]) if n_u < 9 else np.array([7, 5, 0, 11, 5, 3, 9, 1, 5])
    row = int(batch[1])
    seed = 2024
    full = ctx.gauss_sample_rows(USER, batch, 9, draw0=0, seed=seed)
    assert np.isfinite(full).all()
    alone = ctx.gauss_sample_rows(USER, [row], 9, draw0=0, seed=seed)
    np.testing.assert_array_equal(alone[0], full[1])                              # alone or in a batch of 9
    for q in np.flatnonzero(batch == row):
        np.testing.assert_array_equal(full[q], full[1])                           # repeated in the batch
    np.testing.assert_array_equal(ctx.gauss_sample_rows(USER, [row], 1, draw0=8, seed=seed)[0, 0], full[1, 8])   # draw index, not position
    np.testing.assert_array_equal(ctx.gauss_sample_rows(USER, batch, 1, draw0=8, seed=seed)[:, 0], full[:, 8])
    np.testing.assert_array_equal(ctx.gauss_sample_rows(USER, batch, 9, draw0=0, seed=seed), full)                # a second call
    assert (full[:, 0] != full[:, 1]).any() and (ctx.gauss_sample_rows(USER, batch, 9, seed=seed + 1) != full).any()
    # user row and item row of one id: the side is part of the counter.  Compare the normals, not the draws: z = Ct^-1 (x - m)
    r = min(5, n_u - 1)
    zs = []
    for side in (USER, ITEM):
        Ct, m = _factor(ctx, side, [r])
        x = ctx.gauss_sample_rows(side, [r], 1, seed=seed)[0, 0]
        zs.append(np.linalg.solve(Ct[0], x - m[0]))
    assert np.abs(zs[0] - zs[1]).max() > 1e-3


@pytest.mark.parametrize("K,dtype", [(1, "f32"), (9, "f32"), (64, "f32"), (72, "f32"), (64, "f64")])
def test_a_row_that_is_not_positive_definite_gives_nan_and_nothing_else(K, dtype):
    """Documented input, not a fault: the row's pivots go negative (or its scale is NaN), its draws are NaN in every
    element, and the rows beside it in the block are what they are without it."""
    from pmf_hip import ARR_COV, USER
    ctx = _context(K, dtype)
    bad = 6
    keep = ctx.get_array_rows(USER, ARR_COV, [bad])
    try:
        lam, Q = np.linalg.eigh(keep[0])
        lam[0 if K == 1 else K // 2] *= -1.0
        ctx.set_array_rows(USER, ARR_COV, [bad], ((Q * lam) @ Q.T)[None])
        for nd in (1, 9):
            with_bad = ctx.gauss_sample_rows(USER, [4, bad, 5, 7], nd, seed=3)
            without = ctx.gauss_sample_rows(USER, [4, 5, 7], nd, seed=3)
            assert np.isnan(with_bad[1]).all()
            np.testing.assert_array_equal(with_bad[[0, 2, 3]], without)
            assert np.isfinite(without).all()
    finally:
        ctx.set_array_rows(USER, ARR_COV, [bad], keep)
    np.testing.assert_array_equal(ctx.get_array_rows(USER, ARR_COV, [bad]), keep)


def _raw(ctx, side, n, ids, n_draws, draw0, z, out):
    lib = ctx._lib
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    rc = lib.pmf_gauss_sample_rows(ctx._h, side, n, p(ids, C.c_int32), n_draws, draw0, C.c_uint64(1), p(z, C.c_double), p(out, C.c_double))
    return rc, lib.pmf_last_error().decode()


def test_argument_errors_name_the_fault_and_write_nothing():
    import pmf_hip
    from pmf_hip import ARR_FACTOR, USER
    ctx = _context(9, "f32")
    ids = np.array([1, 0, 11], dtype=np.int32)
    sentinel = -7.25
    out = np.full((3, 2, 9), sentinel)
    cases = [
        ((USER, 3, None, 2, 0, None, out), -1, "null row_ids"),
        ((USER, 3, ids, 2, 0, None, None), -1, "null out"),
        ((2, 3, ids, 2, 0, None, out), -1, "bad side 2"),
        ((-1, 3, ids, 2, 0, None, out), -1, "bad side -1"),
        ((USER, -1, ids, 2, 0, None, out), -1, "negative n_rows"),
        ((USER, 3, ids, 0, 0, None, out), -1, "n_draws=0"),
        ((USER, 3, ids, 2, -1, None, out), -1, "negative draw0 -1"),
        ((USER, 3, np.array([1, 12, 13], dtype=np.int32), 2, 0, None, out), -4, "row id 12 at position 1 outside [0, 12)"),
        ((USER, 3, np.array([1, 2, -1], dtype=np.int32), 2, 0, None, out), -4, "row id -1 at position 2 outside [0, 12)"),
    ]
    for args, status, text in cases:
        rc, msg = _raw(ctx, *args)
        assert rc == status and msg.startswith("pmf_gauss_sample_rows: ") and text in msg, (args[:2], rc, msg)
        assert (out == sentinel).all()
    lib = ctx._lib
    assert lib.pmf_gauss_sample_rows(None, USER, 3, None, 1, 0, C.c_uint64(0), None, None) == -1
    assert "null context" in lib.pmf_last_error().decode()
    # no rows: nothing is touched, whatever else is passed
    assert _raw(ctx, USER, 0, None, 0, -1, None, None)[0] == 0
    assert ctx.gauss_sample_rows(USER, [], 3).shape == (0, 3, 9)
    # a context without covariances -- every count-model context -- is refused by name
    with pmf_hip.Context(5, 4, 9) as poisson:
        poisson.set_array(USER, ARR_FACTOR, np.ones((5, 9)))
        rc, msg = _raw(poisson, USER, 3, np.array([0, 1, 2], dtype=np.int32), 2, 0, None, out)
        assert rc == -1 and "pmf_gauss_sample_rows" in msg and "COV" in msg.upper(), msg
        assert (out == sentinel).all()
    with pmf_hip.Context(5, 4, 9) as empty:
        rc, msg = _raw(empty, USER, 3, np.array([0, 1, 2], dtype=np.int32), 2, 0, None, out)
        assert rc == -1 and "pmf_gauss_sample_rows" in msg, msg
    with pytest.raises(ValueError, match="z: expected shape"):
        ctx.gauss_sample_rows(USER, [0, 1], 2, z=np.zeros((2, 3, 9)))
    with pytest.raises(pmf_hip.PmfError, match="n_draws=0"):
        ctx.gauss_sample_rows(USER, [0, 1], 0)


def test_many_rounds_give_the_bits_of_one(monkeypatch):
    """PMF_STAGE_BYTES small enough for one row per round (and for pinned steps inside the download): the same bits, with
    and without supplied z."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, USER
    big = _context(17, "f32")
    rows = np.array([3, 9, 3, 0, 11, 7, 2])
    z = np.random.default_rng(5).uniform(-1, 1, (len(rows), 9, 17))
    want = big.gauss_sample_rows(USER, rows, 9, seed=11), big.gauss_sample_rows(USER, rows, 9, z=z)
    monkeypatch.setenv("PMF_STAGE_BYTES", "700")          # one row of 9 draws is 9 * 20 * 4 = 720 bytes
    with pmf_hip.Context(big.n_users, big.n_items, 17, dtype="f32") as small:
        small.set_array(USER, ARR_COV, big.get_array(USER, ARR_COV))
        small.set_array(USER, ARR_FACTOR, big.get_array(USER, ARR_FACTOR))
        np.testing.assert_array_equal(small.gauss_sample_rows(USER, rows, 9, seed=11), want[0])
        np.testing.assert_array_equal(small.gauss_sample_rows(USER, rows, 9, z=z), want[1])


def test_the_call_only_reads_the_context():
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    ctx = _context(33, "f32")
    before = [ctx.get_array(s, a) for s in (USER, ITEM) for a in (ARR_FACTOR, ARR_COV)]
    ctx.gauss_sample_rows(USER, np.arange(12), 9, seed=1)
    ctx.gauss_sample_rows(ITEM, np.arange(7), 2, seed=1)
    for b, a in zip(before, [ctx.get_array(s, a) for s in (USER, ITEM) for a in (ARR_FACTOR, ARR_COV)]):
        np.testing.assert_array_equal(a, b)


def _swept_context(K, dtype):
    """64 x 64 rows, random means, identity covariances, then one user and one item sweep on 300 ratings"""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(K)
    ctx = pmf_hip.Context(64, 64, K, dtype=dtype)
    cells = rng.choice(64 * 64, 300, replace=False)
    ctx.set_ratings((cells // 64).astype(np.int32), (cells % 64).astype(np.int32), rng.standard_normal(300))
    for side in (USER, ITEM):
        ctx.set_array(side, ARR_FACTOR, 0.3 * rng.standard_normal((64, K)))
        ctx.set_cov_identity(side, 0.5)
    for side in (USER, ITEM):
        ctx.gauss_factor_sweep(side, 0.4, 0.7)
    return ctx


def _row_results(ctx):
    from pmf_hip import USER
    _, per_row = ctx.gauss_elbo_terms(USER, with_data=False, per_row=True)
    return per_row, ctx.gauss_sample_rows(USER, np.arange(3, 64, 8), 2, seed=9)


@pytest.mark.parametrize("dtype,K_a,K_b", [("f32", 200, 72), ("f64", 130, 66)])
def test_two_contexts_share_the_block_per_row_kernels(dtype, K_a, K_b):
    """A (large K, more dynamic LDS than the default) and B (small K) are alive together on one device and launch the same
    block-per-row ELBO and sample functions in the order A, B, A: A's second results are its first bit for bit, and B's are
    those of a context like it that ran alone -- the LDS size a function may use belongs to the process, not to a context."""
    with _swept_context(K_b, dtype) as alone:
        want_b = _row_results(alone)
    with _swept_context(K_a, dtype) as a, _swept_context(K_b, dtype) as b:
        first_a = _row_results(a)
        got_b = _row_results(b)
        again_a = _row_results(a)
    for got, want in zip(got_b + again_a, want_b + first_a):
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got, want)
