"""Thompson-sampled top-k (`pmf_topk_sampled`, `top_k_items(sample_seed=..)`) and the model-level draws on a fitted
GaussianMFCAVI with biases, 300 users x 257 items: K = 16 in f32 (the fused scan), K = 130 in f32 and K = 16 in f64 (the
two-phase path; the f64 model is fitted under PMF_TOPK_QUERY_ROWS=32, so its 300 users go in ten rounds).

Reference: NumPy top-k (tests/query_reference.py: order, ties, exclusion) of  sample_factors(user) @ sample_factors(item)'
+ the mean biases in float64.  Tolerance of a score: f64 sums K products of doubles in another order than NumPy,
f32 sums them in f32, so |score - reference| <= (K + 2) eps (|b_u| + |b_i| + sum_k |theta_k beta_k|), eps of the dtype; the
test takes the largest such magnitude over a row's candidates.  Ids are compared through their scores (a swap inside a
near-tie cannot fail), and exactly where the reference's neighbouring scores are further apart than twice the tolerance."""
import os

import numpy as np
import pandas as pd
import pytest

import query_reference as qr

pytestmark = pytest.mark.gpu

U, I, N = 300, 257, 9000
CONFIGS = {"k16_f32": (16, "f32", None), "k130_f32": (130, "f32", None), "k16_f64": (16, "f64", "32")}
_FITTED = {}


def _frame():
    rng = np.random.default_rng(42)
    u, i = rng.integers(0, U, N), rng.integers(0, I, N)
    u[0], i[0] = U - 1, I - 1
    return pd.DataFrame({"u": u, "i": i, "rating": rng.integers(1, 6, N).astype(float) - 3.0})


def _model(name):
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    if name not in _FITTED:
        K, dtype, round_rows = CONFIGS[name]
        if round_rows:
            os.environ["PMF_TOPK_QUERY_ROWS"] = round_rows
        try:
            cfg = GaussianMFCAVIConfig(n_factors=K, sigma2=0.5, eta_theta2=0.5, eta_beta2=0.5, eta_bias2=1.0, max_iter=2, tol=0.0,
                                       random_state=3, verbose=False)
            df = _frame()
            _FITTED[name] = (GaussianMFCAVI(cfg, dtype=dtype).fit(df, global_mean=0.0), df)
        finally:
            os.environ.pop("PMF_TOPK_QUERY_ROWS", None)
    return _FITTED[name]


def _reference(m, users, seed, draw):
    """(full [n, I] float64 scores of the draw, magnitude [n]: the largest |b_u| + |b_i| + sum |theta beta| of a row)"""
    from pmf_hip import ARR_BIAS, ITEM, USER
    theta = m.sample_factors("user", users, 1, seed, draw0=draw)[:, 0]
    beta = m.sample_factors("item", np.arange(I), 1, seed, draw0=draw)[:, 0]
    bu, bi = m._ctx.get_array_rows(USER, ARR_BIAS, users), m._ctx.get_array(ITEM, ARR_BIAS)
    full = qr.score_matrix(theta, beta, qr.SCORE_BIAS, bu, bi)
    mag = (np.abs(bu)[:, None] + np.abs(bi)[None, :] + np.abs(theta) @ np.abs(beta).T).max(axis=1)
    return full, mag


def _check(full, mag, lists, got, k, K, eps):
    ids, scores = got
    want_ids, want_scores = qr.topk(full, k, lists)
    for q in range(len(full)):
        tol = (K + 2) * eps * mag[q]
        assert (ids[q] >= 0).all() and len(set(ids[q].tolist())) == k
        assert lists is None or not set(ids[q].tolist()) & set(lists[q])
        assert (np.diff(scores[q]) <= 0).all()
        assert np.abs(scores[q] - want_scores[q]).max() <= tol, (q, np.abs(scores[q] - want_scores[q]).max(), tol)
        assert np.abs(scores[q] - full[q][ids[q]]).max() <= tol
        # positions whose reference neighbours (the k + 1st included) are further than 2 tol away must hold the same id
        s = np.sort(np.where(np.isin(np.arange(full.shape[1]), [] if lists is None else list(lists[q])), -np.inf, full[q]))[::-1][:k + 1]
        apart = (s[:k] - s[1:k + 1]) > 2 * tol                      # position p against position p + 1
        clear = apart & np.concatenate([[True], apart[:-1]])
        assert (ids[q][clear] == want_ids[q][clear]).all()


def _train_lists(df, users):
    return [sorted(set(df["i"][df["u"] == u].tolist())) for u in users]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_sampled_topk_equals_numpy_on_the_sampled_rows(name):
    m, df = _model(name)
    K, dtype, _ = CONFIGS[name]
    eps = float(np.finfo(np.float64 if dtype == "f64" else np.float32).eps)
    users = np.concatenate([np.arange(U), [7, 7, 299]])            # every user, and repeated query ids
    k, seed, draw = 10, 77, 4
    full, mag = _reference(m, users, seed, draw)
    assert np.isfinite(full).all()
    _check(full, mag, None, m.top_k_items(users, k=k, sample_seed=seed, draw=draw), k, K, eps)
    lists = _train_lists(df, users)
    assert max(len(v) for v in lists) > 30
    got = m.top_k_items(users, k=k, exclude_train=True, sample_seed=seed, draw=draw)
    _check(full, mag, lists, got, k, K, eps)
    np.testing.assert_array_equal(got[0][7], got[0][U]); np.testing.assert_array_equal(got[1][7], got[1][U + 1])
    # the binding's own form with lists in any order and with repeats gives the same bytes
    from pmf_hip import ITEM, PREDICT_BIAS, USER
    messy = [list(reversed(v)) + v[:2] for v in lists]
    again = m._ctx.topk_sampled(ITEM, k, users, query_side=USER, score=PREDICT_BIAS, exclude=qr.csr(messy), seed=seed, draw=draw)
    np.testing.assert_array_equal(again[0], got[0]); np.testing.assert_array_equal(again[1], got[1])
    # users as candidates of sampled item rows: the other direction, without biases
    items = np.array([5, 256, 5, 0])
    ids, scores = m._ctx.topk_sampled(USER, 7, items, query_side=ITEM, score=0, seed=seed, draw=draw)
    theta = m.sample_factors("user", np.arange(U), 1, seed, draw0=draw)[:, 0]
    beta = m.sample_factors("item", items, 1, seed, draw0=draw)[:, 0]
    _check(qr.score_matrix(beta, theta), (np.abs(beta) @ np.abs(theta).T).max(axis=1), None, (ids, scores), 7, K, eps)


@pytest.mark.parametrize("name", ["k16_f32", "k16_f64"])
def test_one_seed_repeats_to_the_bit_and_two_seeds_differ(name):
    m, _ = _model(name)
    users = np.arange(0, U, 3)
    a = m.top_k_items(users, k=10, sample_seed=5, draw=1)
    b = m.top_k_items(users, k=10, sample_seed=5, draw=1)
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
    c = m.top_k_items(users, k=10, sample_seed=6, draw=1)
    d = m.top_k_items(users, k=10, sample_seed=5, draw=2)
    assert (a[0] != c[0]).any(axis=1).any() and (a[0] != d[0]).any(axis=1).any()
    assert (a[1] != c[1]).any()


def test_the_sample_table_is_counted_once():
    m, _ = _model("k16_f32")
    m.top_k_items([0], k=3, sample_seed=1)
    before = m._ctx.device_bytes()
    assert before >= I * m._ctx.kpad * 4
    m.top_k_items(np.arange(50), k=3, sample_seed=2, draw=9)
    assert m._ctx.device_bytes() == before


@pytest.mark.parametrize("name", ["k16_f32", "k130_f32"])
def test_a_vanishing_covariance_gives_the_unsampled_lists(name):
    """COV = 1e-12 I on both sides (NOT 0: a zero covariance is not positive definite and every draw is NaN, by the
    documented rule): the draws sit within ~1e-6 |z| of the means, so users whose first k + 1 unsampled scores are
    further than 1e-4 apart keep their lists."""
    from pmf_hip import ARR_COV, ITEM, USER
    m, _ = _model(name)
    ctx, k = m._ctx, 10
    keep = [ctx.get_array(s, ARR_COV) for s in (USER, ITEM)]
    try:
        for s in (USER, ITEM):
            ctx.set_cov_identity(s, 1e-12)
        users = np.arange(U)
        plain_ids, plain_scores = m.top_k_items(users, k=k + 1)
        ids, scores = m.top_k_items(users, k=k, sample_seed=123, draw=0)
        assert np.isfinite(scores).all()
        clear = (-np.diff(plain_scores, axis=1)).min(axis=1) > 1e-4
        assert clear.sum() > U // 4, clear.sum()
        np.testing.assert_array_equal(ids[clear], plain_ids[clear, :k])
        np.testing.assert_allclose(scores[clear], plain_scores[clear, :k], atol=1e-4, rtol=0)
    finally:
        for s, v in zip((USER, ITEM), keep):
            ctx.set_array(s, ARR_COV, v)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_without_a_seed_top_k_items_is_the_item_call(name):
    from pmf_hip import ITEM, PREDICT_BIAS, USER
    m, _ = _model(name)
    users = np.array([3, 299, 3, 0, 150])
    for exclude_train in (False, True):
        got = m.top_k_items(users, k=10, exclude_train=exclude_train)
        again = m.top_k_items(users, k=10, exclude_train=exclude_train, sample_seed=None, draw=5)
        want = m._ctx.topk_items(users, 10, use_bias=PREDICT_BIAS, exclude_train=exclude_train)
        for a in (got, again):
            assert a[0].tobytes() == want[0].tobytes() and a[1].tobytes() == want[1].tobytes()
    q = m._ctx.topk_query(ITEM, 10, ids=users, query_side=USER, score=PREDICT_BIAS)
    got = m.top_k_items(users, k=10)
    assert got[0].tobytes() == q[0].tobytes() and got[1].tobytes() == q[1].tobytes()


def test_refusals_name_the_argument_and_write_nothing():
    import ctypes as C
    import pmf_hip
    from pmf_hip import ITEM, PREDICT_SCALE, SCORE_COSINE, USER
    m, _ = _model("k16_f32")
    ctx = m._ctx
    for score in (SCORE_COSINE, PREDICT_SCALE, 3):
        with pytest.raises(pmf_hip.PmfError, match="pmf_topk_sampled: score must be 0 or PMF_PREDICT_BIAS"):
            ctx.topk_sampled(ITEM, 5, [0, 1], query_side=USER, score=score)
    with pytest.raises(pmf_hip.PmfError, match="negative draw -1"):
        ctx.topk_sampled(ITEM, 5, [0, 1], query_side=USER, draw=-1)
    with pytest.raises(pmf_hip.PmfError, match="query id 300 at position 1"):
        ctx.topk_sampled(ITEM, 5, [0, 300], query_side=USER)
    with pytest.raises(pmf_hip.PmfError, match="k=258"):
        ctx.topk_sampled(ITEM, 258, [0], query_side=USER)
    with pytest.raises(pmf_hip.PmfError, match="query_side == cand_side"):
        ctx.topk_sampled(ITEM, 5, [0], query_side=ITEM, score=1)
    ids, scores = np.full((2, 5), -9, dtype=np.int32), np.full((2, 5), -9.0)
    q = np.array([0, 1], dtype=np.int32)
    rc = ctx._lib.pmf_topk_sampled(ctx._h, ITEM, 2, USER, q.ctypes.data_as(C.POINTER(C.c_int32)), SCORE_COSINE, None, None, 5,
                                   C.c_uint64(1), 0, ids.ctypes.data_as(C.POINTER(C.c_int32)), scores.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -1 and (ids == -9).all() and (scores == -9.0).all()
    assert ctx._lib.pmf_topk_sampled(ctx._h, ITEM, 2, USER, None, 0, None, None, 5, C.c_uint64(1), 0, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                     scores.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert "null query_ids" in ctx._lib.pmf_last_error().decode()
    # a context without covariances
    with pmf_hip.Context(6, 5, 8) as bare:
        bare.set_array(USER, pmf_hip.ARR_FACTOR, np.ones((6, 8))); bare.set_array(ITEM, pmf_hip.ARR_FACTOR, np.ones((5, 8)))
        with pytest.raises(pmf_hip.PmfError, match="(?i)pmf_topk_sampled: array cov"):
            bare.topk_sampled(ITEM, 2, [0], query_side=USER)


def test_predict_draws_are_the_dots_of_the_sampled_rows():
    from pmf_hip import ARR_BIAS, ITEM, USER
    m, _ = _model("k16_f64")
    u, i = np.array([4, 4, 17, 250, 4]), np.array([9, 200, 9, 9, 9])
    draws = m.predict_draws(u, i, 6, seed=31, global_mean=2.5)
    assert draws.shape == (5, 6)
    theta, beta = m.sample_factors("user", u, 6, 31), m.sample_factors("item", i, 6, 31)
    bu, bi = m._ctx.get_array_rows(USER, ARR_BIAS, u), m._ctx.get_array_rows(ITEM, ARR_BIAS, i)
    np.testing.assert_allclose(draws, np.einsum("ndk,ndk->nd", theta, beta) + (bu + bi)[:, None] + 2.5, rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(draws[0], draws[4])                      # the same pair twice
    np.testing.assert_array_equal(theta[0], theta[1])                      # two pairs of one user share that user's draw
    # the mean of many draws approaches predict, their spread predict_variance (without noise): 6 standard errors
    n = 4000
    d = m.predict_draws(u[:3], i[:3], n, seed=8)
    mean, var = m.predict(u[:3], i[:3]), m.predict_variance(u[:3], i[:3], include_noise=False)
    assert (np.abs(d.mean(axis=1) - mean) <= 6 * np.sqrt(var / n)).all()
    assert (np.abs(d.var(axis=1) / var - 1.0) <= 0.25).all()
    with pytest.raises(ValueError, match="side must be"):
        m.sample_factors("users", [0])


def test_classes_without_a_full_posterior_refuse():
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config

    class TwoRanks:
        world, rank = 2, 0
    sharded = GaussianMFCAVI(GaussianMFCAVIConfig(n_factors=4, verbose=False), comm=TwoRanks())
    for call in (lambda: sharded.sample_factors("item", [0]), lambda: sharded.predict_draws([0], [0], 2),
                 lambda: sharded.top_k_items([0], k=1, sample_seed=0)):
        with pytest.raises(NotImplementedError, match="comm="):
            call()
    df = _frame()
    sgd = GaussianMFSGD(GaussianMFSGDConfig(n_factors=8, max_iter=1, verbose=False)).fit(df, global_mean=0.0)
    hpf = HPF_CAVI(HPF_CAVI_Config(n_factors=8, max_iter=1, tol=None, verbose=False)).fit(df.assign(rating=df["rating"] + 3.0))
    try:
        for model in (sgd, hpf):
            for call in (lambda: model.sample_factors("user", [0]), lambda: model.predict_draws([0], [0], 2),
                         lambda: model.top_k_items([0], k=1, sample_seed=0)):
                with pytest.raises(NotImplementedError, match="covariances"):
                    call()
            assert model.top_k_items([0, 1], k=3)[0].shape == (2, 3)           # the unsampled call is what it was
    finally:
        sgd.close(); hpf.close()
