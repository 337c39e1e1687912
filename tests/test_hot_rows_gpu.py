"""The Gaussian gather cache policy (PMF_GAUSS_HOT_MB): the most-rated rows of each side, as many as fit the budget,
are gathered with the default cache policy and all others non-temporally.  Only load instructions change, so every
state must be bit-identical to the policy switched off; and the hot set must be exactly the top-degree rows that fit."""
import numpy as np
import pytest

from helpers import skewed_problem
from oracle import cavi_oracle as orc

pytestmark = pytest.mark.gpu

U, I, N = 3000, 2000, 40000


def _run(K, budget_mb, monkeypatch, dtype="f32", iters=3):
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER
    if budget_mb is None:
        monkeypatch.delenv("PMF_GAUSS_HOT_MB", raising=False)
    else:
        monkeypatch.setenv("PMF_GAUSS_HOT_MB", str(budget_mb))
    u, i, x = skewed_problem(200 + K, U, I, N, rating_kind="centered")
    init = orc.init_gaussian(U, I, K, seed=5, bias=True)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_ratings(u, i, x)
        ctx.set_array(USER, ARR_FACTOR, init["m_theta"]); ctx.set_array(ITEM, ARR_FACTOR, init["m_beta"])
        ctx.set_cov_identity(USER); ctx.set_cov_identity(ITEM)
        ctx.set_array(USER, ARR_BIAS, init["m_user_bias"]); ctx.set_array(ITEM, ARR_BIAS, init["m_item_bias"])
        hot = {USER: ctx.hot_rows(USER), ITEM: ctx.hot_rows(ITEM)}
        row_bytes = (ctx.cov_stride + ctx.kpad) * 4
        for _ in range(iters):
            ctx.gauss_factor_sweep(USER, 0.3, 0.5)
            ctx.gauss_factor_sweep(ITEM, 0.3, 0.5)
            ctx.gauss_bias_sweep(USER, 0.3, 1.0)
            ctx.gauss_bias_sweep(ITEM, 0.3, 1.0)
        state = {(s, a): ctx.get_array(s, a) for s in (USER, ITEM) for a in (ARR_FACTOR, ARR_COV, ARR_BIAS)}
    return state, hot, row_bytes, (np.bincount(u, minlength=U), np.bincount(i, minlength=I))


@pytest.mark.parametrize("K", [64, 48, 16])   # one pair per trip (K = 64) and 2 / 8 pairs per trip (K = 48 / 16)
def test_states_bit_identical_for_every_budget(K, monkeypatch):
    _, _, _, (du, di) = _run(K, 0, monkeypatch, iters=0)
    # (split into 32-rating tasks: the task length at N = 40 000.  Hot and cold rows inside the later 64-rating batches
    #  of one task are the business of tests/test_gauss_long_tasks_gpu.py)
    assert du.max() > 512 and di.max() > 512, "need rows split over several accumulate tasks"
    off, hot_off, _, _ = _run(K, 0, monkeypatch)
    assert all(len(h) == 0 for h in hot_off.values())
    for budget in (1, None):   # 1 MB: hot and cold rows mixed inside trips; None: the default budget
        got, hot, row_bytes, (du, di) = _run(K, budget, monkeypatch)
        if budget == 1:
            for h, deg in ((hot[0], du), (hot[1], di)):
                assert 0 < len(h) < np.count_nonzero(deg)
        for key in off:
            assert np.array_equal(got[key], off[key]), (budget, key)


@pytest.mark.parametrize("K", [64, 16])
@pytest.mark.parametrize("budget", [1, 2])
def test_hot_rows_are_the_top_degree_rows_within_budget(K, budget, monkeypatch):
    _, hot, row_bytes, degs = _run(K, budget, monkeypatch, iters=0)
    for side, deg in enumerate(degs):
        order = np.lexsort((np.arange(len(deg)), -deg))   # most-rated first, ties by ascending id
        n = min(budget * 2**20 // row_bytes, np.count_nonzero(deg))
        assert np.array_equal(hot[side], order[:n]), side
        assert len(hot[side]) * row_bytes <= budget * 2**20
        assert (deg[hot[side]] > 0).all()


def test_policy_off_outside_the_fp32_k64_kernel(monkeypatch):
    for K, dtype in ((64, "f64"), (72, "f32")):
        _, hot, _, _ = _run(K, 64, monkeypatch, dtype=dtype, iters=0)
        assert all(len(h) == 0 for h in hot.values()), (K, dtype)
