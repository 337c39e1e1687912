"""Device-memory accounting (pmf_ctx_device_bytes, bench.py's `device_GB`): every device buffer of a context is
counted when it is allocated and taken off by exactly that amount when it is released.  The checks need no recorded
number: repeating a step changes nothing, going to a smaller problem and back returns to the same figure, and one
more state array costs exactly its padded size."""
import numpy as np
import pytest

from helpers import skewed_problem

pytestmark = pytest.mark.gpu

U, I, K = 600, 200, 16


def _problem(seed, n):
    """heavy head rows (split over several tasks: the partial-sum buffer is in use) and empty rows"""
    u, i, x = skewed_problem(seed, U, I, n, rating_kind="count")
    assert np.bincount(i, minlength=I).max() > 64
    return u, i, x


def _iterate(ctx):
    """one Gaussian iteration (factors + biases), then one Poisson iteration from a positive state"""
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(1)
    ctx.set_array(USER, ARR_FACTOR, 0.1 * rng.standard_normal((U, K))); ctx.set_array(ITEM, ARR_FACTOR, 0.1 * rng.standard_normal((I, K)))
    ctx.set_cov_identity(USER); ctx.set_cov_identity(ITEM)
    ctx.set_array(USER, ARR_BIAS, np.zeros(U)); ctx.set_array(ITEM, ARR_BIAS, np.zeros(I))
    for side in (USER, ITEM):
        ctx.gauss_factor_sweep(side, 0.3, 0.5)
    for side in (USER, ITEM):
        ctx.gauss_bias_sweep(side, 0.3, 1.0)
    ctx.set_array(USER, ARR_FACTOR, rng.gamma(1.0, 0.5, (U, K))); ctx.set_array(ITEM, ARR_FACTOR, rng.gamma(1.0, 0.5, (I, K)))
    for side in (USER, ITEM):
        ctx.gamma_sweep(side, 0.3, 1.0)
    ctx.sync()


def _assert_repeatable(ctx, step, what):
    """the first call may size buffers; the second, identical one must leave the figure alone"""
    step()
    before = ctx.device_bytes()
    step()
    assert ctx.device_bytes() == before, (what, before, ctx.device_bytes())


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_repeating_a_step_leaves_device_bytes_unchanged(dtype):
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    u, i, x = _problem(1, 6000)
    rng = np.random.default_rng(2)
    vu, vi, vy = rng.integers(0, U, 900), rng.integers(0, I, 900), rng.integers(1, 6, 900).astype(np.float64)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        assert ctx.device_bytes() == 0
        _assert_repeatable(ctx, lambda: ctx.set_ratings(u, i, x), "set_ratings")
        assert ctx.device_bytes() > 0
        _assert_repeatable(ctx, lambda: _iterate(ctx), "sweeps")
        _assert_repeatable(ctx, lambda: ctx.eval_set(vu, vi, vy), "eval_set")
        _assert_repeatable(ctx, lambda: ctx.eval_run(), "eval_run")
        _assert_repeatable(ctx, lambda: ctx.topk_items(np.arange(50), 5), "topk_items")
        for arr in (ARR_FACTOR, ARR_COV):
            _assert_repeatable(ctx, lambda: ctx.get_array_rows(USER, arr, [3, 0, U - 1]), "get_array_rows")
        _assert_repeatable(ctx, lambda: ctx.set_row_chunks(ITEM, 3), "set_row_chunks")
        _assert_repeatable(ctx, lambda: _iterate(ctx), "sweeps with row chunks")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_smaller_problem_and_back_returns_to_the_same_figure(dtype):
    import pmf_hip
    from pmf_hip import ITEM
    a, b = _problem(1, 6000), _problem(2, 2000)
    rng = np.random.default_rng(3)
    vu, vi, vy = rng.integers(0, U, 900), rng.integers(0, I, 900), rng.integers(1, 6, 900).astype(np.float64)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        seen = []
        for data in (a, b, a):
            ctx.set_ratings(*data)
            _iterate(ctx)
            seen.append(ctx.device_bytes())
        assert seen[2] == seen[0], seen
        assert 0 < seen[1] < seen[0], seen   # the index arrays are proportional to the ratings; nothing else shrinks

        seen = []
        for n in (900, 300, 900):
            assert ctx.eval_set(vu[:n], vi[:n], vy[:n])
            ctx.eval_run()
            seen.append(ctx.device_bytes())
        assert seen[2] == seen[0] and seen[1] < seen[0], seen

        seen = []
        for chunks in (1, 4, 1):
            ctx.set_row_chunks(ITEM, chunks)
            _iterate(ctx)
            seen.append(ctx.device_bytes())
        assert seen[2] == seen[0], seen


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_more_array_costs_its_padded_size(dtype):
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ARR_RATE, ARR_SHAPE, ITEM, USER
    u, i, x = _problem(1, 6000)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        elem = np.dtype(ctx.np_dtype).itemsize
        ctx.set_ratings(u, i, x)
        assert ctx.device_bytes() > 0
        for side, arr in ((USER, ARR_FACTOR), (ITEM, ARR_FACTOR), (USER, ARR_SHAPE), (ITEM, ARR_RATE)):
            before = ctx.device_bytes()
            ctx.set_array(side, arr, np.ones((ctx.rows(side), K)))
            assert ctx.device_bytes() - before == ctx.rows(side) * ctx.kpad * elem, (side, arr)
            ctx.set_array(side, arr, np.zeros((ctx.rows(side), K)))   # already there: nothing more
            assert ctx.device_bytes() - before == ctx.rows(side) * ctx.kpad * elem, (side, arr)
