"""The Gaussian item-bias sweep from the factor sweep's mean sums (gauss_bias_sums_kernel: no second gather of the
mean rows) against the gathering sweep (PMF_GAUSS_BIAS_GATHER=1: the kernel every other configuration runs), the CPU
oracle and fp64 NumPy on the state actually on the device -- through the C ABI, fp32.

Shapes: `skewed_problem` at U = 1500, I = 300, N = 40000 (task length 32: most items are split rows, no task longer
than one 64-rating batch) and, with PMF_TASK_CHUNK=512, I = 40, N = 60000 (tasks of several batches, rows of 3+ slots).
"""
import numpy as np
import pytest

import gauss_bias_sums_reference as ref
from helpers import max_abs, skewed_problem
from oracle import cavi_oracle as orc
from test_gauss_gpu import TOL

pytestmark = pytest.mark.gpu

SIGMA2, ETA2, ETA_B2 = 0.3, 0.5, 1.0
SHORT = dict(U=1500, I=300, N=40000)             # task length 32
LONG = dict(U=1500, I=40, N=60000, chunk=512)    # PMF_TASK_CHUNK=512


def _bits_differ(a, b):
    return np.asarray(a, dtype=np.float32).view(np.uint32) != np.asarray(b, dtype=np.float32).view(np.uint32)


def _run(monkeypatch, K, U, I, N, chunk=None, gather=False, env=(), dtype="f32", iters=1, shift=0.0, user_bias=None,
         between=None, user_bias_sweep=True):
    """`iters` iterations in the reference's order; `between(ctx, data)` runs before the LAST item-bias sweep and may
    return other ratings (u, i, x), which are then what that sweep saw.  Returns the final state, the state after the
    first iteration's factor sweeps ("first_*") and bias sweeps ("it1_*"), and the ratings of the last bias sweep."""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER
    for key in ("PMF_GAUSS_BIAS_GATHER", "PMF_TASK_CHUNK", "PMF_GAUSS_UNFUSED", "PMF_GAUSS_GENERIC"):
        monkeypatch.delenv(key, raising=False)
    if gather:
        monkeypatch.setenv("PMF_GAUSS_BIAS_GATHER", "1")
    if chunk:
        monkeypatch.setenv("PMF_TASK_CHUNK", str(chunk))
    for key in env:
        monkeypatch.setenv(key, "1")
    u, i, x = skewed_problem(100 + K, U, I, N, rating_kind="centered")
    x = x + shift
    init = orc.init_gaussian(U, I, K, seed=5, bias=True)
    out = {"ratings": (u, i, x)}
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        def state(prefix, cov=False):
            out[prefix + "m_theta"], out[prefix + "m_beta"] = ctx.get_array(USER, ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
            out[prefix + "m_user_bias"], out[prefix + "m_item_bias"] = ctx.get_array(USER, ARR_BIAS), ctx.get_array(ITEM, ARR_BIAS)
            if cov:
                out[prefix + "V_theta"], out[prefix + "V_beta"] = ctx.get_array(USER, ARR_COV), ctx.get_array(ITEM, ARR_COV)
        ctx.set_ratings(u, i, x)
        ctx.set_array(USER, ARR_FACTOR, init["m_theta"]); ctx.set_array(ITEM, ARR_FACTOR, init["m_beta"])
        ctx.set_cov_identity(USER); ctx.set_cov_identity(ITEM)
        ctx.set_array(USER, ARR_BIAS, init["m_user_bias"] if user_bias is None else user_bias)
        ctx.set_array(ITEM, ARR_BIAS, init["m_item_bias"])
        for it in range(iters):
            ctx.gauss_factor_sweep(USER, SIGMA2, ETA2)
            ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA2)
            if it == 0 and between is None:
                state("first_", cov=True)   # (reading the state writes nothing: the sums stay valid)
            if user_bias_sweep:
                ctx.gauss_bias_sweep(USER, SIGMA2, ETA_B2)
            if it == iters - 1 and between is not None:
                out["ratings"] = between(ctx, (u, i, x)) or out["ratings"]
                state("before_")
            ctx.gauss_bias_sweep(ITEM, SIGMA2, ETA_B2)
            if it == 0:
                state("it1_")
        state("", cov=True)
    for key in ("PMF_GAUSS_BIAS_GATHER", "PMF_TASK_CHUNK") + tuple(env):
        monkeypatch.delenv(key, raising=False)
    return out


def _numpy_item_bias(r, prefix):
    """the item-bias sweep in fp64 NumPy from the device state `prefix` names (what the sweep read)"""
    u, i, x = r["ratings"]
    I = r["m_item_bias"].shape[0]
    return ref.bias_sweep(i, u, x, I, r[prefix + "m_beta"], r[prefix + "m_theta"], r[prefix + "m_item_bias"],
                          r[prefix + "m_user_bias"], SIGMA2, ETA_B2)


PARITY = [(K, "short") for K in (5, 16, 32, 33, 48, 50, 64)] + [(16, "long"), (64, "long")]

_ORACLE = {}


def _oracle(K, U, I, N):
    """Two iterations of the CPU oracle on the problem `_run` sets up, once per problem: its per-row loop, which at
    K = 64 is several times faster than the vectorised form (that one gathers N x K x K covariances at once)."""
    if (K, U, I, N) not in _ORACLE:
        u, i, x = skewed_problem(100 + K, U, I, N, rating_kind="centered")
        st = orc.init_gaussian(U, I, K, seed=5, bias=True)
        idx = (orc.group_positions(u, U), orc.group_positions(i, I))
        for _ in range(2):
            orc.gaussian_iteration(st, idx, u, i, x, SIGMA2, ETA2, ETA2, ETA_B2, vectorised=False)
        _ORACLE[(K, U, I, N)] = st
    return _ORACLE[(K, U, I, N)]


@pytest.mark.parametrize("K,shape", PARITY)
def test_parity_with_oracle_and_gathering_sweep(K, shape, monkeypatch):
    """Both KB, every PU, K not a multiple of 4; two iterations of the reference's order."""
    sz = dict(SHORT if shape == "short" else LONG)
    fast = _run(monkeypatch, K, iters=2, **sz)
    slow = _run(monkeypatch, K, iters=2, gather=True, **sz)
    chunk = sz.pop("chunk", None)
    if chunk:   # the longest item row is cut into three or more tasks of more than one 64-rating batch
        assert np.bincount(fast["ratings"][1]).max() > 2 * chunk
    st = _oracle(K, sz["U"], sz["I"], sz["N"])
    for key in ("m_theta", "m_beta", "m_user_bias", "m_item_bias"):
        assert max_abs(fast[key], st[key]) <= 2e-4, key
    # the accumulate's sums and their order have not changed: the first factor sweeps agree to the bit
    for key in ("first_m_theta", "first_m_beta", "first_V_theta", "first_V_beta"):
        assert np.array_equal(fast[key], slow[key]), key
    assert np.array_equal(fast["it1_m_user_bias"], slow["it1_m_user_bias"])
    assert max_abs(fast["it1_m_item_bias"], slow["it1_m_item_bias"]) <= 3e-5
    assert max_abs(fast["m_item_bias"], slow["m_item_bias"]) <= 3e-5
    # the sums form really ran: another summation order cannot agree to the bit on most rows
    nonempty = np.bincount(fast["ratings"][1], minlength=sz["I"]) > 0
    differ = _bits_differ(fast["it1_m_item_bias"], slow["it1_m_item_bias"])
    assert differ[nonempty].sum() >= 0.5 * nonempty.sum(), (int(differ[nonempty].sum()), int(nonempty.sum()))
    # rows without ratings keep their bias (gaussian_mf_cavi_bias.py:134-135)
    assert (~nonempty).any() and np.array_equal(fast["m_item_bias"][~nonempty], np.zeros((~nonempty).sum()))


@pytest.mark.parametrize("K", [16, 64])
def test_cancellation_error_against_fp64(K, monkeypatch):
    """Ratings left uncentred and large user biases: sum (x - b_u) and m_i . H_i are both large against their
    difference.  The sums form may lose at most 4 x what the gathering form loses on the same input (or TOL f32).
    Measured on an MI355X: K = 16 sums form 8.9e-7, gathering form 3.2e-7; K = 64 6.9e-7 against 1.5e-7."""
    user_bias = np.random.default_rng(11).normal(0.0, 2.0, SHORT["U"])
    kw = dict(shift=3.5, user_bias=user_bias, user_bias_sweep=False, between=lambda ctx, data: None, **SHORT)
    fast = _run(monkeypatch, K, **kw)
    slow = _run(monkeypatch, K, gather=True, **kw)
    for key in ("before_m_theta", "before_m_beta", "before_m_user_bias"):
        assert np.array_equal(fast[key], slow[key]), key
    want = _numpy_item_bias(fast, "before_")
    u, i, x = fast["ratings"]
    first = np.bincount(i, weights=x - fast["before_m_user_bias"][u], minlength=SHORT["I"])
    assert np.abs(first).max() > 1e3     # the first sum is large ...
    err_fast, err_slow = max_abs(fast["m_item_bias"], want), max_abs(slow["m_item_bias"], want)
    print(f"cancellation K={K}: sums form {err_fast:.3e}, gathering form {err_slow:.3e}")
    assert _bits_differ(fast["m_item_bias"], slow["m_item_bias"]).any()
    assert err_fast <= max(4 * err_slow, TOL["f32"][1]), (err_fast, err_slow)


def _other_factor(side_rows, K, seed):
    return 0.3 * np.random.default_rng(seed).standard_normal((side_rows, K))


def _stale_set_user(ctx, data):
    from pmf_hip import ARR_FACTOR, USER
    ctx.set_array(USER, ARR_FACTOR, _other_factor(SHORT["U"], 16, 21))


def _stale_set_user_rows(ctx, data):
    from pmf_hip import ARR_FACTOR, USER
    rows = np.unique(data[0])[:10]     # ten users that have ratings
    ctx.set_array_rows(USER, ARR_FACTOR, rows, 1.0 + _other_factor(10, 16, 22))


def _stale_set_item(ctx, data):
    from pmf_hip import ARR_FACTOR, ITEM
    ctx.set_array(ITEM, ARR_FACTOR, _other_factor(SHORT["I"], 16, 23))


def _stale_factor_sweep(ctx, data):
    from pmf_hip import USER
    ctx.gauss_factor_sweep(USER, SIGMA2, ETA2)


def _stale_sgd_sweep(ctx, data):
    from pmf_hip import USER
    ctx.gauss_sgd_sweep(USER, 0.05, SIGMA2, ETA2, ETA_B2)


def _stale_set_ratings(ctx, data):
    u, i, x = data
    rng = np.random.default_rng(24)
    u2 = rng.permutation(u)            # the same users, items and values, paired anew
    u2[0] = u[0]
    ctx.set_ratings(u2, i, x)
    return u2, i, x


@pytest.mark.parametrize("between", [_stale_set_user, _stale_set_user_rows, _stale_set_item, _stale_factor_sweep,
                                     _stale_sgd_sweep, _stale_set_ratings], ids=lambda f: f.__name__[7:])
def test_a_write_between_the_sweeps_falls_back_to_the_gather(between, monkeypatch):
    """Anything that writes a FACTOR array or the ratings between the item factor sweep and the item bias sweep
    invalidates the mean sums: the bias sweep is then the gathering kernel itself -- the same bits as the forced run
    -- and right for the state on the device (a stale sum is off by O(0.1) here)."""
    K = 16
    fast = _run(monkeypatch, K, between=between, **SHORT)
    slow = _run(monkeypatch, K, between=between, gather=True, **SHORT)
    for key in ("before_m_theta", "before_m_beta", "before_m_user_bias"):
        assert np.array_equal(fast[key], slow[key]), key
    assert np.array_equal(fast["m_item_bias"], slow["m_item_bias"])
    assert max_abs(fast["m_item_bias"], _numpy_item_bias(fast, "before_")) <= 2e-4


def test_a_stale_sum_would_show(monkeypatch):
    """the bound of the test above separates: the sums of the state before `_stale_set_user` miss it by far"""
    K = 16
    r = _run(monkeypatch, K, between=_stale_set_user, **SHORT)
    u, i, x = r["ratings"]
    stale = dict(r, before_m_theta=orc.init_gaussian(SHORT["U"], SHORT["I"], K, seed=5)["m_theta"])
    assert max_abs(_numpy_item_bias(stale, "before_"), _numpy_item_bias(r, "before_")) > 50 * 2e-4


@pytest.mark.parametrize("case", ["unfused", "generic", "f64", "k72"])
def test_configurations_without_mean_sums_run_the_gathering_kernel(case, monkeypatch):
    kw = dict(unfused=dict(K=16, env=("PMF_GAUSS_UNFUSED",)), generic=dict(K=16, env=("PMF_GAUSS_GENERIC",)),
              f64=dict(K=16, dtype="f64"), k72=dict(K=72))[case]
    kw.update(U=800, I=50, N=7000)
    a = _run(monkeypatch, **kw)
    b = _run(monkeypatch, gather=True, **kw)
    for key in ("m_theta", "m_beta", "m_user_bias", "m_item_bias"):
        assert np.array_equal(a[key], b[key]), key


def test_empty_rows_keep_their_bias(monkeypatch):
    """gaussian_mf_cavi_bias.py:134-135, with a bias that is not zero to begin with"""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, USER
    monkeypatch.delenv("PMF_GAUSS_BIAS_GATHER", raising=False)
    U, I, K = 40, 30, 8
    rng = np.random.default_rng(1)
    u = rng.integers(0, U, 300); i = rng.integers(0, I, 300)
    u[u == 7] = 8; i[i == 3] = 4; u[0], i[0] = U - 1, I - 1
    x = rng.normal(size=300)
    bu, bi = rng.normal(size=U), rng.normal(size=I)
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        ctx.set_ratings(u, i, x)
        ctx.set_array(USER, ARR_FACTOR, rng.normal(size=(U, K))); ctx.set_array(ITEM, ARR_FACTOR, rng.normal(size=(I, K)))
        ctx.set_cov_identity(USER, 1.0); ctx.set_cov_identity(ITEM, 1.0)
        ctx.set_array(USER, ARR_BIAS, bu); ctx.set_array(ITEM, ARR_BIAS, bi)
        ctx.gauss_factor_sweep(USER, SIGMA2, ETA2); ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA2)
        ctx.gauss_bias_sweep(USER, SIGMA2, ETA_B2); ctx.gauss_bias_sweep(ITEM, SIGMA2, ETA_B2)
        got_u, got_i = ctx.get_array(USER, ARR_BIAS), ctx.get_array(ITEM, ARR_BIAS)
        m_u, m_i = ctx.get_array(USER, ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
    assert got_u[7] == np.float32(bu[7]) and got_i[3] == np.float32(bi[3])
    want = ref.bias_sweep(i, u, x, I, m_i, m_u, bi, got_u, SIGMA2, ETA_B2)
    want[3] = np.float32(bi[3])
    assert max_abs(got_i, want) <= 2e-5
