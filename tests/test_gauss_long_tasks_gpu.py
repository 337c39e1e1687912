"""The Gaussian accumulate on tasks longer than one 64-rating batch, entry by entry against fp64 NumPy.

`gauss_accum_mfma_kernel` (fp32, K <= 64) and `gauss_accum_mfma128_kernel` (fp32, 64 < K <= 128) read a task's row
ids, ratings and hot flags 64 at a time, hand them out with v_readlane, run full trips of 2 PU ratings and finish
with one partial trip.  The second and later batch reloads, the index clamp of a later batch, a partial trip that
starts at j >= 64, the hot mask of a later batch and a full trip ending on a batch edge all need a task of more than
64 ratings -- and the task length follows the rating COUNT (32 up to 2^21 ratings, 512 only above 2^24), not the row
length.  PMF_TASK_CHUNK fixes it instead, `Context.task_max_len` reports what the work lists really hold, and every
test here asserts that (and the split of each row it implies) before it looks at a number.

The problem
-----------
One "long" side of one row per length in LENGTHS (1 .. 800: below, at and above 64, 128, 512 and their multiples),
three rows without ratings (one of them the last id but one), and -- for the smallest K only, where 1 MB of hot rows
is more rows than 5355 ratings can gather -- short filler rows.  The gathered ids are uniform with replacement
(duplicates inside a row), the ratings centred reals in random COO order.  Every gathered row is another matrix,
V_o = s_o (A_o A_o^T / K + I) with s_o in [0.5, 1] and A_o uniform in [-1, 1], so that every diagonal entry of
every V_o lies in [0.5, 2]; means are uniform in [-1, 1], biases N(0, 0.1^2).  The reference reads the tables back
from the device, i.e. it starts from the values the device holds.

Test A: the bound
-----------------
    S_r = sum_j (V[o_j] + m_j m_j^T)            w_r = sum_j m_j (x_j - b_r - b_{o_j})
The kernels sum the n_r covariance rows and the n_r outer products as two separate sums (vector adds / MFMA
accumulators) and add the two once; a split row is the same terms in another order plus the combine.  A sum of n
floating-point terms in ANY order is within (n - 1) u sum |t_j| of the exact one to first order (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2); one more rounding for each product m_i m_j, for the final add and for
the combine of the partial slots stay inside the "+ 8":
    |dS| <= (n_r + 8) u sum_j (|V_j| + |m_j| |m_j|^T)                 entrywise
    |dw| <= (n_r + 8) u sum_j |m_j| (|x_j| + |b_r| + |b_{o_j}|)       (two roundings for the residual, one per fma)
with u = 2^-24 (fp32 contexts) or 2^-53 (fp64 contexts).  Nothing in it is tuned and it is indifferent to how a row
was cut into tasks.

It is tight enough to see ONE wrong rating: dropping a rating from a row, or repeating one, moves every diagonal entry
of S by V_kk + m_k^2 >= 0.5, while the bound on a diagonal entry of the 800-rating row is at most
808 * 2^-24 * 800 * (2 + 1) = 0.116 (0.055 at most for the values drawn here).  `_assert_one_rating_is_visible` asserts
0.5 > 4 * bound for every row of every constructed problem before any device call; it is a condition on the
construction, not a measurement.

Test B: the tolerance
---------------------
The same long and split tasks through `gauss_factor_sweep` (the fused solve for whole-row tasks, combine + the
standalone solve for split rows), against V = inv(P), P = I / eta2 + S / sigma2, m = V w / sigma2 in fp64.  It checks
that long tasks reach the right solver with the right sums; the rows are well conditioned by construction (asserted:
cond_2(P_r) <= 100).  Per row, in the spectral norm:
    tol_V = ||V||_2^2 ||E_r||_F / sigma2  +  c K u cond_2(P_r) ||V||_2
    tol_m = tol_V ||w||_2 / sigma2  +  ||V||_2 ||e_r||_2 / sigma2
The first term of tol_V is the first-order perturbation of an inverse under Test A's entrywise bound matrix E_r, the
second the solver's own rounding; tol_m follows from m = V w / sigma2 with V off by tol_V and w off by Test A's bound
vector e_r.  The constant c is measured, not guessed, and not on the code under test: the error of NumPy's fp32 LAPACK
inverse of the same P_r against the fp64 inverse (spectral norm), over all rows and all K of this file, is at most
0.257 K u cond_2(P_r) ||V_r||_2 (the largest ratio: K = 5, an 8-rating row; it falls with K, 0.0044 at K = 128);
c = 4 * 0.257 = 1.03.  The largest cond_2(P_r) of the file is 41 (K = 150).
"""
import functools

import numpy as np
import pytest

from helpers import DeviceStats, rel_err
from oracle import cavi_oracle as orc

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 66, 79, 127, 128, 129, 130, 191, 193, 255, 257, 511, 512, 513, 514,
           640, 800)
SIGMA2, ETA2 = 0.3, 0.5
SOLVER_C = 1.03   # 4 x the largest err / (K u cond ||V||) of the fp32 LAPACK inverse (module docstring)

# One K per accumulate instantiation (launch_accum_mfma / launch_accum_mfma128 in csrc/pmf_gauss.hip; the accumulate
# pass runs the FUSE = false form, the sweep of Test B the fused one with its KS / MT):
#   K  <KB, NT[, KS]>  PU        K  <KB, NT[, KS]>  PU        K    mfma128 <NT[, MT]>
#   5  <32, 1, 8>      8        33  <64, 3, 48>     2         70   <9, 5>
#   8  <32, 1, 8>      8        40  <64, 4, 48>     2         88   <9, 6>
#  12  <32, 1, 16>     8        48  <64, 5, 48>     1         96   <13, 6>
#  16  <32, 1, 16>     8        50  <64, 5, 56>     1        100   <13, 7>
#  20  <32, 1>         8        52  <64, 6, 56>     1        120   <17, 8>
#  23  <32, 2>         4        56  <64, 7, 56>     1        128   <17, 8>
#  32  <32, 3>         2        57  <64, 7>         1
#                               60  <64, 8>         1
#                               64  <64, 9>         1
K_MFMA = (5, 8, 12, 16, 20, 23, 32, 33, 40, 48, 50, 52, 56, 57, 60, 64)
K_MFMA128 = (70, 88, 96, 100, 120, 128)

# Gathered rows U and filler rows per K.  fp32, K <= 64 runs with a 1 MB hot budget, which holds
# 2^20 / (4 (cov_stride + kpad)) rows: U is 600 where between a quarter and three quarters of the gathered rows are
# then hot (asserted), fewer for the widest rows and more for the narrow ones; at K = 5 and 8 the budget holds more
# rows than the 5355 ratings of LENGTHS can gather at all, so short filler rows gather more.  K > 64 (no hot policy):
# 300, which keeps the host tables (U K^2 doubles) under 100 MB.
SIZES = {5: (40000, 5000), 8: (20000, 2500), 12: (20000, 0), 16: (4000, 0), 20: (2500, 0), 23: (2000, 0), 32: (1000, 0),
         33: (1000, 0), 57: (300, 0), 60: (300, 0), 64: (300, 0)}


def _sizes(K):
    return SIZES.get(K, (600, 0) if K <= 64 else (300, 0))


def _task_lengths(n, chunk):
    """build_tasks (csrc/pmf_ctx.hip): rows above the chunk are cut into ceil(n / chunk) tasks of equal length +- 1"""
    if n <= chunk:
        return [n]
    q = -(-n // chunk)
    return [n // q + (1 if c < n % q else 0) for c in range(q)]


class Problem:
    """Ratings and tables of one K (shared by every chunk, side and switch; nothing in it is ever modified)."""

    def __init__(self, K, U, n_fill):
        rng = np.random.default_rng(1000 + K)
        self.K, self.U, self.R = K, U, len(LENGTHS) + 3 + n_fill
        lengths = np.concatenate([np.array(LENGTHS), 1 + np.arange(n_fill) % 9]).astype(np.int64)
        empty = (3, 11, self.R - 2)
        ids = np.setdiff1d(np.arange(self.R), empty)
        self.n = np.zeros(self.R, dtype=np.int64)
        self.n[rng.permutation(ids)] = lengths
        order = rng.permutation(int(self.n.sum()))
        self.row = np.repeat(np.arange(self.R), self.n)[order]
        self.other = rng.integers(0, U, len(order))
        self.x = rng.normal(0.0, 1.0, len(order))
        self.x -= self.x.mean()
        A = rng.uniform(-1.0, 1.0, (U, K, K))
        s = rng.uniform(0.5, 1.0, U)
        self.V = s[:, None, None] * (A @ np.swapaxes(A, 1, 2) / K + np.eye(K))
        self.m = rng.uniform(-1.0, 1.0, (U, K))
        self.b_other = rng.normal(0.0, 0.1, U)
        self.b_self = rng.normal(0.0, 0.1, self.R)
        self.m_self = rng.uniform(-1.0, 1.0, (self.R, K))
        diag = np.einsum("nkk->nk", self.V)
        assert 0.5 <= diag.min() and diag.max() <= 2.0
        assert self.n[self.R - 2] == 0 and self.n[self.R - 1] > 0 and sorted(self.n[self.n > 9]) == sorted(l for l in LENGTHS if l > 9)
        assert len(np.unique(self.other[self.row == np.argmax(self.n)])) < self.n.max()   # duplicates inside a row

    def coo(self, side):
        """(user_ids, item_ids): the long rows are item rows (side = ITEM) or user rows (side = USER)"""
        return (self.other, self.row) if side == 1 else (self.row, self.other)


@functools.lru_cache(maxsize=1)
def _problem(K):
    return Problem(K, *_sizes(K))


def _reference(p, V, m, b_self, b_other, u):
    """fp64 S, w and the entrywise bounds E (on S) and e (on w) of every long-side row, from the tables the device
    holds.  Full K x K per row."""
    K, R = p.K, p.R
    ptr, pos = orc.group_positions(p.row, R)
    S, E = np.zeros((R, K, K)), np.zeros((R, K, K))
    w, e = np.zeros((R, K)), np.zeros((R, K))
    absV = np.abs(V)
    for r in range(R):
        sel = pos[ptr[r]:ptr[r + 1]]
        if sel.size == 0:
            continue
        o = p.other[sel]
        uniq, cnt = np.unique(o, return_counts=True)
        mo = m[o]
        S[r] = np.tensordot(cnt.astype(np.float64), V[uniq], 1) + mo.T @ mo
        E[r] = (sel.size + 8) * u * (np.tensordot(cnt.astype(np.float64), absV[uniq], 1) + np.abs(mo).T @ np.abs(mo))
        w[r] = mo.T @ (p.x[sel] - b_self[r] - b_other[o])
        e[r] = (sel.size + 8) * u * (np.abs(mo).T @ (np.abs(p.x[sel]) + abs(b_self[r]) + np.abs(b_other[o])))
    return S, w, E, e


def _assert_one_rating_is_visible(p, E):
    """Dropping or repeating one rating moves a diagonal entry of S by V_kk + m_k^2 >= 0.5 (V_kk >= 0.5 is asserted
    by the construction): the fp32 bound must stay four times below that on every row."""
    worst = np.einsum("rkk->rk", E).max(axis=1)
    assert (0.5 > 4 * worst).all(), (int(np.argmax(worst)), float(worst.max()))


_REF = {}


def _cached_reference(key, make):
    """one reference per (K, dtype, side) at a time: the cases of one K follow each other"""
    if key not in _REF:
        _REF.clear()
        _REF[key] = make()
    return _REF[key]


def _new_context(n_users, n_items, K, dtype):
    import pmf_hip
    return pmf_hip.Context(n_users, n_items, K, dtype=dtype)


def _device():
    import torch
    return torch.device("cuda", 0)


def _device_sync():
    import torch
    torch.cuda.synchronize()


def _open(p, side, dtype, chunk, monkeypatch, hot_mb=None, unfused=False):
    """A context with the problem's ratings and tables, the long rows on `side`, under the given switches."""
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR
    monkeypatch.setenv("PMF_TASK_CHUNK", str(chunk))
    if hot_mb is None:
        monkeypatch.delenv("PMF_GAUSS_HOT_MB", raising=False)
    else:
        monkeypatch.setenv("PMF_GAUSS_HOT_MB", str(hot_mb))
    if unfused:
        monkeypatch.setenv("PMF_GAUSS_UNFUSED", "1")
    else:
        monkeypatch.delenv("PMF_GAUSS_UNFUSED", raising=False)
    other = 1 - side
    ctx = _new_context(*((p.U, p.R) if side == 1 else (p.R, p.U)), p.K, dtype)
    u, i = p.coo(side)
    ctx.set_ratings(u, i, p.x)
    ctx.set_array(other, ARR_FACTOR, p.m)
    ctx.set_array(other, ARR_COV, p.V)
    ctx.set_array(other, ARR_BIAS, p.b_other)
    ctx.set_array(side, ARR_BIAS, p.b_self)
    ctx.set_array(side, ARR_FACTOR, p.m_self)   # every Gaussian entry point wants both tables of both sides
    ctx.set_cov_identity(side)
    return ctx


def _assert_layout(ctx, p, side, chunk):
    """The work list holds what the test claims to run: the longest task, and with it the cut of every row."""
    tasks = [t for n in p.n[p.n > 0] for t in _task_lengths(int(n), chunk)]
    assert ctx.task_max_len(side, "gauss") == min(chunk, 800) == max(tasks)
    assert ctx.task_max_len(side, "sgd") == 256
    if chunk >= 128:
        assert {65, 128} <= set(tasks)      # a partial trip that starts at j = 64; full trips ending on a batch edge
        assert any(t > 64 and t % 64 not in (0, 1) and t % 2 for t in tasks)   # odd tail inside a later batch


def _device_tables(ctx, side, u_round):
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR
    other = 1 - side
    return (ctx.get_array(other, ARR_COV), ctx.get_array(other, ARR_FACTOR), ctx.get_array(side, ARR_BIAS),
            ctx.get_array(other, ARR_BIAS), u_round)


def _accumulate(ctx, p, side):
    """raw statistics of every row of `side`: ([R, cov_stride] packed S, [R, kpad] w) as the device wrote them"""
    width = ctx.cov_stride + ctx.kpad
    stats = DeviceStats(p.R * width, ctx.np_dtype, _device())
    _device_sync()   # torch zero-fills on its own stream, the context writes on another
    ctx.gauss_factor_accumulate(side, stats.ptr)
    ctx.sync()
    got = stats.tensor.cpu().numpy().reshape(p.R, width)
    return got[:, :ctx.cov_stride], got[:, ctx.cov_stride:]


def _check_statistics(p, got_S, got_w, ref):
    S, w, E, e = ref
    K, kp = p.K, p.K * (p.K + 1) // 2
    lo = np.tril_indices(K)   # packed lower triangle, row-major: (r, c), c <= r at r (r + 1) / 2 + c
    empty = p.n == 0
    assert empty.sum() == 3 and not got_S[empty].any() and not got_w[empty].any()
    assert not got_S[:, kp:].any() and not got_w[:, K:].any()            # row padding
    dS = np.abs(got_S[:, :kp].astype(np.float64) - S[:, lo[0], lo[1]])
    bad = np.argwhere(dS > E[:, lo[0], lo[1]])
    assert bad.size == 0, ("S", [(int(r), int(p.n[r]), int(lo[0][q]), int(lo[1][q]), float(dS[r, q])) for r, q in bad[:8]])
    dw = np.abs(got_w[:, :K].astype(np.float64) - w)
    bad = np.argwhere(dw > e)
    assert bad.size == 0, ("w", [(int(r), int(p.n[r]), int(k), float(dw[r, k])) for r, k in bad[:8]])


def _run_statistics(K, dtype, chunk, side, monkeypatch):
    p = _problem(K)
    u_round = 2.0 ** -53 if dtype == "f64" else 2.0 ** -24
    hot_policy = dtype == "f32" and K <= 64
    other = 1 - side
    with _open(p, side, dtype, chunk, monkeypatch, hot_mb=1 if hot_policy else None) as ctx:
        _assert_layout(ctx, p, side, chunk)
        ref = _cached_reference((K, dtype, side), lambda: _reference(p, *_device_tables(ctx, side, u_round)))
        if dtype == "f32":
            _assert_one_rating_is_visible(p, ref[2])
        gathered = len(np.unique(p.other))
        n_hot = len(ctx.hot_rows(other))
        if hot_policy:   # hot and cold rows alternate inside every batch, later batches of a task included
            assert 0.25 * gathered <= n_hot <= 0.75 * gathered, (n_hot, gathered)
        else:
            assert n_hot == 0
        got_S, got_w = _accumulate(ctx, p, side)
    _check_statistics(p, got_S, got_w, ref)
    if hot_policy:   # only load instructions differ: bit-identical to the policy switched off
        with _open(p, side, dtype, chunk, monkeypatch, hot_mb=0) as off:
            assert len(off.hot_rows(other)) == 0 and off.task_max_len(side, "gauss") == min(chunk, 800)
            off_S, off_w = _accumulate(off, p, side)
        assert np.array_equal(got_S, off_S) and np.array_equal(got_w, off_w)


STAT_CASES = ([(K, "f32", c) for K in K_MFMA + K_MFMA128 for c in (64, 128, 512)] +
              [(150, "f32", 128)] +                                           # fp32 beyond 128 factors: the generic kernel
              [(K, "f64", c) for K in (16, 64) for c in (64, 512)])           # fp64: the generic kernel


@pytest.mark.parametrize("K,dtype,chunk", STAT_CASES)
def test_statistics_entry_by_entry(K, dtype, chunk, monkeypatch):
    """Test A: every packed entry of S and every entry of w of every item row within the a-priori bound."""
    _run_statistics(K, dtype, chunk, 1, monkeypatch)


@pytest.mark.parametrize("K,dtype,chunk", [(64, "f32", 512), (23, "f32", 128)])
def test_statistics_of_long_user_rows(K, dtype, chunk, monkeypatch):
    """Test A with the roles swapped: the long rows are user rows and the item tables are gathered."""
    _run_statistics(K, dtype, chunk, 0, monkeypatch)


SWEEP_CASES = ([(K, c, False) for K in K_MFMA for c in (64, 512)] +
               [(K, c, unfused) for K in K_MFMA128 for unfused in (False, True) for c in (64, 512)])


@pytest.mark.parametrize("K,chunk,unfused", SWEEP_CASES)
def test_sweep_of_long_tasks(K, chunk, unfused, monkeypatch):
    """Test B: whole-row tasks through the fused solve, split rows through combine + the standalone solve."""
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM
    p = _problem(K)
    u_round = 2.0 ** -24
    with _open(p, ITEM, "f32", chunk, monkeypatch, unfused=unfused) as ctx:
        _assert_layout(ctx, p, ITEM, chunk)
        S, w, E, e = _cached_reference((K, "f32", ITEM), lambda: _reference(p, *_device_tables(ctx, ITEM, u_round)))
        m0, V0 = ctx.get_array(ITEM, ARR_FACTOR), ctx.get_array(ITEM, ARR_COV)
        ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA2)
        got_m, got_V = ctx.get_array(ITEM, ARR_FACTOR), ctx.get_array(ITEM, ARR_COV)
    live = p.n > 0
    assert np.array_equal(got_m[~live], m0[~live]) and np.array_equal(got_V[~live], V0[~live])   # no ratings: untouched
    P = np.eye(K) / ETA2 + S[live] / SIGMA2
    V = np.linalg.inv(P)
    m = np.einsum("rkl,rl->rk", V, w[live]) / SIGMA2
    cond = np.linalg.cond(P)
    assert cond.max() <= 100, float(cond.max())
    nV = np.linalg.norm(V, 2, axis=(1, 2))
    tol_V = nV ** 2 * np.linalg.norm(E[live], axis=(1, 2)) / SIGMA2 + SOLVER_C * K * u_round * cond * nV
    tol_m = tol_V * np.linalg.norm(w[live], axis=1) / SIGMA2 + nV * np.linalg.norm(e[live], axis=1) / SIGMA2
    err_V = np.linalg.norm(got_V[live] - V, 2, axis=(1, 2))
    err_m = np.linalg.norm(got_m[live] - m, axis=1)
    rows, n = np.flatnonzero(live), p.n[live]
    print(f"K={K} chunk={chunk} unfused={unfused}: max err_V/tol_V {np.max(err_V / tol_V):.3g} "
          f"(n={n[np.argmax(err_V / tol_V)]}), max err_m/tol_m {np.max(err_m / tol_m):.3g} (n={n[np.argmax(err_m / tol_m)]})")
    bad = np.flatnonzero(err_V > tol_V)
    assert bad.size == 0, ("V", [(int(rows[k]), int(n[k]), float(err_V[k]), float(tol_V[k])) for k in bad[:8]])
    bad = np.flatnonzero(err_m > tol_m)
    assert bad.size == 0, ("m", [(int(rows[k]), int(n[k]), float(err_m[k]), float(tol_m[k])) for k in bad[:8]])


# ---- Test C: the other lists honour the override ----------------------------------------------------------------
# tolerances of test_gamma_gpu.py::test_half_sweeps_vs_oracle_skewed (relative, every element) ...
GAMMA_TOL = {"f64": 1e-11, "f32": 3e-5}
# ... and of test_gauss_gpu.py::test_half_sweeps_vs_oracle_skewed for the biases (absolute: they are O(0.1))
BIAS_TOL = {"f64": 1e-10, "f32": 2e-4}


@pytest.mark.parametrize("chunk", [128, 512])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("K", [8, 40])
def test_gamma_sweep_honours_the_task_chunk(K, dtype, chunk, monkeypatch):
    from pmf_hip import ARR_FACTOR, ARR_RATE, ARR_SHAPE, ITEM
    p = _problem(K)
    rng = np.random.default_rng(K)
    x = rng.integers(1, 6, len(p.x)).astype(np.float64)
    Et, Eb = rng.gamma(2.0, 0.3, (p.U, K)) + 0.05, rng.gamma(2.0, 0.3, (p.R, K)) + 0.05
    u, i = p.coo(ITEM)
    monkeypatch.setenv("PMF_TASK_CHUNK", str(chunk))
    with _new_context(p.U, p.R, K, dtype) as ctx:
        ctx.set_ratings(u, i, x)
        assert ctx.task_max_len(ITEM, "gamma") == min(chunk, 800) and ctx.task_max_len(ITEM, "sgd") == 256
        ctx.set_array(0, ARR_FACTOR, Et)
        ctx.set_array(ITEM, ARR_FACTOR, Eb)
        Et_dev, Eb_dev = ctx.get_array(0, ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
        ctx.gamma_sweep(ITEM, 0.3, 0.7)
        got = ctx.get_array(ITEM, ARR_SHAPE), ctx.get_array(ITEM, ARR_RATE), ctx.get_array(ITEM, ARR_FACTOR)
    a, b = orc.gamma_half_sweep_rows(Eb_dev, Et_dev, *orc.group_positions(i, p.R), u, x, 0.3, 0.7)
    for name, g, want in zip(("shape", "rate", "factor"), got, (a, b, a / b)):
        assert rel_err(g, want) <= GAMMA_TOL[dtype], name


@pytest.mark.parametrize("chunk", [128, 512])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_bias_sweep_honours_the_task_chunk(dtype, chunk, monkeypatch):
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM
    p = _problem(40)
    with _open(p, ITEM, dtype, chunk, monkeypatch) as ctx:
        assert ctx.task_max_len(ITEM, "bias") == min(chunk, 800) and ctx.task_max_len(ITEM, "sgd") == 256
        tables = [ctx.get_array(ITEM, ARR_BIAS), ctx.get_array(0, ARR_BIAS), ctx.get_array(ITEM, ARR_FACTOR),
                  ctx.get_array(0, ARR_FACTOR)]
        ctx.gauss_bias_sweep(ITEM, SIGMA2, 1.0)
        got = ctx.get_array(ITEM, ARR_BIAS)
    want = orc.gauss_bias_sweep_rows(*tables, *orc.group_positions(p.row, p.R), p.other, p.x, SIGMA2, 1.0)
    assert np.array_equal(got[p.n == 0], tables[0][p.n == 0])
    assert np.max(np.abs(got - want)) <= BIAS_TOL[dtype]


@pytest.mark.parametrize("value", ["", "48", "16", "1024", "512"])
def test_sgd_list_and_unset_switch(value, monkeypatch):
    """The gradient mode's list keeps its 256 whatever the switch says; a value that is no power of two in [32, 512]
    (or none) leaves the rule by rating count in force: 32 at this size."""
    p = _problem(16)
    if value:
        monkeypatch.setenv("PMF_TASK_CHUNK", value)
    else:
        monkeypatch.delenv("PMF_TASK_CHUNK", raising=False)
    want = 512 if value == "512" else 32
    with _new_context(p.U, p.R, 16, "f32") as ctx:
        ctx.set_ratings(*p.coo(1), p.x)
        for side in (0, 1):
            assert ctx.task_max_len(side, "sgd") == (256 if side == 1 else int(np.bincount(p.other).max()))
        assert [ctx.task_max_len(1, kind) for kind in ("gamma", "gauss", "bias")] == [want] * 3
