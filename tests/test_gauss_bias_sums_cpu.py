"""The sums form of the Gaussian bias half-sweep against the per-rating residual form, both in fp64 NumPy
(tests/gauss_bias_sums_reference.py), and the residual form against the CPU oracle's.  Pins what the mean sums H
must count: every listed rating, duplicates of a (user, item) pair included."""
import numpy as np
import pytest

import gauss_bias_sums_reference as ref
from oracle import cavi_oracle as orc


def _problem(seed, U, I, N, K, dup):
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, U, N), rng.integers(0, I, N)
    u[u == 3] = 4                       # user 3, items 5 and I - 2: no ratings
    i[(i == 5) | (i == I - 2)] = 6
    if dup:                             # every fifth rating again, some of them three times, with other values
        k = np.arange(0, N, 5)
        u, i = np.concatenate([u, u[k], u[k[::3]]]), np.concatenate([i, i[k], i[k[::3]]])
    x = rng.normal(3.5, 1.0, u.size)
    st = dict(m_u=rng.normal(0, 0.4, (U, K)), m_i=rng.normal(0, 0.4, (I, K)),
              b_u=rng.normal(0, 2.0, U), b_i=rng.normal(0, 1.0, I))
    return u, i, x, st


@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("K", [1, 7, 64])
def test_sums_form_equals_residual_form(K, dup):
    U, I = 60, 25
    u, i, x, st = _problem(K, U, I, 900, K, dup)
    if dup:
        pairs = np.stack([u, i], 1)
        assert np.unique(pairs, axis=0).shape[0] < pairs.shape[0]
    for rows, other, n, ms, mo, bs, bo in ((i, u, I, st["m_i"], st["m_u"], st["b_i"], st["b_u"]),
                                           (u, i, U, st["m_u"], st["m_i"], st["b_u"], st["b_i"])):
        a = ref.bias_sweep(rows, other, x, n, ms, mo, bs, bo, 0.3, 1.0, form="residual")
        b = ref.bias_sweep(rows, other, x, n, ms, mo, bs, bo, 0.3, 1.0, form="sums")
        assert np.max(np.abs(a - b)) <= 1e-12
        empty = np.bincount(rows, minlength=n) == 0
        assert empty.any() and np.array_equal(a[empty], bs[empty]) and np.array_equal(b[empty], bs[empty])
        # the residual form is the oracle's sweep
        ptr, pos = orc.group_positions(rows, n)
        want = orc.gauss_bias_sweep_rows(bs, bo, ms, mo, ptr, pos, other, x, 0.3, 1.0)
        assert np.max(np.abs(a - want)) <= 1e-12


def test_duplicates_are_counted_in_the_mean_sums():
    """H from the distinct pairs only is a different number: the agreement above is not vacuous."""
    U, I, K = 60, 25, 7
    u, i, x, st = _problem(2, U, I, 900, K, True)
    H = ref.mean_sums(i, u, I, st["m_u"])
    _, first = np.unique(np.stack([u, i], 1), axis=0, return_index=True)
    H_distinct = ref.mean_sums(i[first], u[first], I, st["m_u"])
    assert np.max(np.abs(H - H_distinct)) > 0.1
    for r in range(I):
        assert np.allclose(H[r], st["m_u"][u[i == r]].sum(axis=0), atol=1e-13)
