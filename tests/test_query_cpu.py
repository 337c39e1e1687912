"""The NumPy reference of the query calls (tests/query_reference.py) and the exact cosine tables, checked without a GPU."""
import numpy as np
import pytest

import query_reference as qr
from topk_exclude_reference import topk_excluding


def test_dot_reference_equals_the_excluding_reference_on_integer_tables():
    rng = np.random.default_rng(3)
    U, I, K, k = 23, 41, 7, 9
    A, B = rng.integers(-2, 3, (U, K)).astype(float), rng.integers(-2, 3, (I, K)).astype(float)
    B[3] = np.nan
    B[I - 2] = B[1]
    users = rng.integers(0, U, 30)
    train = {u: set(rng.permutation(I)[:rng.integers(0, I)].tolist()) for u in range(0, U, 2)}
    train[1] = set(range(I))
    with np.errstate(invalid="ignore"):
        full = A @ B.T
    want = topk_excluding(full, users, train, k)
    got = qr.topk(qr.score_matrix(A[users], B), k, exclude=[train.get(int(u), ()) for u in users])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ranks are the positions of the top-k
    ids, _ = got
    targets = [row[row >= 0].tolist() for row in ids]
    r, c = qr.ranks(qr.score_matrix(A[users], B), targets, exclude=[train.get(int(u), ()) for u in users])
    assert np.array_equal(r, np.concatenate([np.arange(len(t)) for t in targets]))
    assert np.array_equal(c, [(~np.isnan(full[u])).sum() - len(train.get(int(u), set()) - {3}) for u in users])


@pytest.mark.parametrize("K", [20, 64])
def test_cosine_tables_have_power_of_two_inverse_norms_and_exact_fp32_scores(K):
    A, B = qr.cosine_tables(40, 33, K, seed=K)
    for T in (A, B):
        assert set(np.unique(T)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        nz = (T != 0).sum(axis=1)
        assert set(nz.tolist()) <= {0, 1, 4, 16, 64} and (nz == 0).sum() == 1
        assert all(len(set(np.abs(row[row != 0]))) <= 1 for row in T)
        inv = qr.inv_norm(T)
        finite = np.isfinite(inv)
        m, e = np.frexp(inv[finite])
        assert (m == 0.5).all()                                           # a power of two
        assert np.isinf(inv[qr.zero_rows(len(T))])
        assert np.array_equal(T[1], 2.0 * T[0])
    # fp32 arithmetic in the device's order gives the float64 reference exactly
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_a = np.float32(1) / np.sqrt((A32 * A32).sum(axis=1, dtype=np.float32))
        inv_b = np.float32(1) / np.sqrt((B32 * B32).sum(axis=1, dtype=np.float32))
        s32 = (A32 @ B32.T) * (inv_a[:, None] * inv_b[None, :])
    assert s32.dtype == np.float32
    full = qr.score_matrix(A, B, qr.SCORE_COSINE)
    assert np.array_equal(s32.astype(np.float64), full, equal_nan=True)
    assert np.isnan(full[qr.zero_rows(40)]).all() and np.isnan(full[:, qr.zero_rows(33)]).all()
    assert np.array_equal(full[:, 0], full[:, 1], equal_nan=True)           # the planted tie
    ids, scores = qr.topk(full, 5)
    assert (ids[qr.zero_rows(40)] == -1).all() and not (ids == qr.zero_rows(33)).any()
