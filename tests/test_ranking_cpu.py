"""Host side of the ranking evaluation: the (user, item) pairs -> CSR batch helper of `pmf_hip.engine` and
`src.evaluation.ranking.ranking_metrics`, both pure NumPy (no GPU, no library)."""
import numpy as np
import pytest


def _check_batch(u, i):
    from pmf_hip.engine import rank_batch
    users, row_ptr, items, order = rank_batch(u, i)
    u, i = np.asarray(u), np.asarray(i)
    assert np.array_equal(users, np.unique(u))                      # sorted, distinct
    assert row_ptr.dtype == np.int64 and row_ptr[0] == 0 and row_ptr[-1] == len(u) and (np.diff(row_ptr) >= 0).all()
    assert len(row_ptr) == len(users) + 1
    assert sorted(order.tolist()) == list(range(len(u)))            # a permutation of the input positions
    assert np.array_equal(items, i[order])
    assert np.array_equal(np.repeat(users, np.diff(row_ptr)), u[order])
    for r in range(len(users)):                                     # a user's items keep their input order
        assert np.array_equal(order[row_ptr[r]:row_ptr[r + 1]], np.nonzero(u == users[r])[0])
    back = np.empty(len(u), dtype=np.int64)                         # out[order] = batch result undoes the grouping
    back[order] = items
    assert np.array_equal(back, i)


def test_rank_batch_round_trips_pairs():
    rng = np.random.default_rng(0)
    _check_batch(rng.integers(0, 50, 400), rng.integers(0, 1000, 400))          # repeated users, unsorted input
    _check_batch([7, 3, 7, 7, 9, 3], [1, 2, 3, 1, 5, 0])                         # user 9 has one target; a repeated pair
    _check_batch([4], [2])
    from pmf_hip.engine import rank_batch
    users, row_ptr, items, order = rank_batch([], [])                            # the empty input
    assert len(users) == 0 and row_ptr.tolist() == [0] and len(items) == 0 and len(order) == 0
    with pytest.raises(ValueError):
        rank_batch([1, 2], [1])


def _brute(user_ids, ranks, cand, ks):
    out = {"n_skipped": 0, "n_pairs": 0}
    per = {name: [] for name in ["mrr", "percentile"] + [f"{m}@{k}" for k in ks for m in ("recall", "precision", "hit_rate", "ndcg")]}
    for uu in sorted(set(user_ids)):
        mine = [n for n in range(len(user_ids)) if user_ids[n] == uu]
        r = [int(ranks[n]) for n in mine if ranks[n] >= 0]
        out["n_skipped"] += len(mine) - len(r)
        out["n_pairs"] += len(r)
        if not r:
            continue
        T, c = len(r), int(cand[mine[0]])
        for k in ks:
            hits = sum(x < k for x in r)
            per[f"recall@{k}"].append(hits / T)
            per[f"precision@{k}"].append(hits / k)
            per[f"hit_rate@{k}"].append(float(hits > 0))
            per[f"ndcg@{k}"].append(sum(1 / np.log2(x + 2) for x in r if x < k) / sum(1 / np.log2(p + 2) for p in range(min(T, k))))
        per["mrr"].append(1 / (min(r) + 1))
        per["percentile"].append(np.mean(r) / max(c - 1, 1))
    out["n_users"] = len(per["mrr"])
    out.update({name: float(np.mean(v)) if v else float("nan") for name, v in per.items()})
    return out


def test_ranking_metrics_on_a_hand_computed_example():
    from src.evaluation.ranking import ranking_metrics
    # user 10: ranks 0 and 4 of 11 candidates; user 20: rank 2 of 101; user 30: ranks 1, 3 (and one unranked pair) of 5
    users = [10, 20, 10, 30, 30, 30]
    ranks = [0, 2, 4, 1, -1, 3]
    cand = [11, 101, 11, 5, 5, 5]
    m = ranking_metrics(users, ranks, cand, ks=(1, 3))
    assert (m["n_users"], m["n_pairs"], m["n_skipped"]) == (3, 5, 1)
    assert m["recall@1"] == pytest.approx((1 / 2 + 0 + 0) / 3)
    assert m["precision@1"] == pytest.approx((1 + 0 + 0) / 3)
    assert m["hit_rate@1"] == pytest.approx(1 / 3)
    assert m["ndcg@1"] == pytest.approx((1.0 + 0 + 0) / 3)
    assert m["recall@3"] == pytest.approx((1 / 2 + 1 + 1 / 2) / 3)
    assert m["precision@3"] == pytest.approx((1 / 3 + 1 / 3 + 1 / 3) / 3)
    assert m["hit_rate@3"] == 1.0
    ideal2 = 1 + 1 / np.log2(3)
    assert m["ndcg@3"] == pytest.approx((1 / ideal2 + (1 / np.log2(4)) / 1 + (1 / np.log2(3)) / ideal2) / 3)
    assert m["mrr"] == pytest.approx((1 + 1 / 3 + 1 / 2) / 3)
    assert m["percentile"] == pytest.approx((2 / 10 + 2 / 100 + 2 / 4) / 3)


def test_ranking_metrics_match_a_brute_force_implementation():
    from src.evaluation.ranking import ranking_metrics
    rng = np.random.default_rng(3)
    n_users, ks = 40, (1, 5, 10)
    users = rng.integers(0, n_users, 600) * 3 + 1          # ~15 targets per user: T > k for every k
    cand_of = rng.integers(20, 60, n_users * 3 + 1)
    cand_of[users[0]] = 1                                  # candidates = 1: the percentile's denominator is clamped
    cand = cand_of[users]
    ranks = rng.integers(0, 20, 600)
    ranks[users == users[0]] = 0
    ranks[rng.random(600) < 0.1] = -1                      # unranked pairs
    ranks[users == users[1]] = -1                          # a user whose targets are all unranked: not averaged over
    got, want = ranking_metrics(users, ranks, cand, ks=ks), _brute(users.tolist(), ranks, cand, ks)
    assert set(got) == set(want)
    assert want["n_users"] == len(set(users.tolist())) - 1 and want["n_skipped"] > 0
    for name in want:
        assert got[name] == pytest.approx(want[name], rel=1e-12, abs=0), name
    empty = ranking_metrics([1, 2], [-1, -1], [5, 5], ks=(3,))
    assert (empty["n_users"], empty["n_pairs"], empty["n_skipped"]) == (0, 0, 2) and np.isnan(empty["recall@3"])
