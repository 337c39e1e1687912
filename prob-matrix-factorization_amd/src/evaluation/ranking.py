"""Ranking metrics from held-out item ranks (no reference counterpart: `metrics.py` mirrors the reference's point
errors).  Pure NumPy; the ranks come from `pmf_hip.Context.rank_items` / `DeviceModel.heldout_ranks`."""
from __future__ import annotations

import numpy as np


def ranking_metrics(user_ids, ranks, candidates, ks=(10,)):
    """Per user with T ranked targets (pairs with rank -1 are dropped and counted in `n_skipped`), hits_k = #{r < k}:

        recall@k = hits_k / T        precision@k = hits_k / k        hit_rate@k = [hits_k > 0]
        ndcg@k   = sum_{r < k} 1 / log2(r + 2)  /  sum_{p < min(T, k)} 1 / log2(p + 2)
        mrr      = 1 / (min r + 1)   percentile  = mean r / max(candidates - 1, 1)

    each averaged over the users with at least one ranked target.  Returns a dict with `recall@k`, `precision@k`,
    `hit_rate@k`, `ndcg@k` for every k of `ks`, `mrr`, `percentile`, `n_users`, `n_pairs` and `n_skipped`
    (the averages are NaN when no pair is ranked)."""
    u = np.asarray(user_ids).reshape(-1)
    r = np.asarray(ranks, dtype=np.int64).reshape(-1)
    c = np.asarray(candidates, dtype=np.int64).reshape(-1)
    if not (len(u) == len(r) == len(c)):
        raise ValueError("user_ids, ranks and candidates must have the same length")
    keep = r >= 0
    out = {"n_skipped": int((~keep).sum()), "n_pairs": int(keep.sum())}
    u, r, c = u[keep], r[keep], c[keep]
    users, row = np.unique(u, return_inverse=True)
    n = len(users)
    out["n_users"] = n
    mean = lambda per_user: float(per_user.mean()) if n else float("nan")
    T = np.bincount(row, minlength=n)
    gain = 1.0 / np.log2(r + 2.0)
    for k in ks:
        k = int(k)
        hit = r < k
        hits = np.bincount(row, weights=hit, minlength=n)
        ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(k) + 2.0))])[np.minimum(T, k)]
        out[f"recall@{k}"] = mean(hits / np.maximum(T, 1))
        out[f"precision@{k}"] = mean(hits / k)
        out[f"hit_rate@{k}"] = mean((hits > 0).astype(np.float64))
        out[f"ndcg@{k}"] = mean(np.bincount(row, weights=gain * hit, minlength=n) / np.where(T > 0, ideal, 1.0))
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, row, r)
    out["mrr"] = mean(1.0 / (best + 1.0))
    pct = r / np.maximum(c - 1, 1)
    out["percentile"] = mean(np.bincount(row, weights=pct, minlength=n) / np.maximum(T, 1))
    return out


__all__ = ["ranking_metrics"]
