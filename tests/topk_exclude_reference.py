"""NumPy reference of `pmf_topk_items_excluding`: the k best candidates per query user, best first, where a user's
excluded items and the items whose score is NaN are no candidates; score descending, ties to the lower item id
(-0.0 == +0.0, as NumPy compares them); -1 / 0.0 where fewer than k candidates remain."""
import numpy as np


def topk_excluding(full, users, train, k):
    """`full[u, j]`: score of item j for user u.  `users`: the query users (repeats allowed).  `train`: user -> iterable
    of that user's excluded items (a missing user excludes nothing), or None.  Returns (items int32 [n, k], scores
    float64 [n, k])."""
    full = np.asarray(full, dtype=np.float64)
    ids = np.arange(full.shape[1])
    items = np.full((len(users), k), -1, dtype=np.int32)
    scores = np.zeros((len(users), k), dtype=np.float64)
    for r, u in enumerate(users):
        s = full[int(u)]
        ok = ~np.isnan(s)
        if train is not None and len(train.get(int(u), ())):
            ok[np.fromiter(train[int(u)], dtype=np.int64)] = False
        cand = ids[ok]
        order = cand[np.lexsort((cand, -s[cand]))][:k]      # stable in (-score, item id)
        items[r, :len(order)] = order
        scores[r, :len(order)] = s[order]
    return items, scores


def train_sets(users, items):
    """user -> set of its items, from (possibly repeated) training pairs"""
    out = {}
    for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        out.setdefault(int(u), set()).add(int(i))
    return out
