"""NumPy reference of `pmf_topk_query` / `pmf_rank_query`: the score matrix of query rows against candidate rows under a
`score` mode, and from it the k best candidates and the ranks of targets with per-ROW exclusion lists.  Order: score
descending, ties to the lower candidate id (-0.0 == +0.0, as NumPy compares them); a NaN score never ranks."""
import numpy as np

SCORE_DOT, SCORE_BIAS, SCORE_SCALE, SCORE_COSINE = 0, 1, 2, 4


def inv_norm(F):
    """1 / sqrt(sum_k f_k^2) per row, float64 (a zero row gives inf)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1.0 / np.sqrt(np.sum(np.asarray(F, dtype=np.float64) ** 2, axis=1))


def score_matrix(Q, B, score=SCORE_DOT, cq=None, cb=None):
    """full[q, j] of query row q (rows of `Q`, coefficients `cq`) against candidate j (rows of `B`, coefficients `cb`),
    float64, in the device's order of operations."""
    Q, B = np.asarray(Q, dtype=np.float64), np.asarray(B, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        dot = Q @ B.T
        if score == SCORE_BIAS:
            return np.asarray(cq)[:, None] + np.asarray(cb)[None, :] + dot
        if score == SCORE_SCALE:
            return dot * (np.asarray(cq)[:, None] * np.asarray(cb)[None, :])
        if score == SCORE_COSINE:
            return dot * (inv_norm(Q)[:, None] * inv_norm(B)[None, :])
    return dot


def _candidates(s, excluded):
    ok = ~np.isnan(s)
    if excluded is not None and len(excluded):
        ok[np.asarray(list(excluded), dtype=np.int64)] = False
    return ok


def topk(full, k, exclude=None):
    """`full[q]`: the scores of query row q.  `exclude`: per query row an iterable of candidate ids (any order, repeats
    allowed), or None.  Returns (ids int32 [n, k], scores float64 [n, k]), -1 / 0.0 where fewer than k remain."""
    full = np.asarray(full, dtype=np.float64)
    all_ids = np.arange(full.shape[1])
    ids = np.full((len(full), k), -1, dtype=np.int32)
    scores = np.zeros((len(full), k), dtype=np.float64)
    for q, s in enumerate(full):
        cand = all_ids[_candidates(s, None if exclude is None else exclude[q])]
        order = cand[np.lexsort((cand, -s[cand]))][:k]      # stable in (-score, id)
        ids[q, :len(order)] = order
        scores[q, :len(order)] = s[order]
    return ids, scores


def ranks(full, targets, exclude=None):
    """`targets[q]`: the target ids of query row q.  Returns (ranks int64, flat in row order; -1 for a target whose own
    score is NaN), (candidates int64 [n]).  Exclusion applies to competitors only."""
    full = np.asarray(full, dtype=np.float64)
    all_ids = np.arange(full.shape[1])
    out, cand = [], []
    with np.errstate(invalid="ignore"):
        for q, s in enumerate(full):
            ok = _candidates(s, None if exclude is None else exclude[q])
            cand.append(int(ok.sum()))
            for t in targets[q]:
                if np.isnan(s[t]):
                    out.append(-1)
                    continue
                beats = ((s > s[t]) | ((s == s[t]) & (all_ids < t))) & ok & (all_ids != t)
                out.append(int(beats.sum()))
    return np.asarray(out, dtype=np.int64), np.asarray(cand, dtype=np.int64)


def csr(lists):
    """per-row lists -> (row_ptr int64, ids int64)"""
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    ids = np.concatenate([np.asarray(list(v), dtype=np.int64) for v in lists]) if len(lists) else np.zeros(0, dtype=np.int64)
    return ptr, ids.astype(np.int64)


def cosine_tables(U, I, K, seed):
    """Tables on which cosine is exact in fp32: entries in {0, +-1, +-2}, every row with exactly 1, 4, 16 or 64 nonzeros
    (as many as K allows) of one magnitude, so that sum f^2 is a power of 4 and the inverse norm a power of two.  Planted:
    B[1] = 2 B[0] (an exact cosine tie for every query, lower id first), A[1] = 2 A[0], and a zero row in each table
    (`zero_rows`)."""
    rng = np.random.default_rng(seed)
    counts = [n for n in (1, 4, 16, 64) if n <= K]

    def table(rows):
        T = np.zeros((rows, K))
        for r in range(rows):
            n, mag = counts[rng.integers(len(counts))], float(rng.integers(1, 3))
            at = rng.permutation(K)[:n]
            T[r, at] = mag * rng.choice([-1.0, 1.0], n)
        T[0] = np.where(T[0] != 0, np.sign(T[0]), 0.0)       # magnitude 1, so that twice it stays in the alphabet
        T[1] = 2.0 * T[0]
        T[zero_rows(rows)] = 0.0
        return T
    return table(U), table(I)


def zero_rows(rows):
    return min(5, rows - 1)
