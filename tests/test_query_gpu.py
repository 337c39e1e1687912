"""`pmf_topk_query` / `pmf_rank_query`: top-k and ranks for any query rows against all rows of one side.

Three kinds of check: byte equality with the item calls (`topk_items`, `rank_items`) where the query rows are users and
the candidates items; equality with tests/query_reference.py on tables whose scores are exact in fp32 (small integers;
for cosine the tables of `query_reference.cosine_tables`); and, at model level, agreement with NumPy on what the fold-in
records predict, to the tolerance of the arithmetic (float64 sums of K products: 1e-12 relative; fp32: 1e-5)."""
import ctypes as C

import numpy as np
import pytest

import query_reference as qr
from helpers import frames, load_case
from test_topk_exclude_gpu import _fill, _tables, _training_pairs
from topk_exclude_reference import train_sets

pytestmark = pytest.mark.gpu

_EDGES = [(5, 7, 3, 7), (40, 33, 16, 10), (33, 64, 8, 1), (64, 64, 64, 64), (130, 95, 128, 50), (257, 1000, 100, 64)]


# ---- helpers ----------------------------------------------------------------------------------------------------------
def _arrays(ctx, side, score):
    """(FACTOR, coefficient array or None) of a side as the device holds them"""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ARR_SCALE
    coef = {pmf_hip.PREDICT_BIAS: ARR_BIAS, pmf_hip.PREDICT_SCALE: ARR_SCALE}.get(score)
    return ctx.get_array(side, ARR_FACTOR), (None if coef is None else ctx.get_array(side, coef))


def _full(ctx, cand_side, score, query_side=None, ids=None, factor=None, coef=None):
    """the reference's score matrix [query rows x candidates] from what the device holds"""
    B, cb = _arrays(ctx, cand_side, score)
    if ids is not None:
        Q, cq = _arrays(ctx, query_side, score)
        Q, cq = Q[ids], (None if cq is None else cq[ids])
    else:
        Q, cq = np.asarray(factor, dtype=ctx.np_dtype).astype(np.float64), coef
    return qr.score_matrix(Q, B, score, cq, cb)


def _messy(lists, rng):
    """the lists shuffled, some entries twice"""
    out = []
    for v in lists:
        v = list(v)
        v = v + [v[j] for j in rng.integers(0, len(v), len(v) // 3 + 1)] if v else v
        out.append(rng.permutation(np.asarray(v, dtype=np.int64)).tolist())
    return out


def _targets(rng, n, C, most=6):
    """0 .. `most` random targets per row (more than the four slots of a device row: the splitting path)"""
    return [rng.integers(0, C, rng.integers(0, most + 1)).tolist() for _ in range(n)]


def _check_both(ctx, cand_side, k, full, lists, targets, **query):
    """topk_query and rank_query against the reference"""
    ex = None if lists is None else qr.csr(lists)
    got = ctx.topk_query(cand_side, k, exclude=ex, **query)
    want = qr.topk(full, k, exclude=lists)
    assert got[0].dtype == np.int32 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    r, c = ctx.rank_query(cand_side, qr.csr(targets), exclude=ex, **query)
    want_r, want_c = qr.ranks(full, targets, exclude=lists)
    assert np.array_equal(r, want_r)
    assert np.array_equal(c, want_c)
    return got


# ---- 1. byte equality with the item calls -------------------------------------------------------------------------------
_BYTES = [(257, 1000, 100, 64, "f32", 0), (257, 1000, 100, 64, "f32", 1), (257, 1000, 100, 64, "f32", 2),
          (130, 95, 16, 50, "f64", 0), (130, 95, 130, 50, "f32", 0), (257, 1000, 100, 65, "f32", 0)]


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("U,I,K,k,dtype,mode", _BYTES)
def test_users_against_items_gives_the_bytes_of_the_item_calls(U, I, K, k, dtype, mode, exclude):
    """The fused scan, fp64, Kpad > 128 and k > 64 (two-phase): ids and scores of `topk_query` are those of `topk_items`,
    ranks and candidates of `rank_query` those of `rank_items` -- with the training lists handed over shuffled and with
    repeats where the item calls read the context's own."""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ARR_SCALE, ITEM, USER
    rng = np.random.default_rng(U + I + K + k)
    tu, ti = _training_pairs(U, I, seed=U + I)
    users = np.concatenate([rng.permutation(U), rng.integers(0, U, 9)])
    targets = _targets(rng, len(users), I)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_array(USER, ARR_FACTOR, rng.normal(size=(U, K))); ctx.set_array(ITEM, ARR_FACTOR, rng.normal(size=(I, K)))
        for arr in ([ARR_BIAS] if mode == 1 else [ARR_SCALE] if mode == 2 else []):
            ctx.set_array(USER, arr, rng.normal(size=U)); ctx.set_array(ITEM, arr, rng.normal(size=I))
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        train = train_sets(tu, ti)
        ex = qr.csr(_messy([sorted(train.get(int(u), ())) for u in users], rng)) if exclude else None
        want = ctx.topk_items(users, k, use_bias=mode, exclude_train=exclude)
        got = ctx.topk_query(ITEM, k, ids=users, query_side=USER, score=mode, exclude=ex)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        tp, tids = qr.csr(targets)
        want = ctx.rank_rows(users, tp, tids, use_bias=mode, exclude_train=exclude)
        got = ctx.rank_query(ITEM, (tp, tids), ids=users, query_side=USER, score=mode, exclude=ex)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ---- 2. the caller's rows equal the context's rows ------------------------------------------------------------------------
@pytest.mark.parametrize("U,I,K,k,dtype", [(257, 1000, 100, 64, "f32"), (130, 95, 16, 50, "f64")])
def test_vector_mode_gives_the_bytes_of_ids_mode(U, I, K, k, dtype):
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(U + K)
    ids = np.concatenate([rng.permutation(U), rng.integers(0, U, 9)])
    lists = [rng.integers(0, I, rng.integers(0, 20)).tolist() for _ in ids]
    targets = _targets(rng, len(ids), I)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_array(USER, ARR_FACTOR, rng.normal(size=(U, K))); ctx.set_array(ITEM, ARR_FACTOR, rng.normal(size=(I, K)))
        ctx.set_array(USER, ARR_BIAS, rng.normal(size=U)); ctx.set_array(ITEM, ARR_BIAS, rng.normal(size=I))
        factor, coef = ctx.get_array(USER, ARR_FACTOR)[ids], ctx.get_array(USER, ARR_BIAS)[ids]
        for score in (0, pmf_hip.PREDICT_BIAS, pmf_hip.SCORE_COSINE):
            by_id = dict(ids=ids, query_side=USER, score=score, exclude=qr.csr(lists))
            by_row = dict(factor=factor, coef=coef, score=score, exclude=qr.csr(lists))
            a, b = ctx.topk_query(ITEM, k, **by_id), ctx.topk_query(ITEM, k, **by_row)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            a, b = ctx.rank_query(ITEM, qr.csr(targets), **by_id), ctx.rank_query(ITEM, qr.csr(targets), **by_row)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 3. the reference on exact tables: users as candidates, one side against itself ----------------------------------------
@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("U,I,K,k", _EDGES)
def test_either_side_as_candidates_equals_the_reference(U, I, K, k, max_blocks, monkeypatch):
    """Small-integer tables (two identical item rows, a NaN item row, a zero user row): items query users under every
    score, items against items and users against users with the row itself left out."""
    import pmf_hip
    from pmf_hip import ITEM, USER
    if max_blocks:
        monkeypatch.setenv("PMF_TOPK_MAX_BLOCKS", str(max_blocks))
    A, B, bias, scale = _tables(U, I, K, seed=1000 * U + I + K, counts=K == 16)
    rng = np.random.default_rng(U * I)
    for mode in (0, pmf_hip.PREDICT_BIAS, pmf_hip.PREDICT_SCALE):
        with pmf_hip.Context(U, I, K) as ctx:
            _fill(ctx, A, B, bias, scale, mode)
            items = np.concatenate([rng.permutation(I), rng.integers(0, I, 3)])
            lists = [rng.integers(0, U, rng.integers(0, U + 1)).tolist() for _ in items]
            full = _full(ctx, USER, mode, query_side=ITEM, ids=items)
            _check_both(ctx, USER, min(k, U), full, lists, _targets(rng, len(items), U), ids=items, query_side=ITEM, score=mode)
            if mode:
                continue
            for side, n in ((ITEM, I), (USER, U)):
                ids = rng.permutation(n)
                full = _full(ctx, side, 0, query_side=side, ids=ids)
                got = _check_both(ctx, side, min(k, n), full, [[int(q)] for q in ids], _targets(rng, n, n), ids=ids,
                                  query_side=side, score=0)
                assert not (got[0] == ids[:, None]).any()                       # the row itself is left out


# ---- 4. cosine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("U,I", [(40, 33), (257, 1000)])
@pytest.mark.parametrize("K", [20, 64])
def test_cosine_equals_the_reference_on_exact_tables(K, U, I, dtype, two_phase, monkeypatch):
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    if two_phase:
        monkeypatch.setenv("PMF_TOPK_TWO_PHASE", "1")
    A, B = qr.cosine_tables(U, I, K, seed=U + K)
    rng = np.random.default_rng(K)
    k = 10
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_array(USER, ARR_FACTOR, A); ctx.set_array(ITEM, ARR_FACTOR, B)
        ids = rng.permutation(U)
        lists = [rng.integers(0, I, rng.integers(0, 8)).tolist() for _ in ids]
        targets = _targets(rng, U, I)
        full = _full(ctx, ITEM, qr.SCORE_COSINE, query_side=USER, ids=ids)
        for query in (dict(ids=ids, query_side=USER), dict(factor=A[ids])):
            got = _check_both(ctx, ITEM, k, full, lists, targets, score=pmf_hip.SCORE_COSINE, **query)
            zero = np.flatnonzero(ids == qr.zero_rows(U))[0]
            assert (got[0][zero] == -1).all() and (got[1][zero] == 0.0).all()     # the zero query row
            assert not (got[0] == qr.zero_rows(I)).any()                          # the zero candidate
        # similar items: the planted pair B[1] = 2 B[0] has cosine 1 with each other
        items = np.arange(I)
        full = _full(ctx, ITEM, qr.SCORE_COSINE, query_side=ITEM, ids=items)
        got = _check_both(ctx, ITEM, k, full, [[j] for j in items], _targets(rng, I, I), ids=items, query_side=ITEM,
                          score=pmf_hip.SCORE_COSINE)
        assert got[0][0, 0] == 1 and got[1][0, 0] == 1.0 and got[0][1, 0] == 0


# ---- 5. rounds and per-row lists ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rounds_of_32_rows_with_a_list_per_row(dtype, monkeypatch):
    """70 query rows in rounds of 32: rows 0 and 40 are the same user with different lists, every row has a list of its
    own, some are empty, one excludes every candidate; rows with more than four targets are cut across rounds."""
    import pmf_hip
    from pmf_hip import ITEM, USER
    monkeypatch.setenv("PMF_TOPK_QUERY_ROWS", "32")
    U, I, K, k, n = 50, 90, 16, 12, 70
    A, B, bias, scale = _tables(U, I, K, seed=5, counts=True)
    rng = np.random.default_rng(11)
    ids = rng.integers(0, U, n)
    ids[40] = ids[0]
    lists = [rng.permutation(I)[:rng.integers(1, I // 2)].tolist() for _ in range(n)]
    lists[3], lists[31], lists[32], lists[69] = [], [], [], []
    lists[33] = list(range(I))
    targets = _targets(rng, n, I)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        _fill(ctx, A, B, bias, scale, pmf_hip.PREDICT_BIAS)
        full = _full(ctx, ITEM, pmf_hip.PREDICT_BIAS, query_side=USER, ids=ids)
        best = int(np.nanargmax(full[0]))                                  # the same user twice: one row excludes its best item
        lists[0] = [best] + [j for j in lists[0] if j != best]
        lists[40] = [j for j in lists[40] if j != best]
        factor, coef = _arrays(ctx, USER, pmf_hip.PREDICT_BIAS)
        for query in (dict(ids=ids, query_side=USER), dict(factor=factor[ids], coef=coef[ids])):
            got = _check_both(ctx, ITEM, k, full, _messy(lists, rng), targets, score=pmf_hip.PREDICT_BIAS, **query)
            assert (got[0][33] == -1).all()
            assert not np.array_equal(got[0][0], got[0][40])


# ---- 6. a segmented candidate range --------------------------------------------------------------------------------------------
def _segment_bounds(n_rows, C):
    """first candidates of the segments of a fused scan (topk_segments in csrc/pmf_topk.hip)"""
    waves = (n_rows + 31) // 32
    nseg = min(64, max(1, 4096 // waves))
    nseg = min(nseg, max(1, C // 2048))
    seg = ((C + nseg - 1) // nseg + 31) // 32 * 32
    return list(range(seg, C, seg))


@pytest.mark.parametrize("U,I,K,k", [(3, 6200, 20, 10), (129, 4097, 12, 3)])
def test_exclusion_on_both_sides_of_every_segment_boundary(U, I, K, k):
    import pmf_hip
    from pmf_hip import ITEM, USER
    bounds = _segment_bounds(U, I)
    assert bounds                                                          # the range IS cut at these shapes
    A, B, bias, scale = _tables(U, I, K, seed=U + I)
    rng = np.random.default_rng(U)
    edge = [b + d for b in bounds for d in (-2, -1, 0, 1)]
    B[edge] = 2.0                                                          # ... and the boundary rows score high
    ids = np.arange(U)
    lists = [[b - 1 for b in bounds] + [b for b in bounds] + rng.integers(0, I, 40).tolist() if q % 3 != 2 else
             [b - 1 for b in bounds] for q in ids]
    with pmf_hip.Context(U, I, K) as ctx:
        _fill(ctx, A, B, bias, scale, 0)
        full = _full(ctx, ITEM, 0, query_side=USER, ids=ids)
        _check_both(ctx, ITEM, k, full, lists, [edge[:6] for _ in ids], ids=ids, query_side=USER, score=0)


# ---- 7. position is the rank ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank_targets", [0, 1])
@pytest.mark.parametrize("score", ["cosine", "bias"])
@pytest.mark.parametrize("U,I,K,k,dtype", [(257, 1000, 100, 64, "f32"), (130, 95, 16, 50, "f64")])
def test_the_position_in_topk_query_is_the_rank_of_rank_query(U, I, K, k, dtype, score, rank_targets, monkeypatch):
    """Random normal tables, the caller's rows, per-row exclusion: column p of a row holds the candidate of rank p, and
    min(k, candidates) entries are valid.  Some candidate rows are copies of others (exact ties) and one is NaN."""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, USER
    if rank_targets:
        monkeypatch.setenv("PMF_RANK_TARGETS", str(rank_targets))
    score = pmf_hip.SCORE_COSINE if score == "cosine" else pmf_hip.PREDICT_BIAS
    rng = np.random.default_rng(U + rank_targets)
    B = rng.normal(size=(I, K))
    B[I // 2:I // 2 + 20] = B[:20]
    B[7] = np.nan
    bias_i = rng.normal(size=I)
    bias_i[I // 2:I // 2 + 20] = bias_i[:20]
    n = 70
    factor, coef = rng.normal(size=(n, K)), rng.normal(size=n)
    lists = [rng.integers(0, I, rng.integers(0, 60)).tolist() for _ in range(n)]
    lists[5] = rng.permutation(I)[:I - 20].tolist()                        # fewer than k candidates left
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_array(USER, ARR_FACTOR, rng.normal(size=(U, K))); ctx.set_array(ITEM, ARR_FACTOR, B)
        ctx.set_array(USER, ARR_BIAS, rng.normal(size=U)); ctx.set_array(ITEM, ARR_BIAS, bias_i)
        query = dict(factor=factor, coef=coef, score=score, exclude=qr.csr(lists))
        ids, _ = ctx.topk_query(ITEM, k, **query)
        valid = ids >= 0
        targets = [row[row >= 0].tolist() for row in ids]
        ranks, cand = ctx.rank_query(ITEM, qr.csr(targets), **query)
    assert np.array_equal(valid.sum(axis=1), np.minimum(k, cand))
    assert (valid[:, :-1] >= valid[:, 1:]).all()                             # the valid entries come first
    assert np.array_equal(ranks, np.nonzero(valid)[1])
    assert cand[5] <= 20 and valid[5].sum() == cand[5]


# ---- 8. the contract -----------------------------------------------------------------------------------------------------------
def _raw(ctx, fn, cand_side, n, query_side, ids, factor, coef, score, ex, tail):
    """a direct call: (status, message)"""
    import pmf_hip
    from pmf_hip import ptr
    lib = pmf_hip.load()
    opt = lambda a, t: None if a is None else ptr(a, t)
    rc = getattr(lib, fn)(ctx._h, cand_side, n, query_side, opt(ids, C.c_int32), opt(factor, C.c_double), opt(coef, C.c_double),
                          score, opt(None if ex is None else ex[0], C.c_int64), opt(None if ex is None else ex[1], C.c_int32), *tail)
    return rc, (lib.pmf_last_error() or b"").decode()


def test_argument_errors_name_the_fault_and_write_nothing():
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, USER, ptr
    U, I, K, k, n = 20, 30, 8, 5, 4
    EINVAL, ERANGE = -1, -4
    rng = np.random.default_rng(0)
    ids = np.array([0, 3, 3, 19], dtype=np.int32)
    factor, coef = rng.normal(size=(n, K)), rng.normal(size=n)
    ex = (np.array([0, 1, 1, 2, 3], dtype=np.int64), np.array([2, 29, 0], dtype=np.int32))
    tgt = (np.array([0, 1, 2, 2, 3], dtype=np.int64), np.array([1, 2, 3], dtype=np.int32))
    with pmf_hip.Context(U, I, K) as ctx:
        ctx.set_array(USER, ARR_FACTOR, rng.normal(size=(U, K))); ctx.set_array(ITEM, ARR_FACTOR, rng.normal(size=(I, K)))
        out_i, out_s = np.full((n, k), -7, dtype=np.int32), np.full((n, k), -7.0)
        out_r, out_c = np.full(3, -7, dtype=np.int64), np.full(n, -7, dtype=np.int64)
        topk_tail = lambda kk=k: (kk, ptr(out_i, C.c_int32), ptr(out_s, C.c_double))
        rank_tail = lambda t=tgt: (None if t[0] is None else ptr(t[0], C.c_int64), None if t[1] is None else ptr(t[1], C.c_int32),
                                   ptr(out_r, C.c_int64), ptr(out_c, C.c_int64))
        bad_ex0 = (np.array([1, 1, 1, 2, 3], dtype=np.int64), ex[1])
        bad_ex1 = (np.array([0, 2, 1, 2, 3], dtype=np.int64), ex[1])
        far_ex = (ex[0], np.array([2, 30, 0], dtype=np.int32))
        cases = [   # (cand_side, query_side, ids, factor, coef, score, ex), status, message part
            ((2, USER, ids, None, None, 0, None), EINVAL, "bad cand_side 2"),
            ((ITEM, 5, ids, None, None, 0, None), EINVAL, "bad query_side 5"),
            ((ITEM, USER, ids, factor, None, 0, None), EINVAL, "both query_ids and query_factor"),
            ((ITEM, USER, None, None, None, 0, None), EINVAL, "neither query_ids nor query_factor"),
            ((ITEM, USER, None, factor, None, pmf_hip.PREDICT_BIAS, None), EINVAL, "null query_coef"),
            ((ITEM, USER, ids, None, None, 3, None), EINVAL, "score must be"),
            ((ITEM, ITEM, ids, None, None, pmf_hip.PREDICT_BIAS, None), EINVAL, "query_side == cand_side"),
            ((ITEM, USER, ids, None, None, pmf_hip.PREDICT_BIAS, None), EINVAL, "BIAS"),
            ((ITEM, USER, ids, None, None, 0, bad_ex0), EINVAL, "ex_ptr[0] = 1"),
            ((ITEM, USER, ids, None, None, 0, bad_ex1), EINVAL, "ex_ptr decreases at row 1"),
            ((ITEM, USER, np.array([0, 3, 20, 19], dtype=np.int32), None, None, 0, None), ERANGE, "query id 20 at position 2"),
            ((ITEM, USER, ids, None, None, 0, far_ex), ERANGE, "excluded id 30 at position 1"),
        ]
        for fn, tail in (("pmf_topk_query", topk_tail()), ("pmf_rank_query", rank_tail())):
            for (cs, qs, i_, f_, c_, sc, e_), status, part in cases:
                rc, msg = _raw(ctx, fn, cs, n, qs, i_, f_, c_, sc, e_, tail)
                assert rc == status and part in msg and fn in msg, (fn, part, rc, msg)
        for kk in (0, I + 1, 1025):
            rc, msg = _raw(ctx, "pmf_topk_query", ITEM, n, USER, ids, None, None, 0, None, topk_tail(kk))
            assert rc == ERANGE and f"k={kk}" in msg
        rc, msg = _raw(ctx, "pmf_rank_query", ITEM, n, USER, ids, None, None, 0, None,
                       rank_tail((tgt[0], np.array([1, 30, 3], dtype=np.int32))))
        assert rc == ERANGE and "target id 30 at position 1" in msg
        rc, msg = _raw(ctx, "pmf_rank_query", ITEM, n, USER, ids, None, None, 0, None,
                       rank_tail((np.array([0, 2, 1, 2, 3], dtype=np.int64), tgt[1])))
        assert rc == EINVAL and "tgt_ptr decreases at row 1" in msg
        rc, msg = _raw(ctx, "pmf_rank_query", ITEM, n, USER, ids, None, None, 0, None, rank_tail((None, tgt[1])))
        assert rc == EINVAL and "null tgt_ptr" in msg
        lib = pmf_hip.load()
        assert lib.pmf_topk_query(None, ITEM, n, USER, ptr(ids, C.c_int32), None, None, 0, None, None, *topk_tail()) == EINVAL
        assert b"null context" in lib.pmf_last_error()
        # n_query = 0 touches nothing, whatever else is passed
        assert _raw(ctx, "pmf_topk_query", ITEM, 0, USER, None, None, None, 0, None, (k, None, None))[0] == 0
        assert _raw(ctx, "pmf_rank_query", ITEM, 0, USER, None, None, None, 0, None, (None, None, None, None))[0] == 0
        for out in (out_i, out_s, out_r, out_c):
            assert (out == -7).all()
    with pmf_hip.Context(U, I, K) as ctx:                                   # a missing FACTOR array
        ctx.set_array(USER, ARR_FACTOR, rng.normal(size=(U, K)))
        with pytest.raises(pmf_hip.PmfError, match="FACTOR"):
            ctx.topk_query(ITEM, k, ids=ids, query_side=USER)
        with pytest.raises(pmf_hip.PmfError, match="FACTOR"):
            ctx.topk_query(USER, k, ids=ids, query_side=ITEM)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_calls_read_the_context_only_and_repeat_to_the_bit(dtype):
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    U, I, K, k = 130, 95, 16, 20
    rng = np.random.default_rng(1)
    A, B = rng.normal(size=(U, K)), rng.normal(size=(I, K))
    A[3] = np.nan
    users = rng.permutation(U)
    lists = [rng.integers(0, I, rng.integers(0, 30)).tolist() for _ in users]
    targets = _targets(rng, U, I)
    tu, ti = _training_pairs(U, I, seed=2)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_array(USER, ARR_FACTOR, A); ctx.set_array(ITEM, ARR_FACTOR, B)
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        before = [ctx.get_array(USER, ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)]
        old = ctx.topk_items(users, k, exclude_train=True), ctx.rank_items(tu[:200], ti[:200], exclude_train=True)

        def calls():
            out = []
            for score in (0, pmf_hip.SCORE_COSINE):
                query = dict(score=score, exclude=qr.csr(lists))
                out += ctx.topk_query(ITEM, k, ids=users, query_side=USER, **query)
                out += ctx.topk_query(ITEM, k, factor=A[users], **query)
                out += ctx.rank_query(ITEM, qr.csr(targets), ids=users, query_side=USER, **query)
                out += ctx.topk_query(ITEM, k, ids=np.arange(I), query_side=ITEM, **dict(query, exclude=None))
            return [a.tobytes() for a in out]
        first = calls()
        grown = ctx.device_bytes()
        assert calls() == first
        assert ctx.device_bytes() == grown                                 # the staging buffers are sized by the first call
        after = [ctx.get_array(USER, ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)]
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
        new = ctx.topk_items(users, k, exclude_train=True), ctx.rank_items(tu[:200], ti[:200], exclude_train=True)
        assert all(a.tobytes() == b.tobytes() for x, y in zip(old, new) for a, b in zip(x, y))


# ---- 9. model level ------------------------------------------------------------------------------------------------------------
def _fit(case, dtype):
    d, meta = load_case(case)
    train, _ = frames(d)
    kw = dict(meta["base_cfg"], n_factors=meta["K"], random_state=meta["seed"], max_iter=5, verbose=False)
    if meta["kind"] == "hpf":
        from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
        return HPF_CAVI(HPF_CAVI_Config(tol=None, **kw), dtype=dtype).fit(train), train
    from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
    return GaussianMFCAVI(GaussianMFCAVIConfig(tol=0.0, **kw), dtype=dtype).fit(train, global_mean=float(d["global_mean"])), train


def _new_users(m, train, n=12):
    """a frame of new user labels (>= n_users) whose ratings copy those of existing users"""
    import pandas as pd
    parts = []
    for j, u in enumerate(np.unique(train["u"].to_numpy())[:n]):
        part = train[train["u"] == u].copy()
        part["u"] = m.n_users + 5 + 2 * j
        parts.append(part)
    return pd.concat(parts, ignore_index=True)


def _numpy_topk_check(full, seen, got, k, rtol):
    """the returned scores are the k largest non-seen NumPy scores (sorted vectors: a swap inside a near-tie cannot
    fail), and every returned id's NumPy score is its returned score"""
    ids, scores = got
    for r in range(len(full)):
        s = full[r].copy()
        s[list(seen[r])] = -np.inf
        want = np.sort(s)[::-1][:k]
        assert (ids[r] >= 0).all() and not set(ids[r].tolist()) & set(seen[r])
        np.testing.assert_allclose(np.sort(scores[r])[::-1], want, rtol=rtol, atol=0)
        np.testing.assert_allclose(scores[r], full[r][ids[r]], rtol=rtol, atol=0)


@pytest.mark.parametrize("case", ["hpf_s7_k16", "gauss_bias_s7_k16"])
def test_top_k_for_folded_in_users_matches_fold_predict(case):
    k = 10
    for dtype, rtol in (("f64", 1e-12), ("f32", 1e-5)):
        m, train = _fit(case, dtype)
        try:
            df = _new_users(m, train)
            fold = m.fold_in_users(df, n_iter=3)
            assert fold.side == 0 and len(fold.seen_ptr) == len(fold.ids) + 1
            n = len(fold.ids)
            seen = [set(fold.seen_ids[fold.seen_ptr[r]:fold.seen_ptr[r + 1]].tolist()) for r in range(n)]
            rows, items = np.repeat(np.arange(n), m.n_items), np.tile(np.arange(m.n_items), n)
            full = fold.predict(rows, items).reshape(n, m.n_items)
            ids, scores = m.top_k_for(fold, k=k)
            if dtype == "f64":
                _numpy_topk_check(full, seen, (ids, scores), k, rtol)
            else:
                assert all(not set(ids[r].tolist()) & seen[r] for r in range(n))
                assert (scores[:, :-1] >= scores[:, 1:]).all()
                np.testing.assert_allclose(scores, np.take_along_axis(full, ids.astype(np.int64), axis=1), rtol=rtol, atol=0)
            ids_all, _ = m.top_k_for(fold, k=k, exclude_seen=False)
            assert ids_all.shape == (n, k)
        finally:
            m.close()


@pytest.mark.parametrize("case", ["hpf_s7_k16", "gauss_bias_s7_k16"])
def test_similar_items_and_top_k_users_match_numpy(case):
    m, _ = _fit(case, "f64")
    try:
        k = 10
        E_u, E_i = (m.E_theta, m.E_beta) if case.startswith("hpf") else (m.m_theta, m.m_beta)
        items = np.arange(m.n_items)
        unit = E_i / np.sqrt((E_i ** 2).sum(axis=1))[:, None]
        got = m.similar_items(items, k=k)
        _numpy_topk_check(unit @ unit.T, [{int(j)} for j in items], got, k, 1e-12)
        dot = m.similar_users(np.arange(20), k=k, metric="dot")
        _numpy_topk_check(E_u[:20] @ E_u.T, [{j} for j in range(20)], dot, k, 1e-12)
        full = E_i @ E_u.T
        if not case.startswith("hpf"):
            full = m.m_item_bias[:, None] + m.m_user_bias[None, :] + full
        _numpy_topk_check(full, [set() for _ in items], m.top_k_users(items, k=k), k, 1e-12)
        with pytest.raises(ValueError, match="metric"):
            m.similar_items(items, metric="euclid")
    finally:
        m.close()


# ---- 10. the cold-start number ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hpf_s7_k16", "gauss_bias_s7_k16"])
def test_evaluate_ranking_fold_in_assembles_the_device_ranks_which_numpy_brackets(case):
    """The metrics are `ranking_metrics` of `heldout_ranks_for`'s output, and in f64 every device rank r lies in [lo, hi]:
    lo counts the NumPy competitors whose score is above s by more than 1e-12 |s|, hi those not below s by more than
    1e-12 |s| (|s|, so that the interval also brackets a negative score of the bias model), the target itself aside --
    an interval, so no allowance for mismatches is needed."""
    import pandas as pd
    from src.evaluation.ranking import ranking_metrics
    m, train = _fit(case, "f64")
    try:
        df = _new_users(m, train)
        rng = np.random.default_rng(4)
        held = rng.random(len(df)) < 0.3
        support, heldout = df[~held], df[held]
        # rows that count as skipped: an unknown item, a user absent from the support
        heldout = pd.concat([heldout, pd.DataFrame({"u": [int(df["u"].iloc[0]), 10 ** 6], "i": [m.n_items + 1, 0],
                                                    "rating": [1.0, 1.0]})], ignore_index=True)
        got = m.evaluate_ranking_fold_in(support, heldout, ks=(5, 10), n_iter=3)
        fold = m.fold_in_users(support, n_iter=3)
        ranks, cand = m.heldout_ranks_for(fold, heldout)
        want = ranking_metrics(heldout["u"].to_numpy(), ranks, cand, ks=(5, 10))
        assert got == want and got["n_skipped"] >= 2 and got["n_pairs"] > 0
        assert ranks[-1] == -1 and ranks[-2] == -1
        n = len(fold.ids)
        full = fold.predict(np.repeat(np.arange(n), m.n_items), np.tile(np.arange(m.n_items), n)).reshape(n, m.n_items)
        label, item = heldout["u"].to_numpy(), heldout["i"].to_numpy()
        for p in np.flatnonzero(ranks >= 0):
            r = int(np.searchsorted(fold.ids, label[p]))
            ok = np.ones(m.n_items, dtype=bool)
            ok[fold.seen_ids[fold.seen_ptr[r]:fold.seen_ptr[r + 1]]] = False
            ok[item[p]] = False                                            # the target itself aside
            s = full[r, item[p]]
            lo = int((full[r][ok] > s + abs(s) * 1e-12).sum())
            hi = int((full[r][ok] >= s - abs(s) * 1e-12).sum())
            assert lo <= ranks[p] <= hi, (p, lo, ranks[p], hi)
            assert cand[p] == m.n_items - len(set(fold.seen_ids[fold.seen_ptr[r]:fold.seen_ptr[r + 1]].tolist()))
    finally:
        m.close()
