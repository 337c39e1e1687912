"""`pmf_topk_items_excluding`: top-k over the items a user has not rated, against tests/topk_exclude_reference.py applied
to what the device holds.  The factor tables, biases and scales are small integers, so every fp32 score is exact in any
summation order and the comparison is `array_equal` on items and on scores -- ties, NaN rows and all."""
import numpy as np
import pytest

from helpers import frames, load_case
from topk_exclude_reference import topk_excluding, train_sets

pytestmark = pytest.mark.gpu


# ---- problems -------------------------------------------------------------------------------------------------------
def _planted(U, I):
    """(the two tied item rows, the NaN item row, the all-zero user)"""
    return (1, I - 2), 3, min(4, U - 1)


def _tables(U, I, K, seed, counts=False):
    rng = np.random.default_rng(seed)
    lo, hi = (0, 4) if counts else (-2, 3)
    A, B = rng.integers(lo, hi, (U, K)).astype(float), rng.integers(lo, hi, (I, K)).astype(float)
    bias = [rng.integers(-3, 4, U).astype(float), rng.integers(-3, 4, I).astype(float)]
    scale = [rng.integers(1, 4, U).astype(float), rng.integers(1, 4, I).astype(float)]
    (t0, t1), nan_item, zero_user = _planted(U, I)
    B[t1] = B[t0]                                          # two identical item rows: an exact tie for every user
    bias[1][t1], scale[1][t1] = bias[1][t0], scale[1][t0]
    B[nan_item] = np.nan                                   # an item whose scores are NaN (and somebody's training item)
    A[zero_user] = 0.0                                     # a user whose scores are all zero (of both signs)
    return A, B, bias, scale


def _training_pairs(U, I, seed, extra=()):
    """User 0 rated everything, user 1 all but two items, user 2 nothing, user 3 the first / last columns of the 32-item
    tiles, the others about I / 4 random items -- user 4 (the all-zero one) the NaN item among them; `extra`: further
    (user, items) lists; some pairs twice."""
    rng = np.random.default_rng(seed + 1)
    _, nan_item, zero_user = _planted(U, I)
    sets = {0: list(range(I)), 1: sorted(rng.permutation(I)[:I - 2].tolist()), 2: [],
            3: [i for i in (0, 31, 32, I - 1) if i < I]}
    for u in range(4, U):
        sets[u] = rng.permutation(I)[:max(1, I // 4)].tolist()
    sets = {u: v for u, v in sets.items() if u < U}
    sets[zero_user].append(nan_item)
    for u, items in extra:
        sets[u] = list(sets[u]) + list(items)
    tu = np.concatenate([np.full(len(v), u) for u, v in sets.items()]).astype(np.int64)
    ti = np.concatenate([np.asarray(v, dtype=np.int64) for v in sets.values()])
    dup = rng.permutation(len(tu))[:max(3, len(tu) // 10)]                # duplicate pairs count once
    tu, ti = np.concatenate([tu, tu[dup]]), np.concatenate([ti, ti[dup]])
    order = rng.permutation(len(tu))
    return tu[order], ti[order]


def _fill(ctx, A, B, bias, scale, mode):
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ARR_SCALE, ITEM, USER
    ctx.set_array(USER, ARR_FACTOR, A); ctx.set_array(ITEM, ARR_FACTOR, B)
    if mode == pmf_hip.PREDICT_BIAS:
        ctx.set_array(USER, ARR_BIAS, bias[0]); ctx.set_array(ITEM, ARR_BIAS, bias[1])
    if mode == pmf_hip.PREDICT_SCALE:
        ctx.set_array(USER, ARR_SCALE, scale[0]); ctx.set_array(ITEM, ARR_SCALE, scale[1])


def _device_scores(ctx, mode):
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ARR_SCALE, ITEM, USER
    with np.errstate(invalid="ignore"):
        full = ctx.get_array(USER, ARR_FACTOR) @ ctx.get_array(ITEM, ARR_FACTOR).T
        if mode == pmf_hip.PREDICT_BIAS:
            full = ctx.get_array(USER, ARR_BIAS)[:, None] + ctx.get_array(ITEM, ARR_BIAS)[None, :] + full
        if mode == pmf_hip.PREDICT_SCALE:
            full = full * (ctx.get_array(USER, ARR_SCALE)[:, None] * ctx.get_array(ITEM, ARR_SCALE)[None, :])
    return full


def _run(U, I, K, k, mode=0, dtype="f32", counts=False, extra=(), users=None):
    """(items, scores) of the excluding call, the reference's, the score matrix, the training sets"""
    import pmf_hip
    A, B, bias, scale = _tables(U, I, K, seed=1000 * U + I + K, counts=counts)
    tu, ti = _training_pairs(U, I, seed=U + I, extra=extra)
    users = np.random.default_rng(U).permutation(U) if users is None else np.asarray(users)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        _fill(ctx, A, B, bias, scale, mode)
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        items, scores = ctx.topk_items(users, k, use_bias=mode, exclude_train=True)
        full = _device_scores(ctx, mode)
    train = train_sets(tu, ti)
    want_i, want_s = topk_excluding(full, users, train, k)
    return (items, scores), (want_i, want_s), full, train, users


def _check(got, want):
    assert got[0].dtype == np.int32 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


def _check_planted(U, I, k, got, users):
    items = got[0]
    row = {int(u): items[r] for r, u in enumerate(users)}
    assert (row[0] == -1).all()                                          # rated everything
    assert (row[1][2:] == -1).all()                                      # two items left (one of them may be the NaN row)
    assert not (items == _planted(U, I)[1]).any()                        # the NaN item never ranks
    assert not np.isin(row[3], [0, 31, 32, I - 1]).any()                 # the tile's first and last columns


# ---- 1. tile and stage edges of the fused kernel ----------------------------------------------------------------------
_EDGES = [(5, 7, 3, 7), (40, 33, 16, 10), (33, 64, 8, 1), (64, 64, 64, 64), (130, 95, 128, 50), (257, 1000, 100, 64)]


@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("U,I,K,k", _EDGES)
def test_fused_edge_shapes_equal_the_reference(U, I, K, k, max_blocks, monkeypatch):
    """Fewer items than a tile, one item past a tile, exactly one stage, k = 1 and k = 64, user counts around the 32 / 128
    tile edges, a partial last stage behind full ones.  `max_blocks` = 2: two blocks walk all user tiles, so the cursors
    are set up again for every tile."""
    if max_blocks:
        monkeypatch.setenv("PMF_TOPK_MAX_BLOCKS", str(max_blocks))
    got, want, _, _, users = _run(U, I, K, k, counts=K == 16)
    _check(got, want)
    _check_planted(U, I, k, got, users)


@pytest.mark.parametrize("buffers", [1, 2])
@pytest.mark.parametrize("U,I,K,k", [(5, 7, 3, 7), (257, 1000, 100, 64)])
def test_fused_edge_shapes_with_either_stage_buffering(U, I, K, k, buffers, monkeypatch):
    monkeypatch.setenv("PMF_TOPK_STAGE_BUFFERS", str(buffers))
    got, want, _, _, _ = _run(U, I, K, k)
    _check(got, want)


# ---- 2. the best item excluded; a tie group whose lower id is excluded ------------------------------------------------
def test_k1_with_the_best_item_excluded_and_a_tie_whose_lower_id_is_excluded():
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    U, I, K = 40, 70, 16
    A, B, _, _ = _tables(U, I, K, seed=7, counts=True)
    (t0, t1), nan_item, _ = _planted(U, I)
    A[5:9] = 3.0
    B[t0] = B[t1] = 3.0                                    # for users 5 .. 8 the tied pair is the top of the list (9 K)
    with np.errstate(invalid="ignore"):
        full = A @ B.T
    best = np.nanargmax(np.where(np.isnan(full), -np.inf, full), axis=1)
    tu = np.array([0, 1, 2, 5, 7, 7, 8], dtype=np.int64)   # users 0 .. 2: their best item; 5: the tie's lower id; 7: both; 8: the upper
    ti = np.array([best[0], best[1], best[2], t0, t0, t1, t1], dtype=np.int64)
    users = np.arange(U)
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        ctx.set_array(USER, ARR_FACTOR, A); ctx.set_array(ITEM, ARR_FACTOR, B)
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        got = ctx.topk_items(users, 1, exclude_train=True)
        got2 = ctx.topk_items(users, 2, exclude_train=True)
    train = train_sets(tu, ti)
    _check(got, topk_excluding(full, users, train, 1))
    _check(got2, topk_excluding(full, users, train, 2))
    assert got[0][5, 0] == t1 and got[0][6, 0] == t0 and got[0][8, 0] == t0      # the next id wins / nothing excluded / upper excluded
    assert got[0][7, 0] not in (t0, t1)
    for u in (0, 1, 2):
        assert got[0][u, 0] != best[u] and full[u, got[0][u, 0]] <= full[u, best[u]]


# ---- 3. segments of the item range --------------------------------------------------------------------------------
def _segments(n_query, I):
    """tests' copy of the rule the library cuts the item range by (pmf_topk.hip, topk_segments)"""
    waves = (n_query + 31) // 32
    nseg = min(64, max(1, 4096 // waves))
    nseg = min(nseg, max(1, I // 2048))
    seg_items = ((I + nseg - 1) // nseg + 31) // 32 * 32
    return (I + seg_items - 1) // seg_items, seg_items


@pytest.mark.parametrize("U,I,K,k", [(129, 4097, 12, 3), (3, 6200, 20, 10)])
def test_segmented_item_range_with_excluded_items_on_both_sides_of_every_boundary(U, I, K, k):
    nseg, seg_items = _segments(U, I)
    assert nseg > 1
    edges = [s * seg_items + d for s in range(1, nseg) for d in (-1, 0)]
    extra = [(u, edges) for u in range(2, U)]                         # (users 0 and 1 hold them already, or nearly)
    got, want, _, train, users = _run(U, I, K, k, extra=extra)
    _check(got, want)
    assert not np.isin(got[0][users >= 2], edges).any()


# ---- 4. score modes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,I,K,k,mode", [(40, 33, 16, 10, 1), (257, 1000, 100, 64, 2)])
def test_bias_and_scale_modes(U, I, K, k, mode):
    got, want, _, _, _ = _run(U, I, K, k, mode=mode, counts=mode == 2)
    _check(got, want)


# ---- 5. the two-phase path ------------------------------------------------------------------------------------------
def test_two_phase_path_equals_the_fused_kernel(monkeypatch):
    fused, want, _, _, _ = _run(257, 1000, 100, 64)
    monkeypatch.setenv("PMF_TOPK_TWO_PHASE", "1")
    two, _, _, _, _ = _run(257, 1000, 100, 64)
    _check(two, want)
    assert np.array_equal(two[0], fused[0]) and np.array_equal(two[1], fused[1])


@pytest.mark.parametrize("U,I,K,k,dtype", [(257, 1000, 100, 65, "f32"), (130, 95, 16, 50, "f64"), (130, 95, 130, 50, "f32")])
def test_two_phase_path_long_lists_fp64_and_wide_factors(U, I, K, k, dtype):
    got, want, _, _, users = _run(U, I, K, k, dtype=dtype)
    _check(got, want)
    _check_planted(U, I, k, got, users)


# ---- 6. agreement with pmf_rank_items -------------------------------------------------------------------------------
@pytest.mark.parametrize("U,I,K,k,dtype", [(257, 1000, 100, 64, "f32"), (130, 95, 16, 50, "f64")])
def test_position_is_the_rank_pmf_rank_items_gives(U, I, K, k, dtype):
    import pmf_hip
    A, B, bias, scale = _tables(U, I, K, seed=3)
    tu, ti = _training_pairs(U, I, seed=3)
    users = np.arange(U)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        _fill(ctx, A, B, bias, scale, 0)
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        items, _ = ctx.topk_items(users, k, exclude_train=True)
        valid = items >= 0
        qu, qi = np.repeat(users, k).reshape(U, k)[valid], items[valid]
        ranks, _ = ctx.rank_items(qu, qi, exclude_train=True)
        _, cand = ctx.rank_items(users, np.zeros(U, dtype=np.int64), exclude_train=True)
    assert np.array_equal(ranks, np.nonzero(valid)[1])                  # the column index
    assert np.array_equal(valid.sum(axis=1), np.minimum(k, cand))
    assert (valid[:, :-1] >= valid[:, 1:]).all()                        # valid entries come first


# ---- 7. contract ----------------------------------------------------------------------------------------------------
def test_contract_of_the_call():
    import ctypes as C

    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    U, I, K, k = 130, 95, 20, 10
    A, B, bias, scale = _tables(U, I, K, seed=11)
    tu, ti = _training_pairs(U, I, seed=11)
    users = np.concatenate([np.arange(U), [7, 7, 0, 129, 7]])           # repeated query users
    lib = pmf_hip.load()

    def raw(ctx, exclude, items, scores):
        u = np.ascontiguousarray(users, dtype=np.int32)
        return lib.pmf_topk_items_excluding(ctx._h, len(u), u.ctypes.data_as(C.POINTER(C.c_int32)), k, 0, exclude,
                                            items.ctypes.data_as(C.POINTER(C.c_int32)), scores.ctypes.data_as(C.POINTER(C.c_double)))

    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        _fill(ctx, A, B, bias, scale, 0)
        before = [ctx.get_array(s, ARR_FACTOR) for s in (USER, ITEM)]
        # exclude_train without ratings: PMF_EINVAL, the documented message, outputs untouched
        items, scores = np.full((len(users), k), -7, dtype=np.int32), np.full((len(users), k), -7.0)
        assert raw(ctx, 1, items, scores) == -1                          # PMF_EINVAL
        msg = lib.pmf_last_error().decode()
        assert msg == ("pmf_topk_items_excluding: exclude_train needs the training ratings (pmf_ctx_set_ratings); "
                       "the context holds none")
        assert (items == -7).all() and (scores == -7.0).all()
        with pytest.raises(pmf_hip.PmfError, match="exclude_train needs the training ratings"):
            ctx.topk_items(users, k, exclude_train=True)
        # exclude_train = 0 through the new symbol is pmf_topk_items, byte for byte
        plain = ctx.topk_items(users, k)
        assert raw(ctx, 0, items, scores) == 0
        assert items.tobytes() == plain[0].tobytes() and scores.tobytes() == plain[1].tobytes()
        # the distinct-item lists are built by the first excluding call, once
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        ctx.topk_items(users, k)
        bytes_0 = ctx.device_bytes()
        first = ctx.topk_items(users, k, exclude_train=True)
        bytes_1 = ctx.device_bytes()
        second = ctx.topk_items(users, k, exclude_train=True)
        again = ctx.topk_items(users, k)
        assert bytes_1 > bytes_0 and ctx.device_bytes() == bytes_1
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()   # repeatable
        assert again[0].tobytes() == plain[0].tobytes() and again[1].tobytes() == plain[1].tobytes()     # no leak into the plain call
        full = _device_scores(ctx, 0)
        _check(first, topk_excluding(full, users, train_sets(tu, ti), k))
        assert np.array_equal(first[0][-5], first[0][7]) and np.array_equal(first[0][-3], first[0][0])   # repeats: the same rows
        # new ratings: the exclusion follows them
        tu2, ti2 = _training_pairs(U, I, seed=12)
        ctx.set_ratings(tu2, ti2, np.ones(len(tu2)))
        _check(ctx.topk_items(users, k, exclude_train=True), topk_excluding(full, users, train_sets(tu2, ti2), k))
        for want, side in zip(before, (USER, ITEM)):                    # the model is read only
            assert np.array_equal(ctx.get_array(side, ARR_FACTOR), want, equal_nan=True)
        items0, scores0 = ctx.topk_items([], k, exclude_train=True)     # n_query = 0
        assert items0.shape == (0, k) and scores0.shape == (0, k)
    # the lists pmf_rank_items built serve the top-k call: it adds nothing
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        _fill(ctx, A, B, bias, scale, 0)
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        ctx.topk_items(users, k)                                        # (the call's scratch)
        ctx.rank_items([0, 1], [1, 2], exclude_train=True)
        bytes_r = ctx.device_bytes()
        ctx.topk_items(users, k, exclude_train=True)
        assert ctx.device_bytes() == bytes_r


# ---- 8. model level -------------------------------------------------------------------------------------------------
def test_model_top_k_items_without_training_items():
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    d, meta = load_case("hpf_s7_k16")
    train, _ = frames(d)
    kw = dict(meta["base_cfg"], n_factors=meta["K"], random_state=meta["seed"], max_iter=5, verbose=False, tol=None)
    tu, ti = train["u"].to_numpy(dtype=int), train["i"].to_numpy(dtype=int)
    sets = train_sets(tu, ti)
    lists = {}
    for dtype in ("f64", "f32"):
        m = HPF_CAVI(HPF_CAVI_Config(**kw), dtype=dtype).fit(train)
        users = np.arange(m.n_users)
        items, scores = m.top_k_items(users, 10, exclude_train=True)
        for u in users:                                                 # no returned pair is a training pair
            assert not (set(items[u][items[u] >= 0].tolist()) & sets.get(int(u), set())), u
        if dtype == "f64":
            want_i, want_s = topk_excluding(m.E_theta @ m.E_beta.T, users, sets, 10)
            assert np.array_equal(items, want_i)
            np.testing.assert_allclose(scores, want_s, rtol=1e-12)
        plain, _ = m.top_k_items(users, 10)
        assert (plain != items).any()                                   # (the plain list does hold training items)
        lists[dtype] = items
        m.close()
    assert np.mean(lists["f32"] == lists["f64"]) > 0.97
