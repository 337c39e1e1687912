"""The later rounds of the loops that stage work through a bounded buffer: `pmf_topk_items*` and `pmf_rank_items` (rounds
of at most 2^20 query rows, or 512 MB of scores on the two-phase path) and the array exchanges (rounds of 64 MiB).  No
test shape reaches those caps, so `PMF_TOPK_QUERY_ROWS` and `PMF_STAGE_BYTES` (read when a context is created) lower
them: a few hundred query rows then take three rounds with a ragged last one, ten rows of an array four.

What a later round can get wrong and the first cannot: the output offset, a staging buffer reused too early, counters
zeroed per round, a caller row of `pmf_rank_items` whose query rows lie on both sides of a round boundary, exclusion
lists indexed by user while the staged user ids change per round, segment and candidate counts fixed from a full round
while the last one is ragged.

The top-k and ranking tables are the small-integer tables of tests/test_ranking_gpu.py: every score is exact in fp32 in
any summation order and the data is full of exact ties, so every comparison is equality.  Each case checks (a) that
the capped context returns the bits of an uncapped one, (b) that both equal the fp64 NumPy reference of what the
device holds, (c) that the rounds really ran: the profiler's launch count of the top-k kernel class is one per round."""
import numpy as np
import pytest

from test_ranking_gpu import _csr, _device_scores, _fill, _integer_tables, _main_problem, _ref_rows
from test_topk_gpu import _rank
from topk_exclude_reference import topk_excluding, train_sets

pytestmark = pytest.mark.gpu

CAP = 128


def _rounds(n, cap):
    return -(-n // cap)


def _both(monkeypatch, cap, open_ctx, mode, call):
    """`call(ctx)` on a context without the cap and on one with it: [(result, launches of the top-k class, fp64 score
    matrix of what the device holds)] in that order."""
    out = []
    for value in (None, cap):
        if value is None:
            monkeypatch.delenv("PMF_TOPK_QUERY_ROWS", raising=False)
        else:
            monkeypatch.setenv("PMF_TOPK_QUERY_ROWS", str(value))        # read when the context is created
        with open_ctx() as ctx:
            ctx.prof_enable(True)
            ctx.prof_reset()
            res = call(ctx)
            launches = ctx.prof_get()["topk"][1]
            out.append((res, launches, _device_scores(ctx, mode)))
    return out


# ---- top-k ------------------------------------------------------------------------------------------------------------
TOPK_U, TOPK_I, TOPK_N = 700, 4100, 333           # 4100 items: two item segments at these query counts, merged per round
ZERO_USER, NAN_ITEM, NO_RATINGS_USER, FEW_LEFT_USER = 5, 77, 2, 9
FEW_LEFT = (3, NAN_ITEM, 500, 2081, 4099, 11)     # what FEW_LEFT_USER has not rated: five candidates and the NaN item
_TOPK = {}


def _topk_problem(K, mode):
    """Tables, the 333 query users (drawn from 700 with repeats) and the training pairs: computed once per (K, mode)."""
    if (K, mode) in _TOPK:
        return _TOPK[K, mode]
    rng = np.random.default_rng(100 * K + mode)
    U, I = TOPK_U, TOPK_I
    A, B, bias, scale = _integer_tables(rng, U, I, K, signed=(K + mode) % 2 == 1)
    B[I - 1] = B[2100] = B[11]                    # exact ties across the two segments
    bias[1][[I - 1, 2100]] = bias[1][11]
    scale[1][[I - 1, 2100]] = scale[1][11]
    B[NAN_ITEM] = np.nan                          # an item whose scores are NaN never ranks
    A[ZERO_USER] = 0.0                            # all scores equal: the lowest ids win
    users = rng.integers(0, U, TOPK_N)
    users[0] = users[300] = ZERO_USER             # the same user in the first and in the last round
    users[1] = users[130] = users[299] = 40       # and one in all three
    users[200] = NO_RATINGS_USER
    users[310] = FEW_LEFT_USER                    # fewer than k candidates left, in the last round
    tu, ti = [], []
    for u in range(U):
        if u == NO_RATINGS_USER:
            continue
        mine = np.setdiff1d(np.arange(I), FEW_LEFT) if u == FEW_LEFT_USER else rng.integers(0, I, 40)
        tu.append(np.full(len(mine), u)); ti.append(mine)
    tu, ti = np.concatenate(tu), np.concatenate(ti)
    tu, ti = np.concatenate([tu, tu[:900]]), np.concatenate([ti, ti[:900]])          # some pairs twice
    order = rng.permutation(len(tu))
    _TOPK[K, mode] = (A, B, bias, scale, users, tu[order], ti[order])
    return _TOPK[K, mode]


def _topk_case(monkeypatch, K, mode, k, dtype, exclude, cap=CAP, want_rounds=None):
    import pmf_hip
    A, B, bias, scale, users, tu, ti = _topk_problem(K, mode)

    def open_ctx():
        ctx = pmf_hip.Context(TOPK_U, TOPK_I, K, dtype=dtype)
        _fill(ctx, A, B, bias, scale, mode)
        if exclude:
            ctx.set_ratings(tu, ti, np.ones(len(tu)))
        return ctx

    (plain, n_plain, full), (capped, n_capped, full_c) = _both(
        monkeypatch, cap, open_ctx, mode, lambda ctx: ctx.topk_items(users, k, use_bias=mode, exclude_train=exclude))
    assert n_plain == 1
    assert n_capped == (_rounds(TOPK_N, cap) if want_rounds is None else want_rounds)
    assert np.array_equal(full, full_c, equal_nan=True)
    # (a) the bits of the uncapped call
    assert capped[0].shape == (TOPK_N, k) and capped[0].dtype == np.int32
    assert np.array_equal(capped[0], plain[0])
    assert capped[1].tobytes() == plain[1].tobytes()
    # (b) the reference on what the device holds
    if exclude:
        want_i, want_s = topk_excluding(full, users, train_sets(tu, ti), k)
        row = capped[0][310]                                             # the -1 / 0.0 fill lands in the last round's rows
        assert (row[:5] >= 0).all() and (row[5:] == -1).all() and (capped[1][310, 5:] == 0.0).all()
        assert set(row[:5].tolist()) == set(FEW_LEFT) - {NAN_ITEM}
    else:
        ranked = np.where(np.isnan(full), -np.inf, full)[users]
        want_i = _rank(ranked, k)
        want_s = np.take_along_axis(ranked, want_i, axis=1)
    assert np.array_equal(capped[0], want_i)
    assert np.array_equal(capped[1], want_s)
    assert not (capped[0] == NAN_ITEM).any()
    assert np.array_equal(capped[0][0], capped[0][300]) and np.array_equal(capped[0][1], capped[0][299])   # repeated users
    assert np.array_equal(capped[0][1], capped[0][130])


@pytest.mark.parametrize("K,mode,k", [(20, 1, 10), (64, 0, 64), (100, 2, 33)])
def test_fused_topk_in_three_rounds(K, mode, k, monkeypatch):
    """Rounds of 128, 128 and 77 query users; two item segments, so the merge kernel runs in every round."""
    _topk_case(monkeypatch, K, mode, k, "f32", exclude=False)


@pytest.mark.parametrize("K,mode,k", [(64, 0, 10), (20, 1, 64)])
def test_fused_topk_excluding_in_three_rounds(K, mode, k, monkeypatch):
    """The exclusion lists are indexed by user id while the staged ids are those of the round."""
    _topk_case(monkeypatch, K, mode, k, "f32", exclude=True)


# (dtype, K, mode, k, PMF_TOPK_TWO_PHASE): K = 136 pads past 128 and takes the two-phase path by itself
_TWO_PHASE = [("f32", 64, 1, 10, True), ("f32", 136, 0, 10, False), ("f32", 64, 2, 65, True), ("f64", 16, 1, 10, True)]


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("dtype,K,mode,k,switch", _TWO_PHASE)
def test_two_phase_topk_in_three_rounds(dtype, K, mode, k, switch, exclude, monkeypatch):
    """Score matrix in HBM, then select: the cap applies on top of the 512 MB rule (which allows 352 rows here)."""
    if switch:
        monkeypatch.setenv("PMF_TOPK_TWO_PHASE", "1")
    _topk_case(monkeypatch, K, mode, k, dtype, exclude)


@pytest.mark.parametrize("cap,rounds", [(1024, 1), (130, 3), (5, 11)])
def test_cap_is_rounded_to_32_rows_and_a_cap_above_the_batch_is_one_round(cap, rounds, monkeypatch):
    """1024 rows hold the whole batch; 130 rounds down to 128; 5 is raised to 32 (rounds of 32 .. 32, 13)."""
    _topk_case(monkeypatch, 64, 0, 10, "f32", exclude=True, cap=cap, want_rounds=rounds)


def test_two_phase_512_mb_rule_takes_a_second_round_by_itself():
    """No switch: fp64 scores of 40,000 items are 320,000 bytes a row, 512 MiB hold 1677 rows, rounded down to 1664, so
    1,700 query users are rounds of 1664 and 36.  Real-valued gamma factors; the criterion is that of
    tests/test_topk_gpu.py::test_topk_matches_numpy_ranking for fp64: items equal, scores to 1e-12."""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(8)
    U, I, K, k, n = 2000, 40000, 8, 5, 1700
    per_round = (512 << 20) // (I * 8) // 32 * 32
    assert per_round == 1664 and min(per_round, (n + 31) // 32 * 32) == 1664 and n - per_round == 36
    A, B = rng.gamma(0.5, 1.0, (U, K)), rng.gamma(0.5, 1.0, (I, K))
    users = rng.permutation(U)[:n]
    with pmf_hip.Context(U, I, K, dtype="f64") as ctx:
        ctx.set_array(USER, ARR_FACTOR, A); ctx.set_array(ITEM, ARR_FACTOR, B)
        ctx.prof_enable(True)
        ctx.prof_reset()
        items, scores = ctx.topk_items(users, k)
        launches = ctx.prof_get()["topk"][1]
        Ad, Bd = ctx.get_array(USER, ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
    assert launches == 2
    want_i, want_s = np.empty((n, k), dtype=np.int64), np.empty((n, k))
    for lo in range(0, n, 425):                                          # (the host product in four blocks of 136 MB)
        full = Ad[users[lo:lo + 425]] @ Bd.T
        best = np.argpartition(-full, k - 1, axis=1)[:, :k]              # the k winners, then their order
        vals = np.take_along_axis(full, best, axis=1)
        order = np.lexsort((best, -vals), axis=1)
        want_i[lo:lo + 425] = np.take_along_axis(best, order, axis=1)
        want_s[lo:lo + 425] = np.take_along_axis(vals, order, axis=1)
    assert items.shape == (n, k)
    assert np.array_equal(items, want_i)
    np.testing.assert_allclose(scores, want_s, rtol=1e-12, atol=1e-12)


# ---- ranking ----------------------------------------------------------------------------------------------------------
N_LEAD, N_LONG, N_TAIL = 120, 70, 150


def _rank_batch_rows(rng, U, I):
    """120 one-target rows, the row of 70 targets, a row without targets, the NaN user, the tie group 5 / 17 / 1500 as
    three rows of one user, the NaN item as a target, 150 one-target rows (tables: test_ranking_gpu._main_problem)."""
    users = rng.integers(0, U, N_LEAD).tolist()
    targets = [[int(rng.integers(I))] for _ in range(N_LEAD)]
    users.append(7); targets.append(rng.permutation(I)[:N_LONG].tolist())
    users += [0, 21, 11, 11, 11, 30]
    targets += [[], [4, 5], [1500], [5], [17], [77]]
    users += rng.integers(0, U, N_TAIL).tolist()
    targets += [[int(rng.integers(I))] for _ in range(N_TAIL)]
    return np.array(users), targets


def _query_rows(row_ptr, slots):
    """First query row of every caller row (and, last, the total): a row's targets go in runs of `slots`, a row without
    targets keeps one query row (pmf_rank_items)."""
    per_row = np.maximum(1, -(-np.diff(row_ptr) // slots))
    first = np.concatenate([[0], np.cumsum(per_row)])
    return first, int(first[-1])


def _rank_training_pairs(rng, U, I, users, targets):
    tu, ti = rng.integers(0, U, 6000), rng.integers(0, I, 6000)
    keep = tu != 2                                                       # user 2: no ratings
    tu, ti = np.concatenate([tu[keep], tu[keep][:500]]), np.concatenate([ti[keep], ti[keep][:500]])   # duplicate pairs
    own = [(int(u), int(t[0])) for u, t in zip(users[::3], targets[::3]) if len(t)]                  # targets that are training items
    for u, t in zip(users, targets):                                     # of the rows of several targets: one of them twice
        if len(t) > 1:
            own += [(int(u), int(t[0])), (int(u), int(t[0])), (int(u), int(t[len(t) // 2]))]
    own.append((11, 5))                                                  # the lowest id of the tie group
    tu, ti = np.concatenate([tu, [p[0] for p in own]]), np.concatenate([ti, [p[1] for p in own]])
    order = rng.permutation(len(tu))
    return tu[order], ti[order]


def _rank_case(monkeypatch, K, mode, dtype, exclude, slots=4, cap=CAP, one_target=False, flat=False):
    import pmf_hip
    from pmf_hip.engine import rank_batch
    A, B, bias, scale, _, _ = _main_problem(K, signed=(K + mode) % 2 == 1, seed=4)
    U, I = A.shape[0], B.shape[0]
    rng = np.random.default_rng(K + 10 * mode)
    if one_target:
        users = rng.integers(0, U, 390)
        users[[0, 1, 2, 130, 300, 389]] = [11, 11, 11, 21, 13, 11]       # the tie group, the NaN user, the all-zero user
        targets = [[int(rng.integers(I))] for _ in users]
        targets[0], targets[1], targets[2], targets[300], targets[389] = [1500], [5], [17], [77], [17]
    else:
        users, targets = _rank_batch_rows(rng, U, I)
    row_ptr, items = _csr(targets)
    first, n_query = _query_rows(row_ptr, slots)
    if not one_target:
        # the straddle: the long row's first query row lies in the first round, its last in a later one
        assert row_ptr[N_LEAD + 1] - row_ptr[N_LEAD] == N_LONG and first[N_LEAD] == N_LEAD
        lo, hi = first[N_LEAD], first[N_LEAD + 1] - 1                    # the long row's query rows
        assert hi - lo + 1 == -(-N_LONG // slots)
        assert hi // cap - lo // cap == (2 if slots == 1 else 1)         # boundaries between them
    assert _rounds(n_query, cap) >= 3 and n_query % cap != 0            # a third, ragged round
    tu, ti = _rank_training_pairs(rng, U, I, users, targets)

    def open_ctx():
        ctx = pmf_hip.Context(U, I, K, dtype=dtype)
        _fill(ctx, A, B, bias, scale, mode)
        if exclude:
            ctx.set_ratings(tu, ti, np.ones(len(tu)))
        return ctx

    if slots != 4:
        monkeypatch.setenv("PMF_RANK_TARGETS", str(slots))
    (plain, n_plain, full), (capped, n_capped, _) = _both(
        monkeypatch, cap, open_ctx, mode, lambda ctx: ctx.rank_rows(users, row_ptr, items, use_bias=mode, exclude_train=exclude))
    assert n_plain == 1 and n_capped == _rounds(n_query, cap)
    want_r, want_c = _ref_rows(full, users, targets, train_sets(tu, ti) if exclude else None)
    for got in (plain, capped):
        assert np.array_equal(got[0], want_r) and np.array_equal(got[1], want_c)
    if not one_target:
        tie = capped[0][row_ptr[N_LEAD + 3]:row_ptr[N_LEAD + 6]]         # targets 1500, 5, 17 of user 11: ranked by item id
        assert exclude or tie[1] < tie[2] < tie[0]
        assert (capped[0][row_ptr[N_LEAD + 2]:row_ptr[N_LEAD + 3]] == -1).all() and capped[1][N_LEAD + 2] == 0   # the NaN user
        assert capped[0][row_ptr[N_LEAD + 6]] == -1                      # the NaN item as a target
    if flat:                                                             # the same pairs through rank_items
        has = np.diff(row_ptr) > 0
        pu = np.repeat(users, np.diff(row_ptr))
        _, f_ptr, _, _ = rank_batch(pu, items)
        _, f_query = _query_rows(f_ptr, slots)
        (f_plain, fn_plain, _), (f_capped, fn_capped, _) = _both(
            monkeypatch, cap, open_ctx, mode, lambda ctx: ctx.rank_items(pu, items, use_bias=mode, exclude_train=exclude))
        assert fn_plain == 1 and fn_capped == _rounds(f_query, cap) >= 2
        for got in (f_plain, f_capped):
            assert np.array_equal(got[0], want_r)
            assert np.array_equal(got[1], np.repeat(want_c[has], np.diff(row_ptr)[has]))


# K = 64 and 20: the fused scan with four target slots; K = 136 and fp64: the generic kernel
_RANK_KERNELS = [("f32", 64, 0), ("f32", 64, 1), ("f32", 20, 2), ("f32", 136, 1), ("f64", 16, 2)]


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("dtype,K,mode", _RANK_KERNELS)
def test_rank_rows_in_three_rounds_with_a_row_across_the_boundary(dtype, K, mode, exclude, monkeypatch):
    """294 query rows in rounds of 128, 128 and 38.  The row of 70 targets is query rows 120 .. 137: its candidates are
    written by the first round, most of its ranks by the second."""
    _rank_case(monkeypatch, K, mode, dtype, exclude)


@pytest.mark.parametrize("exclude", [False, True])
def test_one_target_rows_in_several_rounds(exclude, monkeypatch):
    """390 rows of one target each, rounds of 128, 128, 128 and 6: the scan's one-slot instantiation; then the same pairs as
    flat `rank_items` pairs (grouped by user: rows of several targets)."""
    _rank_case(monkeypatch, 64, 0, "f32", exclude, one_target=True, flat=True)


@pytest.mark.parametrize("slots,cap", [(2, CAP), (1, 32)])
def test_rank_rows_with_fewer_target_slots(slots, cap, monkeypatch):
    """PMF_RANK_TARGETS=2: the row of 70 targets is the 35 query rows 120 .. 154.  PMF_RANK_TARGETS=1 in rounds of 32: it is
    the 70 query rows 120 .. 189, across the boundaries at 128 and 160 -- only its first run may write its candidates."""
    _rank_case(monkeypatch, 64, 1, "f32", exclude=True, slots=slots, cap=cap)


# ---- array exchange ---------------------------------------------------------------------------------------------------
ROWS_U, ROWS_I = 10, 13                          # rounds of 3, 3, 3, 1 and of 3, 3, 3, 3, 1 rows
_LAYOUT = {}


def _row_bytes(K, dtype, array):
    """Bytes of one device row of `array`: the padded factor row, the packed covariance row, one element."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR
    if (K, dtype) not in _LAYOUT:
        with pmf_hip.Context(1, 1, K, dtype=dtype) as ctx:
            _LAYOUT[K, dtype] = (ctx.kpad, ctx.cov_stride)
    kpad, cov_stride = _LAYOUT[K, dtype]
    elem = 8 if dtype == "f64" else 4
    return elem * (kpad if array == ARR_FACTOR else cov_stride if array == ARR_COV else 1)


def _stages(K, dtype, array):
    """The two PMF_STAGE_BYTES values of a case -> rows per round"""
    return {3 * _row_bytes(K, dtype, array) + 1: 3, 1: 1}


def _host_array(rng, rows, K, array):
    from pmf_hip import ARR_COV, ARR_FACTOR
    if array == ARR_COV:
        a = rng.standard_normal((rows, K, K))
        return a + a.transpose(0, 2, 1)                                  # symmetric, every row different
    return rng.standard_normal((rows, K)) if array == ARR_FACTOR else rng.standard_normal(rows)


def _array_id(name):
    import pmf_hip
    return getattr(pmf_hip, "ARR_" + name)


@pytest.mark.parametrize("name", ["FACTOR", "COV", "BIAS"])
@pytest.mark.parametrize("K", [5, 20, 70])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_set_array_get_array_round_trip_in_rounds(dtype, K, name, monkeypatch):
    """K = 20 in fp32 is the line-padded factor row (kpad 32); K = 5 a covariance row that is no multiple of 16 bytes."""
    import pmf_hip
    from pmf_hip import ARR_COV, ITEM, USER
    array = _array_id(name)
    rng = np.random.default_rng(K)
    host = {side: _host_array(rng, rows, K, array) for side, rows in ((USER, ROWS_U), (ITEM, ROWS_I))}
    np_dtype = np.float64 if dtype == "f64" else np.float32
    got = {}
    for stage in [None] + list(_stages(K, dtype, array)):
        if stage is None:
            monkeypatch.delenv("PMF_STAGE_BYTES", raising=False)
        else:
            monkeypatch.setenv("PMF_STAGE_BYTES", str(stage))            # read when the context is created
        with pmf_hip.Context(ROWS_U, ROWS_I, K, dtype=dtype) as ctx:
            for side in (USER, ITEM):
                ctx.set_array(side, array, host[side])
            got[stage] = {side: ctx.get_array(side, array) for side in (USER, ITEM)}
    for stage, back in got.items():
        for side in (USER, ITEM):
            assert np.array_equal(back[side], host[side].astype(np_dtype).astype(np.float64)), (stage, side)
            assert back[side].tobytes() == got[None][side].tobytes(), (stage, side)
            if array == ARR_COV:
                assert np.array_equal(back[side], back[side].transpose(0, 2, 1)), (stage, side)


@pytest.mark.parametrize("name", ["FACTOR", "COV", "BIAS"])
@pytest.mark.parametrize("K", [5, 20, 70])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_row_exchange_in_rounds(dtype, K, name, monkeypatch):
    """`get_array_rows` of 10 ids (shuffled, one twice, the last row among them) and `set_array_rows` of 10 distinct ids
    in rounds of three rows and of one.  FACTOR and COV rows are copied in 16-byte units, BIAS in 4- and 8-byte ones.  The
    row exchange has no launch counter: the growth of `device_bytes()` by the first `get_array_rows` of a fresh context
    is its device staging -- [step rows, to 16 bytes][step int64 ids] -- and says that the step was the capped one."""
    import pmf_hip
    from pmf_hip import ARR_COV, USER
    array = _array_id(name)
    rng = np.random.default_rng(K + 1)
    U, n = 40, 10
    base = _host_array(rng, U, K, array)
    new = _host_array(rng, n, K, array)
    ids = rng.permutation(U - 1)[:n]
    ids[3], ids[7], ids[8] = U - 1, ids[0], 0                            # the last row, a repeat, the first row
    write_ids = rng.permutation(U)[:n]
    np_dtype = np.float64 if dtype == "f64" else np.float32
    row_bytes = _row_bytes(K, dtype, array)

    def staging(step):
        return (step * row_bytes + 15) // 16 * 16 + step * 8

    assert len({staging(1), staging(3), staging(n)}) == 3
    for stage, step in [(None, n)] + list(_stages(K, dtype, array).items()):
        if stage is None:
            monkeypatch.delenv("PMF_STAGE_BYTES", raising=False)
        else:
            monkeypatch.setenv("PMF_STAGE_BYTES", str(stage))
        with pmf_hip.Context(U, 3, K, dtype=dtype) as ctx:
            ctx.set_array(USER, array, base)
            full = ctx.get_array(USER, array)
            before = ctx.device_bytes()
            got = ctx.get_array_rows(USER, array, ids)
            assert ctx.device_bytes() - before == staging(step), (stage, step)
            assert np.array_equal(got, full[ids]), stage
            ctx.set_array_rows(USER, array, write_ids, new)
            after = ctx.get_array(USER, array)
            want = full.copy()
            want[write_ids] = new.astype(np_dtype).astype(np.float64)    # the written rows; every other row untouched
            assert np.array_equal(after, want), stage
            if array == ARR_COV:
                assert np.array_equal(after, after.transpose(0, 2, 1))


@pytest.mark.parametrize("K,dtype", [(20, "f32"), (5, "f64")])
def test_fold_in_downloads_in_rounds(K, dtype, monkeypatch):
    """`gauss_fold_in` and `gamma_fold_in` of 10 new rows: every returned array has the bits it has with the default
    stage, in rounds of three rows and of one row of each downloaded array."""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(K)
    I, n = 30, 10
    lengths = [0, 1, 2, 5, 7, 3, 12, 1, 4, 9]
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, I, row_ptr[-1]).astype(np.int32)
    x = rng.integers(1, 6, row_ptr[-1]).astype(np.float64)
    m_item = np.abs(0.5 * rng.standard_normal((I, K))) + 0.1
    bias_item = 0.1 * rng.standard_normal(I)
    stages = [None, 1] + [3 * _row_bytes(K, dtype, a) + 1 for a in (ARR_FACTOR, ARR_COV, ARR_BIAS)]
    out = {}
    for stage in stages:
        if stage is None:
            monkeypatch.delenv("PMF_STAGE_BYTES", raising=False)
        else:
            monkeypatch.setenv("PMF_STAGE_BYTES", str(stage))
        with pmf_hip.Context(n, I, K, dtype=dtype) as ctx:
            ctx.set_array(ITEM, ARR_FACTOR, m_item)
            ctx.set_cov_identity(ITEM, 0.5)
            ctx.set_array(ITEM, ARR_BIAS, bias_item); ctx.set_array(USER, ARR_BIAS, np.zeros(n))   # (a model with biases)
            gauss = ctx.gauss_fold_in(USER, row_ptr, ids, x - 3.0, 0.3, 0.5, 1.0, n_iter=2)
            gamma = ctx.gamma_fold_in(USER, row_ptr, ids, x, 0.3, 0.0, True, 0.3 + K * 0.3, 5.0, n_iter=3)
        out[stage] = [a for a in gauss + gamma]
        assert len(out[stage]) == 8 and all(a is not None and len(a) == n for a in out[stage])
    assert all(np.abs(a[-1]).max() > 0 for a in out[None])              # the last row of every array arrived
    for stage in stages[1:]:
        for a, b in zip(out[stage], out[None]):
            assert a.tobytes() == b.tobytes(), stage


def test_gather_user_rows_and_host_all_reduce_in_rounds(monkeypatch):
    """One-rank RCCL communicator (tests/test_sharded_fit_gpu.py::test_pipelined_item_sweep_over_real_rccl_single_rank):
    `gather_user_rows` in rounds of three rows, and a host all-reduce of 8193 doubles -- one more than its 64 KB buffer
    holds, so rounds of 8192 and 1."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, USER, TRANSPORT_RCCL, dist as pdist
    from pmf_hip.engine import Context
    rng = np.random.default_rng(0)
    U, K = 10, 20
    comm = pdist.Comm(0, 1, 0, Context.comm_unique_id(), "rccl")
    try:
        for array in (ARR_FACTOR, ARR_COV):
            monkeypatch.setenv("PMF_STAGE_BYTES", str(3 * _row_bytes(K, "f32", array)))
            with pmf_hip.Context(U, 4, K, dtype="f32") as ctx:
                comm.attach(ctx)
                assert ctx.comm_info() == (1, 0, TRANSPORT_RCCL)
                ctx.set_array(USER, array, _host_array(rng, U, K, array))
                full = ctx.get_array(USER, array)
                assert np.array_equal(ctx.gather_user_rows(array, [0, U]), full)
                assert np.abs(full[-1]).max() > 0
        values = rng.standard_normal(8193)
        assert np.array_equal(comm.all_reduce_host(values), values)
        assert np.array_equal(comm.all_reduce_host(values, op="max"), values)
    finally:
        comm.close()
