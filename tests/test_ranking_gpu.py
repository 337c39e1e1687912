"""`pmf_rank_items`: the rank of held-out items among a user's candidates, against an fp64 NumPy ranking of what the
device holds (`ctx.get_array`), as tests/test_topk_gpu.py does for the top-k lists.  Most tables here are small integers:
every score is then exact in fp32 in any summation order, the data is full of exact ties, and the device must give
NumPy's ranks exactly."""
import numpy as np
import pytest

from helpers import frames, load_case

pytestmark = pytest.mark.gpu


# ---- the reference ---------------------------------------------------------------------------------------------------
def _device_scores(ctx, mode):
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ARR_SCALE, ITEM, USER
    full = ctx.get_array(USER, ARR_FACTOR) @ ctx.get_array(ITEM, ARR_FACTOR).T
    if mode == pmf_hip.PREDICT_BIAS:
        full = ctx.get_array(USER, ARR_BIAS)[:, None] + ctx.get_array(ITEM, ARR_BIAS)[None, :] + full
    if mode == pmf_hip.PREDICT_SCALE:
        full = full * (ctx.get_array(USER, ARR_SCALE)[:, None] * ctx.get_array(ITEM, ARR_SCALE)[None, :])
    return full


def _ref_rows(full, users, targets, train=None):
    """NumPy ranks / candidates of a CSR batch: `targets[r]` are the target items of row r (user users[r]); `train` maps
    a user to the set of its training items (excluded as competitors and candidates)."""
    ids = np.arange(full.shape[1])
    ranks, cand = [], []
    with np.errstate(invalid="ignore"):
        for u, tg in zip(users, targets):
            s = full[u]
            ok = np.ones(len(s), dtype=bool)
            if train is not None and train.get(int(u)):
                ok[list(train[int(u)])] = False
            cand.append(int((ok & ~np.isnan(s)).sum()))
            for i in tg:
                if np.isnan(s[i]):
                    ranks.append(-1)
                    continue
                before = (s > s[i]) | ((s == s[i]) & (ids < i))
                ranks.append(int((before & ok & (ids != i)).sum()))
    return np.array(ranks, dtype=np.int64), np.array(cand, dtype=np.int64)


def _csr(targets):
    row_ptr = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int64)
    items = np.concatenate([np.asarray(t, dtype=np.int64) for t in targets]) if len(targets) else np.zeros(0, dtype=np.int64)
    return row_ptr, items


def _integer_tables(rng, U, I, K, signed):
    if signed:
        A, B = rng.integers(-2, 3, (U, K)).astype(float), rng.integers(-2, 3, (I, K)).astype(float)
    else:
        A, B = rng.integers(0, 4, (U, K)).astype(float), rng.integers(0, 4, (I, K)).astype(float)
    bias = (rng.integers(-3, 4, U).astype(float), rng.integers(-3, 4, I).astype(float))
    scale = (rng.integers(1, 4, U).astype(float), rng.integers(1, 4, I).astype(float))
    return A, B, bias, scale


def _fill(ctx, A, B, bias, scale, mode):
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_FACTOR, ARR_SCALE, ITEM, USER
    ctx.set_array(USER, ARR_FACTOR, A); ctx.set_array(ITEM, ARR_FACTOR, B)
    if mode == pmf_hip.PREDICT_BIAS:
        ctx.set_array(USER, ARR_BIAS, bias[0]); ctx.set_array(ITEM, ARR_BIAS, bias[1])
    if mode == pmf_hip.PREDICT_SCALE:
        ctx.set_array(USER, ARR_SCALE, scale[0]); ctx.set_array(ITEM, ARR_SCALE, scale[1])


def _main_problem(K, signed, seed=0):
    """U = 333 users x I = 1999 items (neither a multiple of 32) of integer tables with the layouts that can go wrong."""
    rng = np.random.default_rng(1000 * K + seed)
    U, I = 333, 1999
    A, B, bias, scale = _integer_tables(rng, U, I, K, signed)
    B[17] = B[1500] = B[5]                      # duplicate item rows: exact ties among one user's targets
    bias[1][[17, 1500]] = bias[1][5]
    scale[1][[17, 1500]] = scale[1][5]
    B[77] = np.nan                              # a NaN item row: never outranks, no candidate, rank -1 as a target
    A[21] = np.nan                              # a NaN user row: every rank -1, no candidates
    A[13] = 0.0                                 # an all-zero user (zeros of both signs with signed items)
    users = [0, 7, 9, 11, 13, 21, 7, 30, 332, 331]
    targets = [[],                                                       # a row without targets
               rng.permutation(I)[:70].tolist(),                         # 70 targets: many query rows
               rng.permutation(I).tolist(),                              # all items: ranks are a permutation
               [1500, 5, 17],                                            # the three tied rows
               [3, 77, 1998, 0],                                         # the all-zero user; one NaN target
               [4, 5],                                                   # the NaN user
               [1, 2, 3],                                                # user 7 again
               [77], [1998], [0]]
    for u in rng.permutation(U)[:150]:                                   # one target each
        users.append(int(u))
        targets.append([int(rng.integers(I))])
    return A, B, bias, scale, np.array(users), targets


_ENV = {"": {}, "targets2": {"PMF_RANK_TARGETS": "2"}, "blocks2": {"PMF_TOPK_MAX_BLOCKS": "2"}}


# every K x score mode x dtype; the environment variations (read when the context is created) on the fused kernel's K classes
_CASES = [(K, mode, dtype, "") for K in (8, 20, 64, 100, 128, 136) for mode in (0, 1, 2) for dtype in ("f32", "f64")]
_CASES += [(K, mode, "f32", env) for K in (20, 64, 128) for mode in (0, 1, 2) for env in ("targets2", "blocks2")]


@pytest.mark.parametrize("K,mode,dtype,env", _CASES)
def test_ranks_equal_numpy_on_integer_tables(K, mode, dtype, env, monkeypatch):
    import pmf_hip
    for name, value in _ENV[env].items():
        monkeypatch.setenv(name, value)                                  # read when the context is created
    signed = (K + mode) % 2 == 1
    A, B, bias, scale, users, targets = _main_problem(K, signed)
    row_ptr, items = _csr(targets)
    with pmf_hip.Context(A.shape[0], B.shape[0], K, dtype=dtype) as ctx:
        _fill(ctx, A, B, bias, scale, mode)
        ranks, cand = ctx.rank_rows(users, row_ptr, items, use_bias=mode)
        full = _device_scores(ctx, mode)
    want_r, want_c = _ref_rows(full, users, targets)
    assert np.array_equal(cand, want_c)
    assert np.array_equal(ranks, want_r)
    all_items = ranks[row_ptr[2]:row_ptr[3]]                             # user 9: every item is a target
    ranked = all_items[all_items >= 0]
    assert len(ranked) == len(all_items) - 1 and np.array_equal(np.sort(ranked), np.arange(len(ranked)))
    assert (ranks[row_ptr[5]:row_ptr[6]] == -1).all() and cand[5] == 0   # the NaN user
    assert cand[0] == B.shape[0] - 1                                     # the row without targets still has candidates


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("U,I,K,mode", [(5000, 7, 8, 0), (5000, 70, 20, 1), (5000, 70, 64, 2), (3, 40000, 64, 0), (3, 40000, 100, 1)])
def test_ranks_equal_numpy_on_edge_shapes(U, I, K, mode, dtype):
    """Fewer items than one tile, a few tiles and many user tiles; three users over 40,000 items (the item range is cut
    into segments whose counts are added)."""
    import pmf_hip
    rng = np.random.default_rng(U + I + K)
    A, B, bias, scale = _integer_tables(rng, U, I, K, signed=True)
    users = np.arange(U)
    targets = [rng.integers(0, I, 1 + (u % 97 == 0) * 6).tolist() for u in users]
    if U == 3:
        B[39999] = B[11] = B[20000]                                      # ties across segments
        targets = [[39999, 11, 20000, 5], rng.integers(0, I, 9).tolist(), [0]]
    row_ptr, items = _csr(targets)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        _fill(ctx, A, B, bias, scale, mode)
        ranks, cand = ctx.rank_rows(users, row_ptr, items, use_bias=mode)
        full = _device_scores(ctx, mode)
    want_r, want_c = _ref_rows(full, users, targets)
    assert np.array_equal(cand, want_c) and np.array_equal(ranks, want_r)


def _one_target_rows(rng, U, I, n_random):
    """Rows of at most one target each -- the call then runs the scan's one-slot instantiation, a kernel of its own beside
    the four-slot one: the tie group 5 / 17 / 1500 as three rows of one user, the NaN item as a target, the NaN user, the
    all-zero user, the first and the last item, rows without a target, repeated users."""
    users = [11, 11, 11, 30, 21, 13, 13, 0, 7, 7, 7, 2, 1]
    targets = [[1500], [5], [17], [77], [4], [77], [I - 1], [], [0], [I - 1], [3], [], [1500]]
    for u in rng.integers(0, U, n_random):
        users.append(int(u))
        targets.append([int(rng.integers(I))])
    return np.array(users) % U, targets


# K = 8, 20, 64, 100 and 128: the scan's register classes KH = 8, 16, 32, 64 and 64
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("K", [8, 20, 64, 100, 128])
def test_one_target_rows_equal_numpy_on_integer_tables(K, mode):
    import pmf_hip
    A, B, bias, scale, _, _ = _main_problem(K, signed=(K + mode) % 2 == 0, seed=2)
    U, I = A.shape[0], B.shape[0]
    users, targets = _one_target_rows(np.random.default_rng(K + mode), U, I, 400)
    row_ptr, items = _csr(targets)
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        _fill(ctx, A, B, bias, scale, mode)
        ranks, cand = ctx.rank_rows(users, row_ptr, items, use_bias=mode)
        flat_r, flat_c = ctx.rank_items(users[row_ptr[:-1] < row_ptr[1:]], items, use_bias=mode)      # the same as flat pairs
        full = _device_scores(ctx, mode)
    want_r, want_c = _ref_rows(full, users, targets)
    assert np.array_equal(cand, want_c) and np.array_equal(ranks, want_r)
    assert np.array_equal(flat_r, want_r) and np.array_equal(flat_c, want_c[row_ptr[:-1] < row_ptr[1:]])
    assert ranks[3] == -1 and ranks[4] == -1 and cand[4] == 0            # the NaN item as a target; the NaN user
    assert ranks[1] < ranks[2] < ranks[0]                                # the tie group ranks by item id: 5, 17, 1500


@pytest.mark.parametrize("K,mode,max_blocks", [(8, 1, 0), (20, 2, 0), (64, 0, 0), (64, 1, 2), (100, 0, 0)])
def test_one_target_rows_over_item_segments_and_many_user_tiles(K, mode, max_blocks, monkeypatch):
    """The one-slot scan where the item range is cut into segments (3 users x 40,000 items: the segments' counts are
    added) and where blocks walk many user tiles (5,000 rows x 70 items; `max_blocks`: two blocks walk all of them)."""
    import pmf_hip
    if max_blocks:
        monkeypatch.setenv("PMF_TOPK_MAX_BLOCKS", str(max_blocks))
    rng = np.random.default_rng(K)
    for U, I in ((3, 40000), (5000, 70)):
        A, B, bias, scale = _integer_tables(rng, U, I, K, signed=True)
        B[I - 1] = B[11] = B[I // 2]                                     # ties across segments
        bias[1][[I - 1, 11]], scale[1][[I - 1, 11]] = bias[1][I // 2], scale[1][I // 2]
        B[40] = np.nan
        if U == 3:
            users = np.array([0, 0, 0, 1, 2, 2, 1, 0, 2])
            targets = [[I - 1], [11], [I // 2], [40], [0], [], [I - 2], [31], [32]]
        else:
            users = rng.permutation(U)
            targets = [[int(rng.integers(I))] for _ in users]
        row_ptr, items = _csr(targets)
        with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
            _fill(ctx, A, B, bias, scale, mode)
            ranks, cand = ctx.rank_rows(users, row_ptr, items, use_bias=mode)
            full = _device_scores(ctx, mode)
        want_r, want_c = _ref_rows(full, users, targets)
        assert np.array_equal(cand, want_c) and np.array_equal(ranks, want_r), (U, I)


@pytest.mark.parametrize("K,mode", [(20, 1), (64, 0), (100, 2)])
def test_one_target_rows_with_exclusion(K, mode):
    import pmf_hip
    A, B, bias, scale, _, _ = _main_problem(K, signed=K == 20, seed=3)
    U, I = A.shape[0], B.shape[0]
    rng = np.random.default_rng(K)
    users, targets = _one_target_rows(rng, U, I, 300)
    tu, ti = rng.integers(0, U, 5000), rng.integers(0, I, 5000)
    keep = tu != 2                                                       # user 2: no ratings
    tu, ti = np.concatenate([tu[keep], tu[keep][:300], [11, 11, 7]]), np.concatenate([ti[keep], ti[keep][:300], [5, 17, 3]])
    train = {}                                                           # (duplicate pairs; targets that are training items)
    for u, i in zip(tu.tolist(), ti.tolist()):
        train.setdefault(u, set()).add(i)
    row_ptr, items = _csr(targets)
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        _fill(ctx, A, B, bias, scale, mode)
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        ranks, cand = ctx.rank_rows(users, row_ptr, items, use_bias=mode, exclude_train=True)
        full = _device_scores(ctx, mode)
    want_r, want_c = _ref_rows(full, users, targets, train)
    assert np.array_equal(cand, want_c) and np.array_equal(ranks, want_r)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K,mode,env", [(20, 0, ""), (64, 1, ""), (64, 0, "targets2"), (128, 2, ""), (136, 1, "")])
def test_exclusion_of_training_items(K, mode, env, dtype, monkeypatch):
    import pmf_hip
    for name, value in _ENV[env].items():
        monkeypatch.setenv(name, value)
    A, B, bias, scale, users, targets = _main_problem(K, signed=K % 3 == 0, seed=1)
    U, I = A.shape[0], B.shape[0]
    rng = np.random.default_rng(K)
    tu, ti = rng.integers(0, U, 6000), rng.integers(0, I, 6000)
    keep = (tu != 2) & (tu != 3)                                         # user 2: no ratings
    tu, ti = tu[keep], ti[keep]
    tu, ti = np.concatenate([tu, tu[:500]]), np.concatenate([ti, ti[:500]])             # duplicate (u, i) pairs
    lone = 1234                                                          # user 3 rated every item but this one (77, the NaN row, too)
    tu, ti = np.concatenate([tu, np.full(I - 1, 3)]), np.concatenate([ti, np.delete(np.arange(I), lone)])
    tu, ti = np.concatenate([tu, [7, 7, 11]]), np.concatenate([ti, [targets[1][0], targets[1][0], 5]])   # targets that are training items
    order = rng.permutation(len(tu))
    tu, ti = tu[order], ti[order]
    users = np.concatenate([users, [2, 3]])
    targets = targets + [[8, 9], [lone]]
    train = {}
    for u, i in zip(tu.tolist(), ti.tolist()):
        train.setdefault(u, set()).add(i)
    row_ptr, items = _csr(targets)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        _fill(ctx, A, B, bias, scale, mode)
        with pytest.raises(pmf_hip.PmfError, match="ratings"):
            ctx.rank_rows(users, row_ptr, items, use_bias=mode, exclude_train=True)
        ctx.set_ratings(tu, ti, np.ones(len(tu)))
        ranks, cand = ctx.rank_rows(users, row_ptr, items, use_bias=mode, exclude_train=True)
        bytes_1 = ctx.device_bytes()
        ranks_2, cand_2 = ctx.rank_rows(users, row_ptr, items, use_bias=mode, exclude_train=True)
        bytes_2 = ctx.device_bytes()
        plain, plain_c = ctx.rank_rows(users, row_ptr, items, use_bias=mode)           # the lists do not leak into a plain call
        full = _device_scores(ctx, mode)
    want_r, want_c = _ref_rows(full, users, targets, train)
    assert np.array_equal(cand, want_c) and np.array_equal(ranks, want_r)
    assert np.array_equal(ranks_2, ranks) and np.array_equal(cand_2, cand) and bytes_2 == bytes_1
    assert ranks[-1] == 0 and cand[-1] == 1                              # user 3: the one item left
    assert cand[-2] == I - 1                                             # user 2: nothing excluded but the NaN item
    ref_r, ref_c = _ref_rows(full, users, targets)
    assert np.array_equal(plain, ref_r) and np.array_equal(plain_c, ref_c)


@pytest.mark.parametrize("dtype,K,mode", [("f32", 64, 0), ("f32", 20, 1), ("f64", 16, 2), ("f64", 40, 0)])
def test_ranks_of_the_topk_list_are_its_positions(dtype, K, mode):
    """rank_items(u repeated k, topk_items(u, k)) = 0 .. k - 1, for k = 10 and k = n_items: the two calls share one order.
    Integer tables in fp32 (exact in any summation order), real-valued ones in fp64."""
    import pmf_hip
    rng = np.random.default_rng(K)
    U, I = 60, 517
    if dtype == "f32":
        A, B, bias, scale = _integer_tables(rng, U, I, K, signed=mode == 1)
    else:
        A, B = rng.gamma(0.5, 1.0, (U, K)), rng.gamma(0.5, 1.0, (I, K))
        bias, scale = (rng.normal(size=U), rng.normal(size=I)), (rng.gamma(2.0, 1.0, U), rng.gamma(2.0, 1.0, I))
    B[400] = B[3]
    bias[1][400], scale[1][400] = bias[1][3], scale[1][3]
    users = np.arange(U)
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        _fill(ctx, A, B, bias, scale, mode)
        for k in (10, I):
            items, _ = ctx.topk_items(users, k, use_bias=mode)
            ranks, cand = ctx.rank_items(np.repeat(users, k), items.reshape(-1), use_bias=mode)
            assert np.array_equal(ranks.reshape(U, k), np.tile(np.arange(k), (U, 1))), k
            assert (cand == I).all()


@pytest.mark.parametrize("K", [8, 20, 64, 100, 128])
def test_real_valued_fp32_ranks_stay_within_the_near_ties(K):
    """Gamma(0.5, 1) factors as in test_topk_matches_numpy_ranking.  The fp32 summation order differs from NumPy's fp64
    product, so a rank may differ from the fp64 one by at most the number of other items whose fp64 score lies within
    1e-5 |s_ui| of the target's (the relative slack that test grants), and at least 99 % of the pairs must agree
    exactly."""
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(K)
    U, I, n = 333, 1999, 4000
    A, B = rng.gamma(0.5, 1.0, (U, K)), rng.gamma(0.5, 1.0, (I, K))
    pu, pi = rng.integers(0, U, n), rng.integers(0, I, n)
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        ctx.set_array(USER, ARR_FACTOR, A); ctx.set_array(ITEM, ARR_FACTOR, B)
        ranks, cand = ctx.rank_items(pu, pi)
        full = ctx.get_array(USER, ARR_FACTOR) @ ctx.get_array(ITEM, ARR_FACTOR).T
    assert (cand == I).all()
    rows = full[pu]
    own = rows[np.arange(n), pi][:, None]
    ids = np.arange(I)[None, :]
    rank64 = ((rows > own) | ((rows == own) & (ids < pi[:, None]))).sum(axis=1)
    near = (np.abs(rows - own) <= 1e-5 * np.abs(own)).sum(axis=1) - 1          # other items within the slack
    off = np.abs(ranks - rank64)
    print(f"K={K}: exact share {np.mean(off == 0):.4f}, largest |rank - rank64| {off.max()}, pairs off {int((off > 0).sum())}")
    assert (off <= near).all()
    assert np.mean(off == 0) >= 0.99


def test_argument_errors():
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(0)
    U, I, K = 40, 50, 8
    with pmf_hip.Context(U, I, K, dtype="f32") as ctx:
        with pytest.raises(pmf_hip.PmfError, match="has not been set"):
            ctx.rank_items([0], [0])
        ctx.set_array(USER, ARR_FACTOR, rng.normal(size=(U, K))); ctx.set_array(ITEM, ARR_FACTOR, rng.normal(size=(I, K)))
        with pytest.raises(pmf_hip.PmfError, match="outside"):
            ctx.rank_items([0, U], [1, 1])
        with pytest.raises(pmf_hip.PmfError, match="outside"):
            ctx.rank_items([0, 1], [1, I])
        with pytest.raises(pmf_hip.PmfError, match="outside"):
            ctx.rank_items([0, 1], [-1, 2])
        with pytest.raises(pmf_hip.PmfError, match="row_ptr"):
            ctx.rank_rows([0, 1], [0, 2, 1], [1])
        with pytest.raises(pmf_hip.PmfError, match="row_ptr"):
            ctx.rank_rows([0, 1], [1, 1, 2], [1, 2])
        with pytest.raises(pmf_hip.PmfError, match="use_bias"):
            ctx.rank_items([0], [0], use_bias=3)
        with pytest.raises(pmf_hip.PmfError, match="has not been set"):
            ctx.rank_items([0], [0], use_bias=pmf_hip.PREDICT_BIAS)
        ranks, cand = ctx.rank_items([], [])                              # n_rows = 0
        assert ranks.shape == (0,) and cand.shape == (0,) and ranks.dtype == np.int64
        ranks, cand = ctx.rank_rows([3, 4], [0, 0, 0], [])                # rows without targets
        assert ranks.shape == (0,) and cand.tolist() == [I, I]


@pytest.mark.parametrize("case", ["hpf_s7_k16", "gauss_bias_s7_k16", "poisson_ext_s7_k16"])
def test_models_evaluate_ranking_like_numpy(case):
    from src.evaluation.ranking import ranking_metrics
    d, meta = load_case(case)
    train, val = frames(d)
    kw = dict(meta["base_cfg"], n_factors=meta["K"], random_state=meta["seed"], max_iter=5, verbose=False)
    if meta["kind"] == "hpf":
        from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
        m = HPF_CAVI(HPF_CAVI_Config(tol=None, **kw), dtype="f64").fit(train)
        full = m.E_theta @ m.E_beta.T
    elif case.startswith("gauss"):
        from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
        m = GaussianMFCAVI(GaussianMFCAVIConfig(tol=0.0, **kw), dtype="f64").fit(train, global_mean=float(d["global_mean"]))
        full = m.m_user_bias[:, None] + m.m_item_bias[None, :] + m.m_theta @ m.m_beta.T
    else:
        from src.models.poisson_mf_extended_cavi import PoissonMFExtendedCAVI, PoissonMFExtendedCAVIConfig
        m = PoissonMFExtendedCAVI(PoissonMFExtendedCAVIConfig(tol=None, **kw), dtype="f64").fit(train)
        full = (m.E_phi[:, None] * m.E_psi[None, :]) * (m.E_theta @ m.E_beta.T)
    # some validation rows carry ids the fit has not seen: append two more so that the case is never empty
    import pandas as pd
    val = pd.concat([val, pd.DataFrame({"u": [m.n_users + 3, 0], "i": [0, m.n_items], "rating": [1.0, 1.0]})], ignore_index=True)
    vu, vi = val["u"].to_numpy(), val["i"].to_numpy()
    seen = (vu < m.n_users) & (vi < m.n_items)
    train_sets = {}
    for u, i in zip(train["u"].tolist(), train["i"].tolist()):
        train_sets.setdefault(u, set()).add(i)
    for exclude in (True, False):
        ranks, cand = m.heldout_ranks(val, exclude_train=exclude)
        assert ranks.shape == cand.shape == (len(val),)
        assert (ranks[~seen] == -1).all() and (cand[~seen] == -1).all() and (ranks[seen] >= 0).all()
        want_r, want_c = _ref_rows(full, vu[seen], [[i] for i in vi[seen]], train_sets if exclude else None)
        assert np.array_equal(ranks[seen], want_r) and np.array_equal(cand[seen], want_c)      # aligned with the frame
        got = m.evaluate_ranking(val, ks=(5, 10), exclude_train=exclude)
        all_r, all_c = np.full(len(val), -1), np.full(len(val), -1)
        all_r[seen], all_c[seen] = want_r, want_c
        want = ranking_metrics(vu, all_r, all_c, ks=(5, 10))
        assert got["n_skipped"] == int((~seen).sum()) >= 2 and got["n_pairs"] == int(seen.sum())
        for name, value in want.items():
            assert got[name] == pytest.approx(value, rel=1e-12, abs=1e-12), name
    m.close()
