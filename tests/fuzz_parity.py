"""Randomised parity sweep: the model classes (HIP engine, f64 parity mode and f32) against the CPU oracle on many
small random problems -- odd shapes (one user, one item, one factor, one rating), duplicates, rows far longer than a
task, empty rows, validation ids outside the training range.  Prints the worst deviation per model kind and every
failing case.  Test infrastructure (it drives the oracle): `tests/test_fuzz_gpu.py` runs a short sweep;
    python tests/fuzz_parity.py [n_trials] [seed]    runs a long one."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "prob-matrix-factorization_amd"), ROOT]
import numpy as np, pandas as pd
from oracle import cavi_oracle as orc
from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
from src.models.poisson_mf_extended_cavi import PoissonMFExtendedCAVI, PoissonMFExtendedCAVIConfig
from src.models import gaussian_mf_cavi as gnb, gaussian_mf_cavi_bias as gb

KEYS = {
    "hpf": ["gamma_a_theta", "gamma_b_theta", "gamma_a_beta", "gamma_b_beta", "E_theta", "E_beta", "E_xi", "E_eta",
            "gamma_b_xi", "gamma_b_eta"],
    "poisson": ["a_theta", "b_theta", "a_beta", "b_beta", "E_theta", "E_beta"],
    "poisson_ext": ["a_theta", "b_theta", "a_beta", "b_beta", "a_phi", "b_phi", "a_psi", "b_psi", "E_theta", "E_beta",
                    "E_phi", "E_psi"],
    "gauss_bias": ["m_theta", "m_beta", "V_theta", "V_beta", "m_user_bias", "m_item_bias"],
    "gauss": ["m_theta", "m_beta", "V_theta", "V_beta"],
    "sgd": ["m_theta", "m_beta", "m_user_bias", "m_item_bias"],     # gradient mode: no reference counterpart, own oracle
}


def problem(rng):
    shape = rng.choice(["tiny", "one_user", "one_item", "heavy_row", "plain", "sparse"])
    U, I = int(rng.integers(1, 70)), int(rng.integers(1, 50))
    N = int(rng.integers(1, 500))
    if shape == "tiny":
        U, I, N = int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 6))
    if shape == "one_user":
        U = 1
    if shape == "one_item":
        I = 1
    u, i = rng.integers(0, U, N), rng.integers(0, I, N)
    if shape == "heavy_row":                      # one row holds most ratings (several tasks), duplicates included
        u[: (3 * N) // 4] = int(rng.integers(0, U))
        i[: N // 2] = int(rng.integers(0, I))
    if shape == "sparse":                         # ids far apart: most rows are empty
        U, I = U * 7, I * 5
        u, i = u * 7, i * 5
    x = rng.integers(0, 6, N).astype(np.float64)
    nv = int(rng.integers(1, 40))
    vu, vi = rng.integers(0, U + 3, nv), rng.integers(0, I + 3, nv)      # some ids outside the training range
    vx = rng.integers(0, 6, nv).astype(np.float64)
    return shape, u, i, x, (vu, vi, vx)


def run(kind, dtype, u, i, x, val, K, seed, iters, tol_gamma=None, tol_gauss=-1e9):
    train = pd.DataFrame({"u": u, "i": i, "rating": x})
    vdf = pd.DataFrame({"u": val[0], "i": val[1], "rating": val[2]})
    gm = 0.0
    if kind == "hpf":
        cfg = dict(n_factors=K, a=0.3, a_prime=2.0, b_prime=1.5, c=0.4, c_prime=3.0, d_prime=0.7, max_iter=iters,
                   tol=tol_gamma, random_state=seed)
        train["rating"] += 1; vdf["rating"] += 1
        m = HPF_CAVI(HPF_CAVI_Config(verbose=False, **cfg), dtype=dtype)
    elif kind == "poisson":
        cfg = dict(n_factors=K, a0=0.2, b0=0.6, max_iter=iters, tol=tol_gamma, random_state=seed)
        m = PoissonMFCAVI(PoissonMFCAVIConfig(verbose=False, **cfg), dtype=dtype)
    elif kind == "poisson_ext":
        cfg = dict(n_factors=K, a0=0.2, b0=0.6, max_iter=iters, tol=None, random_state=seed)
        train["rating"] += 1; vdf["rating"] += 1
        m = PoissonMFExtendedCAVI(PoissonMFExtendedCAVIConfig(verbose=False, **cfg), dtype=dtype)
    elif kind == "sgd":
        from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
        cfg = dict(n_factors=K, sigma2=0.4, eta_theta2=0.6, eta_beta2=0.9, eta_bias2=1.3, lr=0.02, max_iter=iters, tol=-1e9,
                   random_state=seed)
        gm = float(train["rating"].mean())
        train["rating"] -= gm; vdf["rating"] -= gm
        m = GaussianMFSGD(GaussianMFSGDConfig(verbose=False, **cfg), dtype=dtype)
    else:
        cfg = dict(n_factors=K, sigma2=0.4, eta_theta2=0.6, eta_beta2=0.9, max_iter=iters, tol=tol_gauss, random_state=seed)
        gm = float(train["rating"].mean())
        train["rating"] -= gm; vdf["rating"] -= gm
        if kind == "gauss_bias":
            cfg["eta_bias2"] = 1.3
            m = gb.GaussianMFCAVI(gb.GaussianMFCAVIConfig(verbose=False, **cfg), dtype=dtype)
        else:
            m = gnb.GaussianMFCAVI(gnb.GaussianMFCAVIConfig(verbose=False, **cfg), dtype=dtype)
    tr = (train["u"].to_numpy(), train["i"].to_numpy(), train["rating"].to_numpy())
    va = (vdf["u"].to_numpy(), vdf["i"].to_numpy(), vdf["rating"].to_numpy())
    if kind.startswith("gauss") or kind == "sgd":
        m.fit(train, vdf, global_mean=gm)
    else:
        m.fit(train, vdf)
    if kind == "sgd":
        U_, I_ = orc.infer_dims(tr[0], tr[1])
        st = orc.init_gaussian(U_, I_, K, seed, bias=True)
        idx_ = (orc.group_positions(tr[0], U_), orc.group_positions(tr[1], I_))
        hist = {"val_rmse": []}
        for _ in range(iters):
            orc.gauss_sgd_epoch(st, idx_, tr[0], tr[1], tr[2], cfg["lr"], cfg["sigma2"], cfg["eta_theta2"], cfg["eta_beta2"],
                                cfg["eta_bias2"])
            hist["val_rmse"].append(orc.gaussian_eval(st, va[0], va[1], va[2], gm, bias=True)[0])
    else:
        st, hist = orc.fit(kind, *tr, cfg, val=va, global_mean=gm)
    worst = 0.0
    for key in KEYS[kind]:
        got, want = np.asarray(getattr(m, key), dtype=np.float64), np.asarray(st[key], dtype=np.float64)
        if got.shape != want.shape:
            return float("inf"), f"{key}: shape {got.shape} != {want.shape}"
        scale = max(1.0, float(np.max(np.abs(want))) if want.size else 1.0)
        err = float(np.max(np.abs(got - want))) / scale if want.size else 0.0
        if not np.isfinite(err):
            return float("inf"), f"{key}: non-finite"
        worst = max(worst, err)
    if kind not in ("sgd", "poisson_ext") and (m.history_["iterations"], m.history_["stopped_early"]) != \
            (hist["iterations"], hist["stopped_early"]):
        return float("inf"), f"stopped after {m.history_['iterations']} ({m.history_['stopped_early']}), oracle after " \
                             f"{hist['iterations']} ({hist['stopped_early']})"
    hv = np.asarray(m.history_["val_rmse"], dtype=np.float64)
    ov = np.asarray(hist["val_rmse"], dtype=np.float64)
    if hv.shape != ov.shape:
        return float("inf"), f"val_rmse trajectory length {hv.shape} != {ov.shape}"
    both_nan = np.isnan(hv) & np.isnan(ov)
    if hv.size and not np.all(both_nan | (np.abs(hv - ov) <= 1e-6 * np.maximum(1.0, np.abs(ov)) + (0 if dtype == "f64" else 1e-3))):
        return float("inf"), f"val_rmse {hv} != {ov}"
    # the fitted model's own API on fresh id lists (ids outside the trained range included)
    tol_api = 1e-9 if dtype == "f64" else 2e-3
    rng = np.random.default_rng(seed + 1)
    U, I = int(np.max(u)) + 1, int(np.max(i)) + 1
    qu, qi = rng.integers(0, U + 2, 25), rng.integers(0, I + 2, 25)
    if kind == "poisson_ext":
        want = orc.ext_predict(st, qu, qi)
        got = m.predict(qu, qi)
    elif kind.startswith("gauss") or kind == "sgd":
        bias = kind != "gauss"
        want = orc.predict_dot(st["m_theta"], st["m_beta"], qu, qi, st["m_user_bias"] if bias else None,
                               st["m_item_bias"] if bias else None, gm)
        got = m.predict(qu, qi, gm)
    else:
        want = orc.predict_dot(st["E_theta"], st["E_beta"], qu, qi)
        got = m.predict(qu, qi)
    if got.shape != want.shape or not np.allclose(got, want, rtol=tol_api, atol=tol_api):
        return float("inf"), f"predict {got} != {want}"
    if kind != "poisson_ext":
        if kind.startswith("gauss") or kind == "sgd":
            e_want = orc.gaussian_eval(st, va[0], va[1], va[2], gm, bias=(kind != "gauss"))
            e_got = (m.evaluate_rmse(vdf, gm), m.evaluate_macro_mae(vdf, gm))
        else:
            e_want = orc.gamma_eval(st, *va)
            e_got = (m.evaluate_rmse(vdf), m.evaluate_macro_mae(vdf))
        for a, b in zip(e_got, e_want):
            if not ((np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol_api * max(1.0, abs(b))):
                return float("inf"), f"evaluate {e_got} != {e_want}"
    # top-k under the model's own score: every returned list must be a correct ranking of its own predictions
    k = int(min(I, rng.integers(1, 8)))
    users = rng.integers(0, U, 6)
    items, scores = m.top_k_items(users, k)
    every = np.arange(I)
    for row, uu in enumerate(users):
        full = m.predict(np.full(I, uu), every, gm) - gm if (kind.startswith("gauss") or kind == "sgd") \
            else m.predict(np.full(I, uu), every)
        order = np.lexsort((every, -full))[:k]
        if not np.allclose(scores[row], full[items[row]], rtol=tol_api, atol=tol_api):
            return float("inf"), f"top-k scores {scores[row]} vs predict {full[items[row]]}"
        if not np.allclose(np.sort(full[items[row]])[::-1], full[order], rtol=10 * tol_api, atol=10 * tol_api):
            return float("inf"), f"top-k of user {uu}: {items[row]} vs {order}"
        if dtype == "f64" and len(set(np.round(full, 12))) == I and not np.array_equal(items[row], order):
            return float("inf"), f"top-k order of user {uu}: {items[row]} vs {order}"
    if hasattr(m, "close"):
        m.close()
    return worst, ""


def sweep(n_trials, seed, quiet=False):
    """Returns (failures, {(kind, dtype): worst deviation})."""
    rng = np.random.default_rng(seed)
    worst = {}
    bad = 0
    for t in range(n_trials):
        kind = str(rng.choice(list(KEYS)))
        dtype = str(rng.choice(["f64", "f64", "f32"]))
        K = int(rng.choice([1, 2, 3, 5, 8, 12, 16, 17, 24, 31, 32, 33, 40, 48, 49, 56, 57, 64, 65, 72, 79, 80, 81, 88, 95, 96, 100, 128, 130]))
        if (kind.startswith("gauss") or kind == "sgd") and K > 64 and rng.random() < 0.5:
            K = int(rng.integers(1, 64))              # keep most Gaussian cases cheap for the CPU oracle
        shape, u, i, x, val = problem(rng)
        seed, iters = int(rng.integers(0, 1000)), int(rng.integers(1, 4))
        tol = 1e-9 if dtype == "f64" else 5e-3
        tol_gamma, tol_gauss = None, -1e9
        if dtype == "f64" and rng.random() < 0.5:       # the early-stop rules (f64: the decision cannot hinge on rounding)
            iters = int(rng.integers(3, 8))
            tol_gamma = float(rng.choice([1e-3, 0.02, 0.2]))
            tol_gauss = float(rng.choice([1e-3, 0.02, -1.0]))
        try:
            err, msg = run(kind, dtype, u, i, x, val, K, seed, iters, tol_gamma, tol_gauss)
        except Exception as e:     # noqa: BLE001 -- the sweep reports and goes on
            err, msg = float("inf"), f"{type(e).__name__}: {e}"
        key = (kind, dtype)
        if err <= tol:
            worst[key] = max(worst.get(key, 0.0), err)
        else:
            bad += 1
            print(f"FAIL trial {t}: {kind} {dtype} K={K} shape={shape} U={u.max() + 1} I={i.max() + 1} N={len(u)} seed={seed} "
                  f"iters={iters}: err={err:.3e} {msg}", flush=True)
        if not quiet and t % 500 == 499:
            print(f"... {t + 1} trials, {bad} failures", flush=True)
    return bad, worst


def sweep_three_stage(n_trials, seed, quiet=False):
    """The multi-GPU code path against the fused one, on random problems: a context with a ONE-rank RCCL
    communicator runs its ITEM half-sweeps as accumulate -> ncclAllReduce per row chunk -> finalize on three
    streams, over a random number of item row chunks; a plain context runs the fused sweeps.  Same rows, same
    arithmetic: the states must agree to rounding (the split-row sums are combined in another kernel).
    Returns (failures, worst deviation)."""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER, dist as pdist
    from pmf_hip.engine import Context
    rng = np.random.default_rng(seed)
    comm = pdist.Comm(0, 1, 0, Context.comm_unique_id(), "rccl")
    bad, worst = 0, 0.0
    try:
        for t in range(n_trials):
            kind = str(rng.choice(["poisson", "hpf", "gauss", "sgd"]))
            dtype = str(rng.choice(["f64", "f32"]))
            K = int(rng.choice([1, 3, 8, 16, 20, 32, 33, 40, 50, 56, 64, 72, 96, 128, 140]))
            shape, u, i, x, _ = problem(rng)
            U, I = int(u.max()) + 1, int(i.max()) + 1
            n_chunks = int(rng.integers(1, min(I, 6) + 1))
            a_u, a_i = rng.gamma(1.0, 0.3, (U, K)) + 0.05, rng.gamma(1.0, 0.3, (I, K)) + 0.05
            m_u, m_i = 0.1 * rng.standard_normal((U, K)), 0.1 * rng.standard_normal((I, K))
            states = []
            try:
                for with_comm in (True, False):
                    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
                        if with_comm:
                            comm.attach(ctx)
                            ctx.comm_set_exchange(["allreduce", "scatter_gather"][t % 2])   # ncclAllReduce | ncclReduceScatter + ncclAllGather
                            ctx.set_row_chunks(ITEM, n_chunks)
                        if kind in ("poisson", "hpf"):
                            ctx.set_ratings(u, i, x + 1.0)
                            ctx.set_array(USER, ARR_FACTOR, a_u); ctx.set_array(ITEM, ARR_FACTOR, a_i)
                            if kind == "hpf":
                                ctx.set_array(USER, ARR_PRIOR_RATE, np.full(U, 1.3)); ctx.set_array(ITEM, ARR_PRIOR_RATE, np.full(I, 0.8))
                            for _ in range(2):
                                for side in (USER, ITEM):
                                    if kind == "hpf":
                                        ctx.gamma_sweep(side, 0.3, 0.0, True, 2.0 + K * 0.3, 1.5)
                                    else:
                                        ctx.gamma_sweep(side, 0.2, 0.6)
                            arrays = [(s, a) for s in (USER, ITEM) for a in (ARR_SHAPE, ARR_RATE, ARR_FACTOR)]
                            if kind == "hpf":
                                arrays += [(USER, ARR_PRIOR_RATE), (ITEM, ARR_PRIOR_RATE)]
                        else:
                            ctx.set_ratings(u, i, x - x.mean())
                            ctx.set_array(USER, ARR_FACTOR, m_u); ctx.set_array(ITEM, ARR_FACTOR, m_i)
                            ctx.set_array(USER, ARR_BIAS, np.zeros(U)); ctx.set_array(ITEM, ARR_BIAS, np.zeros(I))
                            if kind == "gauss":
                                ctx.set_cov_identity(USER); ctx.set_cov_identity(ITEM)
                            for _ in range(2):
                                if kind == "gauss":
                                    ctx.gauss_factor_sweep(USER, 0.4, 0.6); ctx.gauss_factor_sweep(ITEM, 0.4, 0.9)
                                    ctx.gauss_bias_sweep(USER, 0.4, 1.3); ctx.gauss_bias_sweep(ITEM, 0.4, 1.3)
                                else:
                                    ctx.gauss_sgd_sweep(USER, 0.05, 0.4, 0.6, 1.3); ctx.gauss_sgd_sweep(ITEM, 0.05, 0.4, 0.9, 1.3)
                            arrays = [(s, a) for s in (USER, ITEM) for a in (ARR_FACTOR, ARR_BIAS)]
                            if kind == "gauss":
                                arrays += [(USER, ARR_COV), (ITEM, ARR_COV)]
                        states.append([ctx.get_array(s, a) for s, a in arrays])
                err = 0.0
                for got, want in zip(*states):
                    scale = max(1.0, float(np.max(np.abs(want))) if want.size else 1.0)
                    e = float(np.max(np.abs(got - want))) / scale if want.size else 0.0
                    err = max(err, e if np.isfinite(e) else float("inf"))
                msg = ""
            except Exception as e:     # noqa: BLE001
                err, msg = float("inf"), f"{type(e).__name__}: {e}"
            if err <= (1e-11 if dtype == "f64" else 2e-4):
                worst = max(worst, err) if dtype == "f32" else worst
            else:
                bad += 1
                print(f"FAIL three-stage trial {t}: {kind} {dtype} K={K} shape={shape} U={U} I={I} N={len(u)} "
                      f"chunks={n_chunks}: err={err:.3e} {msg}", flush=True)
            if not quiet and t % 500 == 499:
                print(f"... three-stage {t + 1} trials, {bad} failures", flush=True)
    finally:
        comm.close()
    return bad, worst


def sweep_index(n_trials, seed):
    """Device index build (radix sort + row pointers, pmf_index.hip) against the host counting sort
    (PMF_INDEX_HOST=1) on random rating lists up to 60k entries: the fitted arrays must be bit-identical
    (both builds are stable, so every row sums its ratings in the same order)."""
    import fuzz_sharded
    rng = np.random.default_rng(seed)
    bad = 0
    for t in range(n_trials):
        kind = str(rng.choice(["hpf", "gauss_bias"]))
        U, I = int(rng.integers(1, 3000)), int(rng.integers(1, 800))
        N = int(rng.integers(1, 60000))
        u = rng.permutation(U)[np.floor(U * rng.random(N) ** 2.0).astype(np.int64)]
        i = rng.permutation(I)[np.floor(I * rng.random(N) ** 3.0).astype(np.int64)]
        x = rng.integers(0, 6, N).astype(np.float64)
        K = int(rng.choice([3, 16, 40]))
        train = pd.DataFrame({"u": u, "i": i, "rating": x})
        gm = float(x.mean())
        states = []
        try:
            for flag in (None, "1"):
                if flag:
                    os.environ["PMF_INDEX_HOST"] = flag
                m = fuzz_sharded.build(kind, K, 3, 2)
                if kind.startswith("gauss"):
                    m.fit(train.assign(rating=train["rating"] - gm), global_mean=gm)
                else:
                    m.fit(train.assign(rating=train["rating"] + 1.0))
                states.append([np.asarray(getattr(m, k)) for k in fuzz_sharded.KEYS[kind]])
                m.close()
            same = all(np.array_equal(a, b) for a, b in zip(*states))
            msg = "" if same else "arrays differ"
        except Exception as e:     # noqa: BLE001
            same, msg = False, f"{type(e).__name__}: {e}"
        finally:
            os.environ.pop("PMF_INDEX_HOST", None)
        if not same:
            bad += 1
            print(f"FAIL index trial {t}: {kind} K={K} U={U} I={I} N={N}: {msg}", flush=True)
    return bad


def sweep_medium(n_trials, seed):
    """Medium problems -- 2.2M to 9M ratings, where the HPF trials' work lists use 64-, 128- and 256-rating tasks (the
    small sweeps above see 32, the full-size tests 512) -- against the oracle's vectorised form: direct C-ABI sweeps,
    one iteration, f64 and f32.  The Gaussian trials stay below 4M ratings (the oracle is O(N K^2)), i.e. at 64-rating
    tasks: one batch of the accumulate kernels per task; longer Gaussian tasks are tests/test_gauss_long_tasks_gpu.py's.
    Returns (failures, worst f64 deviation)."""
    import pmf_hip
    from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER
    rng = np.random.default_rng(seed)
    bad, worst = 0, 0.0
    for t in range(n_trials):
        kind = "gauss" if t % 3 == 2 else "hpf"
        N = int(rng.integers(2_200_000, 9_000_000)) if kind == "hpf" else int(rng.integers(2_200_000, 4_000_000))
        U, I = int(rng.integers(20_000, 200_000)), int(rng.integers(500, 20_000))
        K = int(rng.choice([4, 12, 16, 32])) if kind == "hpf" else int(rng.choice([4, 8, 16]))
        dtype = str(rng.choice(["f64", "f32"]))
        u = rng.permutation(U)[np.floor(U * rng.random(N) ** 2.0).astype(np.int64)]
        i = rng.permutation(I)[np.floor(I * rng.random(N) ** 3.0).astype(np.int64)]
        u[0], i[0] = U - 1, I - 1
        x = rng.integers(0, 6, N).astype(np.float64)
        idx = (orc.group_positions(u, U), orc.group_positions(i, I))
        try:
            with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
                if kind == "hpf":
                    st = orc.init_hpf(U, I, K, 0.3, 5.0, 5.0, 0.3, 5.0, 5.0, seed=3)
                    ctx.set_ratings(u, i, x + 1.0)
                    ctx.set_array(USER, ARR_FACTOR, st["E_theta"]); ctx.set_array(ITEM, ARR_FACTOR, st["E_beta"])
                    ctx.set_array(USER, ARR_PRIOR_RATE, st["E_xi"]); ctx.set_array(ITEM, ARR_PRIOR_RATE, st["E_eta"])
                    orc.hpf_iteration(st, idx, u, i, x + 1.0, 0.3, 5.0, 0.3, 5.0, orc.gamma_half_sweep_segsum)
                    ctx.gamma_sweep(USER, 0.3, 0.0, True, st["gamma_a_xi"], 5.0)
                    ctx.gamma_sweep(ITEM, 0.3, 0.0, True, st["gamma_a_eta"], 5.0)
                    pairs = [("gamma_a_theta", USER, ARR_SHAPE), ("gamma_b_theta", USER, ARR_RATE), ("gamma_a_beta", ITEM, ARR_SHAPE),
                             ("gamma_b_beta", ITEM, ARR_RATE), ("E_theta", USER, ARR_FACTOR), ("E_beta", ITEM, ARR_FACTOR)]
                else:
                    st = orc.init_gaussian(U, I, K, 5, bias=True)
                    xc = x - x.mean()
                    ctx.set_ratings(u, i, xc)
                    ctx.set_array(USER, ARR_FACTOR, st["m_theta"]); ctx.set_array(ITEM, ARR_FACTOR, st["m_beta"])
                    ctx.set_cov_identity(USER); ctx.set_cov_identity(ITEM)
                    ctx.set_array(USER, ARR_BIAS, np.zeros(U)); ctx.set_array(ITEM, ARR_BIAS, np.zeros(I))
                    orc.gaussian_iteration(st, idx, u, i, xc, 0.4, 0.6, 0.9, 1.3, True)
                    ctx.gauss_factor_sweep(USER, 0.4, 0.6); ctx.gauss_factor_sweep(ITEM, 0.4, 0.9)
                    ctx.gauss_bias_sweep(USER, 0.4, 1.3); ctx.gauss_bias_sweep(ITEM, 0.4, 1.3)
                    pairs = [("m_theta", USER, ARR_FACTOR), ("m_beta", ITEM, ARR_FACTOR), ("V_theta", USER, ARR_COV),
                             ("V_beta", ITEM, ARR_COV), ("m_user_bias", USER, ARR_BIAS), ("m_item_bias", ITEM, ARR_BIAS)]
                err = 0.0
                for key, side, arr in pairs:
                    got, want = ctx.get_array(side, arr), st[key]
                    err = max(err, float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want))))))
            msg = ""
        except Exception as e:     # noqa: BLE001
            err, msg = float("inf"), f"{type(e).__name__}: {e}"
        if err <= (1e-9 if dtype == "f64" else 5e-4):
            worst = max(worst, err) if dtype == "f64" else worst
        else:
            bad += 1
            print(f"FAIL medium trial {t}: {kind} {dtype} K={K} U={U} I={I} N={N}: err={err:.3e} {msg}", flush=True)
    return bad, worst


def sweep_threads(n_threads, trials_per_thread, seed):
    """The same parity trials from several host threads at once, every thread on contexts of its own (what the
    tuner's concurrent trials do): distinct contexts are independent -- separate streams, buffers, error strings.
    Returns the number of failures over all threads."""
    import threading
    results = [None] * n_threads

    def work(k):
        results[k] = sweep(trials_per_thread, seed + k, quiet=True)[0]

    threads = [threading.Thread(target=work, args=(k,)) for k in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    return sum(r if r is not None else trials_per_thread for r in results)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    failures, worst_by_kind = sweep(n, int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    for k in sorted(worst_by_kind):
        print(f"{k[0]:12s} {k[1]}: worst relative deviation {worst_by_kind[k]:.2e}")
    print(f"{n} trials, {failures} failures")
    f3, w3 = sweep_three_stage(n // 2, 7)
    print(f"three-stage path vs fused sweeps: {n // 2} trials, {f3} failures, worst f32 deviation {w3:.2e}")
    fi = sweep_index(n // 10, 9)
    print(f"device index build vs host build: {n // 10} trials, {fi} failures")
    sys.exit(1 if failures or f3 or fi else 0)
