"""Every home of the Gaussian K x K row solve (csrc/pmf_gauss.hip) on planted matrices, against the float64 / long
double reference of tests/gauss_solver_reference.py, with the scaled errors bounded by C eps (kappa + K).

Sweep route: every row has exactly one rating, so row r solves S_r = A_r + m_r m_r' with w_r = x_r m_r from the
ITEM tables planted here -- a one-task row, which the fused kernels solve themselves.  Finalize route: exact S and an
unrelated w written as statistics rows, solved by the stand-alone kernels.  The K of the default path are ALL of them
(the dispatch decides which kernel a K gets, not a list); the other homes run at the edges of their size classes.
Each test prints its worst figures (ratio = scaled error / (eps (kappa + K)), to be compared with C) before asserting."""
import numpy as np
import pytest

import gauss_solver_reference as gsr

pytestmark = pytest.mark.gpu

# kernel switches, read when the context is created.  PMF_GAUSS_LDS_SOLVE only chooses among the stand-alone solvers, so
# it goes with PMF_GAUSS_UNFUSED: alone, the fused kernel would still solve every one-task row.
HOMES = {"default": (), "unfused": ("PMF_GAUSS_UNFUSED",), "generic": ("PMF_GAUSS_GENERIC",),
         "lds": ("PMF_GAUSS_UNFUSED", "PMF_GAUSS_LDS_SOLVE")}


def _has_fused_form(dtype, K):
    return K <= (128 if dtype == "f32" else 64)


def _block_kernel_place(dtype, K):
    return "LDS" if K <= (200 if dtype == "f32" else 141) else "scratch"


def _solver_name(dtype, K, home):
    """which code solves a one-task row (DESIGN.md section 4.3 tabulates the worst ratios under these names)"""
    if home == "default" and _has_fused_form(dtype, K):
        if dtype == "f64":
            return "fused, gauss_accum_generic_kernel<double>"
        return "fused, gauss_accum_mfma_kernel" if K <= 64 else "fused, gauss_accum_mfma128_kernel"
    if K <= 64:
        return f"gauss_solve_reg_kernel {dtype}"
    if dtype == "f32" and K <= 128 and home != "lds":
        return "gauss_solve_pair_kernel"
    return f"gauss_solve_lds_kernel {dtype} ({_block_kernel_place(dtype, K)})"


def _report(route, home, dtype, K, worst, fails):
    print(f"SOLVER route={route} home={home} dtype={dtype} K={K} solver=[{_solver_name(dtype, K, home)}] "
          f"ratioV={worst[0]:.3f} ratiom={worst[1]:.3f} kappa={worst[2]:.4g} ulps={worst[3]:.2f} C={gsr.C}")
    assert not fails, fails[:8]


def _sweep_rows(K, dtype, home, monkeypatch):
    """Plant the battery of (K, dtype), run the USER half-sweep under every pair of hyperparameters and judge every
    row; the launches of the solve class say which path ran."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM, USER
    for name in HOMES[home]:
        monkeypatch.setenv(name, "1")
    cases = gsr.battery(K, dtype)
    R = len(cases)
    x = np.array([c.x for c in cases])
    worst, fails = np.zeros(4), []
    with pmf_hip.Context(R, R, K, dtype=dtype) as ctx:
        ctx.set_ratings(np.arange(R), np.arange(R), x)
        ctx.set_array(ITEM, ARR_COV, np.stack([c.S - np.multiply.outer(c.m, c.m) for c in cases]))
        ctx.set_array(ITEM, ARR_FACTOR, np.stack([c.m for c in cases]))
        ctx.set_array(USER, ARR_FACTOR, np.zeros((R, K)))
        ctx.set_cov_identity(USER)
        # the reference is built from what the device holds
        A, M = ctx.get_array(ITEM, ARR_COV), ctx.get_array(ITEM, ARR_FACTOR)
        S = A + M[:, :, None] * M[:, None, :]
        w = gsr.rounded(x, dtype)[:, None] * M
        ctx.prof_enable(True)
        want_solves = 0 if home == "default" and _has_fused_form(dtype, K) else 1
        for sigma2, eta2 in gsr.PAIRS:
            ctx.prof_reset()
            ctx.gauss_factor_sweep(USER, sigma2, eta2)
            V, m = ctx.get_array(USER, ARR_COV), ctx.get_array(USER, ARR_FACTOR)
            solves = ctx.prof_get()["gauss_solve"][1]
            if solves != want_solves:
                fails.append(f"({sigma2}, {eta2}): {solves} launches in the solve class, expected {want_solves}")
            for r, c in enumerate(cases):
                figs, bad = gsr.judge(dtype, c.name, V[r], m[r], S[r], w[r], sigma2, eta2,
                                      ("sweep", dtype, K, c.name, sigma2, eta2))
                worst = np.maximum(worst, figs)
                fails += [f"{c.name} ({sigma2}, {eta2}): {b}" for b in bad]
    _report("sweep", home, dtype, K, worst, fails)


@pytest.mark.parametrize("dtype,K", [(d, K) for d in ("f32", "f64") for K in gsr.DEFAULT_K[d]])
def test_default_path(dtype, K, monkeypatch):
    """Every K: the fused homes (fp32 K <= 128, fp64 K <= 64 -- nothing launches in the solve class there) and the
    block-per-row kernel beyond, up to and across its LDS-to-scratch edge."""
    _sweep_rows(K, dtype, "default", monkeypatch)


@pytest.mark.parametrize("K", gsr.SMALL_EDGE_K)
@pytest.mark.parametrize("home,dtype", [("unfused", "f32"), ("unfused", "f64"), ("generic", "f32")])
def test_stand_alone_homes_one_wavefront(home, dtype, K, monkeypatch):
    """gauss_solve_reg_kernel behind the accumulate-only kernels, at the edges of its register classes (8 / 16 / 32 /
    64) and of the fused kernel's (48 / 56): exactly one solve launch per sweep."""
    _sweep_rows(K, dtype, home, monkeypatch)


@pytest.mark.parametrize("K", gsr.PAIR_EDGE_K)
@pytest.mark.parametrize("home", ["unfused", "lds", "generic"])
def test_stand_alone_homes_two_wavefronts(home, K, monkeypatch):
    """fp32, 64 < K <= 128: gauss_solve_pair_kernel at both sides of every tile-count and chunk-count edge (80 | 81,
    95 | 96, 112 | 113, 114 | 115), and the block-per-row kernel forced onto the same sizes."""
    _sweep_rows(K, "f32", home, monkeypatch)


@pytest.mark.parametrize("dtype,K", [(d, K) for d in ("f32", "f64") for K in gsr.FINALIZE_K[d]])
def test_finalize_route(dtype, K):
    """The battery's S exactly (packed lower triangle) and right-hand sides unrelated to it as statistics rows; a row
    of zero statistics keeps its COV / FACTOR row bit for bit."""
    import torch

    import pmf_hip
    from helpers import DeviceStats
    from pmf_hip import ARR_COV, ARR_FACTOR, ITEM
    cases = gsr.battery(K, dtype)
    R, zero_row = len(cases) + 1, 3
    rows = [r for r in range(R) if r != zero_row]
    rng = np.random.default_rng(K)
    worst, fails = np.zeros(4), []
    with pmf_hip.Context(1, R, K, dtype=dtype) as ctx:
        ctx.set_ratings(np.zeros(R, dtype=np.int64), np.arange(R), np.zeros(R))
        g = rng.normal(size=(R, K, K))
        ctx.set_array(ITEM, ARR_COV, g + np.swapaxes(g, 1, 2))
        ctx.set_array(ITEM, ARR_FACTOR, rng.normal(size=(R, K)))
        before = ctx.get_array(ITEM, ARR_COV)[zero_row], ctx.get_array(ITEM, ARR_FACTOR)[zero_row]
        width, kp = ctx.cov_stride + ctx.kpad, K * (K + 1) // 2
        S = np.stack([gsr.rounded(c.S, dtype) for c in cases])
        w = gsr.rounded(gsr.finalize_rhs(K, len(cases)), dtype)
        host = np.zeros((R, width), dtype=ctx.np_dtype)
        for q, r in enumerate(rows):
            host[r, :kp] = gsr.pack_lower(S[q])
            host[r, ctx.cov_stride:ctx.cov_stride + K] = w[q]
        stats = DeviceStats(R * width, ctx.np_dtype, "cuda:0")
        stats.tensor.copy_(torch.from_numpy(host.reshape(-1)))
        torch.cuda.synchronize()
        ctx.prof_enable(True)
        for sigma2, eta2 in gsr.PAIRS:
            ctx.prof_reset()
            ctx.gauss_factor_finalize(ITEM, stats.ptr, sigma2, eta2)
            V, m = ctx.get_array(ITEM, ARR_COV), ctx.get_array(ITEM, ARR_FACTOR)
            if ctx.prof_get()["gauss_solve"][1] != 1:
                fails.append(f"({sigma2}, {eta2}): not one solve launch")
            if not (np.array_equal(V[zero_row], before[0]) and np.array_equal(m[zero_row], before[1])):
                fails.append(f"({sigma2}, {eta2}): the row of zero statistics changed")
            for q, r in enumerate(rows):
                figs, bad = gsr.judge(dtype, cases[q].name, V[r], m[r], S[q], w[q], sigma2, eta2,
                                      ("finalize", dtype, K, cases[q].name, sigma2, eta2))
                worst = np.maximum(worst, figs)
                fails += [f"{cases[q].name} ({sigma2}, {eta2}): {b}" for b in bad]
    _report("finalize", "finalize", dtype, K, worst, fails)


@pytest.mark.parametrize("K", gsr.LOGDET_K)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_log_det_of_planted_covariances(dtype, K):
    """The eliminations behind the ELBO's LOGDET column (one wavefront per row up to K = 64, one block per row with the
    packed triangle in LDS beyond) on the battery's Sigma as covariance rows, against float64 slogdet of the rows the
    device holds:  |error| <= K C eps (kappa + K)."""
    import pmf_hip
    from pmf_hip import ARR_COV, ARR_FACTOR, ELBO_LOGDET, USER
    named = gsr.covariance_rows(K, dtype)
    R = len(named)
    worst, fails = 0.0, []
    with pmf_hip.Context(R, 1, K, dtype=dtype) as ctx:
        ctx.set_array(USER, ARR_COV, np.stack([s for _, s in named]))
        ctx.set_array(USER, ARR_FACTOR, np.zeros((R, K)))
        held = ctx.get_array(USER, ARR_COV)
        _, per_row = ctx.gauss_elbo_terms(USER, per_row=True)
    for r, (name, _) in enumerate(named):
        sign, want = np.linalg.slogdet(held[r])
        assert sign > 0, name
        lim = gsr.logdet_bound(dtype, gsr.scaled_cond(held[r]), K)
        err = abs(per_row[r, ELBO_LOGDET] - want)
        worst = max(worst, err / lim)
        if not (err <= lim):
            fails.append(f"{name}: log det {per_row[r, ELBO_LOGDET]!r}, slogdet {want!r}, bound {lim:.3e}")
    kernel = "gauss_elbo_row_reg_kernel" if K <= 64 else "gauss_elbo_row_lds_kernel"   # (packed triangle: in LDS at these K)
    print(f"LOGDET dtype={dtype} K={K} solver=[{kernel} {dtype}] worst_over_bound={worst:.4f}")
    assert not fails, fails
