"""The test-side half of the Gaussian row-solver contract (tests/gauss_solver_reference.py), without a GPU: the cases
are as conditioned as the bound assumes, and the NumPy restatement of the unpivoted Jacobi-scaled sweep stays within a
quarter of the constant C that tests/test_gauss_solver_gpu.py allows the device -- so C cannot go stale."""
import numpy as np
import pytest

import gauss_solver_reference as gsr

N_CHUNKS = 16    # the K of a dtype dealt out over this many test cases


def _sweep_rows(K, dtype):
    """(case, S, w) as the sweep route plants them: S and w = x m rounded to the dtype"""
    T = gsr.NP_DTYPE[dtype]
    for case in gsr.battery(K, dtype):
        yield case, gsr.rounded(case.S, dtype), (T(case.x) * case.m.astype(T)).astype(np.float64)


def _measure(dtype, K, rows, route):
    """worst (ratio V, ratio m, kappa, ulps) of the restatement over `rows` and the four pairs, after asserting what
    must hold of every case and of the restatement's own result"""
    worst = np.zeros(4)
    for sigma2, eta2 in gsr.PAIRS:
        kappas = []
        for name, S, w in rows:
            V, m, _, _ = gsr.sweep_restatement(S, w, sigma2, eta2, dtype)
            figs, fails = gsr.judge(dtype, name, V, m, S, w, sigma2, eta2, (route, dtype, K, name, sigma2, eta2))
            assert not fails, (K, name, sigma2, eta2, fails)
            assert max(figs[0], figs[1]) <= gsr.C / 4, (K, name, sigma2, eta2, figs)
            assert gsr.bound(dtype, figs[2], K) <= gsr.CAP[dtype], (K, name, sigma2, eta2, figs[2])
            kappas.append(figs[2])
            worst = np.maximum(worst, figs)
        assert min(kappas) <= 10.0, (K, sigma2, eta2, kappas)      # one tight case per K, dtype and pair
    return worst


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_restatement_stays_within_a_quarter_of_C(dtype, chunk):
    worst = np.zeros(4)
    for K in gsr.DEFAULT_K[dtype][chunk::N_CHUNKS]:
        worst = np.maximum(worst, _measure(dtype, K, [(c.name, S, w) for c, S, w in _sweep_rows(K, dtype)], "sweep"))
    print(f"restatement {dtype} chunk {chunk}: ratio V {worst[0]:.3f}  m {worst[1]:.3f}  max kappa {worst[2]:.4g}  "
          f"diag ulps {worst[3]:.2f}")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_restatement_on_the_finalize_route(dtype):
    """exact S, right-hand sides that have nothing to do with it"""
    worst = np.zeros(4)
    for K in gsr.FINALIZE_K[dtype]:
        cases = gsr.battery(K, dtype)
        rhs = gsr.rounded(gsr.finalize_rhs(K, len(cases)), dtype)
        rows = [(c.name, gsr.rounded(c.S, dtype), rhs[r]) for r, c in enumerate(cases)]
        worst = np.maximum(worst, _measure(dtype, K, rows, "finalize"))
    print(f"restatement {dtype} finalize: ratio V {worst[0]:.3f}  m {worst[1]:.3f}")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_restatement_log_det(dtype):
    """the pivots of the same elimination give log det of a covariance within K C eps (kappa + K), and a quarter of it
    here"""
    worst = 0.0
    for K in gsr.LOGDET_K:
        for name, sigma in gsr.covariance_rows(K, dtype):
            sigma = gsr.rounded(sigma, dtype)
            kappa = gsr.scaled_cond(sigma)
            assert gsr.bound(dtype, kappa, K) <= gsr.CAP[dtype], (K, name, kappa)
            sign, want = np.linalg.slogdet(sigma)
            assert sign > 0
            got = gsr.restatement_logdet_V(sigma, dtype)
            lim = gsr.logdet_bound(dtype, kappa, K)
            assert abs(got - want) <= lim / 4, (K, name, got, want, lim)
            worst = max(worst, abs(got - want) / lim)
    print(f"restatement {dtype} log det: worst |error| / bound {worst:.3f}")


def test_battery_is_what_it_says():
    for K in (1, 2, 3, 4, 5, 18, 19, 70, 113, 114, 128):
        for dtype in ("f32", "f64"):
            cases = {c.name: c for c in gsr.battery(K, dtype)}
            assert len(cases) == (14 if dtype == "f64" else 12)
            for c in cases.values():
                assert c.S.shape == (K, K) and np.array_equal(c.S, c.S.T), c.name
                assert np.linalg.eigvalsh(c.S).min() > 0, c.name
                assert c.exact == (not c.m.any())
            assert np.count_nonzero(cases["diag"].S) == K
            ranges = gsr.block_ranges(K)
            assert ranges[0][0] == 0 and ranges[-1][1] == K and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            assert not gsr.cross_block_zero(np.ones((K, K)), ranges) or len(ranges) == 1
            assert gsr.cross_block_zero(cases["blocks"].S, ranges)
            for lo, hi in ranges:
                assert (cases["blocks"].S[lo:hi, lo:hi] != 0).all()
            if K >= 5:
                w = min(4, K)
                lead, tail = cases["lead4"].S, cases["tail4"].S
                assert lead[0, w - 1] == 999.0 and lead[0, w] == 0 and tail[K - 1, K - w] == 999.0 and tail[K - 1, K - w - 1] == 0
                arrow = cases["arrow"].S
                assert arrow[0, K - 1] == 900.0 and np.count_nonzero(arrow) == K + 2


def test_reference_agrees_with_three_steps_all_in_long_double():
    """the reference's two refinement steps (correction product in float64) against three steps with every product in
    long double: the difference is a small fraction of what the float64 solver is allowed"""
    for K, name in ((64, "spec1e+08"), (100, "equicorr"), (33, "scaled"), (2, "tail4")):
        case = {c.name: c for c in gsr.battery(K, "f64")}[name]
        for sigma2, eta2 in gsr.PAIRS:
            V, m, kappa = gsr.reference(case.S, case.m, sigma2, eta2)
            P = gsr.precision_matrix(case.S, sigma2, eta2).astype(np.longdouble)
            W = np.linalg.inv(P.astype(np.float64)).astype(np.longdouble)
            for _ in range(3):
                W = W + np.dot(W, np.eye(K, dtype=np.longdouble) - np.dot(P, W))
            mW = (np.dot(W, case.m.astype(np.longdouble)) / np.longdouble(sigma2)).astype(np.float64)
            eV, em = gsr.errors(V, m, W.astype(np.float64), mW, case.m, sigma2)
            assert max(eV, em) <= 0.01 * gsr.EPS["f64"] * (kappa + K), (K, name, sigma2, eta2, eV, em)
