"""Device time of the Gaussian half-sweeps with per-rating confidence weights (`pmf_ctx_set_ratings_weighted`) against
the same sweeps without, at the benchmark's Gaussian shape: K = 64 fp32, 1M x 100k rows, 50M ratings.

One fresh context per variant, min of 5 (as tools/probe_hot_rows.py):
  - bias model, default mode: user and item factor sweep, user and item bias sweep;
  - bias-free model under PMF_ZEROS_OBSERVED (weight 0.1): one iteration (user + item factor sweep).
Each variant is timed without weights and with weights drawn from {0.25, 0.5, 1, 2, 4}.  The expectation from bytes for
the factor sweeps is (8588 + 4) / 8588: a rating gathers a packed covariance row and a mean row (8576 bytes at K = 64),
its id, its rating and a hot flag, and now 4 bytes of weight.

    python tools/probe_gauss_weights.py [--tree DIR] [--unweighted-only]

`--tree DIR` loads the package from another checkout of this repository (a build of another commit, which need not
know about weights: use `--unweighted-only`), so that the default path of two commits can be compared by one script.
"""
import os
import sys
import time

import numpy as np

argv = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in argv:
    ROOT = os.path.abspath(argv[argv.index("--tree") + 1])
unweighted_only = "--unweighted-only" in argv
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

K, U, I, N = 64, 1_000_000, 100_000, 50_000_000
SIGMA2, ETA2, ETA_BIAS2, W0 = 0.5, 1.0, 1.0, 0.1
u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
r = r - r.mean()
rng = np.random.default_rng(1)
fu, fi = 0.1 * rng.standard_normal((U, K)), 0.1 * rng.standard_normal((I, K))
weights = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], N)
print(f"package: {os.path.dirname(pmf_hip.__file__)}", flush=True)


def min_of_5(ctx, call, between=None):
    ts = []
    for _ in range(5):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
        if between:
            between()
    return min(ts), sorted(ts)[2], max(ts)


def report(name, t):
    print(f"{name}: {t[0]:.2f} ms (min of 5), median {t[1]:.2f} ms, max {t[2]:.2f} ms", flush=True)
    return t[0]


best = {}
for weighted in ([False] if unweighted_only else [False, True]):
    tag = "weighted" if weighted else "unweighted"
    w = (weights,) if weighted else ()
    with pmf_hip.Context(U, I, K) as ctx:       # the bias model, default mode
        ctx.set_ratings(u, i, r, *w)
        ctx.set_array(USER, ARR_FACTOR, fu)
        ctx.set_array(ITEM, ARR_FACTOR, fi)
        ctx.set_cov_identity(USER)
        ctx.set_cov_identity(ITEM)
        ctx.set_array(USER, ARR_BIAS, np.zeros(U))
        ctx.set_array(ITEM, ARR_BIAS, np.zeros(I))
        for _ in range(2):
            ctx.gauss_factor_sweep(USER, SIGMA2, ETA2)
            ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA2)
        ctx.sync()
        for side, name in ((USER, "user"), (ITEM, "item")):
            best[name, tag] = report(f"{tag} {name} factor sweep", min_of_5(
                ctx, lambda: ctx.gauss_factor_sweep(side, SIGMA2, ETA2), lambda: ctx.gauss_factor_sweep(1 - side, SIGMA2, ETA2)))
        # each bias sweep right after its side's factor sweep: both forms then take the mean sums the fused factor sweep
        # left (H_r = sum_j c_j m_j in the weighted form), and the weighted one streams 4 more bytes per rating
        for side, name in ((USER, "user"), (ITEM, "item")):
            ts = []
            for _ in range(5):
                ctx.gauss_factor_sweep(1 - side, SIGMA2, ETA2)
                ctx.gauss_factor_sweep(side, SIGMA2, ETA2)
                ctx.sync()
                t0 = time.perf_counter()
                ctx.gauss_bias_sweep(side, SIGMA2, ETA_BIAS2)
                ctx.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            best[name + " bias", tag] = report(f"{tag} {name} bias sweep", (min(ts), sorted(ts)[2], max(ts)))
    with pmf_hip.Context(U, I, K) as ctx:       # the bias-free model, unlisted cells as zeros of weight W0
        ctx.set_ratings(u, i, r, *w)
        ctx.set_array(USER, ARR_FACTOR, fu)
        ctx.set_array(ITEM, ARR_FACTOR, fi)
        ctx.set_cov_identity(USER)
        ctx.set_cov_identity(ITEM)
        ctx.set_gauss_zeros(True, W0)

        def iteration():
            ctx.gauss_factor_sweep(USER, SIGMA2, ETA2)
            ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA2)

        iteration()
        best["zero-mode iteration", tag] = report(f"{tag} zero-mode iteration", min_of_5(ctx, iteration))

if not unweighted_only:
    for name in ("user", "item", "user bias", "item bias", "zero-mode iteration"):
        a, b = best[name, "unweighted"], best[name, "weighted"]
        print(f"{name}: weighted / unweighted = {b / a:.4f}  ({a:.2f} -> {b:.2f} ms)", flush=True)
    print(f"expectation from bytes for the factor sweeps: {(8588 + 4) / 8588:.5f}")
