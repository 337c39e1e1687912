"""Device time of the logistic model's xi refresh (`pmf_gauss_logit_refresh`) against the weighted
Gaussian factor sweep of the same side, and of a logistic iteration against a weighted Gaussian one, at the benchmark's
Gaussian shape: K = 64 fp32, 1M x 100k rows, 50M ratings (`pmf_hip.synth`, thresholded at their median -> 0 / 1).

Kernel times from the library's event brackets (`prof_get`: the refresh under "predict_var", a sweep under "gauss_accum" +
"gauss_solve" + "gauss_combine"); two warm-ups, then the median of 7 with min - max.  Per rating a refresh gathers one packed
covariance row and one mean row of the other side (8576 bytes at K = 64), as the accumulate does.

    python tools/probe_logit.py [n_ratings]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_FACTOR, ITEM, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

K, U, I = 64, 1_000_000, 100_000
N = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
ETA2 = 1.0
u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
median = np.median(r)
x = max(((r > median), (r >= median)), key=lambda b: min(b.mean(), 1.0 - b.mean())).astype(np.float64)   # the less lopsided side of a tie at the median
print(f"{N} ratings, base rate {x.mean():.3f}", flush=True)
rng = np.random.default_rng(1)
fu, fi = 0.1 * rng.standard_normal((U, K)), 0.1 * rng.standard_normal((I, K))
SWEEP = ("gauss_accum", "gauss_solve", "gauss_combine")
BYTES = (K * (K + 1) // 2 + K) * 4


def timed(ctx, call, kernels, between=None, warm=2, runs=7):
    ts = []
    for k in range(warm + runs):
        ctx.sync()
        ctx.prof_reset()
        call()
        ctx.sync()
        prof = ctx.prof_get()
        if k >= warm:
            ts.append(sum(prof[name][0] for name in kernels))
        if between:
            between()
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def report(name, t, ratings=None):
    rate = f", {ratings * BYTES / t[0] / 1e6:.0f} GB/s of gathered rows at the median" if ratings else ""
    print(f"{name}: median {t[0]:.2f} ms ({t[1]:.2f} - {t[2]:.2f}){rate}", flush=True)
    return t[0]


c0 = 0.25
with pmf_hip.Context(U, I, K) as ctx:
    ctx.set_ratings(u, i, (x - 0.5) / c0, np.full(N, c0))
    ctx.set_array(USER, ARR_FACTOR, fu)
    ctx.set_array(ITEM, ARR_FACTOR, fi)
    ctx.set_cov_identity(USER)
    ctx.set_cov_identity(ITEM)
    ctx.prof_enable(True)

    def logistic_iteration():
        ctx.gauss_logit_refresh(USER, want_data_term=False)
        ctx.gauss_factor_sweep(USER, 1.0, ETA2)
        ctx.gauss_logit_refresh(ITEM, want_data_term=False)
        ctx.gauss_factor_sweep(ITEM, 1.0, ETA2)

    def gaussian_iteration():
        ctx.gauss_factor_sweep(USER, 1.0, ETA2)
        ctx.gauss_factor_sweep(ITEM, 1.0, ETA2)

    for _ in range(2):
        logistic_iteration()
    med = {}
    for side, name in ((USER, "user"), (ITEM, "item")):
        med[name, "refresh"] = report(f"{name} refresh", timed(ctx, lambda: ctx.gauss_logit_refresh(side, want_data_term=False),
                                                               ("predict_var",)), N)
        med[name, "refresh+D"] = report(f"{name} refresh with the data term", timed(ctx, lambda: ctx.gauss_logit_refresh(side),
                                                                                    ("predict_var",)), N)
        med[name, "sweep"] = report(f"{name} weighted factor sweep", timed(ctx, lambda: ctx.gauss_factor_sweep(side, 1.0, ETA2), SWEEP,
                                                                           between=lambda: ctx.gauss_logit_refresh(side, want_data_term=False)), N)
        print(f"{name}: refresh / sweep = {med[name, 'refresh'] / med[name, 'sweep']:.3f}", flush=True)
    a = report("logistic iteration", timed(ctx, logistic_iteration, SWEEP + ("predict_var",)))
    b = report("weighted Gaussian iteration", timed(ctx, gaussian_iteration, SWEEP))
    print(f"logistic / weighted Gaussian iteration = {a / b:.3f}", flush=True)
