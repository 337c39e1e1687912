"""Per-side launch time of the Gaussian factor half-sweep (K = 64, bench data) by hot-row budget
PMF_GAUSS_HOT_MB: the most-rated rows of the gathered table that fit the budget are loaded with the
default cache policy, every other row non-temporally.  One fresh context per budget.

    python tools/probe_hot_rows.py [MB,MB,...]      (default 0,32,64,128,192,224,256)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

K, U, I, N = 64, 1_000_000, 100_000, 50_000_000
budgets = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [0, 32, 64, 128, 192, 224, 256]
u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
deg = {USER: np.bincount(u, minlength=U), ITEM: np.bincount(i, minlength=I)}
rng = np.random.default_rng(1)
fu, fi = 0.1 * rng.standard_normal((U, K)), 0.1 * rng.standard_normal((I, K))
for mb in budgets:
    os.environ["PMF_GAUSS_HOT_MB"] = str(mb)
    with pmf_hip.Context(U, I, K) as ctx:
        ctx.set_ratings(u, i, r - r.mean())
        ctx.set_array(USER, ARR_FACTOR, fu)
        ctx.set_array(ITEM, ARR_FACTOR, fi)
        ctx.set_cov_identity(USER); ctx.set_cov_identity(ITEM)
        ctx.set_array(USER, ARR_BIAS, np.zeros(U)); ctx.set_array(ITEM, ARR_BIAS, np.zeros(I))
        hot = {s: ctx.hot_rows(s) for s in (USER, ITEM)} if hasattr(ctx, "hot_rows") else {USER: [], ITEM: []}
        for _ in range(2):
            ctx.gauss_factor_sweep(USER, 0.5, 1.0); ctx.gauss_factor_sweep(ITEM, 0.5, 1.0)
        ctx.sync()
        for side, name, other in ((USER, "user sweep (gathers item rows)", ITEM), (ITEM, "item sweep (gathers user rows)", USER)):
            ts = []
            for _ in range(5):
                ctx.sync(); t0 = time.perf_counter()
                ctx.gauss_factor_sweep(side, 0.5, 1.0)
                ctx.sync(); ts.append((time.perf_counter() - t0) * 1e3)
                ctx.gauss_factor_sweep(1 - side, 0.5, 1.0)
            share = deg[other][np.asarray(hot[other], dtype=np.int64)].sum() / N
            print(f"PMF_GAUSS_HOT_MB={mb} {name}: {min(ts):.2f} ms (min of 5), median {sorted(ts)[2]:.2f} ms, "
                  f"max {max(ts):.2f} ms; {len(hot[other])} hot rows take {share:.3f} of the gathers", flush=True)
