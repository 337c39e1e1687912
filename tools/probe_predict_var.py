"""Device time of the posterior predictive variance kernel (`pmf_predict_var`) at the benchmark's table sizes: a K = 64
fp32 context of 1M x 100k rows, identity covariances, random factors, 2M uniformly random pairs.  The kernel time comes
from the library's own event brackets (`prof_get()["predict_var"]`), so the staging copies of the ids and of the result
are not in it.  Prints pairs/s and the algorithmic GB/s, 2 (cov_stride + kpad) sizeof(T) bytes per pair.

    python tools/probe_predict_var.py [n_pairs] [launches]      (default 2000000 9)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_FACTOR, ITEM, USER  # noqa: E402

K, U, I = 64, 1_000_000, 100_000
n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 9
rng = np.random.default_rng(1)
with pmf_hip.Context(U, I, K) as ctx:
    ctx.set_array(USER, ARR_FACTOR, 0.1 * rng.standard_normal((U, K)))
    ctx.set_array(ITEM, ARR_FACTOR, 0.1 * rng.standard_normal((I, K)))
    ctx.set_cov_identity(USER)
    ctx.set_cov_identity(ITEM)
    u, i = rng.integers(0, U, n), rng.integers(0, I, n)
    bytes_per_pair = 2 * (ctx.cov_stride + ctx.kpad) * 4
    ctx.prof_enable(True)
    for _ in range(2):                       # warm-up: code object load, scratch growth
        got = ctx.predict_var(u, i)
    want = (ctx.get_array_rows(USER, ARR_FACTOR, u[:1000]) ** 2).sum(axis=1) \
        + (ctx.get_array_rows(ITEM, ARR_FACTOR, i[:1000]) ** 2).sum(axis=1) + K     # identity covariances
    assert np.allclose(got[:1000], want, rtol=1e-5), float(np.max(np.abs(got[:1000] - want)))
    ms = []
    for _ in range(launches):
        ctx.prof_reset()
        ctx.predict_var(u, i)
        t, count = ctx.prof_get()["predict_var"]
        assert count == 1
        ms.append(t)
    ms = np.sort(ms)
    for name, t in (("min", ms[0]), ("median", ms[len(ms) // 2]), ("max", ms[-1])):
        print(f"predict_var K={K} fp32 {U} x {I} rows, {n} pairs, {bytes_per_pair} B/pair: {name} {t:.3f} ms  "
              f"{n / t / 1e6:.3f} Gpairs/s  {n * bytes_per_pair / t / 1e9:.3f} TB/s")
    print("all launches (ms):", " ".join(f"{t:.3f}" for t in ms))
