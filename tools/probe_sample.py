"""Device time of the posterior draws, in one process on one context: K = 64 fp32, 1M x 100k rows, covariances after two
CAVI iterations from random factors (the draws read no ratings: `nnz` only shapes those covariances).  Times come from
the library's event brackets (`prof_get()`), two warm-ups and the median of `repeats` calls.

  (a) row pass: `gauss_sample_rows` over ALL user rows with n_draws = 1 and 8 (class gauss_solve, summed over the call's
      rounds; the download is made and discarded) against the ELBO row pass `gauss_elbo_terms(USER, with_data=False)`
      (class gauss_solve): the same elimination on the same bytes.
  (b) Thompson top-k: `topk_sampled` for `n_query` users, k = 10 (gauss_solve + topk) against `topk_query` in ids mode
      (topk) for the same users.

    python tools/probe_sample.py [repeats] [n_users] [n_items] [nnz] [n_query] [out.json]   (default 7 1000000 100000 10000000 262144)
"""
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the engine: pmf_hip.load() explains)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, PREDICT_BIAS, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

K = 64
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
U = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
I = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
N = int(sys.argv[4]) if len(sys.argv) > 4 else 10_000_000
Q = int(sys.argv[5]) if len(sys.argv) > 5 else 262_144
out_path = sys.argv[6] if len(sys.argv) > 6 else None
SIGMA2, ETA2, ETA_B2 = 0.5, 1.0, 1.0
WARMUPS = 2


def timed(ctx, call, classes):
    """per-class ms of `repeats` calls after the warm-ups: {class: [ms, ...]} and their per-call sums"""
    for _ in range(WARMUPS):
        call()
    ctx.sync()
    parts = {c: [] for c in classes}
    for _ in range(repeats):
        ctx.prof_reset()
        call()
        ctx.sync()
        p = ctx.prof_get()
        for c in classes:
            parts[c].append(p[c][0])
    return parts, [sum(parts[c][n] for c in classes) for n in range(repeats)]


med = lambda v: float(np.sort(v)[len(v) // 2])   # noqa: E731

u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
r = r - r.mean()
rng = np.random.default_rng(1)
with pmf_hip.Context(U, I, K) as ctx:
    ctx.set_ratings(u, i, r)
    ctx.set_array(USER, ARR_FACTOR, 0.1 * rng.standard_normal((U, K)))
    ctx.set_array(ITEM, ARR_FACTOR, 0.1 * rng.standard_normal((I, K)))
    ctx.set_cov_identity(USER); ctx.set_cov_identity(ITEM)
    ctx.set_array(USER, ARR_BIAS, np.zeros(U)); ctx.set_array(ITEM, ARR_BIAS, np.zeros(I))
    for _ in range(2):      # real covariances and biases on both sides
        ctx.gauss_factor_sweep(USER, SIGMA2, ETA2); ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA2)
        ctx.gauss_bias_sweep(USER, SIGMA2, ETA_B2); ctx.gauss_bias_sweep(ITEM, SIGMA2, ETA_B2)
    ctx.prof_enable(True)
    rows = np.arange(U, dtype=np.int32)
    result = {"shape": {"n_users": U, "n_items": I, "nnz": N, "K": K, "dtype": "f32", "n_query": Q}, "repeats": repeats}

    _, elbo = timed(ctx, lambda: ctx.gauss_elbo_terms(USER, with_data=False), ("gauss_solve",))
    result["elbo_rows_ms"] = elbo
    print(f"ELBO row pass over {U} rows: median {med(elbo):.3f} ms (min {min(elbo):.3f}, max {max(elbo):.3f}), "
          f"{med(elbo) * 1e6 / U:.1f} ns per row", flush=True)
    for nd in (1, 8):
        first = ctx.gauss_sample_rows(USER, rows[:4096], nd, seed=7)
        _, ms = timed(ctx, lambda: ctx.gauss_sample_rows(USER, rows, nd, seed=7), ("gauss_solve",))
        assert ctx.gauss_sample_rows(USER, rows[:4096], nd, seed=7).tobytes() == first.tobytes() and np.isfinite(first).all()
        result[f"sample_rows_{nd}_ms"] = ms
        result[f"sample_rows_{nd}_ratio"] = med(ms) / med(elbo)
        print(f"sample_rows, n_draws = {nd}: median {med(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), "
              f"{med(ms) * 1e6 / (U * nd):.1f} ns per row and draw; {med(ms) / med(elbo):.3f} x the ELBO row pass (expected < 1.5 at one draw)",
              flush=True)

    users = np.sort(np.random.default_rng(2).permutation(U)[:Q]).astype(np.int32)
    _, plain = timed(ctx, lambda: ctx.topk_query(ITEM, 10, ids=users, query_side=USER, score=PREDICT_BIAS), ("topk",))
    parts, sampled = timed(ctx, lambda: ctx.topk_sampled(ITEM, 10, users, query_side=USER, score=PREDICT_BIAS, seed=7, draw=1),
                           ("gauss_solve", "topk"))
    result.update(topk_query_ms=plain, topk_sampled_ms=sampled, topk_sampled_parts_ms=parts, topk_ratio=med(sampled) / med(plain))
    print(f"topk_query(ids) for {Q} users, k = 10: median {med(plain):.3f} ms (min {min(plain):.3f}, max {max(plain):.3f})")
    print(f"topk_sampled: median {med(sampled):.3f} ms (min {min(sampled):.3f}, max {max(sampled):.3f}), of which sampling "
          f"{med(parts['gauss_solve']):.3f} ms and scan {med(parts['topk']):.3f} ms; {med(sampled) / med(plain):.3f} x topk_query")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
