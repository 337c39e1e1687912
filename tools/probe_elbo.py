"""Device time of `pmf_gauss_elbo_terms(USER, with_data=1)` against a plain `pmf_gauss_factor_accumulate(USER)` into a
caller buffer, in one process on one context: the benchmark's K = 64 fp32 bias context of 1M x 100k rows and 50M
ratings, state after two CAVI iterations from random factors.  Times come from the library's event brackets
(`prof_get()`), summed over every kernel class a call touches (the ELBO call: its c_r and row kernels under
gauss_solve, the accumulate and the split-row combine under their own classes).  The two calls alternate; the ratio of
the medians is the figure DESIGN.md section 4.8 quotes.  PMF_ELBO_ROWS in the environment sets the rows of a window.

    python tools/probe_elbo.py [repeats] [n_users] [n_items] [nnz] [out.json]      (default 7 1000000 100000 50000000)
"""
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the engine: pmf_hip.load() explains)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_BIAS, ARR_FACTOR, ITEM, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

K = 64
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
U = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
I = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
N = int(sys.argv[4]) if len(sys.argv) > 4 else 50_000_000
out_path = sys.argv[5] if len(sys.argv) > 5 else None
SIGMA2, ETA2, ETA_B2 = 0.5, 1.0, 1.0
ELBO_CLASSES = ("gauss_accum", "gauss_combine", "gauss_solve")

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
    width = ctx.cov_stride + ctx.kpad
    stats = torch.zeros(U * width, dtype=torch.float32, device="cuda:0")
    window_rows = min(int(os.environ.get("PMF_ELBO_ROWS", "0")) or U, (256 << 20) // (width * 4), U)
    print(f"task length of the user list: {ctx.task_max_len(USER, 'gauss')}; window of {window_rows} rows "
          f"({window_rows * width * 4 / 2 ** 20:.0f} MB), {-(-U // window_rows)} windows", flush=True)
    ctx.prof_enable(True)
    for _ in range(2):      # warm-up of both calls: code objects, the window task list, scratch
        ctx.gauss_factor_accumulate(USER, stats.data_ptr())
        first = ctx.gauss_elbo_terms(USER, with_data=True)
    ctx.sync()
    acc_ms, elbo_ms, parts, wall_ms = [], [], [], []
    for _ in range(repeats):
        ctx.prof_reset()
        ctx.gauss_factor_accumulate(USER, stats.data_ptr())
        ctx.sync()
        p = ctx.prof_get()
        acc_ms.append(p["gauss_accum"][0] + p["gauss_combine"][0])
        ctx.prof_reset()
        t0 = time.perf_counter()
        got = ctx.gauss_elbo_terms(USER, with_data=True)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        p = ctx.prof_get()
        parts.append({k: p[k][0] for k in ELBO_CLASSES})
        elbo_ms.append(sum(parts[-1].values()))
        assert got.tobytes() == first.tobytes()                  # two calls give the same bits
    # the ESS total against the accumulate's statistics of a few rows, in float64 on the host
    s = stats.view(U, width)[:4].double().cpu().numpy()
    print("totals (SQNORM, LOGDET, BIAS_SQ, ESS):", got, "  S[0, :3] of row 0:", s[0, :3], flush=True)
    med = lambda v: float(np.sort(v)[len(v) // 2])   # noqa: E731
    result = {"shape": {"n_users": U, "n_items": I, "nnz": N, "K": K, "dtype": "f32"}, "window_rows": window_rows,
              "repeats": repeats, "accumulate_ms": acc_ms, "elbo_ms": elbo_ms, "elbo_wall_ms": wall_ms,
              "elbo_parts_ms": parts, "accumulate_median_ms": med(acc_ms), "elbo_median_ms": med(elbo_ms),
              "ratio": med(elbo_ms) / med(acc_ms), "totals": got.tolist()}
    print(f"accumulate(USER): median {med(acc_ms):.3f} ms (min {min(acc_ms):.3f}, max {max(acc_ms):.3f})")
    print(f"elbo_terms(USER, data): median {med(elbo_ms):.3f} ms (min {min(elbo_ms):.3f}, max {max(elbo_ms):.3f}); "
          f"whole call with download and host sum {med(wall_ms):.3f} ms; classes of the median-like last call {parts[-1]}")
    print(f"ratio {result['ratio']:.3f}  (bar: 1.25)")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
