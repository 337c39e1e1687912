"""Device time of the bias-free Gaussian calls with unlisted cells counted as weighted zeros (`pmf_ctx_set_gauss_zeros`,
PMF_ZEROS_OBSERVED) at the benchmark's Gaussian shape: the K = 64 fp32 context of 1M x 100k rows and 50M ratings
(state after two default CAVI iterations).  Timed, from the library's event brackets (`prof_get()`):

  - the Gram pass alone (`pmf_gauss_gram`) on the user side (8.3 GB of packed covariances) and on the item side
    (0.83 GB), against bytes / the stream ceiling DESIGN.md section 5 records;
  - a whole iteration (user + item factor half-sweep) in each mode, by its kernels and by wall clock.

The two modes alternate inside one loop on one context, after one warm-up round; medians, minima and maxima over the
rounds are reported.

    python tools/probe_gauss_implicit.py [--json PATH] [rounds]        (default 5 rounds)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_FACTOR, ITEM, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

argv = sys.argv[1:]
json_path = None
if argv[:1] == ["--json"]:
    json_path, argv = argv[1], argv[2:]
rounds = int(argv[0]) if argv else 5
K, U, I, N = 64, 1_000_000, 100_000, 50_000_000
SIGMA2, ETA2, W0 = 1.0, 1.0, 0.1
STREAM_TBS = 6.3            # the measured stream ceiling, TB/s
KERNELS = ("gauss_accum", "gauss_combine", "gauss_solve")
report = {"shape": {"K": K, "users": U, "items": I, "ratings": N, "dtype": "f32", "rounds": rounds, "zero_weight": W0}}


def stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def timed(ctx, call):
    """({kernel class: ms}, wall clock ms) of `call`: the event brackets, and a host clock around the call and the
    synchronise that reading the brackets implies"""
    ctx.prof_reset()
    t0 = time.perf_counter()
    call()
    p = ctx.prof_get()                       # (synchronises)
    return {k: p[k][0] for k in KERNELS}, 1e3 * (time.perf_counter() - t0)


def iteration(ctx):
    ctx.gauss_factor_sweep(USER, SIGMA2, ETA2)
    ctx.gauss_factor_sweep(ITEM, SIGMA2, ETA2)


u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
r = r - r.mean()
ctx = pmf_hip.Context(U, I, K)
ctx.set_ratings(u, i, r)
rng = np.random.default_rng(1)
ctx.set_array(USER, ARR_FACTOR, 0.1 * rng.standard_normal((U, K)))
ctx.set_array(ITEM, ARR_FACTOR, 0.1 * rng.standard_normal((I, K)))
ctx.set_cov_identity(USER, 1.0)
ctx.set_cov_identity(ITEM, 1.0)
for _ in range(2):
    iteration(ctx)
ctx.sync()
ctx.prof_enable(True)

names = ["gram_user", "gram_item"]
for mode in ("missing", "zero"):
    names += [f"iteration_kernels_{mode}", f"iteration_wall_{mode}"] + [f"iteration_{k}_{mode}" for k in KERNELS]
samples = {k: [] for k in names}
for k in range(rounds + 1):                  # round 0 warms up
    row = {}
    ctx.set_gauss_zeros(False)
    row["gram_user"] = timed(ctx, lambda: ctx.gauss_gram(USER))[0]["gauss_combine"]
    row["gram_item"] = timed(ctx, lambda: ctx.gauss_gram(ITEM))[0]["gauss_combine"]
    for mode in ("missing", "zero"):
        ctx.set_gauss_zeros(mode == "zero", W0)
        by_kernel, wall = timed(ctx, lambda: iteration(ctx))
        row[f"iteration_kernels_{mode}"], row[f"iteration_wall_{mode}"] = sum(by_kernel.values()), wall
        for name, ms in by_kernel.items():
            row[f"iteration_{name}_{mode}"] = ms
    if k == 0:
        held = ctx.device_bytes()
    else:
        for name, ms in row.items():
            samples[name].append(ms)
report["device_bytes_grew_after_the_first_round"] = ctx.device_bytes() - held
report["ms"] = {name: stats(v) for name, v in samples.items()}
ms = {name: s["median"] for name, s in report["ms"].items()}
cov_stride = ctx.cov_stride
byte_time = {"gram_user": U * (cov_stride + K) * 4 / (STREAM_TBS * 1e12) * 1e3, "gram_item": I * (cov_stride + K) * 4 / (STREAM_TBS * 1e12) * 1e3}
report["gram_byte_time_ms"] = byte_time
report["ratios"] = {
    "gram_user_over_byte_time": ms["gram_user"] / byte_time["gram_user"],
    "gram_item_over_byte_time": ms["gram_item"] / byte_time["gram_item"],
    "zero_over_missing_iteration_kernels": ms["iteration_kernels_zero"] / ms["iteration_kernels_missing"],
    "zero_over_missing_iteration_wall": ms["iteration_wall_zero"] / ms["iteration_wall_missing"],
}
for name, s in report["ms"].items():
    print(f"{name:>34}: median {s['median']:9.4f} ms   (min {s['min']:.4f}, max {s['max']:.4f})")
for name, x in report["ratios"].items():
    print(f"{name:>44}: {x:.3f}")
print("byte time of the Gram passes (ms):", byte_time, "| device bytes grown after the first round:",
      report["device_bytes_grew_after_the_first_round"])
ctx.close()
if json_path:
    with open(json_path, "w") as f:
        json.dump(report, f, indent=1)
