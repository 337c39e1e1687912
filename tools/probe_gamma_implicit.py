"""Device time of the Poisson MF / HPF calls with unlisted cells counted as zeros (`pmf_ctx_set_gamma_zeros`,
PMF_ZEROS_OBSERVED) at the benchmark's shape: the K = 64 fp32 HPF context of 1M x 100k rows and 50M ratings (state after
two CAVI iterations of the reference's update).  Timed, from the library's event brackets (`prof_get()`):

  - the column-sum launches alone (`pmf_gamma_column_sums`, from FACTOR) on the user table (256 MB) and on the item
    table (25.6 MB), against bytes / the stream ceiling DESIGN.md section 5 records;
  - a whole iteration (user + item half-sweep) in each mode, under the reference's and the exact update;
  - an `elbo()`'s two device calls in each mode, by their kernels and by wall clock.

The two modes alternate inside one loop on one context, after one warm-up round; medians, minima and maxima over the
rounds are reported.

    python tools/probe_gamma_implicit.py [--json PATH] [rounds]        (default 7 rounds)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

argv = sys.argv[1:]
json_path = None
if argv[:1] == ["--json"]:
    json_path, argv = argv[1], argv[2:]
rounds = int(argv[0]) if argv else 7
K, U, I, N = 64, 1_000_000, 100_000, 50_000_000
A, A_PRIME, B_PRIME = 0.3, 5.0, 5.0
KAPPA = A_PRIME + K * A
PRIOR = (A, 0.0, True, KAPPA, B_PRIME)
STREAM_TBS = 6.3            # the measured stream ceiling, TB/s
report = {"shape": {"K": K, "users": U, "items": I, "ratings": N, "dtype": "f32", "rounds": rounds}}


def stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def start_state(ctx):
    """The HPF class's initial draw: shapes a + noise, rates b' + noise, h = b'."""
    rng = np.random.default_rng(1)
    for side, rows in ((USER, U), (ITEM, I)):
        shape, rate = A + rng.gamma(1.0, 0.1, size=(rows, K)), B_PRIME + rng.gamma(1.0, 0.1, size=(rows, K))
        ctx.set_array(side, ARR_SHAPE, shape)
        ctx.set_array(side, ARR_RATE, rate)
        ctx.set_array(side, ARR_FACTOR, shape / rate)
        ctx.set_array(side, ARR_HYPER_RATE, np.full(rows, B_PRIME))
        ctx.set_array(side, ARR_PRIOR_RATE, np.full(rows, KAPPA / B_PRIME))


def kernels_ms(ctx, call):
    """(gamma_final, gamma_sweep, wall clock) of `call`, in ms: the event brackets, and a host clock around the call and
    the synchronise that reading the brackets implies"""
    ctx.prof_reset()
    t0 = time.perf_counter()
    call()
    p = ctx.prof_get()                       # (synchronises)
    return p["gamma_final"][0], p["gamma_sweep"][0], 1e3 * (time.perf_counter() - t0)


def iteration(ctx, sweep):
    sweep(USER, *PRIOR)
    sweep(ITEM, *PRIOR)


def elbo_calls(ctx):
    ctx.gamma_elbo_terms(USER, with_data=True, hierarchical=True)
    ctx.gamma_elbo_terms(ITEM, with_data=False, hierarchical=True)


u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
r = r + 1.0
ctx = pmf_hip.Context(U, I, K)
ctx.set_ratings(u, i, r)
start_state(ctx)
for _ in range(2):
    iteration(ctx, ctx.gamma_sweep)
ctx.sync()
ctx.prof_enable(True)

names = ["colsum_user", "colsum_item"]
for mode in ("missing", "zero"):
    names += [f"iteration_reference_{mode}", f"iteration_exact_{mode}", f"elbo_kernels_{mode}", f"elbo_wall_{mode}"]
samples = {k: [] for k in names}
for k in range(rounds + 1):                  # round 0 warms up
    row = {}
    ctx.set_gamma_zeros(False)
    row["colsum_user"] = kernels_ms(ctx, lambda: ctx.gamma_column_sums(USER))[0]
    row["colsum_item"] = kernels_ms(ctx, lambda: ctx.gamma_column_sums(ITEM))[0]
    for mode in ("missing", "zero"):
        ctx.set_gamma_zeros(mode == "zero")
        row[f"iteration_reference_{mode}"] = sum(kernels_ms(ctx, lambda: iteration(ctx, ctx.gamma_sweep))[:2])
        row[f"iteration_exact_{mode}"] = sum(kernels_ms(ctx, lambda: iteration(ctx, ctx.gamma_exact_sweep))[:2])
        final, sweep, wall = kernels_ms(ctx, lambda: elbo_calls(ctx))
        row[f"elbo_kernels_{mode}"], row[f"elbo_wall_{mode}"] = final + sweep, wall
    if k == 0:
        held = ctx.device_bytes()
    else:
        for name, ms in row.items():
            samples[name].append(ms)
report["device_bytes_grew_after_the_first_round"] = ctx.device_bytes() - held
report["ms"] = {name: stats(v) for name, v in samples.items()}
ms = {name: s["median"] for name, s in report["ms"].items()}
byte_time = {"colsum_user": U * K * 4 / (STREAM_TBS * 1e12) * 1e3, "colsum_item": I * K * 4 / (STREAM_TBS * 1e12) * 1e3}
report["colsum_byte_time_ms"] = byte_time
report["ratios"] = {
    "colsum_user_over_byte_time": ms["colsum_user"] / byte_time["colsum_user"],
    "colsum_item_over_byte_time": ms["colsum_item"] / byte_time["colsum_item"],
    "colsums_over_reference_iteration": (ms["colsum_user"] + ms["colsum_item"]) / ms["iteration_reference_missing"],
    "zero_over_missing_iteration_reference": ms["iteration_reference_zero"] / ms["iteration_reference_missing"],
    "zero_over_missing_iteration_exact": ms["iteration_exact_zero"] / ms["iteration_exact_missing"],
    "zero_over_missing_elbo_kernels": ms["elbo_kernels_zero"] / ms["elbo_kernels_missing"],
    "zero_over_missing_elbo_wall": ms["elbo_wall_zero"] / ms["elbo_wall_missing"],
}
for name, s in report["ms"].items():
    print(f"{name:>28}: median {s['median']:9.4f} ms   (min {s['min']:.4f}, max {s['max']:.4f})")
for name, x in report["ratios"].items():
    print(f"{name:>44}: {x:.3f}")
print("byte time of the column sums (ms):", byte_time, "| device bytes grown after the first round:",
      report["device_bytes_grew_after_the_first_round"])
ctx.close()
if json_path:
    with open(json_path, "w") as f:
        json.dump(report, f, indent=1)
