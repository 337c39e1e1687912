"""Device time of `pmf_gamma_elbo_terms` at the benchmark's shape: the K = 64 fp32 HPF context of 1M x 100k rows and 50M
ratings (state after two CAVI iterations).  Timed: the whole `with_data` call of the user side (wall clock, the download
of the per-row terms and the host's sum included) and its two passes from the library's event brackets (`prof_get()`: the
row pass of both tables plus the split rows' sums as gamma_final, the data pass as gamma_sweep); the call of the item
side without data, which completes an `elbo()`.

Beside it, on the same context: the two half-sweeps of `pmf_gamma_sweep` of this build and `pmf_prof_gather_ceiling` of
the user side.  With `--parent-library PATH` (a libpmf_hip.so built from the parent commit's tree) the same two
half-sweeps run through that library too, on a context of its own holding the same ratings and the same start state:
the yardstick a change to csrc/pmf_gamma.hip cannot have touched.  All of them alternate inside one loop, after one
warm-up round; medians, minima and maxima over the rounds are reported.

    python tools/probe_gamma_elbo.py [--json PATH] [--parent-library PATH] [rounds]        (default 7 rounds)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_FACTOR, ARR_PRIOR_RATE, ITEM, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

argv = sys.argv[1:]
json_path = parent_path = None
while argv[:1] and argv[0] in ("--json", "--parent-library"):
    if argv[0] == "--json":
        json_path = argv[1]
    else:
        parent_path = argv[1]
    argv = argv[2:]
rounds = int(argv[0]) if argv else 7
K, U, I, N = 64, 1_000_000, 100_000, 50_000_000
A, A_PRIME, B_PRIME = 0.3, 5.0, 5.0
PRIOR = (A, 0.0, True, A_PRIME + K * A, B_PRIME)
report = {"shape": {"K": K, "users": U, "items": I, "ratings": N, "dtype": "f32", "rounds": rounds}}


def stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def parent_context(path):
    """A Context whose calls go to the library at `path` (an older build: only the symbols it has are bound)."""
    import ctypes as C
    lib = C.CDLL(path)
    for name, (res, args) in pmf_hip.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    lib.pmf_path = path
    return pmf_hip.Context(U, I, K, lib=lib)


def fitted(ctx, u, i, r):
    rng = np.random.default_rng(1)
    ctx.set_ratings(u, i, r)
    ctx.set_array(USER, ARR_FACTOR, A + rng.gamma(1.0, 0.1, size=(U, K)))
    ctx.set_array(ITEM, ARR_FACTOR, A + rng.gamma(1.0, 0.1, size=(I, K)))
    ctx.set_array(USER, ARR_PRIOR_RATE, np.ones(U))
    ctx.set_array(ITEM, ARR_PRIOR_RATE, np.ones(I))
    for _ in range(2):
        ctx.gamma_sweep(USER, *PRIOR)
        ctx.gamma_sweep(ITEM, *PRIOR)
    ctx.sync()
    ctx.prof_enable(True)


def half_sweep_ms(ctx, side):
    ctx.prof_reset()
    ctx.gamma_sweep(side, *PRIOR)
    p = ctx.prof_get()                       # (synchronises)
    return p["gamma_sweep"][0] + p["gamma_final"][0]


u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
r = r + 1.0
ctx = pmf_hip.Context(U, I, K)
fitted(ctx, u, i, r)
parent = parent_context(parent_path) if parent_path else None
if parent is not None:
    fitted(parent, u, i, r)
before = ctx.device_bytes()
samples = {k: [] for k in ("elbo_user_whole_call", "elbo_user_row_pass", "elbo_user_data_pass", "elbo_item_whole_call", "elbo_item_row_pass",
                           "sweep_user", "sweep_item", "parent_sweep_user", "parent_sweep_item", "gather_ceiling_user")}
value = None
for k in range(rounds + 1):                  # round 0 warms up
    row = {}
    ctx.prof_reset()
    t0 = time.perf_counter()
    user = ctx.gamma_elbo_terms(USER, with_data=True, hierarchical=True)
    row["elbo_user_whole_call"] = (time.perf_counter() - t0) * 1e3
    p = ctx.prof_get()
    row["elbo_user_row_pass"], row["elbo_user_data_pass"] = p["gamma_final"][0], p["gamma_sweep"][0]
    ctx.prof_reset()
    t0 = time.perf_counter()
    item = ctx.gamma_elbo_terms(ITEM, with_data=False, hierarchical=True)
    row["elbo_item_whole_call"] = (time.perf_counter() - t0) * 1e3
    row["elbo_item_row_pass"] = ctx.prof_get()["gamma_final"][0]
    if k == 0:
        value = (user, item)
        report["scratch_bytes_after_first_calls"] = ctx.device_bytes() - before
    row["sweep_user"], row["sweep_item"] = half_sweep_ms(ctx, USER), half_sweep_ms(ctx, ITEM)
    if parent is not None:
        row["parent_sweep_user"], row["parent_sweep_item"] = half_sweep_ms(parent, USER), half_sweep_ms(parent, ITEM)
    row["gather_ceiling_user"] = ctx.gather_ceiling_ms(USER, repeats=3)
    if k:
        for name, ms in row.items():
            samples[name].append(ms)
report["ms"] = {name: stats(v) for name, v in samples.items() if v}
ms = {name: s["median"] for name, s in report["ms"].items()}
yard = "parent_sweep" if parent is not None else "sweep"
report["yardstick"] = "half-sweeps of the parent commit's library" if parent is not None else "half-sweeps of this build (no --parent-library)"
kernels = ms["elbo_user_row_pass"] + ms["elbo_user_data_pass"]
iteration = ms[yard + "_user"] + ms[yard + "_item"]
report["ratios"] = {
    "elbo_user_kernels_over_user_half_sweep": kernels / ms[yard + "_user"],
    "elbo_user_data_pass_over_user_half_sweep": ms["elbo_user_data_pass"] / ms[yard + "_user"],
    "elbo_user_data_pass_over_gather_ceiling": ms["elbo_user_data_pass"] / ms["gather_ceiling_user"],
    "user_half_sweep_over_gather_ceiling": ms[yard + "_user"] / ms["gather_ceiling_user"],
    "elbo_user_whole_call_over_iteration": ms["elbo_user_whole_call"] / iteration,
    "elbo_both_calls_over_iteration": (ms["elbo_user_whole_call"] + ms["elbo_item_whole_call"]) / iteration,
    "elbo_both_calls_kernels_over_iteration": (kernels + ms["elbo_item_row_pass"]) / iteration,
}
for name, s in report["ms"].items():
    print(f"{name:>24}: median {s['median']:9.3f} ms   (min {s['min']:.3f}, max {s['max']:.3f})")
for name, x in report["ratios"].items():
    print(f"{name:>44}: {x:.3f}")
print("yardstick:", report["yardstick"], "| scratch held after the first calls:", report["scratch_bytes_after_first_calls"], "bytes")
from src.models._gamma_elbo import elbo_from_gamma_terms  # noqa: E402
L, parts = elbo_from_gamma_terms(value[0], value[1], U, I, K, (A, A_PRIME, B_PRIME), (A, A_PRIME, B_PRIME), hierarchical=True)
report["elbo_of_the_state"] = {"value": L, "parts": parts}
print("ELBO of the state:", L)
assert np.isfinite(L)
ctx.close()
if parent is not None:
    parent.close()
if json_path:
    with open(json_path, "w") as f:
        json.dump(report, f, indent=1)
