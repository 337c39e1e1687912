"""Device time of `pmf_gamma_predictive` at the benchmark's shape: the K = 64 fp32 HPF context of 1M x 100k rows, its
state after three CAVI iterations on the benchmark's 50M synthetic ratings, and 5M uniformly random (user, item) pairs
with ratings drawn like the training ones.

Timed, from the library's event brackets (`prof_get()`), for with_bound = 0 and 1, with and without per-pair outputs: the
pair pass (class `eval`) and, under with_bound, the table pass (class `gamma_final`); and the wall clock of the whole
call.  Yardstick, in the same rounds of the same process: `pmf_eval_run` (existing code) over the same 5M pairs stored as
the validation set.  Everything alternates inside one loop, after one warm-up round; medians, minima and maxima over the
rounds are reported, and every variant's pair pass and whole kernel time as a ratio to `pmf_eval_run`'s.

    python tools/probe_gamma_predictive.py [--json PATH] [rounds]        (default 5 rounds)
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
json_path = None
if argv[:1] == ["--json"]:
    json_path, argv = argv[1], argv[2:]
rounds = int(argv[0]) if argv else 5
K, U, I, N, PAIRS = 64, 1_000_000, 100_000, 50_000_000, 5_000_000
A, A_PRIME, B_PRIME = 0.3, 5.0, 5.0
KAPPA = A_PRIME + K * A
PRIOR = (A, 0.0, True, KAPPA, B_PRIME)
report = {"shape": {"K": K, "users": U, "items": I, "ratings": N, "pairs": PAIRS, "dtype": "f32", "rounds": rounds, "iterations": 3}}


def stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
r = r + 1.0
ctx = pmf_hip.Context(U, I, K)
ctx.set_ratings(u, i, r)
rng = np.random.default_rng(1)
ctx.set_array(USER, ARR_FACTOR, (A + rng.gamma(1.0, 0.1, size=(U, K))) / (B_PRIME + rng.gamma(1.0, 0.1, size=(U, K))))
ctx.set_array(ITEM, ARR_FACTOR, (A + rng.gamma(1.0, 0.1, size=(I, K))) / (B_PRIME + rng.gamma(1.0, 0.1, size=(I, K))))
ctx.set_array(USER, ARR_PRIOR_RATE, np.full(U, KAPPA / B_PRIME))
ctx.set_array(ITEM, ARR_PRIOR_RATE, np.full(I, KAPPA / B_PRIME))
for _ in range(3):
    ctx.gamma_sweep(USER, *PRIOR)
    ctx.gamma_sweep(ITEM, *PRIOR)
ctx.sync()
pu, pi = rng.integers(0, U, PAIRS).astype(np.int32), rng.integers(0, I, PAIRS).astype(np.int32)
px = r[rng.integers(0, N, PAIRS)]
del u, i
assert ctx.eval_set(pu, pi, px)
ctx.prof_enable(True)

variants = [(wb, pp) for wb in (False, True) for pp in (False, True)]
name_of = lambda wb, pp: ("bound" if wb else "no_bound") + ("_per_pair" if pp else "_totals_only")
samples = {"eval_run_kernel": [], "eval_run_wall": []}
for wb, pp in variants:
    for part in ("pair_pass", "table_pass", "wall"):
        samples[f"{name_of(wb, pp)}_{part}"] = []
before = ctx.device_bytes()
for k in range(rounds + 1):                  # round 0 warms up
    row = {}
    ctx.prof_reset()
    t0 = time.perf_counter()
    ctx.eval_run()
    row["eval_run_wall"] = (time.perf_counter() - t0) * 1e3
    row["eval_run_kernel"] = ctx.prof_get()["eval"][0]
    for wb, pp in variants:
        ctx.prof_reset()
        t0 = time.perf_counter()
        res = ctx.gamma_predictive(pu, pi, px, with_bound=wb, per_pair=pp)
        row[f"{name_of(wb, pp)}_wall"] = (time.perf_counter() - t0) * 1e3
        p = ctx.prof_get()                   # (synchronises)
        row[f"{name_of(wb, pp)}_pair_pass"], row[f"{name_of(wb, pp)}_table_pass"] = p["eval"][0], p["gamma_final"][0]
        assert np.isfinite(res.totals[[0, 1, 3]]).all() and np.isfinite(res.totals[2]) == wb
    if k == 0:
        held = ctx.device_bytes()
        report["bytes_held_after_the_first_calls"] = held - before
    else:
        for name, ms in row.items():
            samples[name].append(ms)
report["device_bytes_grew_after_the_first_round"] = ctx.device_bytes() - held
report["ms"] = {name: stats(v) for name, v in samples.items()}
ms = {name: s["median"] for name, s in report["ms"].items()}
report["ratios_to_eval_run_kernel"] = {}
for wb, pp in variants:
    n = name_of(wb, pp)
    report["ratios_to_eval_run_kernel"][n + "_pair_pass"] = ms[n + "_pair_pass"] / ms["eval_run_kernel"]
    report["ratios_to_eval_run_kernel"][n + "_kernels"] = (ms[n + "_pair_pass"] + ms[n + "_table_pass"]) / ms["eval_run_kernel"]
for name, s in report["ms"].items():
    print(f"{name:>36}: median {s['median']:9.3f} ms   (min {s['min']:.3f}, max {s['max']:.3f})")
for name, x in report["ratios_to_eval_run_kernel"].items():
    print(f"{name:>44}: {x:.3f}")
print("bytes held after the first calls:", report["bytes_held_after_the_first_calls"], "| grown after:",
      report["device_bytes_grew_after_the_first_round"])
ctx.close()
if json_path:
    with open(json_path, "w") as f:
        json.dump(report, f, indent=1)
