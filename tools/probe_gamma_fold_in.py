"""Device time of `pmf_gamma_fold_in` at the benchmark's shape: the K = 64 fp32 HPF context of 1M x 100k rows and 50M
ratings (state after two CAVI iterations), 100 000 new users of 50 ratings each whose item ids are drawn from the
training ratings (so the gathers follow the items' popularity), n_iter = 10.  Kernel times come from the library's
event brackets (`prof_get()`), the whole call from the wall clock.

Beside it, what the library offered for the same job before the fold-in existed (existing entry points only): a second
context of 100 000 x 100k rows that holds the batch as its ratings, the item FACTOR copied in, the same start values,
ten `gamma_sweep(USER, hierarchical)` calls -- its summed kernel time, and its whole time from `Context(...)` and
`set_ratings` to the read-back of the five arrays.

Then the two measurements behind kGammaFoldLongRow: the batch above with one row of 128 .. 4096 ratings added, that row
walked by a lane group like the others or sent to the block kernel; and the threshold sweep, 256 rows each of
2^6 .. 2^16 ratings with the lane-group kernel forced (PMF_GAMMA_FOLD_LONG huge) and with the block kernel forced
(PMF_GAMMA_FOLD_LONG=1).

    python tools/probe_gamma_fold_in.py [--json PATH] [n_users] [ratings_per_user] [n_iter] [calls]   (default 100000 50 10 5)
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
K, U, I, N = 64, 1_000_000, 100_000, 50_000_000
n_new = int(argv[0]) if len(argv) > 0 else 100_000
per_user = int(argv[1]) if len(argv) > 1 else 50
n_iter = int(argv[2]) if len(argv) > 2 else 10
calls = int(argv[3]) if len(argv) > 3 else 5
A, A_PRIME, B_PRIME = 0.3, 5.0, 5.0
PRIOR = (A, 0.0, True, A_PRIME + K * A, B_PRIME)
STATE = (ARR_FACTOR, ARR_SHAPE, ARR_RATE, ARR_PRIOR_RATE, ARR_HYPER_RATE)
report = {"shape": {"K": K, "users": U, "items": I, "ratings": N, "dtype": "f32", "new_users": n_new, "ratings_per_user": per_user,
                    "n_iter": n_iter, "timed_calls": calls}}


def stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def kernel_ms(ctx):
    p = ctx.prof_get()
    return p["gamma_sweep"][0], p["gamma_final"][0], {k: p[k][1] for k in ("gamma_sweep", "gamma_final")}


u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
r = r + 1.0
rng = np.random.default_rng(1)
pick = rng.integers(0, N, n_new * per_user)
row_ptr = np.arange(n_new + 1, dtype=np.int64) * per_user
ids, x = i[pick].astype(np.int32), r[pick]
nnz = n_new * per_user
with pmf_hip.Context(U, I, K) as ctx:
    ctx.set_ratings(u, i, r)
    ctx.set_array(USER, ARR_FACTOR, A + rng.gamma(1.0, 0.1, size=(U, K)))
    ctx.set_array(ITEM, ARR_FACTOR, A + rng.gamma(1.0, 0.1, size=(I, K)))
    ctx.set_array(USER, ARR_PRIOR_RATE, np.ones(U)); ctx.set_array(ITEM, ARR_PRIOR_RATE, np.ones(I))
    for _ in range(2):
        ctx.gamma_sweep(USER, *PRIOR); ctx.gamma_sweep(ITEM, *PRIOR)
    E_beta = ctx.get_array(ITEM, ARR_FACTOR)
    ctx.prof_enable(True)
    fold = ctx.gamma_fold_in(USER, row_ptr, ids, x, *PRIOR, n_iter=n_iter)     # warm-up
    rows = []
    for _ in range(calls):
        ctx.prof_reset()
        t0 = time.perf_counter()
        fold = ctx.gamma_fold_in(USER, row_ptr, ids, x, *PRIOR, n_iter=n_iter)
        wall = (time.perf_counter() - t0) * 1e3
        row_ms, block_ms, launches = kernel_ms(ctx)
        rows.append((row_ms + block_ms, wall))
    report["fold_in"] = {"kernel_ms": stats([a for a, _ in rows]), "whole_call_ms": stats([b for _, b in rows]), "launches": launches}
    print(f"fold-in of {n_new} users x {per_user} ratings, n_iter = {n_iter}, launches per call {launches}", flush=True)
    print(f"fold-in kernel: {report['fold_in']['kernel_ms']} ms = {report['fold_in']['kernel_ms']['median'] * 1e6 / (nnz * n_iter):.3f} ns "
          f"per rating and update; whole call {report['fold_in']['whole_call_ms']} ms", flush=True)

# ---- the same job through the entry points that existed before: a second context and ten half-sweeps ----
rho0 = PRIOR[3] / PRIOR[4]
theta0 = np.full((n_new, K), A / rho0)
new_u = np.repeat(np.arange(n_new, dtype=np.int32), per_user)
rows = []
for k in range(calls + 1):                                           # run 0 warms up
    t0 = time.perf_counter()
    with pmf_hip.Context(n_new, I, K) as c2:
        c2.set_ratings(new_u, ids, x)
        c2.set_array(ITEM, ARR_FACTOR, E_beta)
        c2.set_array(USER, ARR_FACTOR, theta0)
        c2.set_array(USER, ARR_PRIOR_RATE, np.full(n_new, rho0))
        c2.prof_enable(True)
        for _ in range(n_iter):
            c2.gamma_sweep(USER, *PRIOR)
        yard = tuple(c2.get_array(USER, a) for a in STATE)
        wall = (time.perf_counter() - t0) * 1e3
        sweep_ms, final_ms, launches = kernel_ms(c2)
    if k:
        rows.append((sweep_ms + final_ms, wall))
report["yardstick"] = {"kernel_ms": stats([a for a, _ in rows]), "whole_ms": stats([b for _, b in rows]), "launches": launches}
print(f"second context + {n_iter} half-sweeps: kernels {report['yardstick']['kernel_ms']} ms, whole {report['yardstick']['whole_ms']} ms, "
      f"launches {launches}", flush=True)
spread = report["yardstick"]["kernel_ms"]["max"] - report["yardstick"]["kernel_ms"]["min"]
excess = report["fold_in"]["kernel_ms"]["median"] - report["yardstick"]["kernel_ms"]["median"]
report["requirement"] = {"fold_in_minus_yardstick_kernel_ms": excess, "yardstick_min_max_spread_ms": spread, "met": bool(excess <= spread)}
print(f"fold-in kernel time - yardstick kernel time = {excess:.3f} ms; the yardstick's own min-max spread is {spread:.3f} ms", flush=True)
diff = [float(np.max(np.abs(g - w) / np.abs(w))) for g, w in zip(fold, yard)]
report["max_rel_difference_fold_in_vs_half_sweeps"] = dict(zip(("factor", "shape", "rate", "prior_rate", "hyper_rate"), diff))
print("largest relative difference between the two, per output:", " ".join("%.3g" % d for d in diff), flush=True)
assert max(diff) < 5e-4            # tests/test_gamma_gpu.py:TOL for fp32 and up to 20 updates

# ---- a long row in a full batch: the batch above plus ONE row of L ratings (listed first), all rows with the lane-group
# kernel against the long row alone with the block kernel (PMF_GAMMA_FOLD_LONG = ratings_per_user) ----
tail = []
for length in (128, 256, 512, 1024, 2048, 4096):
    pk = rng.integers(0, N, length)
    rp = np.concatenate([[0], length + row_ptr]).astype(np.int64)
    ids_t, x_t = np.concatenate([i[pk].astype(np.int32), ids]), np.concatenate([r[pk], x])
    entry = {"long_row_ratings": length}
    for name, env in (("all_rows_lane_group_ms", str(1 << 40)), ("long_row_in_block_kernel_ms", str(per_user))):
        os.environ["PMF_GAMMA_FOLD_LONG"] = env
        with pmf_hip.Context(1, I, K) as c3:
            c3.set_array(ITEM, ARR_FACTOR, E_beta)
            c3.prof_enable(True)
            times = []
            for k in range(4):                                      # run 0 warms up
                c3.prof_reset()
                c3.gamma_fold_in(USER, rp, ids_t, x_t, *PRIOR, n_iter=n_iter, want_params=False)
                ms = kernel_ms(c3)
                if k:
                    times.append(ms[0] + ms[1])
        entry[name] = stats(times)
    tail.append(entry)
    print(f"batch + one row of {length} ratings: all lane groups {entry['all_rows_lane_group_ms']['median']:.3f} ms, long row in the "
          f"block kernel {entry['long_row_in_block_kernel_ms']['median']:.3f} ms", flush=True)
report["long_row_in_full_batch"] = tail

# ---- threshold sweep: one lane group per row against one block per row ----
sweep = []
for log2 in range(6, 17):
    length = 1 << log2
    rp = np.arange(257, dtype=np.int64) * length
    pk = rng.integers(0, N, 256 * length)
    entry = {"ratings_per_row": length}
    for name, env, key in (("row_kernel_ms", str(1 << 40), 0), ("block_kernel_ms", "1", 1)):
        os.environ["PMF_GAMMA_FOLD_LONG"] = env
        with pmf_hip.Context(1, I, K) as c3:
            c3.set_array(ITEM, ARR_FACTOR, E_beta)
            c3.prof_enable(True)
            times = []
            for k in range(4):                                      # run 0 warms up
                c3.prof_reset()
                c3.gamma_fold_in(USER, rp, i[pk].astype(np.int32), r[pk], *PRIOR, n_iter=n_iter, want_params=False)
                ms = kernel_ms(c3)
                assert ms[2] == {"gamma_sweep": 1 - key, "gamma_final": key}, ms
                if k:
                    times.append(ms[key])
        entry[name] = stats(times)
    sweep.append(entry)
    print(f"256 rows x {length} ratings: lane group per row {entry['row_kernel_ms']['median']:.3f} ms, block per row "
          f"{entry['block_kernel_ms']['median']:.3f} ms", flush=True)
os.environ.pop("PMF_GAMMA_FOLD_LONG", None)
report["threshold_sweep_256_rows"] = sweep
if json_path:
    with open(json_path, "w") as f:
        json.dump(report, f, indent=1)
