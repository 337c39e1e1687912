"""Device time of `pmf_gamma_fold_in_exact` at the benchmark's shape (the protocol of DESIGN.md section 4.9): the K = 64
fp32 HPF context of 1M x 100k rows and 50M ratings after two exact CAVI iterations, 100 000 new users of 50 ratings each
whose item ids are drawn from the training ratings (so the gathers follow the items' popularity), n_iter = 10, one
warm-up call and then `calls` timed ones.  Kernel times come from the library's event brackets (`prof_get()`), the
whole call from the wall clock.

The yardstick is what the library offered for the same job before the exact fold-in existed: a second context of
100 000 x 100k rows that holds the batch as its ratings, the item SHAPE / RATE copied in, the cold start written into the
users' SHAPE / RATE / PRIOR_RATE, ten `gamma_exact_sweep(USER)` calls -- its summed kernel time (every sweep rebuilds both
sides' tables), and its whole time from `Context(...)` to the read-back of the five arrays.  `--part yardstick` runs only
that, through the package of `--tree PATH` (a checkout of another commit with its library built), and writes it to
`--json`; `--yardstick-json PATH` then takes the yardstick from such a file.  Without either the yardstick runs through
this tree's library.

Also reported: the reference fold-in's kernel time (`pmf_gamma_fold_in`) on the same batch against the same context, and
the ratio of the two.

    python tools/probe_gamma_fold_in_exact.py [--part all|yardstick] [--tree PATH] [--yardstick-json PATH] [--json PATH]
                                              [n_users] [ratings_per_user] [n_iter] [calls]   (default 100000 50 10 5)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
opts = {"--part": "all", "--tree": ROOT, "--yardstick-json": None, "--json": None}
while argv and argv[0] in opts:
    opts[argv[0]], argv = argv[1], argv[2:]
TREE = os.path.abspath(opts["--tree"])
sys.path[:0] = [TREE, os.path.join(TREE, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER  # noqa: E402
from pmf_hip.synth import BASE_SEED, synth_ratings  # noqa: E402

K, U, I, N = 64, 1_000_000, 100_000, 50_000_000
n_new = int(argv[0]) if len(argv) > 0 else 100_000
per_user = int(argv[1]) if len(argv) > 1 else 50
n_iter = int(argv[2]) if len(argv) > 2 else 10
calls = int(argv[3]) if len(argv) > 3 else 5
A, A_PRIME, B_PRIME = 0.3, 5.0, 5.0
PRIOR = (A, 0.0, True, A_PRIME + K * A, B_PRIME)
STATE = (ARR_FACTOR, ARR_SHAPE, ARR_RATE, ARR_PRIOR_RATE, ARR_HYPER_RATE)
NAMES = ("factor", "shape", "rate", "prior_rate", "hyper_rate")
report = {"shape": {"K": K, "users": U, "items": I, "ratings": N, "dtype": "f32", "new_users": n_new, "ratings_per_user": per_user,
                    "n_iter": n_iter, "timed_calls": calls}, "library": "this tree" if TREE == ROOT else "the tree given with --tree"}


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
fold = None
with pmf_hip.Context(U, I, K) as ctx:
    ctx.set_ratings(u, i, r)
    for side, rows in ((USER, U), (ITEM, I)):
        ctx.set_array(side, ARR_SHAPE, A + rng.gamma(1.0, 0.1, size=(rows, K)))
        ctx.set_array(side, ARR_RATE, 1.0 + rng.gamma(1.0, 0.1, size=(rows, K)))
        ctx.set_array(side, ARR_PRIOR_RATE, np.ones(rows))
    for _ in range(2):
        ctx.gamma_exact_sweep(USER, *PRIOR); ctx.gamma_exact_sweep(ITEM, *PRIOR)
    item_shape, item_rate = ctx.get_array(ITEM, ARR_SHAPE), ctx.get_array(ITEM, ARR_RATE)
    if opts["--part"] == "all":
        ctx.prof_enable(True)
        for name, run in (("fold_in_exact", ctx.gamma_fold_in_exact), ("fold_in_reference", ctx.gamma_fold_in)):
            out = run(USER, row_ptr, ids, x, *PRIOR, n_iter=n_iter)     # warm-up
            rows = []
            for _ in range(calls):
                ctx.prof_reset()
                t0 = time.perf_counter()
                out = run(USER, row_ptr, ids, x, *PRIOR, n_iter=n_iter)
                wall = (time.perf_counter() - t0) * 1e3
                row_ms, final_ms, launches = kernel_ms(ctx)
                rows.append((row_ms + final_ms, wall))
            report[name] = {"kernel_ms": stats([a for a, _ in rows]), "whole_call_ms": stats([b for _, b in rows]), "launches": launches}
            print(f"{name}: {n_new} users x {per_user} ratings, n_iter = {n_iter}, launches per call {launches}: kernels "
                  f"{report[name]['kernel_ms']} ms = {report[name]['kernel_ms']['median'] * 1e6 / (nnz * n_iter):.3f} ns per rating and "
                  f"pass; whole call {report[name]['whole_call_ms']} ms", flush=True)
            if name == "fold_in_exact":
                fold = out
        report["exact_over_reference_kernel_time"] = (report["fold_in_exact"]["kernel_ms"]["median"] /
                                                      report["fold_in_reference"]["kernel_ms"]["median"])
        print(f"exact / reference fold-in kernel time: {report['exact_over_reference_kernel_time']:.2f}", flush=True)

# ---- the same job through the entry points that existed before: a second context and ten exact half-sweeps ----
rho0 = float(np.float32(PRIOR[3]) / np.float32(PRIOR[4]))
new_u = np.repeat(np.arange(n_new, dtype=np.int32), per_user)
rows = []
for k in range(calls + 1):                                           # run 0 warms up
    t0 = time.perf_counter()
    with pmf_hip.Context(n_new, I, K) as c2:
        c2.set_ratings(new_u, ids, x)
        c2.set_array(ITEM, ARR_SHAPE, item_shape)
        c2.set_array(ITEM, ARR_RATE, item_rate)
        c2.set_array(USER, ARR_SHAPE, np.full((n_new, K), A))
        c2.set_array(USER, ARR_RATE, np.full((n_new, K), rho0))
        c2.set_array(USER, ARR_PRIOR_RATE, np.full(n_new, rho0))
        c2.prof_enable(True)
        for _ in range(n_iter):
            c2.gamma_exact_sweep(USER, *PRIOR)
        yard = tuple(c2.get_array(USER, a) for a in STATE)
        wall = (time.perf_counter() - t0) * 1e3
        sweep_ms, final_ms, launches = kernel_ms(c2)
    if k:
        rows.append((sweep_ms + final_ms, wall))
here = {"kernel_ms": stats([a for a, _ in rows]), "whole_ms": stats([b for _, b in rows]), "launches": launches, "library": report["library"]}
print(f"second context + {n_iter} exact half-sweeps: kernels {here['kernel_ms']} ms, whole {here['whole_ms']} ms, launches {launches}", flush=True)
if opts["--part"] == "yardstick":
    report["yardstick"] = here
else:
    report["yardstick_this_library"] = here
    if opts["--yardstick-json"]:
        with open(opts["--yardstick-json"]) as f:
            report["yardstick"] = json.load(f)["yardstick"]
    else:
        report["yardstick"] = here
    yk = report["yardstick"]["kernel_ms"]
    spread = yk["max"] - yk["min"]
    excess = report["fold_in_exact"]["kernel_ms"]["median"] - yk["median"]
    report["requirement"] = {"fold_in_minus_yardstick_kernel_ms": excess, "yardstick_min_max_spread_ms": spread, "met": bool(excess <= spread)}
    print(f"fold-in kernel time - yardstick kernel time = {excess:.3f} ms; the yardstick's own min-max spread is {spread:.3f} ms", flush=True)
    diff = [float(np.max(np.abs(g - w) / np.abs(w))) for g, w in zip(fold, yard)]
    report["max_rel_difference_fold_in_vs_half_sweeps"] = dict(zip(NAMES, diff))
    print("largest relative difference between the two, per output:", " ".join("%.3g" % d for d in diff), flush=True)
if opts["--json"]:
    with open(opts["--json"], "w") as f:
        json.dump(report, f, indent=1)
