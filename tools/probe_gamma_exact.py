"""Device time of the exact coordinate-ascent half-sweeps (`pmf_gamma_exact_sweep`) at the benchmark's shape: the K = 64
fp32 HPF context of 1M x 100k rows and 50M ratings (state after two CAVI iterations of the reference's update).  Timed,
from the library's event brackets (`prof_get()`): the user and the item half-sweep, each split into its row pass (both
sides' (E log, E) tables, rebuilt by every call, plus the split rows' sums: gamma_final) and its data pass (gamma_sweep).

Yardsticks, in the same rounds: the two half-sweeps of `pmf_gamma_sweep`, the data pass of a user-side
`pmf_gamma_elbo_terms` call and `pmf_prof_gather_ceiling` of the user side.  With `--parent-library PATH` (a
libpmf_hip.so built from the parent commit's tree) they run through that library, on a context of its own holding the
same ratings and the same start state: code this change cannot have touched.  Without it they run through this build.
Everything alternates inside one loop, after one warm-up round; medians, minima and maxima over the rounds are reported.

Then, from one start state (the classes' draw), 20 iterations under each update and the bound after them.

    python tools/probe_gamma_exact.py [--json PATH] [--parent-library PATH] [rounds]        (default 7 rounds)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]
import pmf_hip  # noqa: E402
from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER  # noqa: E402
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
KAPPA = A_PRIME + K * A
PRIOR = (A, 0.0, True, KAPPA, B_PRIME)
ITERATIONS = 20
report = {"shape": {"K": K, "users": U, "items": I, "ratings": N, "dtype": "f32", "rounds": rounds},
          "table_policy": "both tables rebuilt by every call"}


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


def fitted(ctx, u, i, r):
    ctx.set_ratings(u, i, r)
    start_state(ctx)
    for _ in range(2):
        ctx.gamma_sweep(USER, *PRIOR)
        ctx.gamma_sweep(ITEM, *PRIOR)
    ctx.sync()
    ctx.prof_enable(True)


def passes_ms(ctx, call):
    """(row pass + split rows, data pass) of one call, from the event brackets"""
    ctx.prof_reset()
    call()
    p = ctx.prof_get()                       # (synchronises)
    return p["gamma_final"][0], p["gamma_sweep"][0]


def bound(ctx):
    from src.models._gamma_elbo import elbo_from_gamma_terms
    user = ctx.gamma_elbo_terms(USER, with_data=True, hierarchical=True)
    item = ctx.gamma_elbo_terms(ITEM, with_data=False, hierarchical=True)
    return elbo_from_gamma_terms(user, item, U, I, K, (A, A_PRIME, B_PRIME), (A, A_PRIME, B_PRIME), hierarchical=True)[0]


u, i, r = synth_ratings(U, I, N, seed=BASE_SEED)
r = r + 1.0
ctx = pmf_hip.Context(U, I, K)
fitted(ctx, u, i, r)
yard = ctx
if parent_path:
    yard = parent_context(parent_path)
    fitted(yard, u, i, r)
report["yardstick"] = "the parent commit's library" if parent_path else "this build (no --parent-library)"
before = ctx.device_bytes()
names = ("exact_user_row_pass", "exact_user_data_pass", "exact_item_row_pass", "exact_item_data_pass", "sweep_user", "sweep_item",
         "elbo_user_row_pass", "elbo_user_data_pass", "gather_ceiling_user", "gather_ceiling_item")
samples = {k: [] for k in names}
for k in range(rounds + 1):                  # round 0 warms up
    row = {}
    row["exact_user_row_pass"], row["exact_user_data_pass"] = passes_ms(ctx, lambda: ctx.gamma_exact_sweep(USER, *PRIOR))
    row["sweep_user"] = sum(passes_ms(yard, lambda: yard.gamma_sweep(USER, *PRIOR)))
    row["elbo_user_row_pass"], row["elbo_user_data_pass"] = passes_ms(
        yard, lambda: yard.gamma_elbo_terms(USER, with_data=True, hierarchical=True))
    row["exact_item_row_pass"], row["exact_item_data_pass"] = passes_ms(ctx, lambda: ctx.gamma_exact_sweep(ITEM, *PRIOR))
    row["sweep_item"] = sum(passes_ms(yard, lambda: yard.gamma_sweep(ITEM, *PRIOR)))
    row["gather_ceiling_user"] = yard.gather_ceiling_ms(USER, repeats=3)
    row["gather_ceiling_item"] = yard.gather_ceiling_ms(ITEM, repeats=3)
    if k == 0:
        report["bytes_held_after_the_first_calls"] = ctx.device_bytes() - before
        held = ctx.device_bytes()
    else:
        for name, ms in row.items():
            samples[name].append(ms)
report["device_bytes_grew_after_the_first_round"] = ctx.device_bytes() - held
report["ms"] = {name: stats(v) for name, v in samples.items()}
ms = {name: s["median"] for name, s in report["ms"].items()}
exact_user = ms["exact_user_row_pass"] + ms["exact_user_data_pass"]
exact_item = ms["exact_item_row_pass"] + ms["exact_item_data_pass"]
report["ratios"] = {
    "exact_user_over_user_half_sweep": exact_user / ms["sweep_user"],
    "exact_item_over_item_half_sweep": exact_item / ms["sweep_item"],
    "exact_iteration_over_iteration": (exact_user + exact_item) / (ms["sweep_user"] + ms["sweep_item"]),
    "exact_user_data_pass_over_user_half_sweep": ms["exact_user_data_pass"] / ms["sweep_user"],
    "exact_item_data_pass_over_item_half_sweep": ms["exact_item_data_pass"] / ms["sweep_item"],
    "exact_user_data_pass_over_elbo_user_data_pass": ms["exact_user_data_pass"] / ms["elbo_user_data_pass"],
    "exact_user_data_pass_over_gather_ceiling": ms["exact_user_data_pass"] / ms["gather_ceiling_user"],
    "exact_item_data_pass_over_gather_ceiling": ms["exact_item_data_pass"] / ms["gather_ceiling_item"],
    "exact_user_row_pass_over_exact_user": ms["exact_user_row_pass"] / exact_user,
    "exact_item_row_pass_over_exact_item": ms["exact_item_row_pass"] / exact_item,
}
for name, s in report["ms"].items():
    print(f"{name:>24}: median {s['median']:9.3f} ms   (min {s['min']:.3f}, max {s['max']:.3f})")
for name, x in report["ratios"].items():
    print(f"{name:>48}: {x:.3f}")
print("yardstick:", report["yardstick"], "| bytes held after the first calls:", report["bytes_held_after_the_first_calls"],
      "| grown after:", report["device_bytes_grew_after_the_first_round"])
if yard is not ctx:
    yard.close()

# the bound after ITERATIONS iterations under each update, from one start state
ctx.prof_enable(False)
report["elbo_after_iterations"] = {"iterations": ITERATIONS}
for update, sweep in (("reference", ctx.gamma_sweep), ("exact", ctx.gamma_exact_sweep)):
    start_state(ctx)
    first = bound(ctx)
    for _ in range(ITERATIONS):
        sweep(USER, *PRIOR)
        sweep(ITEM, *PRIOR)
    report["elbo_after_iterations"][update] = bound(ctx)
    report["elbo_after_iterations"]["start"] = first
    print(f"bound after {ITERATIONS} iterations, {update} update: {report['elbo_after_iterations'][update]:.6g}   (start {first:.6g})")
assert all(np.isfinite(v) for v in report["elbo_after_iterations"].values())
ctx.close()
if json_path:
    with open(json_path, "w") as f:
        json.dump(report, f, indent=1)
