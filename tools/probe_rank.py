"""Kernel time of pmf_rank_items beside pmf_topk_items at the top-k benchmark's shape: 262,144 query users x 100,000
items, K = 64, fp32, gamma factors as `bench.py --workload topk` draws them.  Every figure is the hipEvent time of the
`topk` kernel class (`prof_get`), so the host legs of the calls are outside it.
    python tools/probe_rank.py [--json FILE]   # every step, each a process of its own under `timeout`; stops at a failure
    python tools/probe_rank.py --step scan     # one step in this process
--json writes every line and the top-k bar (profiles/rank_items.json is such a file).
Steps (each measures its own yardstick, so that every ratio compares launches of one process; a process's first full-size
measurement runs slower than its later ones, so every step measures its yardstick again at its end):
    scan     pmf_topk_items k = 10 | rank, one target per user | rank, RANK_SLOTS targets per user (full slots) | top-k again
    split    rank, one target per user | RANK_SLOTS targets per user with PMF_RANK_TARGETS=1 (one query row per target)
    exclude  rank, one target per user | the same with exclude_train on ~50 synthetic ratings per user
One JSON line per measurement; `ratio` is the time over the step's first rank measurement (over top-k for that one)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]

STEPS = {"scan": 240, "split": 240, "exclude": 420}     # seconds a step may take
Q, I, K, SLOTS, PEAK = 262_144, 100_000, 64, 4, 157.3


def measure(ctx, call, repeats=3):
    for _ in range(2):                                   # sizes the scratch (and builds the distinct-item lists); clocks settle
        call()
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(repeats):
        call()
    ms, _ = ctx.prof_get()["topk"]
    return ms / repeats


def report(step, what, ms, base_ms, scanned_rows):
    tf = 2.0 * scanned_rows * I * K / (ms * 1e-3) / 1e12
    print(json.dumps({"step": step, "what": what, "kernel_ms": round(ms, 3), "ratio": round(ms / base_ms, 3),
                      "query_rows": scanned_rows, "TFLOP/s": round(tf, 1), f"frac_of_{PEAK}": round(tf / PEAK, 3)}), flush=True)


def run_step(step):
    if step == "split":
        os.environ["PMF_RANK_TARGETS"] = "1"            # read when the context is created
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(0)
    users = np.arange(Q, dtype=np.int32)
    one = rng.integers(0, I, Q).astype(np.int32)
    ptr1 = np.arange(Q + 1, dtype=np.int64)
    with pmf_hip.Context(Q, I, K, dtype="f32") as ctx:
        ctx.set_array(USER, ARR_FACTOR, rng.gamma(0.5, 1.0, (Q, K)))
        ctx.set_array(ITEM, ARR_FACTOR, rng.gamma(0.5, 1.0, (I, K)))
        if step == "scan":
            topk = measure(ctx, lambda: ctx.topk_items(users, 10))
            report(step, "pmf_topk_items k = 10", topk, topk, Q)
        rank1 = measure(ctx, lambda: ctx.rank_rows(users, ptr1, one))
        report(step, "pmf_rank_items, 1 target per user", rank1, topk if step == "scan" else rank1, Q)
        if step in ("scan", "split"):
            many = rng.integers(0, I, Q * SLOTS).astype(np.int32)
            ptr = np.arange(Q + 1, dtype=np.int64) * SLOTS
            ms = measure(ctx, lambda: ctx.rank_rows(users, ptr, many))
            label = f"{SLOTS} targets per user, " + ("one query row each (full slots)" if step == "scan" else "one query row per target")
            report(step, "pmf_rank_items, " + label, ms, rank1, Q if step == "scan" else Q * SLOTS)
        if step == "exclude":
            from pmf_hip.synth import synth_ratings
            tu, ti, tr = synth_ratings(Q, I, 50 * Q, seed=1)
            ctx.set_ratings(tu, ti, tr)
            ms = measure(ctx, lambda: ctx.rank_rows(users, ptr1, one, exclude_train=True))
            report(step, "pmf_rank_items, 1 target per user, exclude_train (~50 ratings per user)", ms, rank1, Q)
        # the yardsticks once more: how far two measurements of one thing lie apart in one process
        again = measure(ctx, lambda: ctx.rank_rows(users, ptr1, one))
        report(step, "pmf_rank_items, 1 target per user, measured again", again, rank1, Q)
        if step == "scan":
            topk2 = measure(ctx, lambda: ctx.topk_items(users, 10))
            report(step, "pmf_topk_items k = 10, measured again", topk2, topk, Q)


def topk_bar(rows):
    """The one-target call over top-k, both from the scan step: first measurements, and the later pair (the process at speed)."""
    ms = {r["what"]: r["kernel_ms"] for r in rows if r["step"] == "scan"}
    first = ms["pmf_rank_items, 1 target per user"] / ms["pmf_topk_items k = 10"]
    later = ms["pmf_rank_items, 1 target per user, measured again"] / ms["pmf_topk_items k = 10, measured again"]
    return {"accepted_ratio": 1.1, "ratio_first_measurements": round(first, 3), "ratio_later_measurements": round(later, 3),
            "met": max(first, later) <= 1.1}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--json", help="write the measurements of all steps and the top-k bar to this file")
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
    else:
        rows = []
        for step, limit in STEPS.items():               # a step that fails or runs out of time ends the probe
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step],
                               stdout=subprocess.PIPE, text=True)
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                sys.exit(f"step {step} ended with status {r.returncode}: nothing further is started")
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
        if args.json:
            with open(args.json, "w") as f:
                json.dump({"what": f"kernel time (hipEvent, `topk` class) of pmf_rank_items beside pmf_topk_items: {Q} users x {I} items, "
                                   f"K = {K}, fp32, gamma(0.5, 1) factors; exclusion on {50 * Q} synthetic ratings (pmf_hip.synth.synth_ratings); "
                                   "3 timed calls after 2 warm-up calls per measurement; every step a process of its own",
                           "command": "python tools/probe_rank.py --json profiles/rank_items.json", "peak_TFLOPs": PEAK,
                           "topk_bar": topk_bar(rows), "measurements": rows}, f, indent=1)
