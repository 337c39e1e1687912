"""What `pmf_topk_items_excluding` costs beside `pmf_topk_items` at the top-k benchmark's shape: 262,144 query users x
100,000 items, K = 64, fp32, gamma factors as `bench.py --workload topk` draws them, and 13.1 M training ratings, 50 per user on average:
synthetic ones (power-law users: `pmf_hip.synth.synth_ratings`, as tools/probe_rank.py), and every user's 50
best-scoring items.  Every figure is the
hipEvent time of the `topk` kernel class (`prof_get`): 2 warm-up calls, then the mean of 3 timed calls.
    python tools/probe_topk_exclude.py [--parent-library PARENT.so] [--stamps-library DIAG.so] [--json FILE]
        every step, each a process of its own under `timeout`; stops at a failure
    python tools/probe_topk_exclude.py --step exclude --k 10     # one step in this process
Steps:
    plain    pmf_topk_items at k = 10, 24, 64 with the library PMF_HIP_LIBRARY names (default: this build).  With
             --parent-library the driver runs it with the parent's library and this build alternating, three runs each
             (the protocol of profiles/topk_shared_score_speed.json): the plain kernels are byte-equal, so the two
             libraries' figures must lie inside each other's spread
    exclude  plain k | excluding k | plain k again | excluding k again, all in one process (a process's first full-size
             figure runs high, so each is measured twice); `ratio` = excluding / plain of the same round.  --ratings
             synthetic (pairs unrelated to the scores) or top (a user's ratings are its 50 best-scoring items)
    events   candidate events (scores that passed their user's threshold and reached drain()) per user and scan, plain
             and excluding, from a -DPMF_TOPK_STAMPS build of pmf_topk.hip (--stamps-library; tools/probe_topk_stamps.py
             has the command lines that build one)
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd")]

LIMIT = {"plain": 240, "exclude": 420, "events": 420}    # seconds a step may take
Q, I, K, PER_USER = 262_144, 100_000, 64, 50


def measure(ctx, call, repeats=3):
    for _ in range(2):                                   # sizes the scratch (and builds the distinct-item lists); clocks settle
        call()
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(repeats):
        call()
    ms, _ = ctx.prof_get()["topk"]
    ctx.prof_enable(False)
    return ms / repeats


def context():
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ITEM, USER
    rng = np.random.default_rng(0)
    ctx = pmf_hip.Context(Q, I, K, dtype="f32")
    ctx.set_array(USER, ARR_FACTOR, rng.gamma(0.5, 1.0, (Q, K)))
    ctx.set_array(ITEM, ARR_FACTOR, rng.gamma(0.5, 1.0, (I, K)))
    return ctx


def set_ratings(ctx, ratings):
    """`synthetic`: pmf_hip.synth's pairs, unrelated to the scores, so hardly any excluded item ever passes a threshold.
    `top`: every user's training items ARE its PER_USER best-scoring items -- what a fitted count model does to them, and the
    most an exclusion list of that length can cost: each entry passes its user's threshold and is dropped in drain()."""
    if ratings == "top":
        users = np.arange(Q, dtype=np.int32)
        tu, ti = np.repeat(users, PER_USER), ctx.topk_items(users, PER_USER)[0].reshape(-1)
        tr = np.ones(len(tu))
    else:
        from pmf_hip.synth import synth_ratings
        tu, ti, tr = synth_ratings(Q, I, PER_USER * Q, seed=1)
    ctx.set_ratings(tu, ti, tr)
    per_user = np.bincount(tu, minlength=Q)
    return {"ratings_are": ratings, "ratings": int(len(tu)), "ratings_per_user_mean": round(float(per_user.mean()), 1), "ratings_per_user_max": int(per_user.max())}


def emit(**row):
    print(json.dumps(row), flush=True)


def run_step(step, ks, label, ratings):
    users = np.arange(Q, dtype=np.int32)
    if label == "parent":                                # the parent's library predates the entry point: do not bind it
        import pmf_hip
        pmf_hip.SIGNATURES.pop("pmf_topk_items_excluding")
    with context() as ctx:
        if step == "plain":
            for k in ks:
                emit(step=step, library=label, k=k, kernel_ms=round(measure(ctx, lambda: ctx.topk_items(users, k)), 3))
            return
        data = set_ratings(ctx, ratings)
        if step == "exclude":
            for k in ks:
                for round_ in ("first", "again"):
                    plain = measure(ctx, lambda: ctx.topk_items(users, k))
                    excl = measure(ctx, lambda: ctx.topk_items(users, k, exclude_train=True))
                    emit(step=step, k=k, round=round_, plain_ms=round(plain, 3), excluding_ms=round(excl, 3),
                         ratio=round(excl / plain, 4), **data)
            return
        import pmf_hip
        lib = pmf_hip.load()                             # the stamped build: per (wavefront, user tile) counters of the last launch
        lib.pmf_debug_topk_stamps.argtypes = [C.c_void_p, C.c_int]
        n_waves = Q // 32
        for k in ks:
            row = {"step": step, "k": k}
            for what, exclude in (("plain", False), ("excluding", True)):
                ctx.topk_items(users, k, exclude_train=exclude)
                raw = np.zeros(n_waves * 8, dtype=np.int64)
                assert lib.pmf_debug_topk_stamps(raw.ctypes.data, n_waves) == 0
                raw = raw.reshape(-1, 8)
                row[f"candidate_events_per_user_{what}"] = round(float(raw[:, 6].mean()) / 32.0, 2)
                row[f"tiles_with_candidates_per_wave_{what}"] = round(float(raw[:, 7].mean()), 1)
                row[f"cycles_in_drain_per_wave_{what}"] = round(float(raw[:, 4].mean()))
            emit(**row, **data)


def spread(rows, library, k):
    ms = [r["kernel_ms"] for r in rows if r.get("step") == "plain" and r["library"] == library and r["k"] == k]
    return {"runs_ms": ms, "min": min(ms), "max": max(ms)} if ms else None


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(LIMIT))
    ap.add_argument("--k", type=int, nargs="+")
    ap.add_argument("--label", default="branch")
    ap.add_argument("--ratings", choices=["synthetic", "top"], default="synthetic")
    ap.add_argument("--parent-library")
    ap.add_argument("--stamps-library")
    ap.add_argument("--json", help="write the measurements of all steps to this file")
    args = ap.parse_args()
    if args.step:
        run_step(args.step, args.k or ([10, 24, 64] if args.step == "plain" else [10, 64]), args.label, args.ratings)
        sys.exit(0)
    plan = []
    for run in range(3 if args.parent_library else 1):
        if args.parent_library:
            plan.append(("plain", [], "parent", args.parent_library))
        plan.append(("plain", [], "branch", None))
    for ratings in ("synthetic", "top"):
        plan += [("exclude", ["--k", "10", "--ratings", ratings], "branch", None),
                 ("exclude", ["--k", "64", "--ratings", ratings], "branch", None)]
        if args.stamps_library:
            plan.append(("events", ["--ratings", ratings], "stamps", args.stamps_library))
    rows = []
    for step, extra, label, library in plan:             # a step that fails or runs out of time ends the probe
        env = dict(os.environ)
        env.pop("PMF_HIP_LIBRARY", None)
        if library:
            env["PMF_HIP_LIBRARY"] = os.path.abspath(library)
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                            "--label", label] + extra, stdout=subprocess.PIPE, text=True, env=env)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            sys.exit(f"step {step} ({label}) ended with status {r.returncode}: nothing further is started")
        rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    if args.json:
        plain = {f"k={k}": {lib: spread(rows, lib, k) for lib in ("parent", "branch")} for k in (10, 24, 64)}
        with open(args.json, "w") as f:
            json.dump({"what": f"kernel time (hipEvent, `topk` class) of pmf_topk_items_excluding beside pmf_topk_items: {Q} users x "
                               f"{I} items, K = {K}, fp32, gamma(0.5, 1) factors; exclusion on {PER_USER * Q} synthetic ratings "
                               "(pmf_hip.synth.synth_ratings); 3 timed calls after 2 warm-up calls per measurement; every step a "
                               "process of its own",
                       "command": "python tools/probe_topk_exclude.py --parent-library PARENT.so --stamps-library DIAG.so --json FILE",
                       "plain_parent_vs_branch": plain, "measurements": rows}, f, indent=1)
